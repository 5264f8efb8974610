"""Every device buffer, pinned buffer, event and stream of the host library has one owner (csrc/tsx_own.h): words 0-2
of tsx_hip_debug_counters count the live ones of the process.  The tests take differences of them around maps that are
created and destroyed, around a second pass over every host entry point that allocates, and around error returns that
come after allocations.  The error codes asserted in C are those of the code before the owners: EIO for a descriptor
that cannot be written, EFORMAT for a damaged database, ERANGE for a short output buffer, EINVAL for a damaged BGZF
member."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, python_counts

pytestmark = pytest.mark.gpu

K, L = 21, 19
READS = 300                      # ~0.5 MB of FASTQ
PIECE = 60000                    # TSX_HIP_PIECE_BYTES: several pieces, and the staging grows with the first text
WRITE_CHUNK = (K + 22) * 100000  # tsx_hip_write_counts_host: 100000 slots per chunk, 6 chunks at l = 19
DB_CHUNK = 1 << 20               # database chunks of ~129000 slots: 5 chunks at l = 19


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    return tsxcount_amd


@pytest.fixture(scope="module")
def text(T):
    from tsxcount_amd import synth
    return synth.fastq(5, 0, READS)


def encoded(counts, k):
    """(k-mers as the library's 2-bit words, their counts) of a dictionary count; one-limb k."""
    kmers = sorted(counts)
    b = np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(len(kmers), k).astype(np.uint64)
    code = ((b >> np.uint64(1)) ^ (b >> np.uint64(2))) & np.uint64(3)
    words = (code << (np.uint64(2) * np.arange(k, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    return words, np.array([counts[x] for x in kmers], dtype=np.uint64)


@pytest.fixture(scope="module")
def want(text):
    return encoded(python_counts(text, K), K)


@pytest.fixture(scope="module")
def probe(T):
    m = T.TSXHashMapHIP(16, 0, K)
    yield m
    m.close()


def counters(T, probe):
    L_ = T.lib()
    L_.tsx_hip_debug_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    out = (ctypes.c_uint64 * 8)()
    assert L_.tsx_hip_debug_counters(probe.handle, out) == 0
    return tuple(int(x) for x in out[:3])


def check_counts(T, m, want):
    kmers, counts = want
    assert np.array_equal(m.getKmerCounts(kmers), counts)
    assert m.stats()["distinct"] == len(kmers)


def wrapped_fasta(text):
    seqs = text.split(b"\n")[1::4]
    return b"".join(b">r%d\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)) for i, s in enumerate(seqs))


def test_create_destroy_returns_the_counters(T, probe):
    base = counters(T, probe)
    for k, l in ((21, 16), (63, 16)):
        m = T.TSXHashMapHIP(l, 0, k)
        during = counters(T, probe)
        assert during[0] > base[0] and during[2] > base[2], (base, during)
        m.close()
        assert counters(T, probe) == base


def one_pass(T, maps, text, fasta, gz, gz_fa, tmp):
    import torch
    from tsxcount_amd import synth
    m, mf, m2, m3 = maps
    for x in maps:
        x.clear()
    m.countFastq(text)                                   # several pieces (PIECE)
    mf.countFastqBgzf(gz)                                # several batches: the second text buffer and the inflate stream
    mf.clear()
    mf.countFastaBgzf(gz_fa)
    mf.clear()
    mf.countFasta(fasta)                                 # wrapped FASTA
    assert T.unwrap_fasta(fasta) == T.join_fasta(fasta)
    assert T.bgzf_inflate(gz) == text
    st = m.queryReads(text, chunk_bytes=100000)
    assert len(st) == READS
    kept, _ = m.filterReads(text, os.path.join(tmp, "kept.fq"), lower=1, chunk_bytes=100000)
    assert kept == READS
    lines, _ = m.writeCounts(os.path.join(tmp, "out.count"), chunk_bytes=WRITE_CHUNK)
    db = os.path.join(tmp, "t.kmerdb")
    entries, _ = m.saveDatabase(db, chunk_bytes=DB_CHUNK)
    assert lines == entries == m.stats()["distinct"]
    assert m2.addDatabase(db, chunk_bytes=DB_CHUNK) == entries      # placed as it is
    assert m3.addDatabase(db, chunk_bytes=DB_CHUNK) == entries      # another l: re-inserted
    assert m.compare(m2)["both"] == entries
    u = m.combine(m3, op="union", counts="sum", iL=L + 1)           # staged chunks of (k-mer, count)
    assert u.combine_stats["out_entries"] == entries
    u.close()
    hist = m.getCountHistogram(64)
    assert int(hist.sum()) == entries
    kmers, _ = m.getAllKmers()
    assert len(kmers) == entries
    assert len(m.getKmerCounts(kmers[:1000])) == 1000               # more than the map's small-lookup scratch
    nb, _, _ = T.synth_sizes(5, 0, 64, K)
    buf = torch.empty(nb + 256, dtype=torch.uint8, device="cuda:0")
    assert T.synth_fastq_device(5, 0, 64, K, buf.data_ptr(), nb + 256)[0] == nb
    thr = synth.zipf_thresholds(16)
    zb = T.synth_zipf_device(7, 64, 100, thr)
    zbuf = torch.empty(zb + 256, dtype=torch.uint8, device="cuda:0")
    assert T.synth_zipf_device(7, 64, 100, thr, zbuf.data_ptr(), zb + 256) == zb
    torch.cuda.synchronize()


def test_second_pass_leaves_the_counters(T, probe, text, want, monkeypatch, tmp_path):
    base = counters(T, probe)
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", str(PIECE))       # read when the map is created
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")               # clamped to the minimum: 128 KiB of text per batch
    maps = [T.TSXHashMapHIP(L, 0, K), T.TSXHashMapHIP(L, 0, K), T.TSXHashMapHIP(L, 0, K), T.TSXHashMapHIP(L + 1, 0, K)]
    fasta = wrapped_fasta(text)
    gz, gz_fa = T.bgzf_compress(text), T.bgzf_compress(fasta)
    one_pass(T, maps, text, fasta, gz, gz_fa, str(tmp_path))    # warm-up: grow-only scratch grows here
    check_counts(T, maps[0], want)                              # D: the results before ...
    warm = counters(T, probe)
    one_pass(T, maps, text, fasta, gz, gz_fa, str(tmp_path))
    assert counters(T, probe) == warm                           # temporaries gone, no scratch regrown
    check_counts(T, maps[0], want)                              # ... and after
    for m in maps:
        m.close()
    assert counters(T, probe) == base


SLAB_CODE = r"""
import ctypes, sys
sys.path.insert(0, %r)
import torch
torch.zeros(1, device="cuda:0")
import numpy as np
import tsxcount_amd as T
from tsxcount_amd import synth
from conftest import python_counts
from test_buffer_ownership import encoded
text = synth.fastq(5, 0, %d)
L_ = T.lib()
L_.tsx_hip_debug_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
def counters(m):
    out = (ctypes.c_uint64 * 8)()
    assert L_.tsx_hip_debug_counters(m.handle, out) == 0
    return tuple(int(x) for x in out[:3])
probe = T.TSXHashMapHIP(16, 0, 21)
base = counters(probe)
m = T.TSXHashMapHIP(25, 0, 21)
m.set_path(2)
m.countFastq(text)
warm = counters(probe)
m.clear()
m.countFastq(text)
assert counters(probe) == warm, (warm, counters(probe))
kmers, counts = encoded(python_counts(text, 21), 21)
assert np.array_equal(m.getKmerCounts(kmers), counts)
m.close()
assert counters(probe) == base, (base, counters(probe))
print("slab ok")
"""


def test_slab_route_leaves_the_counters():
    # (TSX_HIP_SLAB_SEGBITS is read once per process: a process of its own)
    code = SLAB_CODE % (os.path.join(ROOT, "tests"), READS)
    env = dict(os.environ, TSX_HIP_SLAB_SEGBITS="9", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and b"slab ok" in p.stdout, p.stdout.decode()[-2000:]


def test_error_returns_release_what_they_hold(T, probe, text, want, monkeypatch, tmp_path):
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")
    m = T.TSXHashMapHIP(L, 0, K)
    m.countFastq(text)
    m.queryReads(text)        # (what these leave with the map is there before the counters are read)
    ro = os.open(os.devnull, os.O_RDONLY)
    db = str(tmp_path / "t.kmerdb")
    m.saveDatabase(db, chunk_bytes=DB_CHUNK)
    raw = open(db, "rb").read()
    info = T.database_info(db)
    # the second chunk starts behind the header, the carry records and the first chunk (head, bitmap, entries)
    span = (DB_CHUNK - 32) // (8 + 64 * 8) * 64
    first = np.frombuffer(raw, dtype=np.uint64, count=4, offset=128 + info["carry_records"] * 24)
    assert int(first[1]) == span
    second = 128 + info["carry_records"] * 24 + 32 + (span // 64 + int(first[2])) * 8
    cut = str(tmp_path / "cut.kmerdb")
    open(cut, "wb").write(raw[:second + 32 + 100])
    flip = str(tmp_path / "flip.kmerdb")
    b = bytearray(raw)
    b[second + 32 + span // 8 + 40] ^= 0x10                     # an entry word of the second chunk
    open(flip, "wb").write(bytes(b))
    fasta = wrapped_fasta(text)
    gz = bytearray(T.bgzf_compress(text))
    nm, _ = T.bgzf_index(bytes(gz))
    assert nm >= 6
    gz[len(gz) * 3 // 4] ^= 0xFF                                # inside a member of a later batch
    assert T.bgzf_index(bytes(gz)) is not None
    other = T.TSXHashMapHIP(L, 0, K)
    lib = T.lib()

    def write_ro():
        return lib.tsx_hip_write_counts_host(m.handle, ro, 1, (1 << 64) - 1, WRITE_CHUNK, None, None)

    def load(path):
        def f():
            other.clear()
            fd = os.open(path, os.O_RDONLY)
            try:
                return lib.tsx_hip_load_host(other.handle, fd, DB_CHUNK, None)
            finally:
                os.close(fd)
        return f

    def unwrap_short():
        need = len(T.join_fasta(fasta))
        out = ctypes.create_string_buffer(need)
        got = ctypes.c_size_t(0)
        return lib.tsx_hip_unwrap_fasta_host(0, fasta, len(fasta), out, need - 1, ctypes.byref(got))

    def bgzf_damaged():
        other.clear()
        return lib.tsx_hip_count_fastq_bgzf_host(other.handle, bytes(gz), len(gz))

    def filter_ro():
        rule = T.filter_rule(1, None, 0, 1.0, False)
        return lib.tsx_hip_filter_reads_host(m.handle, text, len(text), ctypes.byref(rule), ro, 100000, None, None)

    def save_ro():                                               # fails at the header, before any staging
        return lib.tsx_hip_save_host(m.handle, ro, DB_CHUNK, None, None)

    def reader_gone(write, nbytes):
        """write(fd) into a pipe whose reader takes exactly nbytes and closes: the next write(2) fails with EPIPE (Python
        leaves SIGPIPE ignored; the ctypes call releases the GIL, so the reader runs)."""
        def f():
            r, w = os.pipe()

            def read():
                left = nbytes
                while left:
                    got = os.read(r, min(left, 1 << 20))
                    if not got:
                        break
                    left -= len(got)
                os.close(r)
            t = threading.Thread(target=read)
            t.start()
            try:
                return write(w)
            finally:
                os.close(w)
                t.join()
        return f

    # the first chunk is out and a later one queued on the device when the write fails
    save_gone = reader_gone(lambda w: lib.tsx_hip_save_host(m.handle, w, DB_CHUNK, None, None), second)
    write_gone = reader_gone(lambda w: lib.tsx_hip_write_counts_host(m.handle, w, 1, (1 << 64) - 1, WRITE_CHUNK, None, None),
                             WRITE_CHUNK // 2)

    monkeypatch.setenv("TSX_HIP_COMBINE_PATH", "1")              # the staged path, in chunks of 256 slots
    monkeypatch.setenv("TSX_HIP_COMBINE_CHUNK_BYTES", "4096")
    small = T.TSXHashMapHIP(8, 0, K, hash_seed=1)
    union = T.combine_rule("union", "max")

    def combine_small():
        small.clear()
        return lib.tsx_hip_combine(small.handle, m.handle, m.handle, ctypes.byref(union), None)

    cases = [("write_counts, read-only fd", write_ro, T.EIO), ("load, truncated", load(cut), T.EFORMAT),
             ("load, flipped byte", load(flip), T.EFORMAT), ("unwrap, short buffer", unwrap_short, T.ERANGE),
             ("bgzf, damaged member", bgzf_damaged, T.EINVAL), ("filter, read-only fd", filter_ro, T.EIO),
             ("save, read-only fd", save_ro, T.EIO), ("save, reader gone", save_gone, T.EIO),
             ("write_counts, reader gone", write_gone, T.EIO), ("combine, out too small", combine_small, T.EFULL)]
    for name, call, code in cases:
        call()                                                  # (scratch the call leaves with a map grows here)
        before = counters(T, probe)
        assert call() == code, name
        assert counters(T, probe) == before, name
    os.close(ro)
    small.close()
    for x in (m, other):                                        # still counting correctly
        x.clear()
        x.countFastq(text)
        check_counts(T, x, want)
        x.close()
