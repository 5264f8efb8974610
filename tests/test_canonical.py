"""Canonical counting (tsx_hip_set_canonical): a k-mer and its reverse complement share one counter.

Expectations come from forward counts (python_counts, the golden .count file) folded by strand: the pair {x, rc(x)}
counts f(x) + f(rc x), a palindrome f(x); a dump reports the lexicographically smaller strand."""
import ctypes
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, python_counts

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s[::-1].translate(_COMP)


def fold(fwd):
    """{canonical k-mer (bytes): f(x) + f(rc x)} from forward counts of ACGT k-mers."""
    out = {}
    for x, c in fwd.items():
        y = rc(x)
        key = min(x, y)
        out[key] = out.get(key, 0) + c
    return out


def encode(kmers, k):
    """Vectorised tsx_hip_encode of ACGT byte strings: (n, key_limbs) uint64."""
    wk = (2 * k + 63) // 64
    a = np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(len(kmers), k).astype(np.uint64)
    codes = ((a >> np.uint64(1)) ^ (a >> np.uint64(2))) & np.uint64(3)
    out = np.zeros((len(kmers), wk), dtype=np.uint64)
    for i in range(k):
        out[:, (2 * i) // 64] |= codes[:, i] << np.uint64((2 * i) % 64)
    return out


def decode_all(T, limbs, k):
    return [T.decode(r, k).encode() for r in limbs]


def fastq_of(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def reads_of(text):
    lines = [l for l in text.split(b"\n") if l]
    return lines[1::4]


def check_table(T, m, text, k, lines=4):
    """dump == folded forward counts entry for entry, distinct == pairs, every k-mer asked through both strands."""
    want = fold(python_counts(text, k, lines))
    st = m.stats()
    assert st["distinct"] == len(want), (st, len(want))
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0
    km, cn = m.getAllKmers()
    got = dict(zip(decode_all(T, km, k), (int(c) for c in cn)))
    assert got == want
    keys = list(want)
    counts = np.array([want[x] for x in keys], dtype=np.uint64)
    assert np.array_equal(m.getKmerCounts(encode(keys, k)), counts)
    assert np.array_equal(m.getKmerCounts(encode([rc(x) for x in keys], k)), counts)


# ---- CPU --------------------------------------------------------------------------------------------------------------

def test_canonical_host_against_string_reverse_complement():
    import tsxcount_amd as T
    rnd = random.Random(5)
    for k in range(1, 128):
        seqs = [bytes(rnd.choice(b"ACGT") for _ in range(k)) for _ in range(24)]
        if k % 2 == 0:   # palindromes: a half and its reverse complement
            for _ in range(4):
                h = bytes(rnd.choice(b"ACGT") for _ in range(k // 2))
                seqs.append(h + rc(h))
        seqs += [b"A" * k, b"T" * k, b"C" * k, b"G" * k]
        got = T.canonical(encode(seqs, k), k).reshape(len(seqs), -1)
        assert decode_all(T, got, k) == [min(s, rc(s)) for s in seqs], k
        for s in seqs[:4]:
            assert T.canonical(s.decode(), k) == min(s, rc(s)).decode()


def test_canonical_host_refuses_bad_k():
    import tsxcount_amd as T
    L = T.lib()
    x = np.zeros(4, dtype=np.uint64)
    p = x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    for k in (0, -1, 128, 1000):
        assert L.tsx_hip_canonical_host(k, p, 1, p) == T.EINVAL
    assert L.tsx_hip_canonical_host(31, None, 0, None) == T.OK


def test_canonical_symbols_exported_and_declared():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in ("tsx_hip_set_canonical", "tsx_hip_canonical", "tsx_hip_canonical_host", "tsx_hip_group_set_canonical"):
        assert hasattr(L, name), name
        assert name + "(" in hdr, name


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    assert tsxcount_amd.lib().tsx_hip_device_count() > 0, "no GPU"
    return tsxcount_amd


def small_text(seed=3, n=12):
    from tsxcount_amd import synth
    return synth.fastq(seed, 0, n)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 14, 21, 31, 32, 33, 47, 63, 64, 96, 127])
def test_exact_against_folded_forward_counts(T, k):
    text = small_text(11, 10)
    if k < 8:   # 2k > l: a table of at most 2^(2k-1) slots, kept below half full
        text = fastq_of([r[:90] for r in reads_of(text)[:2]])
    for path in ("auto", "atomic", "partitioned"):
        m = T.TSXHashMapHIP(min(20, 2 * k - 1), 0, k, canonical=True)
        assert m.canonical
        m.set_path(path)
        m.countFastq(text)
        check_table(T, m, text, k)
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31, 63])
def test_strand_symmetry(T, k):
    reads = reads_of(small_text(21, 10))
    R, Rrc = fastq_of(reads), fastq_of([rc(s) for s in reversed(reads)])

    def table(text, canon):
        m = T.TSXHashMapHIP(20, 0, k, canonical=canon)
        m.countFastq(text)
        km, cn = m.getAllKmers()
        o = np.lexsort(km.T[::-1])
        return m, km[o], cn[o]

    _, a, ca = table(R, True)
    _, b, cb = table(Rrc, True)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    _, c, cc = table(R + Rrc, True)
    assert np.array_equal(a, c) and np.array_equal(cc, 2 * ca)
    _, f1, _ = table(R, False)
    _, f2, _ = table(Rrc, False)
    assert f1.shape != f2.shape or not np.array_equal(f1, f2)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["atomic", "partitioned"])
def test_palindromes_and_homopolymers(T, path):
    k = 16
    seqs = [b"ACGT" * 60, b"GTAC" * 40, b"A" * 300, b"T" * 250, b"C" * 200, b"G" * 120,
            b"ACGTTGCA" * 30 + b"A" * 200]
    text = fastq_of(seqs)
    m = T.TSXHashMapHIP(20, 0, k, canonical=True)
    m.set_path(path)
    m.countFastq(text)
    check_table(T, m, text, k)
    nA, nT = 300 - k + 1 + 201 - k + 1, 250 - k + 1   # (the A ending "TGCA" starts the last run)
    assert m.getKmerCount("A" * k) == nA + nT == m.getKmerCount("T" * k)
    assert m.getKmerCount("ACGT" * 4) == sum(1 for s in seqs for i in range(len(s) - k + 1) if s[i:i + k] == b"ACGT" * 4)
    # the walk's hot-key path at a size where every piece takes the partitioned route: long poly-A / poly-T reads
    big = fastq_of([b"A" * 5000, b"T" * 4000] * 40 + reads_of(small_text(4, 20)))
    m2 = T.TSXHashMapHIP(20, 0, 31, canonical=True)
    m2.set_path(path)
    m2.countFastq(big)
    check_table(T, m2, big, 31)


@pytest.mark.gpu
def test_golden_fixture_python_and_cli(T, golden_fastq, golden_counts, tmp_path):
    want = fold({x.encode(): c for x, c in golden_counts.items()})
    m = T.TSXHashMapHIP(22, 0, 14, canonical=True)
    m.countFastq(golden_fastq)
    km, cn = m.getAllKmers()
    assert dict(zip(decode_all(T, km, 14), (int(c) for c in cn))) == want
    fq = tmp_path / "small_t7.1000.fastq"
    fq.write_bytes(golden_fastq)
    with gzip.open(os.path.join(GOLDEN, "small_t7.1000.fastq.14.count.gz"), "rb") as f:
        (tmp_path / "small_t7.1000.fastq.14.count").write_bytes(f.read())
    exe = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
    p = subprocess.run([exe, "--input=%s" % fq, "--k=14", "--mode=HIP", "--canonical", "--check", "--checkabort"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out + p.stderr.decode()
    assert "total errors0" in out
    assert "Added a total of %d different kmers" % len(want) in out
    assert "Reference kmer count: %d" % len(want) in out


@pytest.mark.gpu
def test_seams_and_special_paths(T, monkeypatch):
    from tsxcount_amd import synth
    k = 31
    text = small_text(31, 40)
    # small host pieces, with and without the fused walk
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "70000")
    for fuse in ("2", "0"):
        monkeypatch.setenv("TSX_HIP_FUSE", fuse)
        m = T.TSXHashMapHIP(22, 0, k, canonical=True)
        m.set_path("partitioned")
        m.countFastq(text)
        check_table(T, m, text, k)
        m.close()
    monkeypatch.delenv("TSX_HIP_PIECE_BYTES")
    monkeypatch.delenv("TSX_HIP_FUSE")
    # counts that overflow 2-bit slots into the secondary array
    m = T.TSXHashMapHIP(20, 2, k, canonical=True)
    for _ in range(3):
        m.countFastq(text)
    want = fold(python_counts(text, k))
    keys = list(want)[:5000]
    assert np.array_equal(m.getKmerCounts(encode(keys, k)), 3 * np.array([want[x] for x in keys], dtype=np.uint64))
    assert m.stats()["overflow_used"] > 0
    m.close()
    # load 0.9
    pairs = len(want)
    l = int(np.ceil(np.log2(pairs / 0.9)))
    reads = reads_of(text)
    while pairs / (1 << l) < 0.88:
        reads = reads[:-1]
        pairs = len(fold(python_counts(fastq_of(reads), k)))
    t2 = fastq_of(reads)
    m = T.TSXHashMapHIP(l, 0, k, canonical=True)
    m.countFastq(t2)
    check_table(T, m, t2, k)
    m.close()
    # BGZF and FASTA
    m = T.TSXHashMapHIP(22, 0, k, canonical=True)
    m.countFastqBgzf(T.bgzf_compress(text, block=30000))
    check_table(T, m, text, k)
    m.close()
    fa = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads_of(text)))
    m = T.TSXHashMapHIP(22, 0, k, canonical=True)
    m.set_record_lines(2)
    m.countFastq(fa)
    check_table(T, m, fa, k, lines=2)
    m.close()
    # fuzzed record structure: empty lines, reads with N, short reads
    for seed in (1, 2, 3):
        rnd = random.Random(seed)
        seqs = [bytes(rnd.choice(b"ACGTN") for _ in range(rnd.randrange(0, 200))) for _ in range(60)]
        t = b"".join(b"@f%d\n%s\n%s+\n%s\n" % (i, s, b"\n" * rnd.randrange(2), b"#" * len(s)) for i, s in enumerate(seqs))
        fwd = python_counts(t, 21)
        m = T.TSXHashMapHIP(20, 0, 21, canonical=True)
        m.set_path(rnd.choice(["atomic", "partitioned"]))
        m.countFastq(t)
        # N has the 2-bit code ((b >> 1) ^ (b >> 2)) & 3 = A: the expectation is that of the coded sequence
        coded = {}
        for x, c in fwd.items():
            y = x.replace(b"N", b"A")
            coded[y] = coded.get(y, 0) + c
        want = fold(coded)
        km, cn = m.getAllKmers()
        assert dict(zip(decode_all(T, km, 21), (int(c) for c in cn))) == want, seed


@pytest.mark.gpu
def test_device_windows_and_slabs(T):
    """Device text in small windows, and a table built slab by slab (both read their limits in a process of their own)."""
    code = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import tsxcount_amd as T
from tsxcount_amd import synth
from test_canonical import check_table
text = synth.fastq(9, 0, 300 if sys.argv[1] == "slab" else 60)
buf = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
torch.cuda.synchronize()
m = T.TSXHashMapHIP(int(sys.argv[2]), 0, 31, canonical=True)
m.set_path("partitioned")
m.countFastqDevice(buf.data_ptr(), len(text)); m.sync()
check_table(T, m, text, 31)
print("CANON OK")
''' % (ROOT, os.path.join(ROOT, "tests"))
    for kind, l, env in (("window", 23, {"TSX_HIP_DEV_WINDOW": "8192"}),
                         ("slab", 25, {"TSX_HIP_SLAB_SEGBITS": "9", "TSX_HIP_DEV_WINDOW": str(1 << 17)})):
        p = subprocess.run([sys.executable, "-c", code, kind, str(l)], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0 and b"CANON OK" in p.stdout, p.stdout.decode()[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_merge_equals_one_gpu(T, ranks):
    text = small_text(41, 30)
    for k in (31, 63):
        one = T.TSXHashMapHIP(21, 0, k, canonical=True)
        one.countFastq(text)
        km, cn = one.getAllKmers()
        g = T.TSXHashMapHIPGroup(ranks, 21, 0, k, devices=[0] * ranks, comm="copy", canonical=True)
        g.countFastq(text)
        assert g.stats()["distinct"] == len(cn)
        assert np.array_equal(g.getKmerCounts(km), cn)
        rk = np.array([T.canonical(T.encode(T.revcomp(T.decode(r, k)), k), k) for r in km[:2000]]).reshape(-1, km.shape[1])
        assert np.array_equal(g.getKmerCounts(rk), cn[:2000])
        g.close()


@pytest.mark.gpu
def test_exchanges_refuse_canonical(T, tmp_path):
    from tsxcount_amd import distributed as TD
    m = T.TSXHashMapHIP(24, 0, 31, canonical=True)
    with pytest.raises(ValueError):
        TD.ShardedCounter(m, 1 << 20)
    with pytest.raises(ValueError):
        TD.MinimizerCounter(m, 1 << 20)
    assert T.lib().tsx_hip_mini_supported(m.handle) == 0 and T.lib().tsx_hip_shard_l1_supported(m.handle) == 0
    with pytest.raises(T.TSXException):
        T.TSXHashMapHIPGroup(2, 22, 0, 31, devices=[0, 0], comm="copy", exchange="mini", canonical=True)
    fq = tmp_path / "r.fastq"
    fq.write_bytes(small_text(2, 4))
    exe = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
    p = subprocess.run([exe, "--input=%s" % fq, "--k=31", "--l=20", "--gpus=2", "--devices=0,0", "--comm=copy",
                        "--exchange=mini", "--canonical"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0 and b"--exchange=mini" in p.stderr


@pytest.mark.gpu
def test_mode_rules(T):
    m = T.TSXHashMapHIP(20, 0, 21)
    assert not m.canonical
    m.countFastq(small_text(5, 2))
    with pytest.raises(T.TSXException) as e:
        m.set_canonical(True)
    assert e.value.code == T.EINVAL
    m.clear()
    m.set_canonical(True)
    m.countFastq(small_text(5, 2))
    m.clear()
    assert m.canonical
    text = small_text(6, 4)
    m.countFastq(text)
    check_table(T, m, text, 21)
    with pytest.raises(T.TSXException):
        m.set_canonical(False)
    with pytest.raises(T.TSXException):
        T.TSXHashMapHIP(20, 0, 21, shard_bits=1, canonical=True)
