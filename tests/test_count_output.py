"""Count output: the abundance histogram (tsx_hip_histogram_*) and the `.count` text (tsx_hip_format_counts_device,
tsx_hip_write_counts_host), through the C ABI, Python, the group and the tsxCount CLI.

Expectations come from independent counts only: python_counts, the golden `.count` file, and forward counts folded by
strand for canonical tables -- never from the library under test."""
import ctypes
import gzip
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, python_counts

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
GOLDEN_COUNT = os.path.join(GOLDEN, "small_t7.1000.fastq.14.count.gz")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s[::-1].translate(_COMP)


def fold(fwd):
    """{canonical k-mer: f(x) + f(rc x)}: the pair is keyed by its lexicographically smaller strand."""
    out = {}
    for x, c in fwd.items():
        key = min(x, rc(x))
        out[key] = out.get(key, 0) + c
    return out


def encode(kmers, k):
    """tsx_hip_encode of ACGT byte strings, vectorised: (n, key_limbs) uint64."""
    wk = (2 * k + 63) // 64
    a = np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(len(kmers), k).astype(np.uint64)
    codes = ((a >> np.uint64(1)) ^ (a >> np.uint64(2))) & np.uint64(3)
    out = np.zeros((len(kmers), wk), dtype=np.uint64)
    for i in range(k):
        out[:, (2 * i) // 64] |= codes[:, i] << np.uint64((2 * i) % 64)
    return out


def fastq_of(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def reads_of(text):
    return [l for l in text.split(b"\n") if l][1::4]


def repeated_text(seed, n_reads, max_rep):
    """Synthetic reads, each repeated 1..max_rep times: counts spread over many bins."""
    from tsxcount_amd import synth
    rnd = random.Random(seed)
    seqs = []
    for r in reads_of(synth.fastq(seed, 0, n_reads)):
        seqs += [r] * rnd.randint(1, max_rep)
    rnd.shuffle(seqs)
    return fastq_of(seqs)


def expected_hist(counts, nbins):
    h = np.zeros(nbins, dtype=np.uint64)
    for c, n in Counter(counts).items():
        h[min(c, nbins - 1)] += n
    return h


def parse_count_text(data):
    """{kmer: count} of a .count text; every line well formed, every k-mer once, no leading zeros."""
    assert data == b"" or data.endswith(b"\n")
    out = {}
    for ln in data.split(b"\n")[:-1]:
        kmer, c = ln.split(b"\t")
        assert c == str(int(c)).encode(), ln
        assert kmer not in out, kmer
        out[kmer] = int(c)
    return out


def read_lines(path):
    with open(path, "rb") as f:
        data = f.read()
    parse_count_text(data)
    return sorted(data.split(b"\n")[:-1])


def golden_lines():
    with gzip.open(GOLDEN_COUNT, "rb") as f:
        return sorted(l for l in f.read().split(b"\n") if l)


def run_cli(*args, timeout=300):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


# ---- CPU --------------------------------------------------------------------------------------------------------------

def test_output_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in ("tsx_hip_histogram_device", "tsx_hip_histogram_host", "tsx_hip_format_counts_device",
                 "tsx_hip_write_counts_host", "tsx_hip_group_histogram_host", "tsx_hip_group_write_counts_host"):
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    assert "main.cpp:224-396" in hdr and "TSXHashMap.h:660-722" in hdr
    assert T.EIO == -9 and L.tsx_hip_strerror(T.EIO).decode() == "writing the output failed"


def test_output_entry_points_refuse_bad_arguments_without_a_map():
    import tsxcount_amd as T
    L = T.lib()
    h = np.zeros(4, dtype=np.uint64)
    assert L.tsx_hip_histogram_host(None, T._p(h), 4) == T.EINVAL
    assert L.tsx_hip_histogram_device(None, 0, 0, 4, None, None) == T.EINVAL
    assert L.tsx_hip_write_counts_host(None, 1, 1, 0, 0, None, None) == T.EINVAL
    assert L.tsx_hip_group_histogram_host(None, T._p(h), 4) == T.EINVAL
    assert L.tsx_hip_group_write_counts_host(None, 1, 1, 2, 0, None, None) == T.EINVAL


def test_cli_usage_lists_the_output_options():
    code, out, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--output=FILE", "--lower=N", "--upper=N", "--histo=FILE", "--histo-max=H"):
        assert flag in err, flag
    code, _, err = run_cli("--input=x.fastq", "--lower=5", "--upper=4", timeout=30)
    assert code == 1 and "Usage" in err


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    assert tsxcount_amd.lib().tsx_hip_device_count() > 0, "no GPU"
    return tsxcount_amd


@pytest.mark.gpu
def test_cli_output_equals_golden_file(T, golden_fastq, golden_counts, tmp_path):
    fq = tmp_path / "small_t7.1000.fastq"
    fq.write_bytes(golden_fastq)
    out, histo = tmp_path / "o.count", tmp_path / "o.histo"
    code, so, se = run_cli("--input=%s" % fq, "--k=14", "--output=%s" % out, "--histo=%s" % histo, "--histo-max=5")
    assert code == 0, so + se
    assert read_lines(out) == golden_lines()
    assert len(golden_counts) == 194697
    h = expected_hist(golden_counts.values(), 7)
    want = b"".join(b"%d\t%d\n" % (c, h[c]) for c in range(1, 6) if h[c]) + b"6\t%d\n" % h[6]
    assert histo.read_bytes() == want
    # the console stays as it is without the new flags
    code2, so2, _ = run_cli("--input=%s" % fq, "--k=14")
    assert code2 == 0 and so2 == so


@pytest.mark.gpu
def test_cli_output_then_check_round_trip(T, tmp_path):
    from tsxcount_amd import synth
    fq = tmp_path / "x.fastq"
    fq.write_bytes(synth.fastq(17, 0, 40))
    code, so, se = run_cli("--input=%s" % fq, "--k=31", "--output=%s" % (tmp_path / "x.fastq.31.count"))
    assert code == 0, so + se
    code, so, se = run_cli("--input=%s" % fq, "--k=31", "--check", "--checkabort")
    assert code == 0, so + se
    assert "total errors0" in so
    distinct = int(so.split("Added a total of ")[1].split()[0])
    assert "Reference kmer count: %d\n" % distinct in so
    assert "tsxCount kmer count: %d\n" % distinct in so


@pytest.mark.gpu
@pytest.mark.parametrize("k", [14, 31, 33, 63, 127])
def test_histogram_equals_python_counts(T, k):
    text = repeated_text(100 + k, 6, 12)
    want = python_counts(text, k)
    for path in ("atomic", "partitioned"):
        for l, s, ov in ((20, 0, 0), (16, 2, 16)):
            m = T.TSXHashMapHIP(l, s, k, overflow_l=ov)
            m.set_path(path)
            m.countFastq(text)
            st = m.stats()
            assert st["insert_failures"] == 0 and st["overflow_failures"] == 0
            if s == 2:
                assert st["overflow_used"] > 0   # counts of 4 and more carried: pass B had work
            h = m.getCountHistogram(10002)
            assert np.array_equal(h, expected_hist(want.values(), 10002)), (k, path, l, s)
            assert int(h.sum()) == st["distinct"] == len(want)
            assert h[-1] == 0 and sum(c * int(n) for c, n in enumerate(h)) == st["count_sum"]
            assert np.array_equal(m.getCountHistogram(5), expected_hist(want.values(), 5))
            assert np.array_equal(m.getCountHistogram(2), expected_hist(want.values(), 2))
            m.close()


@pytest.mark.gpu
def test_planted_counts_digits_and_bounds(T, tmp_path):
    k = 31
    planted = [1, 9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 10 ** 19, 2 ** 64 - 1]
    rnd = random.Random(7)
    kmers = []
    while len(kmers) < len(planted):
        x = bytes(rnd.choice(b"ACGT") for _ in range(k))
        if x not in kmers:
            kmers.append(x)
    want = dict(zip(kmers, planted))
    # (add_kmers skips a zero count, so no slot of count 0 can be planted this way)
    for s in (0, 4):
        m = T.TSXHashMapHIP(20, s, k)
        m.addKmers(encode(kmers, k), np.array(planted, dtype=np.uint64))
        assert np.array_equal(m.getKmerCounts(encode(kmers, k)), np.array(planted, dtype=np.uint64))
        h = m.getCountHistogram(11)
        assert list(h) == [0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 8]
        h = m.getCountHistogram(101)
        assert h[1] == h[9] == h[10] == h[99] == 1 and h[100] == 6 and int(h.sum()) == len(planted)
        out = tmp_path / "p.count"
        assert m.writeCounts(str(out)) == (len(planted), sum(k + 2 + len(str(c)) for c in planted))
        assert parse_count_text(out.read_bytes()) == want
        for lo, hi in ((100, 100), (2 ** 32 - 1, 2 ** 32), (10, 99), (2 ** 40, None), (1, 1), (2, 8)):
            m.writeCounts(str(out), lower=lo, upper=hi)
            top = 2 ** 64 - 1 if hi is None else hi
            assert parse_count_text(out.read_bytes()) == {x: c for x, c in want.items() if lo <= c <= top}, (lo, hi)
        m.close()


@pytest.mark.gpu
def test_filters_chunk_seams_and_errors(T, tmp_path):
    k = 31
    text = repeated_text(5, 4, 9)
    want = {x: c for x, c in python_counts(text, k).items()}
    m = T.TSXHashMapHIP(14, 0, k)
    m.countFastq(text)
    one = tmp_path / "one.count"
    n, nb = m.writeCounts(str(one))
    assert parse_count_text(one.read_bytes()) == {x: c for x, c in want.items()}
    assert n == len(want) and nb == one.stat().st_size
    for lo, hi in ((1, 1), (2, 5), (3, 3), (6, None), (100, 200)):
        m.writeCounts(str(one), lower=lo, upper=hi)
        top = 2 ** 64 - 1 if hi is None else hi
        assert parse_count_text(one.read_bytes()) == {x: c for x, c in want.items() if lo <= c <= top}
    m.writeCounts(str(one))
    base = sorted(one.read_bytes().split(b"\n"))
    for chunk in (k + 22, 4096, 3 * 1024 + 7):
        seam = tmp_path / ("c%d.count" % chunk)
        assert m.writeCounts(str(seam), chunk_bytes=chunk) == (n, nb)
        assert sorted(seam.read_bytes().split(b"\n")) == base, chunk
    with pytest.raises(T.TSXException) as e:
        m.writeCounts(str(one), lower=5, upper=4)
    assert e.value.code == T.EINVAL
    with pytest.raises(T.TSXException) as e:
        m.writeCounts(str(one), chunk_bytes=k + 21)
    assert e.value.code == T.EINVAL
    with pytest.raises(T.TSXException) as e:
        m.getCountHistogram(1)
    assert e.value.code == T.EINVAL
    # a descriptor that cannot be written: TSX_HIP_EIO, not a silently short file
    fd = os.open(str(one), os.O_RDONLY)
    try:
        assert T.lib().tsx_hip_write_counts_host(m.handle, fd, 1, 2 ** 64 - 1, 0, None, None) == T.EIO
    finally:
        os.close(fd)
    # an empty table
    m.clear()
    assert not m.getCountHistogram(10).any()
    empty = tmp_path / "empty.count"
    assert m.writeCounts(str(empty)) == (0, 0) and empty.read_bytes() == b""
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_canonical_table_text_and_histogram(T, k, tmp_path):
    text = repeated_text(40 + k, 5, 7)
    want = fold(python_counts(text, k))
    m = T.TSXHashMapHIP(20, 0, k, canonical=True)
    m.countFastq(text)
    out = tmp_path / "c.count"
    assert m.writeCounts(str(out))[0] == len(want)
    assert parse_count_text(out.read_bytes()) == want
    assert np.array_equal(m.getCountHistogram(64), expected_hist(want.values(), 64))
    m.close()


@pytest.mark.gpu
def test_slot_ranges_match_dump_range(T):
    import torch
    k = 31
    text = repeated_text(9, 6, 10)
    m = T.TSXHashMapHIP(16, 2, k, overflow_l=16)
    m.countFastq(text)
    slots = m.getMaxElements()
    _, where = m.getKmerCountDebug(encode([b"A" * k], k))
    pa = int(where[0])
    assert pa < slots
    dev = torch.device("cuda", 0)
    kb = torch.zeros((slots, m.wk), dtype=torch.int64, device=dev)
    cb = torch.zeros(slots, dtype=torch.int64, device=dev)
    nb = torch.zeros(1, dtype=torch.int64, device=dev)
    tb = torch.zeros(slots * (k + 22), dtype=torch.uint8, device=dev)
    tn = torch.zeros(2, dtype=torch.int64, device=dev)
    vp = ctypes.c_void_p
    nbins = 32
    for lo, hi in ((0, slots), (0, 1), (pa, pa + 1), (max(0, pa - 700), min(slots, pa + 901)), (slots // 3, slots // 2),
                   (slots - 1, slots), (5, 5)):
        m.dumpRangeDevice(lo, hi, kb.data_ptr(), cb.data_ptr(), slots, nb.data_ptr())
        n = int(nb.cpu()[0])
        counts = cb[:n].cpu().numpy().view(np.uint64)
        assert np.array_equal(m.getCountHistogram(nbins, lo, hi), expected_hist([int(c) for c in counts], nbins)), (lo, hi)
        # the text of the same range, straight into a device buffer
        assert T.lib().tsx_hip_format_counts_device(m.handle, lo, hi, 1, 2 ** 64 - 1, vp(tb.data_ptr()), tb.numel(),
                                                    vp(tn.data_ptr()), vp(tn.data_ptr() + 8), None) == T.OK
        nbytes, nlines = (int(x) for x in tn.cpu())
        got = parse_count_text(tb[:nbytes].cpu().numpy().tobytes())
        kms = kb[:n].cpu().numpy().view(np.uint64)
        assert nlines == n and got == {T.decode(kms[i], k).encode(): int(counts[i]) for i in range(n)}
    # a buffer that is too small: TSX_HIP_ERANGE, and nothing is written past it
    tb.fill_(0)
    assert T.lib().tsx_hip_format_counts_device(m.handle, 0, slots, 1, 2 ** 64 - 1, vp(tb.data_ptr()), 1000,
                                                vp(tn.data_ptr()), vp(tn.data_ptr() + 8), None) == T.ERANGE
    assert int(tb[1000:].count_nonzero().cpu()) == 0
    assert T.lib().tsx_hip_format_counts_device(m.handle, 0, slots, 3, 2, vp(tb.data_ptr()), tb.numel(),
                                                vp(tn.data_ptr()), vp(tn.data_ptr() + 8), None) == T.EINVAL
    assert T.lib().tsx_hip_histogram_device(m.handle, 0, slots + 1, 4, vp(tb.data_ptr()), None) == T.EINVAL
    m.close()


@pytest.mark.gpu
def test_groups_equal_one_table(T, tmp_path, golden_fastq):
    from tsxcount_amd import synth
    k = 31
    text = synth.fastq(93, 0, 300) + repeated_text(3, 5, 8)
    one = T.TSXHashMapHIP(23, 0, k)
    one.countFastq(text)
    h1 = one.getCountHistogram(100)
    p1 = tmp_path / "one.count"
    one.writeCounts(str(p1))
    lines1 = read_lines(p1)
    one.close()
    for ranks, exchange in ((3, "merge"), (4, "mini")):
        g = T.TSXHashMapHIPGroup(ranks, 23, 0, k, devices=[0] * ranks, comm="copy", exchange=exchange)
        g.countFastq(text)
        assert np.array_equal(g.getCountHistogram(100), h1), exchange
        pg = tmp_path / ("g%d.count" % ranks)
        assert g.writeCounts(str(pg))[0] == len(lines1)
        assert read_lines(pg) == lines1, exchange
        g.close()
    fq = tmp_path / "small_t7.1000.fastq"
    fq.write_bytes(golden_fastq)
    out = tmp_path / "g.count"
    code, so, se = run_cli("--input=%s" % fq, "--k=14", "--gpus=3", "--devices=0,0,0", "--comm=copy", "--output=%s" % out)
    assert code == 0, so + se
    assert read_lines(out) == golden_lines()


@pytest.mark.gpu
def test_bench_shape_histogram(T):
    import torch
    seed, reads, k, l = 20261004, 1087000, 31, 30
    nbytes, _, polya = T.synth_sizes(seed, 0, reads, k, want_polya=True)
    dev = torch.device("cuda", 0)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    T.synth_fastq_device(seed, 0, reads, k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(l, 0, k)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    del text
    st = m.stats()
    h = m.getCountHistogram(1 << 20)
    assert int(h.sum()) == st["distinct"] == 804329712
    assert h[-1] == 1   # the poly-A k-mer, alone above 2^20 - 2
    assert st["count_sum"] - polya == sum(c * int(n) for c, n in enumerate(h[:-1]))
    m.close()
