"""Read queries: per-record k-mer stats (tsx_hip_query_reads_*) and the read filter (tsx_hip_filter_reads_*), through
the C ABI, Python and the tsxCount CLI.

Expectations come from independent counts only -- python_counts-style dictionaries over the counted text (each byte
mapped through base_code first, since the table sees ANNA as AAAA), strand folding for canonical tables, the golden
`.count` file, planted multiplicities -- and from a short Python restatement of the record rules.  Never from the
library under test."""
import ctypes
import gzip
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
U64 = (1 << 64) - 1
_CODE = bytes(b"ACGT"[((b >> 1) ^ (b >> 2)) & 3] for b in range(256))   # base_code as a byte table
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s[::-1].translate(_COMP)


def line_spans(text):
    out, pos = [], 0
    for part in text.split(b"\n"):
        if part:
            out.append((pos, pos + len(part)))
        pos += len(part) + 1
    return out


def records(text, lpr):
    """[(sequence line, record bytes as the filter writes them)] with the reference's record rules."""
    sp = line_spans(text)
    out = []
    for i in range(0, len(sp), lpr):
        grp = sp[i:i + lpr]
        seq = text[grp[1][0]:grp[1][1]] if len(grp) > 1 else b""
        out.append((seq, text[grp[0][0]:grp[-1][1]] + b"\n"))
    return out


def coded_counts(text, k, lpr, canonical=False):
    """{coded k-mer: count}: every window of every sequence line, mapped through base_code; canonical: folded pairs."""
    c = Counter()
    for seq, _ in records(text, lpr):
        s = seq.translate(_CODE)
        for i in range(len(s) - k + 1):
            c[s[i:i + k]] += 1
    if canonical:
        f = Counter()
        for x, n in c.items():
            f[min(x, rc(x))] += n
        return f
    return c


def expected_stats(query, counts, k, lpr, lower, upper, canonical=False):
    out = []
    for seq, _ in records(query, lpr):
        s = seq.translate(_CODE)
        cs = []
        for i in range(len(s) - k + 1):
            x = s[i:i + k]
            cs.append(counts.get(min(x, rc(x)) if canonical else x, 0))
        out.append((len(cs), sum(lower <= c <= upper for c in cs), min(cs) if cs else 0, sum(cs) % (1 << 64)))
    return out


def as_tuples(st):
    return [tuple(int(v) for v in r) for r in st]


def expected_filter(query, stats, lpr, min_in=0, ppm=1000000, invert=False):
    recs = records(query, lpr)
    keep = [(inr >= min_in and inr * 1000000 >= ppm * km) != invert for (km, inr, _, _) in stats]
    return sum(keep), b"".join(r for (_, r), kp in zip(recs, keep) if kp)


def random_seqs(rnd, n, lo, hi, alphabet=b"ACGT"):
    return [bytes(rnd.choice(alphabet) for _ in range(rnd.randint(lo, hi))) for _ in range(n)]


def fastq_of(seqs, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def fasta_of(seqs, tag=b"r"):
    return b"".join(b">%s%d\n%s\n" % (tag, i, s) for i, s in enumerate(seqs))


def run_cli(*args, timeout=300):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


# ---- CPU --------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("tsx_hip_query_reads_device", "tsx_hip_query_reads_host", "tsx_hip_filter_reads_host",
               "tsx_hip_filter_reads_device")


def test_query_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    assert "tsx_hip_read_stats" in hdr and "tsx_hip_filter_rule" in hdr
    assert "TSXHashMap.h:548-638" in hdr and "FastXReader.h:62-116" in hdr
    assert ctypes.sizeof(T.FilterRule) == 32 and T.READ_STATS_DTYPE.itemsize == 32


def test_query_entry_points_refuse_bad_arguments_without_a_map():
    import tsxcount_amd as T
    L = T.lib()
    n = ctypes.c_size_t(7)
    assert L.tsx_hip_query_reads_host(None, b"@a\nACGT\n", 8, 1, 2, None, 0, ctypes.byref(n), 0) == T.EINVAL
    assert n.value == 0
    assert L.tsx_hip_query_reads_device(None, None, 0, 1, 2, None, 0, None, None) == T.EINVAL
    rule = T.filter_rule()
    assert L.tsx_hip_filter_reads_host(None, b"", 0, ctypes.byref(rule), 1, 0, None, None) == T.EINVAL
    assert L.tsx_hip_filter_reads_host(None, b"", 0, None, 1, 0, None, None) == T.EINVAL
    assert L.tsx_hip_filter_reads_device(None, None, 0, ctypes.byref(rule), None, 0, None, None, None) == T.EINVAL


def test_cli_usage_lists_the_query_options():
    code, out, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--filter=OUT", "--filter-input=FILE", "--filter-lower=N", "--filter-upper=N", "--filter-min=M",
                 "--filter-fraction=F", "--filter-invert", "--read-stats=FILE"):
        assert flag in err, flag
    code, _, err = run_cli("--input=x.fastq", "--filter=o", "--filter-lower=5", "--filter-upper=4", timeout=30)
    assert code == 1 and "Usage" in err
    code, _, err = run_cli("--input=x.fastq", "--filter=o", "--filter-fraction=1.5", timeout=30)
    assert code == 1 and "Usage" in err


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def make_map(T, k, l=20, s=0, path=1, lpr=4, canonical=False):
    m = T.TSXHashMapHIP(l, s, k, canonical=canonical)
    m.set_path(path)
    m.set_record_lines(lpr)
    return m


def table_text(rnd, k, lpr, n_reads=160):
    alphabet = b"ACG" if k < 8 else b"ACGT"   # k = 5: at most 3^5 distinct k-mers in a 2^9-slot table
    lo, hi = max(1, k - 3), k + 150
    seqs = random_seqs(rnd, n_reads, lo, hi, alphabet)
    return seqs, (fastq_of if lpr == 4 else fasta_of)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 14, 31, 32, 33, 63, 64, 127])
def test_stats_equal_restatement(T, k):
    rnd = random.Random(1000 + k)
    for lpr in (4, 2):
        seqs, fmt = table_text(rnd, k, lpr)
        half = seqs[: len(seqs) // 2]
        counted = fmt(seqs + half)   # counts of 1 and 2
        others = random_seqs(rnd, 40, max(1, k - 3), k + 120, b"ACG" if k < 8 else b"ACGT")
        queries = (counted, fmt(half + others, b"q"))
        counts = coded_counts(counted, k, lpr)
        for path in (1, 2):
            m = make_map(T, k, l=9 if k == 5 else 20, path=path, lpr=lpr)
            m.countFastq(counted)
            for qi, q in enumerate(queries):
                for lower, upper in ((1, None), (2, 2)):
                    want = expected_stats(q, counts, k, lpr, lower, U64 if upper is None else upper)
                    got = as_tuples(m.queryReads(q, lower, upper))
                    assert got == want, (k, lpr, path, qi, lower)
            m.close()


@pytest.mark.gpu
def test_carried_counts_are_exact(T):
    rnd = random.Random(7)
    k = 21
    seqs = random_seqs(rnd, 30, 40, 90)
    mult = [1, 3, 4, 5, 17, 40, 70, 130]
    planted = []
    for i, s in enumerate(seqs):
        planted += [s] * mult[i % len(mult)]
    rnd.shuffle(planted)
    text = fastq_of(planted)
    counts = coded_counts(text, k, 4)
    assert max(counts.values()) >= 130
    for s_bits, path in ((2, 1), (3, 2), (1, 1)):
        m = make_map(T, k, l=20, s=s_bits, path=path)
        m.countFastq(text)
        assert m.stats()["overflow_carries"] > 0
        for lower, upper in ((1, None), (4, 70), (100, None)):
            q = fastq_of(seqs)
            want = expected_stats(q, counts, k, 4, lower, U64 if upper is None else upper)
            assert as_tuples(m.queryReads(q, lower, upper)) == want, (s_bits, lower)
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 16, 31, 32, 33, 64])
def test_canonical_tables_either_strand(T, k):
    rnd = random.Random(300 + k)
    seqs = random_seqs(rnd, 80, k - 2, k + 100)
    if k % 2 == 0:   # palindromes: x == rc(x)
        for _ in range(5):
            h = bytes(rnd.choice(b"ACGT") for _ in range(k // 2))
            seqs.append(h + rc(h))
    text = fastq_of(seqs + seqs[::3] + [rc(s) for s in seqs[::4]])
    folded = coded_counts(text, k, 4, canonical=True)
    m = make_map(T, k, canonical=True, path=1)
    m.countFastq(text)
    for q in (fastq_of(seqs), fastq_of([rc(s) for s in seqs])):
        for lower in (1, 2, 3):
            want = expected_stats(q, folded, k, 4, lower, U64, canonical=True)
            assert as_tuples(m.queryReads(q, lower)) == want, (k, lower)
    m.close()


EDGE_FASTQ = (b"\n\n@a\nACGTACGTACGTAAACCCGGGTTT\n\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n\n\n"
              b"@short\nACG\n+\nIII\n"
              b"@low\nacgtNNacgtRYKMacgtacgt\r\n+\nIIIIIIIIIIIIIIIIIIIIIII\n"
              b"@emptyseq\n\n\nACGTTTTTTTTTTTTGGA\n+\n\nIIIIIIIIIIIIIIIIII\n"
              b"@tail")


@pytest.mark.gpu
@pytest.mark.parametrize("query", ["edges", "no_newline", "trailing_blank"])
def test_record_rule_edges(T, query):
    k = 7
    q = {"edges": EDGE_FASTQ, "no_newline": EDGE_FASTQ[:-5] + b"@x\nACGTACGTAAA",
         "trailing_blank": EDGE_FASTQ[:-5] + b"\n\n"}[query]
    counted = EDGE_FASTQ + fastq_of([b"ACGTACGTACGTAAACCCGG", b"aaaaaaaaaaaa"])
    counts = coded_counts(counted, k, 4)
    m = make_map(T, k, l=12)
    m.countFastq(counted)
    want = expected_stats(q, counts, k, 4, 1, U64)
    assert as_tuples(m.queryReads(q)) == want
    for chunk in (1, 5, 17, 64):
        assert as_tuples(m.queryReads(q, chunk_bytes=chunk)) == want, chunk
    kept, data = expected_filter(q, expected_stats(q, counts, k, 4, 2, U64), 4)
    p = os.path.join(os.environ.get("TMPDIR", "/tmp"), "tsx_rq_edge_%d.fq" % os.getpid())
    try:
        for chunk in (0, 7, 33):
            assert m.filterReads(q, p, lower=2, chunk_bytes=chunk) == (kept, len(data))
            assert open(p, "rb").read() == data
    finally:
        if os.path.exists(p):
            os.remove(p)
    m.close()


@pytest.mark.gpu
def test_long_fasta_record_spans_tiles_and_workgroups(T):
    rnd = random.Random(99)
    k = 31
    big = bytes(rnd.choice(b"ACGT") for _ in range(210000))
    small = random_seqs(rnd, 20, 10, 300)
    text = b">big\n" + big + b"\n" + fasta_of(small)
    q = fasta_of(small[:5]) + b">big again\n" + big + b"\n\n" + fasta_of([big[1000:5000], b"ACGT" * 40])
    counts = coded_counts(text, k, 2)
    m = make_map(T, k, l=22, lpr=2)
    m.countFastq(text)
    want = expected_stats(q, counts, k, 2, 1, U64)
    assert as_tuples(m.queryReads(q)) == want
    assert as_tuples(m.queryReads(q, chunk_bytes=4096)) == want   # the big record is taken whole
    m.close()


@pytest.mark.gpu
def test_seams_host_pieces_and_device_windows(T):
    import torch
    rnd = random.Random(5)
    k = 25
    seqs = random_seqs(rnd, 400, 20, 300)
    text = fastq_of(seqs + seqs[::2])
    q = b"\n".join(fastq_of(seqs[i:i + 7]) for i in range(0, len(seqs), 7)) + fastq_of(random_seqs(rnd, 30, 20, 200))
    counts = coded_counts(text, k, 4)
    m = make_map(T, k, l=20)
    m.countFastq(text)
    want = expected_stats(q, counts, k, 4, 2, U64)
    for chunk in (0, 4096, 4099, 5000, 10007, 1 << 16):
        assert as_tuples(m.queryReads(q, 2, chunk_bytes=chunk)) == want, chunk
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(q + b"\n" * 64), dtype=torch.uint8).to(dev)
    stats = torch.zeros((len(want) + 3) * 4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    try:
        for win in (None, 4096, 4112, 20000):
            if win:
                os.environ["TSX_HIP_DEV_WINDOW"] = str(win)
            else:
                os.environ.pop("TSX_HIP_DEV_WINDOW", None)
            n = m.queryReadsDevice(d_text.data_ptr(), len(q), stats.data_ptr(), len(want) + 3, lower=2)
            assert n == len(want)
            got = stats.cpu().numpy().view(np.uint64).reshape(-1, 4)[:n]
            assert as_tuples(got) == want, win
    finally:
        os.environ.pop("TSX_HIP_DEV_WINDOW", None)
    # too small a capacity: ERANGE and the count needed
    with pytest.raises(T.TSXException) as e:
        m.queryReadsDevice(d_text.data_ptr(), len(q), stats.data_ptr(), 3, lower=2)
    assert e.value.code == T.ERANGE
    m.close()


RULES = [  # (lower, upper, min_in_range, fraction, invert)
    (2, None, 0, 1.0, False),     # error filter: every k-mer seen at least twice
    (1, None, 1, 0.0, False),     # screening: at least one k-mer in the table
    (2, None, 0, 1.0, True),      # the failures of the error filter
    (0, None, 0, 0.0, False),     # keep all
    (2, 5, 3, 0.5, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("lpr", [4, 2])
def test_filter_python_c_abi_and_device(T, lpr, tmp_path):
    import torch
    rnd = random.Random(40 + lpr)
    k = 19
    fmt = fastq_of if lpr == 4 else fasta_of
    seqs = random_seqs(rnd, 300, 5, 250)
    text = fmt(seqs + seqs[::3])
    q = b"\n\n" + fmt(seqs[::2] + random_seqs(rnd, 60, 5, 200), b"q").replace(b"\n@q1", b"\n\n@q1") + b"\n"
    q = q.replace(b"\n>q1", b"\n\n\n>q1")
    counts = coded_counts(text, k, lpr)
    m = make_map(T, k, lpr=lpr)
    m.countFastq(text)
    L = T.lib()
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(q + b"\n" * 64), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(len(q) + 128, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for lower, upper, mn, frac, inv in RULES:
        st = expected_stats(q, counts, k, lpr, lower, U64 if upper is None else upper)
        kept, data = expected_filter(q, st, lpr, mn, int(round(frac * 1e6)), inv)
        if (lower, mn, frac, inv) == (0, 0, 0.0, False):   # keep all: the input minus the empty lines between records
            assert data == b"".join(r for _, r in records(q, lpr))
        p = str(tmp_path / "py.out")
        assert m.filterReads(q, p, lower, upper, mn, frac, inv) == (kept, len(data))
        assert open(p, "rb").read() == data
        assert m.filterReads(q, p, lower, upper, mn, frac, inv, chunk_bytes=3001) == (kept, len(data))
        assert open(p, "rb").read() == data
        rule = T.filter_rule(lower, upper, mn, frac, inv)
        kk, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        fd = os.open(str(tmp_path / "c.out"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            assert L.tsx_hip_filter_reads_host(m.handle, q, len(q), ctypes.byref(rule), fd, 1024, ctypes.byref(kk),
                                               ctypes.byref(nb)) == T.OK
        finally:
            os.close(fd)
        assert (kk.value, nb.value) == (kept, len(data))
        assert open(str(tmp_path / "c.out"), "rb").read() == data
        assert m.filterReadsDevice(d_text.data_ptr(), len(q), d_out.data_ptr(), d_out.numel(), rule) == (kept, len(data))
        assert bytes(d_out.cpu().numpy()[:len(data)]) == data
    m.close()


@pytest.mark.gpu
def test_filter_cli_inputs(T, tmp_path):
    rnd = random.Random(77)
    k = 17
    seqs = random_seqs(rnd, 200, 10, 200)
    counted = fastq_of(seqs + seqs[::2])
    q = fastq_of(seqs[::3] + random_seqs(rnd, 50, 10, 200), b"q")
    counts = coded_counts(counted, k, 4)
    (tmp_path / "in.fastq").write_bytes(counted)
    (tmp_path / "q.fastq").write_bytes(q)
    with gzip.open(str(tmp_path / "q.fastq.gz"), "wb") as f:
        f.write(q)
    (tmp_path / "qb.fastq.gz").write_bytes(T.bgzf_compress(q, block=1000))
    st = expected_stats(q, counts, k, 4, 2, U64)
    kept, data = expected_filter(q, st, 4)
    for qin in ("q.fastq", "q.fastq.gz", "qb.fastq.gz"):
        out = tmp_path / ("o_" + qin)
        code, so, se = run_cli("--input=" + str(tmp_path / "in.fastq"), "--k=%d" % k, "--l=20",
                               "--filter=" + str(out), "--filter-input=" + str(tmp_path / qin),
                               "--read-stats=" + str(tmp_path / "s.tsv"))
        assert code == 0, so + se
        assert out.read_bytes() == data, qin
        lines = (tmp_path / "s.tsv").read_text().splitlines()
        assert [tuple(int(v) for v in ln.split("\t")) for ln in lines] == [(i,) + s for i, s in enumerate(st)]
    code, so, se = run_cli("--input=" + str(tmp_path / "q.fastq"), "--k=%d" % k, "--l=20", "--filter-invert",
                           "--filter=" + str(tmp_path / "inv.fq"), "--filter-input=" + str(tmp_path / "q.fastq"))
    assert code == 0, so + se
    qc = coded_counts(q, k, 4)
    _, self_inv = expected_filter(q, expected_stats(q, qc, k, 4, 2, U64), 4, invert=True)
    assert (tmp_path / "inv.fq").read_bytes() == self_inv
    # counted input = filter input by default; screening rule
    code, so, se = run_cli("--input=" + str(tmp_path / "in.fastq"), "--k=%d" % k, "--l=20", "--filter-lower=1",
                           "--filter-min=1", "--filter-fraction=0", "--filter=" + str(tmp_path / "all.fq"))
    assert code == 0, so + se
    _, screened = expected_filter(counted, expected_stats(counted, counts, k, 4, 1, U64), 4, 1, 0)
    assert (tmp_path / "all.fq").read_bytes() == screened


@pytest.mark.gpu
def test_golden_cli_filter_and_stats(T, golden_fastq, golden_counts, tmp_path):
    k = 14
    inp = os.path.join(GOLDEN, "small_t7.1000.fastq")
    out, sts = tmp_path / "f.fq", tmp_path / "s.tsv"
    code, so, se = run_cli("--input=" + inp, "--k=14", "--l=24", "--filter=" + str(out), "--read-stats=" + str(sts),
                           "--filter-lower=3", "--filter-fraction=0.5")
    assert code == 0, so + se
    gold = {x.encode(): c for x, c in golden_counts.items()}
    st = expected_stats(golden_fastq, gold, k, 4, 3, U64)
    lines = sts.read_text().splitlines()
    assert len(lines) == 250
    assert [tuple(int(v) for v in ln.split("\t")) for ln in lines] == [(i,) + s for i, s in enumerate(st)]
    kept, data = expected_filter(golden_fastq, st, 4, 0, 500000)
    assert 0 < kept < 250
    assert out.read_bytes() == data


@pytest.mark.gpu
def test_refusals(T, tmp_path):
    text = fastq_of([b"ACGTACGTACGTACGTAAAC", b"ACGTTTTTGGGGACGT"])
    sh = T.TSXHashMapHIP(18, 0, 15, shard_bits=1, shard_index=0)
    with pytest.raises(T.TSXException) as e:
        sh.queryReads(text)
    assert e.value.code == T.EINVAL
    with pytest.raises(T.TSXException) as e:
        sh.filterReads(text, str(tmp_path / "x"))
    assert e.value.code == T.EINVAL
    sh.close()
    m = make_map(T, 15)
    m.countFastq(text)
    for bad in (dict(lower=3, upper=2),):
        with pytest.raises(T.TSXException) as e:
            m.queryReads(text, **bad)
        assert e.value.code == T.EINVAL
        with pytest.raises(T.TSXException) as e:
            m.filterReads(text, str(tmp_path / "x"), **bad)
        assert e.value.code == T.EINVAL
    with pytest.raises(T.TSXException) as e:
        m.filterReads(text, str(tmp_path / "x"), fraction=1.5)
    assert e.value.code == T.EINVAL
    out = np.zeros(1, dtype=T.READ_STATS_DTYPE)
    n = ctypes.c_size_t(0)
    assert T.lib().tsx_hip_query_reads_host(m.handle, text, len(text), 1, U64, out.ctypes.data_as(ctypes.c_void_p), 1,
                                            ctypes.byref(n), 0) == T.ERANGE
    assert n.value == 2
    m.close()
    (tmp_path / "in.fq").write_bytes(text)
    code, so, se = run_cli("--input=" + str(tmp_path / "in.fq"), "--k=15", "--l=18", "--gpus=2", "--comm=copy",
                           "--devices=0,0", "--filter=" + str(tmp_path / "g.out"), timeout=60)
    assert code != 0 and "one GPU" in se
    assert not (tmp_path / "g.out").exists()


@pytest.mark.gpu
def test_bench_shape(T):
    import torch
    from tsxcount_amd import synth
    seed, reads, k, l = 20261004, 1087000, 31, 30
    nbytes, _, polya = T.synth_sizes(seed, 0, reads, k, want_polya=True)
    dev = torch.device("cuda", 0)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    T.synth_fastq_device(seed, 0, reads, k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(l, 0, k)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    st = m.stats()
    stats = torch.zeros(reads * 4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    assert m.queryReadsDevice(text.data_ptr(), nbytes, stats.data_ptr(), reads) == reads
    del text
    s = stats.cpu().numpy().view(np.uint64).reshape(-1, 4)
    del stats
    assert int(s[:, 0].sum(dtype=np.uint64)) == st["kmers_added"]
    # the query text is the counted text: the sum of sum_count over reads is the sum over k-mers of c(x)^2
    h = m.getCountHistogram(1 << 20)
    assert int(h[-1]) == 1   # the pooled last bin holds the poly-A k-mer alone
    nz = np.nonzero(h[:-1])[0]
    binned = sum(int(c) * int(h[c]) for c in nz)
    pa = m.getKmerCount("A" * k)
    assert binned + pa == st["count_sum"] and pa >= polya
    want = (sum(int(c) * int(c) * int(h[c]) for c in nz) + pa * pa) % (1 << 64)
    assert sum(int(v) for v in s[:, 3]) % (1 << 64) == want
    # 2,000 sampled reads against tsx_hip_get_counts_host on their encoded windows (reads from synth.py's host twin)
    rnd = random.Random(3)
    idx = sorted(rnd.sample(range(reads), 2000))
    wins, owner = [], []
    for i in idx:
        seq = synth.fastq(seed, i, 1).split(b"\n")[1]
        wins += [seq[j:j + k] for j in range(len(seq) - k + 1)]
        owner += [i] * max(0, len(seq) - k + 1)
    a = np.frombuffer(b"".join(wins), dtype=np.uint8).reshape(len(wins), k).astype(np.uint64)
    codes = ((a >> np.uint64(1)) ^ (a >> np.uint64(2))) & np.uint64(3)
    enc = np.zeros(len(wins), dtype=np.uint64)
    for j in range(k):
        enc |= codes[:, j] << np.uint64(2 * j)
    got = m.getKmerCounts(enc.reshape(-1, 1))
    per = {}
    for i, cnt in zip(owner, got):
        per.setdefault(i, []).append(int(cnt))
    for i in idx:
        cs = per.get(i, [])
        want_i = (len(cs), sum(1 for c_ in cs if c_ >= 1), min(cs) if cs else 0, sum(cs) % (1 << 64))
        assert tuple(int(v) for v in s[i]) == want_i, i
    m.close()
