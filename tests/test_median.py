"""Read medians on the GPU: the count profile (tsx_hip_count_profile_*), the median of every record
(tsx_hip_median_reads_*) and the filter on it (tsx_hip_filter_median_host), through the C ABI, Python and the tsxCount
CLI.

Expectations come from the Python restatement of test_median_cpu.py only (expected_medians, expected_median_filter)
over coded_counts of the counted text.  Never from the library under test.  Everything is compared exactly; the forms
a case is about (the median that stays, the one that drops, the two middles, ...) are asserted on the restatement's
values, which check_text returns."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from test_median_cpu import NO, SAT, expected_median_filter, expected_medians
from test_read_query import U64, coded_counts, rc, run_cli
from test_trim import GENOME, PLANTS, closed_fd, fasta, fastq, planted_reads, sub
from test_trim_widths import random_bases, scaled_reads

K = 21
REPEAT = GENOME[5000:5200]                                   # counted twice: windows that start in [5000, 5180) have count 2
COUNTED = b">g\n" + GENOME + b"\n>again\n" + REPEAT + b"\n>polyA\n" + b"A" * 60 + b"\n"
COUNTS = coded_counts(COUNTED, K, 2)
HEAVY = [20, 40, 60, 80, 100, 120]                           # every window of a 150-base read holds a substitution


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def new_map(T, k=K, l=18, counted=COUNTED, **kw):
    m = T.TSXHashMapHIP(l, 0, k, **kw)
    m.set_path(1)
    m.set_record_lines(2)
    m.countFastq(counted)
    return m


@pytest.fixture(scope="module")
def gmap(T):
    m = new_map(T)
    yield m
    m.close()


def to_device(text):
    import torch
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    if text:
        dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    return dev


def pairs(a):
    return [(int(x), int(y)) for x, y in a]


def device_forms(m, text, nrec):
    """(profile, medians) of the device forms; the entries behind the text and behind the records stay untouched."""
    import torch
    dev = to_device(text)
    dprof = torch.full((len(text) + 8,), 77, dtype=torch.int32, device="cuda:0")
    m.countProfileDevice(dev.data_ptr(), len(text), dprof.data_ptr())
    prof = dprof.cpu().numpy().view(np.uint32)
    assert (prof[len(text):] == 77).all()
    dmed = torch.full((nrec + 3, 2), -1, dtype=torch.int64, device="cuda:0")
    assert m.medianReadsDevice(dev.data_ptr(), len(text), dmed.data_ptr(), nrec + 3) == nrec
    med = dmed.cpu().numpy()
    assert (med[nrec:] == -1).all()
    return prof[:len(text)], [tuple(r) for r in med[:nrec].tolist()]


def check_text(m, text, lpr, counts=COUNTS, k=K, chunks=(0,), device=True, **kw):
    """Profile and medians of the host forms at every piece size, and of the device forms, against the restatement;
    returns the medians."""
    m.set_record_lines(lpr)
    prof, meds = expected_medians(text, counts, k, lpr, **kw)
    for chunk in chunks:
        got = m.countProfile(text, chunk_bytes=chunk)
        assert got.dtype == np.uint32 and np.array_equal(got, prof), (chunk, np.flatnonzero(got != prof)[:8])
        assert pairs(m.medianReads(text, chunk_bytes=chunk)) == meds, chunk
    if device:
        dprof, dmeds = device_forms(m, text, len(meds))
        assert np.array_equal(dprof, prof), np.flatnonzero(dprof != prof)[:8]
        assert dmeds == meds
    return meds


def filter_out(m, text, tmp_path, **kw):
    p = str(tmp_path / "median.out")
    kept, nbytes = m.filterReadsByMedian(text, p, **kw)
    data = open(p, "rb").read()
    assert nbytes == len(data)
    return kept, data


def shaped_reads(rnd):
    """(reads, index of the first of the named forms).  After 150-base reads with the substitution plants of test_trim.py
    (from the part of the genome counted once): a read with every window hit, reads shorter than k and of exactly k, an
    even and two odd numbers of windows whose middle counts differ, poly-A, a read the table has never seen."""
    seqs = []
    for pl in PLANTS:
        a = rnd.randrange(6000, 19000)
        seqs.append(sub(GENOME[a:a + 150], pl))
    at = len(seqs)
    seqs += [sub(GENOME[9000:9150], HEAVY), GENOME[300:300 + K - 1], GENOME[300:300 + K],
             GENOME[4950:5070], GENOME[4950:5071], GENOME[4949:5070],
             b"A" * 100, random_bases(rnd, 150)]
    return seqs, at


def assert_shapes(meds, at):
    assert meds[:len(PLANTS)] == [(130, 1)] * len(PLANTS)     # up to three plants spoil 42 of 130 windows: the median stays
    assert meds[at:at + 3] == [(130, 0), (0, 0), (1, 1)]       # more than half the windows hit; k - 1; exactly k
    assert meds[at + 3] == (100, 2)                            # 50 ones, 50 twos: the upper middle
    assert meds[at + 4] == (101, 2) and meds[at + 5] == (101, 1)   # 50 + 51 and 51 + 50
    assert meds[at + 6] == (80, 40) and meds[at + 7] == (130, 0)   # poly-A (40 windows of the counted A^60); unseen


@pytest.mark.gpu
@pytest.mark.parametrize("lpr", [4, 2])
def test_record_shapes(T, gmap, lpr):
    seqs, at = shaped_reads(random.Random(31))
    body = (fastq if lpr == 4 else fasta)(seqs)
    head = b"@" if lpr == 4 else b">"
    tail = GENOME[7000:7100]
    texts = {"whole": body,
             "empty_lines": b"\n\n" + body.replace(b"\n" + head + b"r5\n", b"\n\n\n" + head + b"r5\n") + b"\n\n",
             "incomplete": body + head + b"tail\n" + tail + b"\n",
             "incomplete_open": body + head + b"tail\n" + tail,
             "header_only_tail": body + head + b"tail"}
    if lpr == 4:
        texts["unterminated"] = body + b"@u\n" + tail + b"\n+\n" + b"M" * 100
    for name, text in texts.items():
        meds = check_text(gmap, text, lpr, chunks=(0, 1500))
        assert_shapes(meds, at)
        assert len(meds) == len(seqs) + (0 if name in ("whole", "empty_lines") else 1), name
        if name in ("incomplete", "incomplete_open", "unterminated"):
            assert meds[-1] == (80, 1), name
        if name == "header_only_tail":
            assert meds[-1] == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [21, 40, 70, 127])
def test_every_key_width(T, k, canonical):
    rnd = random.Random(8100 + k)
    genome = random_bases(rnd, 4000)
    counted = fasta([genome, genome[1000:1000 + 2 * k + 40]])      # a stretch counted twice
    counts = coded_counts(counted, k, 2, canonical=canonical)
    m = new_map(T, k=k, l=17, counted=counted, canonical=canonical)
    assert m.wk == (2 * k + 63) // 64
    for lpr, fmt in ((4, fastq), (2, fasta)):
        seqs = scaled_reads(rnd, genome, k, copies=2)
        seqs += [genome[999 - k:1000 + 2 * k], genome[999 - k:999 + 2 * k]]   # k + 1 ones, then k + 1 / k twos
        if canonical:
            seqs = [rc(s) if i % 2 else s for i, s in enumerate(seqs)]
        text = fmt(seqs, 7)
        meds = check_text(m, text, lpr, counts=counts, k=k, chunks=(0, len(text) // 5), canonical=canonical)
        assert meds[-2] == (2 * k + 2, 2) and meds[-1] == (2 * k + 1, 1)   # the upper middle of an even count; the middle
        assert meds[0] == (3 * k + 71, 1) and meds[8] == (0, 0) and meds[9][0] == 1   # clean; k - 1; k
        assert meds[11] == (3 * k + 71, 0)                                            # unseen
    m.close()


@pytest.mark.gpu
def test_base_rules(T):
    at = GENOME.index(b"A", 8070) - 70
    read = GENOME[at:at + 150]
    withn = read[:70] + b"N" + read[71:]      # N takes the code of A: a k-mer of the genome unless the rule drops the windows
    text = fastq([withn, read, b"N" * 60])
    m = new_map(T, acgt_only=True)
    meds = check_text(m, text, 4, acgt_only=True, chunks=(0, 400))
    assert meds == [(130 - K, 1), (130, 1), (0, 0)]
    prof = m.countProfile(text)
    s = text.index(withn)
    assert (prof[s + 50:s + 71] == NO).all() and prof[s + 49] == 1 and prof[s + 71] == 1
    m.close()
    m = new_map(T)
    assert check_text(m, text, 4) == [(130, 1), (130, 1), (40, 40)]   # N^60 reads as the counted A^60
    m.set_base_rule(min_qual_char="5")
    q = bytearray(b"I" * 150)
    q[50] = ord("#")
    text = (b"@low\n" + read + b"\n+\n" + bytes(q) + b"\n" + b"@shortq\n" + GENOME[600:690] + b"\n+\n" + b"J" * 40 + b"\n" +
            fastq([read]))
    meds = check_text(m, text, 4, minq=ord("5"), chunks=(0, 400))
    assert meds == [(130 - K, 1), (40 - K + 1, 1), (130, 1)]
    m.close()


@pytest.mark.gpu
def test_saturated_counts(T):
    m = new_map(T)
    poly_c = b"C" * K
    assert COUNTS.get(poly_c, 0) == 0
    m.addKmers(T.encode_many([poly_c], K), [1 << 33])
    counts = dict(COUNTS)
    counts[poly_c] = 1 << 33
    text = fastq([b"C" * 100 + GENOME[200:230], GENOME[200:350], b"C" * K])
    prof, want = expected_medians(text, counts, K, 4)
    assert want[0] == (110, SAT) and want[1] == (130, 1) and want[2] == (1, SAT)
    assert int((prof == SAT).sum()) == 81
    assert check_text(m, text, 4, counts=counts) == want
    m.close()


@pytest.mark.gpu
def test_long_records_take_the_workgroup_form(T, gmap, monkeypatch):
    """One 20 kbp record with its default threshold (the wave form reads it again every pass), then everything longer than
    256 bases through the workgroup form: the same text of reads, a 600-base read (more than 512 windows: past the
    register form) and the long record."""
    rnd = random.Random(33)
    seqs, at = shaped_reads(rnd)
    long = bytearray(GENOME)
    for p in range(3000, 9000, 7):
        long[p] = ord("N")   # (a stretch without seen windows, so that the counts of the record differ)
    seqs += [GENOME[4700:5300], bytes(long), GENOME[4801:5380], GENOME[4802:5381], GENOME[4803:5382], GENOME[0:300]]
    text = fasta(seqs, 3)
    _, want = expected_medians(text, COUNTS, K, 2)
    assert_shapes(want, at)
    n = len(seqs)
    assert want[n - 6] == (580, 1) and want[n - 5][0] == 20000 - K + 1 and want[n - 1] == (280, 1)
    assert [w[0] for w in want[n - 4:n - 1]] == [559] * 3   # records of 585 bytes: their profiles start at every offset mod 4
    for thr in (None, "256", "16384", "20000"):
        if thr:
            monkeypatch.setenv("TSX_HIP_MEDIAN_LONG", thr)
        else:
            monkeypatch.delenv("TSX_HIP_MEDIAN_LONG", raising=False)
        assert check_text(gmap, text, 2, chunks=(0, 6000)) == want, thr
    monkeypatch.delenv("TSX_HIP_MEDIAN_LONG", raising=False)


@pytest.mark.gpu
def test_windows_and_pieces_equal_one_piece(T, monkeypatch):
    seqs = planted_reads(random.Random(34), copies=7) + [GENOME[2000:9000]]   # a record longer than a piece
    seqs += planted_reads(random.Random(35))
    for lpr, fmt in ((4, fastq), (2, fasta)):
        text = fmt(seqs, 5)
        assert len(text) >= 5 * 4096 + 64
        monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "4096")
        monkeypatch.setenv("TSX_HIP_DEV_WINDOW", "4096")
        m = new_map(T)
        monkeypatch.delenv("TSX_HIP_PIECE_BYTES")
        want = check_text(m, text, lpr, chunks=(0, 3000, 700))
        monkeypatch.delenv("TSX_HIP_DEV_WINDOW")
        m.close()
        m = new_map(T)
        assert check_text(m, text, lpr, chunks=(0, 3000)) == want
        m.close()
        assert want[len(seqs) - len(planted_reads(random.Random(35))) - 1] == (7000 - K + 1, 1)


@pytest.mark.gpu
def test_caps_and_small_texts(T, gmap):
    import torch
    seqs, at = shaped_reads(random.Random(36))
    text = fastq(seqs)
    gmap.set_record_lines(4)
    _, want = expected_medians(text, COUNTS, K, 4)
    L = T.lib()
    n = ctypes.c_size_t(0)
    few = np.zeros(6, dtype=T.READ_MEDIAN_DTYPE)
    for chunk in (0, 700):
        few[:] = 0
        few[5] = (9, 9)
        assert L.tsx_hip_median_reads_host(gmap.handle, text, len(text), few.ctypes.data_as(ctypes.c_void_p), 5, ctypes.byref(n),
                                           chunk) == T.ERANGE
        assert n.value == len(want) and pairs(few[:5]) == want[:5] and pairs(few[5:]) == [(9, 9)]
    dev = to_device(text)
    dmed = torch.full((6, 2), -1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(T.TSXException) as e:
        gmap.medianReadsDevice(dev.data_ptr(), len(text), dmed.data_ptr(), 5)
    assert e.value.code == T.ERANGE
    assert [tuple(r) for r in dmed.cpu().tolist()] == want[:5] + [(-1, -1)]
    # an empty text, a text of one header line, a text of empty lines
    for lpr in (4, 2):
        gmap.set_record_lines(lpr)
        assert len(gmap.medianReads(b"")) == 0 and len(gmap.countProfile(b"")) == 0
        assert gmap.medianReadsDevice(dev.data_ptr(), 0, dmed.data_ptr(), 6) == 0
        gmap.countProfileDevice(dev.data_ptr(), 0, dmed.data_ptr())
        for tiny, nrec in ((b"@h", 1), (b"@h\n", 1), (b"\n\n\n", 0)):
            assert check_text(gmap, tiny, lpr) == [(0, 0)] * nrec, tiny
            assert (gmap.countProfile(tiny) == NO).all()


@pytest.mark.gpu
def test_filter_by_median(T, gmap, tmp_path):
    seqs, at = shaped_reads(random.Random(37))
    body = fastq(seqs)
    text = b"\n" + body.replace(b"\n@r4\n", b"\n\n@r4\n") + b"@u\n" + GENOME[7000:7100] + b"\n+\n" + b"M" * 100
    gmap.set_record_lines(4)
    _, meds = expected_medians(text, COUNTS, K, 4)
    assert {md for _, md in meds} == {0, 1, 2, 40}
    rules = [dict(lower=2), dict(upper=1), dict(lower=1, upper=2), dict(lower=1, invert=True), dict(lower=41),
             dict(), dict(lower=50, invert=True)]
    for kw in rules:
        kept, data = expected_median_filter(text, meds, 4, lower=kw.get("lower", 0), upper=kw.get("upper", U64),
                                            invert=kw.get("invert", False))
        for chunk in (0, 1200):
            assert filter_out(gmap, text, tmp_path, chunk_bytes=chunk, **kw) == (kept, data), (kw, chunk)
    kept, data = expected_median_filter(text, meds, 4, lower=41)
    assert (kept, data) == (0, b"")
    kept, data = expected_median_filter(text, meds, 4)
    everything = b"".join(ln + b"\n" for ln in text.split(b"\n") if ln)   # the input minus empty lines, plus a final '\n'
    assert kept == len(meds) and data == everything
    assert expected_median_filter(text, meds, 4, lower=50, invert=True) == (kept, data)
    with pytest.raises(T.TSXException) as e:
        gmap.filterReadsByMedian(text, closed_fd(tmp_path), lower=1)
    assert e.value.code == T.EIO
    # what a map refuses: bad rules, and a shard
    L = T.lib()
    for bad in (T.MedianRule(3, 2, 0, 0), T.MedianRule(0, U64, 0, 1)):
        assert L.tsx_hip_filter_median_host(gmap.handle, text, len(text), ctypes.byref(bad), 1, 0, None, None) == T.EINVAL
    assert L.tsx_hip_filter_median_host(gmap.handle, text, len(text), None, 1, 0, None, None) == T.EINVAL
    shard = T.TSXHashMapHIP(18, 0, K, shard_bits=1, shard_index=0)
    for call in (lambda: shard.medianReads(text), lambda: shard.countProfile(text),
                 lambda: shard.filterReadsByMedian(text, str(tmp_path / "s.out"))):
        with pytest.raises(T.TSXException) as e:
            call()
        assert e.value.code == T.EINVAL
    shard.close()


@pytest.mark.gpu
def test_cross_checks_with_the_read_query(T, gmap):
    """In addition to the restatement: kmers is the query's (no base rule), and a record's profile sums to its sum_count."""
    from test_read_query import line_spans
    seqs, _ = shaped_reads(random.Random(38))
    for lpr, fmt in ((4, fastq), (2, fasta)):
        text = fmt(seqs)
        gmap.set_record_lines(lpr)
        st = gmap.queryReads(text)
        md = gmap.medianReads(text)
        prof = gmap.countProfile(text)
        assert len(st) == len(md) == len(seqs)
        assert [int(x) for x in md["kmers"]] == [int(x) for x in st["kmers"]]
        sp = line_spans(text)
        for r in range(len(seqs)):
            a, b = sp[r * lpr + 1]
            vals = prof[a:b]
            vals = vals[vals != NO]
            assert len(vals) == int(md["kmers"][r]) and int(vals.astype(np.uint64).sum()) == int(st["sum_count"][r])
            assert int(md["median"][r]) == T.median_count(prof[a:b])


@pytest.mark.gpu
def test_golden_cli_medians(T, tmp_path):
    import kmerdb
    k = 14
    db = os.path.join(GOLDEN, "small_t7.first8.k14.v1.db")
    inp = os.path.join(GOLDEN, "small_t7.1000.fastq")
    info = T.database_info(db)
    m = T.TSXHashMapHIP(info["l"], info["count_bits"], k, hash_seed=info["hash_seed"])
    try:
        f = kmerdb.read_db(db, m.hash_rows())
    finally:
        m.close()
    counts = {(x if isinstance(x, bytes) else x.encode()): int(c) for x, c in f.kmers.items()}
    assert len(counts) > 100 and max(counts.values()) > 3
    text = open(inp, "rb").read()
    _, meds = expected_medians(text, counts, k, 4)
    assert len(meds) == 250 and 0 < sum(1 for _, md in meds if md >= 1) < 250   # (the file has 1000 lines)
    tsv, out = tmp_path / "m.tsv", tmp_path / "f.fq"
    code, so, se = run_cli("--load=" + db, "--filter-input=" + inp, "--read-medians=" + str(tsv), "--filter=" + str(out),
                           "--filter-median-lower=1")
    assert code == 0, so + se
    assert [tuple(int(v) for v in ln.split("\t")) for ln in tsv.read_text().splitlines()] == \
        [(i,) + md for i, md in enumerate(meds)]
    kept, data = expected_median_filter(text, meds, 4, lower=1)
    assert out.read_bytes() == data and ("Wrote %d records" % kept) in se
    code, so, se = run_cli("--load=" + db, "--filter-input=" + inp, "--filter=" + str(out), "--filter-median-upper=0",
                           "--filter-invert")
    assert code == 0, so + se
    assert out.read_bytes() == data
