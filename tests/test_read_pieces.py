"""What the read calls share: the host piece driver at piece sizes below, at and just above one record (trim and
medians; test_read_query.py has the query's), the same piece sizes through the calls that write several files (bin
reads, pairs) and through normalization and correction, the TSX_HIP_PIECE_BYTES cap that only the median calls honour,
and the device window walk over an empty text after a call that left a scan carry behind.

Expectations come from the Python restatements of test_read_query.py, test_trim.py, test_median_cpu.py, test_pairs.py,
test_bin_reads.py, normalize_ref.py and correct_model (as test_correct.py uses it) over the counts of the counted
text.  Never from the library under test.  Everything is compared exactly."""
import ctypes
import random

import numpy as np
import pytest

import test_bin_reads as TB
import test_correct as TC
from normalize_ref import normalize
from test_median import filter_out, pairs, to_device
from test_median_cpu import expected_median_filter, expected_medians
from test_pairs import expect_epair, filter_mates, interleaved, pair_model, run_pairs, trim_mates
from test_read_query import U64, as_tuples, coded_counts, expected_filter, expected_stats
from test_trim import as_pairs, expected_trim, sub, write_out

pytestmark = pytest.mark.gpu

K, L = 21, 16
_rnd = random.Random(4242)
GENOME = bytes(_rnd.choice(b"ACGT") for _ in range(3000))
COUNTED = b">g\n" + GENOME + b"\n>again\n" + GENOME[1000:1200] + b"\n"   # medians of 1 and of 2
COUNTS = coded_counts(COUNTED, K, 2)


def _reads(rnd, n=30, shift=0):
    """n reads of 25..120 bases, the first the longest; every third with a substitution, some unseen or shorter than k
    (`shift` moves which)."""
    out = []
    for j in range(n):
        i = j + shift
        ln = 120 if j == 0 else rnd.randint(25, 120)
        at = rnd.randrange(1000, 1200 - ln) if i % 5 == 2 else rnd.randrange(0, len(GENOME) - ln)   # (the part counted twice)
        s = GENOME[at:at + ln]
        if i % 3 == 1:
            s = sub(s, [rnd.randrange(0, ln)])
        if i % 7 == 5:
            s = bytes(rnd.choice(b"ACGT") for _ in range(ln))
        if i % 11 == 9:
            s = s[:K - 1]
        out.append(s)
    return out


def _fastq(seqs, tag=b"r"):
    return [b"@%s%d/x\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs)]


RECS = _fastq(_reads(random.Random(1)))
TEXT = b"".join(RECS)[:-1]                       # the last line without its '\n'
REC = len(RECS[0])
CHUNKS = (1, REC, REC + 1)                       # every piece grows; exactly the first record; one byte more


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def new_map(T):
    m = T.TSXHashMapHIP(L, 0, K)
    m.set_path(1)
    m.set_record_lines(2)
    m.countFastq(COUNTED)
    m.set_record_lines(4)
    return m


@pytest.fixture(scope="module")
def gmap(T):
    m = new_map(T)
    yield m
    m.close()


@pytest.fixture(scope="module")
def want():
    """The restated results of TEXT, computed once."""
    w = {"trim": {mode: expected_trim(TEXT, COUNTS, K, 4, mode=mode) for mode in ("longest", "prefix")}}
    w["prof"], w["meds"] = expected_medians(TEXT, COUNTS, K, 4)
    w["stats"] = expected_stats(TEXT, COUNTS, K, 4, 1, U64)
    return w


def test_the_text_is_what_the_cases_need(want):
    assert len(RECS) == 30 and REC == max(len(r) for r in RECS) and not TEXT.endswith(b"\n")
    assert REC + 1 < len(RECS[0]) + len(RECS[1])                     # one byte more still holds one record only
    spans, out, tot = want["trim"]["longest"]
    assert 0 < tot["kept"] < tot["records"] == 30 and any(0 < ln < len(s) - 4 for (_, ln), s in zip(spans, _reads(random.Random(1))))
    assert {md for _, md in want["meds"]} >= {0, 1, 2}


@pytest.mark.parametrize("chunk", CHUNKS)
def test_trim_at_piece_sizes_around_one_record(gmap, want, chunk, tmp_path):
    for mode in ("longest", "prefix"):
        spans, out, tot = want["trim"][mode]
        assert as_pairs(gmap.trimSpans(TEXT, lower=1, mode=mode, chunk_bytes=chunk)) == spans, mode
        got, gtot = write_out(gmap, TEXT, tmp_path, lower=1, mode=mode, chunk_bytes=chunk)
        assert got == out and gtot == tot, mode


@pytest.mark.parametrize("chunk", CHUNKS)
def test_medians_at_piece_sizes_around_one_record(gmap, want, chunk, tmp_path):
    got = gmap.countProfile(TEXT, chunk_bytes=chunk)
    assert np.array_equal(got, want["prof"]), np.flatnonzero(got != want["prof"])[:8]
    assert pairs(gmap.medianReads(TEXT, chunk_bytes=chunk)) == want["meds"]
    for kw in (dict(lower=1), dict(lower=2), dict(lower=1, upper=1, invert=True)):
        exp = expected_median_filter(TEXT, want["meds"], 4, lower=kw["lower"], upper=kw.get("upper", U64),
                                     invert=kw.get("invert", False))
        assert 0 < exp[0] < 30
        assert filter_out(gmap, TEXT, tmp_path, chunk_bytes=chunk, **kw) == exp, kw


def test_only_the_median_calls_honour_the_piece_cap(T, want, tmp_path, monkeypatch):
    """A map created with TSX_HIP_PIECE_BYTES = 256 (about one record): the query, trim and pair calls with chunk_bytes = 0
    take the text as they do without the cap and give the same results; the median calls cut it into pieces of at most
    256 bytes and give the same results too."""
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "256")   # read when the map is created
    m = new_map(T)
    monkeypatch.delenv("TSX_HIP_PIECE_BYTES")
    try:
        assert as_tuples(m.queryReads(TEXT, lower=1)) == want["stats"]
        exp = expected_filter(TEXT, want["stats"], 4, min_in=1)
        p = str(tmp_path / "f.out")
        assert m.filterReads(TEXT, p, lower=1, min_in_range=1) == (exp[0], len(exp[1])) and open(p, "rb").read() == exp[1]
        assert 0 < exp[0] < 30
        spans, out, tot = want["trim"]["longest"]
        assert as_pairs(m.trimSpans(TEXT, lower=1)) == spans
        assert write_out(m, TEXT, tmp_path, lower=1) == (out, tot)
        # mates: the reads, and other reads under the same names
        a = b"".join(RECS)
        b = b"".join(_fastq(_reads(random.Random(2), shift=1)))
        fw = pair_model(filter_mates(a, 4, COUNTS, K), filter_mates(b, 4, COUNTS, K))
        assert fw[4]["kept"] and fw[4]["single1"] and fw[4]["single2"]
        assert run_pairs(m, "filter", a, b, tmp_path, pairs="both", lower=1, check_names=True) == fw
        tw = pair_model(trim_mates(a, 4, COUNTS, K), trim_mates(b, 4, COUNTS, K), trim=True)
        assert tw[4]["kept"] and tw[4]["single1"] and tw[4]["single2"]
        assert run_pairs(m, "trim", a, b, tmp_path, lower=1, check_names=True) == tw
        # the medians: at most 256 bytes a piece
        assert np.array_equal(m.countProfile(TEXT), want["prof"])
        assert pairs(m.medianReads(TEXT)) == want["meds"]
        exp = expected_median_filter(TEXT, want["meds"], 4, lower=1)
        assert filter_out(m, TEXT, tmp_path, lower=1) == exp
    finally:
        m.close()


# ---- the calls that write several files, and the ones that came after the piece driver -------------------------------
# Mates: the reads, and other reads under the same names (as test_only_the_median_calls_honour_the_piece_cap).
MATES_A = RECS
MATES_B = _fastq(_reads(random.Random(2), shift=1))
B_COUNTED = b">b\n" + GENOME[:1150] + b"\n"       # table B: part of the genome, and most of the part A counted twice
A_RANGE = (2, None)                              # A's hits: the k-mers A counted twice
NORM = dict(cutoff=2, R=4)
RAW_COUNTS = TC.kmer_counts([GENOME, GENOME[1000:1200]], K)   # the table by k-mer bytes, as correct_model takes it


def _pair_want(w, kind, n=None):
    ma, mb = w[kind]
    return pair_model(ma[:n], mb[:n], trim=kind == "trim")


def _interleaved_want(w, kind):
    """The two outputs of an interleaved text (test_pairs.test_interleaved): kept mates alternate, orphans share a file."""
    ma, mb = w[kind]
    t = pair_model(ma, mb, trim=kind == "trim")[4]
    keep = [x[0] and y[0] for x, y in zip(ma, mb)]
    kept = b"".join(x[1] + y[1] for x, y, kp in zip(ma, mb, keep) if kp)
    single = b"".join((x[1] if x[0] else y[1]) for x, y, kp in zip(ma, mb, keep) if not kp and x[0] != y[0])
    return kept, b"", single, b"", dict(t, bytes1=len(kept), bytes2=0, bytes_single1=len(single), bytes_single2=0)


@pytest.fixture(scope="module")
def want_more(T):
    """The restated results of the calls below, computed once.  Every case that takes them is guarded here against a
    trivial expectation: every class and every output file non-empty, reads dropped and reads kept."""
    w = {}
    ca, cb = TB.counts_of(COUNTED, K, 2), TB.counts_of(B_COUNTED, K, 2)
    _, w["cls"] = TB.expected(TEXT, ca, cb, K, 4, a_range=A_RANGE)
    w["bins"] = TB.expected_files(TEXT, w["cls"], 4)
    assert all(w["cls"].count(c) for c in range(4)) and all(w["bins"])
    a, b = b"".join(MATES_A), b"".join(MATES_B)
    w["filter"] = (filter_mates(a, 4, COUNTS, K), filter_mates(b, 4, COUNTS, K))
    w["trim"] = (trim_mates(a, 4, COUNTS, K), trim_mates(b, 4, COUNTS, K))
    for kind in ("filter", "trim"):
        for got in (_pair_want(w, kind), _pair_want(w, kind, 29), _interleaved_want(w, kind)):
            t = got[4]
            assert 0 < t["kept"] < t["pairs"] and t["single1"] and t["single2"], kind
            assert got[0] and got[2] and (got[1] and got[3] or not (got[1] or got[3])), kind   # (interleaved: two files)
    w["norm"] = normalize(TEXT, K, 4, NORM["cutoff"], NORM["R"], counts=COUNTS)
    keep, out, tot, _ = w["norm"]
    assert 0 < tot["kept"] < tot["records"] == 30 and out and tot["rounds"] == 8
    w["correct"] = T.correct.correct_model(TEXT, RAW_COUNTS, K, lower=1)
    out, fixes, tot = w["correct"]
    assert fixes and 0 < len({f[0] for f in fixes}) < 30 and out != TEXT and len(out) == len(TEXT)
    return w


@pytest.fixture(scope="module")
def bmap(T):
    m = T.TSXHashMapHIP(L, 0, K)
    m.set_path(1)
    m.set_record_lines(2)
    m.countFastq(B_COUNTED)
    m.set_record_lines(4)
    yield m
    m.close()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_bin_reads_at_piece_sizes_around_one_record(gmap, bmap, want_more, chunk, tmp_path):
    cls, files = want_more["cls"], want_more["bins"]
    paths = [str(tmp_path / ("%s.out" % n)) for n in TB.NAMES]
    tot = gmap.binReads(bmap, TEXT, *paths, a_range=A_RANGE, chunk_bytes=chunk)
    assert tot == {"records": 30, "n": [cls.count(c) for c in range(4)], "bytes": [len(f) for f in files]}
    assert [open(p, "rb").read() for p in paths] == files
    # two of the four dropped: their classes are counted, with no bytes
    two = [str(tmp_path / ("two_%s.out" % n)) for n in TB.NAMES]
    tot = gmap.binReads(bmap, TEXT, None, two[1], None, two[3], a_range=A_RANGE, chunk_bytes=chunk)
    assert tot == {"records": 30, "n": [cls.count(c) for c in range(4)], "bytes": [0, len(files[1]), 0, len(files[3])]}
    assert open(two[1], "rb").read() == files[1] and open(two[3], "rb").read() == files[3]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["filter", "trim"])
def test_pairs_at_piece_sizes_around_one_record(gmap, want_more, kind, chunk, tmp_path):
    a, b = b"".join(MATES_A), b"".join(MATES_B)
    kw = dict(lower=1, check_names=True, chunk_bytes=chunk, **(dict(pairs="both") if kind == "filter" else {}))
    assert run_pairs(gmap, kind, a, b, tmp_path, **kw) == _pair_want(want_more, kind)
    assert run_pairs(gmap, kind, interleaved(MATES_A, MATES_B), None, tmp_path, **kw) == _interleaved_want(want_more, kind)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["filter", "trim"])
def test_pairs_out_of_step_keep_the_rounds_before(T, gmap, want_more, kind, chunk, tmp_path):
    """Text 2 is one record short.  Every round takes as many records from each text as both pieces hold, so the round
    that fails is the one that finds text 2 used up: the 29 whole pairs before it are in the files, and nothing else."""
    a, b = b"".join(MATES_A), b"".join(MATES_B[:-1])
    kw = dict(lower=1, chunk_bytes=chunk, **(dict(pairs="both") if kind == "filter" else {}))
    why = expect_epair(T, lambda: run_pairs(gmap, kind, a, b, tmp_path, tag="e", **kw))
    assert "text 2 ends after 29 records" in why
    want = _pair_want(want_more, kind, 29)
    assert tuple(open(str(tmp_path / ("e%d" % i)), "rb").read() for i in range(4)) == want[:4]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_normalize_to_a_file_at_piece_sizes_around_one_record(T, want_more, chunk, tmp_path):
    """Rounds of 4 records: a piece of 1 byte grows to a whole record and on to a whole round."""
    keep, out, tot, _ = want_more["norm"]
    path = str(tmp_path / "norm.out")
    m = new_map(T)
    try:
        got = m.normalizeReads(TEXT, path, cutoff=NORM["cutoff"], round_records=NORM["R"], keep=True, chunk_bytes=chunk)
        assert got["keep"].tolist() == keep and {f: got[f] for f in tot} == tot
        assert open(path, "rb").read() == out
    finally:
        m.close()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_correct_at_piece_sizes_around_one_record(T, gmap, want_more, chunk, tmp_path):
    C = T.correct
    out, fixes, tot = want_more["correct"]
    corr, ctot = C.correction_sites(gmap, TEXT, lower=1, chunk_bytes=chunk)
    assert TC.as_tuples(corr) == fixes and ctot == dict(tot, bytes=0)
    path = str(tmp_path / "corrected.fq")
    assert C.correct_reads(gmap, TEXT, path, lower=1, chunk_bytes=chunk) == tot
    assert open(path, "rb").read() == out


def test_an_empty_device_text_has_no_records(T):
    """Through the C ABI: after a count and a query of a device text (which leave line ends in the scan carry), n = 0
    with capacity 0 gives TSX_HIP_OK and no records from each of the three window walks."""
    import torch
    lib = T.lib()
    dev = to_device(TEXT)
    dst = torch.zeros((len(RECS), 4), dtype=torch.int64, device="cuda:0")
    m = T.TSXHashMapHIP(L, 0, K)
    try:
        m.set_record_lines(4)
        m.countFastqDevice(dev.data_ptr(), len(TEXT))
        rule = T.trim_rule(1, None, "longest")
        n = ctypes.c_size_t(0)
        calls = (lambda: lib.tsx_hip_query_reads_device(m.handle, None, 0, 1, U64, None, 0, ctypes.byref(n), None),
                 lambda: lib.tsx_hip_trim_spans_device(m.handle, None, 0, ctypes.byref(rule), None, 0, ctypes.byref(n), None),
                 lambda: lib.tsx_hip_median_reads_device(m.handle, None, 0, None, 0, ctypes.byref(n), None))
        for call in calls:
            assert m.queryReadsDevice(dev.data_ptr(), len(TEXT), dst.data_ptr(), len(RECS)) == len(RECS)
            n.value = 77
            assert call() == T.OK
            assert n.value == 0
    finally:
        m.close()
