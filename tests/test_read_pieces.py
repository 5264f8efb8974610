"""What the read calls share: the host piece driver at piece sizes below, at and just above one record (trim and
medians; test_read_query.py has the query's), the TSX_HIP_PIECE_BYTES cap that only the median calls honour, and the
device window walk over an empty text after a call that left a scan carry behind.

Expectations come from the Python restatements of test_read_query.py, test_trim.py, test_median_cpu.py and
test_pairs.py over coded_counts of the counted text.  Never from the library under test.  Everything is compared
exactly."""
import ctypes
import random

import numpy as np
import pytest

from test_median import filter_out, pairs, to_device
from test_median_cpu import expected_median_filter, expected_medians
from test_pairs import filter_mates, pair_model, run_pairs, trim_mates
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
