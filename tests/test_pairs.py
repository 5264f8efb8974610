"""Paired reads kept in step: tsx_hip_filter_pairs_host / tsx_hip_trim_pairs_host through Python and the tsxCount CLI.

Expectations come from a CPU model built here on the restatements of the single-end tests (coded_counts, expected_stats,
records of test_read_query; expected_trim of test_trim): the verdict of every mate, then the pair rules of
include/tsxcount_hip.h.  Never from the library under test.  Outputs and totals are compared exactly."""
import ctypes
import gzip
import os
import random

import pytest

from conftest import GOLDEN
from test_read_query import U64, coded_counts, expected_stats, line_spans, records, run_cli
from test_trim import expected_trim
import test_trim as TT

pytestmark = pytest.mark.gpu

K, L = 14, 18
_rnd = random.Random(7741)
GENOME = bytes(_rnd.choice(b"ACGT") for _ in range(4000))
COUNTED = b">g\n" + GENOME + b"\n"
COUNTS = coded_counts(COUNTED, K, 2)
TOT_KEYS = ("pairs", "kept", "single1", "single2", "bytes1", "bytes2", "bytes_single1", "bytes_single2", "bases_in", "bases_kept")


def sub(read, positions):
    r = bytearray(read)
    for p in positions:
        r[p] = b"CGTA"[b"ACGT".index(r[p])]
    return bytes(r)


def mate_seqs(rnd, n=300):
    """[(mate 1, mate 2)]: about 50 and about 140 bases of the genome, with substitutions planted so that every
    combination of clean / cut / destroyed mates occurs; two pairs of random bases (no solid window on either side)."""
    out = []
    for i in range(n):
        la, lb = rnd.randint(45, 55), rnd.randint(130, 150)
        at = rnd.randrange(0, len(GENOME) - 200)
        a, b = GENOME[at:at + la], GENOME[at + 40:at + 40 + lb]
        ka, kb = rnd.choice("ccccem"), rnd.choice("ccccemr")
        if ka == "e":
            a = sub(a, [3 if i % 2 else la - 4])   # cut near an end: most of it stays (the prefix mode keeps the second kind)
        elif ka == "m":
            a = sub(a, [la // 2])        # cut in the middle: both halves shorter than 30
        if kb == "e":
            b = sub(b, [lb - 5])
        elif kb == "m":
            b = sub(b, [60])
        elif kb == "r":
            b = bytes(rnd.choice(b"ACGT") for _ in range(lb))
        if i in (17, 203):
            a = bytes(rnd.choice(b"ACGT") for _ in range(la))
            b = bytes(rnd.choice(b"ACGT") for _ in range(lb))
        out.append((a, b))
    return out


def mate_texts(pairs, lpr, long_a=(), long_b=()):
    """Two texts with names p<i>/1 and p<i>/2 and different comments; a long comment on the A records of long_a (so that
    some rounds are limited by A), a long read for the B records of long_b."""
    ta, tb = [], []
    for i, (a, b) in enumerate(pairs):
        ca = b" " + b"c" * 700 if i in long_a else b" first:%d" % i
        if i in long_b:
            b = (b * 6)[:800]
        if lpr == 4:
            ta.append(b"@p%d/1%s\n%s\n+\n%s\n" % (i, ca, a, b"I" * len(a)))
            tb.append(b"@p%d/2\tsecond\n%s\n+p%d\n%s\n" % (i, b, i, b"J" * len(b)))
        else:
            ta.append(b">p%d/1%s\n%s\n" % (i, ca, a))
            tb.append(b">p%d/2\tsecond\n%s\n" % (i, b))
    return ta, tb


# ---- the model -------------------------------------------------------------------------------------------------------

def filter_mates(text, lpr, counts=COUNTS, k=K, lower=1, upper=U64, min_in=0, fraction=1.0, invert=False, canonical=False):
    """[(verdict, bytes as the filter writes the record)] of every record."""
    st = expected_stats(text, counts, k, lpr, lower, upper, canonical)
    ppm = int(round(fraction * 1e6))
    return [((inr >= min_in and inr * 1000000 >= ppm * km) != invert, rb) for (km, inr, _, _), (_, rb) in zip(st, records(text, lpr))]


def trim_mates(text, lpr, counts=COUNTS, k=K, **kw):
    """[(survives, bytes as the trim writes the record, bases in, bases kept)] of every record."""
    out = []
    for _, rb in records(text, lpr):
        _, data, tot = expected_trim(rb, counts, k, lpr, **kw)
        out.append((tot["kept"] == 1, data, tot["bases_in"], tot["bases_kept"]))
    return out


def pair_model(ma, mb, mode="both", singles=(True, True), trim=False):
    """(out1, out2, single1, single2, totals) from the mates' verdicts; ma / mb as filter_mates or trim_mates give them."""
    assert len(ma) == len(mb)
    o = [b"", b"", b"", b""]
    t = dict.fromkeys(TOT_KEYS, 0)
    t["pairs"] = len(ma)
    for a, b in zip(ma, mb):
        va, vb = a[0], b[0]
        keep = (va or vb) if mode == "any" else (va and vb)
        if keep:
            o[0] += a[1]; o[1] += b[1]; t["kept"] += 1
        elif va:
            o[2] += a[1]; t["single1"] += 1
        elif vb:
            o[3] += b[1]; t["single2"] += 1
        if trim:
            t["bases_in"] += a[2] + b[2]
            t["bases_kept"] += (a[3] if va else 0) + (b[3] if vb else 0)
    if not singles[0]:
        o[2] = b""
    if not singles[1]:
        o[3] = b""
    t["bytes1"], t["bytes2"], t["bytes_single1"], t["bytes_single2"] = (len(x) for x in o)
    return o[0], o[1], o[2], o[3], t


def rounds_model(ta, tb, chunk):
    """Which text limits each round when two lists of records are taken chunk bytes at a time: a list of 'A', 'B', '='."""
    out, ia, ib = [], 0, 0

    def whole(recs, i, chunk):
        n, used, room = 0, 0, chunk
        total = sum(len(r) for r in recs[i:])
        while True:
            n, used = 0, 0
            for r in recs[i:]:
                if used + len(r) > room:
                    break
                used += len(r); n += 1
            if n or room >= total:
                return n if room < total else len(recs) - i
            room = min(2 * room, total)
    while ia < len(ta) or ib < len(tb):
        ra, rb = whole(ta, ia, chunk), whole(tb, ib, chunk)
        r = min(ra, rb)
        assert r > 0
        out.append("A" if ra < rb else "B" if rb < ra else "=")
        ia += r; ib += r
    return out


# ---- fixtures --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def new_map(T, k=K, l=L, counted=COUNTED, **kw):
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


PAIRS = mate_seqs(random.Random(99))
LONG_A, LONG_B = (40, 41, 42, 150, 151), (77,)
TEXTS = {lpr: mate_texts(PAIRS, lpr, LONG_A, LONG_B) for lpr in (4, 2)}
_MODEL_CACHE = {}


def mates_of(kind, lpr, **kw):
    """The model's mates of TEXTS[lpr], computed once per rule."""
    key = (kind, lpr, tuple(sorted(kw.items())))
    if key not in _MODEL_CACHE:
        fn = trim_mates if kind == "trim" else filter_mates
        _MODEL_CACHE[key] = tuple(fn(b"".join(t), lpr, **kw) for t in TEXTS[lpr])
    return _MODEL_CACHE[key]


def run_pairs(m, kind, a, b, tmp_path, singles=(True, True), tag="o", **kw):
    """(out1, out2, single1, single2, totals) of a call; b = None: interleaved."""
    p = [str(tmp_path / ("%s%d" % (tag, i))) for i in range(4)]
    for f in p:
        if os.path.exists(f):
            os.remove(f)
    call = m.trimPairs if kind == "trim" else m.filterPairs
    tot = call(a, b, p[0], p[1] if b is not None else None,
               singles=(p[2] if singles[0] else None, p[3] if singles[1] and b is not None else None), **kw)
    return tuple(open(f, "rb").read() if os.path.exists(f) else b"" for f in p) + (tot,)


# ---- 1, 2: the two forms against the model ---------------------------------------------------------------------------

@pytest.mark.parametrize("lpr", [4, 2])
def test_filter_two_files(T, gmap, lpr, tmp_path):
    gmap.set_record_lines(lpr)
    a, b = (b"".join(t) for t in TEXTS[lpr])
    for invert in (False, True):
        ma, mb = mates_of("filter", lpr, invert=invert)
        va, vb = [x[0] for x in ma], [x[0] for x in mb]
        both = list(zip(va, vb))
        assert (True, True) in both and (True, False) in both and (False, True) in both and (False, False) in both
        for mode in ("both", "any"):
            for singles in ((True, True), (False, False), (True, False)):
                want = pair_model(ma, mb, mode, singles)
                got = run_pairs(gmap, "filter", a, b, tmp_path, singles, pairs=mode, lower=1, invert=invert, check_names=True)
                assert got == want, (lpr, invert, mode, singles)
                if mode == "any":
                    assert want[4]["single1"] == want[4]["single2"] == 0 and want[4]["kept"] > pair_model(ma, mb)[4]["kept"]


@pytest.mark.parametrize("lpr", [4, 2])
def test_trim_two_files(T, gmap, lpr, tmp_path):
    gmap.set_record_lines(lpr)
    a, b = (b"".join(t) for t in TEXTS[lpr])
    for mode in ("longest", "prefix"):
        ma, mb = mates_of("trim", lpr, mode=mode, min_len=30)
        cut = lambda x: x[0] and x[3] < x[2]
        assert any(cut(x) and cut(y) for x, y in zip(ma, mb)), "a pair with both mates cut"
        assert any(not x[0] and y[0] for x, y in zip(ma, mb)), "an orphan of B"
        assert any(x[0] and not y[0] for x, y in zip(ma, mb)), "an orphan of A"
        assert not ma[17][0] and not mb[17][0] and ma[17][1] == b"" and mb[17][1] == b""   # no solid window on either side
        want = pair_model(ma, mb, trim=True)
        assert want[4]["kept"] and want[4]["single1"] and want[4]["single2"]
        got = run_pairs(gmap, "trim", a, b, tmp_path, lower=1, mode=mode, min_len=30)
        assert got == want, (lpr, mode)
    ma, mb = mates_of("trim", lpr, mode="longest", min_len=30)
    assert any(not x[0] and expected_trim(records(a, lpr)[i][1], COUNTS, K, lpr)[2]["bases_kept"] > 0 and mb[i][0]
               for i, x in enumerate(ma)), "a mate below min_len makes its partner an orphan"
    got = run_pairs(gmap, "trim", a, b, tmp_path, (False, True), lower=1, min_len=30)
    assert got == pair_model(ma, mb, singles=(False, True), trim=True)


# ---- 3: pieces -------------------------------------------------------------------------------------------------------

def test_pieces_equal_one_piece(T, gmap, tmp_path, monkeypatch):
    gmap.set_record_lines(4)
    ta, tb = TEXTS[4]
    a, b = b"".join(ta), b"".join(tb)
    limits = rounds_model(ta, tb, 600)
    assert "A" in limits and "B" in limits, limits
    assert len(tb[77]) > 600 and max(len(r) for r in ta) > 600 > len(ta[0])   # pieces of either text grow on their own
    small = len(tb[0]) - 1
    fw = pair_model(*mates_of("filter", 4, invert=False))
    tw = pair_model(*mates_of("trim", 4, mode="longest", min_len=30), trim=True)
    for chunk in (small, 600, 4096, 0):
        assert run_pairs(gmap, "filter", a, b, tmp_path, pairs="both", lower=1, chunk_bytes=chunk, check_names=True) == fw, chunk
        assert run_pairs(gmap, "trim", a, b, tmp_path, lower=1, min_len=30, chunk_bytes=chunk, check_names=True) == tw, chunk
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "1024")   # read when the map is created: the table is counted in pieces
    m = new_map(T)
    monkeypatch.delenv("TSX_HIP_PIECE_BYTES")
    m.set_record_lines(4)
    assert run_pairs(m, "filter", a, b, tmp_path, pairs="both", lower=1, chunk_bytes=600) == fw
    assert run_pairs(m, "trim", a, b, tmp_path, lower=1, min_len=30, chunk_bytes=600) == tw
    m.close()


# ---- 4: interleaved --------------------------------------------------------------------------------------------------

def interleaved(x, y):
    return b"".join(p + q for p, q in zip(x, y))


@pytest.mark.parametrize("lpr", [4, 2])
def test_interleaved(T, gmap, lpr, tmp_path):
    gmap.set_record_lines(lpr)
    ta, tb = TEXTS[lpr]
    text = interleaved(ta, tb)
    for kind, kw, mk in (("filter", dict(pairs="both", lower=1), dict(invert=False)),
                         ("filter", dict(pairs="any", lower=1), dict(invert=False)),
                         ("trim", dict(lower=1, min_len=30), dict(mode="longest", min_len=30))):
        ma, mb = mates_of(kind, lpr, **mk)
        mode = kw.get("pairs", "both")
        o1, o2, s1, s2, t = pair_model(ma, mb, mode, trim=kind == "trim")
        keep = [((x[0] or y[0]) if mode == "any" else (x[0] and y[0])) for x, y in zip(ma, mb)]
        want_kept = b"".join(x[1] + y[1] for x, y, kp in zip(ma, mb, keep) if kp)
        want_single = b"".join((x[1] if x[0] else y[1]) for x, y, kp in zip(ma, mb, keep) if not kp and (x[0] != y[0]))
        assert len(want_kept) == len(o1) + len(o2) and len(want_single) == len(s1) + len(s2)
        want_t = dict(t, bytes1=len(want_kept), bytes2=0, bytes_single1=len(want_single), bytes_single2=0)
        # 0: one piece; 777 and 1500: odd piece cuts (an A record and a B record differ in length, pieces end anywhere)
        for chunk in (0, 777, 1500):
            got = run_pairs(gmap, kind, text, None, tmp_path, chunk_bytes=chunk, check_names=True, **kw)
            assert got == (want_kept, b"", want_single, b"", want_t), (kind, kw, chunk)
    got = run_pairs(gmap, "filter", text, None, tmp_path, (False, False), pairs="both", lower=1)
    assert got[2] == b"" and got[4]["bytes_single1"] == 0 and got[4]["single1"] > 0


# ---- 5: the line rules, per mate -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def map21(T):
    m = TT.genome_map(T)
    yield m
    m.close()


@pytest.mark.parametrize("name", ["whole", "unterminated", "incomplete", "header_only"])
def test_line_rules_per_mate(T, map21, name, tmp_path):
    odd = TT._line_texts()[name]
    n = len(records(odd, 4))
    reads = [TT.GENOME[900 + 100 * i:1000 + 100 * i] for i in range(n)]
    reads[1] = TT.sub(reads[1], [50])
    good = TT.fastq(reads)
    map21.set_record_lines(4)
    kw = dict(counts=TT.COUNTS, k=TT.K)
    for a, b in ((odd, good), (good, odd), (odd, odd)):
        fa, fb = filter_mates(a, 4, **kw), filter_mates(b, 4, **kw)
        ra, rb = trim_mates(a, 4, **kw), trim_mates(b, 4, **kw)
        for chunk in (0, 150):
            for mode in ("both", "any"):
                got = run_pairs(map21, "filter", a, b, tmp_path, pairs=mode, lower=1, chunk_bytes=chunk)
                assert got == pair_model(fa, fb, mode), (name, chunk, mode)
            assert run_pairs(map21, "trim", a, b, tmp_path, lower=1, chunk_bytes=chunk) == pair_model(ra, rb, trim=True), (name, chunk)
    if name == "unterminated":   # the '\n' the text lacks is added where the last record is written
        got = run_pairs(map21, "filter", odd, good, tmp_path, pairs="any", lower=1, chunk_bytes=150)
        assert got[0].endswith(b"M" * 90 + b"\n") and not odd.endswith(b"\n")


# ---- 6: errors -------------------------------------------------------------------------------------------------------

def expect_epair(T, call):
    with pytest.raises(T.TSXException) as e:
        call()
    assert e.value.code == T.EPAIR
    return str(e.value)


def test_texts_out_of_step(T, gmap, tmp_path):
    gmap.set_record_lines(4)
    ta, tb = TEXTS[4]
    a, b = b"".join(ta), b"".join(tb)
    for kind, kw in (("filter", dict(pairs="both", lower=1)), ("trim", dict(lower=1, min_len=30))):
        for chunk in (0, 4096):
            expect_epair(T, lambda: run_pairs(gmap, kind, a, b"".join(tb[:-1]), tmp_path, chunk_bytes=chunk, **kw))
            expect_epair(T, lambda: run_pairs(gmap, kind, b"".join(ta[:-1]), b, tmp_path, chunk_bytes=chunk, **kw))
            expect_epair(T, lambda: run_pairs(gmap, kind, interleaved(ta, tb) + ta[0], None, tmp_path, chunk_bytes=chunk, **kw))
        # on failure the outputs hold whole pairs of the pieces before: a prefix of the right answer, the same pairs in both
        ma, mb = mates_of(kind, 4, **(dict(invert=False) if kind == "filter" else dict(mode="longest", min_len=30)))
        full = pair_model(ma, mb, trim=kind == "trim")
        p = [str(tmp_path / ("e%d" % i)) for i in range(4)]
        call = gmap.trimPairs if kind == "trim" else gmap.filterPairs
        expect_epair(T, lambda: call(a, b"".join(tb[:-1]), p[0], p[1], singles=(p[2], p[3]), chunk_bytes=4096, **kw))
        o1, o2 = open(p[0], "rb").read(), open(p[1], "rb").read()
        assert full[0].startswith(o1) and full[1].startswith(o2) and len(o1) < len(full[0])
        assert len(line_spans(o1)) == len(line_spans(o2))
        # trailing empty lines only in the longer text are no record
        assert run_pairs(gmap, kind, a + b"\n\n\n", b, tmp_path, chunk_bytes=4096, **kw) == full
        assert run_pairs(gmap, kind, a, b + b"\n" * 5000, tmp_path, chunk_bytes=4096, **kw) == full


def test_name_check(T, gmap, tmp_path):
    gmap.set_record_lines(4)
    ta, tb = TEXTS[4]
    a = b"".join(ta)
    swapped = list(tb)
    swapped[281], swapped[282] = swapped[282], swapped[281]
    bad = b"".join(swapped)
    for kind, kw in (("filter", dict(pairs="both", lower=1)), ("trim", dict(lower=1, min_len=30))):
        for chunk in (0, 4096):
            msg = expect_epair(T, lambda: run_pairs(gmap, kind, a, bad, tmp_path, chunk_bytes=chunk, check_names=True, **kw))
            assert "pair 281" in msg, msg
            msg = expect_epair(T, lambda: run_pairs(gmap, kind, interleaved(ta, swapped), None, tmp_path, chunk_bytes=chunk,
                                                    check_names=True, **kw))
            assert "pair 281" in msg, msg
        # not looked at without check_names: the swapped records are simply mates
        got = run_pairs(gmap, kind, a, bad, tmp_path, chunk_bytes=4096, **kw)
        if kind == "filter":
            want = pair_model(filter_mates(a, 4), filter_mates(bad, 4))
        else:
            want = pair_model(trim_mates(a, 4, min_len=30), trim_mates(bad, 4, min_len=30), trim=True)
        assert got == want
    # names are compared whole: a differing suffix other than /1 /2 fails, a bare name passes
    x = b"@q/1\n" + GENOME[:50] + b"\n+\n" + b"I" * 50 + b"\n"
    for hdr, ok in ((b"@q/2", True), (b"@q", True), (b"@q/2 c/1", True), (b"@q/3", False), (b"@qq/2", False), (b"@Q/2", False)):
        y = hdr + b"\n" + GENOME[60:160] + b"\n+\n" + b"I" * 100 + b"\n"
        assert T.pair_name(hdr) == (b"q" if ok else T.pair_name(hdr))
        if ok:
            assert run_pairs(gmap, "filter", x, y, tmp_path, lower=1, check_names=True)[4]["kept"] == 1
        else:
            assert "pair 0" in expect_epair(T, lambda: run_pairs(gmap, "filter", x, y, tmp_path, lower=1, check_names=True))


def test_each_bad_argument_alone_is_refused(T, gmap, tmp_path):
    from test_pairs_cpu import TEXT, check_with_map
    L = T.lib()
    fds = [os.open(str(tmp_path / ("fd%d" % i)), os.O_WRONLY | os.O_CREAT, 0o644) for i in range(4)]
    tot = T.PairTotals()

    def filt(h, t2, n2, rule, mode, io):
        return L.tsx_hip_filter_pairs_host(h, TEXT, len(TEXT), t2, n2, ctypes.byref(rule) if rule else None, mode, 0,
                                           ctypes.byref(io) if io else None, 0, ctypes.byref(tot))

    def trim(h, t2, n2, rule, io):
        return L.tsx_hip_trim_pairs_host(h, TEXT, len(TEXT), t2, n2, ctypes.byref(rule) if rule else None, 0,
                                         ctypes.byref(io) if io else None, 0, ctypes.byref(tot))
    try:
        gmap.set_record_lines(4)
        two, one = T.PairIO(fds[0], fds[1], -1, -1), T.PairIO(fds[0], -1, -1, -1)
        assert filt(gmap.handle, TEXT, len(TEXT), T.filter_rule(1), 0, two) == T.OK and tot.pairs == 1   # the good call
        assert trim(gmap.handle, TEXT, len(TEXT), T.trim_rule(1), two) == T.OK
        check_with_map(T, gmap.handle, filt, trim, two, one)
        shard = T.TSXHashMapHIP(18, 0, K, shard_bits=1, shard_index=0)
        assert filt(shard.handle, TEXT, len(TEXT), T.filter_rule(1), 0, two) == T.EINVAL
        assert trim(shard.handle, TEXT, len(TEXT), T.trim_rule(1), two) == T.EINVAL
        shard.close()
    finally:
        for fd in fds:
            os.close(fd)


# ---- 7: against the single-end calls ---------------------------------------------------------------------------------

def by_index(*outs, lpr=4):
    recs = [rb for o in outs for _, rb in records(o, lpr)]
    return sorted(recs, key=lambda rb: int(rb[2:rb.index(b"/")]))


def test_cross_check_with_single_end(T, gmap, tmp_path):
    gmap.set_record_lines(4)
    a, b = (b"".join(t) for t in TEXTS[4])
    for kind, kw, single in (("filter", dict(lower=1), gmap.filterReads), ("trim", dict(lower=1, min_len=30), gmap.trimReads)):
        o1, o2, s1, s2, _ = run_pairs(gmap, kind, a, b, tmp_path, chunk_bytes=4096, **kw)
        for text, kept, orphans in ((a, o1, s1), (b, o2, s2)):
            single(text, str(tmp_path / "se"), **kw)
            want = open(str(tmp_path / "se"), "rb").read()
            assert b"".join(by_index(kept, orphans)) == want and len(orphans) > 0
    a1, a2, _, _, t_any = run_pairs(gmap, "filter", a, b, tmp_path, pairs="any", lower=1)
    b1, b2, _, _, t_both = run_pairs(gmap, "filter", a, b, tmp_path, pairs="both", lower=1)
    assert set(records(b1, 4)) < set(records(a1, 4)) and set(records(b2, 4)) < set(records(a2, 4))
    assert t_any["kept"] == t_both["kept"] + t_both["single1"] + t_both["single2"]


# ---- 8: a canonical table, a base rule -------------------------------------------------------------------------------

def test_canonical_table_and_base_rule(T, tmp_path):
    ta, tb = mate_texts(PAIRS[:60], 4)
    tb = [b"@p%d/2\n%s\n+\n%s\n" % (i, TT.rc(p[1]), b"J" * len(p[1])) for i, p in enumerate(PAIRS[:60])]   # mate 2 from the other strand
    a, b = b"".join(ta), b"".join(tb)
    counts = coded_counts(COUNTED, K, 2, canonical=True)
    m = new_map(T, canonical=True)
    m.set_record_lines(4)
    want = pair_model(trim_mates(a, 4, counts=counts, canonical=True, min_len=30), trim_mates(b, 4, counts=counts, canonical=True, min_len=30),
                      trim=True)
    assert want[4]["kept"] > 10
    assert run_pairs(m, "trim", a, b, tmp_path, lower=1, min_len=30, chunk_bytes=2000) == want
    m.close()
    withn = [(p[0][:20] + b"N" + p[0][21:], p[1]) if i % 3 == 0 else p for i, p in enumerate(PAIRS[:60])]
    ta, tb = mate_texts(withn, 4)
    a, b = b"".join(ta), b"".join(tb)
    m = new_map(T, acgt_only=True)
    m.set_record_lines(4)
    want = pair_model(trim_mates(a, 4, acgt_only=True, min_len=30), trim_mates(b, 4, acgt_only=True, min_len=30), trim=True)
    loose = pair_model(trim_mates(a, 4, min_len=30), trim_mates(b, 4, min_len=30), trim=True)
    assert want[4] != loose[4]   # the rule decides: N takes the code of A and would be solid where the genome has A
    assert run_pairs(m, "trim", a, b, tmp_path, lower=1, min_len=30, chunk_bytes=2000) == want
    m.close()


# ---- 9: owners -------------------------------------------------------------------------------------------------------

def test_calls_leave_the_owner_counters(T, gmap, tmp_path):
    L = T.lib()
    L.tsx_hip_debug_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]

    def counters():
        out = (ctypes.c_uint64 * 8)()
        assert L.tsx_hip_debug_counters(gmap.handle, out) == 0
        return tuple(int(x) for x in out[:3])

    gmap.set_record_lines(4)
    ta, tb = TEXTS[4]
    a, b, short = b"".join(ta), b"".join(tb), b"".join(tb[:-1])

    def one_pass():
        for kind, kw in (("filter", dict(pairs="both", lower=1)), ("trim", dict(lower=1, min_len=30))):
            run_pairs(gmap, kind, a, b, tmp_path, chunk_bytes=3000, check_names=True, **kw)
            run_pairs(gmap, kind, interleaved(ta, tb), None, tmp_path, chunk_bytes=3000, **kw)
            expect_epair(T, lambda: run_pairs(gmap, kind, a, short, tmp_path, chunk_bytes=3000, **kw))
            expect_epair(T, lambda: run_pairs(gmap, kind, interleaved(ta, tb) + ta[0], None, tmp_path, chunk_bytes=3000, **kw))

    one_pass()   # warm-up: the map's grow-only line scratch grows here
    warm = counters()
    one_pass()
    assert counters() == warm


# ---- 10: the CLI -----------------------------------------------------------------------------------------------------

def test_golden_cli_pairs(T, tmp_path):
    inp = os.path.join(GOLDEN, "small_t7.1000.fastq")
    text = open(inp, "rb").read()
    recs = [rb for _, rb in records(text, 4)]

    def renamed(rb, i, mate):
        head, rest = rb.split(b"\n", 1)
        return b"@frag%d/%d %s\n" % (i, mate, head[1:]) + rest
    r1 = b"".join(renamed(rb, i // 2, 1) for i, rb in enumerate(recs) if i % 2 == 0)
    r2 = b"".join(renamed(rb, i // 2, 2) for i, rb in enumerate(recs) if i % 2 == 1)
    f1, f2 = tmp_path / "R1.fastq", tmp_path / "R2.fastq.gz"
    f1.write_bytes(r1)
    with gzip.open(str(f2), "wb") as f:
        f.write(r2)
    m = T.TSXHashMapHIP(20, 0, 14)
    m.set_path(1)
    m.countFastq(text)
    names = ["O1", "O2", "S1", "S2"]
    want_f = run_pairs(m, "filter", r1, r2, tmp_path, tag="pf", lower=2, check_names=True)
    want_t = run_pairs(m, "trim", r1, r2, tmp_path, tag="pt", lower=2, check_names=True)
    m.close()
    assert 0 < want_f[4]["kept"] < want_f[4]["pairs"] and want_f[4]["single1"] and want_f[4]["single2"]
    o = [str(tmp_path / ("f" + n)) for n in names]
    code, so, se = run_cli("--input=" + inp, "--k=14", "--l=20", "--filter-input=%s,%s" % (f1, f2), "--filter=%s,%s" % (o[0], o[1]),
                           "--filter-singles=%s,%s" % (o[2], o[3]), "--pair-names")
    assert code == 0, so + se
    assert tuple(open(f, "rb").read() for f in o) == want_f[:4]
    t = want_f[4]
    assert [ln for ln in so.splitlines() if ln.startswith("pairs\t")] == \
        ["pairs\t%d\t%d\t%d\t%d" % (t["pairs"], t["kept"], t["single1"], t["single2"])]
    o = [str(tmp_path / ("t" + n)) for n in names]
    code, so, se = run_cli("--input=" + inp, "--k=14", "--l=20", "--trim-input=%s,%s" % (f1, f2), "--trim=%s,%s" % (o[0], o[1]),
                           "--trim-singles=%s,%s" % (o[2], o[3]), "--pair-names")
    assert code == 0, so + se
    assert tuple(open(f, "rb").read() for f in o) == want_t[:4]
    t = want_t[4]
    assert [ln for ln in so.splitlines() if ln.startswith("pairs\t")] == \
        ["pairs\t%d\t%d\t%d\t%d\t%d\t%d" % (t["pairs"], t["kept"], t["single1"], t["single2"], t["bases_in"], t["bases_kept"])]
    # out of step: the library's text, a non-zero exit
    f3 = tmp_path / "R2short.fastq"
    f3.write_bytes(b"".join(renamed(rb, i // 2, 2) for i, rb in enumerate(recs[:-2]) if i % 2 == 1))
    code, so, se = run_cli("--input=" + inp, "--k=14", "--l=20", "--filter-input=%s,%s" % (f1, f3), "--filter=%s,%s" % (o[0], o[1]))
    assert code != 0 and "text 2 ends after" in se, so + se
