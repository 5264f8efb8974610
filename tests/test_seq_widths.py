"""Sequence queries on the GPU at every piece cut, key width and at the fragment bound: querySequences /
missingIntervals and their BGZF and device forms against sequence_stats / missing_intervals / fasta_records
(tsxcount_amd, CPU) over conftest.python_counts of the table text.  Names, the five integer columns and the interval
triples match exactly; the piecewise = one-piece identities are asserted on top of the reference, never in its place.

The inputs are those of tests/seq_design.py; tests/test_seq_widths_cpu.py shows on the reference alone that they hold
the scenarios, that a key cut short answers otherwise on them and that the fragment bound is reached and not passed."""
import pytest

import seq_design as S
import width_design as W
from conftest import python_counts
from test_seq import check, filled
from test_width_matrix import new_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def rows_of(a):
    return [tuple(int(v) for v in r) for r in a]


def counts_of(T, table, k):
    return python_counts(T.join_fasta(table), k, 2)


# ---- 1. every cut position -------------------------------------------------------------------------------------------------

SWEEP_PARTS = 4
SWEEPS = {"plain": {}, "range": dict(lower=2, upper=3), "canonical": dict(canonical=True)}
SWEEP_CASES = [(31, "plain"), (127, "plain"), (31, "range"), (31, "canonical")]


def sweep_ranges(n, parts):
    """1 .. n in `parts` consecutive ranges of about equal cost: chunk_bytes = c makes ceil(n / c) pieces, and a call
    costs about what six pieces cost before its first one."""
    cost = [6 - (-n // c) for c in range(1, n + 1)]
    total, out, lo, acc = sum(cost), [], 1, 0
    for c in range(1, n + 1):
        acc += cost[c - 1]
        if acc * parts >= total * (len(out) + 1) and len(out) < parts - 1:
            out.append((lo, c))
            lo = c + 1
    out.append((lo, n))
    assert out[0][0] == 1 and out[-1][1] == n and all(a[1] + 1 == b[0] for a, b in zip(out, out[1:])) and len(out) == parts
    return out


_sweep = {}


def sweep_case(T, k, mode):
    """(text, table, records, counts, reference stats and intervals): computed once per (k, mode), never changed."""
    if (k, mode) not in _sweep:
        text, table = S.cut_text(k)
        recs = T.fasta_records(text)
        D = counts_of(T, table, k)
        kw = SWEEPS[mode]
        _sweep[k, mode] = (text, table, recs, D, (T.sequence_stats(recs, D, k, **kw), T.missing_intervals(recs, D, k, **kw)))
    return _sweep[k, mode]


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
@pytest.mark.parametrize("k,mode", SWEEP_CASES, ids=["%d-%s" % c for c in SWEEP_CASES])
def test_every_cut_position(T, k, mode, part):
    """cut_text(k) in pieces of every size chunk_bytes = 1 .. len(text): the last piece sizes cut the text once, at every
    offset; the first give pieces shorter than k, whose carry of bases and of the pending name spans many pieces.  The
    library sets no lower limit on a piece, so the sweep starts at one byte.  The range is split over SWEEP_PARTS ids of
    about equal cost; together they leave out no value."""
    text, table, recs, D, want = sweep_case(T, k, mode)
    kw = SWEEPS[mode]
    lo, hi = sweep_ranges(len(text), SWEEP_PARTS)[part]
    m = filled(T, k, table, l=16, canonical=kw.get("canonical", False))
    try:
        assert check(T, m, text, recs, D, k, **kw) == want                        # one piece, against the reference
        names = [n for n, _ in recs]
        for c in range(lo, hi + 1):                                               # ascending: the first failure is the smallest c
            try:
                got_names, stats = m.querySequences(text, kw.get("lower", 1), kw.get("upper"), c)
                iv = rows_of(m.missingIntervals(text, kw.get("lower", 1), kw.get("upper"), c))
            except T.TSXException as e:
                pytest.fail("chunk_bytes=%d: %s" % (c, e))
            stats = rows_of(stats)
            if got_names != names:
                bad = [(i, g, w) for i, (g, w) in enumerate(zip(got_names, names)) if g != w]
                pytest.fail("chunk_bytes=%d: names differ: %d for %d, first %r" % (c, len(got_names), len(names), bad[:1]))
            if stats != want[0]:
                bad = [(i, names[i], g, w) for i, (g, w) in enumerate(zip(stats, want[0])) if g != w]
                pytest.fail("chunk_bytes=%d: rows differ: %d for %d, first (row, name, got, want) %r" % (c, len(stats), len(want[0]), bad[:1]))
            if iv != want[1]:
                bad = [x for x in zip(iv, want[1]) if x[0] != x[1]]
                pytest.fail("chunk_bytes=%d: intervals differ: %d for %d, first (got, want) %r" % (c, len(iv), len(want[1]), bad[:1]))
    finally:
        m.close()


# ---- 2. device windows and BGZF batches ------------------------------------------------------------------------------------

def test_device_windows_and_bgzf_cuts(T, monkeypatch):
    """cut_text(127) eight times over through device windows of 4096 bytes, and often enough to fill more than two BGZF
    batches of the smallest size (128 KiB, what TSX_HIP_BGZF_BATCH is clamped to) in members of 700 bytes: the window
    and batch borders cut the copies at other offsets each."""
    import torch
    k = 127
    one, table = S.cut_text(k)
    D = counts_of(T, table, k)
    m = filled(T, k, table, l=16)
    try:
        text = (one + b"\n") * 7 + one
        assert len(text) > 2 * 4096
        recs = T.fasta_records(text)
        monkeypatch.setenv("TSX_HIP_DEV_WINDOW", "4096")
        buf = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        names, stats, iv = m.querySequencesDevice(buf.data_ptr(), len(text), missing=True)
        assert names == [n for n, _ in recs]
        assert rows_of(stats) == T.sequence_stats(recs, D, k)
        assert rows_of(iv) == T.missing_intervals(recs, D, k)

        batch = 128 << 10
        big = (one + b"\n") * (2 * batch // (len(one) + 1) + 2)
        assert len(big) > 2 * batch
        recs = T.fasta_records(big)
        monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")                             # clamped to the minimum, 128 KiB
        z = T.bgzf_compress(big, level=1, block=700)
        names, stats = m.querySequencesBgzf(z)
        iv = m.missingIntervalsBgzf(z)
        assert names == [n for n, _ in recs]
        assert rows_of(stats) == T.sequence_stats(recs, D, k)
        assert rows_of(iv) == T.missing_intervals(recs, D, k)
    finally:
        m.close()


# ---- 3. sibling contigs at the rows of the width matrix -------------------------------------------------------------------

SIB_ROWS = W.rows("32-20-0", "31-20-16", "64-20-0", "65-20-0", "80-20-0", "96-18-2", "96-20-32", "97-20-0") + [
    W.Row(127, 20, 0, 4, 4, "WK 4, the widest key")]
RANGES = ((1, None), (2, 2), (5, 5))


def assert_design(T, sib, contigs, recs, D, k, canonical=False):
    """The literal expectations of seq_design.Siblings, on the reference answers the GPU has just been compared with."""
    for lo, up in RANGES:
        stats = T.sequence_stats(recs, D, k, lo, up, canonical)
        iv = T.missing_intervals(recs, D, k, lo, up, canonical)
        for r, c in enumerate(contigs):
            mine = [(s, e) for rr, s, e in iv if rr == r]
            n = len(c.seq) - k + 1
            if c.kind == "cross" and lo == 1:
                assert len(mine) == 1 and mine[0][1] - mine[0][0] == 2 * k - 1 and mine[0] == (c.p - k + 1, c.p + k)
                assert stats[r][2] == stats[r][1] - k == n - k
            elif c.kind in ("within2", "within5"):
                own = int(c.kind[-1])
                assert stats[r][3] == own and stats[r][2] == (n if lo == 1 else k if lo == own else 0)
                assert stats[r][4] == 7 * (n - k) + own * k


@pytest.mark.parametrize("r", SIB_ROWS, ids=[W.row_id(r) for r in SIB_ROWS])
def test_sibling_contigs(T, r):
    k = r.k
    sib = S.sibling_contigs(k)
    text = sib.query()
    recs = T.fasta_records(text)
    D = counts_of(T, sib.table, k)
    m = new_map(T, r)                                                             # (asserts the row's layout class)
    try:
        m.countFasta(sib.table)
        st = m.stats()
        assert st["insert_failures"] == 0 and st["overflow_failures"] == 0
        if r.s == 2:
            assert st["overflow_used"] > 0                                        # counts of 5 and 7 lie in the secondary array
        for lo, up in RANGES:
            check(T, m, text, recs, D, k, lower=lo, upper=up)
        check(T, m, text, recs, D, k, chunk_bytes=S.TILE)                         # and with the text cut at the planted border's size
    finally:
        m.close()
    assert_design(T, sib, sib.contigs(), recs, D, k)


# ---- 4. canonical tables ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [32, 65, 96, 127])
def test_sibling_contigs_canonical(T, k):
    sib = S.sibling_contigs(k)
    text = sib.query(canonical=True)
    recs = T.fasta_records(text)
    contigs = sib.contigs(canonical=True)
    assert any(c.name.endswith(b"_rc") for c in contigs) and (k % 2 == 1 or contigs[-1].kind == "pal")
    D = counts_of(T, sib.table_canonical, k)
    m = T.TSXHashMapHIP(20, 0, k, canonical=True)
    try:
        m.countFasta(sib.table_canonical)
        assert m.stats()["insert_failures"] == 0
        for lo, up in RANGES + ((3, 3),):
            stats, _ = check(T, m, text, recs, D, k, lower=lo, upper=up, canonical=True)
            if k % 2 == 0:                                                        # the palindrome: one key, seen three times
                assert stats[-1][1] == 3 and stats[-1][3] == 3 and stats[-1][2] == (3 if lo in (1, 3) else 0)
    finally:
        m.close()
    assert_design(T, sib, contigs, recs, D, k, canonical=True)


# ---- 5. the base rule, and the stand-in codes without it -------------------------------------------------------------------

@pytest.mark.parametrize("k", [63, 65, 127])
def test_base_rule_at_wide_keys(T, k):
    """Runs of N inside every pair's covering stretch (seq_design.with_n_runs).  A run of N lies over at least k window
    starts, so inside the k missing windows of a single substitution it can only cut the interval short; the 'double'
    contigs, 2k missing windows in a row, are the ones it splits in two.  The N of every contig lies k - 6 or more bases
    in, so the dropped windows hold it at offsets on both sides of 64: in either word of the break mask.  Without the
    rule N, lower case and an IUPAC code are looked up as their stand-in bases."""
    sib = S.sibling_contigs(k)
    text, table, contigs, doubles = S.with_n_runs(sib)
    recs = T.fasta_records(text)
    D = counts_of(T, table, k)
    kinds = [c[2] for c in contigs]
    for acgt_only in (True, False):
        m = filled(T, k, table, l=17, acgt_only=acgt_only)
        try:
            assert m.base_rule[0] == acgt_only
            stats, iv = check(T, m, text, recs, D, k, acgt_only=acgt_only)
            check(T, m, text, recs, D, k, lower=2, upper=5, acgt_only=acgt_only)
            check(T, m, text, recs, D, k, acgt_only=acgt_only, chunk_bytes=300)
        finally:
            m.close()
        if acgt_only:
            for i, r in enumerate(j for j, kind in enumerate(kinds) if kind == "cross"):
                p = sib.cross[i][2]
                assert [(s, e) for rr, s, e in iv if rr == r] == [(p - 3, p + k)]
                assert stats[r][1] < len(recs[r][1]) - k + 1
            for r, (_, p) in zip((j for j, kind in enumerate(kinds) if kind == "double"), doubles):
                assert [(s, e) for rr, s, e in iv if rr == r] == [(p - k + 1, p + 1), (p + 3, p + 2 * k)]
        else:
            assert all(s[1] == len(seq) - k + 1 for s, (_, seq) in zip(stats, recs))   # every window is a k-mer


# ---- 6. the fragment bound -------------------------------------------------------------------------------------------------

def test_fragment_bound_is_reached(T, monkeypatch):
    """Present and missing windows in turn: every whole tile emits SEQ_TILE_FRAGS = 2048 fragments (shown on the
    reference in test_seq_widths_cpu.py), the size of the buffer per tile, and no two of them merge."""
    k, n_tiles = 31, 3
    contig, kmers, counts = S.alternating(k, n_tiles)
    D = dict(zip(kmers, counts))
    text = S.fasta(b"alt", contig)
    recs = T.fasta_records(text)
    n = len(contig) - k + 1
    want_iv = T.missing_intervals(recs, D, k)
    assert want_iv == [(0, i, i + k) for i in range(1, n, 2)]
    assert S.fragments_per_tile(recs, D, k)[1:n_tiles + 1] == [S.TILE_FRAGS] * n_tiles
    m = T.TSXHashMapHIP(18, 0, k)
    try:
        m.addKmers(S.alternating_limbs(kmers, k), counts)
        assert m.stats()["insert_failures"] == 0
        assert rows_of(m.missingIntervals(text)) == want_iv                       # the default buffer
        assert rows_of(m.missingIntervals(text, chunk_bytes=S.TILE)) == want_iv   # the text cut every 4096 bytes
        monkeypatch.setenv("TSX_HIP_SEQ_FRAGS", "1")                              # one tile's worth per launch: the exact bound
        assert rows_of(m.missingIntervals(text)) == want_iv
        assert rows_of(m.missingIntervals(text, chunk_bytes=S.TILE)) == want_iv
        names, stats = m.querySequences(text)
        assert names == [b"alt"] and rows_of(stats) == T.sequence_stats(recs, D, k)
        assert int(stats[0]["kmers"]) == n and int(stats[0]["present"]) == (n + 1) // 2
    finally:
        m.close()


# ---- 7. the read query -----------------------------------------------------------------------------------------------------

def test_agrees_with_the_read_query(T):
    """The contigs of sibling_contigs(65) as FASTQ records through queryReads and as FASTA through querySequences, on one
    map: two kernels against each other and both against the reference."""
    k = 65
    sib = S.sibling_contigs(k)
    contigs = sib.contigs()
    text = sib.query()
    fastq = W.fastq_of([c.seq for c in contigs])
    recs = T.fasta_records(text)
    D = counts_of(T, sib.table, k)
    m = filled(T, k, sib.table, l=17)
    try:
        for lo, up in ((1, None), (2, 3)):
            want = T.sequence_stats(recs, D, k, lo, up)
            _, stats = m.querySequences(text, lo, up)
            reads = m.queryReads(fastq, lo, up)
            assert rows_of(stats) == want
            assert rows_of(reads) == [w[1:] for w in want]
            assert rows_of(reads) == [s[1:] for s in rows_of(stats)]
    finally:
        m.close()
