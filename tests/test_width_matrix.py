"""Every table and read feature at the key and slot widths of tests/width_design.py, on the GPU: three-limb keys with
slots narrower than, as wide as and wider than the key, a three-word slot under a four-limb key, a slot wider than a
one-limb key, and the full-limb k = 32 / 64 / 96.

Each case asserts its row's class against tsx_hip_get_layout before any feature call (new_map), runs on texts built
around sibling reads (k-mers that differ in exactly one base at every offset, on different sides or with different
multiplicities; tests/test_width_matrix_cpu.py shows that a truncated key gives other answers on them) and compares
whole results against the Python reference the feature's own test file uses -- dictionaries over the texts, never the
library under test.  The case ids carry k-l-s."""
import numpy as np
import pytest

import kmerdb
import width_design as D
from combine_ref import OPS, combine_expect
from conftest import python_counts

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def ids(rows):
    return [D.row_id(r) for r in rows]


def new_map(T, r, l=None, s=None, seed=5, text=None, **kw):
    """A map of the row's k (its l and s unless a case builds the 'other' table of a pair).  Of the row's own geometry:
    every field of tsx_hip_get_layout is the row's; of another: the key limbs still are."""
    m = T.TSXHashMapHIP(r.l if l is None else l, r.s if s is None else s, r.k, hash_seed=seed, **kw)
    assert m.layout.key_limbs == r.key_limbs == T.key_limbs(r.k)
    if s is None:
        lay = D.layout_of(r, l)
        for f, v in lay.fields().items():
            if not (f == "overflow_l" and kw.get("overflow_l")):
                assert getattr(m.layout, f) == v, (f, getattr(m.layout, f), v)
        assert m.layout.entry_limbs == r.W
    if text is not None:
        m.countFastq(text)
        st = m.stats()
        assert st["insert_failures"] == 0 and st["overflow_failures"] == 0
    return m


def table_dict(m):
    from test_combine import table_dict as td
    return td(m)


def close(*maps):
    for m in maps:
        m.close()


def pair_texts(r, canonical=False):
    """(text A, text B, dict A, dict B) of the row; canonical: folded, with the palindrome record when k is even."""
    tx = D.texts(r.k)
    ta, tb = tx.text_a, tx.text_b
    pal = None
    if canonical and r.k % 2 == 0:
        pal, rec = D.palindrome_record(r.k)
        ta, tb = ta + rec * 3, tb + rec
    da, db = dict(python_counts(ta, r.k)), dict(python_counts(tb, r.k))
    if canonical:
        da, db = kmerdb.fold_strands(da), kmerdb.fold_strands(db)
        if pal:
            assert da[pal] == 3 and db[pal] == 1
    return ta, tb, da, db


def three_tables(T, r, canonical=False):
    """A, B of A's geometry and seed (the aligned path), B of another seed and l (the general one)."""
    ta, tb, da, db = pair_texts(r, canonical)
    a = new_map(T, r, text=ta, canonical=canonical)
    b = new_map(T, r, text=tb, canonical=canonical)
    b2 = new_map(T, r, l=r.l - 1, seed=6, text=tb, canonical=canonical)
    assert table_dict(a) == da and table_dict(b) == db and table_dict(b2) == db
    if r.s == 2:
        assert a.stats()["overflow_used"] > 0 and b.stats()["overflow_used"] > 0     # counts of 4 and more carry
    return a, b, b2, da, db


# ---- combine -------------------------------------------------------------------------------------------------------------

COMBINE_ROWS = D.rows("65-20-0", "80-20-0", "96-18-2", "96-20-32", "97-20-0", "32-20-0", "64-20-0")
FULL_RULES = ("65-20-0", "96-18-2")          # every op and count mode, with and without ranges
CUT = dict(a_range=(2, 40), b_range=(1, 3))   # drops A's singletons and poly-A k-mers, B's counts of 4 and more


def short_rules():
    for op in OPS:
        for kw in ({}, CUT):
            yield op, "sum" if op in ("intersect", "union") else "min", kw


def run_combine(T, r, canonical, rules, monkeypatch):
    from test_combine import all_rules, check_result
    a, b, b2, da, db = three_tables(T, r, canonical)
    rules = list(all_rules()) if rules == "all" else list(short_rules())
    short = set((op, mode, tuple(sorted(kw))) for op, mode, kw in short_rules())
    outs = {}
    try:
        for op, mode, kw in rules:
            want, want_st = combine_expect(da, db, op, mode, **kw)
            if kw:
                assert want_st["a_in_range"] < len(da) and want_st["b_in_range"] < len(db)
            # (B, TSX_HIP_COMBINE_PATH, OUT's seed): aligned with OUT aligned, aligned with OUT elsewhere, the general
            # path forced on aligned tables, the general path by the tables
            forms = [(b, "2", None), (b2, "0", None)]
            if (op, mode, tuple(sorted(kw))) in short:
                forms += [(b, "2", 77), (b, "1", None)]
            for bb, path, out_seed in forms:
                monkeypatch.setenv("TSX_HIP_COMBINE_PATH", path)
                key = out_seed
                if key not in outs:
                    outs[key] = a.combine(bb, op, mode, hash_seed=out_seed, **kw)
                    assert outs[key].canonical == canonical and outs[key].layout.entry_limbs == r.W
                else:
                    outs[key].clear()
                    assert a.combine(bb, op, mode, out=outs[key], **kw) is outs[key]
                check_result(outs[key], want, want_st)
    finally:
        monkeypatch.delenv("TSX_HIP_COMBINE_PATH", raising=False)
        close(a, b, b2, *outs.values())


@pytest.mark.parametrize("r", COMBINE_ROWS, ids=ids(COMBINE_ROWS))
def test_combine(T, r, monkeypatch):
    run_combine(T, r, False, "all" if D.row_id(r) in FULL_RULES else "short", monkeypatch)


@pytest.mark.parametrize("r", D.rows("65-20-0", "96-20-32"), ids=["65-20-0", "96-20-32"])
def test_combine_canonical(T, r, monkeypatch):
    run_combine(T, r, True, "short", monkeypatch)


# ---- joint spectrum --------------------------------------------------------------------------------------------------------

def run_joint(T, r, canonical):
    a, b, b2, da, db = three_tables(T, r, canonical)
    try:
        for na, nb in ((1002, 1002), (3, 200), (65, 65), (4, 4)):
            want = T.joint_histogram(da, db, na, nb)
            for bb in (b, b2):
                got = a.jointHistogram(bb, na, nb)
                assert got.dtype == np.uint64 and np.array_equal(got, want), (na, nb, np.argwhere(got != want)[:5])
                assert np.array_equal(bb.jointHistogram(a, nb, na), want.T), (na, nb)
        m = T.joint_histogram(da, db, 1002, 1002)
        assert m[1:, 0].sum() and m[0, 1:].sum() and m[1:, 1:].sum()
        assert m[D.CROSS_A, 0] and m[0, D.CROSS_B] and m[D.CROSS_A, D.CROSS_B]     # the cross pairs: apart and together
        if r.s == 2:
            assert m[4:, :].sum() and m[:, 4:].sum()      # bins that only the secondary array's counts reach
    finally:
        close(a, b, b2)


@pytest.mark.parametrize("r", COMBINE_ROWS, ids=ids(COMBINE_ROWS))
def test_joint(T, r):
    run_joint(T, r, False)


@pytest.mark.parametrize("r", D.rows("96-18-2"), ids=["96-18-2"])
def test_joint_canonical(T, r):
    run_joint(T, r, True)


# ---- read binning ----------------------------------------------------------------------------------------------------------

BIN_ROWS = D.rows("65-20-0", "80-20-0", "96-18-2", "32-20-0", "64-20-0")
BIN_RULES = [dict(), dict(a_range=(2, None), b_range=(2, 4), min_hits=5, ratio_milli=1500)]


def bin_expect(tx, k, **rule):
    from test_bin_reads import counts_of, expected
    return expected(tx.query, counts_of(tx.text_a, k, 4), counts_of(tx.text_b, k, 4), k, 4, **rule)


def bin_kw(rule):
    return dict(a_range=rule.get("a_range", (1, None)), b_range=rule.get("b_range", (1, None)),
                min_hits=rule.get("min_hits", 1), ratio=rule.get("ratio_milli", 1000) / 1000)


@pytest.mark.parametrize("r", BIN_ROWS, ids=ids(BIN_ROWS))
def test_bin_reads(T, r):
    """B like A (one seed: one LUT, one hash) and B of another seed, l and storage bits (the re-hash form)."""
    from test_bin_reads import as_tuples
    tx = D.texts(r.k)
    a = new_map(T, r, text=tx.text_a)
    b_like = new_map(T, r, text=tx.text_b)
    b_other = new_map(T, r, l=r.l - 1, s=5, seed=977, overflow_l=12, text=tx.text_b)
    try:
        for rule in BIN_RULES:
            want_st, want_cls = bin_expect(tx, r.k, **rule)
            if not rule:
                assert len(set(want_cls)) == 4, "the default rule meets every class"
                assert any(0 < hb < ha for _, ha, hb, _ in want_st)       # a cross pair's R: fewer hits in B than in A
            for name, b in (("like A", b_like), ("other layout", b_other)):
                st, cls = a.binStats(b, tx.query, **bin_kw(rule))
                assert as_tuples(st) == want_st, (name, rule)
                assert cls.tolist() == want_cls, (name, rule)
    finally:
        close(a, b_like, b_other)


@pytest.mark.parametrize("r", D.rows("96-20-32"), ids=["96-20-32"])
def test_bin_reads_host_pieces(T, r):
    from test_bin_reads import as_tuples, records
    tx = D.texts(r.k)
    want_st, want_cls = bin_expect(tx, r.k)
    a = new_map(T, r, text=tx.text_a)
    b = new_map(T, r, l=r.l - 2, seed=4, text=tx.text_b)
    longest = max(len(rec) for _, _, rec in records(tx.query, 4))
    try:
        # pieces that end inside records, and pieces shorter than the longest record (they grow)
        for chunk in (0, 600, 4096, 4097, longest + 1):
            st, cls = a.binStats(b, tx.query, chunk_bytes=chunk)
            assert as_tuples(st) == want_st and cls.tolist() == want_cls, chunk
    finally:
        close(a, b)


# ---- read query and filter ---------------------------------------------------------------------------------------------------

QUERY_ROWS = D.rows("65-20-0", "80-20-0", "96-18-2")


@pytest.mark.parametrize("r", QUERY_ROWS, ids=ids(QUERY_ROWS))
def test_read_query_and_filter(T, r, tmp_path):
    from test_read_query import as_tuples, coded_counts, expected_filter, expected_stats
    k = r.k
    tx = D.texts(k)
    counts = coded_counts(tx.text_a, k, 4)
    m = new_map(T, r, text=tx.text_a)
    p = str(tmp_path / "kept.fq")
    try:
        for lower, upper in ((1, None), (2, 3), (4, None)):
            want = expected_stats(tx.query, counts, k, 4, lower, U64 if upper is None else upper)
            assert len({st[1] for st in want}) > 3
            for chunk in (0, 4099):
                assert as_tuples(m.queryReads(tx.query, lower, upper, chunk_bytes=chunk)) == want, (lower, chunk)
        # (lower, upper, min_in_range, fraction, invert): every k-mer seen twice; one k-mer in the table; the failures
        for lower, upper, mn, frac, inv in ((2, None, 0, 1.0, False), (1, None, 1, 0.0, False), (2, None, 0, 1.0, True),
                                            (3, 3, 40, 0.3, False)):
            st = expected_stats(tx.query, counts, k, 4, lower, U64 if upper is None else upper)
            kept, data = expected_filter(tx.query, st, 4, mn, int(round(frac * 1e6)), inv)
            assert 0 < kept < len(st)
            assert m.filterReads(tx.query, p, lower, upper, mn, frac, inv) == (kept, len(data))
            assert open(p, "rb").read() == data
    finally:
        m.close()


# ---- count output ------------------------------------------------------------------------------------------------------------

OUTPUT_ROWS = D.rows("32-20-0", "64-20-0", "65-20-0", "96-18-2", "97-20-0", "31-20-16", "96-20-32")


@pytest.mark.parametrize("r", OUTPUT_ROWS, ids=ids(OUTPUT_ROWS))
def test_count_output(T, r, tmp_path):
    from test_count_output import expected_hist, parse_count_text
    k = r.k
    tx = D.texts(k)
    text = tx.text_a + tx.sib_b
    want = dict(python_counts(text, k))
    m = new_map(T, r, text=text)
    out = tmp_path / "t.count"
    try:
        for nbins in (10002, 5, 2):
            assert np.array_equal(m.getCountHistogram(nbins), expected_hist(want.values(), nbins)), nbins
        n, nb = m.writeCounts(str(out))
        data = out.read_bytes()
        assert parse_count_text(data) == want and n == len(want) and nb == len(data)
        assert set(data.split(b"\n")[:-1]) == {x + b"\t%d" % c for x, c in want.items()}      # every line, k-mer text included
        for lo, hi in ((2, 3), (5, None)):
            m.writeCounts(str(out), lower=lo, upper=hi, chunk_bytes=64 * (k + 22))
            cut = {x: c for x, c in want.items() if lo <= c <= (U64 if hi is None else hi)}
            assert cut and parse_count_text(out.read_bytes()) == cut, (lo, hi)
    finally:
        m.close()


# ---- prefilter ---------------------------------------------------------------------------------------------------------------

PREFILTER_ROWS = D.rows("32-20-0", "64-20-0", "65-20-0", "96-18-2")


@pytest.mark.parametrize("r", PREFILTER_ROWS, ids=ids(PREFILTER_ROWS))
def test_prefilter(T, r):
    """Pass 1 against the numpy model, tsx_hip_prefilter_mask_host against the plain-integer one, and the armed count:
    the windows of B's own pairs that cover the substitution are seen once in R and four times in R'."""
    from test_prefilter import check_contract, check_filters, truth
    from test_prefilter_cpu import c_masks, masks_py
    k, bits = r.k, 24
    tx = D.texts(k)
    text = tx.text_b
    kept, enc, counts = truth(text, k)
    assert dict(kept) == dict(python_counts(text, k))
    once = [D.covering(a, p, k) for a, _, p in tx.within_b]
    again = [D.covering(b, p, k) for _, b, p in tx.within_b]
    assert all(kept[x] == 1 for c in once for x in c.values()) and all(kept[x] == 4 for c in again for x in c.values())
    # the host function on the sibling k-mers and a sample of the others
    sample = kmerdb.kmers_to_limbs([c[o] for c in once + again for o in range(k)], k)
    sample = np.concatenate([sample, enc[:: max(1, len(enc) // 200)]])
    wa, wb, mk = T.prefilter_masks(sample, k, bits)
    ca, cb, cm = c_masks(T, sample, k, bits)
    assert np.array_equal(wa, ca) and np.array_equal(wb, cb) and np.array_equal(mk, cm)
    for i in range(0, len(sample), 7):
        assert (int(wa[i]), int(wb[i]), int(mk[i])) == masks_py([int(x) for x in sample[i]], bits), i
    m = new_map(T, r)
    try:
        m.prefilter(text, bits=bits)
        check_filters(T, m, enc, counts, k, bits, int(counts.sum()))
        assert m.stats()["distinct"] == 0
        m.armPrefilter()
        m.countFastq(text)
        m.armPrefilter(False)
        ones, singles = check_contract(m, (enc, counts), int(counts.sum()), bits)
        assert singles > 3000 and ones <= singles // 100
        got = m.getKmerCounts(kmerdb.kmers_to_limbs([c[o] for c in again for o in range(k)], k))
        assert (got == 4).all()
    finally:
        m.close()


# ---- wrapped FASTA -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", D.rows("65-20-0", "96-18-2"), ids=["65-20-0", "96-18-2"])
def test_wrapped_fasta(T, r):
    from test_fasta_wrapped import check_table, expected, wrap
    k = r.k
    tx = D.texts(k)
    seqs = D.seqs_of(tx.text_a) + D.seqs_of(tx.sib_b)
    for width in (7, k - 1, k, k + 1, 2 * k + 40, 3 * k):      # below k, k, above it, a sibling read's length, beyond
        text = b"".join(b">r%d w%d\n" % (i, width) + wrap(s, width) for i, s in enumerate(seqs))
        want = expected(T, text, k)
        assert dict(want) == dict(python_counts(tx.text_a + tx.sib_b, k))       # the unwrapped reads' dictionary
        for path in (1, 2):
            m = new_map(T, r)
            m.set_path(path)
            m.countFasta(text)
            check_table(m, k, want)
            assert table_dict(m) == dict(want)
            m.close()


# ---- het pairs ---------------------------------------------------------------------------------------------------------------

HET_CASES = [("95-17-0", False), ("95-17-0", True), ("97-17-0", False), ("97-17-0", True), ("95-17-32", False)]


def het_dict(rng, k, canonical):
    """test_het.planted, and near-families: for every limb t a k-mer that differs from a family member in the middle base
    AND in one base of limb t.  It is no partner; a partner lookup that ignored limb t would report it."""
    from test_het import planted
    d = planted(rng, k, canonical)
    p = (k - 1) // 2
    members = [x for x, c in d.items() if c >= 50][:8]
    sub = lambda x, i: x[:i] + bytes([b"ACGT"[(b"ACGT".index(x[i]) + 1) % 4]]) + x[i + 1:]
    c = 700
    for j, x in enumerate(members):
        for t in range((2 * k + 63) // 64):
            at = min(32 * t + 1 + j, k - 1) if 32 * t + 1 + j != p else 32 * t
            y = sub(sub(x, p), at)
            assert sum(1 for u, v in zip(x, y) if u != v) == 2 and at // 32 == t
            d.setdefault(y, c)
            c += 1
    return kmerdb.fold_strands(d) if canonical else d


@pytest.mark.parametrize("name,canonical", HET_CASES, ids=["%s%s" % (n, "-canonical" if c else "") for n, c in HET_CASES])
def test_het_pairs(T, name, canonical):
    from test_het import pair_list
    r = D.row(name)
    k = r.k
    d = het_dict(np.random.default_rng(2000 + k + r.s), k, canonical)
    m = new_map(T, r, seed=k, canonical=canonical)
    try:
        names = sorted(d)
        m.addKmers(kmerdb.kmers_to_limbs(names, k), np.array([d[x] for x in names], dtype=np.uint64))
        assert table_dict(m) == d
        for mode in ("unique", "all"):
            for lower, upper in ((1, None), (8, 400)):
                want_pairs, want_stats = T.het_pairs(d, k, lower, upper, mode, canonical=canonical)
                assert want_stats["pairs"] and want_stats["families_2"] and (mode == "unique" or want_stats["families_3plus"])
                for nm, nM in ((1002, 1002), (3, 200)):
                    got, st = m.hetHistogram(nm, nM, lower, upper, mode)
                    assert np.array_equal(got, T.het_histogram(want_pairs, nm, nM)), (mode, nm, nM)
                    assert st == want_stats, (mode, st, want_stats)
                assert pair_list(m, m.hetPairs(lower, upper, mode)) == want_pairs, (mode, lower)
    finally:
        m.close()


# ---- identities by lookup, on every row -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", D.ROWS, ids=D.IDS)
def test_lookup_identities(T, r):
    """The joint spectrum of a table with itself is its histogram on the diagonal; intersect(min) of a table with itself
    is the table.  Both look every k-mer of the sweep up again."""
    from test_combine import check_result
    from test_count_output import expected_hist
    k = r.k
    tx = D.texts(k)
    text = tx.sib_a + tx.sib_b + tx.synth_a[:len(tx.synth_a) // 2]
    text = text[:text.rindex(b"\n@") + 1]
    want = dict(python_counts(text, k))
    m = new_map(T, r, text=text)
    try:
        n = 40
        h = m.getCountHistogram(n)
        assert np.array_equal(h, expected_hist(want.values(), n))
        j = m.jointHistogram(m, n, n)
        assert np.array_equal(np.diag(j)[1:], h[1:]) and j.sum() == np.trace(j) == len(want)
        out = m.combine(m, "intersect", "min")
        check_result(out, *combine_expect(want, want, "intersect", "min"))
        assert table_dict(out) == want
        out.close()
    finally:
        m.close()
