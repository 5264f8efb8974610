"""The width matrix on the CPU: every row's (key limbs, slot words) class through kmerdb.Layout, and that the texts of
tests/width_design.py are sharp -- a table whose compares or lookups ignore part of the key would give other answers
on them, so the GPU cases of tests/test_width_matrix.py, which compare whole results, would fail on such a kernel.

The defects are stated on the reference side only: the Python dictionary of a text (conftest.python_counts,
test_read_query.coded_counts) is computed exactly and with every key cut to bases [0, 32), to bases [0, 64) and to the
bases below the partial top limb (width_design.truncations).  No kernel is made wrong, here or anywhere else."""
import pytest

import kmerdb as K
import width_design as D
from conftest import python_counts
from test_read_query import coded_counts

ROWS = D.ROWS
IDS = D.IDS


def test_rows_hold_every_class():
    classes = {(r.key_limbs, r.W) for r in ROWS}
    assert {(1, 1), (1, 2), (2, 2), (3, 2), (3, 3), (3, 4), (4, 3)} <= classes
    assert {r.k for r in ROWS if D.full_top_limb(r)} == {32, 64, 96}
    # these four rows and the W > WK rows stand in test_database_format.MATRIX with the same values
    from test_database_format import MATRIX
    have = {m[:5] for m in MATRIX}
    for name in ("31-20-16", "65-20-0", "80-20-0", "96-18-2", "96-20-32", "97-20-0"):
        r = D.row(name)
        assert (r.k, r.l, r.s, r.key_limbs, r.W) in have, name


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_layout_class(r):
    lay = D.layout_of(r)
    assert lay.fields()["key_limbs"] == r.key_limbs and lay.fields()["entry_limbs"] == r.W
    assert lay.slots <= 1 << 20
    if r.s:
        assert lay.C == r.s
    if r.note.endswith("carry"):
        assert lay.C == 2                      # counts of 4 and more carry: the texts' multiplicities reach 5
    # the class holds at the lowered l the GPU cases may use
    for l in (17, 18):
        if l < r.l:
            D.layout_of(r, l)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_sibling_windows_differ_in_one_base_at_every_offset(r):
    k = r.k
    tx = D.texts(k)
    for a, b, p in tx.pairs():
        assert len(a) == len(b) == 2 * k + 40 and a[p] != b[p] and a[:p] + a[p + 1:] == b[:p] + b[p + 1:]
        ca, cb = D.covering(a, p, k), D.covering(b, p, k)
        assert sorted(ca) == sorted(cb) == list(range(k))            # every offset 0 .. k - 1
        for off in range(k):
            x, y = ca[off], cb[off]
            assert len(x) == k and [i for i in range(k) if x[i] != y[i]] == [off]
        # so the two differ in every limb, the top one included
        la, lb = K.kmers_to_limbs([ca[o] for o in range(k)], k), K.kmers_to_limbs([cb[o] for o in range(k)], k)
        for t in range(r.key_limbs):
            rows_t = [o for o in range(k) if o // 32 == t]
            assert rows_t and all(la[o, t] != lb[o, t] and (la[o] != lb[o]).sum() == 1 for o in rows_t)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_texts_are_not_degenerate(r):
    k = r.k
    tx = D.texts(k)
    da, db = python_counts(tx.text_a, k), python_counts(tx.text_b, k)
    assert da == coded_counts(tx.text_a, k, 4) and db == coded_counts(tx.text_b, k, 4)     # ACGT texts: one reference
    assert set(da) - set(db) and set(db) - set(da) and set(da) & set(db)
    sa, sb = python_counts(tx.sib_a, k), python_counts(tx.sib_b, k)
    assert set(sa) - set(sb) and set(sb) - set(sa) and set(sa) & set(sb)
    assert {D.CROSS_A} | set(D.WITHIN_A) <= set(sa.values()) and {D.CROSS_B} | set(D.WITHIN_B) <= set(sb.values())
    # shared k-mers whose counts differ between the sides, and counts on both sides of 2 (the prefilter's threshold)
    assert any(sa[x] != sb[x] for x in set(sa) & set(sb))
    assert 1 in sb.values() and max(sb.values()) >= 4 and max(sa.values()) >= 5
    # the query: reads that hit A alone, B alone, both and neither, and one without a window
    dq = python_counts(tx.query, k)
    hits = [(sum(1 for i in range(len(s) - k + 1) if s[i:i + k] in da), sum(1 for i in range(len(s) - k + 1) if s[i:i + k] in db))
            for s in tx.query_seqs]
    assert any(a and not b for a, b in hits) and any(b and not a for a, b in hits) and any(a and b for a, b in hits)
    assert sum(1 for a, b in hits if not a and not b) >= 3 and min(len(s) for s in tx.query_seqs) == k - 1
    assert set(dq) - set(da) - set(db)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_truncated_keys_give_other_dictionaries(r):
    k = r.k
    tx = D.texts(k)
    cuts = D.truncations(k)
    assert cuts and all(0 < n < k for n in cuts.values())
    if r.key_limbs >= 3:
        assert {"bases [0, 32)", "bases [0, 64)"} <= set(cuts)
        assert ("top partial limb dropped" in cuts) == (not D.full_top_limb(r))
    exact_a, exact_b = python_counts(tx.sib_a, k), python_counts(tx.sib_b, k)
    whole_a, whole_b = python_counts(tx.text_a, k), python_counts(tx.text_b, k)
    for label, n in cuts.items():
        for exact in (exact_a, exact_b, whole_a, whole_b):
            cut = D.truncated(exact, n)
            assert len(cut) < len(exact), label                                   # other distinct k-mers
            assert sum(cut.values()) == sum(exact.values())
            wrong = [x for x in exact if cut[x[:n]] != exact[x]]
            assert wrong, label                                                    # and another count for some k-mer
        # through the siblings, not through chance: the windows of a pair that differ at an offset >= n merge, and their
        # counts differ, in one table (the pairs of A) and across the two (the cross pairs)
        for a, b, p in tx.within_a:
            ca, cb = D.covering(a, p, k), D.covering(b, p, k)
            for off in range(n, k):
                assert ca[off][:n] == cb[off][:n] and exact_a[ca[off]] != exact_a[cb[off]], (label, off)
            for off in range(n):
                assert ca[off][:n] != cb[off][:n]
        cut_b = D.truncated(exact_b, n)
        for a, b, p in tx.cross:
            ca = D.covering(a, p, k)
            only_a = [ca[off] for off in range(k) if ca[off] not in exact_b]
            assert len(only_a) == k
            found = [x for x in only_a if x[:n] in cut_b]
            assert len(found) >= k - n, label       # A's k-mers that a cut lookup finds in B, which does not hold them


@pytest.mark.parametrize("r", [x for x in ROWS if x.k % 2 == 0], ids=[D.row_id(x) for x in ROWS if x.k % 2 == 0])
def test_palindrome_record(r):
    pal, rec = D.palindrome_record(r.k)
    assert len(pal) == r.k and K.revcomp(pal) == pal
    d = K.fold_strands(python_counts(rec * 3, r.k))
    assert d[pal] == 3 and sum(d.values()) == 9
