"""The designers of tests/twin_design.py checked with kmerdb alone, on seeded random invertible GF(2) matrices as the
mapping's rows: no library, no GPU.  For every family: its hashed keys differ exactly in the field asked for, the slot
words kmerdb.encode_slot gives at equal reprobe count are equal except word t (for the halves of word 0: the other half
is equal), and a strand-tie k-mer and its reverse complement have one canonical key, the smaller of two keys whose top
limbs are equal."""
import functools

import pytest

import kmerdb as K
import twin_design as D

# k, l, s: shapes of tests/test_database_format.py's table
LAYOUTS = [(31, 16, 0), (31, 20, 16), (33, 20, 0), (63, 18, 0), (63, 20, 32), (65, 20, 0), (96, 18, 2), (97, 20, 0),
           (127, 18, 2)]
SHAPES = {(31, 16, 0): (1, 1), (31, 20, 16): (1, 2), (33, 20, 0): (2, 1), (63, 18, 0): (2, 2), (63, 20, 32): (2, 3),
          (65, 20, 0): (3, 2), (96, 18, 2): (3, 3), (97, 20, 0): (4, 3), (127, 18, 2): (4, 4)}      # key limbs, W
IDS = ["k%d-l%d-s%d" % r for r in LAYOUTS]
T = 48


@functools.lru_cache(maxsize=None)
def mapping(k):
    rows = D.random_rows(k, 1000 + k)
    return rows, K.inverse_rows(rows, k)


def family_size(lay, field):
    """48, or every value of a field narrower than six bits"""
    return min(T, 1 << D.field_bits(lay, field)[1])


def test_every_field_occurs_and_the_shapes_are_the_tables():
    seen = set()
    for k, l, s in LAYOUTS:
        lay = K.Layout(k, l, s)
        assert (lay.key_limbs, lay.W) == SHAPES[(k, l, s)], lay
        first = 0
        for f in D.FIELDS:                                   # the fields tile the func bits
            a, w = D.field_bits(lay, f)
            if w:
                assert a == first
                first = a + w
                seen.add(f)
        assert first == lay.F
    assert seen == set(D.FIELDS), sorted(set(D.FIELDS) - seen)


@pytest.mark.parametrize("field", D.FIELDS)
@pytest.mark.parametrize("kls", LAYOUTS, ids=IDS)
def test_key_twins(kls, field):
    k, l, s = kls
    lay = K.Layout(k, l, s)
    first, width = D.field_bits(lay, field)
    if width == 0:
        pytest.skip("%r holds no func bits of %r" % (field, lay))
    rows, inv = mapping(k)
    n = family_size(lay, field)
    home = (0x5A5A5A5A5 + 977 * k) & (lay.slots - 1)
    kmers, keys = D.key_twins(lay, inv, home, n, field, seed=k * 100 + l)
    assert len(kmers) == n == len(set(kmers)) and all(len(x) == k and set(x) <= set(b"ACGT") and len(set(x)) > 1 for x in kmers)
    # the keys are those of the k-mers under the forward mapping
    assert K.table_keys(kmers, rows, k) == keys
    fmask = ((1 << width) - 1) << (first + l)
    assert all(key & (lay.slots - 1) == home for key in keys)
    assert len({key & ~fmask for key in keys}) == 1                       # equal outside the field ...
    assert len({key & fmask for key in keys}) == n                        # ... pairwise different inside
    # the slot words at equal reprobe count
    for i in (1, 7):
        words = [K.encode_slot(lay, key, i, 3) for key in keys]
        if field.startswith("limb0"):
            t = 0
            half = (lambda w: w & 0xFFFFFFFF) if field == "limb0_hi" else (lambda w: w >> 32)
            other = (lambda w: w >> 32) if field == "limb0_hi" else (lambda w: w & 0xFFFFFFFF)
            assert len({half(w[0]) for w in words}) == 1
            assert len({other(w[0]) for w in words}) == n
        else:
            t = int(field[6:-1])
        for u in range(lay.W):
            assert len({w[u] for w in words}) == (n if u == t else 1), (field, u)
        assert all(K.decode_slot(lay, lay.probe(home, i), w)[0] == key for w, key in zip(words, keys))
    with pytest.raises(ValueError):
        D.key_twins(lay, inv, lay.slots, n, field, seed=1)                # no such home slot
    if width <= 8:
        with pytest.raises(ValueError):
            D.key_twins(lay, inv, home, (1 << width) + 1, field, seed=1)  # more twins than the field has values


@pytest.mark.parametrize("k", [33, 63, 65, 96, 97, 127])
def test_h0_twins(k):
    rows, inv = mapping(k)
    wk = (2 * k + 63) // 64
    taken = set()
    for t in range(1, wk):
        n = min(40, 1 << min(64, 2 * k - 64 * t))          # (k = 33: limb 1 holds two bits)
        kmers, keys = D.h0_twins(k, inv, n, t, seed=k + t, taken=taken)
        taken.update(kmers)
        assert K.table_keys(kmers, rows, k) == keys and len(set(kmers)) == n
        limbs = K.ints_to_limbs(keys, wk)
        for u in range(wk):
            assert len(set(limbs[:, u].tolist())) == (n if u == t else 1)
        with pytest.raises(ValueError):
            D.h0_twins(k, inv, 5 if n < 40 else 1 << 70, t, seed=1)
    if k == 33:
        return
    # accept() picks among the candidates
    kmers, keys = D.h0_twins(k, inv, 8, 1, seed=5, accept=lambda key: (key >> 64) % 4 == 1)
    assert all((key >> 64) % 4 == 1 for key in keys) and len(set(keys)) == 8


@pytest.mark.parametrize("k", [63, 96, 127])
def test_text_twins(k):
    wk = (2 * k + 63) // 64
    for t in range(wk):
        kmers = D.text_twins(k, 100, t, seed=k + t)
        assert len(set(kmers)) == 100
        lo, hi = 32 * t, min(k, 32 * t + 32)
        assert len({x[:lo] + x[hi:] for x in kmers}) == 1 and len({x[lo:hi] for x in kmers}) == 100
        limbs = K.kmers_to_limbs(kmers, k)
        for u in range(wk):
            assert len(set(limbs[:, u].tolist())) == (100 if u == t else 1)


@pytest.mark.parametrize("k", [63, 96, 127])
def test_sliding_twins(k):
    wk = (2 * k + 63) // 64
    for t in range(wk):
        m = 16
        reads = D.sliding_twins(k, t, m, 30, seed=k + t)
        assert len(set(reads)) == 30 and all(len(r) == k + m for r in reads)
        wins = [r[i:i + k] for r in reads for i in range(m + 1)]
        assert len(set(wins)) == 30 * (m + 1) and not any(len(set(x)) == 1 for x in wins)
        limbs = K.kmers_to_limbs(wins, k)
        for u in range(wk):                       # all windows of all reads: twins in limb t
            assert len(set(limbs[:, u].tolist())) == (len(wins) if u == t else 1)
    with pytest.raises(ValueError):
        D.sliding_twins(k, wk - 1, 31, 3, seed=1)


# (k = 63 is left out: 62 equations on the 62 dimensions that x ^ reverse(x) spans have a solution for some mappings only)
@pytest.mark.parametrize("k", [47, 65, 80, 96, 127])
def test_strand_ties(k):
    rows, _ = mapping(k)
    wk = (2 * k + 63) // 64
    kmers, pairs = D.strand_ties(rows, k, 12, seed=k)
    top = 64 * (wk - 1)
    assert len(set(kmers) | {K.revcomp(x) for x in kmers}) == 24
    for x, (h, hr) in zip(kmers, pairs):
        r = K.revcomp(x)
        assert K.table_keys([x, r], rows, k) == [h, hr]
        assert h >> top == hr >> top and h != hr                              # a tie in the whole top limb ...
        assert (h >> (top - 64)) & K.M64 != (hr >> (top - 64)) & K.M64        # ... decided in limb WK - 2
        cx, cr = K.table_keys([x, r], rows, k, canonical=True)
        assert cx == cr == min(h, hr)
    # both outcomes occur: the forward strand is the smaller key for some, the reverse strand for others
    assert {h < hr for h, hr in pairs} == {True, False}


def test_reverse_complement_is_the_affine_map():
    for k in (5, 32, 47, 80):
        x = K.limbs_to_kmers(K.ints_to_limbs([0x123456789ABCDEF123456789ABCDEF0123456789 & ((1 << (2 * k)) - 1)],
                                             (2 * k + 63) // 64), k)[0]
        xi = K.keys_to_ints(K.kmers_to_limbs([x], k))[0]
        ri = K.keys_to_ints(K.kmers_to_limbs([K.revcomp(x)], k))[0]
        assert D.revcomp_int(xi, k) == ri and D.reverse_bases(D.reverse_bases(xi, k), k) == xi


def test_strand_ties_refuse_one_limb_keys():
    with pytest.raises(ValueError):
        D.strand_ties(D.random_rows(31, 3), 31, 4, seed=1)
