"""Designers of k-mers that meet in a key compare and differ in one limb or field only, in numpy and Python ints on top
of kmerdb (Layout, hash_keys, inverse_rows, keys_to_kmers): nothing here imports the library.

Random k-mers that meet in a compare differ in limb 0 already, so "limb 0 equal, a higher limb differs" never occurs
with them.  These families make it occur at every compare site of the table:

    key_twins     hashed keys with one home slot that agree in every func bit outside one field of the slot: the low
                  half of slot word 0 ("limb0_lo"), its high half ("limb0_hi"), or slot word t ("spill[t]")
    h0_twins      hashed keys that agree in every 64-bit limb but h[t], t >= 1 (the table of deferred_insert_kernel
                  claims word 0 and compares the others)
    text_twins    k-mers that agree outside bases 32t .. 32t + 31, limb t of the 2-bit encoding (kmer_eq of the scan)
    sliding_twins reads of k + m bases whose m + 1 windows are such twins of each other, at adjacent text positions (the
                  run-length leader test of the scan, sketch and query kernels compares a window with the one before)
    strand_ties   k-mers whose two strand keys h(x), h(rc x) agree in the whole top limb and differ below it (key_less)

What these do NOT reach, on purpose: the spill cache of the skewed level-2 form (spill_record), the "homeless" merge of
partition_ring_kernel and the hot-key cache of the walk.  Those compare keys too, but only a skewed bucket or
homopolymers get there; designing such texts is a second piece of work."""
import random

import numpy as np

import kmerdb

FIELDS = ("limb0_lo", "limb0_hi", "spill[1]", "spill[2]", "spill[3]")


def field_bits(lay, field):
    """(first func bit, number of func bits) of a field of the slot: func bit j sits at bit R + j of slot word 0 for
    j < f0, and at bit (j - f0) % 64 of word 1 + (j - f0) // 64 above."""
    lo = max(0, min(lay.f0, 32 - lay.R))
    if field == "limb0_lo":
        return 0, lo
    if field == "limb0_hi":
        return lo, lay.f0 - lo
    if field.startswith("spill[") and field.endswith("]"):
        t = int(field[6:-1])
        if t < 1:
            raise ValueError(field)
        a = lay.f0 + 64 * (t - 1)
        return a, max(0, min(lay.F, a + 64) - a) if t < lay.W else 0
    raise ValueError("no field %r" % (field,))


def fields_of(lay):
    """The fields of this layout that hold func bits."""
    return [f for f in FIELDS if field_bits(lay, f)[1] > 0]


def _distinct_values(rng, width, T):
    if (1 << width) < T:
        raise ValueError("a field of %d bits has no %d different values" % (width, T))
    if width <= 16:
        return rng.sample(range(1 << width), T)
    out = set()
    while len(out) < T:
        out.add(rng.getrandbits(width))
    return sorted(out, key=lambda v: rng.random())


def _usable(kmers, taken):
    return len(set(kmers)) == len(kmers) and not any(len(set(x)) == 1 or x in taken for x in kmers)


def key_twins(lay, inv, home, T, field, seed, taken=()):
    """T ACGT k-mers (no homopolymer, no duplicate, none of `taken`) whose hashed keys share the home slot and every
    func bit outside `field` and are pairwise different inside it.  inv: kmerdb.inverse_rows of the map's rows.
    Returns (k-mers, hashed keys as ints).  ValueError when the field has fewer than T values."""
    first, width = field_bits(lay, field)
    if not 0 <= home < lay.slots:
        raise ValueError("home slot %d" % home)
    rng = random.Random(seed)
    for _ in range(64):
        base = rng.getrandbits(lay.F) & ~(((1 << width) - 1) << first)
        keys = [((base | (v << first)) << lay.l) | home for v in _distinct_values(rng, width, T)]
        kmers = kmerdb.keys_to_kmers(keys, inv, lay.k)
        if _usable(kmers, taken):
            return kmers, keys
    raise ValueError("no family found")


def h0_twins(k, inv, T, t, seed, taken=(), accept=None):
    """T k-mers whose hashed keys agree in every 64-bit limb except limb t (1 <= t < key limbs), where they all differ:
    one h[0], hence one home slot.  accept(key) -> bool, when given, picks among the candidates (a test may steer the
    keys further).  Returns (k-mers, hashed keys as ints)."""
    wk = (2 * k + 63) // 64
    if not 1 <= t < wk:
        raise ValueError("limb %d of %d" % (t, wk))
    width = min(64, 2 * k - 64 * t)
    if (1 << width) < T:
        raise ValueError("limb %d holds %d key bits: no %d different values" % (t, width, T))
    rng = random.Random(seed)
    for _ in range(64):
        base = rng.getrandbits(2 * k) & ~(((1 << width) - 1) << (64 * t))
        keys, seen = [], set()
        for _ in range(4096 * T):
            v = rng.getrandbits(width)
            key = base | (v << (64 * t))
            if v in seen or (accept is not None and not accept(key)):
                continue
            seen.add(v)
            keys.append(key)
            if len(keys) == T:
                break
        if len(keys) < T:
            raise ValueError("accept() leaves fewer than %d keys" % T)
        kmers = kmerdb.keys_to_kmers(keys, inv, k)
        if _usable(kmers, taken):
            return kmers, keys
    raise ValueError("no family found")


def text_twins(k, T, t, seed, taken=()):
    """T k-mers that are identical outside limb t of the 2-bit encoding: they differ only in bases 32t .. 32t + 31 (or
    what the top limb holds of them)."""
    wk = (2 * k + 63) // 64
    if not 0 <= t < wk:
        raise ValueError("limb %d of %d" % (t, wk))
    width = min(64, 2 * k - 64 * t)
    rng = random.Random(seed)
    for _ in range(64):
        base = rng.getrandbits(2 * k) & ~(((1 << width) - 1) << (64 * t))
        xs = [base | (v << (64 * t)) for v in _distinct_values(rng, width, T)]
        kmers = kmerdb.limbs_to_kmers(kmerdb.ints_to_limbs(xs, wk), k)
        if _usable(kmers, taken):
            return kmers
    raise ValueError("no family found")


def sliding_twins(k, t, m, n_reads, seed, lo="A", hi="C"):
    """n_reads different reads of k + m bases: base `lo` up to position 32t + m, then w - m random bases (w = the bases limb
    t holds: 32, or k - 32t in the top limb), then base `hi` to the end.  Window i = read[i : i + k], i = 0 .. m, is all
    `lo` below limb t and all `hi` above it, so all (m + 1) * n_reads windows are identical outside bases 32t .. 32t + w - 1,
    and the windows of one read sit at adjacent positions of the text.  The random stretch begins with another base than
    `lo` and ends with another than `hi`: the windows of a read are pairwise different and none is a homopolymer."""
    wk = (2 * k + 63) // 64
    if not 0 <= t < wk or lo == hi:
        raise ValueError("limb %d of %d, bases %r %r" % (t, wk, lo, hi))
    w = min(32, k - 32 * t)
    if not 1 <= m <= w - 2:
        raise ValueError("m = %d does not leave two random bases in a limb of %d" % (m, w))
    rng = random.Random(seed)
    reads = set()
    while len(reads) < n_reads:
        mid = [rng.choice("ACGT") for _ in range(w - m)]
        if mid[0] == lo or mid[-1] == hi:
            continue
        reads.add((lo * (32 * t + m) + "".join(mid) + hi * (k - 32 * t - w + m)).encode())
    return sorted(reads, key=lambda r: rng.random())


# ---- strand ties ---------------------------------------------------------------------------------------------------------

def reverse_bases(x, k):
    """Base i of the k-mer x (an int, base j at bits 2j) to base k - 1 - i: a permutation of the 2k bits."""
    out = 0
    for i in range(k):
        out |= ((x >> (2 * i)) & 3) << (2 * (k - 1 - i))
    return out


def revcomp_int(x, k):
    """rc(x) = reverse the bases, then complement (c -> 3 - c = c ^ 3): affine over GF(2)."""
    return reverse_bases(x, k) ^ ((1 << (2 * k)) - 1)


def _parity(v):
    return bin(v).count("1") & 1


def strand_ties(rows, k, T, seed, taken=()):
    """T k-mers x whose strand keys h(x) and h(rc x) agree in every bit of the top key limb (bits 64 (WK - 1) .. 2k - 1)
    and differ in limb WK - 2.  Key bit b = parity(a[b] & x), and rc(x) = P x ^ ones with the symmetric permutation P, so
    bit b of h(x) ^ h(rc x) = parity((a[b] ^ P a[b]) & x) ^ parity(a[b]): one linear equation per bit of the top limb,
    solved by Gaussian elimination, the free variables drawn at random.  ValueError when the system has no solution.
    Returns (k-mers, [(h(x), h(rc x))] as ints)."""
    n, wk = 2 * k, (2 * k + 63) // 64
    if wk < 2:
        raise ValueError("strand ties need a multi-limb key")
    a = [sum(int(rows[n - 1 - b, t]) << (64 * t) for t in range(wk)) for b in range(n)]
    # reduced row echelon form of [mask | rhs]
    piv = {}                                           # pivot bit -> (mask, rhs)
    for b in range(64 * (wk - 1), n):
        m, r = a[b] ^ reverse_bases(a[b], k), _parity(a[b])
        for c, (pm, pr) in piv.items():
            if (m >> c) & 1:
                m, r = m ^ pm, r ^ pr
        if m == 0:
            if r:
                raise ValueError("no k-mer of k = %d has strand keys with equal top limbs" % k)
            continue
        c = m.bit_length() - 1
        for c2, (pm, pr) in list(piv.items()):
            if (pm >> c) & 1:
                piv[c2] = (pm ^ m, pr ^ r)
        piv[c] = (m, r)
    pmask = sum(1 << c for c in piv)
    rng = random.Random(seed)
    apply = lambda x: sum(_parity(a[b] & x) << b for b in range(n))
    xs, pairs = [], []
    for _ in range(64 * T):
        x = rng.getrandbits(n) & ~pmask
        for c, (m, r) in piv.items():                  # m = bit c + free bits only
            if _parity(m & x) ^ r:
                x |= 1 << c
        h, hr = apply(x), apply(revcomp_int(x, k))
        if (h >> (64 * (wk - 1))) != (hr >> (64 * (wk - 1))):
            raise AssertionError("the elimination is wrong")
        lo = 64 * (wk - 2)
        if ((h >> lo) & kmerdb.M64) == ((hr >> lo) & kmerdb.M64) or x in xs or revcomp_int(x, k) in xs:
            continue
        xs.append(x)
        pairs.append((h, hr))
        if len(xs) == T:
            break
    kmers = kmerdb.limbs_to_kmers(kmerdb.ints_to_limbs(xs, wk), k)
    if len(xs) < T or not _usable(kmers, taken):
        raise ValueError("no family found")
    return kmers, pairs


def random_rows(k, seed):
    """A seeded random invertible GF(2) matrix in the form of tsx_hip_hash_rows: (2k, key limbs) uint64, row i the mask
    of key bit 2k - 1 - i.  For tests of the designers that have no map."""
    n, wk = 2 * k, (2 * k + 63) // 64
    rng = random.Random(seed)
    while True:
        masks = [rng.getrandbits(n) for _ in range(n)]
        rows = np.array([[(m >> (64 * t)) & kmerdb.M64 for t in range(wk)] for m in masks], dtype=np.uint64)
        try:
            kmerdb.inverse_rows(rows, k)
            return rows
        except ValueError:
            continue
