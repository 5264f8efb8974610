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

The compares behind a full list -- the spill cache of the skewed level-2 form (spill_record), the "homeless" merge of
partition_ring_kernel, the one-place cache of the fused walk's sub-list-full exit -- see keys only when a bucket is
skewed.  For them (tests/test_twin_keys_skew_cpu.py, tests/test_twin_keys_skew.py):

    hot_h0_families  h0_twins of which two start at one place of the spill cache (spill_places restates its place function)
    half_twins       one-word keys of one segment that agree outside one 32-bit half of the word
    skew_text        one k-mer per read, the family interleaved, then one member back to back, then interleaved again,
                     between ordinary synthetic reads
    model_counts     a Python model of the two compare sites with the compare as a parameter: what a weakened compare
                     would do to such a text -- the kernels themselves are never made wrong

What these do NOT reach: the walk's per-wave hot-key cache holds the four homopolymer keys only (s_homh), so no twin can be
designed into it (it gets a totals case); the plain (not SKEW) form's one-probe cache sees these families only where the
skew probe does not flag their bucket; the multi-GPU exchanges and tables above 2^32 slots are out of scope."""
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


def h0_twins(k, inv, T, t, seed, taken=(), accept=None, fix=None):
    """T k-mers whose hashed keys agree in every 64-bit limb except limb t (1 <= t < key limbs), where they all differ:
    one h[0], hence one home slot.  accept(key) -> bool, when given, picks among the candidates (a test may steer the
    keys further); fix = (mask, value) sets the bits of the common part under mask (outside limb t) to value.
    Returns (k-mers, hashed keys as ints)."""
    wk = (2 * k + 63) // 64
    if not 1 <= t < wk:
        raise ValueError("limb %d of %d" % (t, wk))
    width = min(64, 2 * k - 64 * t)
    if (1 << width) < T:
        raise ValueError("limb %d holds %d key bits: no %d different values" % (t, width, T))
    if fix is not None and fix[0] & (((1 << width) - 1) << (64 * t)):
        raise ValueError("fix reaches into limb %d" % t)
    rng = random.Random(seed)
    for _ in range(64):
        base = rng.getrandbits(2 * k) & ~(((1 << width) - 1) << (64 * t))
        if fix is not None:
            base = (base & ~fix[0]) | (fix[1] & fix[0])
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


# ---- the compares behind a full list: spill cache, homeless merge ------------------------------------------------------------

PHI = 0x9E3779B97F4A7C15
M32 = (1 << 32) - 1
OVF_N = 64            # places of the spill cache (tsx_partition.h)
OVF_PROBES = 4        # places spill_record looks at for one key
OVQ_CAP = 2048        # records of one workgroup's overflow queue (tsxcount_hip.hip)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & kmerdb.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & kmerdb.M64
    return z ^ (z >> 31)


def rec_words(k):
    """Words of a record of the partitioned path: the key limbs padded to 1, 2 or 4."""
    wk = (2 * k + 63) // 64
    return wk if wk <= 2 else 4


def record(key, k):
    return tuple((key >> (64 * t)) & kmerdb.M64 for t in range(rec_words(k)))


def record_places(w):
    """The places of the spill cache spill_record probes for the record w (a tuple of words), in order.  The walk's
    sub-list-full exit (one-word records) looks at the first of them only."""
    mixin = w[0]
    for x in w[1:]:
        mixin ^= (x * PHI) & kmerdb.M64
    s = (mix64(mixin) >> 40) & (OVF_N - 1)
    return [(s + i) & (OVF_N - 1) for i in range(OVF_PROBES)]


def spill_places(key, k):
    return record_places(record(key, k))


def meeting_pairs(keys, k):
    """Pairs of keys that START at one place of the spill cache.  Their probe sequences are the same, places are never
    given back, so whichever of the two is admitted first sits at a place the other one looks at before it finds a free
    one: the compare of the other words (one-word records: of the whole word) runs between two different keys whatever
    the order of the claims -- unless strangers hold all four places, and then neither is cached."""
    first = [spill_places(key, k)[0] for key in keys]
    return [(i, j) for i in range(len(keys)) for j in range(i + 1, len(keys)) if first[i] == first[j]]


def overlapping_pairs(keys, k):
    """Pairs of keys whose four-place probe windows share a place (the weaker condition: they MAY meet)."""
    win = [set(spill_places(key, k)) for key in keys]
    return [(i, j) for i in range(len(keys)) for j in range(i + 1, len(keys)) if win[i] & win[j]]


def radix_split(l, S):
    """(b1, b2): the radix bits of level 1 and level 2 for 2^(l - S) segments, as radix_bits of tsxcount_hip.hip."""
    n = l - S
    b1 = min(9, n if n <= 8 else (n + 1) // 2)
    return b1, n - b1


def list_of(key, l, S):
    """(level-1 bucket, level-2 list) of a hashed key: partition_ring_kernel takes bq = (w[0] >> shift) & (nb - 1) with
    shift = l - b1, nb = 2^b1 at level 1 and shift = S, nb = 2^b2 at level 2 (run_partition_build): bits S .. l - 1 of
    word 0 together, the number of the key's segment."""
    b1, b2 = radix_split(l, S)
    return (key >> (l - b1)) & ((1 << b1) - 1), (key >> S) & ((1 << b2) - 1)


def hot_h0_families(k, inv, T, t, seed, taken=(), accept=None, fix=None, rows=None, canonical=False):
    """h0_twins(k, inv, T, t) -- T k-mers whose records agree in every 64-bit word but word t, so one level-1 bucket, one
    segment, one set of level-2 sub-lists -- of which at least two start at one place of the spill cache (meeting_pairs).
    canonical (needs the map's rows): every member's own strand carries the smaller key, so the record after the strand
    choice is the designed key, and no member is another's reverse complement.  ValueError when no seed gives that."""
    for attempt in range(400):
        try:
            kmers, keys = h0_twins(k, inv, T * (4 if canonical else 1), t, seed * 1000 + attempt, taken, accept, fix)
        except ValueError as e:
            if "limb" in str(e):          # the shape has no such family: no other seed will find one
                raise
            continue
        if canonical:
            hr = kmerdb.table_keys([kmerdb.revcomp(x) for x in kmers], rows, k)
            keep = [i for i in range(len(keys)) if keys[i] < hr[i]][:T]
            if len(keep) < T:
                continue
            kmers, keys = [kmers[i] for i in keep], [keys[i] for i in keep]
            if {kmerdb.revcomp(x) for x in kmers} & set(kmers):
                continue
        if not meeting_pairs(keys, k):
            continue
        words = [record(key, k) for key in keys]
        assert all(len({w[u] for w in words}) == (T if u == t else 1) for u in range(rec_words(k))), "not twins in word %d" % t
        return kmers, keys
    raise ValueError("no family of %d twins in word %d meets in the spill cache" % (T, t))


def half_twins(k, inv, T, half, l, S, seed, taken=()):
    """T k-mers of one-word keys (k <= 32) whose hashed keys agree in every bit outside one 32-bit half of the word ("lo":
    bits 0 .. 31, "hi": bits 32 .. 2k - 1) and in the bits that pick the list at both radix levels (list_of: bits
    S .. l - 1), and of which two start at one place of the spill cache.  Returns (k-mers, keys)."""
    n = 2 * k
    if n > 64 or half not in ("lo", "hi"):
        raise ValueError("half twins are for one-word records: k = %d, half %r" % (k, half))
    a, b = (0, min(32, n)) if half == "lo" else (32, n)
    free = (((1 << b) - 1) & ~((1 << a) - 1)) & ~(((1 << l) - 1) & ~((1 << S) - 1)) if b > a else 0
    if (1 << bin(free).count("1")) < 4 * T:
        raise ValueError("the %s half of a %d-bit key leaves no %d values outside the list bits" % (half, n, T))
    for attempt in range(400):
        rng = random.Random(seed * 1000 + attempt)
        base = rng.getrandbits(n) & ~free
        vals = set()
        while len(vals) < T:
            vals.add(rng.getrandbits(n) & free)
        keys = [base | v for v in sorted(vals, key=lambda v: rng.random())]
        if not meeting_pairs(keys, k):
            continue
        kmers = kmerdb.keys_to_kmers(keys, inv, k)
        if not _usable(kmers, taken):
            continue
        assert len({list_of(key, l, S) for key in keys}) == 1, "the family does not share one list"
        other = ~(M32 if half == "lo" else M32 << 32)
        assert len({key & other for key in keys}) == 1 and len(set(keys)) == T
        return kmers, keys
    raise ValueError("no family found")


def skew_text(members, rounds, b2b, tail, cold_before=b"", cold_after=b"", strand=None):
    """(text, the family's reads in text order).  Every family read is exactly one k-mer: one window per read, so the
    records reach the kernels in the order of the text.  `rounds` times the members interleaved (A, B, C, ..., A, B, C, ...:
    twins sit in neighbouring lanes of a wave's batch, and a member comes back within 64 records when there are at most
    32 of them), then member 0 `b2b` times back to back (a run of equal records: combined records of d >= 2 certainly
    form), then `tail` rounds interleaved again (twins that come AFTER the admission).  strand(x, round) may pick the
    strand a round shows (canonical cases); cold_before / cold_after: FASTQ texts around the family."""
    show = strand if strand is not None else (lambda x, r: x)
    seqs = [show(x, r) for r in range(rounds) for x in members]
    seqs += [show(members[0], j) for j in range(b2b)]
    seqs += [show(x, r) for r in range(tail) for x in members]
    fam = b"".join(b"@t%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    return cold_before + fam + cold_after, seqs


COMPARES = {
    "exact": lambda a, b: a == b,
    "word 0 only": lambda a, b: a[0] == b[0],
    "low halves only": lambda a, b: all((x & M32) == (y & M32) for x, y in zip(a, b)),
    "high halves only": lambda a, b: all((x >> 32) == (y >> 32) for x, y in zip(a, b)),
}


def all_words_but(t):
    return lambda a, b: all(x == y for u, (x, y) in enumerate(zip(a, b)) if u != t)


def model_counts(recs, cap, same):
    """A model of what one level-2 workgroup of the SKEW form does with the records `recs` (tuples of words, in order) of
    one segment whose list holds `cap` records, with the key compare `same(a, b)` as a parameter.  The first cap records
    stay in the list.  The others are homeless: in runs of 64 (a wave's lanes), twice, the first record left is compared
    with all the others and those that are `same` leave as one entry with their number; the rest go one by one.  What
    leaves goes to the cache: 64 places, four probed per record (record_places), a free place is taken only by an entry
    of two or more, an entry that is `same` as the one in the place adds to it; what is not cached is inserted on its own
    (overflow queue, deferred list).  Returns {record: count}.  With the exact compare that is the plain count of recs."""
    from collections import Counter
    out = Counter(recs[:cap])
    cache = [None] * OVF_N

    def spill(rec, d):
        for p in record_places(rec):
            if cache[p] is None:
                if d < 2:
                    break
                cache[p] = [rec, d]
                return
            if same(cache[p][0], rec):
                cache[p][1] += d
                return
        out[rec] += d

    for i in range(cap, len(recs), 64):
        run = list(recs[i:i + 64])
        for _ in range(2):
            if run:
                first = run[0]
                spill(first, sum(1 for r in run if same(r, first)))
                run = [r for r in run if not same(r, first)]
        for r in run:
            spill(r, 1)
    for e in cache:
        if e is not None:
            out[e[0]] += e[1]
    return out
