"""The width matrix of tests/test_width_matrix.py and tests/test_width_matrix_cpu.py: the (k, l, s) rows with their
(key limbs, slot words) class, and texts whose k-mers depend on every limb of the key.

Every kernel that touches a key is a template over WK, the 64-bit limbs of a key, and runs with slots of W words, which
derive_layout picks independently of WK.  The rows below hold one table of every class the features were never run at:
three-limb keys with slots narrower than, as wide as and wider than the key, a three-word slot under a four-limb key, a
slot wider than a one-limb key, and the full-limb values k = 32 / 64 / 96 (top mask ~0, shift amounts that reach 64).

Random reads differ in every limb at once, so a path that mangles one limb alone can hide behind the other limbs.  The
texts here are built around *sibling reads*: a read R of 2k + 40 bases and a copy R' with one base substituted at a
position p with k - 1 <= p <= k + 40.  The k windows of R that cover p differ from the windows of R' at the same
starts in exactly one base, at every offset k - 1 .. 0 of the window: in every limb, and in the partial top limb.  R
and R' go to different sides (table A against table B, counted text against query text, seen once against seen twice)
or into one text with different multiplicities, so a compare or a lookup that ignores any base of the key merges two
k-mers whose expected counts differ.  tests/test_width_matrix_cpu.py shows that on the CPU with truncated keys.

Nothing here imports the library; the synthetic reads come from tsxcount_amd.synth (numpy alone)."""
import random
from collections import Counter, namedtuple

import kmerdb as K

Row = namedtuple("Row", "k l s key_limbs W note")

# k, l, s, key limbs WK, slot words W.  Every row is a derive_layout result: layout_of asserts it through kmerdb.Layout on
# the CPU, new_map (test_width_matrix.py) against tsx_hip_get_layout on the GPU before any feature call.
ROWS = [
    Row(32, 20, 0, 1, 1, "WK 1 full limb, W 1"),
    Row(31, 20, 16, 1, 2, "W > WK"),
    Row(64, 20, 0, 2, 2, "WK 2 full limb, W 2"),
    Row(65, 20, 0, 3, 2, "W < WK"),
    Row(80, 20, 0, 3, 3, "W = WK, partial top limb"),
    Row(96, 18, 2, 3, 3, "WK 3 full limb, counters that carry"),
    Row(96, 20, 32, 3, 4, "WK 3 full limb, W > WK"),
    Row(97, 20, 0, 4, 3, "W 3 under WK 4"),
    # het pairs (odd k on both sides of the step from three to four limbs), l = 17
    Row(95, 17, 0, 3, 3, "odd k below the limb step"),
    Row(97, 17, 0, 4, 3, "odd k above the limb step"),
    Row(95, 17, 32, 3, 4, "odd k, W > WK"),
]


def row_id(r):
    return "%d-%d-%d" % (r.k, r.l, r.s)


IDS = [row_id(r) for r in ROWS]


def row(name):
    return ROWS[IDS.index(name)]


def rows(*names):
    return [row(n) for n in names]


def full_top_limb(r):
    return (2 * r.k) % 64 == 0


def layout_of(r, l=None):
    """kmerdb.Layout of the row (with another l when a case lowers it): the class asserted."""
    lay = K.Layout(r.k, r.l if l is None else l, r.s)
    assert (lay.key_limbs, lay.W) == (r.key_limbs, r.W), (r, lay)
    assert lay.key_limbs == (2 * r.k + 63) // 64 and lay.l <= 20
    return lay


# ---- sibling reads ------------------------------------------------------------------------------------------------------

def rand_seq(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def sibling_pair(rnd, k, j=0):
    """(R, R', p): R of 2k + 40 bases, R' = R with the base at p substituted, k - 1 <= p <= k + 40."""
    n = 2 * k + 40
    p = k - 1 + (7 * j) % 42
    assert k - 1 <= p <= n - k
    r = rand_seq(rnd, n)
    other = rnd.choice(b"ACGT".replace(r[p:p + 1], b""))
    return r, r[:p] + bytes([other]) + r[p + 1:], p


def covering(r, p, k):
    """The k windows of a read that cover position p, by their offset of p in the window: {offset: k-mer}."""
    return {p - i: r[i:i + k] for i in range(p - k + 1, p + 1)}


def fastq_of(seqs, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def seqs_of(fastq):
    return [ln for ln in fastq.split(b"\n") if ln][1::4]


def palindrome_record(k):
    """The palindrome record of test_combine.test_canonical_tables: (the k-mer, the FASTQ record), even k."""
    assert k % 2 == 0
    pal = (b"ACGT" * 32)[:k // 2]
    pal += K.revcomp(pal)
    return pal, b"@pal\n" + pal + b"AC" + b"\n+\n" + b"I" * (k + 2) + b"\n"


CROSS_A, CROSS_B = 3, 2          # multiplicities of R in A and of R' in B
WITHIN_A = (2, 5)                # of R and R' of a pair that lies in A alone
WITHIN_B = (1, 4)                # ... in B alone


class Texts:
    """Two table texts and a query text for one k.

      cross pairs   R three times in A, R' twice in B
      pairs of A    R twice and R' five times in A; pairs of B likewise, once and four times
      synthetic     n_synth reads each, half of them shared
      query         R and R' of every pair once, chimeras of an A read and a B read, the shared and a few unshared
                    synthetic reads, random reads that hit nothing, a read shorter than k

    sib_a / sib_b are the sibling reads of each side alone, as texts (the CPU file's sharpness checks use them, so that
    the poly-A tails of the synthetic reads prove nothing)."""

    def __init__(self, k, seed=None, n_synth=24, n_cross=6, n_within=3):
        from tsxcount_amd import synth
        rnd = random.Random(9000 + k if seed is None else seed)
        self.k = k
        self.cross = [sibling_pair(rnd, k, j) for j in range(n_cross)]
        self.within_a = [sibling_pair(rnd, k, 3 * j + 1) for j in range(n_within)]
        self.within_b = [sibling_pair(rnd, k, 5 * j + 2) for j in range(n_within)]
        a = [r for r, _, _ in self.cross for _ in range(CROSS_A)]
        b = [r2 for _, r2, _ in self.cross for _ in range(CROSS_B)]
        for r, r2, _ in self.within_a:
            a += [r] * WITHIN_A[0] + [r2] * WITHIN_A[1]
        for r, r2, _ in self.within_b:
            b += [r] * WITHIN_B[0] + [r2] * WITHIN_B[1]
        rnd.shuffle(a)
        rnd.shuffle(b)
        self.sib_a, self.sib_b = fastq_of(a, b"a"), fastq_of(b, b"b")
        half = n_synth // 2
        sseed = 500 + k
        self.synth_a = synth.fastq(sseed, 0, n_synth)
        self.synth_b = synth.fastq(sseed, half, n_synth)
        self.text_a, self.text_b = self.sib_a + self.synth_a, self.sib_b + self.synth_b
        q = []
        for r, r2, _ in self.cross + self.within_a + self.within_b:
            q += [r, r2]
        q += [self.cross[0][0][:k + 30] + self.cross[1][1][-(k + 25):], self.within_a[0][1][:k + 5] + self.within_b[0][0][-(k + 9):]]
        q += seqs_of(synth.fastq(sseed, half - 1, 3)) + seqs_of(synth.fastq(sseed, half + n_synth - 1, 2))
        q += [rand_seq(rnd, k + 3 * j) for j in range(6)] + [rand_seq(rnd, k - 1)]
        rnd.shuffle(q)
        self.query_seqs = q
        self.query = fastq_of(q, b"q")

    def pairs(self):
        return self.cross + self.within_a + self.within_b


_TEXTS = {}


def texts(k, **kw):
    key = (k, tuple(sorted(kw.items())))
    if key not in _TEXTS:
        _TEXTS[key] = Texts(k, **kw)
    return _TEXTS[key]


# ---- truncated keys (the CPU file's defects; no kernel is ever made wrong) ------------------------------------------------

def truncations(k):
    """{label: n}: the ways of dropping whole limbs' worth of bases from a k-mer that drop some base and keep some --
    bases [0, 32) kept, bases [0, 64) kept, the partial top limb's bases dropped (n = 32 * (WK - 1)).  A one-limb key has
    none of them, so it gets the low 32-bit half of its limb, bases [0, 16), instead."""
    out = {}
    if k > 32:
        out["bases [0, 32)"] = 32
    if k > 64:
        out["bases [0, 64)"] = 64
    if k > 32 and k % 32:
        out["top partial limb dropped"] = 32 * ((2 * k + 63) // 64 - 1)
    if k <= 32:
        out["low half of limb 0"] = 16
    return out


def truncated(counts, n):
    """{k-mer: count} with every key cut to its first n bases: what a table whose compares see only those bases holds."""
    out = Counter()
    for x, c in counts.items():
        out[x[:n]] += c
    return out
