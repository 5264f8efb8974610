"""What the device computes, stated on the CPU with numpy and the standard library alone: the definitions the GPU results
are tested against.  Nothing here calls the library."""
import numpy as np

from ._abi import (BIN_A, BIN_AMBIGUOUS, BIN_B, BIN_NONE, HET_MODES, JOINT_MAX_CELLS, NO_KMER, PREFILTER_BITS, SEQ_NAME_MAX,
                   SKETCH_PRECISIONS, _upper, key_limbs, revcomp)


def median_count(values):
    """The median as medianReads reports it, on the CPU: element m // 2 of the m sorted values (the upper middle for
    even m, khmer's convention), 0 without values.  Profile entries equal to NO_KMER are no values."""
    v = sorted(int(x) for x in values if int(x) != NO_KMER)
    return v[len(v) // 2] if v else 0


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _kmer_hash(kmers, k):
    """The 64-bit hash of each k-mer that the sketch and the prefilter share: v = 0x9E3779B97F4A7C15, then
    v = mix64(v ^ limb) limb by limb (splitmix64's finaliser), the bits above 2k of the last limb cleared first."""
    wk = key_limbs(k)
    a = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, wk).copy()
    if (2 * k) % 64:
        a[:, wk - 1] &= np.uint64((1 << ((2 * k) % 64)) - 1)
    with np.errstate(over="ignore"):
        v = np.full(len(a), 0x9E3779B97F4A7C15, dtype=np.uint64)
        for t in range(wk):
            v = _mix64(v ^ a[:, t])
    return v


def sketch_registers(kmers, k, precision=14):
    """The HyperLogLog registers of a set of k-mers, on the CPU with numpy alone (the definition the GPU sketch is tested
    against): numpy uint8[2^precision].  kmers: encoded limbs, (n, key_limbs(k)) or flat, taken as given (canonicalise
    first for a canonical map).  Per k-mer x: v = 0x9E3779B97F4A7C15, then v = mix64(v ^ limb) limb by limb (splitmix64's
    finaliser); the register v >> (64 - p) is raised to 1 + the number of leading zeros of the remaining 64 - p bits (all
    zero: 64 - p + 1)."""
    p = int(precision)
    if p not in SKETCH_PRECISIONS:
        raise ValueError("sketch precision must be 10 .. 14, not %r" % (precision,))
    v = _kmer_hash(kmers, k)
    regs = np.zeros(1 << p, dtype=np.uint8)
    if not len(v):
        return regs
    idx = (v >> np.uint64(64 - p)).astype(np.int64)
    rest = v & np.uint64((1 << (64 - p)) - 1)
    # leading zeros among 64 - p bits = (64 - p) - bit length; the bit length by halving (exact, no floating point)
    length = np.zeros(len(v), dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (rest >> np.uint64(s)) != 0
        length += np.where(big, s, 0)
        rest = np.where(big, rest >> np.uint64(s), rest)
    length += (rest != 0).astype(np.int64)
    rank = (64 - p) - length + 1
    np.maximum.at(regs, idx, rank.astype(np.uint8))
    return regs


def merge_sketches(a, b):
    """The sketch of the union of what two sketches of one precision saw: the register-wise maximum."""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    if a.shape != b.shape:
        raise ValueError("sketches of different precision")
    return np.maximum(a, b)


def prefilter_masks(kmers, k, bits):
    """Where a set of k-mers sits in a prefilter of 2^bits bits, on the CPU with numpy alone (the definition the GPU
    filter is tested against): (word_a, word_b, mask), three numpy uint64 arrays.  kmers: encoded limbs, (n, key_limbs(k))
    or flat, taken as given (canonicalise first for a canonical map).  Per k-mer: v = the hash of sketch_registers; the
    64-bit word of filter A is v >> (64 - (bits - 6)), that of filter B v >> (64 - (bits - 8)); the mask, the same in
    both, is the OR of 1 << ((v >> s) & 63) for s = 0, 6, 12, 18.  In a filter: word & mask == mask."""
    b = int(bits)
    if b not in PREFILTER_BITS:
        raise ValueError("prefilter bits must be 12 .. 38, not %r" % (bits,))
    v = _kmer_hash(kmers, k)
    mask = np.zeros(len(v), dtype=np.uint64)
    for s in (0, 6, 12, 18):
        mask |= np.uint64(1) << ((v >> np.uint64(s)) & np.uint64(63))
    return v >> np.uint64(64 - (b - 6)), v >> np.uint64(64 - (b - 8)), mask


def pair_name(header_line):
    """The name of a record as the pair calls compare it (check_names): the header line after its first byte ('@' or
    '>') up to the first space or tab, or the line's end, without one trailing "/1" or "/2"."""
    line = bytes(header_line.encode() if isinstance(header_line, str) else header_line).split(b"\n")[0]
    name = line[1:]
    for i, c in enumerate(name):
        if c in b" \t":
            name = name[:i]
            break
    if name.endswith((b"/1", b"/2")):
        name = name[:-2]
    return name


def joint_histogram(A, B, bins_a=1002, bins_b=1002):
    """The definition of TSXHashMapHIP.jointHistogram on the CPU: A and B map k-mer -> count (any hashable key; a count
    of 0 is an absent k-mer).  Returns numpy uint64[bins_a, bins_b]: [i, j] = the k-mers x of A u B with
    min(A[x], bins_a - 1) == i and min(B[x], bins_b - 1) == j."""
    if bins_a < 2 or bins_b < 2 or bins_a * bins_b > JOINT_MAX_CELLS:
        raise ValueError("joint_histogram: 2 <= bins and bins_a * bins_b <= 2^24")
    keys = list(set(A) | set(B))
    m = np.zeros((bins_a, bins_b), dtype=np.uint64)
    if keys:
        a = np.minimum(np.array([int(A.get(x, 0)) for x in keys], dtype=np.uint64), np.uint64(bins_a - 1)).astype(np.int64)
        b = np.minimum(np.array([int(B.get(x, 0)) for x in keys], dtype=np.uint64), np.uint64(bins_b - 1)).astype(np.int64)
        np.add.at(m, (a, b), np.uint64(1))
        m[0, 0] = 0   # in neither: not a k-mer of A u B
    return m


def het_pairs(D, k, lower=1, upper=None, mode="unique", canonical=False):
    """The definition of TSXHashMapHIP.hetPairs / hetHistogram on the CPU (Smudgeplot's hetkmers).  D maps k-mer string ->
    count, as a dump reports it (canonical: the smaller strand); k is odd.  A k-mer counted outside [lower, upper] is absent.
    The family of x is x and those of its three middle-base variants (canonical: each taken to its smaller strand) that D
    holds in range.  A pair is two members of one family: mode 'unique' counts the pair of a family of exactly two, 'all'
    every pair of every family.  Returns (pairs, stats): pairs a list of (minor k-mer, its count, major k-mer, its count),
    minor being the lower count and on a tie the smaller string, each pair once, sorted; stats the dict of
    kmers_in_range, paired, pairs, families_2, families_3plus (families of exactly 2 / of 3 or 4, each counted once)."""
    if k % 2 == 0:
        raise ValueError("het_pairs: k must be odd (an even k has no middle base)")
    if mode not in HET_MODES:
        raise ValueError("het_pairs: mode is 'unique' or 'all', got %r" % (mode,))
    top = _upper(upper)
    low = max(int(lower), 1)
    canon = (lambda x: min(x, revcomp(x))) if canonical else (lambda x: x)   # (what canonical() gives for a string)
    R = {}
    for x, c in D.items():
        x = x.decode() if isinstance(x, bytes) else x   # (k-mers come back as str)
        if len(x) != k:
            raise ValueError("het_pairs: %r is no %d-mer" % (x, k))
        if low <= int(c) <= top:
            R[canon(x)] = int(c)
    p = (k - 1) // 2
    families = set()
    for x in R:
        fam = {x}
        for b in "ACGT":
            y = canon(x[:p] + b + x[p + 1:])
            if y in R:
                fam.add(y)
        families.add(tuple(sorted(fam)))
    pairs, paired = [], set()
    for fam in families:
        if len(fam) < 2 or (mode == "unique" and len(fam) != 2):
            continue
        for i in range(len(fam)):
            for j in range(i + 1, len(fam)):
                a, b = sorted((fam[i], fam[j]), key=lambda x: (R[x], x))
                pairs.append((a, R[a], b, R[b]))
        paired.update(fam)
    stats = {"kmers_in_range": len(R), "paired": len(paired), "pairs": len(pairs),
             "families_2": sum(1 for f in families if len(f) == 2), "families_3plus": sum(1 for f in families if len(f) > 2)}
    return sorted(pairs), stats


def het_histogram(pairs, bins_minor=1002, bins_major=1002):
    """The matrix of TSXHashMapHIP.hetHistogram from het_pairs' list: numpy uint64[bins_minor, bins_major], [i, j] = the
    pairs with min(minor count, bins_minor - 1) == i and min(major count, bins_major - 1) == j."""
    if bins_minor < 2 or bins_major < 2 or bins_minor * bins_major > JOINT_MAX_CELLS:
        raise ValueError("het_histogram: 2 <= bins and bins_minor * bins_major <= 2^24")
    m = np.zeros((bins_minor, bins_major), dtype=np.uint64)
    for _, cmin, _, cmax in pairs:
        m[min(int(cmin), bins_minor - 1), min(int(cmax), bins_major - 1)] += np.uint64(1)
    return m


def bin_class(hits_a, hits_b, min_hits=1, ratio_milli=1000):
    """The class rule of the bin calls on the CPU (plain integers): a side qualifies with hits >= min_hits and wins when
    it qualifies, has more hits than the other and hits * 1000 >= ratio_milli * the other's; no side qualifies: BIN_NONE;
    nobody wins: BIN_AMBIGUOUS."""
    ha, hb, mh, rm = int(hits_a), int(hits_b), int(min_hits), int(ratio_milli)
    if not 1000 <= rm <= 1000000:
        raise ValueError("bin_class: 1000 <= ratio_milli <= 1000000")
    qa, qb = ha >= mh, hb >= mh
    if qa and ha > hb and ha * 1000 >= rm * hb:
        return BIN_A
    if qb and hb > ha and hb * 1000 >= rm * ha:
        return BIN_B
    return BIN_AMBIGUOUS if (qa or qb) else BIN_NONE


# ---- wrapped FASTA and the sequence queries -------------------------------------------------------------------------------
def fasta_records(text):
    """[(name, sequence)] of a wrapped FASTA text, with the record rules of join_fasta: split at b"\\n", empty lines
    dropped, a line whose first byte is b">" is a header, a record's sequence is every other line up to the next header
    joined, lines in front of the first header are a record with the empty name, a record without a sequence byte
    vanishes, b"\\r" and an inner b">" are ordinary bytes.  The name is the header behind b">" up to the first space or
    tab, cut to SEQ_NAME_MAX bytes.  b"".join(b">\\n" + s + b"\\n" for _, s in fasta_records(t)) == join_fasta(t)."""
    out, name, seq = [], b"", []
    for line in bytes(text).split(b"\n"):
        if not line:
            continue
        if line[:1] == b">":
            if seq:
                out.append((name, b"".join(seq)))
            seq = []
            h = line[1:]
            cut = min([i for i in (h.find(b" "), h.find(b"\t")) if i >= 0] or [len(h)])
            name = h[:min(cut, SEQ_NAME_MAX)]
        else:
            seq.append(line)
    if seq:
        out.append((name, b"".join(seq)))
    return out


def join_fasta(text):
    """The canonical two-line form of a wrapped (multi-line) FASTA text, on the CPU: the statement of the record rules
    that countFasta / unwrap_fasta follow.  The text is split at b"\\n" and empty lines are dropped; a line whose first
    byte is b">" is a header; the sequence of a record is every other line up to the next header (or the end) joined in
    order; lines in front of the first header are a record of their own; a record without a sequence byte vanishes; a
    b">" elsewhere in a line and b"\\r" are ordinary bytes.  The result is b">\\n" + sequence + b"\\n" per record:
    header text is dropped (nothing downstream of counting reads it)."""
    return b"".join(b">\n" + seq + b"\n" for _, seq in fasta_records(text))


_BASE_CODE = bytes(b"ACGT"[((b >> 1) ^ (b >> 2)) & 3] for b in range(256))   # what the table sees of a byte
_ACGT = frozenset(b"ACGTacgt")
_COMP_B = bytes.maketrans(b"ACGT", b"TGCA")


def _seq_table(D, canonical):
    """D ({k-mer bytes: count}) with its keys as the table holds them: folded through base_code, and onto the smaller
    strand when canonical."""
    T = {}
    for x, c in D.items():
        x = bytes(x).translate(_BASE_CODE)
        if canonical:
            x = min(x, x[::-1].translate(_COMP_B))
        T[x] = T.get(x, 0) + int(c)
    return T


def _seq_window_counts(seq, T, k, canonical, acgt_only):
    """Per start position of `seq`: the count of its window in T (_seq_table), or None where the base rule drops the
    window."""
    s = bytes(seq).translate(_BASE_CODE)
    bad = [0]
    for b in bytes(seq):
        bad.append(bad[-1] + (1 if (acgt_only and b not in _ACGT) else 0))
    out = []
    for i in range(len(s) - k + 1):
        if bad[i + k] - bad[i]:
            out.append(None)
            continue
        x = s[i:i + k]
        if canonical:
            x = min(x, x[::-1].translate(_COMP_B))
        out.append(T.get(x, 0))
    return out


def sequence_stats(records, D, k, lower=1, upper=None, canonical=False, acgt_only=False):
    """Per record of fasta_records: (length, kmers, present, min_count, sum_count).  kmers: the windows that are k-mers
    under the table's base rule (as queryReads); present: those whose count in D lies in lower..upper; min_count and
    sum_count as in tsx_hip_read_stats (sum modulo 2^64, min 0 without k-mers)."""
    upper = _upper(upper)
    out, tab = [], _seq_table(D, canonical)
    for _, seq in records:
        cs = [c for c in _seq_window_counts(seq, tab, k, canonical, acgt_only) if c is not None]
        out.append((len(seq), len(cs), sum(lower <= c <= upper for c in cs), min(cs) if cs else 0, sum(cs) % (1 << 64)))
    return out


def missing_intervals(records, D, k, lower=1, upper=None, canonical=False, acgt_only=False):
    """[(seq_index, start, end)]: every maximal run of consecutive start positions s..e whose windows are k-mers with a
    count outside lower..upper, as the half-open base interval [s, e + k) of the joined sequence.  A window the base
    rule drops is neither present nor missing and ends a run.  Ordered by sequence, then start."""
    upper = _upper(upper)
    out, tab = [], _seq_table(D, canonical)
    for r, (_, seq) in enumerate(records):
        start = None
        cs = _seq_window_counts(seq, tab, k, canonical, acgt_only)
        for i, c in enumerate(cs + [None]):
            miss = c is not None and not (lower <= c <= upper)
            if miss and start is None:
                start = i
            elif not miss and start is not None:
                out.append((r, start, i - 1 + k))
                start = None
    return out


def kmer_qv(present, kmers, k):
    """Merqury's consensus quality: -10 log10(1 - (present / kmers)^(1 / k)).  None without k-mers, inf when all are
    present."""
    import math
    if kmers == 0:
        return None
    if present == kmers:
        return math.inf
    if present == 0:
        return 0.0
    return -10.0 * math.log10(1.0 - (float(present) / float(kmers)) ** (1.0 / k))
