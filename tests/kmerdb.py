"""The k-mer database format (DESIGN.md §3 "K-mer database") and the slot layout restated in plain
Python and numpy, independently of the library: a reader that checks a file the way the format text lays it out, and a
writer that builds files the library never wrote.

    Layout(k, l, s)            derive_layout: R, F, W, C, K0, the LOCK bit, the default segment bits S
    encode_slot / decode_slot  the W words of one slot <-> (hashed key, reprobe count, in-slot count)
    hash_keys / inverse_rows   the mapping key bit n-1-i = parity(rows[i] & x) and its inverse by GF(2) elimination
    read_db(path, rows)        every chunk checked (tiling, end marker, checksums), {k-mer: total count}
    build_image / write_image  a table filled by sequential insertion, written with any chunk spans; a test may damage
                               the image in between and still gets valid checksums (write_db does both at once)

Hashed keys are Python ints below 2^2k; k-mers are ACGT byte strings (base j at bits 2j of the limbs, A C G T =
0 1 2 3).  Nothing here imports the library."""
import struct

import numpy as np

MAGIC = b"TSXKMERS"
VERSION = 1
HEADER_BYTES = 128
CHUNK_HEAD = 32
SALT_BM = 0x6A09E667F3BCC909     # chunk checksum, bitmap words
SALT_E = 0xBB67AE8584CAA73B      # chunk checksum, entries
M64 = (1 << 64) - 1
HEADER_FMT = "<8sII8iQ3iI6Q"     # bytes 0 .. 119; the FNV-1a 64 of them follows at byte 120
HEADER_FIELDS = ("magic", "version", "header_bytes", "k", "l", "entry_limbs", "func_bits", "reprobe_bits", "count_bits",
                 "seg_bits", "overflow_l", "hash_seed", "canonical", "acgt_only", "min_qual_char", "pad0", "kmers_added",
                 "distinct", "count_sum", "carry_records", "carry_fnv", "pad1")
_U = np.uint64


class FormatError(ValueError):
    pass


# ---- checksums ----------------------------------------------------------------------------------------------------------

def fnv1a64(data, h=0xCBF29CE484222325):
    for x in bytes(data):
        h = ((h ^ x) * 0x100000001B3) & M64
    return h


def mix64(z):
    """The splitmix64 finalizer on a uint64 array (numpy wraps uint64 arithmetic)."""
    z = np.array(z, dtype=np.uint64, ndmin=1)
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def bitmap_terms(g0, words):
    """Sum mod 2^64 of mix64(mix64(g ^ SALT_BM) ^ b) over bitmap words b with global word indices g0, g0 + 1, ..."""
    words = np.asarray(words, dtype=np.uint64)
    g = np.arange(len(words), dtype=np.uint64) + _U(g0)
    return int(mix64(mix64(g ^ _U(SALT_BM)) ^ words).sum(dtype=np.uint64))


def entry_terms(pos, ent):
    """Sum mod 2^64 over entries: h = mix64(pos ^ SALT_E), then h = mix64(h ^ e[t]) for each of the W words."""
    if not len(pos):
        return 0
    ent = np.asarray(ent, dtype=np.uint64).reshape(len(pos), -1)
    h = mix64(np.asarray(pos, dtype=np.uint64) ^ _U(SALT_E))
    for t in range(ent.shape[1]):
        h = mix64(h ^ ent[:, t])
    return int(h.sum(dtype=np.uint64))


# ---- header ------------------------------------------------------------------------------------------------------------

def pack_header(k=31, l=20, W=1, F=42, R=8, C=14, S=14, ol=16, seed=7, canonical=0, acgt=0, minq=0, added=1000,
                distinct=600, count_sum=1000, carries=0, carry_sum=None, version=1):
    """The 128-byte header; carry_sum defaults to the FNV-1a 64 of an empty carry section."""
    if carry_sum is None:
        carry_sum = fnv1a64(b"")
    b = struct.pack(HEADER_FMT, MAGIC, version, HEADER_BYTES, k, l, W, F, R, C, S, ol, seed, canonical, acgt, minq, 0,
                    added, distinct, count_sum, carries, carry_sum, 0)
    assert len(b) == 120, len(b)
    return b + struct.pack("<Q", fnv1a64(b))


def header_for(lay, seed, added, distinct, count_sum, carry_bytes, carries, canonical=0, acgt=0, minq=0):
    return pack_header(lay.k, lay.l, lay.W, lay.F, lay.R, lay.C, lay.S, lay.overflow_l, seed, canonical, acgt, minq,
                       added, distinct, count_sum, carries, fnv1a64(carry_bytes))


def parse_header(b):
    """The header as a dict (the keys of HEADER_FIELDS); FormatError when the magic, version or checksum is wrong."""
    if len(b) < HEADER_BYTES:
        raise FormatError("short header")
    d = dict(zip(HEADER_FIELDS, struct.unpack(HEADER_FMT, bytes(b[:120]))))
    if d["magic"] != MAGIC or d["version"] != VERSION or d["header_bytes"] != HEADER_BYTES:
        raise FormatError("magic / version")
    if struct.unpack("<Q", bytes(b[120:128]))[0] != fnv1a64(b[:120]):
        raise FormatError("header checksum")
    if d["pad0"] or d["pad1"]:
        raise FormatError("padding not zero")
    return d


# ---- slot layout -------------------------------------------------------------------------------------------------------

def tri(i):
    return i * (i + 1) // 2


class Layout:
    """derive_layout: R = min(l, 8) reprobe bits, F = 2k - l func bits, W limbs per slot, C counter bits (s, or the widest
    that fits when s = 0), K0 = 64 - C - (W > 1) the end of limb 0's key bits, the LOCK bit at K0 when W > 1, and the
    default segment of 2^S slots inside which probes wrap."""

    def __init__(self, k, l, s=0, seg_bits=None):
        self.k, self.l, self.s = k, l, s
        self.key_limbs = (2 * k + 63) // 64
        self.R = min(l, 8)
        self.F = 2 * k - l
        kb = self.R + self.F
        if s == 0:
            W = (kb + 5 + 63) // 64
            C = min(32, 64 * W - kb - (1 if W > 1 else 0))
        else:
            C = s
            W = (kb + C + 63) // 64
            if W > 1:
                W = (kb + C + 1 + 63) // 64
        self.W, self.C = W, C
        self.K0 = 64 - C - (1 if W > 1 else 0)
        if not (1 <= W <= 4 and self.R <= self.K0 <= 63 and kb - self.K0 <= 64 * (W - 1) and 2 * k > l):
            raise ValueError("no layout for k=%d l=%d s=%d" % (k, l, s))
        self.lock_bit = 1 << self.K0 if W > 1 else 0
        smax = 14 if W == 1 else 13 if W == 2 else 12
        self.S = min(l, 12 if (W == 2 and l - 12 <= 18) else smax) if seg_bits is None else seg_bits
        self.max_reprobes = min((1 << self.R) - 1, (1 << l) - 1)
        self.overflow_l = max(10, l - 8 if (s == 0 and C >= 16) else l - 4)
        self.slots = 1 << l
        self.f0 = min(self.F, self.K0 - self.R)          # func bits in limb 0
        self.spill = self.F - self.f0                     # func bits in limbs 1 .. W-1
        self.masks = [((1 << (self.R + self.f0)) - 1) | (((1 << C) - 1) << (64 - C))]
        for t in range(1, W):
            self.masks.append((1 << max(0, min(64, self.spill - 64 * (t - 1)))) - 1)

    def __repr__(self):
        return "Layout(k=%d, l=%d, s=%d: W=%d C=%d S=%d)" % (self.k, self.l, self.s, self.W, self.C, self.S)

    def fields(self):
        """What tsx_hip_get_layout reports."""
        return {"k": self.k, "l": self.l, "key_limbs": self.key_limbs, "entry_limbs": self.W, "func_bits": self.F,
                "reprobe_bits": self.R, "count_bits": self.C, "overflow_l": self.overflow_l,
                "max_reprobes": self.max_reprobes, "slots": self.slots, "table_bytes": self.slots * self.W * 8}

    def home(self, key):
        return key & (self.slots - 1)

    def probe(self, home, i):
        m = (1 << self.S) - 1
        return (home & ~m) | ((home + tri(i)) & m)

    def unprobe(self, pos, i):
        m = (1 << self.S) - 1
        return (pos & ~m) | ((pos - tri(i)) & m)


def encode_slot(lay, key, i, count):
    """The W words of a slot holding hashed key `key` at reprobe count i with in-slot count `count` (< 2^C)."""
    assert 0 <= count < (1 << lay.C) and 0 <= key < (1 << (2 * lay.k))
    func = key >> lay.l
    w0 = i | ((func & ((1 << lay.f0) - 1)) << lay.R) | (count << (64 - lay.C))
    rest = func >> lay.f0
    return [w0] + [(rest >> (64 * (t - 1))) & M64 for t in range(1, lay.W)]


def decode_slot(lay, pos, words):
    """(hashed key, reprobe count, in-slot count, stray) of the words of slot `pos`; stray[t] = the bits of word t that
    lie outside every field (the LOCK bit included)."""
    w0 = int(words[0])
    i = w0 & ((1 << lay.R) - 1)
    func = (w0 >> lay.R) & ((1 << lay.f0) - 1)
    for t in range(1, lay.W):
        func |= (int(words[t]) & lay.masks[t]) << (lay.f0 + 64 * (t - 1))
    key = (func << lay.l) | lay.unprobe(pos, i)
    stray = [int(w) & ~m & M64 for w, m in zip(words, lay.masks)]
    return key, i, w0 >> (64 - lay.C), stray


# ---- the mapping ---------------------------------------------------------------------------------------------------------

def kmers_to_limbs(kmers, k):
    """ACGT byte strings -> (n, key_limbs) uint64."""
    wk = (2 * k + 63) // 64
    if not len(kmers):
        return np.zeros((0, wk), dtype=np.uint64)
    a = np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(len(kmers), k)
    code = np.full(256, 255, dtype=np.uint8)
    code[list(b"ACGT")] = [0, 1, 2, 3]
    c = code[a]
    assert (c < 4).all(), "ACGT k-mers only"
    out = np.zeros((len(kmers), wk), dtype=np.uint64)
    for j in range(k):
        out[:, j // 32] |= c[:, j].astype(np.uint64) << _U(2 * (j % 32))
    return out


def limbs_to_kmers(x, k):
    x = np.asarray(x, dtype=np.uint64).reshape(-1, (2 * k + 63) // 64)
    c = np.empty((len(x), k), dtype=np.uint8)
    for j in range(k):
        c[:, j] = ((x[:, j // 32] >> _U(2 * (j % 32))) & _U(3)).astype(np.uint8)
    return np.ascontiguousarray(np.frombuffer(b"ACGT", dtype=np.uint8)[c]).view("S%d" % k).ravel().tolist()


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def hash_keys(rows, x, k):
    """key bit n-1-i = parity(rows[i] & x), n = 2k, for (m, key_limbs) k-mers (tsx_hip_hash_rows' rows)."""
    n = 2 * k
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(len(x), -1)
    out = np.zeros_like(x)
    for i in range(n):
        par = np.zeros(len(x), dtype=np.uint64)
        for t in range(x.shape[1]):
            par += np.bitwise_count(x[:, t] & rows[i, t])
        b = n - 1 - i
        out[:, b // 64] |= (par & _U(1)) << _U(b % 64)
    return out


def inverse_rows(rows, k):
    """Rows of the inverse mapping (x bit n-1-i = parity(inv[i] & key)) by Gaussian elimination over GF(2)."""
    n, wk = 2 * k, rows.shape[1]
    as_int = lambda r: sum(int(r[t]) << (64 * t) for t in range(wk))
    a = [as_int(rows[n - 1 - b]) for b in range(n)]       # a[b]: key bit b = parity(a[b] & x)
    inv = [1 << b for b in range(n)]
    for c in range(n):
        p = next((r for r in range(c, n) if (a[r] >> c) & 1), None)
        if p is None:
            raise ValueError("the rows are singular")
        a[c], a[p] = a[p], a[c]
        inv[c], inv[p] = inv[p], inv[c]
        for r in range(n):
            if r != c and (a[r] >> c) & 1:
                a[r] ^= a[c]
                inv[r] ^= inv[c]
    out = np.zeros((n, wk), dtype=np.uint64)
    for b in range(n):                                    # x bit b = parity(inv[b] & key)
        for t in range(wk):
            out[n - 1 - b, t] = (inv[b] >> (64 * t)) & M64
    return out


def keys_to_ints(h):
    h = np.asarray(h, dtype=np.uint64)
    return [sum(int(v) << (64 * t) for t, v in enumerate(r)) for r in h]


def ints_to_limbs(keys, wk):
    out = np.zeros((len(keys), wk), dtype=np.uint64)
    for j, v in enumerate(keys):
        for t in range(wk):
            out[j, t] = (v >> (64 * t)) & M64
    return out


def table_keys(kmers, rows, k, canonical=False):
    """The hashed key each k-mer is counted under: h(x), or min(h(x), h(rc x)) in a canonical table."""
    h = keys_to_ints(hash_keys(rows, kmers_to_limbs(kmers, k), k))
    if canonical:
        hr = keys_to_ints(hash_keys(rows, kmers_to_limbs([revcomp(s) for s in kmers], k), k))
        h = [min(a, b) for a, b in zip(h, hr)]
    return h


def keys_to_kmers(keys, inv, k):
    return limbs_to_kmers(hash_keys(inv, ints_to_limbs(keys, (2 * k + 63) // 64), k), k)


def fold_strands(counts):
    """{k-mer: count} summed per strand pair, keyed by the lexicographically smaller strand."""
    out = {}
    for s, c in counts.items():
        r = revcomp(s)
        key = min(s, r)
        out[key] = out.get(key, 0) + c
    return out


# ---- reading -------------------------------------------------------------------------------------------------------------

class DbFile:
    """What read_db found: header (dict), layout, carries [(pos, carry, words)], chunks [(lo, hi, n, checksum)],
    entries {pos: words}, keys {hashed key: total count}, kmers {k-mer: total count} (when rows were given)."""


BM_PIECE = 1 << 20   # bitmap words per read: a 1 GiB bitmap is never held at once


def read_db(path, rows=None):
    with open(path, "rb") as f:
        return _read(f, rows)


def _read_exact(f, n, what):
    b = f.read(n)
    if len(b) != n:
        raise FormatError("truncated (%s)" % what)
    return b


def _read(f, rows):
    h = parse_header(_read_exact(f, HEADER_BYTES, "header"))
    k, l, W, C = h["k"], h["l"], h["entry_limbs"], h["count_bits"]
    # W and C place the fields (K0 = 64 - C - (W > 1)): any storage-bits value that gives both describes the slot
    lay = next((x for x in (Layout(k, l, s, seg_bits=h["seg_bits"]) for s in range(0, 33) if _fits(k, l, s))
                if x.C == C and x.W == W), None)
    if lay is None or lay.F != h["func_bits"] or lay.R != h["reprobe_bits"]:
        raise FormatError("no slot layout with W=%d C=%d" % (W, C))
    slots = 1 << l
    raw = _read_exact(f, h["carry_records"] * (2 + W) * 8, "carry records")
    if fnv1a64(raw) != h["carry_fnv"]:
        raise FormatError("carry section checksum")
    rec = np.frombuffer(raw, dtype=np.uint64).reshape(-1, 2 + W)
    carries = [(int(r[0]), int(r[1]), tuple(int(v) for v in r[2:])) for r in rec]
    cpos = [c[0] for c in carries]
    if any(b <= a for a, b in zip(cpos, cpos[1:])):
        raise FormatError("carry records not sorted by slot or not unique")
    db = DbFile()
    db.header, db.layout, db.carries, db.chunks, db.entries = h, lay, carries, [], {}
    lo_expect = 0
    while True:
        lo, hi, n, cs = struct.unpack("<4Q", _read_exact(f, CHUNK_HEAD, "no end marker"))
        if lo != lo_expect or hi > slots or lo > hi:
            raise FormatError("chunks do not tile [0, 2^l): %d %d" % (lo, hi))
        if lo == hi:
            if lo != slots or n != 0:
                raise FormatError("bad end marker")
            break
        if (hi - lo) % 64 and hi != slots:
            raise FormatError("chunk span not a multiple of 64")
        lo_expect = hi
        nbm = (hi - lo + 63) // 64
        s = 0
        pos = []
        for w0 in range(0, nbm, BM_PIECE):
            bm = np.frombuffer(_read_exact(f, 8 * min(BM_PIECE, nbm - w0), "bitmap"), dtype=np.uint64)
            s += bitmap_terms(lo // 64 + w0, bm)
            nz = np.flatnonzero(bm)
            if len(nz):
                bits = np.unpackbits(bm[nz].view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
                wi, bi = np.nonzero(bits)
                pos.append(_U(lo) + (nz[wi].astype(np.uint64) + _U(w0)) * _U(64) + bi.astype(np.uint64))
        pos = np.concatenate(pos) if pos else np.zeros(0, np.uint64)
        if len(pos) != n:
            raise FormatError("bitmap holds %d entries, the chunk head says %d" % (len(pos), n))
        if len(pos) and int(pos[-1]) >= hi:
            raise FormatError("bitmap bit past the chunk")
        ent = np.frombuffer(_read_exact(f, 8 * n * W, "entries"), dtype=np.uint64).reshape(n, W)
        s += entry_terms(pos, ent)
        if s & M64 != cs:
            raise FormatError("chunk [%d, %d) checksum" % (lo, hi))
        db.chunks.append((lo, hi, n, cs))
        for p, e in zip(pos.tolist(), ent.tolist()):
            db.entries[p] = tuple(e)
    if f.read(1):
        raise FormatError("bytes after the end marker")
    carry_of = {}
    for p, c, words in carries:
        if db.entries.get(p) != words:
            raise FormatError("carry record at %d does not match the entry there" % p)
        carry_of[p] = c
    db.keys = {}
    for p, words in db.entries.items():
        key, i, cnt, stray = decode_slot(lay, p, words)
        if any(stray):
            raise FormatError("bits outside the slot fields at %d" % p)
        if not 1 <= i <= lay.max_reprobes:
            raise FormatError("reprobe count %d at %d" % (i, p))
        total = cnt + (carry_of.get(p, 0) << C)
        if total == 0:
            raise FormatError("entry with count 0 at %d" % p)
        if key in db.keys:
            raise FormatError("key stored twice")
        db.keys[key] = total
    if len(db.entries) != h["distinct"] or sum(db.keys.values()) != h["count_sum"]:
        raise FormatError("header totals")
    if rows is not None:
        keys = list(db.keys)
        db.kmers = dict(zip(keys_to_kmers(keys, inverse_rows(rows, k), k), db.keys.values()))
    return db


def _fits(k, l, s):
    try:
        Layout(k, l, s)
        return True
    except ValueError:
        return False


# ---- writing -------------------------------------------------------------------------------------------------------------

class Image:
    """A database before it is written: header values, the table {pos: [W words]}, carry records [[pos, carry, words]],
    chunk spans [(lo, hi)], and per-chunk adjustments of n_entries.  A test may change any of it: write_image computes
    every checksum over what it writes."""


def build_image(counts, lay, rows, seed, canonical=False, acgt_only=0, min_qual_char=0, kmers_added=None, chunks=None):
    """The table that sequential insertion of `counts` ({k-mer: count}, sorted by hashed key) builds under the
    placement rule: probes i = 1, 2, ... from the home slot inside its segment, the first empty one taken, the count's
    low C bits in the slot and a carry record for count >> C."""
    img = Image()
    img.layout, img.seed = lay, seed
    img.canonical, img.acgt_only, img.min_qual_char = int(canonical), int(acgt_only), int(min_qual_char)
    kmers = list(counts)
    keys = table_keys(kmers, rows, lay.k, canonical)
    by_key = {}
    for key, s in zip(keys, kmers):
        by_key[key] = by_key.get(key, 0) + counts[s]
    img.slots, img.place, img.carries = {}, {}, []
    for key in sorted(by_key):
        c = by_key[key]
        home = lay.home(key)
        for i in range(1, lay.max_reprobes + 1):
            p = lay.probe(home, i)
            if p not in img.slots:
                break
        else:
            raise ValueError("out of reprobes")
        img.slots[p] = encode_slot(lay, key, i, c & ((1 << lay.C) - 1))
        img.place[key] = p
        if c >> lay.C:
            img.carries.append([p, c >> lay.C, None])
    img.carries.sort()
    img.kmer_slot = {s: img.place[key] for s, key in zip(kmers, keys)}
    img.count_sum = sum(by_key.values())
    img.kmers_added = img.count_sum if kmers_added is None else kmers_added
    img.distinct = None
    img.chunks = [(0, lay.slots)] if chunks is None else list(chunks)
    img.n_adjust = {}
    return img


def spans(slots, sizes):
    """Chunk spans [(lo, hi)] of the given sizes, repeated, the last one cut at `slots`."""
    out, lo, j = [], 0, 0
    while lo < slots:
        hi = min(slots, lo + sizes[j % len(sizes)])
        out.append((lo, hi))
        lo, j = hi, j + 1
    return out


def write_image(path, img):
    lay = img.layout
    W = lay.W
    rec = []
    for p, c, words in img.carries:
        rec += [p, c] + list(img.slots[p] if words is None else words)
    carry_bytes = np.array(rec, dtype=np.uint64).tobytes()
    distinct = len(img.slots) if img.distinct is None else img.distinct
    out = [header_for(lay, img.seed, img.kmers_added, distinct, img.count_sum, carry_bytes, len(img.carries),
                      img.canonical, img.acgt_only, img.min_qual_char), carry_bytes]
    occupied = sorted(img.slots)
    for ci, (lo, hi) in enumerate(img.chunks):
        nbm = (hi - lo + 63) // 64
        a, b = np.searchsorted(occupied, [lo, lo + 64 * nbm])   # (a bit past hi is the caller's damage)
        pos = np.array(occupied[a:b], dtype=np.uint64)
        bm = np.zeros(nbm, dtype=np.uint64)
        np.bitwise_or.at(bm, ((pos - _U(lo)) >> _U(6)).astype(np.int64), _U(1) << (pos & _U(63)))
        ent = np.array([img.slots[int(p)] for p in pos], dtype=np.uint64).reshape(len(pos), W)
        cs = (bitmap_terms(lo // 64, bm) + entry_terms(pos, ent)) & M64
        out += [struct.pack("<4Q", lo, hi, len(pos) + img.n_adjust.get(ci, 0), cs), bm.tobytes(), ent.tobytes()]
    out.append(struct.pack("<4Q", lay.slots, lay.slots, 0, 0))
    with open(path, "wb") as f:
        f.write(b"".join(out))


def write_db(path, counts, lay, rows, seed, **kw):
    """build_image + write_image: returns the image (img.kmer_slot: where each k-mer was placed)."""
    img = build_image(counts, lay, rows, seed, **kw)
    write_image(path, img)
    return img
