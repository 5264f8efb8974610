"""A deflate (RFC 1951) and BGZF writer for the tests of the device inflate (tsxcount_amd/csrc/tsx_inflate.h).

zlib's encoder writes a small part of what a deflate stream may hold; this writer puts down bit by bit whatever a case
names: the block type, the two codes by their lengths, how the lengths are themselves coded, every symbol with its
extra bits.  It checks nothing unless asked to, so malformed streams are written the same way.  The expectation of a
test is never what the writer intended but what zlib's decoder makes of the bytes (tests/test_inflate_streams_cpu.py
shows that the two agree)."""
import struct
import zlib

EOB = 256
CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32          # 30 and 31 have a code and no meaning


class BitWriter:
    """Bits go into a byte from its least significant end (RFC 1951 section 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        """n bits of value, least significant first (every field except a Huffman code)."""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 256:
            whole = self.n >> 3
            self.out += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.n -= 8 * whole

    def code(self, code, n):
        """A Huffman code of n bits, most significant first."""
        self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.bits(0, -self.bitpos % 8)

    def raw(self, data):
        assert self.bitpos % 8 == 0
        for b in data:
            self.bits(b, 8)

    def getvalue(self):
        """The bytes so far, the last one filled up with zero bits."""
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def canonical_codes(lengths):
    """The code of every symbol from the lengths alone (RFC 1951 section 3.2.2); None for length 0."""
    count = [0] * (max(lengths) + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * len(count), 0
    for l in range(1, len(count)):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else None)
        nxt[l] += 1 if l else 0
    return out


def kraft(lengths):
    """Sum of 2^-length in units of 2^-15: 32768 for a complete code, more for an over-subscribed one."""
    return sum(1 << (15 - l) for l in lengths if l)


def flat_lengths(n, used=None, rng=None):
    """A complete code over `used` (default: all) of n symbols, lengths differing by at most one; which symbols get
    the shorter codes is drawn from rng.  One used symbol gets a second one beside it: a complete code needs two."""
    used = sorted(range(n) if used is None else set(used))
    if len(used) == 1:
        used = sorted(set(used) | {0 if used[0] else 1})
    m = len(used)
    k = m.bit_length() - 1
    short = (2 << k) - m               # that many codes of k bits, the rest of k + 1
    if rng is not None:
        used = list(used)
        rng.shuffle(used)
    out = [0] * n
    for i, s in enumerate(used):
        out[s] = k if i < short else k + 1
    return out


def length_symbol(length):
    """(symbol - 257, extra value) as zlib writes a length: 258 is symbol 285."""
    if length == 258:
        return 28, 0
    s = max(i for i in range(28) if LBASE[i] <= length)
    return s, length - LBASE[s]


def distance_symbol(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, dist - DBASE[s]


_REV = {}


def _rev_codes(lengths):
    """(codes with their bits reversed, ready for BitWriter.bits; lengths), kept per code: a test writes thousands
    of blocks with the same few codes."""
    key = tuple(lengths)
    if key not in _REV:
        _REV[key] = ([None if c is None else int(format(c, "0%db" % l)[::-1], 2)
                      for c, l in zip(canonical_codes(key), key)] if any(key) else [None] * len(key), key)
    return _REV[key]


def put_symbols(w, symbols, lit_lengths, dist_lengths):
    """Symbols: 0..255 a literal, EOB, any other int a bare literal/length symbol without what should follow it,
    (length, distance), (length, distance, length symbol) to force e.g. 284 with extra 31 for 258, and
    ("raw", length symbol, extra value, distance symbol, extra value) for symbols that mean nothing."""
    lc, ll = _rev_codes(lit_lengths)
    dc, dl = _rev_codes(dist_lengths)
    acc, n = 0, 0
    for s in symbols:
        if isinstance(s, int):
            acc |= lc[s] << n
            n += ll[s]
            continue
        if s[0] == "raw":
            _, ls, lx, ds, dx = s
            ls -= 257
        else:
            ls, lx = length_symbol(s[0])
            if len(s) > 2:
                ls, lx = s[2] - 257, s[0] - LBASE[s[2] - 257]
            ds, dx = distance_symbol(s[1])
        acc |= lc[257 + ls] << n
        n += ll[257 + ls]
        if ls < 29:
            acc |= lx << n
            n += LEXT[ls]
        acc |= dc[ds] << n
        n += dl[ds]
        if ds < 30:
            acc |= dx << n
            n += DEXT[ds]
    w.bits(acc, n)


def stored(w, data, final, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    w.raw(data)


def fixed(w, symbols, final):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_symbols(w, symbols, FIXED_LIT, FIXED_DIST)


def plain_plan(lengths):
    return list(lengths)


def run_plan(lengths):
    """The lengths coded as zlib would: 17 and 18 for runs of zeros, 16 for repeats of the length before."""
    ops, i = [], 0
    while i < len(lengths):
        j = i
        while j < len(lengths) and lengths[j] == lengths[i]:
            j += 1
        run, v = j - i, lengths[i]
        if v == 0:
            while run >= 11:
                ops.append((18, min(run, 138))); run -= min(run, 138)
            if run >= 3:
                ops.append((17, run)); run = 0
        else:
            ops.append(v); run -= 1
            while run >= 3:
                ops.append((16, min(run, 6))); run -= min(run, 6)
        ops += [v] * run
        i = j
    return ops


def expand_plan(ops):
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            out += [out[-1] if op[0] == 16 else 0] * op[1]
    return out


_HEADERS = {}


def dynamic(w, lit_lengths, dist_lengths, symbols, final, clen_plan=None):
    """A dynamic block.  HLIT and HDIST are the lengths of the two lists.  clen_plan: None (every length coded as
    itself) or a dict with any of
      ops         the code lengths as a list of 0..15 and (16 | 17 | 18, repeat count); it is written as given, so a
                  run may cross from the literal into the distance lengths, or not add up to HLIT + HDIST at all;
      cl_lengths  the 19 lengths of the code-length code (default: a flat code over the symbols the ops use);
      hclen       how many of them are written, in CLORDER (default: up to the last that is not zero, at least 4)."""
    key = (tuple(lit_lengths), tuple(dist_lengths), repr(clen_plan))
    if key not in _HEADERS:
        plan = clen_plan or {}
        ops = plan.get("ops", plain_plan(list(lit_lengths) + list(dist_lengths)))
        cl = plan.get("cl_lengths") or flat_lengths(19, [op if isinstance(op, int) else op[0] for op in ops])
        hclen = plan.get("hclen") or max(4, max(i + 1 for i in range(19) if cl[CLORDER[i]]))
        h = BitWriter()
        h.bits(2, 2)
        h.bits(len(lit_lengths) - 257, 5)
        h.bits(len(dist_lengths) - 1, 5)
        h.bits(hclen - 4, 4)
        for i in range(hclen):
            h.bits(cl[CLORDER[i]], 3)
        cc = canonical_codes(cl)
        for op in ops:
            s = op if isinstance(op, int) else op[0]
            h.code(cc[s], cl[s])
            if s == 16:
                h.bits(op[1] - 3, 2)
            elif s == 17:
                h.bits(op[1] - 3, 3)
            elif s == 18:
                h.bits(op[1] - 11, 7)
        _HEADERS[key] = (int.from_bytes(h.getvalue(), "little"), h.bitpos)   # the same few headers, thousands of times
    w.bits(1 if final else 0, 1)
    w.bits(*_HEADERS[key])
    put_symbols(w, symbols, lit_lengths, dist_lengths)


def lz_symbols(data, start=0, min_match=3, max_dist=32768):
    """A plain greedy LZ77 parse of data[start:] into literals and (length, distance): the last place the next three
    bytes were seen (data[:start], the blocks before, included), extended as far as it goes.  No EOB at the end."""
    out, last, i, n = [], {data[t:t + 3]: t for t in range(max(0, start - 2))}, start, len(data)
    while i < n:
        key = data[i:i + 3]
        j = last.get(key, -1)
        last[key] = i
        if len(key) == 3 and j >= 0 and i - j <= max_dist:
            m = 3
            while m < 258 and i + m < n and data[j + m] == data[i + m]:
                m += 1
            if m >= min_match:
                out.append((m, i - j))
                for t in range(i + 1, min(i + m, n - 2)):
                    last[data[t:t + 3]] = t
                i += m
                continue
        out.append(data[i])
        i += 1
    return out


def bgzf_member(raw, text, before=b"", after=b"", crc=None, isize=None, flags=4, bsize=None):
    """One BGZF member around the deflate data `raw`: gzip header with the BC subfield (BSIZE = member size - 1), raw,
    CRC-32 and ISIZE of `text`.  before / after: bytes of the extra field in front of and behind BC (other subfields,
    or padding that XLEN counts and no subfield holds); crc, isize, flags, bsize: written instead of the right value."""
    extra = before + b"BC" + struct.pack("<H", 2)
    xlen = len(extra) + 2 + len(after)
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536 or bsize is not None, "a BGZF member holds at most 64 KiB, header and trailer included"
    extra += struct.pack("<H", total - 1 if bsize is None else bsize) + after
    return (b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra + bytes(raw) +
            struct.pack("<II", (zlib.crc32(text) & 0xFFFFFFFF) if crc is None else crc, len(text) if isize is None else isize))


EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_file(members):
    return b"".join(members) + EOF_MEMBER
