"""The deflate streams that test_inflate_streams_cpu.py (is the writer right?) and test_inflate_streams.py (is the device
inflate right?) share: families of crafted BGZF members, each a Case(name, raw deflate data, the text the writer meant),
and the malformed ones, each a Bad(name, raw, text of the trailer, reason the library gives, crc, isize).

Everything is generated from seeds.  Two things the BGZF format rules out are replaced by the nearest thing it
allows: a member is at most 65536 bytes with header and trailer (BSIZE has 16 bits), so the largest stored block in a
member has 65505 bytes, not 65535, and a "stored" member of 65535 or 65536 bytes of text is a short fixed block (a run)
followed by one stored block; and with HCLEN = 4 only the code-length symbols 16, 17, 18 and 0 have a code, every
length is then zero and there is no end-of-block code, so the smallest HCLEN of a valid block is 5 (HCLEN = 4 is
among the refusals)."""
import random
import zlib
from collections import namedtuple

from deflate_writer import (EOB, BitWriter, DBASE, bgzf_member, dynamic, fixed, flat_lengths, lz_symbols, run_plan, stored)

Case = namedtuple("Case", "name raw text")
Bad = namedtuple("Bad", "name raw text reason crc isize")

NOISE = random.Random(1951).randbytes(70000)          # literals: no period, so a copy from a wrong place shows


def _dyn_code(seed):
    rng = random.Random(seed)
    return flat_lengths(286, rng=rng), flat_lengths(30, rng=rng)


DYN = [_dyn_code(s) for s in range(4)]                # complete 8/9-bit and 4/5-bit codes, shuffled four ways


def render(symbols, out):
    """What the symbols mean, appended to the bytearray out (which is the history of a match)."""
    for s in symbols:
        if isinstance(s, int):
            if s < 256:
                out.append(s)
            continue
        length, dist = s[0], s[1]
        seg = bytes(out[-dist:])
        out += (seg * (length // dist + 1))[:length]


class Member:
    """The blocks of one member, written and rendered side by side."""

    def __init__(self):
        self.w, self.text = BitWriter(), bytearray()

    def fixed(self, symbols, final=False):
        fixed(self.w, symbols, final)
        render(symbols, self.text)
        return self

    def dynamic(self, lit, dist, symbols, final=False, plan=None):
        dynamic(self.w, lit, dist, symbols, final, plan)
        render(symbols, self.text)
        return self

    def block(self, kind, symbols, final=False, code=0):
        """kind "fixed", or "dynamic" with one of the four DYN codes, its lengths coded plainly or with repeats."""
        if kind == "fixed":
            return self.fixed(symbols, final)
        lit, dist = DYN[code % 4]
        return self.dynamic(lit, dist, symbols, final, {"ops": run_plan(lit + dist)} if code & 4 else None)

    def stored(self, data, final=False):
        stored(self.w, data, final)
        self.text += data
        return self

    def case(self, name):
        return Case(name, self.w.getvalue(), bytes(self.text))


def member_of(case, **kw):
    return bgzf_member(case.raw, case.text, **kw)


# ---- one match between literals ---------------------------------------------------------------------------------------

DISTS = list(range(1, 41)) + [63, 64, 65, 255, 256, 257]
LENS = [3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 258]
TAILS = [0, 1, 7, 8, 9, 55, 56, 63, 64, 65]


def match_matrix(kind):
    """p literals, (len, dist), t literals: which copy path of the kernel a match takes depends on dist, len, the
    position p and what is left of the member behind it.  Then two members with 32768 literals in front."""
    cases, n = [], 0
    for dist in DISTS:
        for p in sorted({dist, 7, 8, 9, dist + 8}):
            if p < dist:
                continue
            for length in LENS:
                for t in TAILS:
                    off = (n * 37) % 60000
                    n += 1
                    syms = list(NOISE[off:off + p]) + [(length, dist)] + list(NOISE[off + p:off + p + t]) + [EOB]
                    cases.append(Member().block(kind, syms, True, n).case("%s p=%d len=%d dist=%d t=%d" % (kind, p, length, dist, t)))
    far = list(NOISE[:32768])
    cases.append(Member().block(kind, far + [(258, 32768), 1, 2, 3, (33, 32767), (64, 32768), 4, 5, 6, 7, 8, (3, 32767), (9, 32768)]
                                + list(NOISE[40000:40009]) + [EOB], True, 1).case(kind + " distances 32767 and 32768"))
    cases.append(Member().block(kind, far + [(258, 24577), (40, 24577), 9, (17, 24578), (31, 32768), (8, 32767), 10, EOB], True, 6)
                 .case(kind + " distance 24577, the first of the last distance symbol"))
    return cases


# ---- match, r literals, match ----------------------------------------------------------------------------------------

def match_runs():
    """The second match reads the last bytes of the first and the literals between them: literals that wait in a
    register, or a landing store that runs past its match, show here.  A tail of 70 keeps the fast paths open, a
    tail of 2 is the end of the member.  Fixed and dynamic blocks take turns."""
    cases, n = [], 0
    for d1 in range(1, 13):
        for d2 in range(1, 13):
            for r in range(18):
                for l1 in (3, 10, 21):
                    for l2 in (5, 20):
                        for t in (2, 70):
                            off = (n * 41) % 60000
                            n += 1
                            syms = (list(NOISE[off:off + 12]) + [(l1, d1)] + list(NOISE[off + 12:off + 12 + r]) + [(l2, d2)]
                                    + list(NOISE[off + 30:off + 30 + t]) + [EOB])
                            cases.append(Member().block(("fixed", "dynamic")[n & 1], syms, True, n >> 1)
                                         .case("match (%d, %d), %d literals, match (%d, %d), tail %d" % (l1, d1, r, l2, d2, t)))
    return cases


def block_end_runs():
    """r literals at the end of a block, and then every kind of block behind them."""
    cases, n = [], 0
    for r in range(18):
        for first in ("fixed", "dynamic"):
            for nxt in ("stored", "fixed", "dynamic", "empty fixed"):
                for length, dist in ((7, 1), (13, 1), (7, 5), (13, 5), (7, 9), (13, 9)):
                    off = (n * 43) % 60000
                    n += 1
                    m = Member().block(first, list(NOISE[off:off + 12]) + [(length, dist)] + list(NOISE[off + 12:off + 12 + r]) + [EOB], False, n)
                    if nxt == "stored":
                        m.stored(NOISE[off + 40:off + 45], True)
                    elif nxt == "empty fixed":
                        m.fixed([EOB], True)
                    else:
                        m.block(nxt, [(4, 3), NOISE[off + 50], (9, 2 + r), EOB], True, n + 1)
                    cases.append(m.case("%s block ends with (%d, %d) and %d literals, then a %s block" % (first, length, dist, r, nxt)))
    return cases


# ---- code shapes ------------------------------------------------------------------------------------------------------

def _lengths(n, pairs):
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


FAM_LIT = [0] * 65 + [4] * 8 + [0] * 183 + [2, 3, 3]       # A..H four bits, end-of-block two, lengths 3 and 4 three bits
FAM_DIST = [2, 2, 2, 2]
FAM_SYMS = list(range(65, 73)) + [(3, 1), (4, 4), 66, EOB]
_Z65, _F8, _Z183, _T, _D = [0] * 65, [4] * 8, [0] * 183, [2, 3, 3], [2, 2, 2, 2]


def _fam(name, ops):
    return Member().dynamic(FAM_LIT, FAM_DIST, FAM_SYMS, True, {"ops": ops}).case(name)


def code_shapes():
    cases = []
    ramp = list(range(1, 15)) + [15, 15]                     # a complete code with every length from 1 to 15
    lit = _lengths(259, zip(list(range(97, 111)) + [256, 258], ramp))
    syms = list(range(97, 111)) + [(4, 3), 110, 97, EOB]
    cases.append(Member().dynamic(lit, FAM_DIST, syms, True).case("literal code of 1..15 bits, HCLEN 19"))
    lit = _lengths(259, zip([256, 258] + list(range(97, 111)), ramp))
    cases.append(Member().dynamic(lit, FAM_DIST, syms, True).case("literal code of 1..15 bits, the literals long"))
    m = Member().dynamic(DYN[0][0], ramp, list(NOISE[:200]) + [(3 + s, DBASE[s]) for s in range(16)] + [7, EOB], True)
    cases.append(m.case("distance code of 1..15 bits"))
    for kind in ("fixed", "dynamic"):
        cases.append(Member().block(kind, [65, (258, 1, 284), 66, EOB], True).case(kind + " length 258 as symbol 284 + 31"))
        cases.append(Member().block(kind, [65, (258, 1), 66, EOB], True).case(kind + " length 258 as symbol 285" + (", HLIT 286, HDIST 30" if kind == "dynamic" else "")))
    lit = flat_lengths(257, list(range(65, 73)) + [256])
    cases.append(Member().dynamic(lit, [0], list(b"ABCDEFGHHGFEDCBA") + [EOB], True).case("HLIT 257, no distance code, literals only"))
    lit = flat_lengths(260, [65, 66, 256, 259])
    cases.append(Member().dynamic(lit, [1], [65, (5, 1), 66, (5, 1), EOB], True).case("HDIST 1: one distance code of one bit"))
    cases.append(Member().dynamic(lit, [0, 0, 1], [65, 66, 65, (5, 3), 66, (5, 3), EOB], True).case("one distance code of one bit, distance 3"))
    lit = [0] + [8] * 256                                    # 256 codes of eight bits: the code-length symbols 0, 8 and 16 do
    ops = [0, 8] + [(16, 6)] * 42 + [8, 8, 8] + [0]
    cases.append(Member().dynamic(lit, [0], list(NOISE[100:140].replace(b"\0", b"\1")) + [EOB], True, {"ops": ops}).case("HCLEN 5, the smallest of a valid block"))
    cases.append(_fam("code 16 with a repeat of 3", _Z65 + [4, (16, 3), 4, (16, 3)] + _Z183 + _T + _D))
    cases.append(_fam("code 16 with a repeat of 6", _Z65 + [4, (16, 6), 4] + _Z183 + _T + _D))
    cases.append(_fam("code 16 repeats a zero", [0, (16, 6)] * 9 + [0, 0] + _F8 + _Z183 + _T + _D))
    cases.append(_fam("code 17 with 3", [(17, 3), (18, 62)] + _F8 + run_plan(_Z183) + _T + _D))
    cases.append(_fam("code 17 with 10", [(17, 10), (18, 55)] + _F8 + run_plan(_Z183) + _T + _D))
    cases.append(_fam("code 18 with 11", [(18, 11), (18, 54)] + _F8 + run_plan(_Z183) + _T + _D))
    cases.append(_fam("code 18 with 138", _Z65 + _F8 + [(18, 138), (18, 45)] + _T + _D))
    lit = [0] * 65 + [4] * 8 + [0] * 183 + [3, 3, 3, 3]
    ops = _Z65 + _F8 + run_plan(_Z183) + [3, (16, 6), (16, 5)]
    cases.append(Member().dynamic(lit, [3] * 8, FAM_SYMS[:-1] + [(5, 8), EOB], True, {"ops": ops})
                 .case("a code-16 repeat that runs from the literal into the distance lengths"))
    lit = FAM_LIT + [0] * 10
    ops = _Z65 + _F8 + run_plan(_Z183) + _T + [(18, 13), 2, 2, 2, 2]
    cases.append(Member().dynamic(lit, [0, 0, 0, 2, 2, 2, 2], list(range(65, 73)) + [(3, 4), (4, 5), (3, 7), EOB], True, {"ops": ops})
                 .case("a code-18 repeat that runs from the literal into the distance lengths"))
    only_eob = [0] * 256 + [1]
    cases.append(Member().fixed([72, 105, EOB]).dynamic(only_eob, [0], [EOB], True).case("a dynamic block holding only end-of-block, one code of one bit"))
    cases.append(Member().dynamic(only_eob, [0], [EOB], True).case("an empty member of one dynamic block"))
    cases.append(Member().dynamic(_lengths(257, [(0, 1), (256, 1)]), [0], [EOB]).fixed([72, EOB], True).case("a dynamic block holding only end-of-block, two codes"))
    for k in range(8):                                       # a literal of nine bits moves everything behind it by one bit
        head = [200] * k + [65, 66, 67, EOB]
        cases.append(Member().fixed(head).stored(b"").fixed([(3, 3), 68, EOB], True).case("a stored block of length 0 at bit offset %d" % ((2 + k) % 8)))
        cases.append(Member().fixed(head).stored(b"xyz12").fixed([(6, 7), 68, EOB], True).case("a stored block of 5 bytes at bit offset %d" % ((2 + k) % 8)))
        cases.append(Member().block("dynamic", head, False, k).stored(b"").stored(b"q").block("dynamic", [(3, 3), 68, EOB], True, k + 4)
                     .case("stored blocks behind a dynamic block, %d literals" % k))
    cases.append(Member().stored(NOISE[:65505], True).case("the largest stored block of a member, 65505 bytes"))
    return cases


# ---- member sizes -----------------------------------------------------------------------------------------------------

def _reads_text(n, seed):
    """Lines drawn from a small pool: long matches at small and large distances."""
    rng = random.Random(seed)
    pool = [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(20, 120))) + b"\n" for _ in range(150)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(pool)
    return bytes(out[:n])


SIZES = list(range(131)) + [65535, 65536]


def member_sizes(kind):
    """Every size around the CRC's 32-byte steps, its prefetch of the next 32 and its byte tail, and the largest two."""
    text, cases = _reads_text(65536, 7), []
    for n in SIZES:
        t = text[n:2 * n] if n <= 130 else text[:n]
        m = Member()
        if kind != "stored":
            m.block(kind, lz_symbols(t) + [EOB], True, n)
        elif n <= 130:
            m.stored(t, True)
        else:
            m.fixed(lz_symbols(b"A" * 4096) + [EOB]).stored(NOISE[:n - 4096], True)
        cases.append(m.case("%s member of %d bytes" % (kind, n)))
    return cases


# ---- zlib's encoders --------------------------------------------------------------------------------------------------

def encoder_texts():
    from tsxcount_amd import synth
    return {"fastq": synth.fastq(29, 0, 130), "low entropy": (b"ACGTTGCA" * 7 + b"\n") * 3600,
            "random": random.Random(3).randbytes(210000)}


def encoder_cases(size, texts):
    """Members of `size` bytes from every strategy, memLevel 1, 8, 9 and level 1, 6, 9 of zlib's encoder, and the default
    one again with a sync and a full flush inside the member.  A chunk that does not compress into a member (random
    bytes in the small blocks of memLevel 1) is cut by 1 KiB until it does."""
    strategies = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman only": zlib.Z_HUFFMAN_ONLY,
                  "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}
    combos = [(s, mem, lvl, False) for s in strategies for mem in (1, 8, 9) for lvl in (1, 6, 9)]
    combos += [("default", 8, lvl, True) for lvl in (1, 9)]
    cases = []
    for tname, text in texts.items():
        for ci, (s, mem, lvl, flush) in enumerate(combos):
            for j in range(1 if size > 60000 else 3):
                off = ((ci * 3 + j) * 977) % (len(text) - size)
                chunk = text[off:off + size]
                while True:
                    c = zlib.compressobj(lvl, zlib.DEFLATED, -15, mem, strategies[s])
                    if flush:
                        a, b = (len(chunk) // 3) | 1, (2 * len(chunk) // 3) | 1
                        raw = (c.compress(chunk[:a]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(chunk[a:b]) + c.flush(zlib.Z_FULL_FLUSH)
                               + c.compress(chunk[b:]) + c.flush())
                    else:
                        raw = c.compress(chunk) + c.flush()
                    if len(raw) + 26 <= 65536:
                        break
                    chunk = chunk[:-1024]
                cases.append(Case("%s, %s, memLevel %d, level %d%s, %d bytes #%d" % (tname, s, mem, lvl, ", flushes" if flush else "", size, j), raw, chunk))
    return cases


# ---- a text as irregular members -------------------------------------------------------------------------------------

def irregular_members(text, seed):
    """The text cut into members of 1..5000 bytes: most from zlib, every fifth crafted with a fixed, a stored and a dynamic
    block whose matches reach back across the block borders; runs of 1, 2 and 70 empty members in the middle."""
    rng, members, i = random.Random(seed), [], 0
    while i < len(text):
        chunk = text[i:i + rng.randrange(1, 5001)]
        i += len(chunk)
        if len(members) % 5 == 2:
            a, b = sorted(rng.randrange(len(chunk) + 1) for _ in range(2))
            b = min(b, a + 40)
            m = Member().fixed(lz_symbols(chunk[:a]) + [EOB]).stored(chunk[a:b])
            m.dynamic(DYN[1][0], DYN[1][1], lz_symbols(chunk, b) + [EOB], True)
            assert bytes(m.text) == chunk
            members.append(member_of(m.case("")))
        else:
            c = zlib.compressobj(rng.choice((1, 6, 9)), zlib.DEFLATED, -15)
            members.append(bgzf_member(c.compress(chunk) + c.flush(), chunk))
    empty = bgzf_member(b"\x03\x00", b"")
    for at, run in ((3 * len(members) // 4, 70), (len(members) // 2, 2), (len(members) // 4, 1)):
        members[at:at] = [empty] * run
    return members


# ---- refusals ---------------------------------------------------------------------------------------------------------

TRUNCATED, BLOCK, STORED, LENGTHS, SYMBOL, OUTPUT, SIZE, CRC = (
    "deflate data truncated", "reserved block type", "stored block length check", "bad code lengths", "invalid symbol",
    "output overrun or distance too far", "size differs from ISIZE", "CRC-32 mismatch")


def malformed():
    """One minimal member per way of refusing a stream.  Every one is refused by a check that comes before the store or
    load it would otherwise make: the bit reader's count of the member's bits, dist > pos, pos + len > olen, pos >= olen."""
    x64 = b"x" * 64                                          # ISIZE of the deflate-level cases: room for what they decode
    bad = []

    def add(name, raw, reason, text=x64, crc=None, isize=None):
        bad.append(Bad(name, bytes(raw), text, reason, crc, isize))

    def raw_of(build):
        w = BitWriter()
        build(w)
        return w.getvalue()

    add("the data ends in the block header", raw_of(lambda w: (w.bits(1, 1), w.bits(2, 2), w.bits(29, 5))), TRUNCATED)
    add("the data ends in the code lengths", raw_of(lambda w: dynamic(w, FAM_LIT, FAM_DIST, FAM_SYMS, True))[:20], TRUNCATED)
    add("the data ends inside a match", raw_of(lambda w: fixed(w, list(range(65, 75)) + [(10, 9), EOB], True))[:11], TRUNCATED)
    add("the data ends inside a stored block", raw_of(lambda w: stored(w, b"hello world", True))[:-4], TRUNCATED)
    add("block type 3", raw_of(lambda w: (w.bits(1, 1), w.bits(3, 2))), BLOCK)
    add("LEN and NLEN disagree", raw_of(lambda w: stored(w, b"hello", True, nlen=0x1234)), STORED)
    add("an over-subscribed literal code", raw_of(lambda w: dynamic(w, _lengths(257, [(65, 1), (66, 1), (256, 1)]), [0], [], True)), LENGTHS)
    add("an incomplete literal code of two symbols", raw_of(lambda w: dynamic(w, _lengths(257, [(65, 2), (256, 2)]), [0], [65, EOB], True)), LENGTHS)
    add("an incomplete code-length code", raw_of(lambda w: dynamic(w, [8] * 257, [0], [], True, {"cl_lengths": _lengths(19, [(0, 2), (8, 2), (18, 2)])})), LENGTHS)
    fam_ops = _Z65 + _F8 + _Z183 + _T + _D
    add("a code 16 with no length before it", raw_of(lambda w: dynamic(w, FAM_LIT, FAM_DIST, [], True, {"ops": [(16, 3)] + fam_ops[3:]})), LENGTHS)
    add("a repeat that runs past HLIT + HDIST", raw_of(lambda w: dynamic(w, FAM_LIT, FAM_DIST, [], True, {"ops": _Z65 + _F8 + _Z183 + _T + [(18, 138)]})), LENGTHS)
    add("no end-of-block code", raw_of(lambda w: dynamic(w, _lengths(257, [(65, 1), (66, 1)]), [0], [65, 66], True)), LENGTHS)
    add("HCLEN 4: every length is zero", raw_of(lambda w: dynamic(w, [0] * 257, [0], [], True, {"ops": [(18, 138), (18, 120)], "cl_lengths": _lengths(19, [(0, 1), (18, 1)]), "hclen": 4})), LENGTHS)
    add("length symbol 286 in a fixed block", raw_of(lambda w: fixed(w, [65, 286], True)), SYMBOL)
    add("distance symbol 30 in a fixed block", raw_of(lambda w: fixed(w, [65, ("raw", 257, 0, 30, 0)], True)), SYMBOL)
    add("a distance beyond the output so far", raw_of(lambda w: fixed(w, [65, 66, (3, 3), EOB], True)), OUTPUT)
    # a well-formed stream behind a trailer that is wrong: zlib inflates it, gzip refuses the member
    ten = b"0123456789"
    add("output beyond ISIZE by a literal", raw_of(lambda w: fixed(w, list(ten) + [EOB], True)), OUTPUT, ten, isize=9)
    add("output beyond ISIZE by a match", raw_of(lambda w: fixed(w, [48, (9, 1), EOB], True)), OUTPUT, b"0" * 10, isize=9)
    add("output beyond ISIZE by a stored block", raw_of(lambda w: stored(w, ten, True)), OUTPUT, ten, isize=9)
    add("a stream that ends short of ISIZE", raw_of(lambda w: fixed(w, list(ten) + [EOB], True)), SIZE, ten, isize=11)
    add("a wrong CRC", raw_of(lambda w: fixed(w, list(ten) + [EOB], True)), CRC, ten, crc=(zlib.crc32(ten) ^ 1) & 0xFFFFFFFF)
    return bad


def bad_member(b):
    return bgzf_member(b.raw, b.text, crc=b.crc, isize=b.isize)
