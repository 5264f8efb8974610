"""The inputs of tests/test_seq_widths.py and tests/test_seq_widths_cpu.py: wrapped FASTA texts for sequence queries whose
scenarios are planted, not met by luck.

  cut_text(k)          a short text with every header and record shape the host-side carry of sequence identity tells
                       apart (csrc/tsx_seq.h, seq_names_piece / seq_piece), for a sweep over every piece size
  sibling_contigs(k)   contigs built from width_design.sibling_pair: windows that differ from the table's in ONE base, at
                       every offset of the window, so that a lookup that drops a limb of the key answers otherwise
  alternating(k)       one contig whose windows are present and missing in turn: SEQ_TILE_FRAGS fragments per tile
  fragments_per_tile   the fragments the missing runs fall into when cut at wave rows, stated in plain Python

Nothing here imports the library at module level; the definitions of the CPU reference (tsxcount_amd.missing_intervals,
numpy and the standard library alone) are imported where a function states its result in their terms."""
import random
from collections import Counter

import kmerdb as K
import width_design as W

TILE = 4096          # bytes of the unwrapped text one workgroup takes (csrc/tsx_kernels.h)
ROW = 64             # start positions of one wave row: a run of missing windows is cut there
TILE_FRAGS = TILE // 2


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def fasta(name, seq, width=60):
    return b">" + name + b"\n" + wrap(seq, width)


def other_base(b):
    return b"CGTA"[b"ACGT".index(b)]


def substituted(seq, at):
    return seq[:at] + bytes([other_base(seq[at])]) + seq[at + 1:]


def bases(n, salt):
    """n bases out of a fixed recurrence (no generator state shared with anything): the same text on every run."""
    x = 0x2545F491 ^ (salt * 0x9E3779B1 & 0x7FFFFFFF)
    out = bytearray()
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(b"ACGT"[(x >> 16) & 3])
    return bytes(out)


# ---- the text of the cut sweep -------------------------------------------------------------------------------------------

TAB_NAME = b"t" * 39                       # the header line ">" + 39 bytes + "\t" + ...: the tab is byte 40 of the line
LONG_NAME = b"n" * 299                     # a header line of 300 bytes with no blank: the name is its first 255 bytes


def cut_records(k):
    """[(header line or None, sequence, wrap width, blank lines behind the header, the sequence as the table holds it or
    None, its copies in the table)], in text order.  The record list is fixed by hand."""
    sib, sib2, _ = W.sibling_pair(random.Random(4100 + k), k, 3)
    long_ = bases(2 * k + 40, 8)
    cr = bases(k + 6, 10)
    cr = cr[:6] + b">" + cr[7:k // 2] + b"\r" + cr[k // 2 + 1:]          # '\r' and an inner '>' are sequence bytes
    return [
        (None, bases(k + 2, 0), 60, 0, None, 0),                          # lines in front of the first header; missing
        (b">", bases(6, 1), 60, 0, None, 0),                              # an empty name
        (b">blank x", bases(k + 1, 2), 60, 3, bases(k + 1, 2), 1),        # blank lines between header and sequence
        (b">vanishes", b"", 60, 0, None, 0),                              # two headers in a row: the first vanishes
        (b">after", bases(5, 3), 60, 0, None, 0),
        (b">" + TAB_NAME + b"\t" + b"d" * 259, bases(k + 2, 4), 60, 0, substituted(bases(k + 2, 4), 0), 1),
        (b">" + LONG_NAME, bases(k - 1, 5), 60, 0, None, 0),              # 300 bytes, no blank; a record shorter than k
        (b">short", b"ACG", 60, 0, None, 0),
        (b">exact", bases(k, 7), 60, 0, bases(k, 7), 3),                  # exactly k bases: one window, count 3
        (b">long", long_, 7, 0, substituted(long_, 2), 2),                # many short lines; missing at 0 .. 2, count 2
        (b">sib", sib, 60, 0, sib2, 1),                                   # R against R': k windows missing in the middle
        (b">cr\r", cr, k // 2 + 1, 1, cr, 1),
        (b">last y", bases(k + 5, 11), 60, 0, bases(k + 5, 11), 5),       # no trailing newline; count 5
    ]


def cut_text(k):
    """(query text, table text) of the cut sweep."""
    assert TAB_NAME.find(b" ") < 0 and len(b">" + TAB_NAME + b"\t" + b"d" * 259) == 300 and len(b">" + LONG_NAME) == 300
    text, table = b"", b""
    for head, seq, width, blanks, held, copies in cut_records(k):
        if head is not None:
            text += head + b"\n" + b"\n" * blanks
        text += wrap(seq, width)
        if seq and head == b">blank x":
            text += b"\n\n"
        if held:
            table += fasta(b"t", held, 70) * copies
    assert text.endswith(b"\n")
    return text[:-1], table


def cut_names(k):
    """The names fasta_records has to give for cut_text(k), stated from the record list."""
    out = []
    for head, seq, *_ in cut_records(k):
        if not seq:
            continue
        h = b"" if head is None else head[1:]
        for blank in (b" ", b"\t"):
            if blank in h:
                h = h[:h.index(blank)]
        out.append(h[:255])
    return out


def byte_map(text):
    """Per byte offset of a wrapped text: (kind, line start, record, bases of the record in front of the byte).  kind:
    'h' a byte of a header line, 's' of a sequence line, 'n' a newline; record: the index in fasta_records of the record
    the byte belongs to (for a header: the one it would name), -1 in front of any; by the rules of join_fasta."""
    out, rec, nb, has_seq, line_start, kind = [], -1, 0, False, 0, None
    started = -1
    for i, b in enumerate(text):
        if b == 0x0A:
            out.append(("n", line_start, started, nb))
            line_start, kind = i + 1, None
            continue
        if kind is None:
            kind = "h" if b == 0x3E else "s"
            if kind == "h":
                has_seq, nb = False, 0
            elif not has_seq:
                has_seq, rec, nb = True, rec + 1, 0
                started = rec
        if kind == "h":
            out.append(("h", line_start, rec + 1, 0))
        else:
            out.append(("s", line_start, rec, nb))
            nb += 1
    return out


def line_end(text, at):
    e = text.find(b"\n", at)
    return len(text) if e < 0 else e


def cut_classes(k, text, intervals):
    """{name: predicate(offset)}: the places a cut between text[:o] and text[o:] can fall that seq_names_piece and
    seq_piece tell apart.  intervals: missing_intervals of the whole text (for the classes that speak of missing runs)."""
    bm = byte_map(text)
    first_header = text.index(b"\n>") + 1

    def header_line(o):            # o lies inside a header line (behind its '>'), the line's start and end
        return 0 < o < len(text) and bm[o - 1][0] == "h" and bm[o - 1][1] < o

    def prev_line_is_header(o):    # the last non-empty line in front of o is a header line, and o is a line start
        if not (0 < o <= len(text)) or text[o - 1:o] != b"\n":
            return False
        j = o - 1
        while j >= 0 and text[j:j + 1] == b"\n":
            j -= 1
        return j >= 0 and bm[j][0] == "h"

    def seq_cut(o):                # (record, bases in front) when both sides of the cut hold bases of one record
        if not (0 < o < len(text)) or bm[o - 1][0] == "h":
            return None
        j = o
        while j < len(text) and bm[j][0] == "n":
            j += 1
        if j == len(text) or bm[j][0] != "s" or bm[j][3] == 0:
            return None
        return bm[j][2], bm[j][3]

    def in_run_from_the_carry(o):  # a run of missing windows that begins in the k - 1 carried bases and goes on behind
        c = seq_cut(o)
        return c is not None and any(r == c[0] and c[1] - (k - 1) <= s < c[1] <= e - k for r, s, e in intervals)

    def run_ends_at_the_seam(o):   # the last missing window of a run is the last one the earlier pieces hold whole
        c = seq_cut(o)
        return c is not None and any(r == c[0] and e == c[1] for r, s, e in intervals)

    return {
        "right after the '>' of a header": lambda o: header_line(o) and o - 1 == bm[o - 1][1],
        "between a header's newline and the blank lines behind it": lambda o: prev_line_is_header(o) and text[o - 2:o - 1] != b"\n"
        and text[o:o + 1] == b"\n",
        "among the blank lines behind a header": lambda o: prev_line_is_header(o) and text[o - 2:o - 1] == b"\n" and text[o:o + 1] == b"\n",
        "behind a header's blank lines, in front of its sequence": lambda o: prev_line_is_header(o) and text[o - 2:o - 1] == b"\n"
        and o < len(text) and bm[o][0] == "s",
        "inside a header longer than 256 bytes, within its first 255": lambda o: header_line(o) and line_end(text, o) - bm[o - 1][1] > 256
        and 1 < o - bm[o - 1][1] < 255,
        "inside a header longer than 256 bytes, behind byte 256": lambda o: header_line(o) and o - bm[o - 1][1] > 257,
        "a header's 256 kept bytes end at the cut": lambda o: header_line(o) and o - bm[o - 1][1] == 257 and text[o:o + 1] != b"\n",
        "at the tab that ends a name": lambda o: header_line(o) and text[o:o + 1] == b"\t",
        "in front of the newline of a header": lambda o: header_line(o) and text[o:o + 1] == b"\n",
        "between two headers in a row": lambda o: prev_line_is_header(o) and text[o:o + 1] == b">",
        "before the first header, inside a line": lambda o: 0 < o < first_header and text[o - 1:o] != b"\n",
        "before the first header, at a line start": lambda o: 0 < o <= first_header and text[o - 1:o] == b"\n",
        "inside a sequence line": lambda o: seq_cut(o) is not None and text[o - 1:o] != b"\n" and text[o:o + 1] != b"\n",
        "between two lines of a sequence": lambda o: seq_cut(o) is not None and text[o - 1:o] == b"\n",
        "between a sequence line and its newline": lambda o: seq_cut(o) is not None and text[o:o + 1] == b"\n",
        "between '\\r' and its newline": lambda o: text[o - 1:o] == b"\r" and text[o:o + 1] == b"\n",
        "in front of an inner '>'": lambda o: 0 < o < len(text) and text[o:o + 1] == b">" and bm[o][0] == "s",
        "between a sequence and the next header": lambda o: 0 < o < len(text) and text[o - 1:o] == b"\n" and text[o:o + 1] == b">"
        and not prev_line_is_header(o),
        "inside a run of missing windows that begins in the carried bases": in_run_from_the_carry,
        "a run of missing windows ends with the last whole window in front of the cut": run_ends_at_the_seam,
        "fewer than k - 1 bases of the record in front of the cut": lambda o: seq_cut(o) is not None and seq_cut(o)[1] < k - 1,
    }


# ---- sibling contigs ------------------------------------------------------------------------------------------------------

def limb_positions(k):
    """One window offset per 64-bit limb of a k-base key (the middle of each limb's bases; the top limb's may be partial)."""
    wk = (2 * k + 63) // 64
    return [(32 * i + min(32 * (i + 1), k)) // 2 for i in range(wk)]


class Contig:
    """One query contig: its name and sequence, the pair it comes from and what the design says of it."""

    def __init__(self, name, seq, kind, p):
        self.name, self.seq, self.kind, self.p = name, seq, kind, p      # p: the substituted position IN seq


class Siblings:
    """Contigs and a table text for one k.

      cross pairs    R is a query contig, R' is in the table once: the k windows of R that cover the substituted position
                     are missing and nothing else is -- one interval (p - k + 1, p + k), present == kmers - k
      within pairs   R twice and R' five times in the table, both are query contigs: the k covering windows of R have
                     count 2 and those of R' count 5, every other window 7
      filler         a contig the table holds whole, in front, of the length that puts a 4096-byte tile border of the
                     unwrapped text among the start positions of the first cross pair's covering windows

    One cross and one within pair per limb of the key (and one more where the top limb is partial), the substituted
    position moved along by sibling_pair's j.  Whatever p is, the k covering windows hold it at every offset 0 .. k - 1,
    so every pair reaches every limb; limb_positions names one window per limb for the assertions that say so.

    query(canonical) gives the text; with canonical every second contig is written as its reverse complement and, for
    even k, the palindrome record of width_design is added (three times in the table)."""

    def __init__(self, k):
        rnd = random.Random(7300 + k)
        self.k = k
        n = (2 * k + 63) // 64 + (1 if (2 * k) % 64 else 0)
        self.cross = [W.sibling_pair(rnd, k, j) for j in range(n)]
        self.within = [W.sibling_pair(rnd, k, 3 * j + 1) for j in range(n)]
        p0 = self.cross[0][2]
        self.filler = W.rand_seq(rnd, TILE - 2 - 3 - (p0 - k // 2))      # ">\n" filler "\n" ">\n": the border at p0 - k / 2
        self.pal = W.palindrome_record(k)[0] if k % 2 == 0 else None
        table = fasta(b"filler", self.filler, 70)
        for r, r2, _ in self.cross:
            table += fasta(b"x", r2, 70)
        for r, r2, _ in self.within:
            table += fasta(b"r", r, 70) * 2 + fasta(b"r2", r2, 70) * 5
        self.table = table
        self.table_canonical = table + (fasta(b"pal", self.pal + b"AC", 70) * 3 if self.pal else b"")

    def contigs(self, canonical=False):
        out = [Contig(b"filler", self.filler, "filler", None)]
        for i, (r, _, p) in enumerate(self.cross):
            out.append(Contig(b"cross%d" % i, r, "cross", p))
        for i, (r, r2, p) in enumerate(self.within):
            out.append(Contig(b"within%d_2" % i, r, "within2", p))
            out.append(Contig(b"within%d_5" % i, r2, "within5", p))
        if canonical:
            for c in out[2::2]:                                              # (cross 0 stays: the border is placed in it)
                c.seq, c.p = K.revcomp(c.seq), len(c.seq) - 1 - c.p
                c.name += b"_rc"
            if self.pal:
                out.append(Contig(b"pal", self.pal + b"AC", "pal", None))
        return out

    def query(self, canonical=False):
        return b"".join(fasta(c.name + b" " + c.kind.encode(), c.seq, 60) for c in self.contigs(canonical))

    def border_offset(self, canonical=False):
        """The offset in cross pair 0's contig of the first tile border of the unwrapped text, computed as
        test_seq.make_case does: out_pos runs over ">\\n" + sequence + "\\n" per record."""
        out_pos = 0
        for c in self.contigs(canonical):
            out_pos += 2
            if c.kind == "cross":
                return (out_pos // TILE + 1) * TILE - out_pos
            out_pos += len(c.seq) + 1


_SIB = {}


def sibling_contigs(k):
    if k not in _SIB:
        _SIB[k] = Siblings(k)
    return _SIB[k]


def with_n_runs(sib, run=2):
    """The query of the base-rule cases, as [(name, sequence, kind)].  Every contig of sib gets a run of N inside its
    pair's covering stretch, `run` bases long and 5 bases in front of the substituted position p.  With acgt_only the
    windows over the run are dropped, which leaves the missing windows n + run .. p of the k covering ones: the interval
    is cut short (a run of N spans at least k window starts, so it cannot split k missing windows in two).  The N lies
    at least k - 6 bases into the contig, so the windows it drops hold it at every offset up to k - 1: in the first and,
    for k > 64, in the second 64-bit word of the break mask.

    'double' contigs split: R against a table copy with TWO substitutions, at p and p + k, has 2k missing windows in a
    row, and the run of N at p + 1 leaves window p - k + 1 on one side and p + 1 + run .. p + k on the other.

    'lower' and 'iupac' contigs: a cross contig with its covering stretch in lower case, and one with an IUPAC code at p + 3."""
    k = sib.k
    out = []
    for c in sib.contigs():
        if c.p is None:
            out.append((c.name, c.seq, c.kind))
            continue
        n = c.p - 5
        assert n >= k - 6 and n + run <= c.p
        out.append((c.name + b"_n", c.seq[:n] + b"N" * run + c.seq[n + run:], c.kind))
    rnd = random.Random(7400 + k)
    doubles = []
    for j in range(2):
        r = W.rand_seq(rnd, 3 * k + 40)
        p = k - 1 + 9 * j
        held = substituted(substituted(r, p), p + k)
        out.append((b"double%d" % j, r[:p + 1] + b"N" * run + r[p + 1 + run:], "double"))
        doubles.append((held, p))
    r, _, p = sib.cross[0]
    out.append((b"lower", r[:p - k + 1] + r[p - k + 1:p + k].lower() + r[p + k:], "lower"))
    iupac = b"Y" if r[p + 3:p + 4] == b"C" else b"R"                        # R is looked up as C, Y as G: never the base itself
    out.append((b"iupac", r[:p + 3] + iupac + r[p + 4:], "iupac"))
    table = sib.table + b"".join(fasta(b"d", held, 70) for held, _ in doubles)
    text = b"".join(fasta(name, seq, 60) for name, seq, _ in out)
    return text, table, out, doubles


# ---- alternating present and missing windows -----------------------------------------------------------------------------

def alternating(k, n_tiles=3, seed=5):
    """(contig, k-mers at even start positions, their counts): the contig's record ">\\n" + contig + "\\n" has a valid
    window at every byte of tiles 1 .. n_tiles of the unwrapped text (tile 0 begins with the two bytes ">\\n").  No k-mer
    at an odd start equals one at an even start: a table of the even ones leaves every odd window missing."""
    n = (n_tiles + 1) * TILE + k
    for attempt in range(20):
        contig = W.rand_seq(random.Random(seed + 1000 * attempt), n)
        even = Counter(contig[i:i + k] for i in range(0, n - k + 1, 2))
        if not any(contig[i:i + k] in even for i in range(1, n - k + 1, 2)):
            kmers = sorted(even)
            return contig, kmers, [even[x] for x in kmers]
    raise AssertionError("no contig without a collision between odd and even windows")


def alternating_limbs(kmers, k):
    return K.kmers_to_limbs(kmers, k)


# ---- the fragment model --------------------------------------------------------------------------------------------------

def fragments_per_tile(records, D, k, lower=1, upper=None, canonical=False, acgt_only=False):
    """[fragments of tile 0, of tile 1, ...] of the unwrapped text b"".join(b">\\n" + s + b"\\n" for _, s in records): the
    pieces the runs of missing windows (tsxcount_amd.missing_intervals) fall into when every run is cut where its start
    positions pass from one 64-position row of the text to the next.  A tile is 64 rows; a row of 64 start positions
    holds at most 32 runs, which is what SEQ_TILE_FRAGS = TILE / 2 says."""
    from tsxcount_amd import missing_intervals
    off, at = [], 0
    for _, s in records:
        off.append(at + 2)
        at += len(s) + 3
    tiles = [0] * ((at + TILE - 1) // TILE)
    for r, s, e in missing_intervals(records, D, k, lower, upper, canonical, acgt_only):
        first, last = off[r] + s, off[r] + e - k                          # text positions of the run's first and last start
        for row in range(first // ROW, last // ROW + 1):
            tiles[row * ROW // TILE] += 1
    return tiles
