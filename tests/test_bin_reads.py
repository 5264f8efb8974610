"""Read binning by two tables (tsx_hip_bin_stats_*, tsx_hip_bin_reads_host) through the C ABI, Python and the tsxCount
CLI, on the GPU.

Expectations come from Python dictionaries over the counted texts and from the short restatement below of the record
rules (empty lines dropped, lpr non-empty lines a record, the second one the sequence), of the base rule (a window with
a byte outside ACGTacgt, or with a quality byte below the minimum, is no k-mer), of a hit (the count lies in the table's
range, a lower bound of 0 taken as 1) and of the class rule.  Never from the library under test."""
import ctypes
import gzip
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
U64 = (1 << 64) - 1
_CODE = bytes(b"ACGT"[((b >> 1) ^ (b >> 2)) & 3] for b in range(256))   # base_code as a byte table
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = frozenset(b"ACGTacgt")
A, B, AMB, NONE = 0, 1, 2, 3
NAMES = ("a", "b", "ambiguous", "none")


# ---- the restatement ----------------------------------------------------------------------------------------------

def records(text, lpr):
    """[(sequence line, quality line, record bytes as a kept record is written)]."""
    spans, pos = [], 0
    for part in text.split(b"\n"):
        if part:
            spans.append((pos, pos + len(part)))
        pos += len(part) + 1
    out = []
    for i in range(0, len(spans), lpr):
        g = spans[i:i + lpr]
        seq = text[g[1][0]:g[1][1]] if len(g) > 1 else b""
        qual = text[g[3][0]:g[3][1]] if lpr == 4 and len(g) > 3 else b""
        out.append((seq, qual, text[g[0][0]:g[-1][1]] + b"\n"))
    return out


def kmers_of(seq, qual, k, canonical, acgt_only, minq):
    """The coded k-mers of a sequence line: the windows that are k-mers under the base rule, strand pairs folded."""
    s = seq.translate(_CODE)
    q = ord(minq) if minq else 0
    bad = [(acgt_only and seq[i] not in ACGT) or (q and (i >= len(qual) or qual[i] < q)) for i in range(len(seq))]
    pre = [0]
    for b in bad:
        pre.append(pre[-1] + (1 if b else 0))
    out = []
    for i in range(len(seq) - k + 1):
        if pre[i + k] - pre[i]:
            continue
        x = s[i:i + k]
        out.append(min(x, x[::-1].translate(_COMP)) if canonical else x)
    return out


def counts_of(text, k, lpr, canonical=False, acgt_only=False, minq=None):
    c = Counter()
    for seq, qual, _ in records(text, lpr):
        c.update(kmers_of(seq, qual, k, canonical, acgt_only, minq))
    return c


def classify(ha, hb, min_hits=1, ratio_milli=1000):
    qa, qb = ha >= min_hits, hb >= min_hits
    if qa and ha > hb and ha * 1000 >= ratio_milli * hb:
        return A
    if qb and hb > ha and hb * 1000 >= ratio_milli * ha:
        return B
    return AMB if (qa or qb) else NONE


def expected(query, ca, cb, k, lpr, a_range=(1, None), b_range=(1, None), min_hits=1, ratio_milli=1000, canonical=False,
             acgt_only=False, minq=None):
    """([(kmers, hits_a, hits_b, hits_both)], [class]) per record."""
    al, au = max(1, a_range[0]), U64 if a_range[1] is None else a_range[1]
    bl, bu = max(1, b_range[0]), U64 if b_range[1] is None else b_range[1]
    stats, cls = [], []
    for seq, qual, _ in records(query, lpr):
        km = kmers_of(seq, qual, k, canonical, acgt_only, minq)
        ina = [al <= ca.get(x, 0) <= au for x in km]
        inb = [bl <= cb.get(x, 0) <= bu for x in km]
        st = (len(km), sum(ina), sum(inb), sum(p and q for p, q in zip(ina, inb)))
        stats.append(st)
        cls.append(classify(st[1], st[2], min_hits, ratio_milli))
    return stats, cls


def expected_files(query, cls, lpr):
    """The bytes of the four outputs: every record in its class's file, in input order."""
    out = [b"", b"", b"", b""]
    for (_, _, rec), c in zip(records(query, lpr), cls):
        out[c] += rec
    return out


def as_tuples(st):
    return [tuple(int(v) for v in r) for r in st]


# ---- the texts ----------------------------------------------------------------------------------------------------

def rand_seq(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def fmt(seqs, lpr, tag=b"r", quals=None):
    if lpr == 2:
        return b"".join(b">%s%d\n%s\n" % (tag, i, s) for i, s in enumerate(seqs))
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, quals[i] if quals else b"I" * len(s)) for i, s in enumerate(seqs))


def tiled(genome, length=400, step=150):
    return [genome[i:i + length] for i in range(0, max(1, len(genome) - length + step), step)]


class Texts:
    """Two planted table texts and a query text.  A's text covers the regions GA and GS, B's covers GB and GS; every
    region is read twice in A and three times in B's own part, so that count ranges can tell them apart."""

    def __init__(self, seed, lpr, with_n=False, with_lowq=False):
        rnd = random.Random(seed)
        self.lpr = lpr
        ga, gb, gs = rand_seq(rnd, 3000), rand_seq(rnd, 3000), rand_seq(rnd, 2000)
        a_reads = tiled(ga) * 2 + tiled(gs)
        b_reads = tiled(gb) * 3 + tiled(gs) * 2
        if with_n:   # a few bytes outside ACGT in the counted texts too
            a_reads = [s[:50] + b"N" + s[51:] if i % 5 == 0 else s for i, s in enumerate(a_reads)]
        self.text_a, self.text_b = fmt(a_reads, lpr, b"a"), fmt(b_reads, lpr, b"b")

        def draw(g):
            n = rnd.randint(20, 300)
            at = rnd.randint(0, len(g) - n)
            return g[at:at + n]

        reads = []
        for _ in range(60):
            reads.append(draw(ga))
            reads.append(draw(gb))
            reads.append(draw(gs))
            half_a, half_b = draw(ga), draw(gb)
            reads.append(half_a[:150] + half_b[:150])          # from both
            reads.append(rand_seq(rnd, rnd.randint(20, 300)))   # from neither
        reads.append(b"ACGTACGTACG")                            # shorter than every k here
        # one record of about 10 kB: it spans three 4096-byte tiles and many waves; pieces of both genomes and noise
        big = b"".join(x for i in range(0, 3000, 600) for x in (ga[i:i + 600], rand_seq(rnd, 200), gb[i:i + 700], gs[i:i + 500]))
        reads.insert(len(reads) // 2, big)
        rnd.shuffle(reads)
        reads.insert(100, big[37:37 + 10240])
        quals = None
        if with_n:
            reads = [self._edit(rnd, s, b"N", 3) if i % 3 == 0 else s for i, s in enumerate(reads)]
        if with_lowq and lpr == 4:
            quals = [self._edit(rnd, b"I" * len(s), b"#", 2) if i % 3 == 1 else b"I" * len(s) for i, s in enumerate(reads)]
            quals[7] = quals[7][:len(quals[7]) // 2]           # a quality line shorter than its sequence
        body = fmt(reads, lpr, b"q", quals)
        # an empty sequence line: empty lines are no lines, so the header's record takes the NEXT non-empty lines (its
        # sequence is "+" or "more"); one more line puts the records behind it back in step.  Then a trailing record
        # without its last '\n'.
        last = draw(gb)
        if lpr == 4:
            tail = b"@emptyseq\n\n+\nIIII\nmore\n@t1\n" + draw(ga) + b"\n+\n" + b"I" * 300 + b"\n@last\n" + last + b"\n+\n" + b"I" * len(last)
        else:
            tail = b">emptyseq\n\nmore\n>t1\n" + draw(ga) + b"\n>last\n" + last
        self.query = b"\n" + body + tail
        assert not self.query.endswith(b"\n")
        self.max_record = max(len(r) for _, _, r in records(self.query, lpr))

    @staticmethod
    def _edit(rnd, s, byte, n):
        s = bytearray(s)
        for _ in range(n):
            s[rnd.randrange(len(s))] = byte[0]
        return bytes(s)


_TEXTS = {}


def texts(seed, lpr, with_n=False, with_lowq=False):
    key = (seed, lpr, with_n, with_lowq)
    if key not in _TEXTS:
        _TEXTS[key] = Texts(seed, lpr, with_n, with_lowq)
    return _TEXTS[key]


_EXPECT = {}


def expect(tx, k, canonical=False, acgt_only=False, minq=None, **rule):
    key = (id(tx), k, canonical, acgt_only, minq, tuple(sorted(rule.items())))
    if key not in _EXPECT:
        ca = counts_of(tx.text_a, k, tx.lpr, canonical, acgt_only, minq)
        cb = counts_of(tx.text_b, k, tx.lpr, canonical, acgt_only, minq)
        _EXPECT[key] = expected(tx.query, ca, cb, k, tx.lpr, canonical=canonical, acgt_only=acgt_only, minq=minq, **rule)
    return _EXPECT[key]


# ---- GPU ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def table(T, text, k, lpr, l=15, s=0, seed=1, canonical=False, acgt_only=False, minq=None, overflow_l=0):
    m = T.TSXHashMapHIP(l, s, k, hash_seed=seed, overflow_l=overflow_l, canonical=canonical, acgt_only=acgt_only, min_qual_char=minq)
    m.set_record_lines(lpr)
    m.countFastq(text)
    return m


CONFIGS = {
    "fastq": dict(lpr=4), "fasta": dict(lpr=2), "canonical": dict(lpr=4, canonical=True),
    "acgt_only": dict(lpr=4, acgt_only=True, with_n=True), "min_qual": dict(lpr=4, minq="5", with_lowq=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("k", [14, 33, 63, 127])
def test_stats_and_classes(T, k, config):
    """Key widths 1, 2, 2 and 4 limbs.  B once built like A (one seed: one LUT, one hash) and once with another l,
    other storage bits and another seed (two LUTs): the same answers."""
    c = dict(CONFIGS[config])
    lpr, with_n, with_lowq = c.pop("lpr"), c.pop("with_n", False), c.pop("with_lowq", False)
    tx = texts(100 + k, lpr, with_n, with_lowq)
    rules = [dict(), dict(a_range=(2, None), b_range=(3, 3), min_hits=5, ratio_milli=1500)]
    a = table(T, tx.text_a, k, lpr, **c)
    b_like = table(T, tx.text_b, k, lpr, **c)
    b_other = table(T, tx.text_b, k, lpr, l=17, s=5, seed=977, overflow_l=12, **c)
    try:
        for rule in rules:
            want_st, want_cls = expect(tx, k, **c, **rule)
            assert len(set(want_cls)) == 4 or rule, "the default rule meets every class"
            kw = dict(a_range=rule.get("a_range", (1, None)), b_range=rule.get("b_range", (1, None)),
                      min_hits=rule.get("min_hits", 1), ratio=rule.get("ratio_milli", 1000) / 1000)
            for name, b in (("like A", b_like), ("other layout", b_other)):
                st, cls = a.binStats(b, tx.query, **kw)
                assert st.dtype == T.BIN_STATS_DTYPE and cls.dtype == np.uint8
                assert as_tuples(st) == want_st, (k, config, name, rule)
                assert cls.tolist() == want_cls, (k, config, name, rule)
    finally:
        for m in (a, b_like, b_other):
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [14, 63])
def test_a_is_b(T, k):
    tx = texts(100 + k, 4)
    a = table(T, tx.text_a, k, 4)
    ca = counts_of(tx.text_a, k, 4)
    want_st, want_cls = expected(tx.query, ca, ca, k, 4)
    st, cls = a.binStats(a, tx.query)
    assert as_tuples(st) == want_st
    assert (st["hits_a"] == st["hits_b"]).all() and (st["hits_a"] == st["hits_both"]).all() and st["hits_a"].any()
    assert cls.tolist() == want_cls and not ((cls == A) | (cls == B)).any()
    # two ranges on one table do split it: counts of exactly 1 against counts of 2 and more
    want_st, want_cls = expected(tx.query, ca, ca, k, 4, a_range=(1, 1), b_range=(2, None))
    st, cls = a.binStats(a, tx.query, a_range=(1, 1), b_range=(2, None))
    assert as_tuples(st) == want_st and cls.tolist() == want_cls and not st["hits_both"].any()
    a.close()


@pytest.mark.gpu
def test_carried_counts_and_ranges_above_the_slot_field(T):
    """Two storage bits hold counts up to 3 in the slot: everything above lives in the secondary array."""
    rnd = random.Random(5)
    k = 21
    seqs = [rand_seq(rnd, rnd.randint(40, 120)) for _ in range(40)]
    mult_a = [1, 3, 4, 5, 17, 40, 70, 130]
    mult_b = [90, 2, 6, 1, 4, 33, 3, 8]
    ta = fmt([s for i, s in enumerate(seqs) for _ in range(mult_a[i % 8])], 4, b"a")
    tb = fmt([s for i, s in enumerate(seqs[:32]) for _ in range(mult_b[i % 8])], 4, b"b")
    q = fmt(seqs + [seqs[0][:30] + seqs[1][:40]], 4, b"q")
    ca, cb = counts_of(ta, k, 4), counts_of(tb, k, 4)
    a = table(T, ta, k, 4, l=14, s=2, overflow_l=12)   # (most k-mers carry: room for them)
    b = table(T, tb, k, 4, l=13, s=2, seed=3, overflow_l=12)
    assert a.stats()["overflow_carries"] > 0 and b.stats()["overflow_carries"] > 0
    for ar, br in (((1, None), (1, None)), ((4, 70), (4, 33)), ((100, None), (34, None)), ((5, 5), (0, 3))):
        want_st, want_cls = expected(q, ca, cb, k, 4, a_range=ar, b_range=br)
        st, cls = a.binStats(b, q, a_range=ar, b_range=br)
        assert as_tuples(st) == want_st, (ar, br)
        assert cls.tolist() == want_cls, (ar, br)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [14, 63])
def test_seams_host_pieces(T, k, monkeypatch):
    tx = texts(100 + k, 4, False, True)
    want_st, want_cls = expect(tx, k, minq="5")
    a = table(T, tx.text_a, k, 4, minq="5")
    b = table(T, tx.text_b, k, 4, minq="5", seed=4)
    whole = a.binStats(b, tx.query)
    assert as_tuples(whole[0]) == want_st and whole[1].tolist() == want_cls
    # pieces that end inside the text, inside records, and pieces shorter than the long record (they grow)
    for chunk in (600, 4096, 4097, tx.max_record + 1, 30000):
        st, cls = a.binStats(b, tx.query, chunk_bytes=chunk)
        assert as_tuples(st) == want_st and cls.tolist() == want_cls, chunk
    a.close()
    b.close()
    # TSX_HIP_PIECE_BYTES is not read by the bin calls: maps made under it answer the same with the default pieces
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "4096")
    a = table(T, tx.text_a, k, 4, minq="5")
    b = table(T, tx.text_b, k, 4, minq="5", seed=4)
    st, cls = a.binStats(b, tx.query)
    assert as_tuples(st) == want_st and cls.tolist() == want_cls
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [14, 127])
def test_device_form_windows_and_capacity(T, k, monkeypatch):
    import torch
    tx = texts(100 + k, 4, True, False)
    want_st, _ = expect(tx, k, acgt_only=True)
    nrec = len(want_st)
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(tx.query + b"\n" * 64), dtype=torch.uint8).to(dev)
    a = table(T, tx.text_a, k, 4, acgt_only=True)
    b = table(T, tx.text_b, k, 4, acgt_only=True, seed=11, l=16)
    SENT = 0x5A5A5A5A5A5A5A5A

    def run(cap):
        d_stats = torch.full(((nrec + 1) * 4,), SENT, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        try:
            n = a.binStatsDevice(b, d_text.data_ptr(), len(tx.query), d_stats.data_ptr(), cap)
            code = T.OK
        except T.TSXException as e:
            n, code = None, e.code
        torch.cuda.synchronize()
        return n, code, d_stats.cpu().numpy().view(np.uint64).reshape(-1, 4)

    for win in (None, 4096, 4112, 20000):
        if win:
            monkeypatch.setenv("TSX_HIP_DEV_WINDOW", str(win))
        else:
            monkeypatch.delenv("TSX_HIP_DEV_WINDOW", raising=False)
        n, code, got = run(nrec)
        assert code == T.OK and n == nrec, win
        assert as_tuples(got[:nrec]) == want_st, win
        assert (got[nrec] == np.uint64(0x5A5A5A5A5A5A5A5A)).all(), "the row behind the capacity is untouched"
    # a capacity below the record count: ERANGE, the first rows right, nothing behind them written
    cap = nrec // 3
    n, code, got = run(cap)
    assert code == T.ERANGE
    assert as_tuples(got[:cap]) == want_st[:cap]
    assert (got[cap:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    a.close()
    b.close()


@pytest.mark.gpu
def test_host_capacity_sentinel(T):
    k = 33
    tx = texts(100 + k, 2)
    want_st, want_cls = expect(tx, k)
    nrec = len(want_st)
    a = table(T, tx.text_a, k, 2)
    b = table(T, tx.text_b, k, 2, seed=2)
    L = T.lib()
    rule = T.bin_rule()
    for cap, chunk in ((nrec // 2, 0), (nrec // 2, 3000), (nrec - 1, 0), (1, 5000), (0, 0)):
        st = np.full(cap + 1, 0x77, dtype=np.uint8).repeat(32).view(T.BIN_STATS_DTYPE)
        cls = np.full(cap + 1, 0x77, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        code = L.tsx_hip_bin_stats_host(a.handle, b.handle, tx.query, len(tx.query), ctypes.byref(rule),
                                        st.ctypes.data_as(ctypes.c_void_p), cls.ctypes.data_as(ctypes.c_void_p), cap,
                                        ctypes.byref(n), chunk)
        assert code == T.ERANGE and n.value == nrec, (cap, chunk)
        assert as_tuples(st[:cap]) == want_st[:cap] and cls[:cap].tolist() == want_cls[:cap]
        assert cls[cap] == 0x77 and st[cap:].view(np.uint8).tolist() == [0x77] * 32
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lpr", [4, 2])
def test_bin_reads_files_totals_and_tables_unchanged(T, lpr, tmp_path):
    k = 33
    tx = texts(100 + k, lpr)
    a = table(T, tx.text_a, k, lpr)
    b = table(T, tx.text_b, k, lpr, seed=6, l=16, s=6)
    before = [(m.getCountHistogram(64).tolist(), m.stats()["distinct"], m.stats()["kmers_added"]) for m in (a, b)]
    paths = [str(tmp_path / ("%s.out" % n)) for n in NAMES]
    for rule in (dict(), dict(min_hits=40, ratio_milli=3000)):
        _, want_cls = expect(tx, k, **rule)
        files = expected_files(tx.query, want_cls, lpr)
        kw = dict(min_hits=rule.get("min_hits", 1), ratio=rule.get("ratio_milli", 1000) / 1000)
        for chunk in (0, 5000, tx.max_record + 3):
            tot = a.binReads(b, tx.query, *paths, chunk_bytes=chunk, **kw)
            assert tot == {"records": len(want_cls), "n": [want_cls.count(c) for c in range(4)], "bytes": [len(f) for f in files]}
            for p, f in zip(paths, files):
                assert open(p, "rb").read() == f, (p, chunk)
        # two outputs dropped: their classes are still counted, with no bytes
        tot = a.binReads(b, tx.query, paths[0], None, paths[2], None, chunk_bytes=7000, **kw)
        assert tot["n"] == [want_cls.count(c) for c in range(4)]
        assert tot["bytes"] == [len(files[0]), 0, len(files[2]), 0]
        assert open(paths[0], "rb").read() == files[0] and open(paths[2], "rb").read() == files[2]
        # every record exactly once, each file in input order
        recs = [r for _, _, r in records(tx.query, lpr)]
        assert sorted(recs) == sorted(r for f in files for _, _, r in records(f, lpr))
    # a descriptor that cannot be written
    fd = os.open(paths[1], os.O_RDONLY)
    try:
        with pytest.raises(T.TSXException) as e:
            a.binReads(b, tx.query, paths[0], fd)
        assert e.value.code == T.EIO
    finally:
        os.close(fd)
    # an empty text: no records, empty files
    assert a.binReads(b, b"", *paths) == {"records": 0, "n": [0] * 4, "bytes": [0] * 4}
    after = [(m.getCountHistogram(64).tolist(), m.stats()["distinct"], m.stats()["kmers_added"]) for m in (a, b)]
    assert after == before
    a.close()
    b.close()


@pytest.mark.gpu
def test_refusals_with_real_maps(T):
    tx = texts(114, 4)
    a = table(T, tx.text_a, 14, 4)
    for other, word in ((T.TSXHashMapHIP(15, 0, 15), "differ in k"), (T.TSXHashMapHIP(15, 0, 14, canonical=True), "canonical"),
                        (T.TSXHashMapHIP(15, 0, 14, acgt_only=True), "base rule")):
        with pytest.raises(T.TSXException) as e:
            a.binStats(other, tx.query)
        assert e.value.code == T.EINVAL and word in str(e.value)
        other.close()
    a.close()


def run_cli(*args, timeout=300):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.gpu
def test_cli_end_to_end(T, tmp_path):
    k = 33
    tx = texts(100 + k, 4)
    fa, fb, fq = tmp_path / "a.fastq", tmp_path / "b.fastq", tmp_path / "q.fastq.gz"
    fa.write_bytes(tx.text_a)
    fb.write_bytes(tx.text_b)
    with gzip.open(fq, "wb") as f:
        f.write(tx.query)
    da, db = tmp_path / "a.db", tmp_path / "b.db"
    for src, db_path, l, seed in ((fa, da, 15, 1), (fb, db, 16, 8)):
        code, _, err = run_cli("--input=%s" % src, "--k=%d" % k, "--l=%d" % l, "--seed=%d" % seed, "--save=%s" % db_path)
        assert code == 0, err[-400:]
    outs = [tmp_path / ("bin_%s.fq" % n) for n in NAMES]
    stats = tmp_path / "bin_stats.tsv"
    args = ["--load=%s" % da, "--with=%s" % db, "--bin-input=%s" % fq, "--bin-a=%s" % outs[0], "--bin-b=%s" % outs[1],
            "--bin-ambiguous=%s" % outs[2], "--bin-none=%s" % outs[3], "--bin-stats=%s" % stats]

    def check(extra, rule):
        code, out, err = run_cli(*(args + extra))
        assert code == 0, err[-400:]
        want_st, want_cls = expect(tx, k, **rule)
        files = expected_files(tx.query, want_cls, 4)
        for p, f in zip(outs, files):
            assert p.read_bytes() == f, p
        lines = stats.read_text().splitlines()
        assert lines == ["%d\t%d\t%d\t%d\t%d\t%s" % ((i,) + st + (NAMES[c],)) for i, (st, c) in enumerate(zip(want_st, want_cls))]
        bin_lines = [l for l in out.splitlines() if l.startswith("bin\t")]
        assert bin_lines == ["bin\t%d\t%d\t%d\t%d\t%d" % ((len(want_cls),) + tuple(want_cls.count(c) for c in range(4)))]
        return out

    check([], dict())
    check(["--bin-min-hits=40", "--bin-ratio=2.5", "--a-lower=2", "--b-upper=3"],
          dict(min_hits=40, ratio_milli=2500, a_range=(2, None), b_range=(1, 3)))
    # together with --joint-histo: both run, each with its own line
    j = tmp_path / "joint.tsv"
    out = check(["--joint-histo=%s" % j], dict())
    assert j.exists() and any(l.startswith("joint\t") for l in out.splitlines())
