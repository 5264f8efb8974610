"""Read correction on the GPU (tsx_hip_correct_*, tsxcount_amd.correct): every case compares the device's corrections,
totals and output bytes with the CPU model (correct_model: the text and a Counter of the counted k-mers, nothing of the
device path) for exact equality.

Inputs: a random genome of 3,000 bases, error-free reads of length L = max(100, 2k + 40) tiled over it every L // 10
bases (about 10x) fill the table, the query reads are drawn from the genome's interior and get their errors planted.
The planted-substitution cases first assert on the CPU that the model alone restores every planted read; that holds
for the seeds recorded here (SEED below; 4^k >> 3,000 makes a chance hit of a wrong alternative unlikely, the assertion
makes it certain)."""
import os
import random
from collections import Counter

import numpy as np
import pytest

SEED = 9100   # genome and reads of case (k, canonical) come from Random(SEED + 2 * k + canonical)
GENOME_LEN = 3000


def read_len(k):
    return max(100, 2 * k + 40)


def sub(read, at, to=None):
    r = bytearray(read)
    for p in at:
        r[p] = to if to is not None else b"CGTA"[b"ACGT".index(bytes([r[p] & 0xDF]))] | (r[p] & 0x20)
    return bytes(r)


def fastq(seqs, pad=0):
    return b"".join(b"@r%d%s\n%s\n+\n%s\n" % (i, b"x" * (pad if i == 0 else 0), s, b"I" * len(s)) for i, s in enumerate(seqs))


def fasta(seqs):
    return b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def kmer_counts(seqs, k):
    c = Counter()
    for s in seqs:
        for i in range(len(s) - k + 1):
            c[s[i:i + k]] += 1
    return c


class Case:
    """A genome, the reads that fill the table, their k-mer counts."""

    def __init__(self, k, canonical=False, seed=None, extra=()):
        self.k, self.canonical, self.L = k, canonical, read_len(k)
        self.rnd = random.Random(SEED + 2 * k + int(canonical) if seed is None else seed)
        self.genome = bytes(self.rnd.choice(b"ACGT") for _ in range(GENOME_LEN))
        step = self.L // 10
        self.tiles = [self.genome[a:a + self.L] for a in range(0, GENOME_LEN - self.L + 1, step)] + list(extra)
        self.counts = kmer_counts(self.tiles, k)

    def read(self, L=None):
        L = L or self.L
        at = self.rnd.randrange(2 * self.L, GENOME_LEN - 2 * self.L - L)   # the interior: every window is counted ~10 times
        return self.genome[at:at + L]

    def table(self, T, l=16, s=0, **kw):
        m = T.TSXHashMapHIP(l, s, self.k, canonical=self.canonical, **kw)
        m.set_path(1)
        m.set_record_lines(2)
        m.countFastq(fasta(self.tiles))
        return m


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def as_tuples(corr):
    return [(int(c["record"]), int(c["pos"]), int(c["from"]), int(c["to"]), int(c["windows"])) for c in corr]


def compare(T, m, case, text, lpr=4, acgt_only=False, chunk_bytes=0, **rule):
    """Sites, totals and output bytes of the host calls against the model; returns the model's answer."""
    C = T.correct
    m.set_record_lines(lpr)
    out, fixes, tot = C.correct_model(text, case.counts, case.k, canonical=case.canonical, acgt_only=acgt_only,
                                      lines_per_record=lpr, **rule)
    corr, ctot = C.correction_sites(m, text, chunk_bytes=chunk_bytes, **rule)
    print("model", tot, "device", ctot)
    assert as_tuples(corr) == fixes
    assert ctot == dict(tot, bytes=0)
    got, gtot = C.correct_reads(m, text, None, chunk_bytes=chunk_bytes, **rule)
    assert len(got) == len(text) and got == out
    assert gtot == tot
    assert [i for i in range(len(text)) if got[i] != text[i]] == sorted(_positions(text, lpr, fixes))
    return out, fixes, tot


def _positions(text, lpr, fixes):
    """Text offsets of the corrected bytes: the start of every record's sequence line + pos."""
    starts, pos, lines = [], 0, 0
    for part in text.split(b"\n"):
        if part:
            if lines % lpr == 1:
                starts.append(pos)
            lines += 1
        pos += len(part) + 1
    return [starts[f[0]] + f[1] for f in fixes]


def on_device(T, m, text, lpr, **rule):
    """(sorted corrections, totals, out-of-place bytes, in-place bytes) of the device entries."""
    import torch
    C = T.correct
    m.set_record_lines(lpr)
    n = len(text)
    dev = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
    dev[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    cap = n // 16 + 16
    dcorr = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda:0")
    nc, tot = C.correction_sites_device(m, dev.data_ptr(), n, dcorr.data_ptr(), cap, **rule)
    corr = np.frombuffer(dcorr.cpu().numpy().tobytes(), dtype=C.CORRECTION_DTYPE)[:nc]
    corr = sorted(as_tuples(corr))
    dout = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
    tot2 = C.correct_reads_device(m, dev.data_ptr(), n, dout.data_ptr(), **rule)
    out = bytes(dout[:n].cpu().numpy())
    tot3 = C.correct_reads_device(m, dev.data_ptr(), n, dev.data_ptr(), **rule)
    assert tot2 == tot3 and tot2 == dict(tot, bytes=n)
    return corr, tot2, out, bytes(dev[:n].cpu().numpy())


def planted(case, copies=1):
    """Reads with one substitution at each boundary position of the three clauses, and the reads they came from."""
    k, L = case.k, case.L
    clean, bad = [], []
    for _ in range(copies):
        for p in (0, 1, k - 2, k - 1, k, L // 2, L - k - 1, L - k, L - 2, L - 1):
            r = case.read()
            clean.append(r)
            bad.append(sub(r, [p]))
        r = case.read()
        clean.append(r)
        bad.append(r)
    return clean, bad


WIDTHS = [15, 31, 32, 33, 63, 65, 96, 127]   # one limb: 15-32; two: 33, 63; three: 65, 96; four: 127


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", WIDTHS)
def test_planted_substitutions_at_every_key_width(T, k, canonical):
    case = Case(k, canonical)
    clean, bad = planted(case, copies=20)   # 220 reads
    text = fastq(bad)
    out, fixes, tot = T.correct.correct_model(text, case.counts, k, canonical=canonical)
    assert out == fastq(clean) and tot["corrected"] == 200 == tot["sites"]   # the model alone restores every planted read
    m = case.table(T)
    try:
        assert compare(T, m, case, text)[0] == out
        corr, dtot, dout, inplace = on_device(T, m, text, 4)
        assert corr == fixes and dtot == tot and dout == out and inplace == out
        # a second call on the output changes nothing
        assert compare(T, m, case, out)[1] == []
    finally:
        m.close()


@pytest.mark.gpu
def test_palindromic_flanks_on_a_canonical_table():
    """A read that is its own reverse complement around the error: rc(window) is another window of the same read, so for
    half of the windows the reverse strand's key is the smaller one and hr ^ H[k - 1 - j] decides."""
    import tsxcount_amd as T
    if T.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    k = 31
    case = Case(k, True)
    half = case.read(60)
    pal = half + half[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))   # 120 bases, pal == rc(pal)
    case = Case(k, True, extra=[pal] * 3)
    bad = [sub(pal, [p]) for p in (0, 40, 59, 60, 80, 119)] + [pal]
    text = fastq(bad)
    out, fixes, tot = T.correct.correct_model(text, case.counts, k, canonical=True)
    assert out == fastq([pal] * 7) and tot["corrected"] == 6
    m = case.table(T)
    try:
        compare(T, m, case, text)
    finally:
        m.close()


@pytest.fixture(scope="module")
def case21(T):
    case = Case(21)
    m = case.table(T)
    yield case, m
    m.close()


@pytest.mark.gpu
def test_two_substitutions_in_one_read(T, case21):
    case, m = case21
    k = case.k
    r = [case.read() for _ in range(4)]
    bad = [sub(r[0], [30, 30 + k + 1]), sub(r[1], [30, 30 + k]), sub(r[2], [30, 35]), sub(r[3], [0, case.L - 1])]
    out, fixes, tot = compare(T, m, case, fastq(bad))
    assert out == fastq([r[0], bad[1], bad[2], r[3]]) and tot["sites"] == 4


@pytest.mark.gpu
def test_ambiguous_unfixable_and_bytes_that_are_no_base(T):
    k = 21
    base = Case(k)
    r = base.read()
    bad = sub(r, [50])
    other = sub(r, [50], to=[b for b in b"ACGT" if b not in (r[50], bad[50])][0])
    noise = bytes(base.rnd.choice(b"ACGT") for _ in range(base.L))
    case = Case(k, extra=[other] * 3)   # two alternatives at base 50 are solid
    def pick(cond):
        while True:
            r = case.read()
            if cond(r):
                return r

    # an N codes for A: where the read has another base the N breaks its windows under either rule, and the site's
    # suspect byte is no base; where the read has an A the default rule does not see the N at all
    n_mid = sub(pick(lambda r: r[40] != ord("A")), [40], to=ord("N"))
    n_two = sub(sub(pick(lambda r: r[45] == ord("A")), [40]), [45], to=ord("N"))
    lower = case.read()
    lower = sub(lower[:30] + lower[30:70].lower() + lower[70:], [50])
    two_head = sub(case.read(), [0, 5])   # a head run of six windows: no base at 5 repairs the window that holds base 0
    seqs = [bad, noise, n_mid, n_two, lower, two_head, case.read()]
    for acgt_only in (False, True):
        m = case.table(T, acgt_only=acgt_only)
        try:
            out, fixes, tot = compare(T, m, case, fastq(seqs), acgt_only=acgt_only)
            assert (tot["ambiguous"], tot["unfixable"]) == (1, 2)
            # the second N: invisible to the default rule (the error at 40 is undone), one long run under acgt_only
            assert [f[:2] for f in fixes] == ([(4, 50)] if acgt_only else [(3, 40), (4, 50)])
            assert sum(out.count(c) for c in b"acgt") == 40
            corr, dtot, dout, inplace = on_device(T, m, fastq(seqs), 4)
            assert corr == fixes and dout == out and inplace == out
        finally:
            m.close()


def pick(case, cond):
    while True:
        r = case.read()
        if cond(r):
            return r


@pytest.mark.gpu
@pytest.mark.parametrize("k,canonical", [(21, False), (31, True), (63, True), (96, False), (127, True)])
def test_a_second_n_inside_a_site(T, k, canonical):
    """An N in a window of a head or tail site, where the read has an A (the code an N gets): the default rule does not
    see it and undoes the error; under acgt_only the windows that hold the N are dropped, no alternative makes them solid
    and the site is unfixable.  The N's place among the bases the site covers is 2, k - 3 and k + 2: at k = 63 and above
    the last two lie behind base 64 of the stage (lanes 16 and up), where the prefix counts of earlier lanes matter."""
    case = Case(k, canonical)
    L, A = case.L, ord("A")
    seqs = [sub(sub(pick(case, lambda r: r[2] == A), [5]), [2], to=ord("N")),                # head run 0..5, p = 5
            sub(sub(pick(case, lambda r: r[k - 3] == A), [k - 1]), [k - 3], to=ord("N")),    # head run 0..k-1, p = k - 1
            sub(sub(pick(case, lambda r: r[L - 3] == A), [L - 6]), [L - 3], to=ord("N")),    # tail run of 6, p = L - 6
            sub(case.read(), [L // 2]), case.read()]
    text = fastq(seqs)
    for acgt_only in (False, True):
        m = case.table(T, acgt_only=acgt_only)
        try:
            out, fixes, tot = compare(T, m, case, text, acgt_only=acgt_only)
            assert (tot["sites"], tot["corrected"], tot["unfixable"]) == ((4, 1, 3) if acgt_only else (4, 4, 0))
            corr, dtot, dout, inplace = on_device(T, m, text, 4)
            assert corr == fixes and dtot == tot and dout == out and inplace == out
        finally:
            m.close()


@pytest.mark.gpu
def test_empty_lines_behind_the_last_record_are_output(T, case21):
    """The output is the input byte for byte, also where a piece holds no record: empty lines behind the last record with
    a seam in front of them, and a text of empty lines only."""
    case, m = case21
    clean, bad = planted(case)
    body = fastq(bad[:4])
    for text, chunks in ((body + b"\n\n\n", (0, len(body), len(body) + 1, 300)), (b"\n", (0,)), (b"\n\n\n\n\n", (0, 2))):
        for chunk in chunks:
            out, fixes, tot = compare(T, m, case, text, chunk_bytes=chunk)
            assert tot["bytes"] == len(text) and len(fixes) == (4 if len(text) > 5 else 0)


@pytest.mark.gpu
def test_upper_and_carried_counts(T):
    k = 21
    base = Case(k)
    rep = base.read()
    case = Case(k, extra=[rep] * 40)      # the windows of rep are counted ~50 times
    clean, bad = planted(case, copies=2)
    seqs = bad + [sub(rep, [50]), rep]
    for s_bits in (0, 2):                 # 2: counters of two bits, every count above 3 lives in the secondary array
        m = case.table(T, s=s_bits, l=16)
        try:
            if s_bits:
                assert m.stats()["overflow_carries"] > 0
            for rule in (dict(), dict(upper=30), dict(lower=5), dict(lower=5, upper=30), dict(lower=45)):
                compare(T, m, case, fastq(seqs), **rule)
        finally:
            m.close()


@pytest.mark.gpu
def test_min_windows(T, case21):
    case, m = case21
    clean, bad = planted(case, copies=2)
    seen = set()
    for mw in (1, 3, case.k):
        seen.add(compare(T, m, case, fastq(bad), min_windows=mw)[2]["sites"])
    assert len(seen) == 3


@pytest.mark.gpu
def test_record_shapes(T, case21):
    case, m = case21
    k = case.k
    clean, bad = planted(case)
    compare(T, m, case, fasta(bad), lpr=2)
    body = (b"\n\n@a\n" + bad[0] + b"\n\n+\n" + b"I" * case.L + b"\n\n\n@b\n" + bad[5] + b"\n+\n" + b"J" * 40 + b"\n"
            b"@short\n" + case.read(k - 1) + b"\n+\n!\n@k\n" + case.read(k) + b"\n+\n!\n@k1\n" + sub(case.read(k + 1), [0]) +
            b"\n+\n!\n@last\n" + bad[9])
    for text in (body, body + b"\n+\n" + b"I" * 7, body + b"\n+", b"@only\n", b""):
        compare(T, m, case, text)
        compare(T, m, case, text, lpr=2)
        if text:
            corr, dtot, dout, inplace = on_device(T, m, text, 4)
            assert dout == T.correct.correct_model(text, case.counts, k)[0] == inplace


@pytest.mark.gpu
def test_a_long_read(T):
    """70,000 bases, ten planted errors: more than CORRECT_LONG_WORDS bitmap words, the wave walks the record."""
    k = 21
    rnd = random.Random(SEED + 777)
    long = bytes(rnd.choice(b"ACGT") for _ in range(70000))
    case = Case(k, extra=[long, long])
    at = [0, 63, 130, 5000, 5000 + k + 1, 5100, 33333, 40000 - 1, 69950, 69999]   # head, word seams, k + 1 apart, tail
    bad = sub(long, at)
    text = b">long\n" + bad + b"\n" + fasta([sub(case.read(), [3])])
    m = case.table(T, l=19)
    try:
        out, fixes, tot = compare(T, m, case, text, lpr=2)
        assert tot["sites"] == 11 == tot["corrected"] and out == b">long\n" + long + b"\n" + out[70007:]
        compare(T, m, case, text, lpr=2, chunk_bytes=20000)
        corr, dtot, dout, inplace = on_device(T, m, text, 2)
        assert corr == fixes and dout == out and inplace == out
    finally:
        m.close()


@pytest.mark.gpu
def test_seams_of_pieces_and_windows(T, monkeypatch):
    case = Case(21)
    clean, bad = planted(case, copies=10)
    text = fastq(bad, pad=5)
    want = T.correct.correct_model(text, case.counts, 21)
    assert len(text) > 12 * 1300
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "1300")   # read when the map is made: a dozen pieces and more
    m = case.table(T)
    try:
        assert compare(T, m, case, text) == want
        assert compare(T, m, case, text, chunk_bytes=700) == want
        for win in ("4096", "4400"):                      # 4400: no multiple of a record (217 bytes), nor of 64
            monkeypatch.setenv("TSX_HIP_DEV_WINDOW", win)
            corr, dtot, dout, inplace = on_device(T, m, text, 4)
            assert (corr, dtot, dout) == (want[1], want[2], want[0]) and inplace == dout
        monkeypatch.delenv("TSX_HIP_DEV_WINDOW")
        corr, dtot, dout, inplace = on_device(T, m, text, 4)
        assert (corr, dtot, dout) == (want[1], want[2], want[0])
    finally:
        m.close()


@pytest.mark.gpu
def test_output_to_a_descriptor_and_a_small_cap(T, case21, tmp_path):
    case, m = case21
    C = T.correct
    clean, bad = planted(case, copies=2)
    text = fastq(bad)
    m.set_record_lines(4)
    out, fixes, tot = C.correct_model(text, case.counts, case.k)
    path = str(tmp_path / "corrected.fq")
    assert C.correct_reads(m, text, path) == tot and open(path, "rb").read() == out
    fd = os.open(path, os.O_WRONLY | os.O_TRUNC)
    try:
        assert C.correct_reads(m, text, fd) == tot
    finally:
        os.close(fd)
    assert open(path, "rb").read() == out == C.correct_reads(m, text)[0]
    # a small cap: ERANGE, the first cap of the sorted order written, the count reported
    rule = C.correct_rule()
    room = np.zeros(5, dtype=C.CORRECTION_DTYPE)
    n, ctot = T.ctypes.c_size_t(0), T._abi.CorrectTotals()
    rc = T.lib().tsx_hip_correct_sites_host(m.handle, text, len(text), T.ctypes.byref(rule), room.ctypes.data_as(T.ctypes.c_void_p), 5,
                                            T.ctypes.byref(n), T.ctypes.byref(ctot), 0)
    assert rc == T.ERANGE and n.value == len(fixes) == 20 and as_tuples(room) == fixes[:5]
    with pytest.raises(T.TSXException) as e:
        C.correction_sites(m, text, cap=3)
    assert e.value.code == T.ERANGE
    import torch
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    dcorr = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(T.TSXException) as e:
        C.correction_sites_device(m, dev.data_ptr(), len(text), dcorr.data_ptr(), 4)
    assert e.value.code == T.ERANGE
    got = as_tuples(np.frombuffer(dcorr.cpu().numpy().tobytes(), dtype=C.CORRECTION_DTYPE))
    assert len(set(got)) == 4 and set(got) <= set(fixes)


@pytest.mark.gpu
def test_refusals(T, case21):
    case, m = case21
    C, L, ct = T.correct, T.lib(), T.ctypes
    text = fastq([case.read()])
    m.set_record_lines(4)

    def refused(handle, rule, words):
        for rc in (L.tsx_hip_correct_sites_host(handle, text, len(text), rule, None, 0, None, None, 0),
                   L.tsx_hip_correct_reads_host(handle, text, len(text), rule, 1, 0, None),
                   L.tsx_hip_correct_sites_device(handle, None, 0, rule, None, 0, None, None, None),
                   L.tsx_hip_correct_reads_device(handle, None, 0, rule, None, 0, None, None)):
            assert rc == T.EINVAL and words in L.tsx_hip_last_error().decode(), (rc, L.tsx_hip_last_error())

    R = T._abi.CorrectRule
    refused(m.handle, None, "no rule")
    refused(m.handle, ct.byref(R(3, 2, 1, 0)), "lower > upper")
    refused(m.handle, ct.byref(R(2, 9, 0, 0)), "min_windows")
    refused(m.handle, ct.byref(R(2, 9, case.k + 1, 0)), "min_windows")
    refused(m.handle, ct.byref(R(2, 9, 1, 7)), "reserved")
    q = T.TSXHashMapHIP(14, 0, case.k, min_qual_char="5")
    sh = T.TSXHashMapHIP(14, 0, case.k, shard_bits=1)
    try:
        refused(q.handle, ct.byref(C.correct_rule()), "min_qual_char")
        refused(sh.handle, ct.byref(C.correct_rule()), "shard_bits")
    finally:
        q.close()
        sh.close()
    with pytest.raises(T.TSXException) as e:
        C.correction_sites(m, text, min_windows=0)
    assert e.value.code == T.EINVAL and "min_windows" in str(e.value)
