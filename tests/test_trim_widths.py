"""Read trimming at every key width (1-4 limbs), with carried counts, homopolymer stretches, wide window halos, canonical
tables and base rules at wide keys.

Expectations are the Python restatement of test_trim.py (solid_flags, pick_span, expected_trim) over coded_counts of the
counted text.  Never the library under test.  Spans, output bytes and totals are compared exactly; the forms a case is
about (an empty span, a cut at base 0, a run across a seam, ...) are asserted from the restatement before any GPU call."""
import random
import re

import pytest

from test_read_query import coded_counts, line_spans, rc
from test_trim import check_text, expected_trim, fasta, fastq, genome_map, pick_span, sub

# key limbs of every k of the width test: (2 k + 63) / 64
LIMBS = {5: 1, 15: 1, 16: 1, 31: 1, 32: 1, 33: 2, 47: 2, 63: 2, 64: 2, 65: 3, 95: 3, 96: 3, 97: 4, 127: 4}


def letters(k):
    return b"ACG" if k < 8 else b"ACGT"   # k = 5: at most 3^5 distinct k-mers in a 2^9-slot table


def table_l(k):
    return 9 if k == 5 else 17


def random_bases(rnd, n, alphabet=b"ACGT"):
    return bytes(rnd.choice(alphabet) for _ in range(n))


def sub_k(read, positions, k):
    """sub(); at k < 8 the genome holds every k-mer of its three letters and no T, so a T is what makes a window unseen."""
    if k >= 8:
        return sub(read, positions)
    r = bytearray(read)
    for p in positions:
        r[p] = ord("T")
    return bytes(r)


def unseen(rnd, n, k):
    if k >= 8:
        return random_bases(rnd, n)
    return bytes(ord("T") if i % 3 == 2 else rnd.choice(b"ACG") for i in range(n))


def read_len(k):
    return 4 * k + 70


N_FORMS = 13   # reads of one copy of scaled_reads


def scaled_reads(rnd, genome, k, copies=1):
    """planted_reads of test_trim.py with lengths and plants scaled to k: none, base 0, the last base, the middle, two at
    distance < k, = k and > k, a tie, lengths k - 1, k and k + 1, no solid window, solid throughout."""
    L = read_len(k)
    plants = ([], [0], [L - 1], [L // 2], [k + 10, k + 10 + max(1, k // 2)], [k + 10, 2 * k + 10], [k + 5, 3 * k + 60])
    seqs = []
    for _ in range(copies):
        for pl in plants:
            at = rnd.randrange(0, len(genome) - L - 1)
            seqs.append(sub_k(genome[at:at + L], pl, k))
        at = rnd.randrange(0, len(genome) - L - 1)
        seqs.append(sub_k(genome[at:at + L + 1], [L // 2], k))   # a tie: L / 2 bases on either side
        seqs += [genome[at:at + k - 1], genome[at:at + k], genome[at:at + k + 1]]
        seqs.append(unseen(rnd, L, k))
        seqs.append(genome[at:at + L])
    assert len(seqs) == copies * N_FORMS
    return seqs


def assert_forms(want, pre, k):
    """The spans of the first copy of scaled_reads, from the restatement: longest mode and prefix mode."""
    L = read_len(k)
    assert want[:4] == [(0, L), (1, L - 1), (0, L - 1), (0, L // 2)]
    assert want[4] == (k + 11 + max(1, k // 2), L - (k + 11 + max(1, k // 2)))
    assert want[5] == (2 * k + 11, L - (2 * k + 11)) and want[6] == (k + 6, 2 * k + 54)
    assert want[7:13] == [(0, L // 2), (0, 0), (0, k), (0, k + 1), (0, 0), (0, L)]   # tie, k - 1, k, k + 1, none, all
    assert pre[1] == (0, 0) and pre[4] == (0, k + 10) and pre[6] == (0, k + 5) and pre[9] == (0, k)
    assert (0, 0) in want and (0, L) in want and any(s > 0 for s, _ in want) and any(n == k for _, n in want)


def reads_up_to(rnd, genome, k, fmt, nbytes):
    seqs = scaled_reads(rnd, genome, k)
    while len(fmt(seqs)) < nbytes:
        seqs += scaled_reads(rnd, genome, k)
    return seqs


def rule_kw(lower, upper):
    return dict(lower=lower) if upper is None else dict(lower=lower, upper=upper)


# ---- CPU --------------------------------------------------------------------------------------------------------------

def brute_span(flags, k, mode):
    """The longest stretch of consecutive set flags over all (start, length) pairs, the leftmost among equals; prefix mode:
    stretches that start at flag 0 only.  length counts bases: windows + k - 1."""
    best = (0, 0)
    for start in range(len(flags)):
        if mode == "prefix" and start > 0:
            break
        for nwin in range(1, len(flags) - start + 1):
            if not all(flags[start:start + nwin]):
                break
            if nwin + k - 1 > best[1]:
                best = (start, nwin + k - 1)
    return best


def test_pick_span_equals_brute_force():
    rnd = random.Random(4242)
    seen = set()
    for i in range(3000):
        n = rnd.randint(0, 40)
        p = (0.3, 0.6, 0.9, 1.0)[i % 4]
        flags = [rnd.random() < p for _ in range(n)]
        for k in (1, 3, 8):
            for mode in ("longest", "prefix"):
                want = brute_span(flags, k, mode)
                assert pick_span(flags, k, mode) == want, (flags, k, mode)
                seen.add((want == (0, 0), want[0] > 0))
    assert seen == {(True, False), (False, False), (False, True)}
    # ties and the prefix rule, spelled out
    t, f = True, False
    assert pick_span([t, t, f, t, t], 3, "longest") == (0, 4) and pick_span([f, t, t, f, t, t], 3, "longest") == (1, 4)
    assert pick_span([f, t, t], 3, "prefix") == (0, 0) and pick_span([t, f, t, t], 3, "prefix") == (0, 3)
    assert pick_span([], 3, "longest") == (0, 0) and pick_span([t], 8, "prefix") == (0, 8)


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def to_device(text):
    import torch
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(LIMBS))
def test_every_key_width(T, k, tmp_path):
    rnd = random.Random(7000 + k)
    genome = random_bases(rnd, 4000, letters(k))
    counted = fasta([genome])
    counts = coded_counts(counted, k, 2)
    texts = []
    for lpr, fmt in ((4, fastq), (2, fasta)):
        text = fmt(reads_up_to(rnd, genome, k, fmt, 10000))
        assert 10000 <= len(text) <= 30000
        chunk = len(text) // 6   # pieces hold whole records and at most `chunk` bytes: at least 6 of them
        assert chunk >= 2 * read_len(k) + 32
        want, _, _ = expected_trim(text, counts, k, lpr)
        pre, _, _ = expected_trim(text, counts, k, lpr, mode="prefix")
        assert_forms(want, pre, k)
        texts.append((lpr, text, chunk))
    for path in (1, 2):
        m = genome_map(T, k=k, l=table_l(k), counted=counted, path=path)
        assert m.wk == LIMBS[k]
        for lpr, text, chunk in texts:
            check_text(m, text, lpr, tmp_path, counts=counts, k=k, chunks=(0, chunk))
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 65, 127])
def test_seams_at_wide_keys(T, k, tmp_path):
    """The first header grows by 0..70 bytes over a text of more than two tiles: the k-byte windows of every read move over
    every offset of the 64-position bitmap words and of the 128-byte halo behind a 4 KiB tile."""
    rnd = random.Random(7200 + k)
    genome = random_bases(rnd, 4000)
    counted = fasta([genome])
    counts = coded_counts(counted, k, 2)
    seqs = reads_up_to(rnd, genome, k, fastq, 2 * 4096 + 1)
    want, _, _ = expected_trim(fastq(seqs), counts, k, 4)
    pre, _, _ = expected_trim(fastq(seqs), counts, k, 4, mode="prefix")
    assert_forms(want, pre, k)
    m = genome_map(T, k=k, l=17, counted=counted)
    assert m.wk == LIMBS[k]
    for pad in range(71):
        text = fastq(seqs, pad)
        assert 2 * 4096 < len(text) <= 30000
        got = check_text(m, text, 4, tmp_path, counts=counts, k=k, modes=("longest",) if pad % 8 else ("longest", "prefix"))
        assert got == want   # the header is no part of a span
    check_text(m, fasta(seqs, 33), 2, tmp_path, counts=counts, k=k)
    m.close()


@pytest.mark.gpu
def test_a_long_record_at_k127(T, tmp_path):
    k = 127
    rnd = random.Random(7327)
    genome = random_bases(rnd, 6000)
    counted = fasta([genome])
    counts = coded_counts(counted, k, 2)
    long = genome[300:5300]
    bad = sub(long, [1500, 1900, 4000])
    text = b">clean\n" + long + b"\n>three\n" + bad + b"\n" + fasta([genome[100:500]])
    want, _, _ = expected_trim(text, counts, k, 2)
    pre, _, _ = expected_trim(text, counts, k, 2, mode="prefix")
    assert want == [(0, 5000), (1901, 2099), (0, 400)]   # more than 64 bitmap words; the longest run is the third
    assert pre[1] == (0, 1500)
    m = genome_map(T, k=k, l=17, counted=counted)
    assert check_text(m, text, 2, tmp_path, counts=counts, k=k, chunks=(0, 3000)) == want
    m.close()


WINDOWS = (4096, 5000)


def window_bytes(win):
    return (win + 63) // 64 * 64   # the spans entry point works in whole bitmap words


def seam_cases(text, spans, k, win):
    """(a solid run with window starts on both sides of a window seam, a read whose sequence line ends within k - 1 bytes
    after a seam and whose last solid window starts before the seam), from the line offsets."""
    return seam_cases_at(line_spans(text), len(text), spans, k, win)


def seam_cases_at(sp, n, spans, k, win):
    crossing = tail = False
    for r, (start, length) in enumerate(spans):
        if not length:
            continue
        a, b = sp[4 * r + 1]
        first, last = a + start, a + start + length - k
        for seam in range(win, n, win):
            crossing |= first < seam <= last
            tail |= seam < b <= seam + k - 1 and last < seam < last + k
    return crossing, tail


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 127])
def test_device_windows_with_a_wide_halo(T, k, tmp_path, monkeypatch):
    import torch
    rnd = random.Random(7400 + k)
    genome = random_bases(rnd, 4000)
    counted = fasta([genome])
    counts = coded_counts(counted, k, 2)
    wins = [window_bytes(w) for w in WINDOWS]
    seqs = reads_up_to(rnd, genome, k, fastq, 4 * max(wins) + 600)   # >= 5 windows of either size, whatever the padding
    want, _, _ = expected_trim(fastq(seqs), counts, k, 4)
    sp0, n0 = line_spans(fastq(seqs)), len(fastq(seqs))

    def padded(p):   # the line offsets with the first header p bytes longer
        return [(a + (p if i else 0), b + p) for i, (a, b) in enumerate(sp0)]

    pad = next(p for p in range(500) if all(all(seam_cases_at(padded(p), n0 + p, want, k, w)) for w in wins))
    text = fastq(seqs, pad)
    assert 4 * max(wins) < len(text) <= 30000
    for w in wins:
        assert seam_cases(text, want, k, w) == (True, True)
    m = genome_map(T, k=k, l=17, counted=counted)
    m.set_record_lines(4)
    dev = to_device(text)
    for mode in ("longest", "prefix"):
        spans, out, tot = expected_trim(text, counts, k, 4, mode=mode)
        assert mode == "prefix" or spans == want
        rule = T.trim_rule(1, None, mode)
        one_window = None
        for win in (None,) + WINDOWS:
            if win:
                monkeypatch.setenv("TSX_HIP_DEV_WINDOW", str(win))
            else:
                monkeypatch.delenv("TSX_HIP_DEV_WINDOW", raising=False)
            dsp = torch.full((len(spans) + 3, 2), -1, dtype=torch.int64, device="cuda:0")
            assert m.trimSpansDevice(dev.data_ptr(), len(text), dsp.data_ptr(), len(spans) + 3, rule) == len(spans)
            got = [tuple(r) for r in dsp.cpu().numpy().tolist()]
            one_window = got if one_window is None else one_window
            assert got == one_window, (mode, win)
            assert got[:len(spans)] == spans, (mode, win)
            assert got[len(spans):] == [(0, 0)] * 3
            dout = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
            dtot = m.trimReadsDevice(dev.data_ptr(), len(text), dout.data_ptr(), len(text) + 64, rule)
            assert dtot == tot, (mode, win)
            assert bytes(dout[:tot["bytes"]].cpu().numpy()) == out, (mode, win)
        monkeypatch.delenv("TSX_HIP_DEV_WINDOW", raising=False)
    m.close()


MULT = [1, 3, 4, 5, 17, 40, 70, 130]


def tiled_genome(rnd, k, order):
    """A genome whose start positions form len(order) regions, and the records that count the k-mers of region i
    order[i] times: the genome once, then order[i] - 1 times the region with the k - 1 bases behind it."""
    bounds = [0]
    for _ in order:
        bounds.append(bounds[-1] + rnd.randint(30, 80))
    g = random_bases(rnd, bounds[-1] + k - 1)
    recs = [g]
    for i, mult in enumerate(order):
        recs += [g[bounds[i]:bounds[i + 1] + k - 1]] * (mult - 1)
    return g, recs


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
@pytest.mark.parametrize("s_bits", [1, 2, 3])
def test_carried_counts_move_the_cut(T, k, s_bits, tmp_path):
    rnd = random.Random(7500 + 10 * k + s_bits)
    recs, seqs = [], []
    for order in (MULT, [70, 4, 130, 1, 40, 3, 17, 5]):
        g, r = tiled_genome(rnd, k, order)
        recs += r
        seqs.append(g)   # every read: neighbouring stretches of different multiplicity
        for _ in range(12):
            at = rnd.randrange(0, len(g) // 2)
            seqs.append(g[at:at + rnd.randrange(150 + k, len(g) // 2 + k)])
    rnd.shuffle(recs)
    counted = fasta(recs)
    counts = coded_counts(counted, k, 2)
    assert set(counts.values()) == set(MULT)
    text = fastq(seqs)
    assert len(text) >= 10000
    top = 1 << s_bits
    rules = [(1, None), (top, None), (top - 1, top - 1), (4, 70), (100, None)]
    wants = [expected_trim(text, counts, k, 4, **rule_kw(*r))[0] for r in rules]
    assert all(wants[i] != wants[j] for i in range(len(rules)) for j in range(i))   # every pair of thresholds cuts elsewhere
    assert wants[0][0] == (0, len(seqs[0])) and wants[4][0][0] > 0
    for path in (1, 2):
        m = genome_map(T, k=k, l=18, counted=counted, s=s_bits, path=path)
        assert m.stats()["overflow_carries"] > 0
        for r, want in zip(rules, wants):
            assert check_text(m, text, 4, tmp_path, counts=counts, k=k, chunks=(0, 3000), **rule_kw(*r)) == want, (path, r)
        m.close()


def homopolymer_genome(rnd, k):
    """Random flanks around runs of one base that are 2 k .. 3 k long; N takes the code of A.  Returns the genome and the
    (start, end) of its runs."""
    runs = [b"A" * (2 * k + 7), b"N" * (2 * k + 3), b"C" * (3 * k), b"T" * (2 * k + 1), b"N" * (2 * k + 11), b"A" * (3 * k - 1),
            b"G" * (2 * k + 5)]
    g, at = b"", []
    for i in range(len(runs) + 1):
        f = bytearray(random_bases(rnd, rnd.randint(k + 30, k + 90)))
        for end, run in ((0, runs[i - 1] if i else b""), (-1, runs[i] if i < len(runs) else b"")):
            f[end] = rnd.choice(bytes(set(b"ACGT") - set(run.replace(b"N", b"A"))))   # a run is as long as written
        g += bytes(f)
        if i < len(runs):
            at.append((len(g), len(g) + len(runs[i])))
            g += runs[i]
    return g, at


def stretches_over_a_word_seam(text, k):
    """Homopolymer stretches whose windows start on both sides of a multiple of 64, counted from the text's first byte."""
    n = 0
    for mt in re.finditer(b"|".join(b"%c{%d,}" % (c, 2 * k) for c in b"ACGTN"), text):
        n += mt.start() // 64 != (mt.end() - k) // 64
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 65])
def test_homopolymer_stretches(T, k, tmp_path):
    """Equal k-mers in neighbouring lanes: the count of a stretch comes from its first lane."""
    rnd = random.Random(7600 + k)
    g, runs = homopolymer_genome(rnd, k)
    counted = fasta([g])
    counts = coded_counts(counted, k, 2)
    poly_a = counts[b"A" * k]
    assert poly_a == sum(e - s - k + 1 for (s, e), base in zip(runs, b"ANCTNAG") if base in b"AN") and poly_a > 3 * k
    seqs = [g]
    for s, e in runs:
        seqs += [g[s - k - 10:e + k + 10], g[s - 5:e + 5]]
    n_read, a_read = seqs[3], seqs[1]   # the first N run and the first A run between their flanks
    rules = [(1, None), (1, poly_a - 1), (1, 3), (2, None), (poly_a, None)]
    text = fastq(seqs)
    wants = [expected_trim(text, counts, k, 4, **rule_kw(*r))[0] for r in rules]
    assert wants[0] == [(0, len(s)) for s in seqs]   # all of it is counted text
    assert wants[1][0] != wants[0][0] and wants[2][0] != wants[1][0]   # polyA out of range; every stretch out of range
    assert wants[3][5] == (k + 10, 3 * k)   # the C run alone: 2 k + 1 times polyC, below polyA
    assert wants[4][1] == (k + 10, 2 * k + 7) and wants[4][3] == (k + 10, 2 * k + 3) and wants[4][5] == (0, 0)
    m = genome_map(T, k=k, l=17, counted=counted)
    for pad in range(71):
        text = fastq(seqs, pad)
        assert stretches_over_a_word_seam(text, k) > 0
        for r in (rules if pad in (0, 33) else [rules[pad % len(rules)]]):
            got = check_text(m, text, 4, tmp_path, counts=counts, k=k, modes=("longest",) if pad % 8 else ("longest", "prefix"),
                             **rule_kw(*r))
            assert got == wants[rules.index(r)], (pad, r)
    check_text(m, fasta(seqs, 17), 2, tmp_path, counts=counts, k=k, chunks=(0, 1500))
    # acgt_only: the N run breaks its read, the A run does not (the table keeps its counts: the rule is a query rule here)
    m.set_base_rule(acgt_only=True)
    for pad in range(0, 71, 6):
        text = fastq(seqs, pad)
        for r in (rules[0], rules[1]):
            got = check_text(m, text, 4, tmp_path, counts=counts, k=k, acgt_only=True,
                             modes=("longest",) if pad else ("longest", "prefix"), **rule_kw(*r))
            if r == rules[0]:   # k + 10 bases on either side of the N run: a tie; with five, none
                assert got[3] == (0, k + 10) and got[4] == (0, 0) and got[1] == (0, len(a_read)) and len(n_read) == 4 * k + 23
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [33, 64, 127])
def test_canonical_tables_at_wide_keys(T, k, tmp_path):
    rnd = random.Random(7700 + k)
    genome = random_bases(rnd, 4000)
    pals = []
    if k % 2 == 0:   # palindromes: x == rc(x)
        for _ in range(5):
            h = random_bases(rnd, k // 2)
            pals.append(h + rc(h))
    counted = fasta([genome, rc(genome[1000:2500])] + pals + pals[:2])
    counts = coded_counts(counted, k, 2, canonical=True)
    assert all(counts[p] == (2 if i < 2 else 1) for i, p in enumerate(pals))
    seqs = scaled_reads(rnd, genome, k) + pals
    L = read_len(k)
    m = genome_map(T, k=k, l=17, counted=counted, canonical=True)
    assert m.wk == LIMBS[k]
    fwd = check_text(m, fastq(seqs, 9), 4, tmp_path, counts=counts, k=k, canonical=True, chunks=(0, 2500))
    rev = check_text(m, fastq([rc(s) for s in seqs], 40), 4, tmp_path, counts=counts, k=k, canonical=True, chunks=(0, 2500))
    assert fwd[1] == (1, L - 1) and fwd[2] == (0, L - 1) and rev[1] == (0, L - 1) and rev[2] == (1, L - 1)
    assert fwd[N_FORMS:] == [(0, k)] * len(pals) == rev[N_FORMS:]
    if pals:   # lower = 2: the palindromes counted twice, and what the second strand covers
        two = check_text(m, fastq(seqs + [genome[900:2600]], 3), 4, tmp_path, counts=counts, k=k, canonical=True, lower=2)
        assert two[N_FORMS:] == [(0, k), (0, k), (0, 0), (0, 0), (0, 0), (100, 1500)]
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 65, 127])
def test_base_rules_at_wide_keys(T, k, tmp_path):
    """A break bit of the base rule anywhere in the k bytes of a window: k = 63 has them all in the first mask word, k = 65
    one and k = 127 sixty-three in the second."""
    rnd = random.Random(7800 + k)
    genome = random_bases(rnd, 4000)
    counted = fasta([genome])
    counts = coded_counts(counted, k, 2)
    L = read_len(k)
    n_at, low_at, short = k + 37, 3 * k + 11, 2 * k + 24
    at = genome.index(b"A", 1000 + n_at) - n_at
    read, other = genome[at:at + L], genome[2000:2000 + L]
    withn = read[:n_at] + b"N" + read[n_at + 1:]   # N takes the code of A: solid throughout unless the rule drops the windows
    low = bytearray(b"I" * L)
    low[low_at] = ord("#")
    text = (fastq([withn, read], 21) + b"@low\n" + read + b"\n+\n" + bytes(low) + b"\n"
            + b"@shortq\n" + other + b"\n+\n" + b"J" * short + b"\n" + fastq([other]))
    right = (n_at + 1, L - n_at - 1)   # 3 k + 32 bases behind the N, k + 37 before it
    m = genome_map(T, k=k, l=17, counted=counted)
    assert m.wk == LIMBS[k]
    assert check_text(m, text, 4, tmp_path, counts=counts, k=k) == [(0, L)] * 5
    m.set_base_rule(acgt_only=True)
    assert check_text(m, text, 4, tmp_path, counts=counts, k=k, acgt_only=True) == [right] + [(0, L)] * 4
    m.set_base_rule(min_qual_char="5")
    assert check_text(m, text, 4, tmp_path, counts=counts, k=k, minq=ord("5"), chunks=(0, 1500)) == \
        [(0, L), (0, L), (0, low_at), (0, short), (0, L)]
    m.set_base_rule(acgt_only=True, min_qual_char="5")
    assert check_text(m, text, 4, tmp_path, counts=counts, k=k, acgt_only=True, minq=ord("5"), chunks=(0, 1500)) == \
        [right, (0, L), (0, low_at), (0, short), (0, L)]
    pre, _, _ = expected_trim(text, counts, k, 4, mode="prefix", acgt_only=True, minq=ord("5"))
    assert pre[0] == (0, n_at)
    m.close()
