"""The overflow routes of the partitioned build (full key-log regions, full level-1 and level-2 sub-lists: spill cache,
overflow queues, deferred list) under the modes that have kernels or branches of their own: multi-limb keys, canonical
counting, the base rule, wrapped FASTA, radix levels of 512 lists.

Every expectation is a dictionary count that shares no code with the kernels (conftest.python_counts, folded by strand
with test_canonical.fold; test_base_rule.oracle; test_fasta_wrapped.expected).  The comparison is exact and covers the
whole table: the dump against the dictionary key for key and count for count, the counters of stats(), no failures.

How a case shows that its forced route ran:
  * TSX_HIP_CAP1 and full level-2 sub-lists: walk_part_kernel and partition_ring_kernel count every key that found its
    list full in stats()["fallback_inserts"]; the bound asserted is keys minus the summed capacity of the lists.
  * TSX_HIP_LOG_CAP: the region-full exit of walk_log_kernel / walk_log_wide_kernel appends to the deferred list and
    does NOT count in fallback_inserts (only the two kernels above add to it).  The route is shown by arithmetic instead:
    the scan runs min(tiles, CUs x workgroups per CU) workgroups of 256 threads, one log region per wave, a tile is
    4096 bytes of text -- at most 4 regions per tile (and per host piece one tile more), LOG_CAP keys each; the keys
    that go to the log (all but the homopolymers, which the wave's hot-key cache takes) are asserted to be more than
    twice that."""
import functools
import random

import numpy as np
import pytest

import test_base_rule as base_rule
import test_fasta_wrapped as fasta_wrapped
from conftest import python_counts
from test_canonical import encode, fastq_of, fold, rc, reads_of

TILE = 4096          # bytes of text per scan tile (tsx_kernels.h)
WALK_BYTES = 8192    # bytes of text per workgroup of the fused walk, at least (g_sp in tsxcount_hip.hip)
HOMS = [b"A", b"C", b"G", b"T"]
PIECE = 20000        # TSX_HIP_PIECE_BYTES of the pieced runs: longer than any record, a small part of any text here


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


# ---- texts (each with the facts its case depends on, asserted on the CPU below) ---------------------------------------

def synth_reads(seed, n):
    from tsxcount_amd import synth
    return reads_of(synth.fastq(seed, 0, n))


def n_windows(seqs, k):
    return sum(max(0, len(s) - k + 1) for s in seqs)


@functools.lru_cache(maxsize=None)
def wide_case(k):
    """Case 1: reads with poly-A tails, a read of each base alone, one ordinary read 50 times.  (text, forward counts)"""
    reads = synth_reads(300 + k, 60)
    seqs = reads + [b"A" * 300, b"C" * 260, b"G" * (k + 40), b"T" * (k + 17)] + [reads[0][:400]] * 50
    text = fastq_of(seqs)
    return text, dict(python_counts(text, k))


@functools.lru_cache(maxsize=None)
def canon_case(k):
    """Case 2: reads, reverse complements of some, a read of each base alone, for even k a palindrome five times.
    (text, forward counts, the palindrome or None)"""
    reads = synth_reads(400 + k, 40)
    seqs = reads + [rc(r) for r in reads[:10]] + [b"A" * 300, b"T" * 280, b"C" * (k + 50), b"G" * (k + 30)]
    pal = None
    if k % 2 == 0:
        rnd = random.Random(k)
        half = bytes(rnd.choice(b"ACGT") for _ in range(k // 2))
        pal = half + rc(half)
        seqs += [pal + b"AC"] * 5
    text = fastq_of(seqs)
    return text, dict(python_counts(text, k)), pal


@functools.lru_cache(maxsize=None)
def rule_case(k, acgt, mq, canonical):
    """Cases 3 and 4: clean reads of quality 'I', then test_base_rule's edited reads (N runs, IUPAC and lower-case bytes,
    3 % low qualities, quality lines of other lengths, an unterminated last record).  A quality rule keeps few windows of
    the edited reads at k = 63 (0.97^63): the clean reads keep every list and region over-full under both rules.
    (text, kept, dropped, windows of all sequence lines)"""
    text = fastq_of(synth_reads(700 + k, 80)) + base_rule.edited_text(500 + k, n_reads=40, k=k)
    kept, dropped = base_rule.oracle(text, k, acgt, mq, canonical)
    return text, dict(kept), dropped, n_windows([s for s, _, _ in base_rule.records(text)], k)


@functools.lru_cache(maxsize=None)
def fasta_text(k):
    """Case 3: records wrapped at 60 and 70 columns; every k-mer but the first of a line spans a line break or two."""
    reads = synth_reads(600 + k, 40)
    return b"".join(b">rec%d wrapped at %d\n" % (i, (60, 70)[i % 2]) + fasta_wrapped.wrap(s, (60, 70)[i % 2])
                    for i, s in enumerate(reads))


_fasta_want = {}


def fasta_case(T, k, canonical):
    if (k, canonical) not in _fasta_want:
        _fasta_want[(k, canonical)] = dict(fasta_wrapped.expected(T, fasta_text(k), k, canonical=canonical))
    return fasta_text(k), _fasta_want[(k, canonical)]


def cap_sub(text_bytes, nseg, cpr2=8):
    """plan_partition's capacity of one level-2 sub-list for a FASTQ text counted in one piece: maxrec = bytes / 2 + 65536
    records at most, spread over nseg segments x cpr2 level-2 workgroups per level-1 bucket, plus a quarter, six standard
    deviations and 64, rounded to 16.  cpr2 = min(8, CUs * 8 / level-1 buckets), a power of two: at most 8."""
    per_sub = (text_bytes // 2 + 65536) // nseg // cpr2
    return (per_sub + per_sub // 4 + 6 * int(np.sqrt(per_sub + 1.0)) + 64 + 15) & ~15


def hot_text(k, n_reads):
    rng = np.random.default_rng(77 + k)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    suffix = lut[rng.integers(0, 4, k + 9)].tobytes()          # 10 k-mers that occur once per read
    bodies = lut[rng.integers(0, 4, (n_reads, 30))]
    qual = b"I" * (30 + k + 9)
    return suffix, b"".join(b"@r%d\n" % i + bodies[i].tobytes() + suffix + b"\n+\n" + qual + b"\n" for i in range(n_reads))


# segments of the l = 23 tables of case 5 (derive_layout): k = 31 has one-limb slots in segments of 2^14, 2^9 of them;
# k = 63 two-limb slots in segments of 2^12, 2^11 of them
HOT_NSEG = {31: 1 << 9, 63: 1 << 11}
HOT_SPILLS = 500   # occurrences of every hot k-mer beyond the capacity of all sub-lists of its segment, at least


@functools.lru_cache(maxsize=None)
def hot_case(k):
    """Case 5: every read ends in the same k + 9 bases.  All n occurrences of a hot k-mer belong to one segment, whose
    sub-lists (one per level-2 workgroup of the bucket, at most 8) hold 8 * cap_sub records together -- and cap_sub grows
    with the text (cap_sub above).  The smallest multiple of 500 reads with n >= 8 * cap_sub(text) + HOT_SPILLS:
    each hot k-mer then leaves the fast path at least HOT_SPILLS times, whatever else its segment holds.
    (n, suffix, text, forward counts)"""
    n = 500
    while True:
        suffix, text = hot_text(k, n)
        if n >= 8 * cap_sub(len(text), HOT_NSEG[k]) + HOT_SPILLS:
            return n, suffix, text, dict(python_counts(text, k))
        n += 500


TANDEM_UNIT = 40


@functools.lru_cache(maxsize=None)
def radix512_case(k):
    """Case 6: reads, and 60 reads of 2000 bases that repeat one unit of 40 bases: 40 distinct k-mers, about 50 times per read.
    (text, forward counts, the 40 tandem k-mers)"""
    rnd = random.Random(900 + k)
    unit = bytes(rnd.choice(b"ACGT") for _ in range(TANDEM_UNIT))
    tandem = (unit * (2000 // TANDEM_UNIT + 2))
    seqs = synth_reads(81 + k, 100) + [tandem[:2000]] * 60
    text = fastq_of(seqs)
    return text, dict(python_counts(text, k)), [tandem[i:i + k] for i in range(TANDEM_UNIT)]


# ---- the comparison -----------------------------------------------------------------------------------------------------

def homopolymer_windows(want, k):
    return sum(want.get(b * k, 0) for b in HOMS)


def check_whole_table(T, m, want, k, reps=1):
    """stats and dump against {k-mer bytes: count}, everything counted reps times."""
    total = sum(want.values())
    st = m.stats()
    assert st["distinct"] == len(want), (st, len(want))
    assert st["kmers_added"] == reps * total and st["count_sum"] == reps * total, (st, reps * total)
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0, st
    keys = sorted(want)
    exp_k = encode(keys, k)
    exp_c = np.array([want[x] for x in keys], dtype=np.uint64) * np.uint64(reps)
    got_k, got_c = m.getAllKmers()
    assert len(got_k) == len(keys)
    a, b = np.lexsort(got_k.T[::-1]), np.lexsort(exp_k.T[::-1])
    assert np.array_equal(got_k[a], exp_k[b]), "the table holds other k-mers than the text"
    bad = np.nonzero(got_c[a] != exp_c[b])[0]
    assert bad.size == 0, [(T.decode(exp_k[b][i], k), int(got_c[a][i]), int(exp_c[b][i])) for i in bad[:5]]
    for row, c in zip(got_k[:50], got_c[:50]):          # the decoder agrees with the encoder used above
        assert want[T.decode(row, k).encode()] * reps == int(c)
    assert np.array_equal(m.getKmerCounts(exp_k), exp_c)
    return st


def check_both_strands(m, want, k, reps=1, step=7):
    keys = sorted(want)[::step]
    exp = np.array([want[x] for x in keys], dtype=np.uint64) * np.uint64(reps)
    assert np.array_equal(m.getKmerCounts(encode(keys, k)), exp)
    assert np.array_equal(m.getKmerCounts(encode([rc(x) for x in keys], k)), exp)


def log_keys_needed(text, log_cap, pieces=1):
    """Twice what all log regions hold together (module docstring)."""
    return 2 * 4 * (-(-len(text) // TILE) + pieces) * log_cap


def fused_lists_hold(text, nb1, cap1, pieces=1, buckets=None):
    """What the level-1 sub-lists of the fused walk hold together, at most: one workgroup per 8192 bytes of text or fewer
    (and one more per host piece), each with one list of cap1 keys per level-1 bucket; `buckets`: those that a given set of
    keys can reach."""
    return (-(-len(text) // WALK_BYTES) + pieces) * (nb1 if buckets is None else min(nb1, buckets)) * cap1


# ---- 7. the inputs, on the CPU ------------------------------------------------------------------------------------------

WIDE_KS = [33, 63, 64, 96, 127]
CANON_KS = [31, 32, 63, 96]
FUSED_KS = [21, 31]
FUSED_MODES = [(False, None, True), (True, None, False), (False, "5", False), (True, "5", True)]   # acgt, min qual, canonical
RULE_WIDE = [(33, True, None, False), (33, False, "5", False), (33, True, "5", False),
             (63, True, None, False), (63, False, "5", False), (63, True, "5", False), (63, True, None, True)]


@pytest.mark.parametrize("k", WIDE_KS)
def test_input_wide(k):
    text, want = wide_case(k)
    for b, n in ((b"A", 300), (b"C", 260), (b"G", k + 40), (b"T", k + 17)):     # runs longer than k, of every base
        assert want[b * k] >= n - k + 1 > 1
    read = reads_of(text)[0][:400]
    hot = [read[i:i + k] for i in range(400 - k + 1)]
    assert len(set(hot)) == len(hot) and all(want[x] >= 50 for x in hot)        # the repeated read: counts carry at s = 2
    assert sum(1 for c in want.values() if c >= 4) >= len(hot) + 4
    for cap in (64, 16):
        assert sum(want.values()) - homopolymer_windows(want, k) > log_keys_needed(text, cap)


@pytest.mark.parametrize("k", CANON_KS)
def test_input_canonical(k):
    text, fwd, pal = canon_case(k)
    want = fold(fwd)
    assert len(want) < len(fwd)                                                 # both strands of some k-mers occur
    reads = reads_of(text)
    both = [x for x in (reads[0][i:i + k] for i in range(0, 400, 13)) if rc(x) in fwd]
    assert both and all(want[min(x, rc(x))] == fwd[x] + fwd[rc(x)] for x in both)
    # (the reads end in poly-A tails, their reverse complements begin with poly-T)
    assert fwd[b"A" * k] > 300 - k and fwd[b"T" * k] > 280 - k and fwd[b"C" * k] == 51 and fwd[b"G" * k] == 31
    assert want[b"A" * k] == fwd[b"A" * k] + fwd[b"T" * k] and want[b"C" * k] == 82
    if k % 2 == 0:
        assert pal == rc(pal) and fwd[pal] == 5 == want[pal]
    else:
        assert pal is None
    assert sum(want.values()) - homopolymer_windows(want, k) > log_keys_needed(text, 64)


@pytest.mark.parametrize("k", FUSED_KS)
@pytest.mark.parametrize("acgt,mq,canonical", FUSED_MODES)
def test_input_fused_rules(k, acgt, mq, canonical):
    text, kept, dropped, windows = rule_case(k, acgt, mq, canonical)
    assert any(b not in base_rule.ACGT for s, _, _ in base_rule.records(text) for b in s)
    assert any(q < ord("5") for _, ql, _ in base_rule.records(text) for q in ql)
    total = sum(kept.values())
    if acgt or mq:
        assert dropped and 500 <= windows - total < 0.9 * windows      # the rule drops a real share
    else:
        assert total == windows
    singles = total - homopolymer_windows(kept, k)
    assert singles > 2 * fused_lists_hold(text, 32, 16, pieces=len(text) // PIECE + 2)
    assert base_rule.max_record(text) < PIECE < len(text) // 3


@pytest.mark.parametrize("k", FUSED_KS)
def test_input_fasta(k):
    import tsxcount_amd as T
    text, want = fasta_case(T, k, False)
    lines = [l for l in text.split(b"\n") if l and not l.startswith(b">")]
    assert {60, 70} <= {len(l) for l in lines} and max(len(l) for l in lines) == 70
    total = sum(want.values())
    assert total == n_windows(synth_reads(600 + k, 40), k)
    assert total - n_windows(lines, k) > total // 4                              # windows that span a line break
    assert sum(want.values()) - homopolymer_windows(want, k) > 2 * fused_lists_hold(text, 32, 16, pieces=len(text) // PIECE + 2)


@pytest.mark.parametrize("k,acgt,mq,canonical", RULE_WIDE)
def test_input_wide_rules(k, acgt, mq, canonical):
    text, kept, dropped, windows = rule_case(k, acgt, mq, canonical)
    total = sum(kept.values())
    assert dropped and 500 <= windows - total < 0.9 * windows
    assert total - homopolymer_windows(kept, k) > log_keys_needed(text, 64)


@pytest.mark.parametrize("k", [31, 63])
def test_input_hot(k):
    n, suffix, text, fwd = hot_case(k)
    assert n % 500 == 0 and n >= 8 * cap_sub(len(text), HOT_NSEG[k]) + HOT_SPILLS
    if n > 500:   # and it is the smallest such count
        assert n - 500 < 8 * cap_sub(len(hot_text(k, n - 500)[1]), HOT_NSEG[k]) + HOT_SPILLS
    hot = [suffix[i:i + k] for i in range(10)]
    assert len(set(hot)) == 10 and all(fwd[x] == n for x in hot)
    want = fold(fwd)
    assert len({min(x, rc(x)) for x in hot}) == 10 and all(want[min(x, rc(x))] == n for x in hot)


@pytest.mark.parametrize("k", [21, 33])
def test_input_radix512(k):
    text, fwd, tandem = radix512_case(k)
    assert len(set(tandem)) == TANDEM_UNIT and len({min(x, rc(x)) for x in tandem}) == TANDEM_UNIT
    m = sum(fwd[x] for x in tandem)
    assert m >= 60 * (2000 - k + 1)
    assert m > 2 * fused_lists_hold(text, 512, 16, buckets=TANDEM_UNIT)         # k = 21: CAP1 on top
    assert sum(fwd.values()) - homopolymer_windows(fwd, k) > log_keys_needed(text, 64)   # k = 33: LOG_CAP on top


# ---- 1. full log regions, wide keys ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDE_KS)
def test_full_log_regions_wide_keys(T, monkeypatch, k):
    """walk_log_wide_kernel's region-full branch (records of 2 and 4 words through defer_append, deferred_insert_kernel) and
    its hot-key flush, on a one-level and a two-level table, with wide counters and with 2-bit counters that carry."""
    text, want = wide_case(k)
    logged = sum(want.values()) - homopolymer_windows(want, k)
    for cap in (64, 16):
        assert logged > log_keys_needed(text, cap)
        monkeypatch.setenv("TSX_HIP_LOG_CAP", str(cap))
        for l in (18, 22 if k == 127 else 23):
            for s, ol in ((0, 0), (2, 14)):
                m = T.TSXHashMapHIP(l, s, k, overflow_l=ol)
                m.set_path("partitioned")
                for rep in (1, 2):          # the second pass rebuilds every segment from its content
                    m.countFastq(text)
                    st = check_whole_table(T, m, want, k, rep)
                if s == 2:   # every count of 4 and more carried into the secondary array
                    assert st["overflow_used"] >= sum(1 for c in want.values() if c >= 4) > 400 - k
                for b in HOMS:
                    assert m.getKmerCount((b * k).decode()) == 2 * want[b * k]
                m.close()


# ---- 2. full log regions, canonical ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", CANON_KS)
def test_full_log_regions_canonical(T, monkeypatch, k):
    """walk_log_kernel<true> (k <= 32: a one-level table, and a two-level one with the fused walk switched off) and
    walk_log_wide_kernel<WK, true> with regions of 64 keys."""
    text, fwd, pal = canon_case(k)
    want = fold(fwd)
    assert sum(want.values()) - homopolymer_windows(want, k) > log_keys_needed(text, 64)
    monkeypatch.setenv("TSX_HIP_LOG_CAP", "64")
    for l, fuse in ((18, None), (23, "0" if k <= 32 else None)):
        if fuse is not None:
            monkeypatch.setenv("TSX_HIP_FUSE", fuse)
        m = T.TSXHashMapHIP(l, 0, k, canonical=True)
        m.set_path("partitioned")
        for rep in (1, 2):
            m.countFastq(text)
            check_whole_table(T, m, want, k, rep)
            check_both_strands(m, want, k, rep)
        assert m.getKmerCount("A" * k) == m.getKmerCount("T" * k) == 2 * (fwd[b"A" * k] + fwd[b"T" * k])
        assert m.getKmerCount("C" * k) == m.getKmerCount("G" * k) == 2 * (fwd[b"C" * k] + fwd[b"G" * k])
        if pal is not None:
            assert m.getKmerCount(pal.decode()) == 2 * 5
        m.close()
        monkeypatch.delenv("TSX_HIP_FUSE", raising=False)


# ---- 3. full fused sub-lists, modes --------------------------------------------------------------------------------------------

def fused_run(T, monkeypatch, text, want, k, piece, fasta=False, **mode):
    """One table at l = 23 (2^9 segments, 32 level-1 buckets) with level-1 sub-lists of 16 keys."""
    if piece:
        monkeypatch.setenv("TSX_HIP_PIECE_BYTES", str(piece))     # read when the map is created
    m = T.TSXHashMapHIP(23, 0, k, **mode)
    monkeypatch.delenv("TSX_HIP_PIECE_BYTES", raising=False)
    m.set_path("partitioned")
    (m.countFasta if fasta else m.countFastq)(text)
    st = check_whole_table(T, m, want, k)
    singles = sum(want.values()) - homopolymer_windows(want, k)
    pieces = len(text) // piece + 2 if piece else 1
    assert st["fallback_inserts"] >= singles - fused_lists_hold(text, 32, 16, pieces) > singles // 2
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("k", FUSED_KS)
@pytest.mark.parametrize("acgt,mq,canonical", FUSED_MODES)
def test_full_fused_sub_lists_rules_and_canonical(T, monkeypatch, k, acgt, mq, canonical):
    """walk_part_kernel<512, CANON> behind strip_desc_kernel<false, BR> with TSX_HIP_CAP1=16: nearly every key leaves
    through the spill cache, the overflow queue or the deferred list."""
    text, kept, dropped, _ = rule_case(k, acgt, mq, canonical)
    monkeypatch.setenv("TSX_HIP_CAP1", "16")
    for piece in (0, PIECE):
        m = fused_run(T, monkeypatch, text, kept, k, piece, acgt_only=acgt, min_qual_char=mq, canonical=canonical)
        if dropped:
            assert not m.getKmerCounts(encode(sorted(dropped), k)).any()
        if canonical:
            check_both_strands(m, kept, k)
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", FUSED_KS)
@pytest.mark.parametrize("canonical", [False, True])
def test_full_fused_sub_lists_wrapped_fasta(T, monkeypatch, k, canonical):
    text, want = fasta_case(T, k, canonical)
    monkeypatch.setenv("TSX_HIP_CAP1", "16")
    for piece in (0, PIECE):
        m = fused_run(T, monkeypatch, text, want, k, piece, fasta=True, canonical=canonical)
        if canonical:
            check_both_strands(m, want, k)
        m.close()


# ---- 4. full log regions, base rule on wide keys -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k,acgt,mq,canonical", RULE_WIDE)
def test_full_log_regions_base_rule_wide_keys(T, monkeypatch, k, acgt, mq, canonical):
    """strip_desc_wide_kernel<WK, true> in front of a walk whose regions hold 64 keys."""
    text, kept, dropped, _ = rule_case(k, acgt, mq, canonical)
    assert sum(kept.values()) - homopolymer_windows(kept, k) > log_keys_needed(text, 64)
    monkeypatch.setenv("TSX_HIP_LOG_CAP", "64")
    for l in (18, 23):
        m = T.TSXHashMapHIP(l, 0, k, acgt_only=acgt, min_qual_char=mq, canonical=canonical)
        m.set_path("partitioned")
        for rep in (1, 2):
            m.countFastq(text)
            check_whole_table(T, m, kept, k, rep)
        assert not m.getKmerCounts(encode(sorted(dropped), k)).any()
        if canonical:
            check_both_strands(m, kept, k, 2)
        m.close()


# ---- 5. level-2 sub-lists filled by hot keys -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k,canonical", [(63, False), (63, True), (31, True)])
def test_hot_keys_fill_level2_sub_lists(T, k, canonical):
    """partition_ring_kernel's spill cache and overflow queues behind the wide and the canonical walks (hot_case: why this
    many reads)."""
    n, suffix, text, fwd = hot_case(k)
    want = fold(fwd) if canonical else fwd
    m = T.TSXHashMapHIP(23, 0, k, canonical=canonical)
    m.set_path("partitioned")
    m.countFastq(text)
    st = check_whole_table(T, m, want, k)
    assert st["fallback_inserts"] >= 10 * (n - 8 * cap_sub(len(text), HOT_NSEG[k])) >= 10 * HOT_SPILLS
    hot = [suffix[i:i + k] for i in range(10)]
    assert (m.getKmerCounts(encode(hot, k)) == n).all()
    assert (m.getKmerCounts(encode([rc(x) for x in hot], k)) == (n if canonical else 0)).all()
    m.close()


# ---- 6. radix levels of 512 lists ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("k", [21, 33])
def test_radix_levels_of_512_lists_modes(T, monkeypatch, k, forced):
    """2^17 segments of 256 slots at l = 25: canonical one-limb keys through walk_part_kernel<1024, true>, two-limb records
    through partition_ring_kernel at 1024 threads; then with 16-key level-1 lists / 64-key log regions on top."""
    text, fwd, tandem = radix512_case(k)
    canonical = k == 21
    want = fold(fwd) if canonical else fwd
    monkeypatch.setenv("TSX_HIP_SEG_BITS", "8")                   # read when the map is created
    m = T.TSXHashMapHIP(25, 0, k, canonical=canonical)
    monkeypatch.delenv("TSX_HIP_SEG_BITS")
    m.set_path("partitioned")
    if forced:
        monkeypatch.setenv("TSX_HIP_CAP1" if k == 21 else "TSX_HIP_LOG_CAP", "16" if k == 21 else "64")
    for rep in (1, 2):
        m.countFastq(text)
        st = check_whole_table(T, m, want, k, rep)
        if forced and k == 21:
            # the 40 tandem k-mers reach at most 40 of a workgroup's 512 lists
            spare = sum(fwd[x] for x in tandem) - fused_lists_hold(text, 512, 16, buckets=TANDEM_UNIT)
            assert st["fallback_inserts"] >= rep * spare > 0
    if forced and k == 33:
        assert sum(want.values()) - homopolymer_windows(want, k) > log_keys_needed(text, 64)
    if canonical:
        check_both_strands(m, want, k, 2)
    m.close()
