"""Keys that differ in a single limb or field, on every compare path of the table (the designers: tests/twin_design.py).

Random reads never bring two different keys with equal limb 0 into one compare, so a compare that stops a limb early, uses
the wrong spill word, masks too much or lets only the top limb order two keys leaves every other test green.  Here the
texts are designed through the inverse of the map's hash (its rows from hash_rows(), inverted in kmerdb): families of
twins on one home slot that agree everywhere but in one field of the slot, in one limb of the hashed key, in one limb of
the k-mer, or whose two strand keys tie in the top limb.  Every expectation is exact and comes from
conftest.python_counts of the text (or the dictionary a case builds itself); nothing is compared within a tolerance.

  (a) insert paths      atomic (count_fastq_kernel -> insert_key) and partitioned (the build kernels), twice without
                        clear(); whole dump, counters, and the slots of a family = the probe chain of its home slot
  (b) absent siblings   lookup_key and the probe of tsx_query.h must not find a twin's sibling, nor its carry
  (c) addKmers          counts that straddle 2^C; dump = saved database = kmerdb.read_db of the file
  (d) deferred list     h[0]-equal families through deferred_insert_kernel's LDS table
  (e) text-space twins  kmer_eq of the atomic scan kernel and of the sketch kernel
  (f) strand ties       key_less / key_min / lex_canonical of canonical tables

The compares behind a full list -- the spill cache of the skewed level-2 form, the "homeless" merge of
partition_ring_kernel, the sub-list-full exit of the fused walk -- need a skewed bucket: tests/test_twin_keys_skew.py
counts families through them, tests/test_twin_keys_skew_cpu.py shows on a model that those texts tell a wrong compare
from a right one.  Not reached (see twin_design): the walk's per-wave hot-key cache holds homopolymer keys only, so no
twin can be designed into it (a totals case there); the multi-GPU exchanges and tables above 2^32 slots are out of scope."""
import functools
import os
import random

import numpy as np
import pytest

import kmerdb as K
import twin_design as D
from conftest import python_counts
from test_build_handout import check, dump_sorted, seg_bits_of
from test_canonical import encode, fastq_of, fold, rc
from test_overflow_paths_modes import log_keys_needed

# k, l, s -> the build kernel run_partition_build picks (tsxcount_hip.hip: one-limb keys in one-word slots take
# build_segments_stream_kernel, <false> on a one-level split; everything else build_segments_wide_stream_kernel<WK>)
LAYOUTS = {
    (31, 16, 0): "build_segments_stream_kernel<false>",
    (31, 20, 16): "build_segments_wide_stream_kernel<1>",
    (33, 20, 0): "build_segments_wide_stream_kernel<2>",
    (63, 18, 0): "build_segments_wide_stream_kernel<2>",
    (63, 20, 32): "build_segments_wide_stream_kernel<2>",
    (65, 20, 0): "build_segments_wide_stream_kernel<3>",
    (96, 18, 2): "build_segments_wide_stream_kernel<3>",
    (97, 20, 0): "build_segments_wide_stream_kernel<4>",
    (127, 18, 2): "build_segments_wide_stream_kernel<4>",
}
KLS = list(LAYOUTS)
IDS = ["k%d-l%d-s%d" % r for r in KLS]
TWINS = 48            # below max_reprobes (255), and tri(48) < 2^12: the chain of a family never wraps onto itself
ABSENT = (1 << 64) - 1


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


_inv = {}


def geometry(T, m, s, tmp_path):
    """(Layout with the map's segment bits, rows, inverse rows), the layout checked against the library's"""
    rows = m.hash_rows()
    key = (m.k, rows.tobytes())
    if key not in _inv:
        _inv[key] = K.inverse_rows(rows, m.k)
    lay = K.Layout(m.k, m.l, s, seg_bits=seg_bits_of(T, m, tmp_path))
    f = lay.fields()
    assert all(int(getattr(m.layout, n)) == v for n, v in f.items()), (f, lay)
    return lay, rows, _inv[key]


def families_for(lay, inv, seed):
    """One family per field of the layout, at least three (fields again on other homes), each in a segment of its own:
    [(field, home, k-mers)] and a few hundred unrelated k-mers whose first probe is a slot of no family's chain and of no
    other unrelated k-mer."""
    fields = D.fields_of(lay)
    fields = (fields * 3)[:max(3, len(fields))]
    nseg = 1 << (lay.l - lay.S)
    assert nseg >= len(fields), (lay, fields)
    fams, taken, chain = [], set(), set()
    for j, f in enumerate(fields):
        home = (((j * 7 + 1) % nseg) << lay.S) | ((0x2F1 * (j + 3) + seed) & ((1 << lay.S) - 1))
        n = min(TWINS, 1 << D.field_bits(lay, f)[1])
        kmers, _ = D.key_twins(lay, inv, home, n, f, seed=seed * 10 + j, taken=taken)
        taken.update(kmers)
        assert not chain & {lay.probe(home, i) for i in range(1, n + 1)}
        chain |= {lay.probe(home, i) for i in range(1, TWINS + 1)}
        fams.append((f, home, kmers))
    rng = random.Random(seed)
    others, first = [], set(chain)
    while len(others) < 300:
        keys = [rng.getrandbits(2 * lay.k) for _ in range(400)]
        for key, x in zip(keys, K.keys_to_kmers(keys, inv, lay.k)):
            p1 = lay.probe(lay.home(key), 1)
            if p1 in first or x in taken or len(set(x)) == 1 or len(others) == 300:
                continue
            first.add(p1)
            taken.add(x)
            others.append(x)
    return fams, others


def twin_text(fams, others, seed):
    """one k-mer per read, twin j 1 + (j % 5) times, the unrelated k-mers once, in a seeded random order"""
    seqs = [x for _, _, kmers in fams for j, x in enumerate(kmers) for _ in range(1 + j % 5)] + list(others)
    order = np.random.default_rng(seed).permutation(len(seqs))
    return fastq_of([seqs[i] for i in order])


def check_chains(m, lay, fams, k):
    for f, home, kmers in fams:
        cnt, pos = m.getKmerCountDebug(encode(kmers, k))
        assert set(pos.tolist()) == {lay.probe(home, i) for i in range(1, len(kmers) + 1)}, (f, home)


# ---- (a) insert paths -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kls", KLS, ids=IDS)
def test_insert_paths(T, tmp_path, kls):
    """Build kernel of the partitioned run, by layout (LAYOUTS above, read off run_partition_build's dispatch):
    (31, 16, 0) build_segments_stream_kernel<false>, whose compare is the two 32-bit halves -- the limb0_lo and limb0_hi
    families; (31, 20, 16) build_segments_wide_stream_kernel<1>; (33, 20, 0), (63, 18, 0), (63, 20, 32) <2>; (65, 20, 0),
    (96, 18, 2) <3>; (97, 20, 0), (127, 18, 2) <4>.  The atomic run is count_fastq_kernel -> insert_key for all."""
    k, l, s = kls
    dumps = []
    for path in ("atomic", "partitioned"):
        m = T.TSXHashMapHIP(l, s, k)
        m.set_path(path)
        lay, rows, inv = geometry(T, m, s, tmp_path)
        fams, others = families_for(lay, inv, seed=k + l)
        text = twin_text(fams, others, seed=k)
        want = dict(python_counts(text, k))
        assert len(want) == sum(len(f[2]) for f in fams) + len(others)
        for rep in (1, 2):                  # the second run over dirty segments
            m.countFastq(text)
            dump = check(T, m, want, k, rep)
            check_chains(m, lay, fams, k)
            if path == "partitioned":
                assert m.stats()["fallback_inserts"] == 0
        dumps.append(dump)
        m.close()
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])


# ---- (b) absent siblings ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kls", KLS, ids=IDS)
def test_absent_siblings(T, tmp_path, kls):
    """Only the even twins are in the table -- 9 times each where s = 2, so that their counts carry into the secondary
    array.  The odd ones are absent for getKmerCounts / getKmerCountDebug (lookup_key) and for queryReads and
    countProfile (the probe of tsx_query.h)."""
    k, l, s = kls
    m = T.TSXHashMapHIP(l, s, k)
    lay, rows, inv = geometry(T, m, s, tmp_path)
    fams, others = families_for(lay, inv, seed=k + l + 1)
    times = 9 if s == 2 else 1
    even = [x for _, _, kmers in fams for x in kmers[0::2]]
    odd = [x for _, _, kmers in fams for x in kmers[1::2]]
    text = fastq_of((even + others[:50]) * times)
    want = dict(python_counts(text, k))
    m.countFastq(text)
    check(T, m, want, k)
    if s == 2:
        assert m.stats()["overflow_used"] >= len(even)
    cnt, pos = m.getKmerCountDebug(encode(odd, k))
    assert not cnt.any() and (pos == np.uint64(ABSENT)).all()
    assert not m.getKmerCounts(encode(odd, k)).any()
    cnt, pos = m.getKmerCountDebug(encode(even, k))
    assert (cnt == times).all() and (pos != np.uint64(ABSENT)).all()
    reads = fastq_of(odd)
    st = m.queryReads(reads)
    assert len(st) == len(odd) and (st["kmers"] == 1).all()
    assert not st["in_range"].any() and not st["min_count"].any() and not st["sum_count"].any()
    prof = m.countProfile(reads)
    starts = prof != T.NO_KMER
    assert starts.sum() == len(odd) and not prof[starts].any()
    st = m.queryReads(fastq_of(even))                   # and the even ones are found there
    assert (st["in_range"] == 1).all() and (st["min_count"] == times).all()
    m.close()


# ---- (c) addKmers with counts ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kls", [(96, 18, 2), (127, 18, 2), (65, 20, 0)], ids=["k96-l18-s2", "k127-l18-s2", "k65-l20-s0"])
def test_add_kmers_with_counts(T, tmp_path, kls):
    """Twins added with counts 2^C - 1, 2^C, 2^C + 1, 1, 2^(C + 1) + 1, ...: the dump, the saved database loaded back and
    kmerdb.read_db of the file hold the same dictionary."""
    k, l, s = kls
    m = T.TSXHashMapHIP(l, s, k)
    lay, rows, inv = geometry(T, m, s, tmp_path)
    fams, others = families_for(lay, inv, seed=k + l + 2)
    kmers = [x for _, _, f in fams for x in f] + others[:40]
    top = 1 << lay.C
    cyc = [top - 1, top, top + 1, 1, 2 * top + 1]
    want = {x: cyc[j % 5] for j, x in enumerate(kmers)}
    m.addKmers(encode(kmers, k), np.array([want[x] for x in kmers], dtype=np.uint64))
    st = m.stats()
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["distinct"] == len(want)
    assert st["count_sum"] == sum(want.values())

    def as_dict(mm):
        kk, cc = mm.getAllKmers()
        return {T.decode(r, k).encode(): int(c) for r, c in zip(kk, cc)}

    assert as_dict(m) == want
    check_chains(m, lay, fams, k)
    path = os.path.join(str(tmp_path), "twins.tsxdb")
    m.saveDatabase(path)
    m2 = T.TSXHashMapHIP.fromDatabase(path)
    assert as_dict(m2) == want
    assert np.array_equal(m2.getKmerCounts(encode(kmers, k)), np.array([want[x] for x in kmers], dtype=np.uint64))
    db = K.read_db(path, rows)
    assert db.kmers == want
    assert len(db.carries) == sum(1 for c in want.values() if c >= top)
    m2.close()
    m.close()


# ---- (d) the deferred list ----------------------------------------------------------------------------------------------------------

PHI = 0x9E3779B97F4A7C15


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & K.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & K.M64
    return z ^ (z >> 31)


def deferred_place(key, wk):
    """Where deferred_insert_kernel starts to look for a key in its LDS table (tsx_partition.h): the table has 1024 places
    for records of two words and 512 for four, the place is mix64(h[0] ^ h[1] * PHI ^ ...) >> 40.  Restated here only to
    choose twins that meet there; the expectations do not depend on it."""
    dn = 1024 if wk == 2 else 512
    mixin = key & K.M64
    for t in range(1, wk):
        mixin ^= (((key >> (64 * t)) & K.M64) * PHI) & K.M64
    return (mix64(mixin) >> 40) & (dn - 1)


def test_deferred_place_restates_the_kernel():
    """deferred_place steers the twins of test_deferred_list into one corner of deferred_insert_kernel's LDS table; if the
    kernel's table size or place function changes, the twins stop meeting there and that test would stay green for the
    wrong reason.  So the lines restated above must still stand in the kernel: when this fails, bring deferred_place (and
    DEFER_PLACES) in line with the kernel, then update the lines here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tsxcount_amd", "csrc", "tsx_partition.h")) as f:
        src = f.read()
    body = src[src.index("void deferred_insert_kernel("):]
    body = body[:body.index("__global__")]
    for line in ("constexpr uint32_t DN = (RW == 1) ? 2048u : (RW == 2) ? 1024u : 512u;",
                 "uint64_t mixin = h[0];",
                 "for (int t = 1; t < WK; ++t) mixin ^= h[t] * 0x9E3779B97F4A7C15ULL;",
                 "uint32_t slot = (uint32_t)(mix64(mixin) >> 40) & (DN - 1);",
                 "slot = (slot + 1) & (DN - 1);"):
        assert line in body, line
    assert mix64(PHI) == 0xE220A8397B1DCDAF          # splitmix64's first output for seed 0: mix64 is that finaliser


DEFER_LEAD = 16        # windows of a read in front of its twin: as many as a log region holds
# by key limbs: the twins start at the first 8 of the table's 1024 / 512 places.  Several places, not one: a share of a
# few dozen records is one wave's work, its lanes claim their places in the same instruction, and a sibling finds a
# published entry only when it lost its own place and steps onto the next.  (With one place the seeded defect "compare
# only t = 1" merged nothing in a run; with eight it merged three entries at k = 127.)
DEFER_PLACES = {2: 8, 4: 8}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 127])
def test_deferred_list(T, tmp_path, monkeypatch, k):
    """Three h[0]-equal families of 200 twins (600 twins, counts 1 .. 3), each family varying one limb h[t], t >= 1 -- at
    k = 127 one family per t = 1, 2, 3.  With log regions of 16 keys (TSX_HIP_LOG_CAP, as test_full_log_regions_wide_keys
    sets it) walk_log_wide_kernel hands what a full region cannot take to the deferred list.  A text of one k-mer per read
    would not fill a region (a wave walks about a KiB of text: eight reads), so every read carries DEFER_LEAD random bases
    in front of its twin: the DEFER_LEAD windows before the twin fill the region of the wave that walks the read.  That
    keys took the route is shown as in that test, by arithmetic: the logged keys are more than twice what all regions
    hold.  deferred_insert_kernel sums equal keys of a workgroup's share in an LDS table that claims word 0 and compares
    the others; the twins are chosen to start at the first eight places of that table (deferred_place, DEFER_PLACES), so that
    siblings of one share meet there now and then: a few times per run, by a measurement with a seeded defect."""
    l = 18
    monkeypatch.setenv("TSX_HIP_LOG_CAP", "16")
    m = T.TSXHashMapHIP(l, 0, k)
    m.set_path("partitioned")
    lay, rows, inv = geometry(T, m, 0, tmp_path)
    wk = lay.key_limbs
    fams, taken = [], set()
    for j in range(3):
        kmers, keys = D.h0_twins(k, inv, 200, 1 + j % (wk - 1), seed=900 + 10 * k + j, taken=taken,
                                 accept=lambda key: deferred_place(key, wk) < DEFER_PLACES[wk])
        assert len({key & K.M64 for key in keys}) == 1
        taken.update(kmers)
        fams.append(kmers)
    rng = np.random.default_rng(k)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = [lut[rng.integers(0, 4, DEFER_LEAD)].tobytes() + x for f in fams for j, x in enumerate(f) for _ in range(1 + j % 3)]
    text = fastq_of([seqs[i] for i in rng.permutation(len(seqs))])
    want = dict(python_counts(text, k))
    assert all(want[x] == 1 + j % 3 for f in fams for j, x in enumerate(f))
    assert not any(len(set(x)) == 1 for x in want)                      # no homopolymer: every window goes to the log
    assert sum(want.values()) > log_keys_needed(text, 16)
    for rep in (1, 2):
        m.countFastq(text)
        dump = check(T, m, want, k, rep)
    for f in fams:     # one home slot per family: 200 slots of its probe chain, whatever else the segment holds
        cnt, pos = m.getKmerCountDebug(encode(f, k))
        home = lay.home(K.table_keys(f[:1], rows, k)[0])
        assert set(pos.tolist()) <= {lay.probe(home, i) for i in range(1, lay.max_reprobes + 1)} and len(set(pos.tolist())) == 200
    m.close()
    a = T.TSXHashMapHIP(l, 0, k)
    a.set_path("atomic")
    a.countFastq(text)
    a.countFastq(text)
    ak, ac = dump_sorted(a)
    a.close()
    assert np.array_equal(ak, dump[0]) and np.array_equal(ac, dump[1])


# ---- (e) text-space twins on the atomic scan kernel ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def text_families(k):
    wk = (2 * k + 63) // 64
    fams, taken = [], set()
    for t in range(wk):
        f = D.text_twins(k, 1500, t, seed=70 * k + t, taken=taken)
        taken.update(f)
        fams.append(f)
    return fams


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "neighbours"])
@pytest.mark.parametrize("k", [63, 96, 127])
def test_text_twins_atomic_scan(T, k, order):
    """One family of 1500 twins per limb t < WK of the k-mer, one read per occurrence, shuffled or ("neighbours") family
    by family with twin j 1 + (j % 5) times in a row.  What this reaches is limited: with one k-mer per read the position
    before a k-mer is never one, so the run-length leader test compares nothing; and a dedup round of 2048 text positions
    holds 8 to 15 such k-mers, so two unequal ones share one of the 4096 dedup places only a few dozen times in a run.
    The case checks the counts and the sketch of these texts; the k-mer compares themselves are the subject of
    test_adjacent_text_twins below."""
    fams = text_families(k)
    seqs = [x for f in fams for j, x in enumerate(f) for _ in range(1 + j % 5)]
    if order == "shuffled":
        seqs = [seqs[i] for i in np.random.default_rng(k).permutation(len(seqs))]
    text = fastq_of(seqs)
    want = dict(python_counts(text, k))
    assert len(want) == 1500 * len(fams)
    m = T.TSXHashMapHIP(20, 0, k)
    m.set_path("atomic")
    for rep in (1, 2):
        m.countFastq(text)
        check(T, m, want, k, rep)
    regs, tot = m.sketchKmers(text)
    assert tot["kmers"] == len(seqs) and tot["records"] == len(seqs)
    assert np.array_equal(regs, T.sketch_registers(encode(sorted(want), k), k))
    m.close()


SLIDE = 16            # a read of k + SLIDE bases: SLIDE + 1 windows, twins of each other, at adjacent text positions
SLIDE_READS = 90      # per limb: 90 * 17 = 1530 twins


@functools.lru_cache(maxsize=None)
def sliding_reads(k):
    """[reads of limb 0, reads of limb 1, ...]: within a limb's list every window of every read is a twin of every other"""
    return [D.sliding_twins(k, t, SLIDE, SLIDE_READS, seed=31 * k + t, lo="ACGT"[t], hi="CGTA"[t])
            for t in range((2 * k + 63) // 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [63, 96, 127])
def test_adjacent_text_twins(T, k):
    """Twins in limb t of the k-mer at adjacent text positions, for every t < WK (twin_design.sliding_twins): the lanes of
    a wave hold consecutive positions, and the leader test of count_fastq_kernel, of the sketch kernel, of the read
    query and of the count profile compares a window with the one in the lane below -- here the two differ in limb t
    alone.  The reads of a limb follow each other, so a dedup round of count_fastq_kernel (2048 positions: a hundred
    windows and more) holds twins of one limb only, and unequal k-mers that share a dedup place are such twins too.
    Counting: read r occurs 1 + (r % 3) times, the dump is the dictionary.  Queries: a second table holds window j with
    count 1 + (j % 5) through addKmers, so neighbouring windows have different counts and a window that took its
    neighbour's count shows in the record's in_range, min and sum and in the profile."""
    fams = sliding_reads(k)
    once = [r for f in fams for r in f]
    seqs = [r for j, r in enumerate(once) for _ in range(1 + j % 3)]
    text = fastq_of(seqs)
    want = dict(python_counts(text, k))
    assert len(want) == (SLIDE + 1) * len(once) and not any(len(set(x)) == 1 for x in want)
    m = T.TSXHashMapHIP(20, 0, k)
    m.set_path("atomic")
    for rep in (1, 2):
        m.countFastq(text)
        check(T, m, want, k, rep)
    regs, tot = m.sketchKmers(text)
    assert tot["kmers"] == (SLIDE + 1) * len(seqs) and tot["records"] == len(seqs)
    assert np.array_equal(regs, T.sketch_registers(encode(sorted(want), k), k))
    m.close()
    # the query side
    wins = [r[i:i + k] for r in once for i in range(SLIDE + 1)]
    cnt = {x: 1 + j % 5 for j, x in enumerate(wins)}
    q = T.TSXHashMapHIP(20, 0, k)
    q.addKmers(encode(wins, k), np.array([cnt[x] for x in wins], dtype=np.uint64))
    assert q.stats()["distinct"] == len(wins)
    qtext = fastq_of(once)
    st = q.queryReads(qtext, lower=2, upper=4)
    per = [[cnt[r[i:i + k]] for i in range(SLIDE + 1)] for r in once]
    assert len(st) == len(once) and (st["kmers"] == SLIDE + 1).all()
    assert st["in_range"].tolist() == [sum(1 for c in p if 2 <= c <= 4) for p in per]
    assert st["min_count"].tolist() == [min(p) for p in per] and st["sum_count"].tolist() == [sum(p) for p in per]
    prof = q.countProfile(qtext)
    assert prof[prof != T.NO_KMER].tolist() == [c for p in per for c in p]
    q.close()


# ---- (f) strand ties ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [47, 80, 127])
def test_strand_ties(T, tmp_path, k):
    """k-mers whose strand keys h(x), h(rc x) agree in the whole top limb and differ in limb WK - 2 (WK = 2, 3, 4):
    canonical tables through both insert paths, x in some reads and rc(x) in others.  The pair is one entry with the sum,
    either strand looks it up, the dump names the lexicographically smaller strand."""
    l = 18
    dumps = []
    for path in ("atomic", "partitioned"):
        m = T.TSXHashMapHIP(l, 0, k, canonical=True)
        m.set_path(path)
        lay, rows, inv = geometry(T, m, 0, tmp_path)
        ties, pairs = D.strand_ties(rows, k, 200, seed=k)
        top = 64 * (lay.key_limbs - 1)
        assert all(h >> top == hr >> top and h != hr for h, hr in pairs)
        assert {h < hr for h, hr in pairs} == {True, False}
        rng = np.random.default_rng(k)
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        others = [lut[rng.integers(0, 4, k)].tobytes() for _ in range(200)]
        seqs = [y for j, x in enumerate(ties) for y in [x] * (1 + j % 3) + [rc(x)] * (1 + j % 4)] + others
        text = fastq_of([seqs[i] for i in rng.permutation(len(seqs))])
        fwd = dict(python_counts(text, k))
        want = fold(fwd)
        assert len(want) == len(ties) + len(others) and len(fwd) == 2 * len(ties) + len(others)
        for j, x in enumerate(ties):
            assert want[min(x, rc(x))] == 2 + j % 3 + j % 4
        for rep in (1, 2):
            m.countFastq(text)
            dump = check(T, m, want, k, rep)          # (the dump's k-mers are the dictionary's keys: the smaller strands)
            if path == "partitioned":
                assert m.stats()["fallback_inserts"] == 0
        exp = np.array([2 * want[min(x, rc(x))] for x in ties], dtype=np.uint64)
        assert np.array_equal(m.getKmerCounts(encode(ties, k)), exp)
        assert np.array_equal(m.getKmerCounts(encode([rc(x) for x in ties], k)), exp)
        c1, p1 = m.getKmerCountDebug(encode(ties, k))
        c2, p2 = m.getKmerCountDebug(encode([rc(x) for x in ties], k))
        assert np.array_equal(p1, p2) and len(set(p1.tolist())) == len(ties)
        # the entry sits in the segment of the smaller strand key
        homes = np.array([lay.home(min(h, hr)) >> lay.S for h, hr in pairs], dtype=np.uint64)
        assert np.array_equal(p1 >> np.uint64(lay.S), homes)
        dumps.append(dump)
        m.close()
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])
