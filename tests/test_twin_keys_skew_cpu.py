"""The designed texts of tests/test_twin_keys_skew.py, checked on the CPU: what they are, that they reach the compares
behind a full list, and that they would tell a wrong compare from a right one.

The GPU file counts families of twin keys through the skew routes of the partitioned path: the spill cache of the SKEW
form of level 2 (spill_record), the "homeless" merge of partition_ring_kernel and the sub-list-full exit of the fused
walk.  Nothing here runs a kernel.  The families are designed in the space of the HASHED keys (twin_design), so the records
of a case are the same whatever mapping turns them into k-mers: here the mapping is twin_design.random_rows, on the GPU
the map's own rows, and the designers assert their conditions themselves in both places.

  * the place function of the spill cache, the chunk size of the deferred list and the radix split are restated in
    Python (twin_design.record_places / radix_split, deferred_chunk below); the lines restated must still stand in the
    sources, so a change of OVF_N or of the mix fails here and does not leave the GPU cases blind;
  * every family has two twins that START at one place of the cache (twin_design.meeting_pairs: stronger than
    overlapping probe windows, which two keys can have without ever meeting);
  * a Python model of the two compare sites (twin_design.model_counts) runs over the records of every case with the
    exact compare -- it then reproduces conftest.python_counts of the text -- and with weakened ones: word 0 only, all
    words but word t, low halves only, high halves only.  Each weakened compare gives another dictionary for the family
    whose field it ignores: the GPU case, which asserts the dictionary, would fail on such a kernel.  The kernels
    themselves are never made wrong, in the tree or anywhere else."""
import functools
import os
from collections import Counter, namedtuple

import pytest

import kmerdb as K
import twin_design as D
from conftest import python_counts
from test_canonical import fold, rc
from test_overflow_paths_modes import HOT_NSEG, HOT_SPILLS, cap_sub, fused_lists_hold

Case = namedtuple("Case", "name k l kind arg canonical env T fams rounds b2b tail steer route cold")


def case(name, k, l, kind, arg, env, T=32, fams=1, rounds=60, b2b=400, tail=20, steer=0, route="level2", canonical=False,
         cold=200):
    return Case(name, k, l, kind, arg, canonical, tuple(sorted(env.items())), T, fams, rounds, b2b, tail, steer, route, cold)


ONE_WG = {"TSX_HIP_CPR2": "1"}          # one level-2 workgroup and one sub-list per segment
# l = 23 throughout: the smallest l of the module whose tables split in two radix levels at every width with default
# segments (HOT_NSEG of test_overflow_paths_modes: 2^9 segments at k = 31, 2^11 at k = 63)
CASES = [
    # one-word records, two radix levels: the fused walk, then level 2
    case("k31-lo-level2", 31, 23, "half", "lo", ONE_WG, rounds=100),
    case("k31-hi-level2", 31, 23, "half", "hi", ONE_WG, rounds=100),
    case("k31-lo-walk", 31, 23, "half", "lo", {"TSX_HIP_CAP1": "16"}, rounds=100, route="walk"),
    case("k31-hi-walk", 31, 23, "half", "hi", {"TSX_HIP_CAP1": "16"}, rounds=100, route="walk"),
    # RW = 2
    case("k63-t1", 63, 23, "h0", 1, ONE_WG),
    # word 1 carries two bits: families of four, four of them in one segment (the skew probe wants eight hot records)
    case("k33-t1", 33, 23, "h0", 1, dict(ONE_WG, TSX_HIP_SEG_BITS="12"), T=4, fams=4, rounds=150, tail=30),
    # RW = 4 with a padded word
    case("k96-t1", 96, 23, "h0", 1, ONE_WG),
    case("k96-t2", 96, 23, "h0", 2, ONE_WG),
    # RW = 4 full
    case("k127-t1", 127, 23, "h0", 1, ONE_WG),
    case("k127-t2", 127, 23, "h0", 2, ONE_WG),
    case("k127-t3", 127, 23, "h0", 3, ONE_WG),
    case("k63-t1-canonical", 63, 23, "h0", 1, ONE_WG, canonical=True),
    # 48 twins that start at 8 places of the cache: at most 11 of them are ever cached, the others fill the overflow
    # queue and then more than one chunk of the deferred list (test_route_sizes)
    case("k63-t1-chunks", 63, 23, "h0", 1, ONE_WG, T=48, rounds=400, tail=10, steer=8),
]
IDS = [c.name for c in CASES]

Design = namedtuple("Design", "case lay members keys fams text seqs want cold_counts family_reads")


def layout_of(c):
    return K.Layout(c.k, c.l, 0, seg_bits=int(dict(c.env)["TSX_HIP_SEG_BITS"]) if "TSX_HIP_SEG_BITS" in dict(c.env) else None)


def cold_texts(c):
    from tsxcount_amd import synth
    half = c.cold // 2
    return synth.fastq(4000 + c.k, 0, half), synth.fastq(4000 + c.k, half, c.cold - half)


def design(c, rows, inv):
    """The families and the text of a case under the mapping `rows` (inv: its inverse).  Several families lie in one
    segment (fix: bits S .. l - 1 of word 0) and are interleaved member by member."""
    lay = layout_of(c)
    seed = 7000 + 10 * c.k + (c.arg if c.kind == "h0" else {"lo": 5, "hi": 6}[c.arg])
    fams, taken = [], set()
    for j in range(c.fams):
        if c.kind == "half":
            kmers, keys = D.half_twins(c.k, inv, c.T, c.arg, lay.l, lay.S, seed + 100 * j, taken)
        else:
            seg_bits = ((1 << lay.l) - 1) & ~((1 << lay.S) - 1)
            fix = (seg_bits, (0x2F1 + c.k) << lay.S) if c.fams > 1 else None
            accept = (lambda key: D.spill_places(key, c.k)[0] < c.steer) if c.steer else None
            kmers, keys = D.hot_h0_families(c.k, inv, c.T, c.arg, seed + 100 * j, taken, accept, fix, rows, c.canonical)
        taken.update(kmers)
        fams.append((kmers, keys))
    members = [f[0][i] for i in range(c.T) for f in fams]
    keys = [f[1][i] for i in range(c.T) for f in fams]
    assert len({D.list_of(key, lay.l, lay.S) for key in keys}) == 1, "the families do not share one list"
    before, after = cold_texts(c)
    strand = (lambda x, r: rc(x) if r & 1 else x) if c.canonical else None
    text, seqs = D.skew_text(members, c.rounds, c.b2b, c.tail, before, after, strand)
    assert all(len(s) == c.k for s in seqs)
    cold_counts = python_counts(before + after, c.k)
    want = dict(python_counts(text, c.k))
    if c.canonical:
        cold_counts, want = Counter(fold(cold_counts)), fold(want)
    names = [min(x, rc(x)) if c.canonical else x for x in members]
    assert not set(names) & set(cold_counts), "a cold read holds a member of the family"
    return Design(c, lay, names, keys, fams, text, seqs, want, cold_counts, len(seqs))


@functools.lru_cache(maxsize=None)
def cpu_mapping(k):
    rows = D.random_rows(k, seed=k)
    return rows, K.inverse_rows(rows, k)


@functools.lru_cache(maxsize=None)
def cpu_design(name):
    c = CASES[IDS.index(name)]
    return design(c, *cpu_mapping(c.k))


def cpr2_of(c):
    return int(dict(c.env).get("TSX_HIP_CPR2", 8))


def lists_hold(d):
    """What the lists the family can reach hold together: the cpr2 sub-lists of its segment (cap_sub), or, on the walk
    route, one level-1 list of TSX_HIP_CAP1 keys per walk workgroup (fused_lists_hold, one bucket)."""
    c = d.case
    if c.route == "walk":
        b1, _ = D.radix_split(d.lay.l, d.lay.S)
        return fused_lists_hold(d.text, 1 << b1, int(dict(c.env)["TSX_HIP_CAP1"]), buckets=1)
    return cpr2_of(c) * cap_sub(len(d.text), 1 << (d.lay.l - d.lay.S), cpr2_of(c))


def spill_bound(d):
    """Occurrences of the family that must leave the fast path, whatever else its segment holds."""
    return d.family_reads - lists_hold(d)


def deferred_chunk(text_bytes, nq2):
    """Records of one private chunk of the deferred list (dch of run_partition_build) for a FASTQ text counted in one
    piece on a fresh map: the list has room for maxrec = bytes / 2 + 65536 records and an eighth and 4096 more
    (ensure_deferred); a quarter of it is shared out over the nq2 level-2 workgroups, a power of two in 64 .. 4096."""
    maxrec = text_bytes // 2 + 65536
    cap = maxrec + maxrec // 8 + 4096
    return next((c for c in (4096, 2048, 1024, 512, 256, 128, 64) if c * nq2 * 4 <= cap), 0)


# ---- the restatements -------------------------------------------------------------------------------------------------

def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tsxcount_amd", "csrc", name)) as f:
        return f.read()


def test_spill_place_restates_the_kernel():
    """twin_design.record_places follows spill_record<RW> of tsx_partition.h (the mix of the words with the golden ratio,
    mix64, >> 40, & (OVF_N - 1), four places probed linearly; a free place is claimed only by d >= 2) and mix64 of
    tsx_device.h; OVF_N and the walk's one-place cache likewise.  When this fails, bring twin_design in line with the
    kernel first, then the lines here."""
    part = _source("tsx_partition.h")
    body = part[part.index("void spill_record("):]
    body = body[:body.index("__global__")]
    for line in ("uint64_t mixin = r.w[0];",
                 "for (int t = 1; t < RW; ++t) mixin ^= r.w[t] * 0x9E3779B97F4A7C15ULL;",
                 "uint32_t slot = (uint32_t)(mix64(mixin) >> 40) & (OVF_N - 1);",
                 "for (int pr = 0; pr < 4; ++pr, slot = (slot + 1) & (OVF_N - 1)) {",
                 "if (d < 2u) break;   // not cached, and not to be",
                 "for (int t = 1; t < RW; ++t) same &= (sp->ovk[slot * RW + t] == r.w[t]);"):
        assert line in body, line
    assert "constexpr uint32_t OVF_N = %d;" % D.OVF_N in part and D.OVF_PROBES == 4
    walk = part[part.index("void walk_part_kernel("):]
    assert "const uint32_t slot = (uint32_t)(mix64(key) >> 40) & (OVF_N - 1);" in walk[:walk.index("inline bool walk_local_form")]
    dev = _source("tsx_device.h")
    for line in ("z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;", "z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;",
                 "return z ^ (z >> 31);"):
        assert line in dev, line
    assert D.mix64(D.PHI) == 0xE220A8397B1DCDAF          # splitmix64's first output for seed 0
    # one-word records: the place is mix64 of the word alone; padded words are zero and add nothing to the mix
    assert D.record_places((5,)) == D.record_places((5, 0)) == D.record_places((5, 0, 0, 0))
    assert D.record(1 << 64 | 7, 96) == (7, 1, 0, 0) and D.rec_words(31) == 1 and D.rec_words(33) == 2 and D.rec_words(65) == 4


def test_geometry_restates_the_host():
    """radix_split, list_of and deferred_chunk follow radix_bits, run_partition_build and ensure_deferred of
    tsxcount_hip.hip; the merge of partition_ring_kernel looks at runs of 64 lanes, twice."""
    host = _source("tsxcount_hip.hip")
    for line in ("const int b1 = std::min(9, (nsegbits <= 8) ? nsegbits : (nsegbits + 1) / 2);",
                 "r.nb = pl.nb1; r.shift = (uint32_t)(p.l - pl.b1); r.capbits = ring_bits(pl.nb1);",
                 "r.nb = pl.nb2; r.shift = (uint32_t)p.S; r.capbits = ring_bits(pl.nb2);",
                 "for (uint32_t c = 4096; c >= 64 && !dch; c >>= 1)",
                 "if ((uint64_t)c * nq2 * 4 <= m->def_cap()) dch = c;",
                 "const size_t cap = maxrec + maxrec / 8 + 4096;",
                 "static const uint32_t OVQ_CAP = %d;" % D.OVQ_CAP):
        assert line in host, line
    part = _source("tsx_partition.h")
    for line in ("bq[q] = (uint32_t)(cur[q][0] >> shift) & (nb - 1);",
                 "for (int rnd = 0; rnd < 2 && todo != 0ULL; ++rnd) {",
                 "if (ovq && d == 1u) {"):
        assert line in part, line
    assert D.radix_split(23, 14) == (5, 4) and D.radix_split(23, 12) == (6, 5) and D.radix_split(18, 12) == (6, 0)
    assert HOT_NSEG == {31: 1 << (23 - layout_of(CASES[0]).S), 63: 1 << (23 - layout_of(CASES[4]).S)}
    assert deferred_chunk(1 << 20, 64) == 2048 and deferred_chunk(1 << 20, 512) == 256


# ---- the families --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IDS)
def test_design_facts(name):
    d = cpu_design(name)
    c, lay = d.case, d.lay
    rows, _ = cpu_mapping(c.k)
    assert K.table_keys(d.members, rows, c.k, canonical=c.canonical) == d.keys       # kmerdb alone: these k-mers, these records
    assert len(set(d.members)) == c.T * c.fams and not any(len(set(x)) == 1 for x in d.members)
    strands = set(d.members) | {rc(x) for x in d.members}
    assert len(strands) == 2 * len(d.members)                   # no member is another's (or its own) reverse complement
    if c.canonical:
        assert all(x < rc(x) for x in d.members) and {s for s in d.seqs} >= strands    # both strands are in the text
    b1, b2 = D.radix_split(lay.l, lay.S)
    assert b2 > 0, "two radix levels"
    assert len({D.list_of(key, lay.l, lay.S) for key in d.keys}) == 1
    rw = D.rec_words(c.k)
    for kmers, keys in d.fams:
        words = [D.record(key, c.k) for key in keys]
        if c.kind == "h0":
            for u in range(rw):
                assert len({w[u] for w in words}) == (c.T if u == c.arg else 1), (u, c.arg)
        else:
            keep = D.M32 << 32 if c.arg == "lo" else D.M32
            assert rw == 1 and len({key & keep for key in keys}) == 1 and len(set(keys)) == c.T
        # two twins that start at one place of the cache: the compare between different keys is certain to run
        assert D.meeting_pairs(keys, c.k) and set(D.meeting_pairs(keys, c.k)) <= set(D.overlapping_pairs(keys, c.k))
    if c.steer:
        assert len({p for key in d.keys for p in D.spill_places(key, c.k)}) <= c.steer + D.OVF_PROBES - 1
    # a member comes back within a wave's 64 records, so combined records form in the interleaved part already
    assert 2 * c.T * c.fams <= 64 or c.steer
    assert d.want == dict(d.cold_counts + Counter(min(s, rc(s)) if c.canonical else s for s in d.seqs))


@pytest.mark.parametrize("name", IDS)
def test_route_sizes(name):
    """The family's occurrences beyond what its lists hold: at least HOT_SPILLS, and before the back-to-back block the
    interleaved part alone has filled the lists.  The chunk case: the records of uncached members, two to an entry at
    most, less a full overflow queue, are more than the largest chunk there is -- with twins on both sides of the
    boundary, since every one of these records is a twin."""
    d = cpu_design(name)
    c = d.case
    assert spill_bound(d) >= HOT_SPILLS, (d.family_reads, lists_hold(d))
    assert c.rounds * c.T * c.fams >= lists_hold(d) + 64 * 4, "the lists must be full before the back-to-back block"
    if c.steer:
        b1, _ = D.radix_split(d.lay.l, d.lay.S)
        dch = deferred_chunk(len(d.text), (1 << b1) * cpr2_of(c))
        cached = c.steer + D.OVF_PROBES - 1
        per_entry = -(-64 // c.T)          # occurrences of one member among 64 interleaved records
        chunked = ((c.T - cached) * c.rounds - lists_hold(d)) // per_entry - D.OVQ_CAP
        assert 64 <= dch <= 4096 < chunked, (dch, chunked)


# ---- the model ------------------------------------------------------------------------------------------------------------

def model_dictionary(d, same):
    """{k-mer: count} of the text when the family's records go through the model with the compare `same`."""
    rec_of = {x: D.record(key, d.case.k) for x, key in zip(d.members, d.keys)}
    name_of = {r: x for x, r in rec_of.items()}
    recs = [rec_of[min(s, rc(s)) if d.case.canonical else s] for s in d.seqs]
    got = D.model_counts(recs, lists_hold(d) if d.case.route == "level2" else 0, same)
    out = Counter(d.cold_counts)
    for r, n in got.items():
        out[name_of[r]] += n
    return dict(out)


@pytest.mark.parametrize("name", IDS)
def test_model_tells_compares_apart(name):
    d = cpu_design(name)
    c = d.case
    assert model_dictionary(d, D.COMPARES["exact"]) == d.want
    if c.kind == "h0":
        weak = {"word 0 only": D.COMPARES["word 0 only"], "all words but %d" % c.arg: D.all_words_but(c.arg)}
    else:
        weak = {"low halves only": D.COMPARES["low halves only"]} if c.arg == "hi" else \
               {"high halves only": D.COMPARES["high halves only"]}
    for label, same in weak.items():
        got = model_dictionary(d, same)
        assert got != d.want, label
        assert sum(got.values()) == sum(d.want.values())       # the occurrences went to a sibling; none is lost
    # and the compares that ignore nothing of this family leave it alone
    if c.kind == "half":
        kept = "low halves only" if c.arg == "lo" else "high halves only"
        assert model_dictionary(d, D.COMPARES[kept]) == d.want


# ---- the homopolymer case ----------------------------------------------------------------------------------------------------

HOM_ROUNDS = 80
HOM_TAIL = 15        # a homopolymer read of k + 15 bases: 16 windows, one strip


@functools.lru_cache(maxsize=None)
def hom_design_cpu():
    return hom_design(*cpu_mapping(31))


def hom_design(rows, inv):
    """k = 31: reads of one base alone (A, C, G, T in turn, 16 windows each) alternate with the reads of a half_twins
    family, one k-mer each; a wave walks about a KiB of text, six such pairs, so all four homopolymers are hot inside
    the strips of one wave.  (text, forward counts, members, family reads)"""
    k, l = 31, 23
    lay = K.Layout(k, l, 0)
    members, keys = D.half_twins(k, inv, 32, "lo", l, lay.S, seed=3100)
    from tsxcount_amd import synth
    seqs = []
    for r in range(HOM_ROUNDS):
        for j, x in enumerate(members):
            seqs.append(b"ACGT"[(r * len(members) + j) % 4:][:1] * (k + HOM_TAIL))
            seqs.append(x)
    fam = b"".join(b"@h%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    text = synth.fastq(4100, 0, 50) + fam + synth.fastq(4100, 50, 50)
    return text, dict(python_counts(text, k)), members, HOM_ROUNDS * len(members)


def test_homopolymer_text():
    text, fwd, members, n = hom_design_cpu()
    k = 31
    per_base = HOM_ROUNDS * 32 // 4 * (HOM_TAIL + 1)
    assert fwd[b"C" * k] == fwd[b"G" * k] == fwd[b"T" * k] == per_base and fwd[b"A" * k] > per_base
    assert all(fwd[x] == HOM_ROUNDS for x in members)
    want = fold(fwd)
    assert want[b"A" * k] == fwd[b"A" * k] + per_base and want[b"C" * k] == 2 * per_base
    assert n - fused_lists_hold(text, 32, 16, buckets=1) >= HOT_SPILLS
    # six reads of a pair's 190 bytes in a KiB: every run of four pairs shows all four bases
    assert 4 * (2 * (k + HOM_TAIL) + 2 * k + 30) < 1024
