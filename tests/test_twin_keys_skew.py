"""Twin keys on the skew routes of the partitioned path: the spill cache of the SKEW form of level 2 (spill_record), the
"homeless" merge of partition_ring_kernel and the sub-list-full exit of the fused walk.  The cases, their designers and
the CPU proof that these texts tell a wrong compare from a right one: tests/test_twin_keys_skew_cpu.py, tests/twin_design.py.

Every case counts a designed text on the partitioned path and compares the WHOLE table with conftest.python_counts of
the text (check_whole_table of test_overflow_paths_modes: the dump key for key and count for count, the totals of
stats(), no failures, getKmerCounts of every k-mer), then counts the text again without clear(): every count doubles.

Why the order of the text makes both sites see twins.  Every family read is one k-mer, so the records reach the kernels
in the order of the text.  All members of a case share the bits of word 0 that pick the list at both levels: one level-1
bucket, one segment, with TSX_HIP_CPR2=1 one sub-list.  First the members come interleaved, A, B, C, ..., A, B, C, ...,
more often than the list holds records (test_route_sizes): the list runs full, the workgroup sets its `skew` flag and
from the next batch on the HOT form of `append` finds these records homeless.  A wave's 64 lanes hold 64 consecutive
records of the bucket: neighbouring lanes hold different twins, which the merge compares word for word with the first
homeless lane's record, and, with at most 32 members, a member twice or more -- a combined record of d >= 2, which the
cache admits.  Then one member comes back to back (whole waves of equal records: d >= 2 for certain), then the members
interleaved again: twins that probe the cache AFTER a sibling sits there.  Two twins of every family start at one place
of the cache (twin_design.meeting_pairs), so the compare of the words behind word 0 runs between different keys.

That the route ran is shown as in test_overflow_paths_modes: stats()["fallback_inserts"] is at least the family's
occurrences minus what the lists it can reach hold (cap_sub, fused_lists_hold -- imported from there), and that bound is
at least HOT_SPILLS; bound and value are printed.  What the host cannot see is WHICH form of level 2 took the bucket:
skew_probe_kernel decides on the device from a sample of up to 4096 records of the bucket and wants eight different records
four times each.  The cases are sized for it -- 16 to 48 hot records, each dozens of times among a few thousand cold
records per bucket -- and where it decides otherwise the plain form's one-probe cache compares the same twins.

Kernels, by case (record words RW; threads; SKEW -- both forms of level 2 are launched for every table, a bucket is
worked by one of them):
    k31-{lo,hi}-level2   walk_part_kernel<512, false, true>, partition_ring_kernel<1, 512, false | true> with
                         pre-formatted records (fmt = 1); half_twins of the low and the high half of the word
    k31-{lo,hi}-walk     the same kernels with level-1 lists of 16 keys (TSX_HIP_CAP1): the walk's `spill`
    k63-t1, k33-t1       walk_log_wide_kernel<2>, partition_ring_kernel<2, 512, false> (level 1), <2, 512, false | true>
                         (level 2); k = 33: word 1 carries two bits, so four families of four twins share one segment
    k96-t1, k96-t2       walk_log_wide_kernel<3>, partition_ring_kernel<4, ...>: records of four words, the fourth zero
    k127-t1 .. t3        walk_log_wide_kernel<4>, partition_ring_kernel<4, ...>
    k63-t1-canonical     walk_log_wide_kernel<2, true>; records are compared after the strand choice, so one canonical
                         case is enough.  Odd rounds of the text show the other strand.
    k63-t1-chunks        spill_record's chunk route across a chunk boundary (dch, DCH_MAX): 48 twins start at 8 places
                         of the cache, at most 11 are ever cached; the records of the others fill the overflow queue
                         (2048) and then more than 4096 places of the deferred list, the largest chunk there is
    homopolymers         walk_part_kernel<512, false | true, true> with TSX_HIP_CAP1: see the test
Not reached: the forms at 1024 threads (levels of 512 lists: partition_ring_kernel<RW, 1024, .>, walk_part_kernel<1024, .>),
the general (not LOCAL) form of the walk and level 1 over received keys (sharded runs), DCH_MAX chunks of one
workgroup (48 or 96 chunks of up to 4096 records: a text of hundreds of MB), the walk's per-wave hot-key cache with twins
(it holds homopolymer keys only).  The multi-GPU exchanges and tables above 2^32 slots stay out of scope."""
import numpy as np
import pytest

import kmerdb as K
import test_twin_keys_skew_cpu as C
import twin_design as D
from test_canonical import encode, fold, rc
from test_overflow_paths_modes import HOT_SPILLS, check_whole_table, fused_lists_hold
from test_twin_keys import geometry


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def new_map(T, monkeypatch, env, k, l, canonical):
    """A map made and used under the case's switches (TSX_HIP_SEG_BITS is read when the map is created, the others when
    a text is counted; monkeypatch takes them all back after the test)."""
    for name, value in env:
        monkeypatch.setenv(name, value)
    m = T.TSXHashMapHIP(l, 0, k, canonical=canonical)
    m.set_path("partitioned")
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.IDS)
def test_twins_on_the_skew_routes(T, tmp_path, monkeypatch, name):
    c = C.CASES[C.IDS.index(name)]
    m = new_map(T, monkeypatch, c.env, c.k, c.l, c.canonical)
    lay, rows, inv = geometry(T, m, 0, tmp_path)
    assert lay.S == C.layout_of(c).S and D.radix_split(lay.l, lay.S)[1] > 0
    d = C.design(c, rows, inv)                 # the designers assert their conditions under the map's own rows
    assert K.table_keys(d.members, rows, c.k, canonical=c.canonical) == d.keys
    bound = C.spill_bound(d)
    assert bound >= HOT_SPILLS
    for rep in (1, 2):
        m.countFastq(d.text)
        st = check_whole_table(T, m, d.want, c.k, rep)
        print("%s rep %d: fallback_inserts %d, bound %d" % (name, rep, st["fallback_inserts"], rep * bound))
        assert st["fallback_inserts"] >= rep * bound
    exp = np.array([2 * d.want[x] for x in d.members], dtype=np.uint64)
    assert np.array_equal(m.getKmerCounts(encode(d.members, c.k)), exp)
    other = m.getKmerCounts(encode([rc(x) for x in d.members], c.k))
    assert np.array_equal(other, exp) if c.canonical else not other.any()
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [False, True])
def test_homopolymers_hot_in_one_wave(T, tmp_path, monkeypatch, canonical):
    """The walk's per-wave hot-key cache (s_hot_key / s_hot_cnt) takes homopolymer k-mers only -- the keys s_homh[b] --,
    so no twin can be designed into it.  It has HOT_N = 8 places per wave for at most four keys (two in a canonical
    table, where A/T and C/G fold): the keys cannot contend for places, and this case is a check of totals.  All four
    homopolymers are hot inside the strips of one wave, the reads of a half_twins family sit between them, and with
    level-1 lists of 16 keys (TSX_HIP_CAP1) the cache's flush (defer_append1) and the family's spill meet in one
    workgroup.  Counts are exact."""
    k = 31
    m = new_map(T, monkeypatch, (("TSX_HIP_CAP1", "16"),), k, 23, canonical)
    lay, rows, inv = geometry(T, m, 0, tmp_path)
    text, fwd, members, n = C.hom_design(rows, inv)
    want = fold(fwd) if canonical else fwd
    bound = n - fused_lists_hold(text, 32, 16, buckets=1)
    assert bound >= HOT_SPILLS
    for rep in (1, 2):
        m.countFastq(text)
        st = check_whole_table(T, m, want, k, rep)
        print("homopolymers rep %d: fallback_inserts %d, bound %d" % (rep, st["fallback_inserts"], rep * bound))
        assert st["fallback_inserts"] >= rep * bound
    for a, b in ((b"A", b"T"), (b"C", b"G")):
        ca, cb = m.getKmerCount((a * k).decode()), m.getKmerCount((b * k).decode())
        assert (ca == cb == 2 * (fwd[a * k] + fwd[b * k])) if canonical else (ca == 2 * fwd[a * k] and cb == 2 * fwd[b * k])
    assert (m.getKmerCounts(encode(members, k)) == 2 * C.HOM_ROUNDS).all()
    m.close()
