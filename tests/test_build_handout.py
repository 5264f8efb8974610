"""The hand-out of build_segments_stream_kernel (tsx_partition.h): a wave takes its stream batch by batch -- four batches of
64 keys in its ring, batch j + 4 refilled when batch j is used up, BK = 16 batches per pass.

Every case counts a small text through the partitioned path and compares the whole table, entry for entry, with a
dictionary count of the same text (conftest.python_counts, which shares no code with the kernels) and with the atomic path
of the same map geometry; the three failure counters must be 0.

The designed texts hold one k-mer per read, and the k-mers are chosen through the inverse of the map's hash so that segment
s receives exactly M[s] keys: the home slot is the low l bits of the hashed key (tsx_device.h: split_key), the segment its
top l - S bits, S taken from the map (DbInfo.seg_bits of its saved image).  With one radix level (l - S <= 8) or one level-2
workgroup per bucket (TSX_HIP_CPR2=1) all 16 waves of the build share the one list of the segment, batch t going to wave
t % 16: a list of M keys gives wave w the stream stream_len(M, w).  That the table was built the way the text was designed
is checked afterwards: every k-mer sits in the segment it was made for (getKmerCountDebug) and no key left the fast path
(fallback_inserts == 0), so the list of segment s held M[s] keys."""
import functools
import os

import numpy as np
import pytest

from conftest import python_counts
from test_canonical import encode, fastq_of, fold, rc

NW = 16           # waves of the build workgroup (1024 threads), all on one list when the segment has one list
BK = 16           # batches a wave holds per pass (tsx_partition.h)
PASS_KEYS = NW * BK * 64


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def stream_len(M, w, nw=NW):
    """keys of wave w's stream when a list of M keys is shared out in batches of 64, batch t to wave t % nw"""
    full, rem = divmod(M, 64)
    return 64 * len(range(w, full, nw)) + (rem if full % nw == w else 0)


# list sizes and the stream lengths they give some wave (asserted in test_designed_sizes_reach_the_stream_lengths)
ONE_PASS = [0, 1, 63, 64, 65, NW * 64 + 1, NW * 64 + 63, 3 * NW * 64 + 63, 3 * NW * 64 + 64, 4 * NW * 64, 4 * NW * 64 + 1,
            4 * NW * 64 + 63, 0, 5 * NW * 64 + 17]
TWO_PASS = [PASS_KEYS, PASS_KEYS + 1]
WANTED = [0, 1, 63, 64, 65, 127, 255, 256, 257, 4 * 64 + 1, 4 * 64 + 63]


def test_designed_sizes_reach_the_stream_lengths():
    got = {stream_len(M, w) for M in ONE_PASS for w in range(NW)}
    assert set(WANTED) <= got, sorted(set(WANTED) - got)
    assert stream_len(PASS_KEYS, 0) == BK * 64 == stream_len(PASS_KEYS, NW - 1)         # the last batch, no refill behind it
    assert stream_len(PASS_KEYS + 1, 0) == BK * 64 + 1                                  # one key in a second pass
    assert -(-(-(-TWO_PASS[1] // 64)) // (NW * BK)) == 2 and -(-(-(-TWO_PASS[0] // 64)) // (NW * BK)) == 1


def seg_bits_of(T, m, tmp_path):
    path = os.path.join(str(tmp_path), "geom_%d_%d.tsxdb" % (m.k, m.l))
    m.saveDatabase(path)
    S = int(T.database_info(path)["seg_bits"])
    os.remove(path)
    return S


def designed(T, m, S, sizes, segs, seed, distinct_per_seg=4096, name_pad=0):
    """One k-mer per read: sizes[i] keys for segment segs[i], at most distinct_per_seg different ones (the rest repeats).
    ({k-mer bytes: count}, {k-mer bytes: segment}, text)"""
    k, l = m.k, m.l
    rng = np.random.default_rng(seed)
    want, where, seqs = {}, {}, []
    for M, s in zip(sizes, segs):
        pool = []
        while len(pool) < min(M, distinct_per_seg):
            hi = int(rng.integers(0, 1 << (2 * k - l)))
            key = (hi << l) | (s << S) | int(rng.integers(0, 1 << S))
            x = T.decode(m.hash_invert(np.array([key], dtype=np.uint64)), k).encode()
            if x in where or len(set(x)) == 1:
                continue
            where[x] = s
            pool.append(x)
        for j in range(M):
            x = pool[j % len(pool)]
            want[x] = want.get(x, 0) + 1
            seqs.append(x)
    order = rng.permutation(len(seqs))
    pad = b" " + b"x" * name_pad if name_pad else b""
    return want, where, b"".join(b"@r%d%s\n%s\n+\n%s\n" % (n, pad, seqs[i], b"I" * k) for n, i in enumerate(order))


def dump_sorted(m):
    kk, cc = m.getAllKmers()
    o = np.lexsort(kk.T[::-1])
    return kk[o], cc[o]


def check(T, m, want, k, reps=1):
    """stats and the whole dump against {k-mer bytes: count}, everything counted reps times; returns the sorted dump"""
    total = sum(want.values())
    st = m.stats()
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0, st
    assert st["distinct"] == len(want), (st, len(want))
    assert st["kmers_added"] == reps * total and st["count_sum"] == reps * total, (st, reps * total)
    keys = sorted(want)
    exp_k = encode(keys, k)
    exp_c = np.array([want[x] for x in keys], dtype=np.uint64) * np.uint64(reps)
    o = np.lexsort(exp_k.T[::-1])
    got_k, got_c = dump_sorted(m)
    assert np.array_equal(got_k, exp_k[o]), "the table holds other k-mers than the text"
    bad = np.nonzero(got_c != exp_c[o])[0]
    assert bad.size == 0, [(T.decode(got_k[i], k), int(got_c[i]), int(exp_c[o][i])) for i in bad[:5]]
    assert np.array_equal(m.getKmerCounts(exp_k), exp_c)
    return got_k, got_c


def check_atomic(T, text, k, l, dump, reps=1, **kw):
    """the atomic path on a map of the same geometry holds the same table"""
    a = T.TSXHashMapHIP(l, kw.pop("s", 0), k, **kw)
    a.set_path("atomic")
    for _ in range(reps):
        a.countFastq(text)
    ak, ac = dump_sorted(a)
    st = a.stats()
    a.close()
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0, st
    assert np.array_equal(ak, dump[0]) and np.array_equal(ac, dump[1])


def check_segments(m, S, where, k):
    keys = sorted(where)
    _, pos = m.getKmerCountDebug(encode(keys, k))
    assert np.array_equal(pos >> np.uint64(S), np.array([where[x] for x in keys], dtype=np.uint64))


# ---- 1. designed lists, one radix level (build_segments_stream_kernel<false>, one list per segment) ----------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 14])
def test_designed_streams_one_level(T, tmp_path, k):
    """Stream lengths 0, 1, 63, 64, 65, 127, 255, 256, 257, 319 and BK * 64, BK * 64 + 1 (a second pass); empty segments
    between full ones; then the same text again without clear() (dirty segments are loaded, not filled), then clear()
    and a text that leaves most segments empty (their stale slots must go)."""
    l = 18
    m = T.TSXHashMapHIP(l, 0, k)
    m.set_path("partitioned")
    S = seg_bits_of(T, m, tmp_path)
    nseg = 1 << (l - S)
    if not (1 <= l - S <= 8 and nseg >= len(ONE_PASS) + len(TWO_PASS)):
        pytest.skip("geometry: l - S = %d gives no one-level build of %d lists" % (l - S, len(ONE_PASS) + len(TWO_PASS)))
    if (1 << S) * 4 < PASS_KEYS + 1:
        pytest.skip("geometry: a segment of 2^%d slots cannot take a two-pass list" % S)
    sizes = ONE_PASS + TWO_PASS
    want, where, text = designed(T, m, S, sizes, list(range(len(sizes))), seed=100 + k)
    assert dict(python_counts(text, k)) == want
    for rep in (1, 2):
        m.countFastq(text)
        dump = check(T, m, want, k, rep)
        assert m.stats()["fallback_inserts"] == 0
    check_segments(m, S, where, k)
    check_atomic(T, text, k, l, dump, reps=2)
    # clear(), then keys for two segments only: every other segment is empty and fresh
    m.clear()
    want2, where2, text2 = designed(T, m, S, [257, 65], [nseg - 1, 1], seed=200 + k)
    m.countFastq(text2)
    dump2 = check(T, m, want2, k)
    check_segments(m, S, where2, k)
    check_atomic(T, text2, k, l, dump2)
    m.close()


# ---- 2. designed lists, two radix levels with one level-2 workgroup per bucket (<true>: pre-formatted records) -----------

@pytest.mark.gpu
def test_designed_streams_two_levels(T, tmp_path, monkeypatch):
    k, l = 31, 23
    monkeypatch.setenv("TSX_HIP_CPR2", "1")
    m = T.TSXHashMapHIP(l, 0, k)
    m.set_path("partitioned")
    S = seg_bits_of(T, m, tmp_path)
    nseg = 1 << (l - S)
    if l - S < 9:
        pytest.skip("geometry: l - S = %d has one radix level" % (l - S))
    sizes = [M for M in ONE_PASS if 0 < M <= 4 * NW * 64 + 63]
    assert set(WANTED) - {0} <= {stream_len(M, w) for M in sizes for w in range(NW)}
    segs = [(5 + 37 * i) % nseg for i in range(len(sizes))]            # spread over the level-1 buckets, empty ones between
    assert len(set(segs)) == len(segs)
    # (long read names: the capacity of a sub-list follows from the bytes of the text)
    want, where, text = designed(T, m, S, sizes, segs, seed=300, name_pad=160)
    assert dict(python_counts(text, k)) == want
    # a sub-list holds more than the longest designed list (plan_partition's cap_sub, from the size of the text)
    per_sub = (len(text) // 2 + 65536) // nseg
    assert per_sub + per_sub // 4 >= max(sizes)
    for rep in (1, 2):
        m.countFastq(text)
        dump = check(T, m, want, k, rep)
        assert m.stats()["fallback_inserts"] == 0
    check_segments(m, S, where, k)
    check_atomic(T, text, k, l, dump, reps=2)
    m.close()


# ---- 3. ordinary reads at the default geometry (level-2 sub-lists, 16 / cpr2 waves per list) ----------------------------

@functools.lru_cache(maxsize=None)
def reads_text(seed, n):
    from tsxcount_amd import synth
    return synth.fastq(seed, 0, n)


@pytest.mark.gpu
@pytest.mark.parametrize("k,l,canonical", [(31, 23, False), (14, 23, False), (31, 23, True), (31, 18, True)])
def test_reads_default_geometry(T, k, l, canonical):
    text = reads_text(77, 120)
    fwd = dict(python_counts(text, k))
    want = fold(fwd) if canonical else fwd
    m = T.TSXHashMapHIP(l, 0, k, canonical=canonical)
    m.set_path("partitioned")
    for rep in (1, 2):
        m.countFastq(text)
        dump = check(T, m, want, k, rep)
    if canonical:
        keys = sorted(want)[::11]
        exp = np.array([want[x] for x in keys], dtype=np.uint64) * np.uint64(2)
        assert np.array_equal(m.getKmerCounts(encode([rc(x) for x in keys], k)), exp)
    check_atomic(T, text, k, l, dump, reps=2, canonical=canonical)
    m.close()


# ---- 4. few k-mers many times over (the add branch, carries at C = 2), and a table at load 0.9 -----------------------------

@pytest.mark.gpu
def test_few_kmers_many_times_small_counters(T):
    k, l = 31, 18
    reads = [r[:200] for r in reads_text(5, 4).split(b"\n")[1::4]]
    text = fastq_of(reads * 400)
    want = dict(python_counts(text, k))
    assert len(want) <= 4 * 170 and min(want.values()) >= 400
    m = T.TSXHashMapHIP(l, 2, k, overflow_l=14)
    m.set_path("partitioned")
    m.countFastq(text)
    dump = check(T, m, want, k)
    st = m.stats()
    assert st["overflow_carries"] > 0 and st["overflow_used"] >= len(want) - 4     # every count carried (poly-A aside)
    check_atomic(T, text, k, l, dump, s=2, overflow_l=14)
    m.close()


@pytest.mark.gpu
def test_load_0_9_long_probe_chains(T):
    k, l = 31, 18
    n = 320
    text = reads_text(9, n)
    want = dict(python_counts(text, k))
    while len(want) > 0.92 * (1 << l):
        n -= 5
        text = reads_text(9, n)
        want = dict(python_counts(text, k))
    assert len(want) >= 0.88 * (1 << l), (len(want), n)
    m = T.TSXHashMapHIP(l, 0, k)
    m.set_path("partitioned")
    m.countFastq(text)
    dump = check(T, m, want, k)
    check_atomic(T, text, k, l, dump)
    m.close()
