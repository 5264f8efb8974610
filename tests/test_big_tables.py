"""Tables above 2^32 slots, and count carries in tables built slab by slab.

A one-limb table of more than 2^32 slots (l - S > 18) is built slab by slab (count_slabs): every slab sees a view of the
table whose `table`, `seg_dirty` and `pos_base` are moved to the slab, while the secondary (count-overflow) array stays
keyed by whole-table slot numbers.  Wider tables of that size take the atomic path, and their word offsets pos * W pass
2^32 even below 2^32 slots.  These tests put keys where those indices cross 32 bits and check every reader of the table.

Expectations come only from independent sources: the oracle at a small table (counts do not depend on the geometry),
planted multiplicities, and a small restatement of where a key must sit:

    home slot  = low l bits of the hashed key
    probe i    = (home & ~segmask) | ((home + i(i+1)/2) & segmask),  i = 1, 2, ...

A cluster is n distinct keys with one home slot in an empty region: they occupy exactly the probes i = 1..n, in an
order that concurrent inserts leave open.  The keys are drawn with the wanted low bits and random high bits and turned
into k-mers with the inverse mapping.

The large cases (64-72 GiB tables) each run in a fresh process, one after another."""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GIB = 1 << 30
BIG_NEED = 96 * GIB      # the largest case: a 64 GiB table + 8 GiB of secondary array + scratch
LOOKBACK = 10            # a background key is placed within its first four probes (offsets <= 10) here
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    assert os.path.exists(tsxcount_amd.LIB_PATH), "HIP extension missing: no fallback"
    assert tsxcount_amd.lib().tsx_hip_device_count() > 0, "no GPU"
    return tsxcount_amd


# ---- the restatement: keys, homes, probes ------------------------------------------------------------------------------

def default_seg_bits(W, l):
    """The segment size a table gets by default (tsx_hip_create_shard); the cases also set it through TSX_HIP_SEG_BITS."""
    smax = 14 if W == 1 else 13 if W == 2 else 12
    return min(l, 12 if (W == 2 and l - 12 <= 18) else smax)


def tri(i):
    return i * (i + 1) // 2


def probe(home, i, S):
    m = (1 << S) - 1
    return (home & ~m) | ((home + tri(i)) & m)


def predicted_slots(home, n, S):
    return {probe(home, i, S) for i in range(1, n + 1)}


def hash_keys(rows, x, k):
    """The mapping applied to many k-mers at once: key bit n-1-i = parity(rows[i] & x), n = 2k (tsx_hip_hash_rows)."""
    n = 2 * k
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(len(x), -1)
    out = np.zeros_like(x)
    for i in range(n):
        par = np.zeros(len(x), dtype=np.uint64)
        for t in range(x.shape[1]):
            par += np.bitwise_count(x[:, t] & rows[i, t])
        b = n - 1 - i
        out[:, b // 64] |= (par & np.uint64(1)) << np.uint64(b % 64)
    return out


def kmer_codes(kmers, k):
    """(n, key_limbs) limbs -> (n, k) base codes 0..3 (base j at bits 2j of the limbs, A C G T = 0 1 2 3)."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(len(kmers), -1)
    codes = np.empty((len(kmers), k), dtype=np.uint8)
    for j in range(k):
        codes[:, j] = ((kmers[:, j // 32] >> np.uint64(2 * (j % 32))) & np.uint64(3)).astype(np.uint8)
    return codes


def codes_to_kmers(codes):
    n, k = codes.shape
    out = np.zeros((n, (2 * k + 63) // 64), dtype=np.uint64)
    for j in range(k):
        out[:, j // 32] |= codes[:, j].astype(np.uint64) << np.uint64(2 * (j % 32))
    return out


def kmer_strings(kmers, k):
    """List of ACGT byte strings, one per k-mer."""
    return np.ascontiguousarray(_ACGT[kmer_codes(kmers, k)]).view("S%d" % k).ravel().tolist()


def rc_kmers(kmers, k):
    return codes_to_kmers(3 - kmer_codes(kmers, k)[:, ::-1])


def lex_canonical(kmers, k):
    """The lexicographically smaller strand of every k-mer (what a canonical table reports)."""
    a = kmer_codes(kmers, k)
    r = (3 - a)[:, ::-1]
    d = a != r
    first = np.argmax(d, axis=1)
    rows = np.arange(len(a))
    take = d.any(axis=1) & (r[rows, first] < a[rows, first])
    return codes_to_kmers(np.where(take[:, None], r, a))


def combine(kmers, counts):
    """Sum the counts of equal k-mers: (unique kmers, summed counts)."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(len(kmers), -1)
    v = kmers.view(np.dtype((np.void, 8 * kmers.shape[1]))).ravel()
    u, first, inv = np.unique(v, return_index=True, return_inverse=True)
    tot = np.zeros(len(u), dtype=np.uint64)
    np.add.at(tot, inv.ravel(), np.asarray(counts, dtype=np.uint64))
    return kmers[first], tot


def sort_rows(kmers, counts):
    o = np.lexsort(kmers.T[::-1])
    return kmers[o], counts[o]


def hist_of(counts, nbins):
    c = np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(nbins - 1)).astype(np.int64)
    return np.bincount(c, minlength=nbins).astype(np.uint64)


def plant_cluster(m, rng, home, n, canonical=False):
    """n distinct k-mers whose hashed keys all have the home slot `home`; with canonical=True every key is also the
    smaller of the k-mer's two strand keys, so a canonical table counts it under that key."""
    k, wk, l = m.k, m.wk, m.l
    top = np.uint64((1 << ((2 * k) % 64 or 64)) - 1)
    low = np.uint64((1 << l) - 1)
    out, seen = [], set()
    while len(out) < n:
        key = np.frombuffer(rng.bytes(8 * wk), dtype=np.uint64).copy()
        key[0] = (key[0] & ~low) | np.uint64(home)
        key[-1] &= top
        x = m.hash_invert(key)
        assert np.array_equal(m.hash_apply(x), key), "hash_invert / hash_apply do not round-trip"
        if canonical:
            kr = m.hash_apply(rc_kmers(x[None], k)[0])
            if tuple(kr[::-1].tolist()) < tuple(key[::-1].tolist()):
                continue
        if x.tobytes() in seen:
            continue
        seen.add(x.tobytes())
        out.append(x)
    return np.array(out, dtype=np.uint64).reshape(n, wk)


def window_is_free(slots, bg_homes, S):
    """No background key has its home within LOOKBACK probes' reach of a predicted slot (bg_homes sorted)."""
    mask = (1 << S) - 1
    for p in slots:
        lo = np.searchsorted(bg_homes, np.uint64(p & ~mask))
        hi = np.searchsorted(bg_homes, np.uint64((p & ~mask) + mask + 1))
        d = (np.uint64(p) - bg_homes[lo:hi]) & np.uint64(mask)
        if (d <= LOOKBACK).any():
            return False
    return True


def records(kmers, reps, k, rng):
    """Every planted k-mer as its own FASTQ record of length k, repeated, in shuffled order."""
    strs = kmer_strings(kmers, k)
    recs = []
    for s, r in zip(strs, reps):
        recs += [b"@p\n" + s + b"\n+\n" + b"I" * k + b"\n"] * int(r)
    order = rng.permutation(len(recs))
    return b"".join(recs[i] for i in order)


def background(k, reads, seed):
    """(text, kmers, counts, k-mers added) of synthetic reads, counted by the oracle at a small table."""
    from oracle.oracle import Oracle
    from tsxcount_amd import synth
    text = synth.fastq(seed, 0, reads)
    o = Oracle(k, 24, 4, seed=1)
    n = o.count_fastq(text)
    kmers, counts = o.dump()
    o.close()
    return text, kmers, counts, n


# ---- what every table is checked for -------------------------------------------------------------------------------

def histogram_range(m, lo, hi, nbins=10002):
    return m.getCountHistogram(nbins, lo, hi)


def check_counts(m, ek, ec, added, nbins=(10002,)):
    """Counts against the expectation in both directions, the totals, and the whole-table histogram."""
    st = m.stats()
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0, st
    assert st["kmers_added"] == added, (st, added)
    assert st["distinct"] == len(ek), (st, len(ek))
    assert st["count_sum"] == int(ec.sum()), (st, int(ec.sum()))
    assert np.array_equal(m.getKmerCounts(ek), ec)
    gk, gc = m.getAllKmers()
    gk, gc = sort_rows(gk.reshape(len(gk), -1), gc)
    xk, xc = sort_rows(ek, ec)
    assert np.array_equal(gk, xk) and np.array_equal(gc, xc)
    for nb in nbins:
        assert np.array_equal(m.getCountHistogram(nb), hist_of(ec, nb)), nb
    return st


def check_clusters(m, clusters, S):
    """Every planted cluster sits on exactly the predicted slots."""
    got_all = []
    for home, keys in clusters:
        _, slots = m.getKmerCountDebug(keys)
        got = set(int(s) for s in slots)
        assert got == predicted_slots(home, len(keys), S), (home, sorted(got))
        got_all += sorted(got)
    return got_all


def check_kmer_starts(T, m, slots_set):
    nb = (int(m.layout.slots) + 7) // 8
    bits = np.zeros(nb, dtype=np.uint8)
    assert T.lib().tsx_hip_kmer_starts_host(m.handle, bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), nb) == T.OK
    assert int(np.bitwise_count(bits).sum(dtype=np.uint64)) == m.stats()["distinct"]
    for s in slots_set:
        assert (bits[s >> 3] >> (s & 7)) & 1, s


def check_range_dump(m, lo, hi, ek, ec, homes):
    """dumpRangeDevice over [lo, hi) (whole segments): exactly the expected keys whose home lies there."""
    import torch
    sel = (homes >= np.uint64(lo)) & (homes < np.uint64(hi))
    xk, xc = sort_rows(ek[sel], ec[sel])
    cap = len(xk) + 64
    dev = torch.device("cuda", m.device)
    kb = torch.zeros((cap, m.wk), dtype=torch.int64, device=dev)
    cb = torch.zeros(cap, dtype=torch.int64, device=dev)
    nb = torch.zeros(1, dtype=torch.int64, device=dev)
    m.dumpRangeDevice(lo, hi, kb.data_ptr(), cb.data_ptr(), cap, nb.data_ptr())
    n = int(nb.cpu()[0])
    assert n == len(xk), (lo, hi, n, len(xk))
    gk, gc = sort_rows(kb[:n].cpu().numpy().view(np.uint64).reshape(n, m.wk), cb[:n].cpu().numpy().view(np.uint64))
    assert np.array_equal(gk, xk) and np.array_equal(gc, xc), (lo, hi)


def read_count_file(path):
    """{kmer: count} of a .count text; every line well formed, every k-mer once."""
    with open(path, "rb") as f:
        data = f.read()
    assert data == b"" or data.endswith(b"\n")
    lines = data.split(b"\n")[:-1]
    out = {}
    for ln in lines:
        kmer, c = ln.split(b"\t")
        out[kmer] = int(c)
    assert len(out) == len(lines)
    return out


def check_text(m, ek, ec, tmpdir, lower=2, upper=1000):
    strs = kmer_strings(ek, m.k)
    want = dict(zip(strs, ec.tolist()))
    path = os.path.join(tmpdir, "t.count")
    lines, _ = m.writeCounts(path, chunk_bytes=64 << 20)
    assert lines == len(want) and read_count_file(path) == want
    sub = {x: c for x, c in want.items() if lower <= c <= upper}
    lines, _ = m.writeCounts(path, lower=lower, upper=upper, chunk_bytes=64 << 20)
    assert lines == len(sub) and read_count_file(path) == sub
    os.unlink(path)


def check_range_histograms(m, cut, ec, homes, whole):
    a = histogram_range(m, 0, cut)
    b = histogram_range(m, cut, int(m.layout.slots))
    assert np.array_equal(a, hist_of(ec[homes < np.uint64(cut)], 10002))
    assert np.array_equal(b, hist_of(ec[homes >= np.uint64(cut)], 10002))
    assert np.array_equal(a + b, whole)


def check_cleared(m):
    st = m.stats()
    assert st["distinct"] == 0 and st["count_sum"] == 0, st
    assert not m.getCountHistogram(10002).any()


# ---- 1. the slot predictor at l = 20 (main process) --------------------------------------------------------------------

@pytest.mark.parametrize("path", ["atomic", "partitioned"])
def test_planted_clusters_sit_where_predicted(T, monkeypatch, path):
    k, l = 31, 20
    S = default_seg_bits(1, l)
    monkeypatch.setenv("TSX_HIP_SEG_BITS", str(S))
    m = T.TSXHashMapHIP(l, 0, k)
    try:
        assert m.layout.entry_limbs == 1
        m.set_path(path)
        rng = np.random.default_rng(20)
        nmax = min(60, int(m.layout.max_reprobes))
        seg = 1 << S
        # one cluster mid-segment, a full-length one, and one whose probes wrap at the end of its segment
        clusters = [(5 * seg + 1000, 8), (9 * seg + 77, nmax), (13 * seg - 2, 6), ((1 << l) - 1, 5)]
        planted = [(h, plant_cluster(m, rng, h, n)) for h, n in clusters]
        assert probe(13 * seg - 2, 2, S) == 12 * seg + 1    # the wrap really happens
        reps = []
        for ci, (_, keys) in enumerate(planted):
            reps += [1 + (ci + j) % 4 for j in range(len(keys))]
        allk = np.concatenate([keys for _, keys in planted])
        m.countFastq(records(allk, reps, k, rng))
        check_counts(m, allk, np.array(reps, dtype=np.uint64), sum(reps))
        check_clusters(m, planted, S)
        assert len(allk) == len(set(s.tobytes() for s in allk))
    finally:
        m.close()


# ---- the large cases: one fresh process each -----------------------------------------------------------------------

def run_case(name, args, env, timeout):
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import torch; torch.zeros(1, device='cuda:0'); torch.cuda.synchronize()\n"
            "import test_big_tables as B\n"
            "B.%s(*%r)\n"
            "print('CASE OK')\n") % (HERE, ROOT, name, tuple(args))
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=timeout, cwd=ROOT)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "CASE OK" in out, "exit %d\n%s" % (p.returncode, out[-4000:])


def need_memory(nbytes):
    import torch
    torch.cuda.empty_cache()
    total = torch.cuda.get_device_properties(0).total_memory
    if total < nbytes:
        pytest.skip("needs %.0f GiB of device memory, the device has %.0f GiB (not an MI355X)" % (nbytes / GIB, total / GIB))


# ---- 2. count carries in slab-built tables (2^25 slots, 4 slabs) ---------------------------------------------------

def case_slab_carries(s):
    import tsxcount_amd as T
    k, l = 31, 25
    S = int(os.environ["TSX_HIP_SEG_BITS"])
    sb = l - S - int(os.environ["TSX_HIP_SLAB_SEGBITS"])
    assert sb == 2
    slab = 1 << (l - sb)
    seg = 1 << S
    rng = np.random.default_rng(1000 + s)
    m = T.TSXHashMapHIP(l, s, k)
    a = T.TSXHashMapHIP(l, s, k)
    try:
        assert m.layout.entry_limbs == 1 and m.layout.count_bits == s
        m.set_path("partitioned")
        a.set_path("atomic")
        rows = m.hash_rows()
        assert np.array_equal(rows, a.hash_rows())
        bg_text, bk, bc, bn = background(k, 200, 77)
        assert np.array_equal(hash_keys(rows, bk[:50], k), np.array([m.hash_apply(x) for x in bk[:50]]))
        bg_homes = np.sort(hash_keys(rows, bk, k)[:, 0] & np.uint64((1 << l) - 1))
        mults = [2 ** s - 1, 2 ** s, 2 ** s + 1, 1000, 65537]
        planted, reps = [], []
        for j in range(1 << sb):
            base = j * slab
            # a cluster in the first segment of the slab, and one at the end of its last segment (its probes wrap)
            for cands in ([base + t for t in range(0, seg, 37)], [base + slab - 1 - t for t in range(0, seg, 5)]):
                home = next(h for h in cands if window_is_free(predicted_slots(h, len(mults), S), bg_homes, S))
                planted.append((home, plant_cluster(m, rng, home, len(mults))))
                rot = len(planted) % len(mults)
                reps += mults[rot:] + mults[:rot]
        assert any(probe(h, len(mults), S) < h for h, _ in planted)   # some cluster wraps
        pk = np.concatenate([keys for _, keys in planted])
        text = bg_text + records(pk, reps, k, rng)
        added = bn + sum(reps)
        ek, ec = combine(np.concatenate([bk, pk]), np.concatenate([bc, np.array(reps, dtype=np.uint64)]))
        homes = hash_keys(rows, ek, k)[:, 0] & np.uint64((1 << l) - 1)
        nb2 = (10002, 1 << 17)

        def slab_hists(mm, cc):
            for j in range(1 << sb):
                sel = (homes >> np.uint64(l - sb)) == np.uint64(j)
                got = mm.getCountHistogram(1 << 17, j * slab, (j + 1) * slab)
                assert np.array_equal(got, hist_of(cc[sel], 1 << 17)), j

        m.countFastq(text)
        st = check_counts(m, ek, ec, added, nb2)
        assert st["overflow_carries"] > 0 and st["overflow_used"] >= len(planted), st
        slots_m = check_clusters(m, planted, S)
        slab_hists(m, ec)
        a.countFastq(text)
        check_counts(a, ek, ec, added, nb2)
        assert check_clusters(a, planted, S) == slots_m
        ak, ac = sort_rows(*a.getAllKmers())
        mk, mc = sort_rows(*m.getAllKmers())
        assert np.array_equal(ak, mk) and np.array_equal(ac, mc)
        # a second count into the same (now dirty) table: every carry lands on the slot that already holds it
        m.countFastq(text)
        check_counts(m, ek, 2 * ec, 2 * added, nb2)
        check_clusters(m, planted, S)
        slab_hists(m, 2 * ec)
        m.clear()
        check_cleared(m)
        m.countFastq(text)
        check_counts(m, ek, ec, added, nb2)
        check_clusters(m, planted, S)
        slab_hists(m, ec)
    finally:
        m.close()
        a.close()


@pytest.mark.parametrize("s", [1, 2])
def test_count_carries_in_slab_built_tables(T, s):
    """Narrow counters (s = 1, 2) in a 2^25-slot table built in 4 slabs (TSX_HIP_SLAB_SEGBITS=9): hot clusters in the
    first and last segment of every slab, so carries from every slab go to the secondary array with pos_base != 0."""
    need_memory(4 * GIB)
    run_case("case_slab_carries", [s], {"TSX_HIP_SLAB_SEGBITS": "9", "TSX_HIP_SEG_BITS": "14",
                                        "TSX_HIP_DEV_WINDOW": str(4 << 20)}, 900)


# ---- 3 and 4. tables whose slot numbers or word offsets pass 2^32 --------------------------------------------------

def case_big(k, l, s, path, canonical, text_homes, add_homes):
    """A 64 GiB table: clusters planted at text_homes (through the FASTQ text) and add_homes (through addKmers with
    explicit counts) on top of a synthetic background; every reader checked against the oracle + planted counts."""
    import tsxcount_amd as T
    S = int(os.environ["TSX_HIP_SEG_BITS"])
    rng = np.random.default_rng(l * 1000 + k)
    m = T.TSXHashMapHIP(l, s, k, canonical=canonical)
    try:
        W = int(m.layout.entry_limbs)
        slots = int(m.layout.slots)
        assert slots == 1 << l and S == default_seg_bits(W, l)
        assert s == 0 or m.layout.count_bits == s      # (s = 0: counters as wide as the slot leaves room for)
        assert W * slots > 1 << 32
        m.set_path(path)
        rows = m.hash_rows()
        bg_text, bk, bc, bn = background(k, 3000 if k == 31 else 1000, 5)
        assert np.array_equal(hash_keys(rows, bk[:50], k), np.array([m.hash_apply(x) for x in bk[:50]]))
        key = hash_keys(rows, bk, k)
        if canonical:   # the key of a strand pair is the smaller of its two (one-limb keys here)
            assert m.wk == 1
            key = np.minimum(key, hash_keys(rows, rc_kmers(bk, k), k))
        bg_homes = np.sort(key[:, 0] & np.uint64(slots - 1))
        mults = [1, 3, 4, 5, 1000, 65537]
        planted, text_k, text_r, add_k, add_c = [], [], [], [], []
        for home in text_homes:
            keys = plant_cluster(m, rng, home, len(mults), canonical)
            planted.append((home, keys))
            text_k.append(keys)
            text_r += mults
        big = [1, 3, 4, 5, 1 << 20, (1 << 40) + 7]
        for home in add_homes:
            keys = plant_cluster(m, rng, home, len(big), canonical)
            planted.append((home, keys))
            add_k.append(keys)
            add_c += big
        for home, keys in planted:
            assert window_is_free(predicted_slots(home, len(keys), S), bg_homes, S), home
        allp = set().union(*(predicted_slots(h, len(kk), S) for h, kk in planted))
        assert len(allp) == sum(len(kk) for _, kk in planted)   # the clusters do not share a slot
        pk = np.concatenate(text_k + add_k)
        pc = np.array(text_r + add_c, dtype=np.uint64)
        text = bg_text + records(np.concatenate(text_k), text_r, k, rng)
        added = bn + sum(text_r) + sum(add_c)
        ek, ec = combine(np.concatenate([bk, pk]), np.concatenate([bc, pc]))
        if canonical:
            ek, ec = combine(lex_canonical(ek, k), ec)
        homes = (np.minimum(hash_keys(rows, ek, k), hash_keys(rows, rc_kmers(ek, k), k)) if canonical
                 else hash_keys(rows, ek, k))[:, 0] & np.uint64(slots - 1)
        cut = (1 << 32) // W if W > 1 else 1 << 32
        tmpdir = tempfile.mkdtemp(prefix="tsx_big_")

        def count():
            m.countFastq(text)
            if add_k:
                m.addKmers(np.concatenate(add_k), counts=np.array(add_c, dtype=np.uint64))

        def check_all():
            check_counts(m, ek, ec, added)
            if canonical:   # either strand finds the pair's counter
                assert np.array_equal(m.getKmerCounts(rc_kmers(ek, k)), ec)
            got = check_clusters(m, planted, S)
            assert max(got) >= cut
            whole = m.getCountHistogram(10002)
            check_range_histograms(m, cut, ec, homes, whole)
            for lo, hi in ((cut - (1 << S), cut + (1 << S)), (slots - (1 << S), slots)):
                check_range_dump(m, lo, hi, ek, ec, homes)
            check_text(m, ek, ec, tmpdir)
            check_kmer_starts(T, m, got)

        count()
        check_all()
        if s:
            assert m.stats()["overflow_used"] >= len(planted)
        m.clear()
        check_cleared(m)
        count()
        check_all()
        os.rmdir(tmpdir)
    finally:
        m.close()


L33_HOMES = [(1 << 32) - 3, 1 << 32, (1 << 32) + 1, (1 << 33) - 1]


@pytest.mark.parametrize("path,s,canonical", [("partitioned", 0, False), ("partitioned", 2, False), ("atomic", 0, False),
                                              ("atomic", 2, False), ("partitioned", 0, True)])
def test_one_limb_table_above_2_32_slots(T, path, s, canonical):
    """k = 31, l = 33: 2^33 one-limb slots (64 GiB); the partitioned path builds it in 2 slabs of 2^32 slots.  Clusters
    wrap inside the last segment of slab 0 (2^32 - 3), start slab 1 (2^32, 2^32 + 1) and end the table (2^33 - 1)."""
    need_memory(BIG_NEED)
    assert probe(L33_HOMES[0], 2, 14) == (1 << 32) - (1 << 14)   # the first cluster wraps inside its segment
    run_case("case_big", [31, 33, s, path, canonical, L33_HOMES, []], {"TSX_HIP_SEG_BITS": str(default_seg_bits(1, 33))},
             1200)


@pytest.mark.parametrize("k,l,W", [(63, 32, 2), (127, 31, 4)])
def test_wide_table_word_offsets_above_2_32(T, k, l, W):
    """2- and 4-limb slots, 64 GiB: the word offset pos * W passes 2^32 at slot 2^32 / W.  Clusters just below that
    slot (wrapping in their segment), at it (through addKmers, carrying at s = 2) and at the last slot."""
    need_memory(BIG_NEED)
    S = default_seg_bits(W, l)
    cut = (1 << 32) // W
    run_case("case_big", [k, l, 2, "atomic", False, [cut - 3, (1 << l) - 1], [cut]], {"TSX_HIP_SEG_BITS": str(S)}, 1200)


# ---- 5. a database of a table above 2^32 slots ---------------------------------------------------------------------

def case_big_database(k, l, s, homes):
    """The partitioned k = 31, l = 33, s = 2 table of case_big saved as a k-mer database: the file read with kmerdb
    (non-zero bitmap words only), placed directly into a fresh l = 33 table, counted on again slab by slab (the build
    merges with the segments the load marked dirty) and re-inserted into a small table."""
    import kmerdb as K
    import tsxcount_amd as T
    S = int(os.environ["TSX_HIP_SEG_BITS"])
    rng = np.random.default_rng(l * 1000 + k + 1)
    tmpdir = tempfile.mkdtemp(prefix="tsx_bigdb_")
    db = os.path.join(tmpdir, "big.db")
    m = T.TSXHashMapHIP(l, s, k)
    try:
        assert m.layout.count_bits == s and S == default_seg_bits(1, l)
        m.set_path("partitioned")
        rows = m.hash_rows()
        bg_text, bk, bc, bn = background(k, 3000, 5)
        bg_homes = np.sort(hash_keys(rows, bk, k)[:, 0] & np.uint64((1 << l) - 1))
        mults = [1, 3, 4, 5, 1000, 65537]
        planted = [(h, plant_cluster(m, rng, h, len(mults))) for h in homes]
        for h, keys in planted:
            assert window_is_free(predicted_slots(h, len(keys), S), bg_homes, S), h
        pk = np.concatenate([keys for _, keys in planted])
        reps = mults * len(homes)
        text = bg_text + records(pk, reps, k, rng)
        added = bn + sum(reps)
        ek, ec = combine(np.concatenate([bk, pk]), np.concatenate([bc, np.array(reps, dtype=np.uint64)]))
        m.countFastq(text)
        check_counts(m, ek, ec, added)
        assert max(check_clusters(m, planted, S)) >= 1 << 32
        m.saveDatabase(db)
    finally:
        m.close()
    f = K.read_db(db, rows)
    assert f.kmers == dict(zip(kmer_strings(ek, k), ec.tolist()))
    assert len(f.carries) >= len(planted) and max(f.entries) >= 1 << 32
    d = T.TSXHashMapHIP(l, s, k)   # direct placement
    try:
        d.addDatabase(db)
        check_counts(d, ek, ec, added)
        check_clusters(d, planted, S)
        d.set_path("partitioned")
        d.countFastq(text)
        check_counts(d, ek, 2 * ec, 2 * added)
        check_clusters(d, planted, S)
    finally:
        d.close()
    r = T.TSXHashMapHIP(24, s, k)   # re-insert
    try:
        r.addDatabase(db)
        check_counts(r, ek, ec, added)
    finally:
        r.close()
    os.unlink(db)
    os.rmdir(tmpdir)


def test_database_of_a_table_above_2_32_slots(T):
    """Save and load a 2^33-slot table: its bitmap alone is 1 GiB."""
    need_memory(BIG_NEED)
    free = shutil.disk_usage(tempfile.gettempdir()).free
    if free < 4 * GIB:
        pytest.skip("needs 4 GiB free in %s for the database, has %.1f GiB" % (tempfile.gettempdir(), free / GIB))
    run_case("case_big_database", [31, 33, 2, L33_HOMES], {"TSX_HIP_SEG_BITS": str(default_seg_bits(1, 33))}, 1500)
