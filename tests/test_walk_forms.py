"""The two forms of walk_part_kernel (tsx_partition.h) and its k-dependent unrolled loops.

A plain one-GPU count launches the LOCAL form of the walk; the same count with four strips per description
(TSX_HIP_LOCAL_LONG=1, read at every call) launches the general form.  Both must leave the same table, and that table
must be the oracle's.  The first-window hash is unrolled over its 4-bit groups and the homopolymer smear over its
doubling steps, both behind tests on k alone: the values of k below cross every group count (2, 3, 4, 5, 8, 9, 15, 16)
and every span boundary of the smear, and the reads end in homopolymer tails of k-2 .. k+1 bases of all four bases, so
that the smear's last partial step decides which windows are homopolymers.

The walk runs only where the table is split by two radix levels (at least 2^9 segments): 2^17 slots in 256-slot
segments (TSX_HIP_SEG_BITS=8, read when the map is made).  A table needs 2k > l, so k <= 8 cannot reach the walk at any
size; those values are counted on the partitioned path of the largest table they admit all the same.  At these sizes a
region holds far fewer than the 512 strips of a batch: every batch is a last batch with idle waves (regions of many
batches are what the full-size tests of test_gpu_parity.py run)."""
import numpy as np
import pytest

K_VALUES = (3, 4, 5, 8, 9, 16, 17, 30, 31, 32)


def tailed_reads(k, n_reads, seed):
    """Reads whose last bases are a homopolymer run of k-2, k-1, k or k+1 bases, of A, C, G and T in turn; the base in
    front of the run is another one.  k <= 5: bodies over A and C only (the table has fewer slots than there are k-mers)."""
    rng = np.random.default_rng(seed)
    alpha = b"AC" if k <= 5 else b"ACGT"
    lut = np.frombuffer(alpha, dtype=np.uint8)
    recs = []
    for r in range(n_reads):
        base = b"ACGT"[r % 4:r % 4 + 1]
        run = max(1, k - 2 + (r // 4) % 4)
        n = int(rng.integers(k, k + 90)) if r % 7 else int(rng.integers(1, k + 2))   # some reads at or below k
        body = lut[rng.integers(0, len(alpha), n)].tobytes()
        other = b"C" if base == b"A" else b"A"
        seq = body + other + base * run
        recs.append(b"@r%d\n" % r + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    return b"".join(recs)


def geometry(k):
    """(l, reads): the two-level table of the walk where the key is wide enough, else the largest table k admits."""
    if 2 * k > 17:
        return 17, 300
    return 2 * k - 1, (6 if k <= 5 else 200)


_expect = {}


def expected(T, k, canonical):
    """Oracle counts of the text for k, sorted; canonical: folded by strand.  Computed once per (k, canonical)."""
    key = (k, canonical)
    if key not in _expect:
        from oracle.oracle import Oracle
        l, reads = geometry(k)
        text = tailed_reads(k, reads, 500 + k)
        o = Oracle(k, min(max(l, 16), 24, 2 * k - 1), 4, seed=1)
        n = o.count_fastq(text)
        kmers, counts = o.dump()
        o.close()
        if canonical:
            can = T.canonical(kmers, k).reshape(len(kmers), -1)
            uniq, inv = np.unique(can, axis=0, return_inverse=True)
            tot = np.zeros(len(uniq), dtype=np.uint64)
            np.add.at(tot, inv.ravel(), counts)
            kmers, counts = uniq, tot
        order = np.lexsort(kmers.T[::-1])
        _expect[key] = (text, n, kmers[order], counts[order])
        for a in _expect[key][2:]:
            a.setflags(write=False)
    return _expect[key]


def table_of(T, text, k, l, canonical):
    m = T.TSXHashMapHIP(l, 0, k, canonical=canonical)
    m.set_path("partitioned")
    try:
        m.countFastq(text)
        st = m.stats()
        assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0
        gk, gc = m.getAllKmers()
        order = np.lexsort(gk.T[::-1])
        return st["kmers_added"], gk[order], gc[order]
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", K_VALUES)
def test_local_and_general_walk_leave_the_oracles_table(k, canonical, monkeypatch):
    import tsxcount_amd as T
    assert T.lib().tsx_hip_device_count() > 0, "no GPU"
    l, _ = geometry(k)
    text, n, want_k, want_c = expected(T, k, canonical)
    monkeypatch.setenv("TSX_HIP_SEG_BITS", "8")
    monkeypatch.delenv("TSX_HIP_LOCAL_LONG", raising=False)
    n_loc, k_loc, c_loc = table_of(T, text, k, l, canonical)        # LOCAL form
    monkeypatch.setenv("TSX_HIP_LOCAL_LONG", "1")
    n_gen, k_gen, c_gen = table_of(T, text, k, l, canonical)        # general form (long descriptions)
    assert n_loc == n and n_gen == n
    assert np.array_equal(k_loc, k_gen) and np.array_equal(c_loc, c_gen)
    assert np.array_equal(k_loc, want_k) and np.array_equal(c_loc, want_c)


@pytest.mark.parametrize("k", K_VALUES)
def test_group_tables_map_nibble_zero_to_zero(k):
    """The unrolled first-window hash looks up all 4-bit groups of the masked window without a guard per group, the
    groups at and above bit 2k included: their nibble is 0 and must contribute nothing.  The map's own tables
    (tsx_hip_lut4_host, host only): entry 0 of every group is 0, the groups above bit 2k are 0 throughout, and the XOR
    over all 16 groups is GF(2)-linear in the window."""
    import ctypes
    import tsxcount_amd as T
    n = 2 * k
    top = (1 << n) - 1
    for seed in (1, 2, 77, 2 ** 63 + 11):
        lut = np.zeros(256, dtype=np.uint64)
        T._check(T.lib().tsx_hip_lut4_host(k, min(n - 1, 17), seed, lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        table = [[int(v) for v in lut[16 * g:16 * g + 16]] for g in range(16)]
        assert all(table[g][0] == 0 for g in range(16))
        assert all(table[g][v] == 0 for g in range((n + 3) // 4, 16) for v in range(16))
        assert any(table[0][v] for v in range(1, 16))

        def h(x):
            out = 0
            for g in range(16):
                out ^= table[g][(x >> (4 * g)) & 15]
            return out
        rng = np.random.default_rng(k)
        for _ in range(32):
            x, y = (int(v) & top for v in rng.integers(0, 2 ** 63, 2) * 2 + rng.integers(0, 2, 2))
            assert h(x ^ y) == h(x) ^ h(y) and h(x) <= top and (x == 0 or h(x) != 0)
