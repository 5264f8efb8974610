"""Where the level-1 sub-lists of the fused walk lie (csrc/tsx_layout.h): workgroup-major after the LOCAL walk of a
plain one-GPU count, bucket-major after every other walk.  walk_part_kernel writes them; partition_ring_kernel and
skew_probe_kernel read them as the pieces of a bucket.

The GPU tests count k = 31 on the partitioned path and on the atomic path and compare every k-mer of the text and the
table's totals.  The table is the smallest that plan_partition splits by two radix levels with the fused walk: 2^17
slots in 256-slot segments (TSX_HIP_SEG_BITS=8, read when the map is made), as tests/test_walk_forms.py; the poly-A
shape needs 2^22 slots for its 1.5e6 distinct k-mers, same segments.  tsx_hip_level1_sizes_host hands out the shape,
the order and the published sizes of the lists the last walk left; the tests read them in the library's own order
(tsx_hip_sublist_first) to show that the text really drives level 2 over the piece addressing it is meant to.

A level-2 workgroup reads 2048 records per batch (RING_NT threads x 4 words).  A piece of 2048 records and more -- a
batch that leaves a piece after several full batches of it -- needs a text of 32 buckets x 512 workgroups x 2048
records, about 80 MB: not a test of seconds.  The crossings here are those of pieces shorter than a batch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31
L_SMALL = 17
BATCH_REC = 2048


# ---- the rule itself, on the CPU -------------------------------------------------------------------------------------
RULE_PROGRAM = r"""
#include "tsx_layout.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    const uint32_t nb = (uint32_t)atoi(argv[1]), G = (uint32_t)atoi(argv[2]);
    const uint64_t cap = (uint64_t)atoll(argv[3]);
    const int wgm = atoi(argv[4]);
    const tsx::SubListOrder o = tsx::sublist_order(nb, G, wgm);
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t g = 0; g < G; ++g)
            printf("%u %u %u %llu\n", b, g, tsx::sublist_number(o, b, g), (unsigned long long)tsx::sublist_first(o, b, g, cap));
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("sublist_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(RULE_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tsxcount_amd", "csrc"),
                           "-o", str(exe), str(src)])
    return str(exe)


@pytest.mark.parametrize("nb,G,cap", [(1, 1, 16), (2, 3, 16), (4, 4, 32), (8, 5, 48), (32, 18, 112), (3, 7, 16), (256, 9, 7696)])
@pytest.mark.parametrize("wgm", [0, 1])
def test_layout_rule_ranges_are_disjoint_aligned_and_invertible(rule_program, nb, G, cap, wgm):
    """cap is a multiple of 16 records, as plan_partition rounds it.  Every list lies on a 128-B line, inside the buffer
    of nb * G * cap records, apart from every other list; a list's size is published at its number, so the numbers are
    a permutation of 0 .. nb * G - 1.  Level 2 names a piece by (bucket r, piece g) and walks g = c, c + cpr, ...: that
    is the walk's (b, g) read backwards, so number -> (b, g) must be unique.  Workgroup-major: the nb lists of a
    workgroup are one stretch of nb * cap records; bucket-major: the G lists of a bucket are."""
    out = subprocess.check_output([rule_program, str(nb), str(G), str(cap), str(wgm)]).decode().split("\n")
    rows = np.array([[int(x) for x in line.split()] for line in out if line], dtype=np.int64)
    assert len(rows) == nb * G
    b, g, num, first = rows.T
    assert np.array_equal(first, num * cap)
    assert np.all((first * 8) % 128 == 0)
    assert first.min() == 0 and np.all(first + cap <= nb * G * cap)
    order = np.argsort(first)
    assert np.all(np.diff(first[order]) >= cap)                      # disjoint
    assert np.array_equal(np.sort(num), np.arange(nb * G))            # every size has a place of its own
    back = {int(n): (int(bb), int(gg)) for bb, gg, n in zip(b, g, num)}
    assert len(back) == nb * G                                        # piece number -> (bucket, workgroup) is a function
    if wgm:
        for gg in range(G):
            assert np.array_equal(np.sort(num[g == gg]), np.arange(gg * nb, (gg + 1) * nb))
    else:
        for bb in range(nb):
            assert np.array_equal(np.sort(num[b == bb]), np.arange(bb * G, (bb + 1) * G))
    # the library's host-side copy of the rule (what the GPU tests below read sizes with) is the same function
    import tsxcount_amd as T
    f = T.lib().tsx_hip_sublist_first
    assert all(f(nb, G, wgm, int(bb), int(gg), cap) == int(a) for bb, gg, a in zip(b, g, first))


# ---- counts on the GPU -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    assert os.path.exists(tsxcount_amd.LIB_PATH), "HIP extension missing: no fallback"
    assert tsxcount_amd.lib().tsx_hip_device_count() > 0, "no GPU"
    return tsxcount_amd


def kmers_of_text(text):
    from tsxcount_amd.verify import kmers_of
    seqs = [s for s in text.split(b"\n") if s][1::4]
    return np.unique(np.vstack([kmers_of(s, K) for s in seqs]), axis=0)


def level1(T, m):
    """(shape, sizes[b, g]) of the level-1 lists the last plain count of m left, read in the library's order."""
    sh = T.Level1Shape()
    T._check(m._lib.tsx_hip_level1_sizes_host(m.handle, ctypes.byref(sh), None, 0))
    flat = np.zeros(sh.nb * sh.G, dtype=np.uint64)
    T._check(m._lib.tsx_hip_level1_sizes_host(m.handle, ctypes.byref(sh), flat.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                               flat.size))
    f = T.lib().tsx_hip_sublist_first
    num = np.array([[f(sh.nb, sh.G, sh.wg_major, b, g, 1) for g in range(sh.G)] for b in range(sh.nb)], dtype=np.int64)
    return sh, np.minimum(flat[num], np.uint64(sh.cap)).astype(np.int64)


def crossings(sh, sizes):
    """Level-2 batches that run from the end of one piece into the next piece of their stream: workgroup c of bucket r
    streams pieces c, c + cpr2, ... in batches of 2048 records (partition_ring_kernel, next_batch)."""
    n = 0
    for r in range(sh.nb):
        for c in range(sh.cpr2):
            pc = [int(v) for v in sizes[r, c::sh.cpr2]]
            pi = poff = 0
            while True:
                while pi < len(pc) and poff >= pc[pi]:
                    poff -= pc[pi]
                    pi += 1
                if pi >= len(pc):
                    break
                left = pc[pi] - poff
                nxt = pc[pi + 1] if pi + 1 < len(pc) else 0
                nvalid = min(BATCH_REC, left + nxt)
                if nvalid > min(left, BATCH_REC):
                    n += 1
                if left > BATCH_REC:
                    poff += BATCH_REC
                else:
                    pi += 1
                    poff = nvalid - left
    return n


def counted(T, text, l, path):
    m = T.TSXHashMapHIP(l, 0, K)
    m.set_path(path)
    m.countFastq(text)
    return m


def assert_same_tables(part, atom, kmers):
    sp, sa = part.stats(), atom.stats()
    for key in ("distinct", "count_sum", "kmers_added"):
        assert sp[key] == sa[key], key
    for st in (sp, sa):
        assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0
    assert np.array_equal(part.getKmerCounts(kmers), atom.getKmerCounts(kmers))


def both_paths(T, text, l, monkeypatch):
    """The text counted on the partitioned path (LOCAL walk, workgroup-major lists) and on the atomic path: same table.
    Returns the partitioned map (open) for a look at its lists."""
    monkeypatch.setenv("TSX_HIP_SEG_BITS", "8")
    monkeypatch.delenv("TSX_HIP_LOCAL_LONG", raising=False)
    kmers = kmers_of_text(text)
    part, atom = counted(T, text, l, "partitioned"), counted(T, text, l, "atomic")
    try:
        assert_same_tables(part, atom, kmers)
    finally:
        atom.close()
    return part, kmers


def sparse_text():
    """Three clusters of three synth reads in a megabyte of records that hold no k-mer (2000-byte headers, 8 bases): the
    walk's G = bytes / 8192 = 126 workgroups share bytes / 1024 description regions (one per wave of a 4096-byte tile,
    workgroup g walks regions g, g + G, ...), and only the regions under a cluster hold strips.  The filler runs of
    74, 74, 74 and 278 records put the clusters on regions that are 18..29, 44..51 and 70..77 modulo G: about 28
    workgroups get strips, the others none -- every bucket's pieces are empty in front, between the clusters and behind."""
    from tsxcount_amd import synth

    def filler(n):
        return b"".join(b"@f%d " % i + b"h" * 2000 + b"\nACGTACGT\n+\n&&&&&&&&\n" for i in range(n))
    return (filler(74) + synth.fastq(41, 0, 3) + filler(74) + synth.fastq(41, 3, 3) + filler(74) + synth.fastq(41, 6, 3) +
            filler(278))


@pytest.mark.gpu
def test_mostly_empty_pieces(T, monkeypatch):
    from oracle.oracle import Oracle
    text = sparse_text()
    part, kmers = both_paths(T, text, L_SMALL, monkeypatch)
    try:
        sh, sizes = level1(T, part)
        assert sh.wg_major == 1 and sh.nb >= 2 and sh.G >= 64 and sh.cap % 16 == 0
        idle = int((sizes.sum(axis=0) == 0).sum())
        assert 2 * idle > sh.G, (idle, sh.G)                     # most workgroups got no strip
        lead = inner = trail = 0
        for b in range(sh.nb):
            full = np.flatnonzero(sizes[b])
            if len(full) >= 2:
                lead += full[0] > 0
                trail += full[-1] < sh.G - 1
                inner += bool(np.any(np.diff(full) > 1))
        assert lead and inner and trail, (lead, inner, trail)   # buckets with empty pieces in front, between and behind
        # the smallest shape: against the CPU restatement as well
        o = Oracle(K, 20, 4, seed=1)
        n = o.count_fastq(text)
        ok, oc = o.dump()
        st = part.stats()
        assert st["kmers_added"] == n and st["distinct"] == o.distinct() == len(kmers)
        assert np.array_equal(part.getKmerCounts(ok), oc)
        o.close()
    finally:
        part.close()


@pytest.mark.gpu
def test_batches_that_run_into_the_next_piece(T, monkeypatch):
    """70 synth reads, about 140 KB: the walk runs G = ceil(bytes / 8192) = 18 workgroups, more than the cpr2 <= 8
    level-2 workgroups of a bucket, so a level-2 stream (pieces c, c + cpr2, ...) holds two or three pieces; a piece has
    about 6e4 records / (32 buckets x 18 workgroups) = 100 records, far below a batch of 2048: the first batch of every
    stream takes what is left of its piece and goes on in the next one.  The published sizes must say so."""
    from tsxcount_amd import synth
    text = synth.fastq(52, 0, 70)
    part, _ = both_paths(T, text, L_SMALL, monkeypatch)
    try:
        sh, sizes = level1(T, part)
        assert sh.wg_major == 1 and sh.G > sh.cpr2
        assert crossings(sh, sizes) >= sh.nb, crossings(sh, sizes)   # (at least stream 0 of every bucket)
    finally:
        part.close()


@pytest.mark.gpu
def test_polya_tailed_reads_under_the_skew_probe(T, monkeypatch):
    """2000 reads as the bench's (500-1000 random bases + 100-300 A): the k-mers of j = 1..5 bases in front of 26+ A's
    occur once per read and land in a few buckets, where skew_probe_kernel samples runs of 16 records out of the pieces
    (a piece has about 1.7e6 records / (128 buckets x G) = 27 of them) and level 2 spills what a list cannot hold."""
    from tsxcount_amd import synth
    text = synth.fastq(63, 0, 2000)
    part, _ = both_paths(T, text, 22, monkeypatch)
    try:
        sh, sizes = level1(T, part)
        assert sh.wg_major == 1
        assert int((sizes >= 16).sum()) > sizes.size // 2           # pieces the probe can sample
    finally:
        part.close()


@pytest.mark.gpu
def test_general_walks_keep_their_order_next_to_plain_counts(T, monkeypatch):
    """One map: a plain count (LOCAL walk, workgroup-major), the same count with long descriptions (general form, the
    same buffers, bucket-major), a sharded walk at one rank (minimizer exchange with one share: general form, the step's
    own lists, bucket-major) and a plain count again.  The table must hold what the atomic path holds after the same
    texts -- the homopolymers of the exchanged text excepted, which its sender counts on the side."""
    import torch
    from tsxcount_amd import synth
    monkeypatch.setenv("TSX_HIP_SEG_BITS", "8")
    monkeypatch.delenv("TSX_HIP_LOCAL_LONG", raising=False)
    text_a, text_b = synth.fastq(52, 0, 70), synth.fastq(74, 0, 30)
    kmers = kmers_of_text(text_a + text_b)
    hom = np.array([int(v) in (0, (1 << 62) // 3, 2 * ((1 << 62) // 3), (1 << 62) - 1) for v in kmers[:, 0]])
    m = T.TSXHashMapHIP(L_SMALL, 0, K)
    m.set_path("partitioned")
    L, vp = m._lib, ctypes.c_void_p
    try:
        m.countFastq(text_a)
        sh, sizes = level1(T, m)
        assert sh.wg_major == 1 and sizes.sum() > 0
        monkeypatch.setenv("TSX_HIP_LOCAL_LONG", "1")                 # general form: four strips per description
        m.countFastq(text_a)
        sh2, sizes2 = level1(T, m)
        assert sh2.wg_major == 0 and sizes2.sum() == sizes.sum()
        monkeypatch.delenv("TSX_HIP_LOCAL_LONG")
        # the sharded walk of text_b, one rank (as test_minimizer_split_lists_hold_what_the_host_function_says)
        assert L.tsx_hip_mini_supported(m.handle)
        buf = torch.frombuffer(bytearray(text_b + b"\n" * 64), dtype=torch.uint8).to("cuda:0")
        cap = ctypes.c_size_t(0)
        assert L.tsx_hip_mini_capacity(m.handle, len(text_b) + 256, 1, ctypes.byref(cap)) == 0
        cap = cap.value
        i64 = dict(dtype=torch.int64, device="cuda:0")
        dsc, cnt, emit = torch.empty((2 * cap,), **i64), torch.zeros((5,), **i64), torch.zeros((2,), **i64)
        assert L.tsx_hip_mini_window_device(m.handle, vp(buf.data_ptr()), len(text_b), 0, len(text_b), 1, vp(dsc.data_ptr()),
                                            cap, vp(cnt.data_ptr()), vp(emit.data_ptr()), None) == 0
        m.sync()
        n_desc = int(cnt[0].item())
        assert 0 < n_desc <= cap
        assert L.tsx_hip_shard_walk_device(m.handle, vp(dsc.data_ptr()), n_desc, 2, 0, 1, len(text_b), vp(emit[1:].data_ptr()),
                                           None) == 0
        assert L.tsx_hip_shard_build_l1_device(m.handle, None) == 0
        m.sync()
        m.countFastq(text_a)                                          # plain again, into the lists the first count used
        sh3, sizes3 = level1(T, m)
        assert sh3.wg_major == 1 and np.array_equal(sizes3, sizes)
        got = m.getKmerCounts(kmers)
        st = m.stats()
    finally:
        m.close()
    atom_a, atom_b = counted(T, text_a, L_SMALL, "atomic"), counted(T, text_b, L_SMALL, "atomic")
    try:
        want = 3 * atom_a.getKmerCounts(kmers) + np.where(hom, 0, atom_b.getKmerCounts(kmers)).astype(np.uint64)
    finally:
        atom_a.close()
        atom_b.close()
    assert np.array_equal(got, want)
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0
    assert st["count_sum"] == int(want.sum()) and st["distinct"] == int((want > 0).sum())
