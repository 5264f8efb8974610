"""Stage timing over the call sequences that split one count over several entry points: the sharded steps (scan or
describe per window, level 1 or walks per window, then level 2 + build once) and the slab-by-slab build (describe per
window, then walks + level 2 + build per slab).  Every scanned or described window opens one tuple of eight events, a
slab opens one of its own; the tuples that wait for a partition phase in another call are parked on the map, oldest
first.  What is pinned here is that bookkeeping: how many tuples a sequence reports, that all of their events were
recorded (every interval finite), and that the parked tuples are gone afterwards."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

STAGES = {"line", "scan", "level1", "level2", "build", "gap", "post"}


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    assert os.path.exists(tsxcount_amd.LIB_PATH), "HIP extension missing: no fallback"
    assert tsxcount_amd.lib().tsx_hip_device_count() > 0, "no GPU"
    return tsxcount_amd


@pytest.fixture(scope="module")
def whole_counts():
    """The oracle's counts of the 400 reads both ranks share out, computed once."""
    from oracle.oracle import Oracle
    from tsxcount_amd import synth
    o = Oracle(31, 21, 4, seed=1)
    o.count_fastq(synth.fastq(66, 0, 400))
    return o.dump()


@pytest.mark.parametrize("mode,flt", [("keys", None), ("desc", "1"), ("desc", "0")])
def test_sharded_step_reports_one_tuple_per_window(T, monkeypatch, whole_counts, mode, flt):
    """world = 2 as two threads on cuda:0 (tests/_thread_comm.py), shard_bits = 1, l = 23 (two radix levels), three
    windows.  keys: scan_window x 3, l1_window x 3, build_l1;  desc, filter 1: desc_window x 3, shard_filter x 3,
    build_l1;  desc, filter 0: desc_window x 3, shard_walk x 3, build_l1.  Each rank reports three tuples -- the first
    carries the partition phase, the other two were closed where they were opened."""
    import threading
    import torch
    from _thread_comm import ThreadComm, ThreadWorld
    from tsxcount_amd import distributed as TD
    from tsxcount_amd import synth
    monkeypatch.setenv("TSX_HIP_SHARD_MODE", mode)
    if flt is not None:
        monkeypatch.setenv("TSX_HIP_SHARD_FILTER", flt)
    world, k, l, n_reads, windows = 2, 31, 23, 400, 3
    kmers, counts = whole_counts
    tw = ThreadWorld(world)
    got = [None] * world
    errs = []

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            first, cnt = TD.shard_reads(n_reads, rank, world)
            text = synth.fastq(66, first, cnt)
            buf = torch.frombuffer(bytearray(text + b"\n" * 64), dtype=torch.uint8).to("cuda:0")
            m = T.TSXHashMapHIP(l, 0, k, device=0, shard_bits=1, shard_index=rank)
            m.set_timing(True)
            sc = TD.ShardedCounter(m, len(text), group=ThreadComm(tw, rank), windows=windows)
            torch.cuda.synchronize()
            sc.step(buf.data_ptr(), len(text))
            assert sc.last["key_sum_diff"] == 0 and sc.last.get("mode", "keys") == mode
            stage, tuples = m.get_stage_timing()
            again = m.get_stage_timing()
            got[rank] = (m.getKmerCounts(kmers), stage, tuples, again)
            m.close()
        except BaseException as e:   # noqa: BLE001 -- a dead rank must not leave the other in a barrier
            errs.append((rank, repr(e)))
            tw.barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errs, errs
    for rank, (_, stage, tuples, again) in enumerate(got):
        print("rank %d: %d tuples, %s; then %d" % (rank, tuples, stage, again[1]))
        assert tuples == windows, (rank, tuples)
        assert set(stage) == STAGES
        assert all(math.isfinite(v) and v >= 0 for v in stage.values()), (rank, stage)
        assert stage["level1"] + stage["level2"] + stage["build"] > 0, (rank, stage)
        assert again[1] == 0 and all(v == 0 for v in again[0].values()), (rank, again)
    # nothing of the step is left behind for a plain count on another map
    plain = T.TSXHashMapHIP(l, 0, k)
    plain.set_timing(True)
    plain.countFastq(synth.fastq(66, 0, n_reads))
    stage, tuples = plain.get_stage_timing()
    assert tuples >= 1 and stage["scan"] > 0, (tuples, stage)
    assert np.array_equal(plain.getKmerCounts(kmers), counts)
    plain.close()
    total = sum(g[0].astype(np.int64) for g in got)
    assert np.array_equal(total.astype(np.uint64), counts), "sum over the 2 shards != oracle"


def test_slab_build_reports_one_tuple_per_window_and_per_slab():
    """count_slabs (tsxcount_hip.hip): every text window is described once -- one tuple each, closed there, and the
    parked ones dropped before the slabs start -- then every slab opens a tuple of its own around its walks, level 2
    and build.  l = 25 with TSX_HIP_SLAB_SEGBITS=9: 4 slabs (as test_tables_built_slab_by_slab); 1 MiB text windows.
    In a process of its own: the limit is read once per process."""
    code = r'''
import math, os, sys
import numpy as np
sys.path.insert(0, %r)
import tsxcount_amd as T
from oracle.oracle import Oracle
from tsxcount_amd import synth
l, k, reads, slabs = 25, 31, 3000, 4
text = synth.fastq(77, 0, reads)
o = Oracle(k, 24, 4, seed=1)
n = o.count_fastq(text)
kmers, counts = o.dump()
m = T.TSXHashMapHIP(l, 0, k)
m.set_path("partitioned")
m.set_timing(True)
m.countFastq(text)
stage, tuples = m.get_stage_timing()
windows = max(1, (len(text) + (1 << 20) - 1) >> 20)
print("tuples", tuples, "windows", windows, "slabs", slabs, stage)
assert windows > 1
assert tuples == windows + slabs, (tuples, windows, slabs)
assert all(math.isfinite(v) and v >= 0 for v in stage.values()), stage
assert stage["build"] > 0, stage
assert m.get_stage_timing()[1] == 0
st = m.stats()
assert st["kmers_added"] == n and st["distinct"] == len(kmers) and st["insert_failures"] == 0, st
assert np.array_equal(m.getKmerCounts(kmers), counts)
print("SLAB TIMING OK")
''' % (ROOT,)
    env = dict(os.environ, TSX_HIP_SLAB_SEGBITS="9", TSX_HIP_DEV_WINDOW=str(1 << 20))
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    print(p.stdout.decode()[-3000:])
    assert p.returncode == 0 and b"SLAB TIMING OK" in p.stdout, p.stdout.decode()[-3000:]
