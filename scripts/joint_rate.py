"""Rate of the joint histogram of two tables on the bench's table (one GPU).

A is the bench's table (bench.py's reads and seed, counted on the device), B the table of as many reads that share
half their read range with A's (scripts/combine_rate.py's pair).  Warm (one untimed call of each first), --runs runs
each, every value kept, median and spread (max - min) reported:
  joint_aligned / joint_general   tsx_hip_joint_histogram_host at --bins x --bins, TSX_HIP_COMBINE_PATH=2 / 1
  stats_aligned / stats_general   tsx_hip_combine(out = NULL), UNION, on the same pair and path: the same two sweeps and
                                  probes without the bins, so the difference is what the binning costs (an INTERSECT
                                  would not probe on side 1)
  histogram                       tsx_hip_histogram_host of A alone: the streaming floor of one sweep
These three are host calls that return when their work is done: host clock around each.  The *_device forms take a
stream, so the joint histogram (both paths) and the histogram are timed once more with events on a stream of the caller's
(joint_*_event_s, histogram_event_s); tsx_hip_combine has no such form.
--lib names another build of the library (one with -DTSX_JH_LDS_A=.. -DTSX_JH_LDS_B=.. for another LDS corner).
Prints one JSON line.

    python scripts/joint_rate.py [--k 31] [--l 30] [--reads 1087000] [--runs 5] [--bins 1002] [--lib PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402


def counted(a, first, dev, seed=1):
    nbytes, _, _ = T.synth_sizes(a.seed, first, a.reads, a.k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, first, a.reads, a.k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(a.l, 0, a.k, hash_seed=seed)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    del text
    torch.cuda.empty_cache()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bins", type=int, default=1002)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        T._abi.LIB_PATH = T.LIB_PATH = os.path.abspath(a.lib)   # (lib() reads its own module's)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    A = counted(a, 0, dev)
    B = counted(a, a.reads // 2, dev)          # same l, layout and seed: both paths apply
    sa, sb = A.stats(), B.stats()
    nb = a.bins
    out = {"k": a.k, "l": a.l, "bins": nb, "a_distinct": sa["distinct"], "b_distinct": sb["distinct"], "runs": a.runs,
           "lib": os.path.basename(T.LIB_PATH)}
    rule = T.combine_rule("union", "min")   # (UNION: side 1 probes A as well, as the joint histogram's side 1 does)

    def timed(fn):
        fn()   # warm
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    stream = torch.cuda.Stream(dev)
    buf = torch.empty(nb * nb, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def timed_events(fn):
        fn()
        stream.synchronize()
        ts = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3)
        return ts

    mats, stats = {}, {}
    for name, path in (("aligned", "2"), ("general", "1")):
        os.environ["TSX_HIP_COMBINE_PATH"] = path
        out["joint_%s_s" % name] = timed(lambda: mats.__setitem__(name, A.jointHistogram(B, nb, nb)))
        out["stats_%s_s" % name] = timed(lambda: stats.__setitem__(name, A._combine(B, rule, None)))
        out["joint_%s_event_s" % name] = timed_events(
            lambda: A.jointHistogramDevice(B, buf.data_ptr(), nb, nb, stream=stream.cuda_stream))
        assert np.array_equal(buf.cpu().numpy().view(np.uint64).reshape(nb, nb), mats[name]), name
    del os.environ["TSX_HIP_COMBINE_PATH"]
    hist = []
    out["histogram_s"] = timed(lambda: hist.append(A.getCountHistogram(nb)))
    hbuf = torch.empty(nb, dtype=torch.int64, device=dev)
    out["histogram_event_s"] = timed_events(lambda: T._check(T.lib().tsx_hip_histogram_device(
        A.handle, 0, int(A.layout.slots), nb, hbuf.data_ptr(), stream.cuda_stream)))

    # the results against each other and against what existed before
    m = mats["aligned"]
    assert np.array_equal(m, mats["general"])
    assert np.array_equal(m.sum(axis=1)[1:], hist[-1][1:]) and np.array_equal(m.sum(axis=0)[1:], B.getCountHistogram(nb)[1:])
    assert int(m[1:, 1:].sum()) == stats["aligned"]["both"] == stats["general"]["both"] and m[0, 0] == 0
    assert {f: A.stats()[f] for f in sa} == sa and {f: B.stats()[f] for f in sb} == sb
    out["a_only"], out["b_only"], out["both"] = int(m[1:, 0].sum()), int(m[0, 1:].sum()), int(m[1:, 1:].sum())
    out["nonzero_cells"] = int(np.count_nonzero(m))
    out["kmers_in_64x64"] = int(m[:64, :64].sum())
    out["kmers_in_128x32"] = int(m[:128, :32].sum())
    for f in list(out):
        if f.endswith("_s"):
            v = sorted(out[f])
            out[f[:-2] + "_median_s"] = v[len(v) // 2]
            out[f[:-2] + "_spread_s"] = v[-1] - v[0]
    # k-mers swept per second: both tables for the joint histogram and the stats, A alone for the histogram
    both_tables = sa["distinct"] + sb["distinct"]
    for f in ("joint_aligned", "joint_general", "stats_aligned", "stats_general"):
        out[f + "_Gkmers_per_s"] = both_tables / out[f + "_median_s"] / 1e9
    out["histogram_Gkmers_per_s"] = sa["distinct"] / out["histogram_median_s"] / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
