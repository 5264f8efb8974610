"""Rate of read binning by two tables against two query passes, on the bench's text and table (one GPU).

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed).  Table A counts the whole
text, table B its first half (another seed with --b-seed: the two-LUT form of the kernel; the same seed: one LUT), so
that every read hits A and half of them hit B.  Then, interleaved round by round so that drift hits both sides alike,
each timed with HIP events on one stream (both calls wait for their stream):
  bin        tsx_hip_bin_stats_device(A, B) over the whole text: one scan, both tables probed per window;
  two_query  tsx_hip_query_reads_device over A and then over B, the same text: two scans -- existing code, the yardstick.
After --warmup untimed rounds, --reps rounds; medians, the spread (min .. max) and the ratio of the medians.  The stats of
both sides are compared: kmers and the hits in A and in B must agree.  Prints one JSON line.

    python scripts/bin_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 9] [--warmup 2] [--b-seed 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402


def once(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--b-seed", type=int, default=7, help="hash seed of table B (1 = A's: the one-LUT form)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    k = a.k
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    nbytes, kmers, _ = T.synth_sizes(a.seed, 0, a.reads, k)
    half_bytes, _, _ = T.synth_sizes(a.seed, 0, a.reads // 2, k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    A = T.TSXHashMapHIP(a.l, 0, k)
    B = T.TSXHashMapHIP(a.l - 1, 0, k, hash_seed=a.b_seed)
    A.countFastqDevice(text.data_ptr(), nbytes)
    B.countFastqDevice(text.data_ptr(), half_bytes)
    A.sync()
    B.sync()
    stream = torch.cuda.Stream(dev)   # not torch's default stream: that one does not wait for the maps' own
    sp = stream.cuda_stream

    bins = torch.zeros(a.reads * 4, dtype=torch.int64, device=dev)
    qa = torch.zeros(a.reads * 4, dtype=torch.int64, device=dev)
    qb = torch.zeros(a.reads * 4, dtype=torch.int64, device=dev)

    def fused():
        assert A.binStatsDevice(B, text.data_ptr(), nbytes, bins.data_ptr(), a.reads, stream=sp) == a.reads

    def two():
        assert A.queryReadsDevice(text.data_ptr(), nbytes, qa.data_ptr(), a.reads, 1, None, sp) == a.reads
        assert B.queryReadsDevice(text.data_ptr(), nbytes, qb.data_ptr(), a.reads, 1, None, sp) == a.reads

    for _ in range(a.warmup):
        fused()
        two()
    torch.cuda.synchronize()
    t_bin, t_two = [], []
    for _ in range(a.reps):
        t_bin.append(once(stream, fused))
        t_two.append(once(stream, two))
    torch.cuda.synchronize()

    s = bins.cpu().numpy().view(np.uint64).reshape(-1, 4)
    sa = qa.cpu().numpy().view(np.uint64).reshape(-1, 4)
    sb = qb.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert int(s[:, 0].sum(dtype=np.uint64)) == kmers
    assert np.array_equal(s[:, 0], sa[:, 0]) and np.array_equal(s[:, 1], sa[:, 1]) and np.array_equal(s[:, 2], sb[:, 1])
    assert (s[:, 3] <= np.minimum(s[:, 1], s[:, 2])).all()

    def side(ts):
        m = float(np.median(ts))
        return {"ms": round(m, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "all_ms": [round(t, 3) for t in ts],
                "windows_per_s": round(kmers / m * 1e3), "text_GB_per_s": round(nbytes / m / 1e6, 1)}

    res = {"k": k, "l_a": a.l, "l_b": a.l - 1, "one_lut": a.b_seed == 1, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers,
           "hits_a": int(s[:, 1].sum(dtype=np.uint64)), "hits_b": int(s[:, 2].sum(dtype=np.uint64)),
           "warmup": a.warmup, "reps": a.reps, "bin": side(t_bin), "two_query": side(t_two),
           "two_query_over_bin": round(float(np.median(t_two)) / float(np.median(t_bin)), 3)}
    print(json.dumps(res))
    A.close()
    B.close()


if __name__ == "__main__":
    main()
