"""Rate of the table-sizing sketch next to the count it sizes, on the bench's text and table (one GPU).

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed).  Then, in this one process
and alternating, each as the median of --reps timings with a host clock around a call that ends in a synchronise, after
one warm-up round:
  count     tsx_hip_clear (not timed), then tsx_hip_count_fastq_device into the bench's table and tsx_hip_sync;
  sketch    tsx_hip_sketch_device into zeroed registers (2^14) and a synchronise of its stream.
Prints one JSON line -- ms (median), every timing, the spread (max - min) / median, GB/s of text, sketch / count, the
estimate against the exact distinct count the table reports -- and appends it to profiles/estimate_rate.txt.

    python scripts/estimate_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 5]
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


def entry(all_ms, nbytes, **more):
    ms = float(np.median(all_ms))
    d = {"ms": round(ms, 3), "all_ms": [round(t, 3) for t in all_ms], "spread": round((max(all_ms) - min(all_ms)) / ms, 3),
         "text_GB_per_s": round(nbytes / ms / 1e6, 1)}
    d.update(more)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_rate.txt"))
    a = ap.parse_args()
    k, p = a.k, a.precision
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    nbytes, kmers, _ = T.synth_sizes(a.seed, 0, a.reads, k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(a.l, 0, k)
    regs = torch.zeros(1 << p, dtype=torch.int32, device=dev)
    tot = torch.zeros(2, dtype=torch.int64, device=dev)
    tp = text.data_ptr()

    def count():
        m.clear()
        m.sync()
        t0 = time.perf_counter()
        m.countFastqDevice(tp, nbytes)
        m.sync()
        return (time.perf_counter() - t0) * 1e3

    def sketch():
        regs.zero_()
        tot.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.sketchKmersDevice(tp, nbytes, regs.data_ptr(), precision=p, totals_ptr=tot.data_ptr())
        m.sync()
        return (time.perf_counter() - t0) * 1e3

    count(), sketch()   # warm-up: code objects, the partition scratch, the line scratch
    c_all, s_all = [], []
    for _ in range(a.reps):
        c_all.append(count())
        s_all.append(sketch())
    st = m.stats()
    assert st["kmers_added"] == kmers, (st, kmers)
    t = tot.cpu().numpy()
    assert int(t[0]) == kmers and int(t[1]) == a.reads, (t, kmers, a.reads)
    r = regs.cpu().numpy().astype(np.uint8)
    est = T.sketch_estimate(r)
    l = T.suggest_l(est, k)
    c_ms, s_ms = float(np.median(c_all)), float(np.median(s_all))
    res = {
        "k": k, "l": a.l, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers, "reps": a.reps, "precision": p,
        "count": entry(c_all, nbytes, kmers_per_s=round(kmers / c_ms * 1e3)),
        "sketch": entry(s_all, nbytes, kmers_per_s=round(kmers / s_ms * 1e3)),
        "sketch_over_count": round(s_ms / c_ms, 3),
        "distinct": st["distinct"], "estimate": round(est, 1), "estimate_over_distinct": round(est / st["distinct"], 5),
        "suggested_l": l, "load_at_suggested_l": round(st["distinct"] / float(1 << l), 3),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
