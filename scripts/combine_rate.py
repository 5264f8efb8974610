"""Rate of the table set operations on the bench's table (one GPU).

A is the bench's table (bench.py's reads and seed, counted on the device), B the table of as many reads that share
half their read range with A's, OUT an empty table.  INTERSECT / MIN, host clock around single calls (each returns
when its work is done), --runs runs each, every value kept:
  baseline       what existing entry points give: tsx_hip_dump_range_device of A in chunks -> tsx_hip_get_counts_device
                 on B -> torch minimum + compaction -> tsx_hip_add_kmers_device into OUT
  general        tsx_hip_combine, TSX_HIP_COMBINE_PATH=1
  aligned        tsx_hip_combine, TSX_HIP_COMBINE_PATH=2 (OUT of A's geometry: nothing staged)
  aligned_staged the aligned join into an OUT with another seed (survivors staged as k-mers)
  *_stats        out == NULL on either path
The results are compared by stats.  Prints one JSON line.

    python scripts/combine_rate.py [--k 31] [--l 30] [--reads 1087000] [--runs 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def baseline(A, B, OUT, chunk_slots, bufs, stream):
    kmers, counts, cb, n = bufs
    slots = int(A.layout.slots)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        for lo in range(0, slots, chunk_slots):
            hi = min(slots, lo + chunk_slots)
            A.dumpRangeDevice(lo, hi, kmers.data_ptr(), counts.data_ptr(), hi - lo, n.data_ptr(), s)
            got = int(n.item())
            if not got:
                continue
            B.getKmerCountsDevice(kmers.data_ptr(), got, cb.data_ptr(), s)
            keep = cb[:got] > 0
            kk = kmers[:got][keep].contiguous()
            cc = torch.minimum(counts[:got][keep], cb[:got][keep]).contiguous()
            if kk.shape[0]:
                T._check(T.lib().tsx_hip_add_kmers_device(OUT.handle, kk.data_ptr(), cc.data_ptr(), kk.shape[0], s))
            stream.synchronize()   # (kk and cc are freed on return to the loop)
    OUT.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk-slots", type=int, default=1 << 24)
    a = ap.parse_args()
    assert a.k <= 32, "the baseline's torch arithmetic is for one-limb k-mers"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    A = counted(a, 0, dev)
    B = counted(a, a.reads // 2, dev)
    sa, sb = A.stats(), B.stats()
    out = {"k": a.k, "l": a.l, "a_distinct": sa["distinct"], "b_distinct": sb["distinct"], "runs": a.runs}
    OUT = T.TSXHashMapHIP(a.l, 0, a.k)
    OUT2 = T.TSXHashMapHIP(a.l, 0, a.k, hash_seed=2)
    rule = T.combine_rule("intersect", "min")

    def timed(fn, target):
        ts = []
        for _ in range(a.runs):
            if target is not None:
                target.clear()
                target.sync()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    cs = min(a.chunk_slots, int(A.layout.slots))
    bufs = (torch.empty(cs, dtype=torch.int64, device=dev), torch.empty(cs, dtype=torch.int64, device=dev),
            torch.empty(cs, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    stream = torch.cuda.Stream(dev)
    out["baseline_s"] = timed(lambda: baseline(A, B, OUT, cs, bufs, stream), OUT)
    key = ("distinct", "count_sum", "kmers_added")
    want = {f: OUT.stats()[f] for f in key}
    out["out_distinct"] = want["distinct"]
    del bufs
    torch.cuda.empty_cache()

    for name, path, target in (("general", "1", OUT), ("aligned", "2", OUT), ("aligned_staged", "2", OUT2)):
        os.environ["TSX_HIP_COMBINE_PATH"] = path
        out[name + "_s"] = timed(lambda: A._combine(B, rule, target), target)
        assert {f: target.stats()[f] for f in key} == want, name
    for name, path in (("general_stats", "1"), ("aligned_stats", "2")):
        os.environ["TSX_HIP_COMBINE_PATH"] = path
        res = []
        out[name + "_s"] = timed(lambda: res.append(A._combine(B, rule, None)), None)
        assert res[-1]["out_entries"] == want["distinct"] and res[-1]["out_count_sum"] == want["count_sum"], name
    del os.environ["TSX_HIP_COMBINE_PATH"]
    assert {f: A.stats()[f] for f in sa} == sa and {f: B.stats()[f] for f in sb} == sb
    for f in list(out):
        if f.endswith("_s"):
            out[f[:-2] + "_median_Gkmers_per_s"] = sa["distinct"] / sorted(out[f])[len(out[f]) // 2] / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
