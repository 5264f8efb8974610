"""Rate of the read queries on the bench's text and table (one GPU).

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed) and counted once.  Then,
each as the median of --reps timings with HIP events on one stream:
  query        tsx_hip_query_reads_device over the whole text (stats of every read; the call waits for its stream);
  filter       tsx_hip_filter_reads_device over the whole text with the screening rule (at least one k-mer in the table:
               every read passes, so the compaction moves the whole text): record scan, stats, kept lengths, their scan
               and the compaction into a device buffer (the call allocates its scratch and waits twice);
  get_counts   tsx_hip_get_counts_device over the table's dumped k-mers: one lookup per distinct k-mer, the in-repo
               baseline for random lookups.
Rates are per k-mer looked up (query, filter: every window of the text; get_counts: every distinct k-mer) and per byte
of text.  Prints one JSON line.

    python scripts/query_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 5]
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


def timed(stream, fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 3) for t in times], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    k = a.k
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    nbytes, kmers, _ = T.synth_sizes(a.seed, 0, a.reads, k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(a.l, 0, k)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    st = m.stats()
    stream = torch.cuda.Stream(dev)   # not torch's default stream: that one does not wait for the map's own
    sp = stream.cuda_stream

    stats = torch.zeros(a.reads * 4, dtype=torch.int64, device=dev)
    q_ms, q_all, nrec = timed(stream, lambda: m.queryReadsDevice(text.data_ptr(), nbytes, stats.data_ptr(), a.reads, 2, None, sp),
                              a.reps)
    assert nrec == a.reads
    s = stats.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert int(s[:, 0].sum(dtype=np.uint64)) == kmers == st["kmers_added"]
    del stats

    out = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    rule = T.filter_rule(1, None, 1, 0.0, False)
    f_ms, f_all, (kept, fbytes) = timed(stream, lambda: m.filterReadsDevice(text.data_ptr(), nbytes, out.data_ptr(), out.numel(),
                                                                           rule, sp), a.reps)
    assert kept == a.reads and fbytes == nbytes
    del out, text
    torch.cuda.empty_cache()

    # baseline: one lookup per distinct k-mer of the table (its dump), through tsx_hip_get_counts_device
    d = st["distinct"]
    wk = T.key_limbs(k)
    dk = torch.empty(d * wk, dtype=torch.int64, device=dev)
    dc = torch.empty(d, dtype=torch.int64, device=dev)
    dn = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    import ctypes
    L, vp = T.lib(), ctypes.c_void_p
    assert L.tsx_hip_dump_device(m.handle, vp(dk.data_ptr()), vp(dc.data_ptr()), d, vp(dn.data_ptr()), vp(sp)) == T.OK
    stream.synchronize()
    assert int(dn.item()) == d
    got = torch.empty(d, dtype=torch.int64, device=dev)

    def lookups():
        m.getKmerCountsDevice(dk.data_ptr(), d, got.data_ptr(), sp)
    g_ms, g_all, _ = timed(stream, lookups, a.reps)
    stream.synchronize()
    assert torch.equal(got, dc)

    res = {
        "k": k, "l": a.l, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers, "distinct": d,
        "query": {"ms": round(q_ms, 3), "all_ms": q_all, "lookups_per_s": round(kmers / q_ms * 1e3),
                  "ns_per_kmer": round(q_ms * 1e6 / kmers, 4), "text_GB_per_s": round(nbytes / q_ms / 1e6, 1)},
        "filter": {"ms": round(f_ms, 3), "all_ms": f_all, "kept": kept, "bytes": fbytes,
                   "lookups_per_s": round(kmers / f_ms * 1e3), "text_GB_per_s": round(nbytes / f_ms / 1e6, 1)},
        "get_counts": {"ms": round(g_ms, 3), "all_ms": g_all, "lookups_per_s": round(d / g_ms * 1e3),
                       "ns_per_kmer": round(g_ms * 1e6 / d, 4), "kmer_GB_per_s": round(d * wk * 8 / g_ms / 1e6, 1)},
    }
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
