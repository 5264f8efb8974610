"""Rate of the read trimming on the bench's text and table (one GPU), next to the read query and the read filter.

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed) and counted once.  Then,
in this one process, each as the median of --reps timings with HIP events on one stream after one warm-up call:
  trim_spans   tsx_hip_trim_spans_device over the whole text: line pass, solid bitmap, line offsets, runs, finalize;
  trim_reads   tsx_hip_trim_reads_device with lower = 1 (every window of the counted text is solid: every read is kept
               whole, so the copy moves the whole text): the same, then segment lengths, their scan and the copy into a
               device buffer (the call allocates its scratch and waits twice);
  query        tsx_hip_query_reads_device over the same text;
  filter       tsx_hip_filter_reads_device with the screening rule (every read passes): the yardstick of trim_reads.
Prints one JSON line: ms (median), every timing, the spread (max - min) / median, and GB/s of text.

    python scripts/trim_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 7]
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


def entry(ms, all_ms, nbytes, **more):
    d = {"ms": round(ms, 3), "all_ms": all_ms, "spread": round((max(all_ms) - min(all_ms)) / ms, 3),
         "text_GB_per_s": round(nbytes / ms / 1e6, 1)}
    d.update(more)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=7)
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
    stream = torch.cuda.Stream(dev)   # not torch's default stream: that one does not wait for the map's own
    sp = stream.cuda_stream
    tp = text.data_ptr()

    stats = torch.zeros(a.reads * 4, dtype=torch.int64, device=dev)
    q_ms, q_all, nrec = timed(stream, lambda: m.queryReadsDevice(tp, nbytes, stats.data_ptr(), a.reads, 1, None, sp), a.reps)
    assert nrec == a.reads
    s = stats.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert int(s[:, 0].sum(dtype=np.uint64)) == kmers
    all_solid = bool(np.array_equal(s[:, 0], s[:, 1]))   # every window in range: nothing is cut, the checks below are exact
    bases = int(s[:, 0].sum(dtype=np.uint64)) + a.reads * (k - 1)   # (every read of the bench text is at least k long)
    del stats

    out = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    frule = T.filter_rule(1, None, 1, 0.0, False)
    f_ms, f_all, (kept, fbytes) = timed(stream, lambda: m.filterReadsDevice(tp, nbytes, out.data_ptr(), out.numel(), frule, sp),
                                        a.reps)
    assert kept == a.reads and fbytes == nbytes

    trule = T.trim_rule(1, None, "longest")
    spans = torch.zeros(a.reads * 2, dtype=torch.int64, device=dev)
    s_ms, s_all, nrec = timed(stream, lambda: m.trimSpansDevice(tp, nbytes, spans.data_ptr(), a.reads, trule, sp), a.reps)
    assert nrec == a.reads
    v = spans.cpu().numpy().reshape(-1, 2)
    assert not all_solid or ((v[:, 0] == 0).all() and int(v[:, 1].sum()) == bases)   # every read keeps its whole sequence line

    out.zero_()
    t_ms, t_all, tot = timed(stream, lambda: m.trimReadsDevice(tp, nbytes, out.data_ptr(), out.numel(), trule, sp), a.reps)
    assert tot["records"] == a.reads and tot["bases_in"] == bases and tot["bases_kept"] == int(v[:, 1].sum())
    stream.synchronize()
    if all_solid:   # nothing is cut: the output is the text
        assert tot["kept"] == a.reads and tot["bytes"] == nbytes and torch.equal(out[:nbytes], text[:nbytes])

    res = {
        "k": k, "l": a.l, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers, "reps": a.reps, "all_solid": all_solid,
        "trim_spans": entry(s_ms, s_all, nbytes),
        "trim_reads": entry(t_ms, t_all, nbytes, kept=tot["kept"], bytes=tot["bytes"]),
        "query": entry(q_ms, q_all, nbytes),
        "filter": entry(f_ms, f_all, nbytes, kept=kept, bytes=fbytes),
        "trim_reads_over_filter": round(t_ms / f_ms, 3),
    }
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
