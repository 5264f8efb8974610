"""Rate of the read correction on the bench's text (one GPU), next to the trim spans that run the same bitmap pass.

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed) and counted once: the
table of the CLEAN text.  Then --rate (1 %) of the bases of its sequence lines are substituted on the device (torch, a
fixed seed) and, in this one process, each as the median of --reps timings with HIP events on one stream after one
warm-up call:
  trim_spans      tsx_hip_trim_spans_device over the erroneous text: line pass, solid bitmap, line offsets, runs;
  correct_sites   tsx_hip_correct_sites_device: line pass, solid bitmap, line offsets, site pass, probe pass;
  correct_reads   tsx_hip_correct_reads_device into a second buffer: the same, then the copy and the apply.
Prints one JSON line: ms (median), every timing, the spread (max - min) / median, GB/s of text, the totals, and how many
planted bases came back.  The split by pass is the kernel statistics of this script under a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/correct_rate.py

    python scripts/correct_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 3] [--rate 0.01]
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
from tsxcount_amd import correct as C  # noqa: E402


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


def plant(text, nbytes, rate, seed):
    """Substitutes `rate` of the ACGT bytes of the sequence lines (line 1 of every four) in place; returns how many."""
    t = text[:nbytes]
    nl = (t == 10)
    line = torch.cumsum(nl, 0, dtype=torch.int64) - nl.to(torch.int64)   # index of the line a byte lies in
    g = torch.Generator(device=t.device)
    g.manual_seed(seed)
    hit = ((line & 3) == 1) & ~nl & (torch.rand(nbytes, device=t.device, generator=g) < rate)
    del line, nl
    idx = hit.nonzero().squeeze(1)
    del hit
    old = t[idx]
    lut = torch.zeros(256, dtype=torch.uint8, device=t.device)
    for a, b in zip(b"ACGT", b"CGTA"):
        lut[a] = b
    new = lut[old.to(torch.int64)]
    keep = new != 0                     # (the bench text holds ACGT only; anything else stays)
    t[idx[keep]] = new[keep]
    return int(keep.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rate", type=float, default=0.01)
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
    clean = text[:nbytes].clone()
    planted = plant(text, nbytes, a.rate, a.seed)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)   # not torch's default stream: that one does not wait for the map's own
    sp = stream.cuda_stream
    tp = text.data_ptr()

    trule = T.trim_rule(1, None, "longest")
    spans = torch.zeros(a.reads * 2, dtype=torch.int64, device=dev)
    s_ms, s_all, nrec = timed(stream, lambda: m.trimSpansDevice(tp, nbytes, spans.data_ptr(), a.reads, trule, sp), a.reps)
    assert nrec == a.reads
    del spans

    cap = planted + 1024
    corr = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
    c_ms, c_all, (nc, ctot) = timed(stream, lambda: C.correction_sites_device(m, tp, nbytes, corr.data_ptr(), cap, 1, None, 1, sp),
                                    a.reps)
    assert ctot["records"] == a.reads and nc == ctot["corrected"] and ctot["sites"] == nc + ctot["ambiguous"] + ctot["unfixable"]
    del corr

    out = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    r_ms, r_all, rtot = timed(stream, lambda: C.correct_reads_device(m, tp, nbytes, out.data_ptr(), 1, None, 1, sp), a.reps)
    stream.synchronize()
    assert rtot == dict(ctot, bytes=nbytes)
    changed = int((out[:nbytes] != text[:nbytes]).sum().item())
    restored = changed - int(((out[:nbytes] != text[:nbytes]) & (out[:nbytes] != clean)).sum().item())
    left = int((out[:nbytes] != clean).sum().item())
    assert changed == nc

    res = {
        "k": k, "l": a.l, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers, "reps": a.reps, "rate": a.rate,
        "planted": planted, "totals": rtot, "restored": restored, "miscorrected": changed - restored, "bases_still_wrong": left,
        "trim_spans": entry(s_ms, s_all, nbytes),
        "correct_sites": entry(c_ms, c_all, nbytes),
        "correct_reads": entry(r_ms, r_all, nbytes),
        "correct_sites_over_trim_spans": round(c_ms / s_ms, 3),
    }
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
