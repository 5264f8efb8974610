"""Rate of digital normalization on the bench's synthetic text (one GPU), next to the two things it is made of.

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's seed) and repeated --copies times, so
that the coverage of every k-mer exceeds the cutoff and the later copies are dropped.  Then, in this one process, each
as the median of --reps wall-clock timings (the calls wait for the stream themselves) after one warm-up call, every
counting call on a table cleared and zeroed outside the timing:
  count      tsx_hip_count_fastq_device on the atomic path (set_path(1)): every k-mer inserted;
  medians    tsx_hip_median_reads_device against the filled table: every k-mer looked up, every record selected;
  normalize  tsx_hip_normalize_device at R = 65536 and R = 4096.
The yardstick for a normalization that sees S k-mers and adds A of them is  medians + count * A / S.
Prints one JSON line -- ms (median), every timing, the spread (max - min) / median, k-mers/s, the share of tiles the
record gate skipped, the ratio to the yardstick -- and appends it to profiles/normalize_rate.txt.

    python scripts/normalize_rate.py [--k 31] [--l 28] [--reads 250000] [--copies 6] [--cutoff 4] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402


def timed(fn, reps, before=None):
    out = None
    times = []
    for i in range(reps + 1):   # the first is the warm-up
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times], out


def entry(ms, all_ms, kmers, **more):
    d = {"ms": round(ms, 3), "all_ms": all_ms, "spread": round((max(all_ms) - min(all_ms)) / ms, 3),
         "Gkmers_per_s": round(kmers / ms / 1e6, 3)}
    d.update(more)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=28)
    ap.add_argument("--reads", type=int, default=250000)
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--cutoff", type=int, default=4)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_rate.txt"))
    a = ap.parse_args()
    k = a.k
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    one, kmers1, _ = T.synth_sizes(a.seed, 0, a.reads, k)
    part = torch.empty(one + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, part.data_ptr(), one)
    nbytes, kmers, nrec = one * a.copies, kmers1 * a.copies, a.reads * a.copies
    text = torch.full((nbytes + 256,), 10, dtype=torch.uint8, device=dev)
    text[:nbytes] = part[:one].repeat(a.copies)
    del part
    tp = text.data_ptr()
    m = T.TSXHashMapHIP(a.l, 0, k)
    m.set_path(1)

    def fresh():
        m.clear()
        m.stats()   # (zeroes the table now, outside the timing)

    c_ms, c_all, _ = timed(lambda: (m.countFastqDevice(tp, nbytes), m.sync()), a.reps, fresh)
    assert m.stats()["kmers_added"] == kmers
    med = torch.zeros(nrec * 2, dtype=torch.int64, device=dev)
    m_ms, m_all, got = timed(lambda: m.medianReadsDevice(tp, nbytes, med.data_ptr(), nrec), a.reps)
    assert got == nrec
    del med

    res = {"k": k, "l": a.l, "reads": a.reads, "copies": a.copies, "cutoff": a.cutoff, "text_bytes": nbytes, "kmers": kmers,
           "reps": a.reps, "count_atomic": entry(c_ms, c_all, kmers), "medians": entry(m_ms, m_all, kmers)}
    keep = torch.zeros(nrec, dtype=torch.uint8, device=dev)
    dbg = (ctypes.c_uint64 * 8)()
    m._lib.tsx_hip_debug_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    for R in (65536, 4096):
        n_ms, n_all, tot = timed(lambda: m.normalizeReadsDevice(tp, nbytes, keep.data_ptr(), nrec, cutoff=a.cutoff, round_records=R),
                                 a.reps, fresh)
        m.sync()
        assert tot["records"] == nrec and tot["kmers_seen"] == kmers and int(keep.sum()) == tot["kept"]
        assert m.stats()["kmers_added"] == tot["kmers_added"]
        m._lib.tsx_hip_debug_counters(m.handle, dbg)
        yard = m_ms + c_ms * tot["kmers_added"] / kmers
        res["normalize_R%d" % R] = entry(n_ms, n_all, kmers, totals=tot, tiles=int(dbg[3]), tiles_skipped=int(dbg[4]),
                                         skipped_share=round(dbg[4] / max(1, dbg[3]), 3), yardstick_ms=round(yard, 3),
                                         over_yardstick=round(n_ms / yard, 3))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
