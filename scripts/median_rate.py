"""Rate of the count profile and the read medians on the bench's text and table (one GPU), next to the read query.

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed) and counted once.  Then,
in this one process, each as the median of --reps timings with HIP events on one stream after one warm-up call:
  query     tsx_hip_query_reads_device over the whole text: the yardstick (line pass, lookups, per-record reduction);
  profile   tsx_hip_count_profile_device: line pass, the same lookups, 4 bytes stored per text position;
  medians   tsx_hip_median_reads_device: the profile into scratch of the call (4 bytes per text byte, allocated and
            freed by the call), the line offsets, then the selection (wave form; workgroup form for long records).
medians - profile is what the line offsets, the selection and the call's allocations cost on top of the profile.
Prints one JSON line -- ms (median), every timing, the spread (max - min) / median, GB/s of text, the ratios to the
query -- and appends it to profiles/median_rate.txt.

    python scripts/median_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_rate.txt"))
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

    prof = torch.empty(nbytes, dtype=torch.int32, device=dev)
    p_ms, p_all, _ = timed(stream, lambda: m.countProfileDevice(tp, nbytes, prof.data_ptr(), sp), a.reps)
    stream.synchronize()
    valid = prof != -1   # TSX_HIP_NO_KMER
    assert int(valid.sum()) == kmers
    # (no count of the bench text comes near 2^31: the entries are the counts, and sum to the query's sums)
    assert int(prof[valid].to(torch.int64).sum()) == int(s[:, 3].sum(dtype=np.uint64))
    del prof, valid

    med = torch.zeros(a.reads * 2, dtype=torch.int64, device=dev)
    m_ms, m_all, nrec = timed(stream, lambda: m.medianReadsDevice(tp, nbytes, med.data_ptr(), a.reads, sp), a.reps)
    assert nrec == a.reads
    v = med.cpu().numpy().reshape(-1, 2)
    assert np.array_equal(v[:, 0].astype(np.uint64), s[:, 0])
    # the median lies between the smallest count and the mean of the upper half: min <= median, median * ceil(m / 2) <= sum
    assert (v[:, 1].astype(np.uint64) >= s[:, 2]).all()

    res = {
        "k": k, "l": a.l, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers, "reps": a.reps,
        "query": entry(q_ms, q_all, nbytes),
        "profile": entry(p_ms, p_all, nbytes, profile_bytes=4 * nbytes),
        "medians": entry(m_ms, m_all, nbytes, median_of_medians=int(np.median(v[:, 1]))),
        "profile_over_query": round(p_ms / q_ms, 3),
        "medians_over_query": round(m_ms / q_ms, 3),
        "share_of_medians": {"profile": round(p_ms / m_ms, 3), "lines_select_alloc": round(max(m_ms - p_ms, 0.0) / m_ms, 3)},
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
