"""Rate of the paired filter and the paired trim (one GPU), next to the two single-end runs they replace.

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed), counted once, and copied
to the host, where its records are dealt out to two mate texts (even records -> mate 1, odd records -> mate 2).  Then, in
this one process, each as the median of --reps wall-clock timings after one warm-up call, every output to /dev/null:
  filter_pairs  tsx_hip_filter_pairs_host over the two texts (both, orphans written, names checked when --names);
  filter_two    tsx_hip_filter_reads_host over mate text 1, then over mate text 2: the single-end code path;
  trim_pairs    tsx_hip_trim_pairs_host over the two texts;
  trim_two      tsx_hip_trim_reads_host over the one, then the other.
All four are host-text entry points: the time holds the upload of the text and the download of the output.
Prints one JSON line: ms (median), every timing, the spread (max - min) / median, GB/s of text, and the two ratios
pairs / two single-end runs.

    python scripts/pair_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 5] [--chunk-bytes 0] [--names]
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


def timed(fn, reps):
    fn()   # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times], out


def entry(ms, all_ms, nbytes, **more):
    d = {"ms": round(ms, 3), "all_ms": all_ms, "spread": round((max(all_ms) - min(all_ms)) / ms, 3),
         "text_GB_per_s": round(nbytes / ms / 1e6, 2)}
    d.update(more)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--names", action="store_true")
    a = ap.parse_args()
    k = a.k
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    nbytes, _, _ = T.synth_sizes(a.seed, 0, a.reads, k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(a.l, 0, k)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    host = bytes(text[:nbytes].cpu().numpy())
    del text
    lines = host.split(b"\n")[:-1]
    assert len(lines) == 4 * a.reads
    pairs = a.reads // 2
    recs = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, 8 * pairs, 4)]
    if a.names:   # the mates of a pair share a name
        recs = [b"@p%d/%d\n" % (i // 2, i % 2 + 1) + r.split(b"\n", 1)[1] for i, r in enumerate(recs)]
    t1, t2 = b"".join(recs[0::2]), b"".join(recs[1::2])
    del lines, recs, host
    both = len(t1) + len(t2)
    null = [os.open(os.devnull, os.O_WRONLY) for _ in range(4)]
    ck = a.chunk_bytes

    def filter_two():
        x = m.filterReads(t1, null[0], lower=1, chunk_bytes=ck)
        y = m.filterReads(t2, null[1], lower=1, chunk_bytes=ck)
        return x[0] + y[0], x[1] + y[1]

    def trim_two():
        x = m.trimReads(t1, null[0], lower=1, chunk_bytes=ck)
        y = m.trimReads(t2, null[1], lower=1, chunk_bytes=ck)
        return {f: x[f] + y[f] for f in x}

    fp_ms, fp_all, fp = timed(lambda: m.filterPairs(t1, t2, null[0], null[1], singles=(null[2], null[3]), lower=1,
                                                    check_names=a.names, chunk_bytes=ck), a.reps)
    f2_ms, f2_all, f2 = timed(filter_two, a.reps)
    tp_ms, tp_all, tp = timed(lambda: m.trimPairs(t1, t2, null[0], null[1], singles=(null[2], null[3]), lower=1,
                                                  check_names=a.names, chunk_bytes=ck), a.reps)
    t2_ms, t2_all, tt = timed(trim_two, a.reps)
    # every window of the counted text is in range: every pair is kept whole, the outputs are the texts
    assert fp["pairs"] == pairs and fp["kept"] == pairs and fp["bytes1"] + fp["bytes2"] == both
    assert f2 == (2 * pairs, both)
    assert tp["pairs"] == pairs and tp["kept"] + tp["single1"] + tp["single2"] <= pairs
    assert tp["bases_in"] == tt["bases_in"] and tp["bases_kept"] == tt["bases_kept"]
    assert tp["bytes1"] + tp["bytes2"] + tp["bytes_single1"] + tp["bytes_single2"] == tt["bytes"]
    res = {
        "k": k, "l": a.l, "pairs": pairs, "text_bytes": both, "reps": a.reps, "chunk_bytes": ck, "names": a.names,
        "filter_pairs": entry(fp_ms, fp_all, both, kept=fp["kept"]),
        "filter_two_single_end": entry(f2_ms, f2_all, both, kept=f2[0]),
        "trim_pairs": entry(tp_ms, tp_all, both, kept=tp["kept"]),
        "trim_two_single_end": entry(t2_ms, t2_all, both, kept=tt["kept"]),
        "filter_pairs_over_two": round(fp_ms / f2_ms, 3),
        "trim_pairs_over_two": round(tp_ms / t2_ms, 3),
    }
    print(json.dumps(res))
    for fd in null:
        os.close(fd)
    m.close()


if __name__ == "__main__":
    main()
