"""Rate of the coverage track against the sequence stats, on the bench's table and bases (one GPU).

The table and the text are those of scripts/seq_rate.py: the bench text is built on the device and counted once, its
sequence lines are written as one wrapped FASTA of --seqs long sequences (the reads back to back), 80 columns.  Each as
the median wall time of --reps calls (every call waits for its stream):
  seq_stats      tsx_hip_seq_stats_device (querySequencesDevice): names, unwrap, line pass, record scan, seq_stats_kernel;
  track_W        tsx_hip_seq_track_device at every window of --windows: the same front, seq_track_kernel in place of
                 seq_stats_kernel, the bin rows back to the host.
The bins of every sequence are checked against its stats row.  A package without tsxcount_amd.track (the parent commit,
named by TSX_TRACK_RATE_PACKAGE) prints seq_stats only.  Kernel times come from a kernel trace of a run of its own.
Prints one JSON line.

    python scripts/track_rate.py [--k 31] [--l 28] [--reads 200000] [--seqs 4] [--reps 5] [--windows 1000,64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TSX_TRACK_RATE_PACKAGE") or ROOT)   # (another checkout's package measures that one)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402


def timed(fn, reps):
    out = fn()   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times], out


def wrap80(seq):
    """seq (uint8 array) as lines of 80 columns."""
    full = len(seq) // 80
    body = np.empty((full, 81), dtype=np.uint8)
    body[:, :80] = seq[:full * 80].reshape(full, 80)
    body[:, 80] = 10
    tail = seq[full * 80:]
    return body.tobytes() + (tail.tobytes() + b"\n" if len(tail) else b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=28)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--seqs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", default="1000,64")
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
    lines = text[:nbytes].cpu().numpy().tobytes().split(b"\n")[1::4]
    del text
    bases = np.frombuffer(b"".join(lines), dtype=np.uint8)
    del lines
    cuts = [len(bases) * i // a.seqs for i in range(a.seqs + 1)]
    wrapped = b"".join(b">contig%d len=%d\n" % (i, cuts[i + 1] - cuts[i]) + wrap80(bases[cuts[i]:cuts[i + 1]]) for i in range(a.seqs))
    nb = len(bases)
    d_wrapped = torch.empty(len(wrapped) + 256, dtype=torch.uint8, device=dev)
    d_wrapped[:len(wrapped)] = torch.frombuffer(bytearray(wrapped), dtype=torch.uint8).to(dev)
    sp = torch.cuda.Stream(dev).cuda_stream

    def rate(ms):
        return {"ms": round(ms, 3), "bases_GB_per_s": round(nb / ms / 1e6, 2)}

    res = {"k": k, "l": a.l, "reads": a.reads, "seqs": a.seqs, "bases": nb, "wrapped_bytes": len(wrapped)}
    ms_s, all_s, (names, st) = timed(lambda: m.querySequencesDevice(d_wrapped.data_ptr(), len(wrapped), 1, None, False, sp), a.reps)
    assert [int(x) for x in st["length"]] == [cuts[i + 1] - cuts[i] for i in range(a.seqs)]
    res["seq_stats"] = dict(rate(ms_s), all_ms=all_s)
    track = getattr(T, "track", None)
    for W in ([int(w) for w in a.windows.split(",")] if track else []):
        ms, all_ms, (tnames, tst, first, bins) = timed(lambda: track.sequence_track_device(m, d_wrapped.data_ptr(), len(wrapped), W, 1, None, sp), a.reps)
        assert tnames == names and tst.tobytes() == st.tobytes()
        assert [int(x) for x in np.diff(first)] == [(int(n) + W - 1) // W for n in st["length"]]
        for i in range(a.seqs):   # the bins of a sequence sum to its stats row
            rows = bins[int(first[i]):int(first[i + 1])]
            for col in ("kmers", "present", "sum_count"):
                assert int(rows[col].sum(dtype=np.uint64)) == int(st[col][i]), (W, i, col)
            assert int(rows["min_count"][rows["kmers"] > 0].min()) == int(st["min_count"][i])
        res["track_%d" % W] = dict(rate(ms), all_ms=all_ms, bins=int(len(bins)), over_seq_stats=round(ms / ms_s, 3))
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
