"""Rate of canonical counting against the default mode on the bench's synthetic text (one GPU).

The text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed); the same text is counted into a
forward table and into a canonical table (tsx_hip_set_canonical), each timed over --steps passes with the library's
stage timing.  The canonical table is then checked: its totals, the poly-A / poly-T pair, and a sample of k-mers of the
first reads against f(x) + f(rc x) of the forward table (f(x) for a palindrome).  Prints one JSON line.

    python scripts/canonical_rate.py [--k 31] [--l 30] [--reads 1087000] [--steps 3] [--warmup 1]
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
from tsxcount_amd import synth  # noqa: E402


def run(m, text, nbytes, steps, warmup):
    def step():
        m.clear()
        m.countFastqDevice(text.data_ptr(), nbytes)
        m.sync()
    for _ in range(warmup):
        step()
    m.set_timing(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    stage, _ = m.get_stage_timing()
    m.set_timing(False)
    return ms, {k: round(v / steps, 3) for k, v in stage.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample-reads", type=int, default=200)
    a = ap.parse_args()
    k = a.k
    torch.zeros(1, device="cuda:0")
    nbytes, kmers, npolya = T.synth_sizes(a.seed, 0, a.reads, k, want_polya=True)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    torch.cuda.synchronize()

    fwd = T.TSXHashMapHIP(a.l, 0, k)
    ms_f, st_f = run(fwd, text, nbytes, a.steps, a.warmup)
    can = T.TSXHashMapHIP(a.l, 0, k, canonical=True)
    ms_c, st_c = run(can, text, nbytes, a.steps, a.warmup)

    # checks
    sf, sc = fwd.stats(), can.stats()
    ok = sc["kmers_added"] == kmers and sc["count_sum"] == kmers and sc["insert_failures"] == 0
    ok = ok and sf["kmers_added"] == kmers and sc["distinct"] <= sf["distinct"]
    polya = int(fwd.getKmerCount("A" * k)) + int(fwd.getKmerCount("T" * k))
    ok = ok and polya >= npolya and int(can.getKmerCount("A" * k)) == polya == int(can.getKmerCount("T" * k))
    reads = [l for l in synth.fastq(a.seed, 0, a.sample_reads).split(b"\n") if l][1::4]
    sample = sorted({r[i:i + k] for r in reads for i in range(0, len(r) - k + 1, 7)})
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rcs = [s[::-1].translate(comp) for s in sample]
    x, y = T.encode_many([s.decode() for s in sample], k), T.encode_many([s.decode() for s in rcs], k)
    fx, fy = fwd.getKmerCounts(x), fwd.getKmerCounts(y)
    want = np.where(np.array([s == r for s, r in zip(sample, rcs)]), fx, fx + fy)
    sample_ok = bool(np.array_equal(can.getKmerCounts(x), want) and np.array_equal(can.getKmerCounts(y), want))
    ok = ok and sample_ok
    print(json.dumps({
        "k": k, "l": a.l, "reads": a.reads, "kmers": kmers,
        "default": {"ms_per_pass": round(ms_f, 3), "kmers_per_s": kmers / ms_f * 1e3, "stages_ms": st_f,
                    "distinct": sf["distinct"]},
        "canonical": {"ms_per_pass": round(ms_c, 3), "kmers_per_s": kmers / ms_c * 1e3, "stages_ms": st_c,
                      "distinct": sc["distinct"]},
        "canonical_over_default": round(ms_c / ms_f, 3),
        "check": {"pass": bool(ok), "polyA_polyT_pair": polya, "sample_kmers": len(sample), "sample_ok": sample_ok},
    }))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
