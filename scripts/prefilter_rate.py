"""Rate of the two passes of a --min-count=2 count next to the plain count, on the bench's text and table (one GPU), and
the slots the prefilter saves on reads with errors.

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed).  Then, in this one process
and alternating, each as the median of --reps timings with a host clock around a call that ends in a synchronise, after
one warm-up round:
  count_auto / count_atomic   tsx_hip_clear (not timed), then tsx_hip_count_fastq_device into the bench's table on the
                              default path / on the atomic path (tsx_hip_set_path 1), and tsx_hip_sync: the parent's counts;
  pass1                       tsx_hip_prefilter_add_device into zeroed filters of --bits and a synchronise (creating the
                              filters is not timed, and nothing but the call is inside the clock);
  pass2                       the armed count behind pass 1, at --bits and at bits = 12 (saturated: everything admitted).
The second figure: Zipf-template reads (synth.zipf_fastq) with --subst substitutions per base, counted with and without
the prefilter at the default bits (l + 6): occupied slots, and the share of the k-mers seen once that got a slot (exact:
the plain count's histogram gives the singletons).
Prints one JSON line and appends it to profiles/prefilter_rate.txt.

    python scripts/prefilter_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 5] [--bits 36]
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


def entry(all_ms, kmers, **more):
    ms = float(np.median(all_ms))
    d = {"ms": round(ms, 3), "all_ms": [round(t, 3) for t in all_ms], "spread": round((max(all_ms) - min(all_ms)) / ms, 3),
         "G_kmers_per_s": round(kmers / ms / 1e6, 2)}
    d.update(more)
    return d


def reads_with_errors(seed, n_reads, read_len, n_templates, k, subst):
    text = synth.zipf_fastq(seed, n_reads, read_len, n_templates, k)
    lines = text.split(b"\n")
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(1, len(lines), 4):
        s = np.frombuffer(lines[i], dtype=np.uint8).copy()
        hit = np.flatnonzero(rng.random(len(s)) < subst)
        s[hit] = acgt[(np.searchsorted(acgt, s[hit]) + rng.integers(1, 4, len(hit))) & 3]   # another base
        lines[i] = s.tobytes()
    return b"\n".join(lines)


def slots_saved(a):
    k, l = a.k, a.err_l
    text = reads_with_errors(a.seed, a.err_reads, 150, a.err_templates, k, a.subst)
    out = {"reads": a.err_reads, "read_len": 150, "templates": a.err_templates, "subst": a.subst, "l": l}
    m = T.TSXHashMapHIP(l, 0, k)
    m.countFastq(text)
    h = m.getCountHistogram(4)
    st = m.stats()
    out.update(plain_slots=st["distinct"], singletons=int(h[1]), kmers=st["kmers_added"])
    m.clear()
    pst = m.countTwice(text)
    h2 = m.getCountHistogram(4)
    st2 = m.stats()
    assert st2["distinct"] - int(h2[1]) == st["distinct"] - int(h[1]) and int(h2[2]) == int(h[2])   # the contract
    out.update(bits=pst["bits"], filtered_slots=st2["distinct"], singletons_admitted=int(h2[1]),
               share_admitted=round(int(h2[1]) / max(1, int(h[1])), 6), slots_ratio=round(st2["distinct"] / st["distinct"], 4),
               fill_a=round(pst["set_bits_a"] / float(1 << pst["bits"]), 4), fill_b=round(pst["set_bits_b"] / float(1 << (pst["bits"] - 2)), 4))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bits", type=int, default=36)
    ap.add_argument("--err-reads", type=int, default=200000)
    ap.add_argument("--err-templates", type=int, default=1000)
    ap.add_argument("--err-l", type=int, default=26)
    ap.add_argument("--subst", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefilter_rate.txt"))
    a = ap.parse_args()
    k = a.k
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    nbytes, kmers, _ = T.synth_sizes(a.seed, 0, a.reads, k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    torch.cuda.synchronize()
    m = T.TSXHashMapHIP(a.l, 0, k)
    tp = text.data_ptr()

    def count(path, armed=False):
        m.set_path(path)
        m.clear()
        m.sync()
        m.armPrefilter(armed)
        t0 = time.perf_counter()
        m.countFastqDevice(tp, nbytes)
        m.sync()
        dt = (time.perf_counter() - t0) * 1e3
        m.armPrefilter(False)
        return dt

    def pass1(bits):
        m.createPrefilter(bits)
        m.sync()
        t0 = time.perf_counter()
        m.prefilterDevice(tp, nbytes)   # (bits=None: the filter just made; no GPU call but pass 1)
        m.sync()
        return (time.perf_counter() - t0) * 1e3

    names = ("count_auto", "count_atomic", "pass1", "pass2", "pass1_sat", "pass2_sat")

    def one_round():
        r = {"count_auto": count(0), "count_atomic": count(1)}
        r["pass1"] = pass1(a.bits)
        r["pass2"] = count(0, True)
        r["admitted"] = m.prefilter_stats["admitted"]
        r["pass1_sat"] = pass1(12)
        r["pass2_sat"] = count(0, True)
        r["admitted_sat"] = m.prefilter_stats["admitted"]
        return r

    one_round()   # warm-up: code objects, the partition scratch, the line scratch
    rounds = [one_round() for _ in range(a.reps)]
    assert all(r["admitted_sat"] == kmers for r in rounds), (rounds[0], kmers)
    res = {"k": k, "l": a.l, "reads": a.reads, "text_bytes": nbytes, "kmers": kmers, "reps": a.reps, "bits": a.bits,
           "admitted": rounds[-1]["admitted"]}
    for n in names:
        res[n] = entry([r[n] for r in rounds], kmers)
    res["pass2_sat_over_count_atomic"] = round(res["pass2_sat"]["ms"] / res["count_atomic"]["ms"], 3)
    res["pass2_over_count_auto"] = round(res["pass2"]["ms"] / res["count_auto"]["ms"], 3)
    res["two_passes_over_count_auto"] = round((res["pass1"]["ms"] + res["pass2"]["ms"]) / res["count_auto"]["ms"], 3)
    m.close()
    del text
    torch.cuda.empty_cache()
    res["reads_with_errors"] = slots_saved(a)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
