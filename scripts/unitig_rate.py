"""Rate of the unitig calls (one GPU) on read sets where the walks matter, per stage.

The bench's own table is random k-mers, nearly all isolated, and says nothing about walks.  The workloads here:
  (a) the canonical count of error-free reads at --coverage from a random genome of --genome bases at k = 31: few, very long
      unitigs -- the worst case for one lane per chain;
  (b) the same reads with --error substitutions per base, at lower = 1 and lower = 2: many short unitigs.
Reads are made on the device with torch (uniform starts, forward strand, 150 bases) and counted with countFastqDevice.
Warm (one untimed call first), --runs runs each, every value kept, the median reported.  Per workload:
  stats_s     tsx_hip_unitig_stats (degree sweep, walk of the starts, cycle pass), host clock
  unitigs_s   tsx_hip_unitigs_device into buffers that hold the result (the same plus the spelling walk)
  degree_ms, walk_ms, spell_ms, cycle_ms   the stages of the median unitigs_device call (tsx_hip_unitig_last_timing)
  het_s       m.hetHistogram(1002, 1002) on the same table: a sweep with three probes a slot where the degree sweep has
              eight -- a yardstick, not a bar
  nodes_per_s nodes / unitigs_s;  longest and longest_walk_ns_per_step = walk_ms / k-mers of the longest unitig (in (a) the
              walk stage IS the longest walk: every other lane has long finished)
--only a / b runs one workload.  --single is for (a) at a large genome, where one walk takes minutes: ONE cold
tsx_hip_unitigs_device call into buffers sized from the table's distinct count (room for 65536 unitigs), no warm-up, no
stats call (stats_s is then the sum of its three stages inside that call) -- a single value, no spread.
Prints one JSON line per workload and writes the table to --out (appends with --append).

    python scripts/unitig_rate.py [--genome 50000000] [--coverage 30] [--error 0.01] [--runs 3] [--only a|b] [--single]
                                  [--out profiles/unitig_rate.txt] [--append]
"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402
from tsxcount_amd import unitig as U  # noqa: E402

READ = 150


def reads_text(genome, n_reads, error, gen, dev):
    """A FASTQ text on the device: n_reads reads of READ bases from uniform starts, each base replaced by another one
    with probability `error`; four lines a record, each record READ * 2 + 7 bytes."""
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    rec = 2 * READ + 7                       # "@r\n" seq "\n+\n" qual "\n"
    text = torch.empty(n_reads * rec, dtype=torch.uint8, device=dev).view(n_reads, rec)
    text[:, 0], text[:, 1], text[:, 2] = ord("@"), ord("r"), 10
    text[:, 3 + READ], text[:, 4 + READ], text[:, 5 + READ] = 10, ord("+"), 10
    text[:, 6 + READ:6 + 2 * READ] = ord("I")
    text[:, 6 + 2 * READ] = 10
    step = 1 << 20
    for a in range(0, n_reads, step):        # in pieces: the index tensor of all reads at once is 8 bytes a base
        b = min(n_reads, a + step)
        starts = torch.randint(0, genome.numel() - READ + 1, (b - a,), generator=gen, device=dev)
        codes = genome[starts[:, None] + torch.arange(READ, device=dev)[None, :]]
        if error > 0:
            hit = torch.rand(codes.shape, generator=gen, device=dev) < error
            codes = torch.where(hit, (codes + torch.randint(1, 4, codes.shape, generator=gen, device=dev).to(torch.uint8)) & 3, codes)
        text[a:b, 3:3 + READ] = acgt[codes.long()]
    return text.view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_rate.txt"))
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    t_start = time.perf_counter()

    def heartbeat():   # a walk of minutes says nothing by itself
        while True:
            time.sleep(60)
            print("# %.0f s" % (time.perf_counter() - t_start), flush=True)
    threading.Thread(target=heartbeat, daemon=True).start()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    genome = torch.randint(0, 4, (a.genome,), generator=gen, device=dev, dtype=torch.uint8)
    n_reads = int(a.genome * a.coverage / READ)
    rows = []

    def median(fn):
        fn()   # warm
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2], ts

    for name, error, lowers in (("a_error_free", 0.0, (1,)), ("b_errors", a.error, (1, 2))):
        if a.only and not name.startswith(a.only):
            continue
        text = reads_text(genome, n_reads, error, gen, dev)
        torch.cuda.synchronize()
        distinct_guess = a.genome + int(n_reads * READ * error * a.k)
        l = max(20, (2 * distinct_guess - 1).bit_length())       # load at most a half
        m = T.TSXHashMapHIP(l, 0, a.k, canonical=True)
        m.countFastqDevice(text.data_ptr(), text.numel())
        m.sync()
        del text
        torch.cuda.empty_cache()
        het_s, _ = median(lambda: m.hetHistogram(1002, 1002))
        for lower in lowers:
            out = {"workload": name, "lower": lower, "k": a.k, "l": l, "genome": a.genome, "reads": n_reads, "error": error,
                   "distinct": m.stats()["distinct"], "runs": 1 if a.single else a.runs, "het_s": het_s}
            if a.single:
                cap_r = 1 << 16
                cap_s = out["distinct"] + cap_r * (a.k - 1)
                seq = torch.empty(cap_s + 64, dtype=torch.uint8, device=dev)
                rec = torch.empty(cap_r * 5, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, tot = U.unitigs_device(m, seq.data_ptr(), cap_s, rec.data_ptr(), cap_r, lower)
                out["unitigs_s"] = time.perf_counter() - t0
                ms = (ctypes.c_double * 4)()
                T._check(T.lib().tsx_hip_unitig_last_timing(ms))
                out["degree_ms"], out["walk_ms"], out["spell_ms"], out["cycle_ms"] = list(ms)
                out["stats_s"] = (ms[0] + ms[1] + ms[3]) / 1e3
                out.update({f: tot[f] for f in ("nodes", "unitigs", "circular", "bases", "longest", "isolated", "tips", "branching")})
                out["nodes_per_s"] = tot["nodes"] / out["unitigs_s"]
                out["longest_walk_ns_per_step"] = out["walk_ms"] * 1e6 / max(1, tot["longest"] - a.k + 1)
                out["degree_over_het"] = out["degree_ms"] / 1e3 / het_s
                print(json.dumps(out), flush=True)
                rows.append(out)
                del seq, rec
                torch.cuda.empty_cache()
                continue
            res = {}
            out["stats_s"], _ = median(lambda: res.__setitem__("tot", U.unitig_stats(m, lower)))
            tot = res["tot"]
            seq = torch.empty(tot["bases"] + 64, dtype=torch.uint8, device=dev)
            rec = torch.empty((tot["unitigs"] + 1) * 5, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            stages = []

            def full():
                assert U.unitigs_device(m, seq.data_ptr(), tot["bases"], rec.data_ptr(), tot["unitigs"], lower)[2] == tot
                ms = (ctypes.c_double * 4)()
                T._check(T.lib().tsx_hip_unitig_last_timing(ms))
                stages.append(list(ms))
            out["unitigs_s"], ts = median(full)
            pick = stages[1:][ts.index(out["unitigs_s"])]
            out["degree_ms"], out["walk_ms"], out["spell_ms"], out["cycle_ms"] = pick
            out.update({f: tot[f] for f in ("nodes", "unitigs", "circular", "bases", "longest", "isolated", "tips", "branching")})
            out["nodes_per_s"] = tot["nodes"] / out["unitigs_s"]
            out["longest_walk_ns_per_step"] = out["walk_ms"] * 1e6 / max(1, tot["longest"] - a.k + 1)
            out["degree_over_het"] = out["degree_ms"] / 1e3 / het_s
            print(json.dumps(out), flush=True)
            rows.append(out)
            del seq, rec
            torch.cuda.empty_cache()
        m.close()
        torch.cuda.empty_cache()

    cols = ("workload", "lower", "l", "nodes", "unitigs", "longest", "degree_ms", "walk_ms", "spell_ms", "cycle_ms", "stats_s",
            "unitigs_s", "het_s", "nodes_per_s", "longest_walk_ns_per_step")
    with open(a.out, "a" if a.append else "w") as f:
        f.write("unitig calls on one MI355X, k = %d, canonical, genome %d bases, %d reads of %d bases (%gx), %s\n"
                % (a.k, a.genome, n_reads, READ, a.coverage,
                   "ONE cold call, no warm-up" if a.single else "median of %d warm runs" % a.runs))
        f.write("\t".join(cols) + "\n")
        for r in rows:
            f.write("\t".join(("%.4g" % r[c]) if isinstance(r[c], float) else str(r[c]) for c in cols) + "\n")


if __name__ == "__main__":
    main()
