"""Rate of counting wrapped FASTA against the two-line path on the same sequences (one GPU).

About --bases random ACGT bases in --records records, built on the device twice: as 60-column wrapped text with headers
(countFastaDevice: the lines are joined on the device, then counted) and pre-joined as two-line records (countFastqDevice
with 2 lines per record, the yardstick: this path is what the join feeds).  Both texts are resident; each is counted over
--steps timed passes (clear, count, sync) behind --warmup untimed ones.  The join's cost is taken from the library's
stage timing: the events of a pass cover the line pass, the scan and the build, so what the wrapped pass spends outside
them, less what the two-line pass spends outside them (clear, launch gaps), is the pre-pass.  Prints one JSON line and
writes it, with a short reading, to --out (default profiles/fasta_wrapped_rate.txt).

    python scripts/fasta_wrap_rate.py [--k 31] [--l 31] [--bases 1000000020] [--records 33] [--steps 3] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402


def build_texts(bases, records, width, dev):
    """(wrapped text, two-line text, bases per record) as uint8 tensors on the device; every record has the same length, a
    multiple of the line width."""
    per = bases // records // width * width
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    wrapped, joined = [], []
    nl = torch.tensor([10], dtype=torch.uint8, device=dev)
    for r in range(records):
        seq = acgt[torch.randint(0, 4, (per,), device=dev)]
        head = torch.tensor(list(b">chr%d random sequence\n" % r), dtype=torch.uint8, device=dev)
        lines = torch.cat([seq.view(-1, width), nl.expand(per // width, 1)], dim=1).reshape(-1)
        wrapped += [head, lines]
        joined += [torch.tensor(list(b">\n"), dtype=torch.uint8, device=dev), seq, nl]
    pad = torch.full((256,), 10, dtype=torch.uint8, device=dev)
    w, j = torch.cat(wrapped), torch.cat(joined)
    return torch.cat([w, pad]), w.numel(), torch.cat([j, pad]), j.numel(), per


def run(m, count, steps, warmup):
    def step():
        m.clear()
        count()
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
    ap.add_argument("--l", type=int, default=31)
    ap.add_argument("--bases", type=int, default=1000000020)
    ap.add_argument("--records", type=int, default=33)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_wrapped_rate.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(20261017)
    wtext, wbytes, jtext, jbytes, per = build_texts(a.bases, a.records, a.width, dev)
    torch.cuda.synchronize()
    kmers = a.records * max(0, per - a.k + 1)

    m = T.TSXHashMapHIP(a.l, 0, a.k)
    m.set_record_lines(2)
    ms_j, st_j = run(m, lambda: m.countFastqDevice(jtext.data_ptr(), jbytes), a.steps, a.warmup)
    sj = m.stats()
    ms_w, st_w = run(m, lambda: m.countFastaDevice(wtext.data_ptr(), wbytes), a.steps, a.warmup)
    sw = m.stats()
    m.close()
    ok = sj["kmers_added"] == kmers == sw["kmers_added"] and sj["distinct"] == sw["distinct"] and sw["insert_failures"] == 0
    in_j, in_w = sum(st_j.values()), sum(st_w.values())
    pre = max(0.0, (ms_w - in_w) - (ms_j - in_j))
    res = {
        "k": a.k, "l": a.l, "records": a.records, "bases_per_record": per, "line_width": a.width, "kmers": kmers,
        "wrapped_bytes": wbytes, "two_line_bytes": jbytes, "steps": a.steps, "warmup": a.warmup,
        "two_line": {"ms_per_pass": round(ms_j, 3), "kmers_per_s": kmers / ms_j * 1e3, "stages_ms": st_j},
        "wrapped": {"ms_per_pass": round(ms_w, 3), "kmers_per_s": kmers / ms_w * 1e3, "stages_ms": st_w},
        "wrapped_over_two_line": round(ms_w / ms_j, 3),
        "prepass_ms": round(pre, 3), "prepass_share_of_kernel_time": round(pre / (pre + in_w), 3) if pre + in_w else None,
        "prepass_traffic_GBps": round((2 * wbytes + jbytes) / pre / 1e6, 1) if pre else None,
        "check": {"pass": bool(ok), "distinct": sw["distinct"]},
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("scripts/fasta_wrap_rate.py: wrapped FASTA (lines joined on the device) against the two-line path, same sequences\n")
        f.write("two-line  %.3f ms per pass, %.3e k-mers/s\n" % (ms_j, kmers / ms_j * 1e3))
        f.write("wrapped   %.3f ms per pass, %.3e k-mers/s\n" % (ms_w, kmers / ms_w * 1e3))
        f.write("ratio     %.3f (wrapped over two-line)\n" % (ms_w / ms_j))
        f.write("pre-pass  %.3f ms per pass (outside the timed stages, less the two-line pass's share outside them): %s of kernel time\n"
                % (pre, res["prepass_share_of_kernel_time"]))
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
