"""Cost of the base rule (tsx_hip_set_base_rule) against the default pass on the bench's synthetic text (one GPU).

The text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed).  Then, with torch on the device
and from the newline positions, its quality bytes are rewritten uniformly over '!'..'J' and 0.1 % of its sequence bases
become N.  The same text is counted with the default rule, acgt_only, min_qual_char='5' and both, each timed over
--steps passes with the library's stage timing; kmers_added of each is checked against a count of the valid windows
made on the device.  Prints one JSON line.

    python scripts/base_rule_rate.py [--k 31] [--l 30] [--reads 1087000] [--steps 3] [--warmup 1] [--low-share P]
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

RULES = [("default", False, None), ("acgt_only", True, None), ("min_qual_5", False, "5"), ("both", True, "5")]


def span_mask(n, lo, hi, dev):
    """bool[n]: True inside the spans [lo[i], hi[i])."""
    d = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    d.index_add_(0, lo, torch.ones_like(lo, dtype=torch.int32))
    d.index_add_(0, hi, -torch.ones_like(hi, dtype=torch.int32))
    return torch.cumsum(d, 0, dtype=torch.int32)[:n] > 0


def prepare(text, nbytes, k, seed, low_share=None, chunk_records=1 << 16):
    """Rewrites qualities and injects N in place; returns the valid-window count of every rule."""
    dev = text.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nl = torch.nonzero(text[:nbytes] == 10).flatten()
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), nl[:-1] + 1])
    R = nl.numel() // 4          # (the synthetic text: no empty lines, every record terminated)
    valid = {name: 0 for name, _, _ in RULES}
    for c0 in range(0, R, chunk_records):
        c1 = min(R, c0 + chunk_records)
        lo, hi = int(starts[4 * c0]), int(nl[4 * c1 - 1]) + 1
        seg = text[lo:hi]
        n = hi - lo
        s0, s1 = starts[4 * c0 + 1:4 * c1:4] - lo, nl[4 * c0 + 1:4 * c1:4] - lo
        q0, q1 = starts[4 * c0 + 3:4 * c1:4] - lo, nl[4 * c0 + 3:4 * c1:4] - lo
        in_seq, in_qual = span_mask(n, s0, s1, dev), span_mask(n, q0, q1, dev)
        rq = torch.randint(33, 75, (n,), dtype=torch.uint8, device=dev, generator=g)
        if low_share is not None:   # that share below '5', the rest '5' .. 'J'
            lo_q = torch.randint(33, 53, (n,), dtype=torch.uint8, device=dev, generator=g)
            hi_q = torch.randint(53, 75, (n,), dtype=torch.uint8, device=dev, generator=g)
            rq = torch.where(torch.rand(n, device=dev, generator=g) < low_share, lo_q, hi_q)
        seg.copy_(torch.where(in_qual, rq, seg))
        to_n = in_seq & (torch.rand(n, device=dev, generator=g) < 0.001)
        seg.masked_fill_(to_n, ord("N"))
        # quality of each sequence byte: the byte at the same offset of the record's quality line (or none)
        disp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        disp.index_add_(0, s0, q0 - s0)
        disp.index_add_(0, s1, -(q0 - s0))
        disp = torch.cumsum(disp, 0)[:n]
        at = torch.arange(n, device=dev) + disp
        qlen = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        qlen.index_add_(0, s0, q1 - q0)
        qlen.index_add_(0, s1, -(q1 - q0))
        rel = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rel.index_add_(0, s0, s0)
        rel.index_add_(0, s1, -s0)
        off = torch.arange(n, device=dev) - torch.cumsum(rel, 0)[:n]   # offset of a sequence byte in its line
        has_q = off < torch.cumsum(qlen, 0)[:n]
        low = in_seq & (~has_q | (seg[at.clamp(0, n - 1)] < ord("5")))
        u = seg | 0x20
        nonacgt = in_seq & ~((u == ord("a")) | (u == ord("c")) | (u == ord("g")) | (u == ord("t")))
        for name, acgt, mq in RULES:
            bad = ~in_seq
            if acgt:
                bad = bad | nonacgt
            if mq:
                bad = bad | low
            cs = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), torch.cumsum(bad.int(), 0, dtype=torch.int32)])
            valid[name] += int(((cs[k:] - cs[:-k]) == 0).sum()) if n >= k else 0
    return valid


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
    ap.add_argument("--low-share", type=float, default=None,
                    help="quality bytes below '5' with this probability (default: uniform over '!'..'J', where almost no "
                         "window of 31 keeps every base at '5' or above)")
    a = ap.parse_args()
    k = a.k
    torch.zeros(1, device="cuda:0")
    nbytes, kmers = T.synth_sizes(a.seed, 0, a.reads, k)[:2]
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, k, text.data_ptr(), nbytes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    valid = prepare(text, nbytes, k, a.seed, a.low_share)
    prep_s = time.perf_counter() - t0

    out = {"k": k, "l": a.l, "reads": a.reads, "low_share": a.low_share, "text_bytes": nbytes, "kmers_synth": kmers, "prepare_s": round(prep_s, 2)}
    ok = valid["default"] == kmers
    m = T.TSXHashMapHIP(a.l, 0, k)
    base = None
    for name, acgt, mq in RULES:
        m.set_base_rule(acgt, mq)
        ms, st = run(m, text, nbytes, a.steps, a.warmup)
        added = m.stats()["kmers_added"]
        good = added == valid[name]
        ok = ok and good
        base = ms if base is None else base
        out[name] = {"ms_per_pass": round(ms, 3), "over_default": round(ms / base, 3), "kmers_added": added,
                     "valid_windows": valid[name], "ok": bool(good), "stages_ms": st}
    m.close()
    out["pass"] = bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
