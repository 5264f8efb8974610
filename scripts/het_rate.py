"""Rate of the heterozygous pair sweep on the bench's table (one GPU), canonical and not.

The table is the bench's (bench.py's reads and seed, counted on the device).  Warm (one untimed call of each first),
--runs runs each, every value kept, median and spread (max - min) reported, host clock around calls that return when
their work is done:
  het_matrix    tsx_hip_het_histogram_host at --bins x --bins, mode unique: the sweep with three probes a k-mer
  het_list      tsx_hip_het_pairs_device over the whole table into a buffer that holds every pair
  joint_self    m.jointHistogram(m) with TSX_HIP_COMBINE_PATH=1 (the general path): one sweep with one decode, one hash and
                one probe a k-mer -- the one-probe yardstick
  chain         what a user had before: dump the k-mers (tsx_hip_dump_range_device and the copy to the host), make the
                three variants in numpy, send them back, tsx_hip_get_counts_device, fetch the counts.  Timed on the first
                1 / --chain-part of the slots (the whole table's k-mers and variants do not fit the host comfortably);
                chain_whole_table_s is that time multiplied by --chain-part.
Prints one JSON line per table.

    python scripts/het_rate.py [--k 31] [--l 30] [--reads 1087000] [--runs 5] [--bins 1002] [--chain-part 16]
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


def counted(a, dev, canonical):
    nbytes, _, _ = T.synth_sizes(a.seed, 0, a.reads, a.k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, a.k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(a.l, 0, a.k, canonical=canonical)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    del text
    torch.cuda.empty_cache()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bins", type=int, default=1002)
    ap.add_argument("--chain-part", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    vp = ctypes.c_void_p

    def timed(fn):
        fn()   # warm
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    for canonical in (False, True):
        m = counted(a, dev, canonical)
        s0 = m.stats()
        out = {"k": a.k, "l": a.l, "canonical": canonical, "bins": a.bins, "distinct": s0["distinct"], "runs": a.runs}
        res = {}
        out["het_matrix_s"] = timed(lambda: res.__setitem__("het", m.hetHistogram(a.bins, a.bins)))
        mat, st = res["het"]
        out.update(st)
        assert int(mat.sum()) == st["pairs"]
        # the list: room for every pair (and never less than a few records)
        dt = T.het_pair_dtype(a.k)
        words, cap = dt.itemsize // 8, st["pairs"] + 64
        buf = torch.empty(cap * words + 1, dtype=torch.int64, device=dev)
        rule = T.het_rule()
        torch.cuda.synchronize()
        out["het_list_s"] = timed(lambda: T._check(T.lib().tsx_hip_het_pairs_device(
            m.handle, ctypes.byref(rule), 0, int(m.layout.slots), vp(buf.data_ptr()), cap, vp(buf.data_ptr() + cap * words * 8), None)))
        assert int(buf[cap * words].item()) == st["pairs"]
        os.environ["TSX_HIP_COMBINE_PATH"] = "1"
        out["joint_self_s"] = timed(lambda: res.__setitem__("joint", m.jointHistogram(m, a.bins, a.bins)))
        del os.environ["TSX_HIP_COMBINE_PATH"]
        assert int(res["joint"].sum()) == s0["distinct"] == st["kmers_in_range"]

        # the chain on the first 1 / chain_part of the slots
        hi = int(m.layout.slots) // a.chain_part
        cap_k = hi
        d_k = torch.empty(cap_k * m.wk, dtype=torch.int64, device=dev)
        d_c = torch.empty(cap_k, dtype=torch.int64, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        d_v = torch.empty(3 * cap_k * m.wk, dtype=torch.int64, device=dev)
        d_o = torch.empty(3 * cap_k, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        p = (a.k - 1) // 2

        def chain():
            d_n.zero_()
            torch.cuda.synchronize()
            m.dumpRangeDevice(0, hi, d_k.data_ptr(), d_c.data_ptr(), cap_k, d_n.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            n = int(d_n.item())
            kmers = d_k[:n * m.wk].cpu().numpy().view(np.uint64).reshape(n, m.wk)
            counts = d_c[:n].cpu().numpy().view(np.uint64)
            var = np.repeat(kmers[None, :, :], 3, axis=0)
            for d in (1, 2, 3):
                var[d - 1, :, p // 32] ^= np.uint64(d << (2 * (p % 32)))
            d_v[:3 * n * m.wk].copy_(torch.from_numpy(var.reshape(-1).view(np.int64)))
            torch.cuda.synchronize()
            m.getKmerCountsDevice(d_v.data_ptr(), 3 * n, d_o.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            partner = d_o[:3 * n].cpu().numpy().view(np.uint64).reshape(3, n)
            res["chain"] = (n, int(np.count_nonzero(partner)), counts)

        out["chain_s"] = timed(chain)
        out["chain_kmers"], out["chain_partner_hits"] = res["chain"][0], res["chain"][1]
        del d_k, d_c, d_v, d_o
        assert {f: m.stats()[f] for f in s0} == s0
        for f in list(out):
            if f.endswith("_s"):
                v = sorted(out[f])
                out[f[:-2] + "_median_s"] = v[len(v) // 2]
                out[f[:-2] + "_spread_s"] = v[-1] - v[0]
        out["chain_whole_table_s"] = out["chain_median_s"] * a.chain_part
        out["het_matrix_over_joint_self"] = out["het_matrix_median_s"] / out["joint_self_median_s"]
        out["het_list_over_joint_self"] = out["het_list_median_s"] / out["joint_self_median_s"]
        out["chain_over_het_matrix"] = out["chain_whole_table_s"] / out["het_matrix_median_s"]
        out["het_matrix_Gkmers_per_s"] = s0["distinct"] / out["het_matrix_median_s"] / 1e9
        print(json.dumps(out), flush=True)
        m.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
