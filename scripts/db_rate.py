"""Rate of the k-mer database paths on the bench's table (one GPU).

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed) and counted once.  Then,
host clock around each call (each returns when its work is done):
  save_null   tsx_hip_save_host to /dev/null: pack on the device + device-to-host copies + write(2) to nothing
  save_file   tsx_hip_save_host to a file in --dir (the file system is reported as the directory's mount)
  load        tsx_hip_load_host of that file into an empty table of the same geometry (direct placement)
  reinsert    the same file into an empty table with another seed (every k-mer through add_kmers_kernel)
The loaded tables are compared with the counted one by stats.  Prints one JSON line.

    python scripts/db_rate.py [--k 31] [--l 30] [--reads 1087000] [--dir /tmp]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime per process, see tests/conftest.py)

import tsxcount_amd as T  # noqa: E402


def mount_of(path):
    path = os.path.realpath(path)
    best, fs = "", "?"
    with open("/proc/mounts") as f:
        for ln in f:
            dev, mnt, typ = ln.split()[:3]
            if (path == mnt or path.startswith(mnt.rstrip("/") + "/")) and len(mnt) > len(best):
                best, fs = mnt, typ
    return best, fs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--no-reinsert", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    nbytes, _, _ = T.synth_sizes(a.seed, 0, a.reads, a.k)
    text = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    T.synth_fastq_device(a.seed, 0, a.reads, a.k, text.data_ptr(), nbytes)
    m = T.TSXHashMapHIP(a.l, 0, a.k)
    m.countFastqDevice(text.data_ptr(), nbytes)
    m.sync()
    del text
    torch.cuda.empty_cache()
    st = m.stats()
    out = {"k": a.k, "l": a.l, "distinct": st["distinct"], "table_bytes": int(m.layout.table_bytes)}

    t0 = time.perf_counter()
    entries, db_bytes = m.saveDatabase("/dev/null")
    out["save_null_s"] = time.perf_counter() - t0
    out["db_bytes"] = db_bytes
    assert entries == st["distinct"]

    path = os.path.join(a.dir, "db_rate.%d.db" % os.getpid())
    out["dir"], out["fs"] = a.dir, "%s (%s)" % mount_of(a.dir)
    try:
        t0 = time.perf_counter()
        m.saveDatabase(path)
        out["save_file_s"] = time.perf_counter() - t0
        key = ("distinct", "count_sum", "kmers_added")
        want = {f: st[f] for f in key}
        m.close()
        torch.cuda.empty_cache()
        m2 = T.TSXHashMapHIP(a.l, 0, a.k)
        t0 = time.perf_counter()
        m2.addDatabase(path)
        out["load_s"] = time.perf_counter() - t0
        assert {f: m2.stats()[f] for f in key} == want
        m2.close()
        if not a.no_reinsert:
            m3 = T.TSXHashMapHIP(a.l, 0, a.k, hash_seed=2)
            t0 = time.perf_counter()
            m3.addDatabase(path)
            out["reinsert_s"] = time.perf_counter() - t0
            out["reinsert_kmers_per_s"] = st["distinct"] / out["reinsert_s"]
            assert {f: m3.stats()[f] for f in key} == want
            m3.close()
    finally:
        if os.path.exists(path):
            os.unlink(path)
    for f in ("save_null", "save_file", "load"):
        if f + "_s" in out:
            out[f + "_GBps"] = db_bytes / out[f + "_s"] / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
