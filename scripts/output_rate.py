"""Rate of the count output paths on the bench's table (one GPU).

The bench text is built on the device (tsx_hip_synth_fastq_device, bench.py's reads and seed) and counted once.  Then:
  histogram  tsx_hip_histogram_device over the whole table, HIP events around each call (--reps calls);
  format     tsx_hip_format_counts_device over the whole table, chunk by chunk into one device buffer of --chunk-mib,
             HIP events around the whole walk;
  write      tsx_hip_write_counts_host to /dev/null (device text -> pinned host buffers -> write(2)), host clock around
             the call (it returns when everything is written).
Bytes are what each pass must move: the histogram reads word 0 of every slot and the secondary array once; the format
pass reads the table and writes the text (the secondary probes of the counted slots are not included); the write moves
the text to the host.  Shares are of the 8 TB/s HBM peak.  Prints one JSON line.

    python scripts/output_rate.py [--k 31] [--l 30] [--reads 1087000] [--reps 5] [--chunk-mib 256]
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

PEAK_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--l", type=int, default=30)
    ap.add_argument("--reads", type=int, default=1087000)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nbins", type=int, default=10002)
    ap.add_argument("--chunk-mib", type=int, default=256)
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
    del text
    torch.cuda.empty_cache()
    st = m.stats()
    lay = m.layout
    L, vp = T.lib(), ctypes.c_void_p
    stream = torch.cuda.Stream(dev)   # not torch's default stream: that one does not wait for the map's own
    sp = vp(stream.cuda_stream)

    # histogram
    hist = torch.empty(a.nbins, dtype=torch.int64, device=dev)
    def hist_once():
        rc = L.tsx_hip_histogram_device(m.handle, 0, int(lay.slots), a.nbins, vp(hist.data_ptr()), sp)
        assert rc == T.OK, rc
    hist_once()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        hist_once()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    stream.synchronize()
    h = hist.cpu().numpy().view(np.uint64)
    assert int(h.sum()) == st["distinct"], (int(h.sum()), st["distinct"])
    sec_slots = 1 << int(lay.overflow_l)
    hist_bytes = int(lay.slots) * 8 + sec_slots * 8 + st["overflow_used"] * 16
    hist_ms = float(np.median(times))

    # format, chunk by chunk into one device buffer
    chunk = a.chunk_mib << 20
    per = chunk // (k + 22)
    tbuf = torch.empty(chunk, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    def format_all():
        text_bytes = lines = 0
        for lo in range(0, int(lay.slots), per):
            hi = min(int(lay.slots), lo + per)
            rc = L.tsx_hip_format_counts_device(m.handle, lo, hi, 1, 2 ** 64 - 1, vp(tbuf.data_ptr()), chunk,
                                                vp(cnt.data_ptr()), vp(cnt.data_ptr() + 8), sp)
            assert rc == T.OK, rc
            nb, nl = (int(x) for x in cnt.cpu())
            text_bytes += nb
            lines += nl
        return text_bytes, lines
    format_all()
    ftimes = []
    for _ in range(max(1, a.reps // 2)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        text_bytes, lines = format_all()
        e1.record(stream)
        e1.synchronize()
        ftimes.append(e0.elapsed_time(e1))
    assert lines == st["distinct"], (lines, st["distinct"])
    fmt_ms = float(np.median(ftimes))
    fmt_bytes = int(lay.table_bytes) + text_bytes
    del tbuf

    # write to /dev/null
    fd = os.open(os.devnull, os.O_WRONLY)
    wl, wb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    t0 = time.perf_counter()
    rc = L.tsx_hip_write_counts_host(m.handle, fd, 1, 2 ** 64 - 1, 0, ctypes.byref(wl), ctypes.byref(wb))
    write_s = time.perf_counter() - t0
    os.close(fd)
    assert rc == T.OK and wl.value == st["distinct"] and wb.value == text_bytes, (rc, wl.value, wb.value)

    out = {
        "k": k, "l": a.l, "reads": a.reads, "distinct": st["distinct"], "text_bytes": text_bytes,
        "histogram": {"ms": round(hist_ms, 3), "all_ms": [round(t, 3) for t in times], "nbins": a.nbins, "bytes": hist_bytes,
                      "TB_per_s": round(hist_bytes / hist_ms / 1e9, 2), "peak_share": round(hist_bytes / hist_ms / 1e9 / (PEAK_BPS / 1e12), 3)},
        "format": {"ms": round(fmt_ms, 3), "chunk_MiB": a.chunk_mib, "chunks": -(-int(lay.slots) // per), "bytes": fmt_bytes,
                   "TB_per_s": round(fmt_bytes / fmt_ms / 1e9, 2), "peak_share": round(fmt_bytes / fmt_ms / 1e9 / (PEAK_BPS / 1e12), 3),
                   "lines_per_s": round(lines / fmt_ms * 1e3)},
        "write_devnull": {"s": round(write_s, 3), "GB_per_s": round(text_bytes / write_s / 1e9, 2)},
    }
    print(json.dumps(out))
    m.close()


if __name__ == "__main__":
    main()
