"""Table sizing without a GPU: the symbols, the sketch definition worked by hand, the numpy model against the C host
functions, the estimator and its accuracy, the suggest_l table, the refusals of the entry points and of the CLI -- and
the model that tests/test_sketch.py compares the GPU with.

The model (model_sketch) is the window rule of test_base_rule (records, windows) over a text, the kept k-mers encoded
with encode_np, and tsxcount_amd.sketch_registers, which is numpy alone.  Never the GPU path under test."""
import ctypes
import math
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

from test_base_rule import _CODE, ROOT, encode_np, oracle, records, windows
from test_read_query import EDGE_FASTQ, run_cli

NEW_SYMBOLS = ("tsx_hip_sketch_host", "tsx_hip_sketch_bgzf_host", "tsx_hip_sketch_device", "tsx_hip_sketch_kmers_host",
               "tsx_hip_sketch_estimate_host", "tsx_hip_suggest_l")
M64 = (1 << 64) - 1
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)


def sigma5(p):
    """Five standard errors of a sketch of 2^p registers: the margin of suggest_l and the bound of the accuracy tests."""
    return 5 * 1.04 / math.sqrt(1 << p)


def kept_kmers(text, k, lpr=4, acgt_only=False, min_qual=None):
    """Counter of the coded k-mers the counting calls would count: test_base_rule.oracle for any lines per record."""
    kept = Counter()
    for seq, qual, _ in records(text, lpr):
        s = seq.translate(_CODE)
        for i, ok in windows(seq, qual, k, acgt_only, min_qual):
            if ok:
                kept[s[i:i + k]] += 1
    return kept


def model_sketch(text, k, lpr=4, acgt_only=False, min_qual=None, canonical=False, precision=14):
    """(registers, {kmers, records}, distinct) of a text by the model."""
    import tsxcount_amd as T
    kept = kept_kmers(text, k, lpr, acgt_only, min_qual)
    enc = encode_np(sorted(kept), k)
    if canonical and len(enc):
        enc = np.unique(T.canonical(enc, k).reshape(-1, T.key_limbs(k)), axis=0)
    regs = T.sketch_registers(enc, k, precision)
    return regs, {"kmers": sum(kept.values()), "records": len(records(text, lpr))}, len(enc)


def estimate_py(registers):
    """The estimate of tsx_hip_sketch_estimate_host, the same operations in the same order."""
    r = np.asarray(registers, dtype=np.uint8)
    m = len(r)
    p = m.bit_length() - 1
    hist = np.bincount(r, minlength=66)
    total = 0.0
    for rank in range(0, 64 - p + 2):
        total += float(hist[rank]) * math.ldexp(1.0, -rank)
    e = (0.7213 / (1.0 + 1.079 / m)) * m * m / total
    if e <= 2.5 * m and hist[0] > 0:
        e = m * math.log(m / float(hist[0]))
    return e


def c_registers(T, kmers, k, p, regs=None):
    a = np.ascontiguousarray(kmers, dtype=np.uint64)
    out = np.zeros(1 << p, dtype=np.uint8) if regs is None else regs
    n = a.size // T.key_limbs(k)
    assert T.lib().tsx_hip_sketch_kmers_host(k, a.ctypes.data_as(U64P), n, p, out.ctypes.data_as(U8P)) == T.OK
    return out


def random_kmers(k, n, seed):
    wk = (2 * k + 63) // 64
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(n, wk), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, wk), dtype=np.uint64)
    if (2 * k) % 64:
        a[:, wk - 1] &= np.uint64((1 << ((2 * k) % 64)) - 1)
    return a


def test_sketch_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b(int|double) %s\(" % name, hdr), name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tsxcount_amd", "lib", "libtsxcount_hip.so")],
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name
    for words in ("tsx_hip_sketch_totals", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0.7213", "1.079",
                  "2.5 m", "TSX_HIP_BGZF_BATCH", "TSX_HIP_DEV_WINDOW", "TSX_HIP_PIECE_BYTES"):
        assert words in hdr, words
    assert ctypes.sizeof(T.SketchTotals) == 16
    for name in ("sketchKmers", "sketchKmersBgzf", "sketchKmersDevice", "sizedFor"):
        assert callable(getattr(T.TSXHashMapHIP, name)), name
    for name in ("sketch_registers", "sketch_estimate", "suggest_l", "merge_sketches"):
        assert callable(getattr(T, name)), name


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_the_sketch_of_a_text_worked_by_hand():
    import tsxcount_amd as T
    k = 5
    # k-mer, its limb (base i in bits 2i, 2i + 1; A C G T = 0 1 2 3), v = mix64(0x9E3779B97F4A7C15 ^ limb), and at
    # p = 14: idx = the top 14 bits of v, rank = 1 + the leading zeros of the 50 bits below them
    hand = [(b"ACGTA", 228, 0x08400FCC2FFA9314, 528, 7),      # 0000 1000 0100 00|00 0000 1111 ...: six zeros, rank 7
            (b"AAAAA", 0, 0xE220A8397B1DCDAF, 14472, 3),      # 1110 0010 0010 00|00 1010 ...: two zeros, rank 3
            (b"TTGCA", 111, 0xD1024A5FAD64D717, 13376, 1)]    # 1101 0001 0000 00|10 ...: none, rank 1
    for s, limb, v, idx, rank in hand:
        assert int(T.encode(s.decode(), k)[0]) == limb
        assert mix64(0x9E3779B97F4A7C15 ^ limb) == v
        assert v >> 50 == idx
        rest = v & ((1 << 50) - 1)
        assert 50 - rest.bit_length() + 1 == rank
    want = np.zeros(1 << 14, dtype=np.uint8)
    for _, _, _, idx, rank in hand:
        want[idx] = rank
    # ACGTA twice (AAAAA and TTGCA once each) in two records; a line shorter than k; the '+' and quality lines are no k-mers
    text = b"@a\nACGTA\n+\nIIIII\n@b\nAAAAA\n+\nIIIII\n@c\nTTGCA\n+\nIIIII\n@d\nACGTA\n+\nIIIII\n@e\nACGT\n+\nIIII\n"
    regs, tot, distinct = model_sketch(text, k)
    assert np.array_equal(regs, want) and tot == {"kmers": 4, "records": 5} and distinct == 3
    assert np.array_equal(T.sketch_registers(np.array([[228], [0], [111], [228]], dtype=np.uint64), k), want)
    # p = 10 of ACGTA: the top 10 bits 0000 1000 01 = 33, then 00 0000 0000 1111 ...: ten zeros, rank 11
    r10 = T.sketch_registers(np.array([228], dtype=np.uint64), k, precision=10)
    assert np.flatnonzero(r10).tolist() == [33] and r10[33] == 11
    # a hash whose low 64 - p bits are all zero has the highest rank, 64 - p + 1 (the model's formula at rest = 0)
    assert 50 - (0).bit_length() + 1 == 51
    # bits above 2k are not part of the k-mer
    assert np.array_equal(T.sketch_registers(np.array([228 | (1 << 10)], dtype=np.uint64), k), T.sketch_registers(np.array([228], dtype=np.uint64), k))
    with pytest.raises(ValueError):
        T.sketch_registers(np.array([228], dtype=np.uint64), k, precision=15)
    with pytest.raises(ValueError):
        T.sketch_registers(np.array([228], dtype=np.uint64), k, precision=9)
    # the model's window rule is test_base_rule.oracle's at four lines per record
    for rule in ((False, None), (True, None), (False, "5"), (True, "5")):
        assert kept_kmers(EDGE_FASTQ, 7, 4, *rule) == oracle(EDGE_FASTQ, 7, *rule)[0]


@pytest.mark.parametrize("k", [5, 31, 32, 33, 64, 96, 127])
@pytest.mark.parametrize("p", [10, 14])
def test_host_registers_equal_the_model(k, p):
    import tsxcount_amd as T
    a = random_kmers(k, 2000, 100 * k + p)
    want = T.sketch_registers(a, k, p)
    assert want.dtype == np.uint8 and want.shape == (1 << p,) and want.max() <= 64 - p + 1 and np.count_nonzero(want) > 500   # (k = 5: 1024 k-mers in all)
    got = c_registers(T, a, k, p)
    assert np.array_equal(got, want)
    # in two halves into one array: max-combined; and merge_sketches of the halves
    acc = c_registers(T, a[:700], k, p)
    assert np.array_equal(c_registers(T, a[700:], k, p, acc), want)
    assert np.array_equal(T.merge_sketches(T.sketch_registers(a[:700], k, p), T.sketch_registers(a[700:], k, p)), want)


def test_estimate_equals_the_python_formula():
    import tsxcount_amd as T
    for p in (10, 14):
        m = 1 << p
        zero = np.zeros(m, dtype=np.uint8)
        assert T.sketch_estimate(zero) == 0.0 and estimate_py(zero) == 0.0
        full = np.full(m, 64 - p + 1, dtype=np.uint8)           # saturated: every register at its highest rank
        e = T.sketch_estimate(full)
        assert math.isfinite(e) and e > 2.0 ** 60 and abs(e / estimate_py(full) - 1) <= 1e-12
        branches = set()
        for n in (1, 10, m // 8, 2 * m, 3 * m, 40 * m):
            regs = T.sketch_registers(random_kmers(31, n, n + p), 31, p)
            want = estimate_py(regs)
            assert abs(T.sketch_estimate(regs) / want - 1) <= 1e-12, (p, n)
            raw = (0.7213 / (1.0 + 1.079 / m)) * m * m / sum(2.0 ** -int(x) for x in regs)
            branches.add("linear" if raw <= 2.5 * m and (regs == 0).any() else "raw")
            assert abs(want / n - 1) < 0.25, (p, n, want)
        assert branches == {"linear", "raw"}
    L = T.lib()
    bad = np.zeros(1 << 10, dtype=np.uint8)
    bad[3] = 56                                                 # above 64 - 10 + 1
    assert L.tsx_hip_sketch_estimate_host(bad.ctypes.data_as(U8P), 10) < 0
    assert L.tsx_hip_sketch_estimate_host(None, 14) < 0
    for p in (9, 15, 0, -1):
        assert L.tsx_hip_sketch_estimate_host(bad.ctypes.data_as(U8P), p) < 0
    with pytest.raises(ValueError):
        T.sketch_estimate(np.zeros(1000, dtype=np.uint8))
    with pytest.raises(T.TSXException):
        T.sketch_estimate(bad)


@pytest.mark.parametrize("p,n", [(14, 3000), (14, 45000), (14, 200000), (10, 3000), (10, 200000)])
def test_model_accuracy_within_five_sigma(p, n):
    """n distinct random 62-bit values (numpy seed 7): |E / n - 1| <= 5 * 1.04 / sqrt(2^p).  45 000 at p = 14 sits on
    the classic estimator's bias bump just above the switch to linear counting (2.5 m = 40 960)."""
    import tsxcount_amd as T
    rng = np.random.default_rng(7)
    v = np.unique(rng.integers(0, 1 << 62, size=n + n // 8, dtype=np.uint64))
    rng.shuffle(v)
    v = v[:n]
    assert len(np.unique(v)) == n
    e = T.sketch_estimate(T.sketch_registers(v, 31, p))
    print("p=%d n=%d E/n-1=%+.4f bound=%.4f" % (p, n, e / n - 1, sigma5(p)))
    assert abs(e / n - 1) <= sigma5(p)


def test_suggest_l_table():
    import tsxcount_amd as T
    margin = 1 + sigma5(14)                                      # 1.040625
    # exact powers of two: need = 2^20 gives 20, one more k-mer's worth gives 21
    d20 = (1 << 20) * 0.75 / margin
    assert T.suggest_l(d20 * (1 - 1e-9), 31) == 20 and T.suggest_l(d20 * (1 + 1e-9), 31) == 21
    assert T.suggest_l((1 << 20) * 0.5 / margin * (1 - 1e-9), 31, load=0.5) == 20
    # the margin tips a value over: 786 000 / 0.75 = 1 048 000 < 2^20 fits l = 20 without it, not with it
    assert 786000 / 0.75 < 1 << 20 < 786000 * margin / 0.75 and T.suggest_l(786000, 31) == 21
    assert T.suggest_l(786000, 31, precision=10) == 21 and T.suggest_l(700000, 31, precision=10) == 21   # p = 10: a wider margin
    assert T.suggest_l(700000, 31) == 20
    # the lower bound
    assert T.suggest_l(0, 31) == 4 and T.suggest_l(3, 31) == 4 and T.suggest_l(11, 31) == 4 and T.suggest_l(12, 31) == 5
    # the upper bounds: 2k - 1 (k = 14: 27; k = 3: 5) and 36
    assert T.suggest_l(0.9 * (1 << 27) * 0.75 / margin, 14) == 27
    assert T.suggest_l(100e6, 14) == 27                          # clamped from 28: load 0.745, still within 0.9
    for k, d, l in ((14, 130e6, 27), (3, 1000, 5), (40, 70e9, 36)):
        with pytest.raises(T.TSXException) as ei:
            T.suggest_l(d, k)
        assert ei.value.code == T.ERANGE and ei.value.l == l
    assert T.suggest_l(20, 3) == 5 and T.suggest_l(28, 3) == 5   # (28 / 32 = 0.875)
    assert T.suggest_l(60e9, 40) == 36
    # load_ppm 0 is 750000; above 900000 is refused; the other arguments
    L = T.lib()
    l0, l1 = ctypes.c_int(-1), ctypes.c_int(-1)
    for d in (1000.0, 786000.0, 5e8):
        assert L.tsx_hip_suggest_l(31, d, 14, 0, ctypes.byref(l0)) == T.OK
        assert L.tsx_hip_suggest_l(31, d, 14, 750000, ctypes.byref(l1)) == T.OK and l0.value == l1.value
    assert L.tsx_hip_suggest_l(31, 1000.0, 14, 900000, ctypes.byref(l0)) == T.OK
    assert L.tsx_hip_suggest_l(14, 130e6, 14, 0, ctypes.byref(l0)) == T.ERANGE and l0.value == 27
    for args in ((31, 1000.0, 14, 900001), (31, 1000.0, 9, 0), (31, 1000.0, 15, 0), (0, 1000.0, 14, 0), (128, 1000.0, 14, 0),
                 (31, -1.0, 14, 0), (31, float("nan"), 14, 0), (31, float("inf"), 14, 0)):
        assert L.tsx_hip_suggest_l(*args, ctypes.byref(l0)) == T.EINVAL, args
    assert L.tsx_hip_suggest_l(31, 1000.0, 14, 0, None) == T.EINVAL
    with pytest.raises(T.TSXException):
        T.suggest_l(1000, 31, load=0.95)


def test_sketch_entry_points_refuse_bad_arguments_without_a_gpu():
    import tsxcount_amd as T
    L = T.lib()
    vp = ctypes.c_void_p
    text = b"@a\nACGTACGT\n+\nIIIIIIII\n"
    regs = np.zeros(1 << 14, dtype=np.uint8)
    rp = regs.ctypes.data_as(U8P)
    tot = T.SketchTotals()
    fake = vp(0x1000)                                            # a map that is never looked at: the other checks come first
    # a null map, null registers, a bad precision, a null text with bytes
    assert L.tsx_hip_sketch_host(None, text, len(text), 14, rp, ctypes.byref(tot), 0) == T.EINVAL
    assert L.tsx_hip_sketch_host(fake, text, len(text), 14, None, ctypes.byref(tot), 0) == T.EINVAL
    assert L.tsx_hip_sketch_host(fake, None, 5, 14, rp, None, 0) == T.EINVAL
    assert L.tsx_hip_sketch_bgzf_host(None, text, len(text), 14, rp, None) == T.EINVAL
    assert L.tsx_hip_sketch_bgzf_host(fake, text, len(text), 14, None, None) == T.EINVAL
    assert L.tsx_hip_sketch_bgzf_host(fake, None, 5, 14, rp, None) == T.EINVAL
    assert L.tsx_hip_sketch_device(None, vp(0x2000), 16, 14, vp(0x3000), None, None) == T.EINVAL
    assert L.tsx_hip_sketch_device(fake, vp(0x2000), 16, 14, None, None, None) == T.EINVAL
    assert L.tsx_hip_sketch_device(fake, None, 16, 14, vp(0x3000), None, None) == T.EINVAL
    assert L.tsx_hip_sketch_device(fake, vp(0x2008), 16, 14, vp(0x3000), None, None) == T.EINVAL   # not 16-byte aligned
    for p in (9, 15, 0, -3, 64):
        assert L.tsx_hip_sketch_host(fake, text, len(text), p, rp, None, 0) == T.EINVAL, p
        assert L.tsx_hip_sketch_bgzf_host(fake, text, len(text), p, rp, None) == T.EINVAL, p
        assert L.tsx_hip_sketch_device(fake, vp(0x2000), 16, p, vp(0x3000), None, None) == T.EINVAL, p
        assert L.tsx_hip_sketch_kmers_host(31, regs.ctypes.data_as(U64P), 1, p, rp) == T.EINVAL, p
    one = np.zeros(4, dtype=np.uint64)
    assert L.tsx_hip_sketch_kmers_host(31, one.ctypes.data_as(U64P), 1, 14, None) == T.EINVAL
    assert L.tsx_hip_sketch_kmers_host(31, None, 1, 14, rp) == T.EINVAL
    assert L.tsx_hip_sketch_kmers_host(0, one.ctypes.data_as(U64P), 1, 14, rp) == T.EINVAL
    assert L.tsx_hip_sketch_kmers_host(128, one.ctypes.data_as(U64P), 1, 14, rp) == T.EINVAL
    assert L.tsx_hip_sketch_kmers_host(31, None, 0, 14, rp) == T.OK                # nothing to add
    assert not regs.any() and tot.kmers == 0 and tot.records == 0
    # Python: the checks come before the map is touched
    m = T.TSXHashMapHIP.__new__(T.TSXHashMapHIP)
    for call in (lambda: m.sketchKmers(text, precision=15), lambda: m.sketchKmersBgzf(text, precision=9),
                 lambda: m.sketchKmers(text, registers=np.zeros(1 << 10, dtype=np.uint8)),
                 lambda: T.TSXHashMapHIP.sizedFor(text, 31, lines=3), lambda: T.merge_sketches(regs, regs[:1024])):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(T.merge_sketches([1, 0, 7], [0, 2, 3]), [1, 2, 7])


def test_cli_usage_errors_of_the_sizing_options(tmp_path):
    code, _, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--l=L|auto", "--load-factor=F", "--estimate"):
        assert flag in err, flag
    db = tmp_path / "x.db"
    for opt, base in (("--l=auto", ("--input=x.fastq", "--k=15", "--l=auto")), ("--estimate", ("--input=x.fastq", "--k=15", "--estimate"))):
        code, out, err = run_cli(*base, "--gpus=2", timeout=30)
        assert code == 1 and "Usage" in err and opt in err and "one GPU" in err and out == ""
        code, _, err = run_cli(*base, "--load=" + str(db), timeout=30)
        assert code == 1 and "Usage" in err and opt in err and "--load" in err
        code, _, err = run_cli(*base, "--with=" + str(db), "--compare", timeout=30)
        assert code == 1 and "Usage" in err and opt in err and "--with" in err
        code, _, err = run_cli(*base, "--format=fasta-wrapped", timeout=30)
        assert code == 1 and "Usage" in err and opt in err and "wrapped" in err
        for f in ("0", "0.95", "-1"):
            code, _, err = run_cli(*base, "--load-factor=" + f, timeout=30)
            assert code == 1 and "--load-factor" in err, f
    code, out, err = run_cli("--input=x.fastq", "--estimate", timeout=30)
    assert code == 1 and "Usage" in err and "--estimate needs --k" in err and out == ""
    code, _, err = run_cli("--k=15", "--l=auto", timeout=30)
    assert code == 1 and "--l=auto needs --input" in err
