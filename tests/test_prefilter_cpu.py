"""The prefilter without a GPU: the symbols, the numpy definition (tsxcount_amd.prefilter_masks) against the C host function
(tsx_hip_prefilter_mask_host), the shape of masks and word indexes, a pure-Python model of both passes, the refusals of
the entry points and of the CLI -- and the model that tests/test_prefilter.py compares the GPU with."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from test_base_rule import ROOT
from test_read_query import run_cli
from test_sketch_cpu import mix64, random_kmers

NEW_SYMBOLS = ("tsx_hip_prefilter_bits", "tsx_hip_prefilter_create", "tsx_hip_prefilter_free", "tsx_hip_prefilter_add_host", "tsx_hip_prefilter_add_bgzf_host",
               "tsx_hip_prefilter_add_device", "tsx_hip_prefilter_arm", "tsx_hip_prefilter_armed", "tsx_hip_prefilter_stats",
               "tsx_hip_prefilter_read", "tsx_hip_prefilter_mask_host")
M64 = (1 << 64) - 1
U64P = ctypes.POINTER(ctypes.c_uint64)


def masks_py(limbs, bits):
    """(word_a, word_b, mask) of one k-mer given as Python ints, limb 0 first: the definition in plain integers."""
    v = 0x9E3779B97F4A7C15
    for x in limbs:
        v = mix64(v ^ x)
    mask = 0
    for s in (0, 6, 12, 18):
        mask |= 1 << ((v >> s) & 63)
    return v >> (64 - (bits - 6)), v >> (64 - (bits - 8)), mask


def c_masks(T, kmers, k, bits):
    a = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, T.key_limbs(k))
    out = np.zeros((3, len(a)), dtype=np.uint64)
    wa, wb, mk = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    for i, row in enumerate(a):
        row = np.ascontiguousarray(row)
        assert T.lib().tsx_hip_prefilter_mask_host(k, row.ctypes.data_as(U64P), bits, ctypes.byref(wa), ctypes.byref(wb),
                                                   ctypes.byref(mk)) == T.OK
        out[:, i] = (wa.value, wb.value, mk.value)
    return out[0], out[1], out[2]


def model_filters(T, enc_counts, k, bits):
    """(A, B-lower, B-upper) as numpy uint64 word arrays for distinct encoded k-mers `enc` with their counts: A = the OR of
    every mask; B-lower = the OR of the masks of the k-mers seen twice (what B must hold); B-upper = A's masks folded into
    B's words (no bit of B may lie outside it)."""
    enc, counts = enc_counts
    wa, wb, mk = T.prefilter_masks(enc, k, bits)
    A = np.zeros(1 << (bits - 6), dtype=np.uint64)
    lo = np.zeros(1 << (bits - 8), dtype=np.uint64)
    hi = np.zeros(1 << (bits - 8), dtype=np.uint64)
    np.bitwise_or.at(A, wa.astype(np.int64), mk)
    np.bitwise_or.at(hi, wb.astype(np.int64), mk)
    twice = np.asarray(counts) >= 2
    np.bitwise_or.at(lo, wb[twice].astype(np.int64), mk[twice])
    return A, lo, hi


def test_prefilter_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tsxcount_amd", "lib", "libtsxcount_hip.so")],
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name
    assert "} tsx_hip_prefilter_totals;" in hdr
    assert ctypes.sizeof(T.PrefilterTotals) == 56
    for name in ("prefilter", "prefilterBgzf", "prefilterDevice", "armPrefilter", "prefilterWords", "countTwice", "createPrefilter"):
        assert callable(getattr(T.TSXHashMapHIP, name)), name
    assert isinstance(T.TSXHashMapHIP.prefilter_stats, property) and callable(T.prefilter_masks)


@pytest.mark.parametrize("k", [15, 31, 33, 64, 127])
@pytest.mark.parametrize("bits", [12, 20, 38])
def test_numpy_definition_equals_the_c_function(k, bits):
    import tsxcount_amd as T
    wk = T.key_limbs(k)
    a = random_kmers(k, 300, 1000 * k + bits)
    top = (1 << ((2 * k) % 64)) - 1 if (2 * k) % 64 else M64
    edge = np.zeros((4, wk), dtype=np.uint64)
    edge[1, 0] = 1                                               # the lowest bit of the k-mer
    edge[2, wk - 1] = np.uint64(top ^ (top >> 1))                # the highest
    edge[3, :] = np.uint64(M64)
    edge[3, wk - 1] = np.uint64(top)                             # all of them (poly-T)
    a = np.concatenate([edge, a])
    wa, wb, mk = T.prefilter_masks(a, k, bits)
    ca, cb, cm = c_masks(T, a, k, bits)
    assert np.array_equal(wa, ca) and np.array_equal(wb, cb) and np.array_equal(mk, cm)
    for i in (0, 1, 2, 3, 4, 100):
        assert (int(wa[i]), int(wb[i]), int(mk[i])) == masks_py([int(x) for x in a[i]], bits), i
    # one to four bits; the word of B is the word of A without its two low bits; both inside their filters
    pop = np.array([bin(int(x)).count("1") for x in mk])
    assert pop.min() >= 1 and pop.max() <= 4 and (pop == 4).sum() > 200
    assert np.array_equal(wb, wa >> np.uint64(2))
    assert int(wa.max()) < 1 << (bits - 6) and int(wb.max()) < 1 << (bits - 8)
    # the mask does not depend on bits, the words are prefixes of one another
    w20, _, m20 = T.prefilter_masks(a, k, 20)
    assert np.array_equal(m20, mk)
    if bits >= 20:
        assert np.array_equal(wa >> np.uint64(bits - 20), w20)
    # bits above 2k are not part of the k-mer (C and numpy)
    if (2 * k) % 64:
        dirty = a.copy()
        dirty[:, wk - 1] |= np.uint64(1 << ((2 * k) % 64))
        assert np.array_equal(T.prefilter_masks(dirty, k, bits)[2], mk) and np.array_equal(c_masks(T, dirty[:8], k, bits)[2], mk[:8])


def test_masks_may_coincide():
    """The four bit numbers of a mask may coincide: among the 2^22 smallest 15-mers some masks have three bits, some two
    and a few one (about 2^22 * 63 * 62 * 6 / 64^3, 2^22 * 63 * 7 / 64^3 and 2^22 / 64^3 = 16 of them), and numpy, the
    plain-integer definition and the C function agree on them."""
    import tsxcount_amd as T
    k, bits = 15, 20
    a = np.arange(1 << 22, dtype=np.uint64)
    wa, wb, mk = T.prefilter_masks(a, k, bits)
    pop = np.zeros(len(a), dtype=np.int64)
    m = mk.copy()
    while m.any():
        pop += (m & np.uint64(1)).astype(np.int64)
        m >>= np.uint64(1)
    assert pop.min() == 1 and pop.max() == 4
    for n in (1, 2, 3):
        idx = np.flatnonzero(pop == n)[:5]
        assert len(idx) >= 2, n
        ca, cb, cm = c_masks(T, a[idx], k, bits)
        assert np.array_equal(cm, mk[idx]) and np.array_equal(ca, wa[idx]) and np.array_equal(cb, wb[idx])
        for i in idx:
            assert masks_py([int(a[i])], bits) == (int(wa[i]), int(wb[i]), int(mk[i]))
            assert bin(int(mk[i])).count("1") == n


def two_pass_model(occurrences, bits, rnd):
    """Both passes over a list of keys (Python ints used as one-limb k-mers) in a shuffled order, with the stale read the
    kernel allows: a load in front of an atomic may show an OLDER word.  Returns (A, B, admitted Counter)."""
    A, B = {}, {}
    hist_a = {}                                                  # word -> its earlier values (what a stale read may show)
    for key in occurrences:
        wa, wb, mask = masks_py([key], bits)
        stale = rnd.choice(hist_a.get(wa, [0]))                  # any earlier value of the word, or the current one
        seen = (stale & mask) == mask
        if not seen:                                             # the returning atomic: exact
            old = A.get(wa, 0)
            A[wa] = old | mask
            hist_a.setdefault(wa, [0]).append(A[wa])
            seen = (old & mask) == mask
        if seen:
            B[wb] = B.get(wb, 0) | mask
    admitted = {}
    for key in occurrences:
        _, wb, mask = masks_py([key], bits)
        if (B.get(wb, 0) & mask) == mask:
            admitted[key] = admitted.get(key, 0) + 1
    return A, B, admitted


@pytest.mark.parametrize("bits,n", [(20, 6000), (12, 6000), (14, 300)])
def test_python_model_of_both_passes_keeps_the_contract(bits, n):
    rnd = random.Random(bits * 7 + n)
    keys = rnd.sample(range(1 << 60), n)
    counts = {key: (1 if i % 3 else rnd.choice((2, 2, 3, 7))) for i, key in enumerate(keys)}
    occ = [key for key, c in counts.items() for _ in range(c)]
    rnd.shuffle(occ)
    A, B, admitted = two_pass_model(occ, bits, rnd)
    singles = [key for key, c in counts.items() if c == 1]
    for key, c in counts.items():
        wa, wb, mask = masks_py([key], bits)
        assert A[wa] & mask == mask
        if c >= 2:                                               # the contract: in B, and every occurrence admitted
            assert B.get(wb, 0) & mask == mask and admitted.get(key) == c, key
        else:
            assert admitted.get(key, 0) in (0, 1)
    # every bit of B belongs to the mask of some key
    allowed = {}
    for key in counts:
        _, wb, mask = masks_py([key], bits)
        allowed[wb] = allowed.get(wb, 0) | mask
    assert all(B[w] & ~allowed.get(w, 0) == 0 for w in B)
    fp = sum(1 for key in singles if key in admitted)
    print("bits=%d keys=%d singles=%d admitted singles=%d" % (bits, n, len(singles), fp))
    if bits == 20:
        assert fp <= len(singles) // 100
    if bits == 12:
        assert fp > len(singles) // 2                            # saturated: the contract held all the same


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import tsxcount_amd as T
    L = T.lib()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                            # a map that is never looked at: these checks come first
    one = np.zeros(4, dtype=np.uint64)
    w = ctypes.c_uint64()
    for bits in (11, 39, 0, -1, 64):
        assert L.tsx_hip_prefilter_create(fake, bits) == T.EINVAL, bits
        assert L.tsx_hip_prefilter_mask_host(31, one.ctypes.data_as(U64P), bits, ctypes.byref(w), None, None) == T.EINVAL, bits
        with pytest.raises(ValueError):
            T.prefilter_masks(one[:1], 31, bits)
    assert L.tsx_hip_prefilter_create(None, 20) == T.EINVAL
    assert L.tsx_hip_prefilter_mask_host(0, one.ctypes.data_as(U64P), 20, None, None, None) == T.EINVAL
    assert L.tsx_hip_prefilter_mask_host(128, one.ctypes.data_as(U64P), 20, None, None, None) == T.EINVAL
    assert L.tsx_hip_prefilter_mask_host(31, None, 20, None, None, None) == T.EINVAL
    assert L.tsx_hip_prefilter_mask_host(31, one.ctypes.data_as(U64P), 20, None, None, None) == T.OK   # every output is optional
    for call in (L.tsx_hip_prefilter_free, L.tsx_hip_prefilter_armed, L.tsx_hip_prefilter_bits):
        assert call(None) == T.EINVAL
    assert L.tsx_hip_prefilter_arm(None, 1) == T.EINVAL and L.tsx_hip_prefilter_stats(None, None) == T.EINVAL
    assert L.tsx_hip_prefilter_stats(fake, None) == T.EINVAL
    assert L.tsx_hip_prefilter_add_host(None, b"x", 1, 0) == T.EINVAL
    assert L.tsx_hip_prefilter_add_bgzf_host(None, b"x", 1) == T.EINVAL
    assert L.tsx_hip_prefilter_add_device(None, vp(0x2000), 16, None) == T.EINVAL
    assert L.tsx_hip_prefilter_read(None, 0, one.ctypes.data_as(U64P), 4) == T.EINVAL
    m = T.TSXHashMapHIP.__new__(T.TSXHashMapHIP)
    with pytest.raises(ValueError):
        m.prefilterWords("c")


def test_cli_usage_errors_of_the_two_pass_count(tmp_path):
    code, _, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--min-count=1|2", "--prefilter-bits=B", "prefilter<TAB>bits<TAB>kmers<TAB>seen_again<TAB>admitted<TAB>skipped"):
        assert flag in err, flag
    base = ("--input=x.fastq", "--k=15", "--l=12", "--min-count=2")
    for extra, word in ((("--gpus=2",), "one GPU"), (("--format=fasta-wrapped",), "wrapped"), (("--check",), "--check"),
                        (("--load=" + str(tmp_path / "x.db"),), "--load"), (("--l=auto",), "--l=auto"),
                        (("--prefilter-bits=11",), "12 .. 38"), (("--prefilter-bits=39",), "12 .. 38"),
                        (("--prefilter-bits=0",), "12 .. 38"), (("--prefilter-bits=abc",), "12 .. 38"),
                        (("--prefilter-bits=",), "12 .. 38"), (("--prefilter-bits=20x",), "12 .. 38")):
        code, out, err = run_cli(*base, *extra, timeout=30)
        why = err.split("Usage")[0]                              # the sentence in front of the usage text
        assert code == 1 and "Usage" in err and word in why and out == "", (extra, why)
    for v in ("0", "3", "two", ""):
        code, out, err = run_cli("--input=x.fastq", "--k=15", "--min-count=" + v, timeout=30)
        assert code == 1 and "--min-count takes 1" in err and out == "", v
    code, _, err = run_cli("--input=x.fastq", "--k=15", "--prefilter-bits=20", timeout=30)
    assert code == 1 and "--prefilter-bits needs --min-count=2" in err
    code, _, err = run_cli("--k=15", "--min-count=2", timeout=30)
    assert code == 1 and "--min-count=2 needs --input" in err
