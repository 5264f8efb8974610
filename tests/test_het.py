"""Heterozygous k-mer pairs on the GPU: tsx_hip_het_histogram_*, tsx_hip_het_pairs_device and
tsx_hip_write_het_pairs_host through Python, their refusals and the CLI.

The reference is tsxcount_amd.het_pairs / het_histogram (strings on the CPU) over the table's own dump
(getAllKmers -> dict); matrix, stats and the sorted pair list are compared for equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import kmerdb

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
BINS = [(2, 2), (3, 200), (65, 65), (1002, 1002)]   # the least, narrower than the LDS corner one way, one past it, the default
MODES = ("unique", "all")


def run_cli(*args, timeout=300):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def table_dict(m):
    k, c = m.getAllKmers()
    names = kmerdb.limbs_to_kmers(k, m.k)
    d = dict(zip(names, (int(x) for x in c)))
    assert len(d) == len(names)
    return d


def from_dict(d, k, l=15, s=0, **kw):
    import tsxcount_amd as T
    m = T.TSXHashMapHIP(l, s, k, **kw)
    if d:
        names = sorted(d)
        m.addKmers(kmerdb.kmers_to_limbs(names, k), np.array([d[x] for x in names], dtype=np.uint64))
    return m


def random_names(rng, n, k):
    names = kmerdb.limbs_to_kmers(rng.integers(0, 1 << 62, size=(n, (2 * k + 63) // 64), dtype=np.uint64), k)
    return sorted(set(names))


def pair_list(m, rec):
    """hetPairs' records as the sorted tuples het_pairs gives."""
    a = kmerdb.limbs_to_kmers(rec["minor"], m.k) if len(rec) else []
    b = kmerdb.limbs_to_kmers(rec["major"], m.k) if len(rec) else []
    return sorted((x.decode(), int(ca), y.decode(), int(cb)) for x, ca, y, cb in zip(a, rec["minor_count"], b, rec["major_count"]))


def check(m, d=None, bins=((65, 65),), modes=MODES, lower=1, upper=None, lists=True):
    """hetHistogram and hetPairs of m against the CPU statement over its dump; returns {mode: (matrix, stats, pairs)}."""
    import tsxcount_amd as T
    d = table_dict(m) if d is None else d
    out = {}
    for mode in modes:
        want_pairs, want_stats = T.het_pairs(d, m.k, lower, upper, mode, canonical=m.canonical)
        for nm, nM in bins:
            got, st = m.hetHistogram(nm, nM, lower, upper, mode)
            want = T.het_histogram(want_pairs, nm, nM)
            assert got.dtype == np.uint64 and got.shape == (nm, nM)
            assert np.array_equal(got, want), (mode, nm, nM, np.argwhere(got != want)[:5])
            assert st == want_stats, (mode, st, want_stats)
        if lists:
            assert pair_list(m, m.hetPairs(lower, upper, mode)) == want_pairs, mode
        out[mode] = (got, st, want_pairs)
    return out


def planted(rng, k, canonical, copies=3):
    """Families of sizes 1 .. 4 with distinct counts (`copies` of each size, other flanks), a few hundred random k-mers, on
    a canonical table families whose flanks are reverse complements of each other, and two pairs of equal counts (the
    tie rule of the list: the smaller text is the minor, at every key width)."""
    p = (k - 1) // 2
    flank = lambda: bytes(rng.choice(list(b"ACGT"), size=p).astype(np.uint8))
    d = {x: int(c) for x, c in zip(random_names(rng, 300, k), rng.integers(1, 40, size=300))}
    c = 50
    for size in (1, 2, 3, 4) * copies:
        left, right = flank(), flank()
        for b in rng.permutation(list(b"ACGT"))[:size]:
            d[left + bytes([b]) + right] = c
            c += 1
    if canonical:
        for mids in (b"AC", b"TG", b"A"):      # two strand pairs, the other two strands of them, one alone
            left = flank()
            for b in mids:
                d[left + bytes([b]) + kmerdb.revcomp(left)] = c
                c += 1
    for mids in (b"GA", b"CT"):
        left, right = flank(), flank()
        for b in mids:
            d[left + bytes([b]) + right] = c
        c += 1
    return d


# ---- 1. every key width where the middle base moves ---------------------------------------------------------------

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [15, 31, 33, 63, 65, 127])
def test_every_key_width(k, canonical):
    import tsxcount_amd as T
    rng = np.random.default_rng(1000 + k)
    m = from_dict(planted(rng, k, canonical), k, l=14 + k % 3, canonical=canonical, hash_seed=k)
    d = table_dict(m)
    res = check(m, d, bins=[(1002, 1002), (3, 200)])
    for mode in MODES:
        st = res[mode][1]
        assert st["pairs"] and st["families_2"] and st["families_3plus"]
        assert sum(1 for _, ca, _, cb in res[mode][2] if ca == cb) >= 2      # ties: the list's order of a pair is by text
    assert res["all"][1]["pairs"] > res["unique"][1]["pairs"] == res["unique"][1]["families_2"]
    if canonical:
        pairs = res["all"][2]
        assert any(a[:k // 2] == kmerdb.revcomp(a[k // 2 + 1:].encode()).decode() for a, _, _, _ in pairs)   # palindromic flanks
        # a pair whose members are stored under different strands: one as the key of the reported k-mer, one as its mirror's
        key = lambda x: tuple(int(v) for v in m.hash_apply(T.encode(x, k))[::-1])     # (a WK-limb number, top limb first)
        fwd = lambda x: key(x) < key(T.revcomp(x))
        assert any(fwd(a) != fwd(b) for a, _, b, _ in pairs)
    m.close()


# ---- 2. layout independence ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("canonical", [False, True])
def test_layout_independence(canonical, monkeypatch):
    import tsxcount_amd as T
    k = 33
    rng = np.random.default_rng(7)
    d = planted(rng, k, canonical)
    want = None
    tables = [dict(l=14, s=0, hash_seed=1), dict(l=16, s=0, hash_seed=1), dict(l=15, s=6, hash_seed=2), dict(l=15, s=2, hash_seed=3),
              dict(l=15, s=0, hash_seed=4, seg=9)]
    for kw in tables:
        seg = kw.pop("seg", None)
        if seg:
            monkeypatch.setenv("TSX_HIP_SEG_BITS", str(seg))
        m = from_dict(d, k, canonical=canonical, **kw)
        if seg:
            monkeypatch.delenv("TSX_HIP_SEG_BITS")
        assert kw["s"] != 2 or m.stats()["overflow_used"] > 0   # two storage bits (the least a carried-count test here uses): counts of 4 and more carry
        if want is None:
            td = table_dict(m)
            want = {mode: T.het_pairs(td, k, mode=mode, canonical=canonical) for mode in MODES}
            cut = {mode: T.het_pairs(td, k, 8, 60, mode, canonical=canonical) for mode in MODES}
            assert cut["all"][1]["pairs"] and cut["all"][1] != want["all"][1]
        for mode in MODES:
            got, st = m.hetHistogram(65, 65, mode=mode)
            assert st == want[mode][1] and np.array_equal(got, T.het_histogram(want[mode][0], 65, 65)), (kw, mode)
            assert pair_list(m, m.hetPairs(mode=mode)) == want[mode][0], (kw, mode)
            # a range far above the in-slot field: the slot's and the probe's count read the secondary array
            got, st = m.hetHistogram(9, 70, 8, 60, mode)
            assert st == cut[mode][1] and np.array_equal(got, T.het_histogram(cut[mode][0], 9, 70)), (kw, mode)
        m.close()


# ---- 3. bins and ranges ----------------------------------------------------------------------------------------------

def test_bins_and_ranges():
    k = 31
    rng = np.random.default_rng(3)
    ladder = [1, 2, 3, 63, 64, 65, 66, 199, 200, 201, 1000, 1001, 1002, 5000]
    d = {}
    for i in range(len(ladder) * 4):     # pairs, triples and quadruples over the ladder: counts on both sides of each clip
        left = bytes(rng.choice(list(b"ACGT"), size=15).astype(np.uint8))
        right = bytes(rng.choice(list(b"ACGT"), size=15).astype(np.uint8))
        for j, b in enumerate(b"ACGT"[:2 + i % 3]):
            d[left + bytes([b]) + right] = ladder[(i + 5 * j) % len(ladder)]
    m = from_dict(d, k, hash_seed=3)
    assert table_dict(m) == d
    res = check(m, d, bins=BINS + [(64, 64), (70, 20), (20, 70)])
    mat = m.hetHistogram(20, 70, mode="all")[0]
    assert mat[19, 69] and mat[1:19, 69].sum() and mat[:, :69].sum()
    mat = m.hetHistogram(mode="all")[0]
    assert mat[64:, 64:].sum() and mat[:64, :64].sum() and mat[:64, 64:].sum()      # beside the LDS corner, in it, across
    # ranges that cut members out: families of 3 become pairs, pairs become singletons
    for lower, upper in ((2, None), (1, 200), (64, 1001), (3, 3), (0, None)):
        r = check(m, d, bins=[(65, 65), (1002, 1002)], lower=lower, upper=upper)
        assert r["all"][1] != res["all"][1] or lower == 0
    m.close()


# ---- 4. from reads ---------------------------------------------------------------------------------------------------

def test_from_reads_of_two_haplotypes():
    import tsxcount_amd as T
    k = 21
    rng = np.random.default_rng(21)
    hap_a = rng.choice(list(b"ACGT"), size=3000).astype(np.uint8)
    hap_b = hap_a.copy()
    for at in range(30, 3000, 60):
        hap_b[at] = rng.choice([b for b in b"ACGT" if b != hap_a[at]])
    recs = []
    for hap, depth in ((hap_a, 30), (hap_b, 12)):      # unequal depth: the two counts of a pair differ
        for at in rng.integers(0, 3000 - 100, size=depth * 30):
            recs.append(b"@r\n" + bytes(hap[at:at + 100]) + b"\n+\n" + b"I" * 100 + b"\n")
    m = T.TSXHashMapHIP(16, 0, k, canonical=True)
    m.countFastq(b"".join(recs))
    res = check(m, bins=[(1002, 1002)])
    mat, st, _ = res["unique"]
    assert st["pairs"] > 0
    i, j = np.unravel_index(int(np.argmax(mat)), mat.shape)
    assert i != j and i < j
    m.close()


# ---- 5. list mechanics -----------------------------------------------------------------------------------------------

def test_list_by_slot_ranges_capacity_and_chunks(tmp_path):
    import torch
    import tsxcount_amd as T
    k = 63
    rng = np.random.default_rng(5)
    m = from_dict(planted(rng, k, True, copies=8), k, l=14, canonical=True, hash_seed=5)
    d = table_dict(m)
    L = T.lib()
    for mode in MODES:
        want, st = T.het_pairs(d, k, mode=mode, canonical=True)
        assert len(want) > 8
        whole = m.hetPairs(mode=mode)
        assert pair_list(m, whole) == want
        parts = [m.hetPairs(mode=mode, slot_lo=lo, slot_hi=lo + 64) for lo in range(0, 1 << 14, 64)]
        assert sum(len(x) for x in parts) == len(want) and pair_list(m, np.concatenate(parts)) == want
        assert pair_list(m, m.hetPairs(mode=mode, range_slots=1000)) == want
        # a buffer one record short: ERANGE, the true total, cap valid records
        dt = T.het_pair_dtype(k)
        words, cap = dt.itemsize // 8, len(want) - 1
        buf = torch.full((cap * words + 1 + words,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        rule = T.het_rule(1, None, mode)
        vp = ctypes.c_void_p
        rc = L.tsx_hip_het_pairs_device(m.handle, ctypes.byref(rule), 0, 1 << 14, vp(buf.data_ptr()), cap,
                                        vp(buf.data_ptr() + (cap + 1) * words * 8), None)
        assert rc == T.ERANGE
        host = buf.cpu().numpy().view(np.uint64)
        assert int(host[(cap + 1) * words]) == len(want)
        assert (host[cap * words:(cap + 1) * words] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()    # nothing behind the cap
        got = pair_list(m, host[:cap * words].view(dt))
        assert len(set(got)) == cap and set(got) < set(want)
        # the text: one chunk against the smallest chunks
        one, small = str(tmp_path / ("one." + mode)), str(tmp_path / ("small." + mode))
        n1, b1 = m.writeHetPairs(one, mode=mode)
        least = 64 * (2 * (k + 21) + 2) * (3 if mode == "all" else 1)
        n2, b2 = m.writeHetPairs(small, mode=mode, chunk_bytes=least)
        lines = sorted(open(one).read().splitlines())
        assert lines == sorted(open(small).read().splitlines())
        assert lines == sorted("%s\t%d\t%s\t%d" % (a, ca, b, cb) for a, ca, b, cb in want)
        assert n1 == n2 == len(want) and b1 == b2 == os.path.getsize(one) == os.path.getsize(small)
        with pytest.raises(T.TSXException) as e:
            m.writeHetPairs(small, mode=mode, chunk_bytes=least - 1)
        assert e.value.code == T.EINVAL and "chunk_bytes" in str(e.value)
    m.close()


# ---- 6. leaves the table alone, refusals, the device form ----------------------------------------------------------------

def test_table_unchanged_and_device_form(tmp_path):
    import torch
    k = 65
    rng = np.random.default_rng(6)
    m = from_dict(planted(rng, k, False), k, l=14, s=3, hash_seed=6)
    image = lambda name: (m.saveDatabase(str(tmp_path / name)), open(str(tmp_path / name), "rb").read())[1]
    before = table_dict(m), m.stats(), image("0.db")
    host = {mode: m.hetHistogram(70, 33, mode=mode) for mode in MODES}
    check(m, before[0], bins=BINS)
    m.writeHetPairs(str(tmp_path / "p.tsv"), mode="all")
    # the device form on a caller's stream, into garbage: the call zeroes its outputs
    st = torch.cuda.Stream(torch.device("cuda", 0))
    for mode in MODES:
        buf = torch.full((70 * 33 + 5,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        m.hetHistogramDevice(buf.data_ptr(), buf.data_ptr() + 70 * 33 * 8, 70, 33, mode=mode, stream=st.cuda_stream)
        st.synchronize()
        got = buf.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:70 * 33].reshape(70, 33), host[mode][0])
        assert [int(x) for x in got[70 * 33:]] == list(host[mode][1].values())
    assert (table_dict(m), m.stats(), image("1.db")) == before
    # a lazily cleared table is zeroed before it is read
    m.clear()
    mat, stats = m.hetHistogram(65, 65)
    assert not mat.any() and not any(stats.values()) and len(m.hetPairs()) == 0
    m.close()


def test_refusals():
    import tsxcount_amd as T
    m = from_dict({b"ACGTACGTACGTACG": 1}, 15, l=14)
    L = T.lib()
    vp = ctypes.c_void_p
    out = np.zeros(4, dtype=np.uint64)
    st = T.HetStats()
    good = T.het_rule()

    def refused(rc, what):
        assert rc == T.EINVAL
        msg = L.tsx_hip_last_error().decode()
        assert msg and what in msg, msg

    hist = lambda h, rule, nm=2, nM=2, o=out: L.tsx_hip_het_histogram_host(h, ctypes.byref(rule) if rule else None, T._p(o) if o is not None else None, nm, nM, ctypes.byref(st))
    refused(hist(None, good), "map")
    refused(hist(m.handle, None), "rule")
    refused(hist(m.handle, good, o=None), "no matrix")
    refused(L.tsx_hip_het_histogram_device(m.handle, ctypes.byref(good), 2, 2, None, None, None), "no matrix")
    refused(hist(m.handle, T.HetRule(5, 4, 0, 0)), "lower > upper")
    refused(hist(m.handle, T.HetRule(1, 4, 2, 0)), "mode")
    refused(hist(m.handle, T.HetRule(1, 4, -1, 0)), "mode")
    refused(hist(m.handle, T.HetRule(1, 4, 0, 1)), "reserved")
    refused(hist(m.handle, good, 1, 100), "fewer than 2 bins")
    refused(hist(m.handle, good, 100, 1), "fewer than 2 bins")
    refused(hist(m.handle, good, 4097, 4096), "2^24")
    refused(hist(m.handle, good, 2, (1 << 23) + 1), "2^24")
    even = from_dict({}, 14, l=14)
    shard = T.TSXHashMapHIP(14, 0, 15, shard_bits=1, shard_index=0)
    n = np.zeros(1, dtype=np.uint64)
    for h, what in ((even.handle, "even k"), (shard.handle, "shard_bits")):
        refused(hist(h, good), what)
        refused(L.tsx_hip_het_pairs_device(h, ctypes.byref(good), 0, 0, None, 0, vp(1), None), what)
        refused(L.tsx_hip_write_het_pairs_host(h, ctypes.byref(good), 1, 0, None, None), what)
    slots = int(m.layout.slots)
    refused(L.tsx_hip_het_pairs_device(m.handle, ctypes.byref(good), 5, 4, None, 0, vp(1), None), "slot range")
    refused(L.tsx_hip_het_pairs_device(m.handle, ctypes.byref(good), 0, slots + 1, None, 0, vp(1), None), "slot range")
    refused(L.tsx_hip_het_pairs_device(m.handle, ctypes.byref(good), 0, slots, None, 0, None, None), "no output")
    refused(L.tsx_hip_het_pairs_device(m.handle, ctypes.byref(good), 0, slots, None, 4, vp(1), None), "no output")
    refused(L.tsx_hip_write_het_pairs_host(m.handle, ctypes.byref(good), -1, 0, None, None), "no output")
    for call in (lambda: m.hetHistogram(mode="some"), lambda: m.hetPairs(mode="some")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(T.TSXException) as e:
        even.hetHistogram()
    assert e.value.code == T.EINVAL and "even k" in str(e.value)
    with pytest.raises(T.TSXException) as e:
        m.hetHistogram(4097, 4096)
    assert e.value.code == T.EINVAL and "2^24" in str(e.value)
    assert m.hetHistogram(4096, 4096)[1]["kmers_in_range"] == 1      # 2^24 cells are allowed
    for x in (m, even, shard):
        x.close()


# ---- 7. CLI ----------------------------------------------------------------------------------------------------------

def read_counts(path):
    return {line.split("\t")[0]: int(line.split("\t")[1]) for line in open(path)}


def test_cli_end_to_end(tmp_path, golden_fastq):
    import tsxcount_amd as T
    k = 15
    fq = tmp_path / "g.fastq"
    fq.write_bytes(golden_fastq)
    dump, hs, hm, pl = (str(tmp_path / x) for x in ("g.count", "h.tsv", "h.mat", "p.tsv"))
    rc, out, err = run_cli("--input=%s" % fq, "--k=15", "--l=18", "--canonical", "--output=%s" % dump, "--het-histo=%s" % hs,
                           "--het-pairs=%s" % pl)
    assert rc == 0, err
    d = read_counts(dump)
    pairs, st = T.het_pairs(d, k, canonical=True)
    assert st["pairs"] > 0

    def het_line(out, st):
        line = [x for x in out.splitlines() if x.startswith("het\t")]
        assert len(line) == 1
        assert [int(x) for x in line[0].split("\t")[1:]] == list(st.values())

    het_line(out, st)
    want = T.het_histogram(pairs, 1002, 1002)
    rows = [tuple(int(x) for x in line.split("\t")) for line in open(hs)]
    assert rows == sorted(rows) and len(set(r[:2] for r in rows)) == len(rows) and all(r[2] > 0 for r in rows)
    got = np.zeros_like(want)
    for i, j, n in rows:
        got[i, j] = n
    assert np.array_equal(got, want)
    assert sorted(open(pl).read().splitlines()) == sorted("%s\t%d\t%s\t%d" % p for p in pairs)
    # matrix format, another H, mode and range
    rc, out, err = run_cli("--input=%s" % fq, "--k=15", "--l=18", "--canonical", "--het-histo=%s" % hm, "--het-format=matrix",
                           "--het-max=5", "--het-mode=all", "--het-lower=2", "--het-upper=40", "--het-pairs=%s" % pl)
    assert rc == 0, err
    pairs, st = T.het_pairs(d, k, 2, 40, "all", canonical=True)
    het_line(out, st)
    lines = open(hm).read().splitlines()
    assert lines[0] == "# rows: minor count 0..6, columns: major count" and len(lines) == 8
    got = np.array([[int(x) for x in line.split("\t")] for line in lines[1:]], dtype=np.uint64)
    assert np.array_equal(got, T.het_histogram(pairs, 7, 7))
    assert sorted(open(pl).read().splitlines()) == sorted("%s\t%d\t%s\t%d" % p for p in pairs)
    # next to --op: the pairs are those of the table before the op, --output is the result
    db, o = str(tmp_path / "g.db"), str(tmp_path / "i.count")
    rc, _, err = run_cli("--input=%s" % fq, "--k=15", "--l=18", "--canonical", "--save=%s" % db)
    assert rc == 0, err
    rc, out, err = run_cli("--load=%s" % db, "--canonical", "--with=%s" % db, "--op=subtract", "--output=%s" % o, "--het-histo=%s" % hs)
    assert rc == 0, err
    het_line(out, T.het_pairs(d, k, canonical=True)[1])
    assert read_counts(o) == {}
    assert sum(int(line.split("\t")[2]) for line in open(hs)) == T.het_pairs(d, k, canonical=True)[1]["pairs"]
    # --gpus=1 is the one table of this process
    rc, out, err = run_cli("--input=%s" % fq, "--k=15", "--l=18", "--canonical", "--gpus=1", "--het-histo=%s" % hs, "--het-pairs=%s" % pl)
    assert rc == 0, err
    pairs, st = T.het_pairs(d, k, canonical=True)
    het_line(out, st)
    assert sum(int(line.split("\t")[2]) for line in open(hs)) == st["pairs"]
    assert sorted(open(pl).read().splitlines()) == sorted("%s\t%d\t%s\t%d" % p for p in pairs)
    # refusals
    for args, what in ((["--gpus=2", "--k=15"], "one GPU"), (["--k=14"], "odd k"), (["--k=15", "--het-lower=abc"], "--het-lower"),
                       (["--k=15", "--het-upper=-1"], "--het-upper"), (["--k=15", "--het-lower=3x"], "--het-lower")):
        rc, out, err = run_cli("--input=%s" % fq, "--l=18", "--het-histo=%s" % hs, *args)
        assert rc != 0 and what in err, err
