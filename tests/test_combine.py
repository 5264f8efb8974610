"""Table set operations on the GPU: tsx_hip_combine through Python, the C ABI's refusals and the tsxCount CLI.

Every expectation comes from tests/combine_ref.py (plain Python over python_counts dicts) or, for the cross-checks,
from entry points that existed before (addDatabase, getKmerCounts, stats); every k-mer of every result is compared."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, python_counts
from combine_ref import MODES, OPS, combine_expect, jaccard
import kmerdb

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
CUT = dict(a_range=(2, 40), b_range=(1, 3))   # drops the singletons and the poly-A k-mers of A, everything above 3 of B


def run_cli(*args, timeout=300):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def synth_pair(seed, n=36, shared=18):
    """Two texts of n reads each that share `shared` reads; the shared ones are doubled in A so that counts differ."""
    from tsxcount_amd import synth
    a = synth.fastq(seed, 0, n) + synth.fastq(seed, n - shared, shared // 2)
    b = synth.fastq(seed, n - shared, n)
    return a, b


def golden_pair(text):
    recs = text.split(b"\n")
    half = (len(recs) // 8) * 4
    return b"\n".join(recs[:half + 200]) + b"\n", b"\n".join(recs[half - 200:])


def table_dict(m):
    k, c = m.getAllKmers()
    names = kmerdb.limbs_to_kmers(k, m.k)
    d = dict(zip(names, (int(x) for x in c)))
    assert len(d) == len(names)
    return d


def counted(text, k, l=18, s=0, fold=False, **kw):
    import tsxcount_amd as T
    m = T.TSXHashMapHIP(l, s, k, **kw)
    m.countFastq(text)
    d = python_counts(text, k)
    return m, (kmerdb.fold_strands(d) if fold else dict(d))


def from_dict(d, k, l=16, s=0, **kw):
    import tsxcount_amd as T
    m = T.TSXHashMapHIP(l, s, k, **kw)
    if d:
        names = sorted(d)
        m.addKmers(kmerdb.kmers_to_limbs(names, k), np.array([d[x] for x in names], dtype=np.uint64))
    return m


def check_result(out, want, want_st):
    assert table_dict(out) == want
    assert out.combine_stats == want_st, (out.combine_stats, want_st)
    st = out.stats()
    assert st["distinct"] == want_st["out_entries"]
    assert st["count_sum"] == st["kmers_added"] == want_st["out_count_sum"]
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0


def all_rules():
    for op in OPS:
        for mode in (MODES if op in ("intersect", "union") else ("min",)):
            for kw in ({}, CUT):
                yield op, mode, kw


@pytest.mark.parametrize("k", [14, 31, 33, 63, 127])
def test_every_op_and_count_mode(golden_fastq, k):
    ta, tb = golden_pair(golden_fastq) if k == 14 else synth_pair(k)
    a, da = counted(ta, k, hash_seed=5)
    b, db = counted(tb, k, hash_seed=5)
    assert set(da) & set(db) and set(da) - set(db) and set(db) - set(da)
    out = None
    for op, mode, kw in all_rules():
        want, want_st = combine_expect(da, db, op, mode, **kw)
        if kw:
            assert want_st["a_in_range"] < len(da) and want_st["b_in_range"] < len(db)   # the ranges cut real k-mers out
        if out is None:
            out = a.combine(b, op, mode, **kw)
        else:
            out.clear()
            assert a.combine(b, op, mode, out=out, **kw) is out
        check_result(out, want, want_st)
    for m in (a, b, out):
        m.close()


@pytest.mark.parametrize("k", [14, 31, 64])
def test_canonical_tables(golden_fastq, k):
    ta, tb = golden_pair(golden_fastq) if k == 14 else synth_pair(k + 1)
    if k != 31:   # even k: palindromes among the k-mers
        pal = (b"ACGT" * 32)[:k // 2]
        pal += kmerdb.revcomp(pal)
        rec = b"@pal\n" + pal + b"AC" + b"\n+\n" + b"I" * (k + 2) + b"\n"
        ta, tb = ta + rec * 3, tb + rec
    a, da = counted(ta, k, fold=True, canonical=True, hash_seed=2)
    b, db = counted(tb, k, fold=True, canonical=True, hash_seed=3, l=19)   # the general path
    b2, _ = counted(tb, k, fold=True, canonical=True, hash_seed=2)         # the aligned one
    if k != 31:
        assert da[pal] == 3 and db[pal] == 1
    for op, mode, kw in all_rules():
        want, want_st = combine_expect(da, db, op, mode, **kw)
        for bb in (b, b2):
            out = a.combine(bb, op, mode, **kw)
            assert out.canonical
            check_result(out, want, want_st)
            out.close()
    for m in (a, b, b2):
        m.close()


def test_tables_with_a_base_rule():
    import tsxcount_amd as T
    ta, tb = synth_pair(77, 20, 10)
    spoil = lambda t: t.replace(b"ACG", b"ANG", 40)
    ta, tb = spoil(ta), spoil(tb)
    k = 31
    clean = lambda d: {x: c for x, c in d.items() if set(x) <= set(b"ACGT")}
    a, da = counted(ta, k, acgt_only=True)
    b, db = counted(tb, k, acgt_only=True)
    da, db = clean(da), clean(db)
    assert len(da) == a.stats()["distinct"]
    for op in OPS:
        want, want_st = combine_expect(da, db, op, "sum")
        out = a.combine(b, op, "sum")
        assert out.base_rule == (True, None)
        check_result(out, want, want_st)
        out.close()
    plain = T.TSXHashMapHIP(18, 0, k)
    plain.countFastq(tb)
    with pytest.raises(T.TSXException) as e:
        a.combine(plain)
    assert e.value.code == T.EINVAL and "base rule" in str(e.value)
    for m in (a, b, plain):
        m.close()


@pytest.mark.parametrize("k", [31, 63])
def test_counts_that_carry(k):
    """Three storage bits: counts of 8 and more live in the secondary array."""
    rng = np.random.default_rng(k)
    names = kmerdb.limbs_to_kmers(rng.integers(0, 1 << 62, size=(600, (2 * k + 63) // 64), dtype=np.uint64), k)
    names = sorted(set(names))
    da = {x: int(c) for x, c in zip(names[:450], rng.integers(1, 30, size=450))}
    db = {x: int(c) for x, c in zip(names[150:], rng.integers(1, 30, size=len(names) - 150))}
    da[names[200]], db[names[200]] = 5, 6      # SUM carries although neither input does
    da[names[201]], db[names[201]] = 29, 25    # DIFF and MIN: 4 and 25 -- DIFF stops carrying
    da[names[202]], db[names[202]] = 20, 3     # MIN stops carrying
    a, b = from_dict(da, k, s=3, hash_seed=8), from_dict(db, k, s=3, hash_seed=8)
    assert a.stats()["overflow_used"] > 0 and b.stats()["overflow_used"] > 0
    for op, mode, kw in list(all_rules()) + [("intersect", "sum", dict(a_range=(1, 7), b_range=(1, 7)))]:
        want, want_st = combine_expect(da, db, op, mode, **kw)
        for hs in (8, 9):   # aligned, general
            out = a.combine(b, op, mode, hash_seed=hs, **kw)
            check_result(out, want, want_st)
            assert out.stats()["overflow_used"] == sum(1 for c in want.values() if c >= 8)
            if op == "intersect" and mode == "sum" and kw != CUT:
                assert want[names[200]] == 11 and out.getKmerCount(names[200]) == 11
            out.close()
    out = a.combine(b, "diff")
    assert out.getKmerCount(names[201]) == 4 and out.getKmerCount(names[202]) == 17
    out.close()
    out = a.combine(b, "intersect", "min", iStorageBits=0)   # a wide counter: nothing carries in OUT
    assert out.stats()["overflow_used"] == 0 and out.getKmerCount(names[202]) == 3
    check_result(out, *combine_expect(da, db, "intersect", "min"))
    for m in (a, b, out):
        m.close()


def test_geometries_and_both_paths(monkeypatch):
    import tsxcount_amd as T
    k = 33
    ta, tb = synth_pair(9)
    a, da = counted(ta, k, l=18, hash_seed=4)
    others = {"aligned": counted(tb, k, l=18, hash_seed=4)[0], "l": counted(tb, k, l=19, hash_seed=4)[0],
              "seed": counted(tb, k, l=18, hash_seed=6)[0], "bits": counted(tb, k, l=18, s=5, hash_seed=4)[0]}
    db = dict(python_counts(tb, k))
    for op, mode in (("intersect", "min"), ("union", "sum"), ("subtract", "min"), ("diff", "min")):
        want, want_st = combine_expect(da, db, op, mode)
        for name, b in others.items():
            for out_kw in ({}, {"iL": 19}, {"hash_seed": 77}):
                for path in ("0", "1", "2"):
                    monkeypatch.setenv("TSX_HIP_COMBINE_PATH", path)
                    if path == "2" and name != "aligned":
                        with pytest.raises(T.TSXException) as e:
                            a.combine(b, op, mode, **out_kw)
                        assert e.value.code == T.EINVAL and "aligned" in str(e.value)
                        continue
                    out = a.combine(b, op, mode, **out_kw)
                    check_result(out, want, want_st)
                    out.close()
    monkeypatch.delenv("TSX_HIP_COMBINE_PATH")
    a.close()
    for b in others.values():
        b.close()


def test_union_sum_is_add_database(tmp_path):
    import tsxcount_amd as T
    from test_database import assert_same_table
    for k, s in ((31, 0), (63, 4)):
        ta, tb = synth_pair(21 + k, 24, 12)
        a, _ = counted(ta, k, s=s, hash_seed=3)
        b, _ = counted(tb, k, s=s, hash_seed=3)
        dba, dbb = str(tmp_path / "a.db"), str(tmp_path / "b.db")
        a.saveDatabase(dba)
        b.saveDatabase(dbb)
        merged = T.TSXHashMapHIP.fromDatabase(dba)
        merged.addDatabase(dbb)
        out = a.combine(b, "union", "sum")
        assert_same_table(out, merged)
        for m in (a, b, merged, out):
            m.close()


def test_same_table_empty_tables_and_stats_only():
    import tsxcount_amd as T
    k = 31
    ta, tb = synth_pair(5, 16, 8)
    a, da = counted(ta, k)
    b, db = counted(tb, k)
    empty = T.TSXHashMapHIP(18, 0, k)
    cleared = counted(tb, k)[0]
    cleared.clear()
    for op, mode, kw in all_rules():
        for bb, dd in ((a, da), (empty, {}), (cleared, {})):
            want, want_st = combine_expect(da, dd, op, mode, **kw)
            out = a.combine(bb, op, mode, **kw)
            check_result(out, want, want_st)
            out.close()
        want, want_st = combine_expect({}, db, op, mode, **kw)   # empty A
        out = empty.combine(b, op, mode, **kw)
        check_result(out, want, want_st)
        out.close()
    want, want_st = combine_expect(da, db, "intersect", "min", a_range=(1, 1), b_range=(500, 600))
    assert want == {}
    out = a.combine(b, "intersect", "min", a_range=(1, 1), b_range=(500, 600))   # an empty result
    check_result(out, want, want_st)
    out.close()
    # compare(): the stats of the run that writes, and the Jaccard index
    for kw in ({}, CUT):
        _, want_st = combine_expect(da, db, "intersect", "min", **kw)
        got = a.compare(b, **kw)
        assert got.pop("jaccard") == pytest.approx(jaccard(want_st), rel=1e-12)
        assert got == want_st
    # out == NULL for every op: what the rule would write
    for op, mode, kw in all_rules():
        _, want_st = combine_expect(da, db, op, mode, **kw)
        assert a._combine(b, T.combine_rule(op, mode, **kw), None) == want_st
    for m in (a, b, empty, cleared):
        m.close()


def test_inputs_unchanged(tmp_path, monkeypatch):
    k = 63
    ta, tb = synth_pair(15, 16, 8)
    a, _ = counted(ta, k, s=3, hash_seed=1)
    b, _ = counted(tb, k, s=3, hash_seed=1)
    image = lambda m, name: (m.saveDatabase(str(tmp_path / name)), open(str(tmp_path / name), "rb").read(), m.stats())[1:]
    before = image(a, "a0.db"), image(b, "b0.db")
    for path in ("1", "2"):
        monkeypatch.setenv("TSX_HIP_COMBINE_PATH", path)
        for op in OPS:
            a.combine(b, op, "sum").close()
            a.compare(b)
    assert (image(a, "a1.db"), image(b, "b1.db")) == before
    a.close(); b.close()


def test_refusals():
    import tsxcount_amd as T
    k = 31
    ta, tb = synth_pair(3, 8, 4)
    a, _ = counted(ta, k)
    b, _ = counted(tb, k)

    def refused(what, *args, **kw):
        with pytest.raises(T.TSXException) as e:
            a.combine(*args, **kw)
        assert e.value.code == T.EINVAL and what in str(e.value), str(e.value)

    full = counted(tb, k)[0]
    refused("not empty", b, out=full)
    refused("one of the inputs", b, out=a)
    refused("one of the inputs", b, out=b)
    other_k = counted(tb, 29)[0]
    refused("differ in k", other_k)
    refused("differ in k", b, out=T.TSXHashMapHIP(18, 0, 29))
    canon = counted(tb, k, canonical=True)[0]
    refused("canonical", canon)
    refused("canonical", b, out=T.TSXHashMapHIP(18, 0, k, canonical=True))
    refused("base rule", b, out=T.TSXHashMapHIP(18, 0, k, acgt_only=True))
    shard = T.TSXHashMapHIP(17, 0, k, shard_bits=1, shard_index=0)
    refused("shard", shard)
    refused("shard", b, out=shard)
    refused("lower > upper", b, a_range=(5, 4))
    refused("lower > upper", b, b_range=(0, 0))
    refused("unknown op", b, op=4)
    refused("unknown op", b, op=-1)
    refused("count mode", b, counts=5)
    assert a.compare(b)["both"] > 0   # the maps are still usable
    assert T.lib().tsx_hip_combine(None, None, b.handle, None, None) == T.EINVAL


def test_out_too_small_is_efull_and_clear_recovers(monkeypatch):
    import tsxcount_amd as T
    k = 31
    ta, tb = synth_pair(4, 30, 15)
    a, da = counted(ta, k)
    b, db = counted(tb, k)
    for path in ("1", "2"):
        monkeypatch.setenv("TSX_HIP_COMBINE_PATH", path)
        small = T.TSXHashMapHIP(10, 0, k, hash_seed=1)
        assert len(da) > 1024
        with pytest.raises(T.TSXException) as e:
            a.combine(b, "union", "max", out=small)
        assert e.value.code == T.EFULL
        small.clear()
        want, want_st = combine_expect(da, db, "intersect", "min", a_range=(30, None))
        assert 0 < len(want) < 512
        a.combine(b, "intersect", "min", a_range=(30, None), out=small)
        check_result(small, want, want_st)
        small.close()
    a.close(); b.close()


@pytest.mark.parametrize("k", [31, 127])
def test_small_staging_chunks(monkeypatch, k):
    ta, tb = synth_pair(k + 2, 16, 8)
    a, da = counted(ta, k, l=16, hash_seed=1)
    b, db = counted(tb, k, l=17, hash_seed=2)
    monkeypatch.setenv("TSX_HIP_COMBINE_CHUNK_BYTES", "4096")   # 64 .. 256 slots per chunk: hundreds of chunks
    for op, mode in (("union", "sum"), ("intersect", "min"), ("subtract", "min"), ("diff", "min")):
        want, want_st = combine_expect(da, db, op, mode)
        for out_kw in ({}, {"iL": 18, "hash_seed": 5}):
            out = a.combine(b, op, mode, **out_kw)
            check_result(out, want, want_st)
            out.close()
    a.close(); b.close()


def test_larger_tables_by_identities(monkeypatch):
    import tsxcount_amd as T
    rng = np.random.default_rng(12)
    n = 1 << 23
    pool = rng.integers(0, 1 << 62, size=n + n // 2, dtype=np.uint64)
    a = T.TSXHashMapHIP(24, 0, 31, hash_seed=10)
    a.addKmers(pool[:n], rng.integers(1, 5, size=n, dtype=np.uint64))
    sa = a.stats()
    for name, (l, seed) in {"aligned": (24, 10), "general": (25, 11)}.items():
        b = T.TSXHashMapHIP(l, 0, 31, hash_seed=seed)
        b.addKmers(pool[n // 2:], rng.integers(1, 5, size=n, dtype=np.uint64))
        sb = b.stats()
        inter = a.combine(b, "intersect", "min")
        mx = a.combine(b, "intersect", "max")
        sub = a.combine(b, "subtract")
        left = a.combine(b, "intersect", "left")
        uni = a.combine(b, "union", "sum")
        st = inter.combine_stats
        assert st["a_in_range"] == sa["distinct"] and st["b_in_range"] == sb["distinct"] and st["both"] >= n // 2 - 16
        assert inter.stats()["distinct"] + sub.stats()["distinct"] == sa["distinct"]
        assert inter.stats()["count_sum"] + mx.stats()["count_sum"] == st["a_sum_both"] + st["b_sum_both"]
        assert uni.stats()["count_sum"] == sa["count_sum"] + sb["count_sum"]
        assert uni.stats()["distinct"] == sa["distinct"] + sb["distinct"] - st["both"]
        kk, cc = left.getAllKmers()
        assert len(cc) == st["both"] and np.array_equal(a.getKmerCounts(kk), cc)
        assert np.array_equal(np.minimum(cc, b.getKmerCounts(kk)), inter.getKmerCounts(kk))
        assert not sub.getKmerCounts(kk).any() and not b.getKmerCounts(sub.getAllKmers()[0]).any()
        for m in (b, inter, mx, sub, left, uni):
            m.close()
    a.close()


def test_result_read_by_the_independent_reader(tmp_path):
    k = 33
    ta, tb = synth_pair(31, 16, 8)
    a, da = counted(ta, k, s=4)
    b, db = counted(tb, k, s=4)
    out = a.combine(b, "union", "sum", **CUT)
    p = str(tmp_path / "out.db")
    out.saveDatabase(p)
    f = kmerdb.read_db(p, out.hash_rows())
    want, want_st = combine_expect(da, db, "union", "sum", **CUT)
    assert f.kmers == want
    assert f.header["distinct"] == len(want) and f.header["count_sum"] == f.header["kmers_added"] == want_st["out_count_sum"]
    for m in (a, b, out):
        m.close()


def read_counts(path):
    d = {}
    for line in open(path, "rb"):
        x, c = line.rstrip(b"\n").split(b"\t")
        d[x] = int(c)
    return d


def test_cli_end_to_end(tmp_path, golden_fastq):
    import tsxcount_amd as T
    k = 14
    ta, tb = golden_pair(golden_fastq)
    fa, fb = tmp_path / "a.fastq", tmp_path / "b.fastq"
    fa.write_bytes(ta)
    fb.write_bytes(tb)
    da, db = dict(python_counts(ta, k)), dict(python_counts(tb, k))
    dba, dbb = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    for f, d in ((fa, dba), (fb, dbb)):
        rc, _, err = run_cli("--input=%s" % f, "--k=14", "--l=18", "--save=%s" % d)
        assert rc == 0, err
    # subtract: --output and --save see the result
    o, so = str(tmp_path / "sub.count"), str(tmp_path / "sub.db")
    rc, out, err = run_cli("--load=%s" % dba, "--with=%s" % dbb, "--op=subtract", "--output=%s" % o, "--save=%s" % so)
    assert rc == 0, err
    want, want_st = combine_expect(da, db, "subtract")
    assert read_counts(o) == want
    m = T.TSXHashMapHIP.fromDatabase(so)
    assert table_dict(m) == want and m.stats()["kmers_added"] == want_st["out_count_sum"]
    m.close()
    assert "subtract: %d different kmers" % len(want) in out
    # intersect of counted reads with a database, ranges and a count mode, into a histogram
    h = str(tmp_path / "i.histo")
    rc, _, err = run_cli("--input=%s" % fa, "--k=14", "--l=19", "--with=%s" % dbb, "--op=intersect", "--op-count=sum",
                         "--a-lower=2", "--b-upper=3", "--histo=%s" % h, "--histo-max=50")
    assert rc == 0, err
    want, _ = combine_expect(da, db, "intersect", "sum", a_range=(2, None), b_range=(1, 3))
    hist = {}
    for c in want.values():
        hist[min(c, 51)] = hist.get(min(c, 51), 0) + 1
    got = {int(x.split()[0]): int(x.split()[1]) for x in open(h)}
    assert {c: v for c, v in got.items() if v} == hist
    # several --with databases are summed; union / max
    o = str(tmp_path / "u.count")
    rc, _, err = run_cli("--load=%s" % dba, "--with=%s,%s" % (dbb, dba), "--op=union", "--op-count=max", "--output=%s" % o)
    assert rc == 0, err
    both = {x: da.get(x, 0) + db.get(x, 0) for x in set(da) | set(db)}
    assert read_counts(o) == combine_expect(da, both, "union", "max")[0]
    # --compare alone: the table stays A
    o = str(tmp_path / "c.count")
    rc, out, err = run_cli("--load=%s" % dba, "--with=%s" % dbb, "--compare", "--b-lower=2", "--output=%s" % o)
    assert rc == 0, err
    _, st = combine_expect(da, db, "intersect", "min", b_range=(2, None))
    line = [x for x in out.splitlines() if x.startswith("compare\t")][0].split("\t")
    assert [int(x) for x in line[1:4]] == [st["a_in_range"], st["b_in_range"], st["both"]]
    assert float(line[4]) == pytest.approx(jaccard(st), rel=1e-4)
    sums = [x for x in out.splitlines() if x.startswith("compare-sums\t")][0].split("\t")
    assert [int(x) for x in sums[1:]] == [st["a_sum_both"], st["b_sum_both"]]
    assert read_counts(o) == da
    # a database counted in another mode: refused by its header
    rc, _, err = run_cli("--load=%s" % dba, "--with=%s" % dbb, "--op=union", "--canonical")
    assert rc != 0
