"""The joint spectrum of two tables on the GPU: tsx_hip_joint_histogram_* through Python, its refusals and the CLI.

The reference is tsxcount_amd.joint_histogram (numpy on the CPU) over the two tables' own dumps (getAllKmers -> dict);
the whole matrix is compared for equality.  The larger pair is checked by identities against entry points that existed
before (getCountHistogram, compare)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, python_counts
import kmerdb

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
BINS = [(3, 200), (65, 65), (1002, 1002), (2, 2)]   # narrower than the LDS corner one way, one past it, the default, the least


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


def counted(text, k, l=18, s=0, **kw):
    import tsxcount_amd as T
    m = T.TSXHashMapHIP(l, s, k, **kw)
    m.countFastq(text)
    return m


def from_dict(d, k, l=16, s=0, **kw):
    import tsxcount_amd as T
    m = T.TSXHashMapHIP(l, s, k, **kw)
    if d:
        names = sorted(d)
        m.addKmers(kmerdb.kmers_to_limbs(names, k), np.array([d[x] for x in names], dtype=np.uint64))
    return m


def random_names(rng, n, k):
    names = kmerdb.limbs_to_kmers(rng.integers(0, 1 << 62, size=(n, (2 * k + 63) // 64), dtype=np.uint64), k)
    return sorted(set(names))


def check(a, b, da=None, db=None, bins=BINS):
    """a.jointHistogram(b) against the CPU statement over the dumps, for every bin pair; returns the largest matrix."""
    import tsxcount_amd as T
    da = table_dict(a) if da is None else da
    db = table_dict(b) if db is None else db
    best = None
    for na, nb in bins:
        got = a.jointHistogram(b, na, nb)
        want = T.joint_histogram(da, db, na, nb)
        assert got.dtype == np.uint64 and got.shape == (na, nb)
        assert np.array_equal(got, want), (na, nb, np.argwhere(got != want)[:5])
        assert got[0, 0] == 0
        if best is None or got.size > best.size:
            best = got
    return best


@pytest.mark.parametrize("k", [14, 31, 33, 63, 127])
def test_every_key_width(golden_fastq, k):
    ta, tb = golden_pair(golden_fastq)
    a, b = counted(ta, k, hash_seed=5), counted(tb, k, hash_seed=5)      # the aligned path
    b2 = counted(tb, k, l=19, s=6, hash_seed=6)                          # the general one
    da, db = table_dict(a), table_dict(b)
    assert table_dict(b2) == db and (k != 14 or da == dict(python_counts(ta, k)))
    assert set(da) & set(db) and set(da) - set(db) and set(db) - set(da)
    m = check(a, b, da, db, bins=[(1002, 1002), (3, 200)])
    assert m[1:, 0].sum() and m[0, 1:].sum() and m[1:, 1:].sum()    # A-only, B-only, shared
    check(a, b2, da, db, bins=[(65, 65)])
    check(b2, a, db, da, bins=[(2, 2)])
    for x in (a, b, b2):
        x.close()


@pytest.mark.parametrize("k", [14, 31, 64])
def test_canonical_tables(golden_fastq, k):
    ta, tb = golden_pair(golden_fastq) if k == 14 else synth_pair(k + 1)
    if k != 31:   # even k: palindromes among the k-mers
        pal = (b"ACGT" * 32)[:k // 2]
        pal += kmerdb.revcomp(pal)
        rec = b"@pal\n" + pal + b"AC" + b"\n+\n" + b"I" * (k + 2) + b"\n"
        ta, tb = ta + rec * 3, tb + rec
    a = counted(ta, k, canonical=True, hash_seed=2)
    b = counted(tb, k, canonical=True, hash_seed=3, l=19)   # the general path
    b2 = counted(tb, k, canonical=True, hash_seed=2)        # the aligned one
    da, db = table_dict(a), table_dict(b)
    assert da == kmerdb.fold_strands(python_counts(ta, k)) and db == table_dict(b2)
    m = check(a, b, da, db)
    if k != 31:
        assert da[pal] == 3 and db[pal] == 1 and m[3, 1] >= 1
    check(a, b2, da, db)
    for x in (a, b, b2):
        x.close()


def test_tables_with_a_base_rule():
    ta, tb = synth_pair(77, 20, 10)
    spoil = lambda t: t.replace(b"ACG", b"ANG", 40)
    ta, tb = spoil(ta), spoil(tb)
    a, b = counted(ta, 31, acgt_only=True), counted(tb, 31, acgt_only=True, hash_seed=4)
    da = table_dict(a)
    assert da == {x: c for x, c in python_counts(ta, 31).items() if set(x) <= set(b"ACGT")}
    check(a, b, da)
    a.close(); b.close()


def test_counts_in_the_corner_outside_it_and_in_the_last_bin():
    k = 31
    rng = np.random.default_rng(1)
    names = random_names(rng, 900, k)
    ladder = [1, 2, 3, 63, 64, 65, 66, 199, 200, 201, 1000, 1001, 1002, 5000]
    da = {x: ladder[i % len(ladder)] for i, x in enumerate(names[:600])}
    db = {x: ladder[(i // len(ladder)) % len(ladder)] for i, x in enumerate(names[300:])}
    for hs in (7, 8):   # aligned, general
        a, b = from_dict(da, k, hash_seed=7), from_dict(db, k, hash_seed=hs)
        assert table_dict(a) == da and table_dict(b) == db
        check(a, b, da, db, bins=BINS + [(64, 64), (70, 20), (20, 70)])
        m = a.jointHistogram(b, 20, 70)
        assert m[19, 0] and m[0, 69] and m[19, 69] and m[1, 1] and m[19, 1]   # (20, 70): pooled rows and columns
        a.close(); b.close()


def test_many_kmers_in_one_cell():
    """5000 k-mers at (1, 0) and 5000 at (1, 1): whole waves fold into one lane's add, and the corner is flushed."""
    k = 31
    names = random_names(np.random.default_rng(2), 10000, k)
    da = {x: 1 for x in names}
    db = {x: 1 for x in names[5000:]}
    for hs in (3, 4):
        a, b = from_dict(da, k, l=15, hash_seed=3), from_dict(db, k, l=15, hash_seed=hs)
        for na, nb in BINS:
            m = a.jointHistogram(b, na, nb)
            assert m[1, 0] == 5000 and m[1, 1] == len(names) - 5000 and m.sum() == len(names)
        m = b.jointHistogram(a, 65, 65)
        assert m[0, 1] == 5000 and m[1, 1] == len(names) - 5000 and m.sum() == len(names)
        a.close(); b.close()


@pytest.mark.parametrize("k", [31, 63])
def test_counts_that_carry(k):
    """Three storage bits: counts of 8 and more live in the secondary array."""
    rng = np.random.default_rng(k)
    names = random_names(rng, 600, k)
    big_a = {x: int(c) for x, c in zip(names[:450], rng.integers(1, 30, size=450))}
    big_b = {x: int(c) for x, c in zip(names[150:], rng.integers(1, 30, size=len(names) - 150))}
    small_a = {x: 1 + c % 7 for x, c in big_a.items()}
    small_b = {x: 1 + c % 7 for x, c in big_b.items()}
    for da, db in ((big_a, small_b), (small_a, big_b), (big_a, big_b), (small_a, small_b)):
        for hs in (8, 9):   # aligned, general
            a, b = from_dict(da, k, s=3, hash_seed=8), from_dict(db, k, s=3, hash_seed=hs)
            assert (a.stats()["overflow_used"] > 0) == (da is big_a) and (b.stats()["overflow_used"] > 0) == (db is big_b)
            assert table_dict(a) == da and table_dict(b) == db
            m = check(a, b, da, db, bins=[(65, 65), (8, 8), (9, 40)])
            assert (m[8, :].sum() > 0) == (da is big_a)
            a.close(); b.close()


def test_geometries_and_both_paths(monkeypatch):
    import tsxcount_amd as T
    k = 33
    ta, tb = synth_pair(9)
    a = counted(ta, k, l=18, hash_seed=4)
    others = {"aligned": counted(tb, k, l=18, hash_seed=4), "l": counted(tb, k, l=19, hash_seed=4),
              "seed": counted(tb, k, l=18, hash_seed=6), "bits": counted(tb, k, l=18, s=5, hash_seed=4)}
    da, db = table_dict(a), dict(python_counts(tb, k))
    want = T.joint_histogram(da, db, 65, 40)
    for name, b in others.items():
        for path in ("0", "1", "2"):
            monkeypatch.setenv("TSX_HIP_COMBINE_PATH", path)
            if path == "2" and name != "aligned":
                with pytest.raises(T.TSXException) as e:
                    a.jointHistogram(b, 65, 40)
                assert e.value.code == T.EINVAL and "aligned" in str(e.value)
                continue
            assert np.array_equal(a.jointHistogram(b, 65, 40), want), (name, path)
            assert np.array_equal(b.jointHistogram(a, 40, 65), want.T), (name, path)
    monkeypatch.setenv("TSX_HIP_COMBINE_PATH", "3")
    with pytest.raises(T.TSXException) as e:
        a.jointHistogram(others["aligned"], 65, 40)
    assert e.value.code == T.EINVAL
    monkeypatch.delenv("TSX_HIP_COMBINE_PATH")
    a.close()
    for b in others.values():
        b.close()


def test_same_table_is_its_histogram_on_the_diagonal():
    ta, _ = synth_pair(5, 16, 8)
    a = counted(ta * 5, 31, s=3)     # (every count is 5 or more: some carry)
    assert a.stats()["overflow_used"] > 0
    for na, nb in BINS + [(30, 12)]:
        m = a.jointHistogram(a, na, nb)
        h = a.getCountHistogram(max(na, nb))
        n = min(na, nb)
        want = np.zeros((na, nb), dtype=np.uint64)
        for c in range(1, len(h)):
            want[min(c, na - 1), min(c, nb - 1)] += h[c]
        assert np.array_equal(m, want)
        if na == nb:
            assert np.array_equal(np.diag(m)[1:], h[1:n]) and m.sum() == np.trace(m)
    a.close()


def test_empty_and_cleared_tables():
    import tsxcount_amd as T
    k = 31
    ta, tb = synth_pair(5, 16, 8)
    a, b = counted(ta, k), counted(tb, k, hash_seed=2)
    da, db = table_dict(a), table_dict(b)
    empty, empty2 = T.TSXHashMapHIP(18, 0, k), T.TSXHashMapHIP(17, 0, k, hash_seed=9)
    cleared = counted(tb, k)
    cleared.clear()   # (lazily: the call zeroes it before it reads)
    for e in (empty, empty2, cleared):
        check(a, e, da, {})
        check(e, b, {}, db)
        assert not e.jointHistogram(empty, 65, 65).any() and not empty.jointHistogram(e, 3, 200).any()
    assert cleared.stats()["distinct"] == 0
    cleared.countFastq(tb)          # and it is a table like any other afterwards
    check(a, cleared, da, db, bins=[(65, 65)])
    for m in (a, b, empty, empty2, cleared):
        m.close()


def test_inputs_unchanged(tmp_path, monkeypatch):
    k = 63
    ta, tb = synth_pair(15, 16, 8)
    a, b = counted(ta, k, s=3, hash_seed=1), counted(tb, k, s=3, hash_seed=1)
    image = lambda m, name: (m.saveDatabase(str(tmp_path / name)), open(str(tmp_path / name), "rb").read(), m.stats())[1:]
    before = image(a, "a0.db"), image(b, "b0.db")
    for path in ("1", "2"):
        monkeypatch.setenv("TSX_HIP_COMBINE_PATH", path)
        for na, nb in BINS:
            a.jointHistogram(b, na, nb)
        b.jointHistogram(a)
        a.jointHistogram(a)
    assert (image(a, "a1.db"), image(b, "b1.db")) == before
    a.close(); b.close()


def test_larger_tables_by_identities():
    import tsxcount_amd as T
    rng = np.random.default_rng(12)
    n = 300000
    pool = rng.integers(0, 1 << 62, size=n + n // 2, dtype=np.uint64)
    a = T.TSXHashMapHIP(20, 0, 31, hash_seed=10)
    a.addKmers(pool[:n], rng.integers(1, 90, size=n, dtype=np.uint64))
    na, nb = 100, 70
    ha = a.getCountHistogram(na)
    for l, seed in ((20, 10), (21, 11)):   # aligned, general
        b = T.TSXHashMapHIP(l, 0, 31, hash_seed=seed)
        b.addKmers(pool[n // 2:], rng.integers(1, 90, size=n, dtype=np.uint64))
        m = a.jointHistogram(b, na, nb)
        assert np.array_equal(m.sum(axis=1)[1:], ha[1:])
        assert np.array_equal(m.sum(axis=0)[1:], b.getCountHistogram(nb)[1:])
        both = a.compare(b)["both"]
        assert m[1:, 1:].sum() == both and both >= n // 2 - 16
        assert m[0, 0] == 0 and m[1:, 0].sum() == a.stats()["distinct"] - both
        assert m[0, 1:].sum() == b.stats()["distinct"] - both
        assert m[64:, 64:].sum() and m[:64, :64].sum() and m[64:, :64].sum() and m[:64, 64:].sum()
        b.close()
    a.close()


def test_device_form_on_the_maps_own_stream():
    import torch
    import tsxcount_amd as T
    k = 31
    ta, tb = synth_pair(6, 16, 8)
    a, b = counted(ta, k), counted(tb, k, hash_seed=3)
    na, nb = 70, 33
    buf = torch.full((na * nb,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda:0")   # garbage: the call zeroes it
    torch.cuda.synchronize()
    a.jointHistogramDevice(b, buf.data_ptr(), na, nb)     # queued on A's stream, not waited for
    a.sync()
    got = buf.cpu().numpy().view(np.uint64).reshape(na, nb)
    host = a.jointHistogram(b, na, nb)
    assert np.array_equal(got, host)
    assert np.array_equal(host, T.joint_histogram(table_dict(a), table_dict(b), na, nb))
    # on a caller's stream, and B changes right afterwards on its own stream: the sweeps saw B as it was
    st = torch.cuda.Stream(buf.device)
    buf.fill_(-1)
    torch.cuda.synchronize()
    a.jointHistogramDevice(b, buf.data_ptr(), na, nb, stream=st.cuda_stream)
    b.clear()
    st.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint64).reshape(na, nb), host)
    b.sync()
    a.close(); b.close()


def test_refusals():
    import tsxcount_amd as T
    k = 31
    ta, tb = synth_pair(3, 8, 4)
    a, b = counted(ta, k), counted(tb, k)

    def refused(what, other, *bins):
        with pytest.raises(T.TSXException) as e:
            a.jointHistogram(other, *bins)
        assert e.value.code == T.EINVAL and what in str(e.value), str(e.value)

    refused("differ in k", counted(tb, 29))
    refused("canonical", counted(tb, k, canonical=True))
    refused("base rule", counted(tb, k, acgt_only=True))
    refused("base rule", counted(tb, k, min_qual_char="5"))
    refused("shard", T.TSXHashMapHIP(17, 0, k, shard_bits=1, shard_index=0))
    refused("fewer than 2 bins", b, 1, 100)
    refused("fewer than 2 bins", b, 100, 1)
    refused("2^24", b, 4097, 4096)
    refused("2^24", b, 2, (1 << 23) + 1)
    L = T.lib()
    out = np.zeros(4, dtype=np.uint64)
    assert L.tsx_hip_joint_histogram_host(a.handle, None, T._p(out), 2, 2) == T.EINVAL
    assert L.tsx_hip_joint_histogram_host(a.handle, b.handle, None, 2, 2) == T.EINVAL
    assert L.tsx_hip_joint_histogram_device(a.handle, b.handle, 2, 2, None, None) == T.EINVAL
    assert a.jointHistogram(b, 4096, 4096).sum() == len(set(table_dict(a)) | set(table_dict(b)))   # 2^24 cells are allowed
    a.close(); b.close()


def test_cli_end_to_end(tmp_path, golden_fastq):
    import tsxcount_amd as T
    k = 14
    ta, tb = golden_pair(golden_fastq)
    fa, fb = tmp_path / "a.fastq", tmp_path / "b.fastq"
    fa.write_bytes(ta)
    fb.write_bytes(tb)
    da, db = dict(python_counts(ta, k)), dict(python_counts(tb, k))
    dba, dbb = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    for f, d, l in ((fa, dba, 18), (fb, dbb, 19)):   # (B of another l: the general path)
        rc, _, err = run_cli("--input=%s" % f, "--k=14", "--l=%d" % l, "--save=%s" % d)
        assert rc == 0, err

    def joint_line(out, m):
        line = [x for x in out.splitlines() if x.startswith("joint\t")]
        assert len(line) == 1
        assert [int(x) for x in line[0].split("\t")[1:]] == [int(m[1:, 0].sum()), int(m[0, 1:].sum()), int(m[1:, 1:].sum())]

    # sparse (the default), default H = 1000: 1002 bins a side
    js = str(tmp_path / "j.tsv")
    rc, out, err = run_cli("--load=%s" % dba, "--with=%s" % dbb, "--joint-histo=%s" % js)
    assert rc == 0, err
    want = T.joint_histogram(da, db, 1002, 1002)
    rows = [tuple(int(x) for x in line.split("\t")) for line in open(js)]
    assert rows == sorted(rows) and len(set(r[:2] for r in rows)) == len(rows) and all(r[2] > 0 for r in rows)
    got = np.zeros_like(want)
    for i, j, n in rows:
        got[i, j] = n
    assert np.array_equal(got, want)
    joint_line(out, want)
    assert set(da) - set(db) and want[1:, 0].sum() == len(set(da) - set(db))    # a_only is what only A holds
    # matrix, H per side, next to --compare and --op on counted reads: the matrix is of A and B, not of the result
    jm, o = str(tmp_path / "j.mat"), str(tmp_path / "i.count")
    rc, out, err = run_cli("--input=%s" % fa, "--k=14", "--l=19", "--with=%s" % dbb, "--joint-histo=%s" % jm, "--joint-format=matrix",
                           "--joint-max-a=5", "--joint-max-b=70", "--compare", "--op=intersect", "--output=%s" % o)
    assert rc == 0, err
    want = T.joint_histogram(da, db, 7, 72)
    lines = open(jm).read().splitlines()
    assert lines[0] == "# rows: count in A 0..6, columns: count in B" and len(lines) == 8
    got = np.array([[int(x) for x in line.split("\t")] for line in lines[1:]], dtype=np.uint64)
    assert got.shape == (7, 72) and np.array_equal(got, want)
    joint_line(out, want)
    assert any(x.startswith("compare\t") for x in out.splitlines())
    assert sum(1 for _ in open(o)) == want[1:, 1:].sum()
    # canonical tables, the base rule given to both
    for f, d in ((fa, dba), (fb, dbb)):
        rc, _, err = run_cli("--input=%s" % f, "--k=14", "--l=18", "--canonical", "--acgt-only", "--min-qual-char=#", "--save=%s" % d)
        assert rc == 0, err
    rc, out, err = run_cli("--load=%s" % dba, "--with=%s" % dbb, "--canonical", "--acgt-only", "--min-qual-char=#",
                           "--joint-histo=%s" % js, "--joint-max-a=30", "--joint-max-b=30")
    assert rc == 0, err
    a, b = T.TSXHashMapHIP.fromDatabase(dba), T.TSXHashMapHIP.fromDatabase(dbb)
    want = a.jointHistogram(b, 32, 32)
    assert a.canonical and np.array_equal(want, T.joint_histogram(table_dict(a), table_dict(b), 32, 32))
    got = np.zeros_like(want)
    for line in open(js):
        i, j, n = (int(x) for x in line.split("\t"))
        got[i, j] = n
    assert np.array_equal(got, want)
    joint_line(out, want)
    a.close(); b.close()
