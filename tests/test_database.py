"""K-mer database files: tsx_hip_db_read_info, tsx_hip_save_host, tsx_hip_load_host (direct placement and the re-insert
path), through the C ABI, Python and the tsxCount CLI.

Every expectation is a table counted the ordinary way (or python_counts): a loaded or merged table must dump exactly
what counting the same reads into one table dumps."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, python_counts
from kmerdb import fnv1a64 as fnv, pack_header as header   # the header built from the format description

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
GOLDEN_FASTQ = os.path.join(GOLDEN, "small_t7.1000.fastq")


def run_cli(*args, timeout=300):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


# ---- CPU --------------------------------------------------------------------------------------------------------------

def test_header_fields_read_back(tmp_path):
    import tsxcount_amd as T
    p = tmp_path / "h.db"
    p.write_bytes(header(k=33, l=22, W=2, F=44, R=8, C=19, S=13, ol=18, seed=12345, canonical=1, acgt=1, minq=53,
                         added=77, distinct=55, count_sum=70, carries=3))
    d = T.database_info(str(p))
    assert d == {"version": 1, "k": 33, "l": 22, "entry_limbs": 2, "func_bits": 44, "reprobe_bits": 8, "count_bits": 19,
                 "seg_bits": 13, "overflow_l": 18, "canonical": 1, "acgt_only": 1, "min_qual_char": 53, "hash_seed": 12345,
                 "kmers_added": 77, "distinct": 55, "count_sum": 70, "carry_records": 3}
    fd = os.open(str(p), os.O_RDONLY)
    try:
        os.lseek(fd, 50, os.SEEK_SET)   # pread at offset 0: the position does not matter
        assert T.database_info(fd)["k"] == 33
    finally:
        os.close(fd)


@pytest.mark.parametrize("damage", ["magic", "version", "flip", "short", "empty"])
def test_bad_headers_are_format_errors(tmp_path, damage):
    import tsxcount_amd as T
    h = bytearray(header())
    if damage == "magic":
        h[0:8] = b"NOTADB!!"
    elif damage == "version":
        h[8] = 2
        h[120:128] = struct.pack("<Q", fnv(bytes(h[:120])))   # a well-formed header of another version
    elif damage == "flip":
        h[20] ^= 0x01
    elif damage == "short":
        h = h[:100]
    else:
        h = b""
    p = tmp_path / "bad.db"
    p.write_bytes(bytes(h))
    with pytest.raises(T.TSXException) as e:
        T.database_info(str(p))
    assert e.value.code == T.EFORMAT


def test_database_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in ("tsx_hip_db_read_info", "tsx_hip_save_host", "tsx_hip_load_host"):
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "tsx_hip_db_info" in hdr and "TSX_HIP_EFORMAT = -10" in hdr
    assert b"database" in L.tsx_hip_strerror(T.EFORMAT)


def test_cli_usage_lists_save_and_load():
    rc, _, err = run_cli("--help")
    assert rc != 0
    assert "--save=DB" in err and "--load=DB" in err


def test_cli_load_refuses_mismatched_mode_without_gpu(tmp_path):
    p = tmp_path / "h.db"
    p.write_bytes(header(k=14, l=20, F=8, C=4, canonical=1))
    rc, _, err = run_cli("--load=%s" % p, "--output=%s" % (tmp_path / "o"))
    assert rc != 0 and "--canonical" in err
    rc, _, err = run_cli("--load=%s" % (tmp_path / "missing.db"), "--canonical")
    assert rc != 0


# ---- GPU --------------------------------------------------------------------------------------------------------------

def sorted_dump(m):
    k, c = m.getAllKmers()
    if len(c) == 0:
        return k, c
    o = np.lexsort(k.T[::-1])
    return k[o], c[o]


def assert_same_table(a, b, stats=("distinct", "count_sum", "kmers_added")):
    ka, ca = sorted_dump(a)
    kb, cb = sorted_dump(b)
    assert np.array_equal(ka, kb) and np.array_equal(ca, cb)
    sa, sb = a.stats(), b.stats()
    for f in stats:
        assert sa[f] == sb[f], (f, sa, sb)


def synth_text(seed, n):
    from tsxcount_amd import synth
    return synth.fastq(seed, 0, n)


def repeated(text, times):
    recs = [l for l in text.split(b"\n") if l]
    out = []
    for i in range(0, len(recs), 4):
        out += recs[i:i + 4] * (1 + (i // 4) % times)
    return b"\n".join(out) + b"\n"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [14, 31, 33, 63, 127])
def test_round_trip(tmp_path, golden_fastq, k):
    import tsxcount_amd as T
    text = golden_fastq if k == 14 else synth_text(k, 40)
    m = T.TSXHashMapHIP(20, 0, k, hash_seed=99)
    m.countFastq(text)
    db = str(tmp_path / "a.db")
    entries, nbytes = m.saveDatabase(db)
    assert entries == m.stats()["distinct"] and nbytes == os.path.getsize(db)
    info = T.database_info(db)
    assert info["k"] == k and info["hash_seed"] == 99 and info["distinct"] == entries
    m2 = T.TSXHashMapHIP.fromDatabase(db)
    assert_same_table(m, m2)
    for f, _ in T.Layout._fields_:
        assert getattr(m.layout, f) == getattr(m2.layout, f), f
    if k == 14:
        want = python_counts(text, 14)
        kk, cc = m2.getAllKmers()
        assert {T.decode(x, 14).encode(): int(c) for x, c in zip(kk, cc)} == dict(want)
    m.close(); m2.close()


@pytest.mark.gpu
def test_overflow_carries_direct_and_reinsert(tmp_path):
    import tsxcount_amd as T
    text = repeated(synth_text(5, 15), 9)
    m = T.TSXHashMapHIP(18, 2, 31)
    m.countFastq(text)
    assert m.stats()["overflow_used"] > 0
    db = str(tmp_path / "c.db")
    m.saveDatabase(db)
    assert T.database_info(db)["carry_records"] == m.stats()["overflow_used"]
    direct = T.TSXHashMapHIP.fromDatabase(db)
    assert_same_table(m, direct)
    for l, s in ((19, 2), (18, 3), (20, 0)):
        re = T.TSXHashMapHIP.fromDatabase(db, iL=l, iStorageBits=s)
        assert_same_table(m, re)
        re.close()
    want = python_counts(text, 31)
    kk, cc = direct.getAllKmers()
    assert sorted(int(c) for c in cc) == sorted(want.values())
    m.close(); direct.close()


@pytest.mark.gpu
def test_canonical_and_base_rule_round_trip(tmp_path):
    import tsxcount_amd as T
    text = synth_text(8, 40)
    recs = text.split(b"\n")
    recs[1] = recs[1][:30] + b"N" + recs[1][31:]   # a non-ACGT byte for the base rule
    text = b"\n".join(recs)
    for kw, other in (({"canonical": True}, {"canonical": False}),
                      ({"acgt_only": True}, {}),
                      ({"min_qual_char": "&"}, {"min_qual_char": "'"})):
        m = T.TSXHashMapHIP(18, 0, 31, hash_seed=3, **kw)
        m.countFastq(text)
        db = str(tmp_path / "r.db")
        m.saveDatabase(db)
        m2 = T.TSXHashMapHIP.fromDatabase(db)
        assert m2.canonical == m.canonical and m2.base_rule == m.base_rule
        assert_same_table(m, m2)
        m3 = T.TSXHashMapHIP(18, 0, 31, hash_seed=3, **other)
        with pytest.raises(T.TSXException) as e:
            m3.addDatabase(db)
        assert e.value.code == T.EINVAL
        m.close(); m2.close(); m3.close()


@pytest.mark.gpu
def test_geometry_change_reinserts(tmp_path):
    import tsxcount_amd as T
    text = synth_text(21, 50)
    m = T.TSXHashMapHIP(20, 0, 31, hash_seed=4)
    m.countFastq(text)
    db = str(tmp_path / "g.db")
    m.saveDatabase(db)
    big = T.TSXHashMapHIP.fromDatabase(db, iL=22)
    assert big.layout.l == 22
    assert_same_table(m, big)
    other_seed = T.TSXHashMapHIP(20, 0, 31, hash_seed=5)   # same geometry, another seed: re-insert too
    other_seed.addDatabase(db)
    assert_same_table(m, other_seed)
    m.close(); big.close(); other_seed.close()


@pytest.mark.gpu
def test_merge_equals_counting_both(tmp_path):
    import tsxcount_amd as T
    a, b = synth_text(31, 40), repeated(synth_text(32, 40), 3) + synth_text(31, 10)
    dbs = []
    for name, text in (("a", a), ("b", b)):
        m = T.TSXHashMapHIP(19, 4, 31, hash_seed=6)
        m.countFastq(text)
        dbs.append(str(tmp_path / (name + ".db")))
        m.saveDatabase(dbs[-1])
        m.close()
    both = T.TSXHashMapHIP(19, 4, 31, hash_seed=6)
    both.countFastq(a + b)
    m = T.TSXHashMapHIP.fromDatabase(dbs[0])   # direct, then re-insert
    m.addDatabase(dbs[1])
    assert_same_table(both, m)
    m2 = T.TSXHashMapHIP(20, 0, 31, hash_seed=6)   # two re-inserts
    m2.addDatabase(dbs[0])
    m2.addDatabase(dbs[1])
    assert_same_table(both, m2)
    both.close(); m.close(); m2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cleared", [False, True])
def test_incremental_count_on_loaded_table(tmp_path, cleared):
    import tsxcount_amd as T
    a, b = synth_text(41, 60), synth_text(42, 60) + synth_text(41, 20)
    ma = T.TSXHashMapHIP(18, 0, 31, hash_seed=2)
    ma.countFastq(a)
    db = str(tmp_path / "a.db")
    ma.saveDatabase(db)
    both = T.TSXHashMapHIP(18, 0, 31, hash_seed=2)
    both.countFastq(a + b)
    m = T.TSXHashMapHIP(18, 0, 31, hash_seed=2)
    if cleared:   # a lazily cleared table (the partitioned build would write every segment)
        m.countFastq(b)
        m.clear()
    m.addDatabase(db)
    m.set_path("partitioned")
    m.countFastq(b)
    assert_same_table(both, m)
    ma.close(); both.close(); m.close()


def chunk_heads(path):
    """(slot_lo, slot_hi, n_entries) of every chunk of a database file, the end marker last."""
    import tsxcount_amd as T
    info = T.database_info(path)
    W = info["entry_limbs"]
    out = []
    with open(path, "rb") as f:
        f.seek(128 + info["carry_records"] * (2 + W) * 8)
        while True:
            lo, hi, n, _ = struct.unpack("<4Q", f.read(32))
            out.append((lo, hi, n))
            if lo == hi:
                return out
            f.seek(((hi - lo + 63) // 64 + n * W) * 8, os.SEEK_CUR)


@pytest.mark.gpu
def test_small_chunks_and_seams(tmp_path):
    import tsxcount_amd as T
    rng = np.random.default_rng(3)
    for fill in ("text", "sparse"):
        m = T.TSXHashMapHIP(14, 0, 31, hash_seed=8)
        if fill == "text":
            m.countFastq(synth_text(51, 3))
        else:
            m.addKmers(rng.integers(0, 1 << 62, size=24, dtype=np.uint64), rng.integers(1, 9, size=24, dtype=np.uint64))
        db = str(tmp_path / ("s_%s.db" % fill))
        m.saveDatabase(db, chunk_bytes=4096)
        heads = chunk_heads(db)
        assert len(heads) >= 30 and heads[-1] == (1 << 14, 1 << 14, 0)
        assert sum(n for _, _, n in heads) == m.stats()["distinct"]
        if fill == "sparse":
            assert any(n == 0 for _, _, n in heads[:-1])
        for kw in ({}, {"iL": 15}):
            m2 = T.TSXHashMapHIP.fromDatabase(db, chunk_bytes=4096, **kw)
            assert_same_table(m, m2)
            m2.close()
        m.close()


@pytest.mark.gpu
def test_large_table_round_trip(tmp_path):
    import tsxcount_amd as T
    rng = np.random.default_rng(11)
    n = 1 << 23
    kmers = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    counts = rng.integers(1, 5, size=n, dtype=np.uint64)
    m = T.TSXHashMapHIP(24, 0, 31, hash_seed=10)
    m.addKmers(kmers, counts)
    assert m.stats()["distinct"] >= n - 16
    db = str(tmp_path / "big.db")
    m.saveDatabase(db, chunk_bytes=4 << 20)
    m2 = T.TSXHashMapHIP.fromDatabase(db, chunk_bytes=4 << 20)
    assert_same_table(m, m2)
    m.close(); m2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["entry", "truncate", "bitmap"])
def test_damaged_database_is_a_format_error(tmp_path, damage):
    import tsxcount_amd as T
    text = synth_text(61, 30)
    m = T.TSXHashMapHIP(16, 0, 31, hash_seed=1)
    m.countFastq(text)
    db = str(tmp_path / "d.db")
    m.saveDatabase(db)
    info = T.database_info(db)
    assert info["entry_limbs"] == 1
    raw = bytearray(open(db, "rb").read())
    bm0 = 128 + info["carry_records"] * 3 * 8 + 32   # one chunk: header, carry records, chunk head, bitmap, entries
    ent0 = bm0 + (1 << 16) // 64 * 8
    if damage == "entry":
        raw[ent0 + 8 * 5 + 3] ^= 0x10
    elif damage == "bitmap":
        raw[bm0 + 40] ^= 0x01
    else:
        raw = raw[:-32]   # no end marker
    open(db, "wb").write(bytes(raw))
    m2 = T.TSXHashMapHIP(16, 0, 31, hash_seed=1)
    with pytest.raises(T.TSXException) as e:
        m2.addDatabase(db)
    assert e.value.code == T.EFORMAT
    m2.clear()
    m2.countFastq(text)
    assert_same_table(m, m2)
    m.close(); m2.close()


def sorted_lines(path):
    return sorted(open(path, "rb").read().split(b"\n"))


@pytest.mark.gpu
def test_cli_save_load(tmp_path, golden_fastq):
    recs = [l for l in golden_fastq.split(b"\n") if l]
    half = (len(recs) // 8) * 4
    fa, fb = tmp_path / "a.fastq", tmp_path / "b.fastq"
    fa.write_bytes(b"\n".join(recs[:half]) + b"\n")
    fb.write_bytes(b"\n".join(recs[half:]) + b"\n")
    t = lambda name: str(tmp_path / name)
    common = ["--k=14", "--l=20"]

    def ok(*args):
        rc, out, err = run_cli(*args)
        assert rc == 0, (args, out, err)

    ok("--input=" + GOLDEN_FASTQ, *common, "--save=" + t("g.db"), "--output=" + t("g.count"), "--histo=" + t("g.histo"),
       "--filter=" + t("g.filter"))
    ok("--load=" + t("g.db"), "--output=" + t("l.count"), "--histo=" + t("l.histo"), "--filter-input=" + GOLDEN_FASTQ,
       "--filter=" + t("l.filter"))
    assert sorted_lines(t("g.count")) == sorted_lines(t("l.count"))
    assert open(t("g.histo"), "rb").read() == open(t("l.histo"), "rb").read()
    assert open(t("g.filter"), "rb").read() == open(t("l.filter"), "rb").read()
    # the whole golden count, through the database
    want = python_counts(golden_fastq, 14)
    got = dict(ln.split(b"\t") for ln in open(t("l.count"), "rb").read().split(b"\n") if ln)
    assert {k: int(v) for k, v in got.items()} == dict(want)

    ok("--input=" + str(fa), *common, "--save=" + t("a.db"))
    ok("--input=" + str(fb), *common, "--save=" + t("b.db"))
    ok("--load=%s,%s" % (t("a.db"), t("b.db")), "--output=" + t("ab.count"))
    assert sorted_lines(t("ab.count")) == sorted_lines(t("g.count"))
    ok("--load=" + t("a.db"), "--input=" + str(fb), "--output=" + t("inc.count"))
    assert sorted_lines(t("inc.count")) == sorted_lines(t("g.count"))
    ok("--load=" + t("a.db"), "--l=21", "--s=0", "--input=" + str(fb), "--output=" + t("inc2.count"))
    assert sorted_lines(t("inc2.count")) == sorted_lines(t("g.count"))

    rc, _, err = run_cli("--load=" + t("g.db"), "--check")
    assert rc != 0 and "--check" in err
    rc, _, err = run_cli("--load=" + t("g.db"), "--gpus=2", "--output=" + t("x"))
    assert rc != 0 and "one GPU" in err
    rc, _, err = run_cli("--input=" + GOLDEN_FASTQ, *common, "--gpus=2", "--save=" + t("x.db"))
    assert rc != 0
    rc, _, err = run_cli("--load=" + t("g.db"), "--filter=" + t("y"))
    assert rc != 0 and "--filter-input" in err
