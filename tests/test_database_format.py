"""The k-mer database format pinned from outside the library: files the library saves are read with tests/kmerdb.py (the
format text restated in Python), and files kmerdb.py writes are loaded by the library, both ways (direct placement and
the re-insert path).  Malformed files with valid checksums must be format errors on both paths.

Expectations come from python_counts, the mapping's rows and the format text, never from another table."""
import os

import numpy as np
import pytest

import kmerdb as K
from conftest import GOLDEN, python_counts

SEED = 77
# k, l, s, key limbs, W, C: every row is a derive_layout result (checked against the library's layout on the GPU)
MATRIX = [
    (5, 4, 0, 1, 1, 32), (5, 5, 0, 1, 1, 32), (5, 6, 0, 1, 1, 32),     # 16 / 32 / 64 slots: one partial bitmap word
    (14, 20, 0, 1, 1, 32),     # 16 unused bits in limb 0 (golden FASTQ)
    (31, 16, 2, 1, 1, 2),      # carries, W = 1
    (31, 20, 16, 1, 2, 16),    # W > key limbs
    (33, 20, 0, 2, 1, 10),     # W < key limbs
    (63, 20, 0, 2, 2, 13),     # func bits spill exactly one whole limb
    (63, 18, 2, 2, 2, 2),      # carries, W = 2
    (63, 20, 32, 2, 3, 32),    # W = 3 > key limbs
    (65, 20, 0, 3, 2, 9),      # key limbs 3, W = 2
    (80, 20, 0, 3, 3, 32),     # unused bits in the last limb
    (96, 18, 2, 3, 3, 2),      # carries, W = 3
    (96, 20, 32, 3, 4, 32),    # W = 4 > key limbs
    (97, 20, 0, 4, 3, 9),      # key limbs 4, W = 3
    (127, 16, 2, 4, 4, 2),     # carries, W = 4
]
IDS = ["k%d-l%d-s%d" % r[:3] for r in MATRIX]
FIXTURE = os.path.join(GOLDEN, "small_t7.first8.k14.v1.db")


def layout_of(row):
    k, l, s, kl, W, C = row
    lay = K.Layout(k, l, s)
    assert (lay.key_limbs, lay.W, lay.C) == (kl, W, C), lay
    return lay


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", MATRIX, ids=IDS)
def test_header_reads_back(tmp_path, row):
    import tsxcount_amd as T
    lay = layout_of(row)
    carry = np.arange(3 * (2 + lay.W), dtype=np.uint64).tobytes()
    b = K.header_for(lay, 0xFEDCBA9876543210, 1234567, 890, 4321, carry, 3, canonical=1, acgt=1, minq=40)
    p = tmp_path / "h.db"
    p.write_bytes(b)
    assert T.database_info(str(p)) == {
        "version": 1, "k": lay.k, "l": lay.l, "entry_limbs": lay.W, "func_bits": lay.F, "reprobe_bits": lay.R,
        "count_bits": lay.C, "seg_bits": lay.S, "overflow_l": lay.overflow_l, "canonical": 1, "acgt_only": 1,
        "min_qual_char": 40, "hash_seed": 0xFEDCBA9876543210, "kmers_added": 1234567, "distinct": 890,
        "count_sum": 4321, "carry_records": 3}
    h = K.parse_header(b)
    assert h["carry_fnv"] == K.fnv1a64(carry) and h["seg_bits"] == lay.S and h["count_bits"] == lay.C


def test_checksum_vectors():
    # FNV-1a 64 (the published test vectors) and the splitmix64 finalizer (the outputs of splitmix64 seeded with 0)
    assert K.fnv1a64(b"") == 0xCBF29CE484222325
    assert K.fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    assert K.fnv1a64(b"foobar") == 0x85944171F73967E8
    g = 0x9E3779B97F4A7C15
    got = K.mix64(np.array([g, 2 * g & K.M64, 3 * g & K.M64], dtype=np.uint64))
    assert got.tolist() == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert K.mix64(0).tolist() == [0]
    # the chunk terms, by hand for one bitmap word and one two-word entry
    m = lambda v: int(K.mix64(v)[0])
    assert K.bitmap_terms(5, [0x11]) == m(m(5 ^ K.SALT_BM) ^ 0x11)
    assert K.entry_terms([70], [[3, 9]]) == m(m(m(70 ^ K.SALT_E) ^ 3) ^ 9)
    assert K.bitmap_terms(0, [1, 2]) == (K.bitmap_terms(0, [1]) + K.bitmap_terms(1, [2])) & K.M64


@pytest.mark.parametrize("row", MATRIX, ids=IDS)
def test_slot_encoding_round_trips(row):
    lay = layout_of(row)
    rng = np.random.default_rng(row[0] * 1000 + row[1])
    for _ in range(300):
        key = int.from_bytes(rng.bytes(32), "little") & ((1 << (2 * lay.k)) - 1)
        i = int(rng.integers(1, lay.max_reprobes + 1))
        c = int(rng.integers(0, 1 << lay.C))
        pos = lay.probe(lay.home(key), i)
        words = K.encode_slot(lay, key, i, c)
        assert len(words) == lay.W and all(0 <= w <= K.M64 for w in words)
        assert K.decode_slot(lay, pos, words) == (key, i, c, [0] * lay.W)
        assert words[0] & lay.lock_bit == 0
    # every bit outside the fields is reported, in the limb it sits in
    for t, msk in enumerate(lay.masks):
        free = [b for b in range(64) if not (msk >> b) & 1]
        if free:
            key = 12345 % (1 << (2 * lay.k))
            words = K.encode_slot(lay, key, 1, 1)
            words[t] |= 1 << free[-1]
            assert K.decode_slot(lay, lay.probe(lay.home(key), 1), words)[3][t] == 1 << free[-1]


def test_inverse_rows_invert():
    rng = np.random.default_rng(5)
    for k in (5, 31, 33, 97):
        n, wk = 2 * k, (2 * k + 63) // 64
        while True:   # a random invertible matrix
            rows = np.frombuffer(rng.bytes(8 * n * wk), dtype=np.uint64).reshape(n, wk).copy()
            rows[:, -1] &= np.uint64((1 << (n % 64 or 64)) - 1)
            try:
                inv = K.inverse_rows(rows, k)
                break
            except ValueError:
                continue
        x = K.kmers_to_limbs([bytes(rng.choice(list(b"ACGT"), k).tolist()) for _ in range(50)], k)
        assert np.array_equal(K.hash_keys(inv, K.hash_keys(rows, x, k), k), x)


# ---- GPU helpers --------------------------------------------------------------------------------------------------------

def synth_text(seed, n):
    from tsxcount_amd import synth
    return synth.fastq(seed, 0, n)


def repeated(text, times):
    recs = [ln for ln in text.split(b"\n") if ln]
    out = []
    for i in range(0, len(recs), 4):
        out += recs[i:i + 4] * (1 + (i // 4) % times)
    return b"\n".join(out) + b"\n"


def kmer_records(seed, k, n, times=7):
    """n distinct random k-mers as records of their own, the j-th repeated 1 + j % times times."""
    rng = np.random.default_rng(seed)
    seen = []
    while len(seen) < n:
        s = bytes(rng.choice(list(b"ACGT"), k).tolist())
        if s not in seen:
            seen.append(s)
    return b"".join((b"@r\n" + s + b"\n+\n" + b"I" * k + b"\n") * (1 + j % times) for j, s in enumerate(seen))


def row_text(row, golden, seed=0):
    k, l = row[0], row[1]
    if k == 5:
        return kmer_records(l * 10 + seed, k, {4: 4, 5: 8, 6: 16}[l])   # three texts together fit the table
    if k == 14:
        return golden if seed == 0 else synth_text(900 + seed, 4)
    return repeated(synth_text(k * 7 + l + seed, {16: 10, 18: 24, 20: 50}[l]), 5)


def dict_add(a, b):
    out = dict(a)
    for x, c in b.items():
        out[x] = out.get(x, 0) + c
    return out


def hist_of(counts, nbins=10002):
    c = np.minimum(np.asarray(list(counts), dtype=np.uint64), np.uint64(nbins - 1)).astype(np.int64)
    return np.bincount(c, minlength=nbins).astype(np.uint64)


def read_count_file(path):
    out = {}
    for ln in open(path, "rb").read().split(b"\n"):
        if ln:
            x, c = ln.split(b"\t")
            assert x not in out
            out[x] = int(c)
    return out


def check_table(m, want, added, tmp_path, canonical=False):
    """Every reader of the table against {k-mer: count}: lookups (both strands), dump, histogram, text, stats."""
    k = m.k
    kmers = list(want)
    counts = np.array([want[x] for x in kmers], dtype=np.uint64)
    assert np.array_equal(m.getKmerCounts(K.kmers_to_limbs(kmers, k)), counts)
    if canonical:
        assert np.array_equal(m.getKmerCounts(K.kmers_to_limbs([K.revcomp(x) for x in kmers], k)), counts)
    gk, gc = m.getAllKmers()
    dump = dict(zip(K.limbs_to_kmers(gk, k), gc.tolist()))
    assert len(dump) == len(gc) and dump == want
    assert np.array_equal(m.getCountHistogram(10002), hist_of(want.values()))
    path = str(tmp_path / "t.count")
    lines, _ = m.writeCounts(path)
    assert lines == len(want) and read_count_file(path) == want
    st = m.stats()
    assert st["distinct"] == len(want) and st["count_sum"] == sum(want.values()) and st["kmers_added"] == added, st
    assert st["insert_failures"] == 0 and st["overflow_failures"] == 0 and st["lock_timeouts"] == 0, st
    return sorted(dump.items())


def expected(text, k, canonical=False):
    want = dict(python_counts(text, k))
    return K.fold_strands(want) if canonical else want


def check_header(h, lay, m, seed):
    st = m.stats()
    assert (h["k"], h["l"], h["entry_limbs"], h["func_bits"], h["reprobe_bits"], h["count_bits"], h["seg_bits"]) == \
        (lay.k, lay.l, lay.W, lay.F, lay.R, lay.C, lay.S)
    assert h["overflow_l"] == m.layout.overflow_l and h["hash_seed"] == seed
    assert (h["kmers_added"], h["distinct"], h["count_sum"], h["carry_records"]) == \
        (st["kmers_added"], st["distinct"], st["count_sum"], st["overflow_used"])


def paths_for(lay):
    return ["atomic", "partitioned"] if lay.l > lay.S else ["atomic"]


def new_map(T, row, seed=SEED, **kw):
    k, l, s = row[:3]
    m = T.TSXHashMapHIP(l, s, k, hash_seed=seed, **kw)
    lay = layout_of(row)
    for f, v in lay.fields().items():
        if not (f == "overflow_l" and kw.get("overflow_l")):
            assert getattr(m.layout, f) == v, (f, getattr(m.layout, f), v)
    return m


# ---- 3. the save side -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("row", MATRIX, ids=IDS)
def test_saved_file_reads_as_the_format_says(tmp_path, golden_fastq, row):
    import tsxcount_amd as T
    lay = layout_of(row)
    text = row_text(row, golden_fastq)
    want = expected(text, lay.k)
    for path in paths_for(lay):
        m = new_map(T, row)
        try:
            m.set_path(path)
            m.countFastq(text)
            if lay.C <= 2:
                assert m.stats()["overflow_used"] > 0
            rows = m.hash_rows()
            for cb in (0, 32 + 8 * 4 + 64 * 8 * lay.W * 4):
                db = str(tmp_path / ("s%d.db" % cb))
                m.saveDatabase(db, chunk_bytes=cb)
                f = K.read_db(db, rows)
                assert f.kmers == want
                check_header(f.header, lay, m, SEED)
                assert len(f.carries) == m.stats()["overflow_used"]
                if cb and lay.slots > 256:
                    assert len(f.chunks) == lay.slots // 256
        finally:
            m.close()


def with_base_rule_damage(text, base):
    """A non-ACGT base (base=True) or a low quality byte in some records (the base rule has something to skip)."""
    lines = text.split(b"\n")
    for r in range(0, len(lines) // 4, 3):
        seq, qual = bytearray(lines[4 * r + 1]), bytearray(lines[4 * r + 3])
        if base:
            seq[40 + r % 50] = ord("N")
        else:
            qual[200 + r % 70] = ord("!")
        lines[4 * r + 1], lines[4 * r + 3] = bytes(seq), bytes(qual)
    return b"\n".join(lines)


def rule_counts(text, k, acgt_only, min_qual):
    """python_counts restricted to windows that pass the base rule."""
    lines = [ln for ln in text.split(b"\n") if ln]
    out = {}
    for seq, qual in zip(lines[1::4], lines[3::4]):
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if acgt_only and any(ch not in b"ACGT" for ch in w):
                continue
            if min_qual and (len(qual) < i + k or min(qual[i:i + k]) < min_qual):
                continue
            out[w] = out.get(w, 0) + 1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["canonical", "acgt_only", "min_qual_char"])
def test_modes_save_and_load(tmp_path, mode):
    """Key limbs 3 with carries (k = 96, l = 18, s = 2), in canonical mode and under each base rule."""
    import tsxcount_amd as T
    row = MATRIX[IDS.index("k96-l18-s2")]
    lay = layout_of(row)
    text = repeated(synth_text(96, 24), 5)
    kw = {mode: "&" if mode == "min_qual_char" else True}   # (synthetic reads have quality '&' throughout)
    canonical = mode == "canonical"
    if canonical:
        want = expected(text, 96, canonical=True)
    else:
        text = with_base_rule_damage(text, mode == "acgt_only")
        want = rule_counts(text, 96, mode == "acgt_only", ord("&") if mode == "min_qual_char" else 0)
        assert want != dict(python_counts(text, 96))
    m = new_map(T, row, **kw)
    try:
        m.countFastq(text)
        assert m.stats()["overflow_used"] > 0
        rows = m.hash_rows()
        db = str(tmp_path / "m.db")
        m.saveDatabase(db)
        f = K.read_db(db, rows)
        h = f.header
        assert (h["canonical"], h["acgt_only"], h["min_qual_char"]) == \
            (int(canonical), int(mode == "acgt_only"), ord("&") if mode == "min_qual_char" else 0)
        check_header(h, lay, m, SEED)
        assert (K.fold_strands(f.kmers) if canonical else f.kmers) == want
        if canonical:   # the stored strand is the one with the smaller hashed key
            inv = K.inverse_rows(rows, 96)
            for key in list(f.keys)[:200]:
                x = K.keys_to_kmers([key], inv, 96)[0]
                assert key == min(K.table_keys([x], rows, 96)[0], K.table_keys([K.revcomp(x)], rows, 96)[0])
        added = m.stats()["kmers_added"]
        for kw2 in ({}, {"iL": 19}):
            m2 = T.TSXHashMapHIP.fromDatabase(db, **kw2)
            try:
                check_table(m2, want, added, tmp_path, canonical)
            finally:
                m2.close()
    finally:
        m.close()


@pytest.mark.gpu
def test_non_default_segment_size(tmp_path, monkeypatch):
    import tsxcount_amd as T
    row = MATRIX[IDS.index("k31-l20-s16")]
    lay = layout_of(row)
    text = repeated(synth_text(3120, 50), 5)
    want = expected(text, 31)
    monkeypatch.setenv("TSX_HIP_SEG_BITS", "9")
    m = T.TSXHashMapHIP(20, 16, 31, hash_seed=SEED)
    monkeypatch.delenv("TSX_HIP_SEG_BITS")
    try:
        m.countFastq(text)
        rows = m.hash_rows()
        db = str(tmp_path / "seg.db")
        m.saveDatabase(db)
        f = K.read_db(db, rows)
        assert f.header["seg_bits"] == 9 and lay.S == 12
        assert f.layout.S == 9 and f.kmers == want
        # some entries sit where only 2^9-slot segments put them (their probes wrapped inside the small segment)
        assert any(f.layout.unprobe(p, w[0] & 0xFF) != lay.unprobe(p, w[0] & 0xFF) for p, w in f.entries.items())
        d = T.TSXHashMapHIP(20, 16, 31, hash_seed=SEED)   # default segments: the re-insert path
        try:
            d.addDatabase(db)
            check_table(d, want, m.stats()["kmers_added"], tmp_path)
        finally:
            d.close()
    finally:
        m.close()


# ---- 4. the load side -----------------------------------------------------------------------------------------------------

def chunk_plans(lay):
    if lay.slots <= 64:
        return [None]
    odd = K.spans(lay.slots, [64 * 3, 64 * 17, 64, 64 * 50, 64 * 2])
    return [None, odd]


@pytest.mark.gpu
@pytest.mark.parametrize("row", MATRIX, ids=IDS)
def test_written_file_loads_four_ways(tmp_path, golden_fastq, row):
    import tsxcount_amd as T
    lay = layout_of(row)
    k, l, s = row[:3]
    text, other, more = (row_text(row, golden_fastq, j) for j in (0, 1, 2))
    want, want_other, want_more = expected(text, k), expected(other, k), expected(more, k)
    added = sum(want.values())
    # 2-bit counters: every k-mer seen 4 times carries, and a merge or recount adds the other texts' carried slots to the
    # secondary array (overflow_l does not decide direct placement)
    kw = {"overflow_l": l - 1} if lay.C <= 2 else {}
    a = new_map(T, row)
    rows = a.hash_rows()
    a.close()
    for ci, chunks in enumerate(chunk_plans(lay)):
        db = str(tmp_path / ("w%d.db" % ci))
        img = K.write_db(db, want, lay, rows, SEED, chunks=chunks)
        f = K.read_db(db, rows)
        assert f.kmers == want
        if chunks:
            assert len(f.chunks) > 1 and f.chunks[-1][1] == lay.slots
            if len(want) < lay.slots // 16:   # (sparse enough for some 64-slot chunks to hold nothing)
                assert any(n == 0 for _, _, n, _ in f.chunks)
        maps = []
        try:
            a = new_map(T, row, **kw)                       # (a) direct placement
            maps.append(a)
            a.addDatabase(db)
            dump_a = check_table(a, want, added, tmp_path)
            kmers = list(want)
            _, slots = a.getKmerCountDebug(K.kmers_to_limbs(kmers, k))
            assert slots.tolist() == [img.kmer_slot[x] for x in kmers]
            b = new_map(T, row, seed=SEED + 1, **kw)     # (b) re-insert: another seed
            maps.append(b)
            b.addDatabase(db)
            assert check_table(b, want, added, tmp_path) == dump_a
            c = new_map(T, row, **kw)                       # (c) merge onto counted reads
            maps.append(c)
            c.countFastq(other)
            c.addDatabase(db)
            check_table(c, dict_add(want, want_other), added + sum(want_other.values()), tmp_path)
            d = new_map(T, row, **kw)                       # (d) direct placement into a lazily cleared table
            maps.append(d)
            d.set_path("partitioned")
            d.countFastq(other)
            d.clear()
            d.addDatabase(db)
            check_table(d, want, added, tmp_path)
            # more reads on top of the directly placed tables: the partitioned build merges with the loaded segments
            for m in (a, d):
                m.set_path("partitioned")
                m.countFastq(more)
                check_table(m, dict_add(want, want_more), added + sum(want_more.values()), tmp_path)
        finally:
            for m in maps:
                m.close()


# ---- 5. malformed files with valid checksums --------------------------------------------------------------------------------

def _first(img, with_carry=None):
    carried = {c[0] for c in img.carries}
    return next(p for p in sorted(img.slots) if with_carry is None or (p in carried) == with_carry)


def _free_bit(mask):
    return next(b for b in range(63, -1, -1) if not (mask >> b) & 1)


def damage(img, kind):
    lay = img.layout
    if kind == "stray_limb0":
        img.slots[_first(img, False)][0] |= 1 << _free_bit(lay.masks[0] | lay.lock_bit)
    elif kind == "stray_last_limb":
        img.slots[_first(img, True if img.carries else None)][lay.W - 1] |= 1 << _free_bit(lay.masks[-1])
    elif kind == "reprobe_0":
        img.slots[_first(img, False)][0] &= ~((1 << lay.R) - 1)
    elif kind == "lock":
        img.slots[_first(img, False)][0] |= lay.lock_bit
    elif kind == "bitmap_past_end":
        img.slots[lay.slots + 3] = list(img.slots[_first(img)])
    elif kind == "n_entries":
        img.n_adjust[next(j for j, (lo, hi) in enumerate(img.chunks) if lo <= _first(img) < hi)] = -1
    elif kind == "span_not_64":
        img.chunks = [(0, 100), (100, lay.slots)]
    elif kind == "carry_on_empty":
        empty = next(p for p in range(lay.slots) if p not in img.slots)
        img.carries = sorted(img.carries + [[empty, 1, list(img.slots[_first(img)])]])
    elif kind == "carry_words_differ":
        c = img.carries[0]
        c[2] = list(img.slots[_first(img, False)])
    elif kind == "carries_unsorted":
        img.carries[0], img.carries[1] = img.carries[1], img.carries[0]
    elif kind == "carries_duplicated":
        img.carries.insert(1, list(img.carries[0]))
    elif kind == "zero_count":
        p = _first(img, False)
        img.slots[p][0] &= (1 << (64 - lay.C)) - 1
    else:
        raise ValueError(kind)


DEFECTS = [("stray_limb0", "k31-l16-s2"), ("stray_limb0", "k14-l20-s0"), ("stray_last_limb", "k63-l18-s2"),
           ("stray_last_limb", "k80-l20-s0"), ("reprobe_0", "k31-l16-s2"), ("lock", "k63-l18-s2"),
           ("bitmap_past_end", "k5-l4-s0"), ("bitmap_past_end", "k5-l5-s0"), ("n_entries", "k31-l16-s2"),
           ("span_not_64", "k31-l16-s2"), ("carry_on_empty", "k63-l18-s2"), ("carry_words_differ", "k31-l16-s2"),
           ("carry_words_differ", "k127-l16-s2"), ("carries_unsorted", "k63-l18-s2"),
           ("carries_duplicated", "k31-l16-s2"), ("zero_count", "k31-l16-s2"), ("zero_count", "k96-l18-s2")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,row_id", DEFECTS, ids=["%s-%s" % d for d in DEFECTS])
def test_malformed_file_is_a_format_error(tmp_path, golden_fastq, kind, row_id):
    import tsxcount_amd as T
    row = MATRIX[IDS.index(row_id)]
    lay = layout_of(row)
    text = row_text(row, golden_fastq)
    want = expected(text, lay.k)
    m = new_map(T, row)
    rows = m.hash_rows()
    m.close()
    img = K.build_image(want, lay, rows, SEED, chunks=K.spans(lay.slots, [1024]) if lay.slots > 1024 else None)
    if kind.startswith("carr"):
        assert len(img.carries) >= 2
    damage(img, kind)
    db = str(tmp_path / "bad.db")
    K.write_image(db, img)
    with pytest.raises(K.FormatError):
        K.read_db(db, rows)
    for seed in (SEED, SEED + 1):   # direct placement, then the re-insert path
        m = new_map(T, row, seed=seed)
        try:
            with pytest.raises(T.TSXException) as e:
                m.addDatabase(db)
            assert e.value.code == T.EFORMAT, (kind, seed, str(e.value))
            m.clear()
            m.countFastq(text)
            check_table(m, want, sum(want.values()), tmp_path)
        finally:
            m.close()


# ---- 6. a file an earlier build wrote ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_committed_version_1_file_loads(tmp_path):
    import tsxcount_amd as T
    from golden import make_db_v1 as G
    want = dict(python_counts(G.first_records(), G.K))
    info = T.database_info(FIXTURE)
    assert (info["version"], info["k"], info["l"], info["count_bits"], info["hash_seed"]) == (1, G.K, G.L, G.S, G.SEED)
    assert info["carry_records"] > 0
    m = T.TSXHashMapHIP(G.L, G.S, G.K, hash_seed=G.SEED)
    try:
        f = K.read_db(FIXTURE, m.hash_rows())
        assert f.kmers == want and len(f.chunks) == (1 << G.L) // 256
    finally:
        m.close()
    for kw in ({}, {"iL": G.L + 2}, {"iStorageBits": 0}):   # direct placement, then the re-insert path twice
        m = T.TSXHashMapHIP.fromDatabase(FIXTURE, **kw)
        try:
            check_table(m, want, info["kmers_added"], tmp_path)
        finally:
            m.close()
