"""Digital normalization on the GPU: tsx_hip_normalize_host / _device through Python, and the tsxCount CLI.

Expectations come from the plain Python definition in tests/normalize_ref.py only -- never from the library under
test.  Everything is compared exactly: the keep flags, the output bytes, the totals, and the table through the count of
every k-mer of the text (those it must not hold included) plus the distinct number and kmers_added of its stats."""
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from normalize_ref import normalize, record_kmers
from test_fasta_wrapped import encode_np
from test_read_query import U64, coded_counts, run_cli
from test_trim_widths import random_bases

TOT_KEYS = ("records", "kept", "kmers_seen", "kmers_added", "rounds")


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def fastq(seqs, qual=None):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, qual[i] if qual else b"I" * len(s)) for i, s in enumerate(seqs))


def fasta(seqs):
    return b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def drawn_reads(seed, k, n=300, templates=8, alphabet=b"ACGT"):
    """n reads drawn with heavy repetition from a few templates: windows of 2k + 20 .. 2k + 60 bases of them."""
    rnd = random.Random(seed)
    tl = 3 * k + 90
    tmpl = [random_bases(rnd, tl, alphabet) for _ in range(templates)]
    seqs = []
    for _ in range(n):
        t = tmpl[min(rnd.randrange(templates), rnd.randrange(templates))]   # the first templates are drawn more often
        ln = rnd.randrange(2 * k + 20, 2 * k + 61)
        a = rnd.randrange(0, tl - ln + 1)
        seqs.append(t[a:a + ln])
    return seqs


def to_device(text):
    import torch
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    if text:
        dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    return dev


def new_map(T, k, l=16, s=0, lpr=4, canonical=False, acgt_only=False, minq=0):
    m = T.TSXHashMapHIP(l, s, k)
    m.set_path(1)
    m.set_record_lines(lpr)
    if canonical:
        m.set_canonical(True)
    if acgt_only or minq:
        m.set_base_rule(acgt_only=acgt_only, min_qual_char=minq if minq else None)
    return m


def check_table(m, k, want, also=()):
    """The table holds `want` and nothing else: the counts of its keys and of `also`, distinct, kmers_added."""
    keys = sorted(set(want) | set(also))
    st = m.stats()
    assert st["distinct"] == len(want) and st["kmers_added"] == sum(want.values()), (st, len(want), sum(want.values()))
    assert st["insert_failures"] == 0
    if keys:
        got = m.getKmerCounts(encode_np(keys, k))
        exp = np.array([want.get(x, 0) for x in keys], dtype=np.uint64)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, [(keys[i], int(got[i]), int(exp[i])) for i in bad[:5]]


def check(T, text, k, cutoff, R, tmp_path, lpr=4, l=16, s=0, chunks=(0,), device=True, prefill=None, **rule):
    """Host form at every piece size and the device form, each on a fresh map, against the definition.  Returns the
    definition's (keep, totals)."""
    before = coded_counts(prefill, k, lpr, canonical=rule.get("canonical", False)) if prefill else None
    keep, out, tot, table = normalize(text, k, lpr, cutoff, R, counts=before, **rule)
    every = {x for keys, _ in record_kmers(text, k, lpr, **rule) for x in keys}
    path = str(tmp_path / "norm.out")
    for chunk in chunks:
        m = new_map(T, k, l, s, lpr, **rule)
        if prefill:
            m.countFastq(prefill)
        got = m.normalizeReads(text, path, cutoff=cutoff, round_records=R, keep=True, chunk_bytes=chunk)
        assert got["keep"].dtype == bool and got["keep"].tolist() == keep, (chunk, np.flatnonzero(got["keep"] != np.array(keep))[:8])
        assert {f: got[f] for f in TOT_KEYS} == tot, chunk
        assert open(path, "rb").read() == out, chunk
        m.sync()
        check_table(m, k, table, every)
        m.close()
    if device:
        import torch
        m = new_map(T, k, l, s, lpr, **rule)
        if prefill:
            m.countFastq(prefill)
        dev = to_device(text)
        dkeep = torch.full((len(keep) + 5,), 7, dtype=torch.uint8, device="cuda:0")
        got = m.normalizeReadsDevice(dev.data_ptr(), len(text), dkeep.data_ptr(), len(keep) + 5, cutoff=cutoff, round_records=R)
        hk = dkeep.cpu().numpy()
        assert hk[:len(keep)].astype(bool).tolist() == keep and (hk[len(keep):] == 7).all()
        assert got == tot
        m.sync()
        check_table(m, k, table, every)
        m.close()
    return keep, tot


@pytest.mark.gpu
def test_round_sizes_decide_differently(T, tmp_path):
    text = fastq(drawn_reads(1, 21))
    keeps = {}
    for R in (1, 3, 64, 1000):
        keeps[R], tot = check(T, text, 21, 4, R, tmp_path)
        assert tot["records"] == 300 and 0 < tot["kept"] <= 300
    assert len({tuple(v) for v in keeps.values()}) == 4      # no R may stand for another
    assert all(keeps[1000]) and not all(keeps[64])            # one round: every record is judged against the empty table


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 31, 33, 65, 127])
def test_key_widths(T, tmp_path, k):
    seqs = drawn_reads(2 + k, k, n=150, alphabet=b"ACG" if k == 5 else b"ACGT")
    keep, tot = check(T, fastq(seqs), k, 3, 16, tmp_path, l=9 if k == 5 else 16)
    assert 0 < tot["kept"] < 150


@pytest.mark.gpu
def test_medians_from_carried_counts(T, tmp_path):
    """storagebits 4: a slot counts to 15, C = 40 is reached in the carries."""
    seqs = drawn_reads(7, 21, n=300, templates=2)
    m = new_map(T, 21, 16, 4)
    m.countFastq(fastq(seqs))
    assert m.stats()["overflow_carries"] > 0
    m.close()
    keep, tot = check(T, fastq(seqs), 21, 40, 8, tmp_path, s=4)
    assert 40 < tot["kept"] < 300 and not all(keep[200:])


@pytest.mark.gpu
def test_table_variants(T, tmp_path):
    rnd = random.Random(9)
    seqs = drawn_reads(9, 21, n=200)
    both = [s if i % 2 else s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")) for i, s in enumerate(seqs)]
    keep, tot = check(T, fastq(both), 21, 4, 16, tmp_path, canonical=True)
    assert 0 < tot["kept"] < 200
    plain, _ = check(T, fastq(both), 21, 4, 16, tmp_path, device=False)
    assert plain != keep                                      # the strands of a template meet in a canonical table only
    # N bases and low qualities: windows the rule drops are no k-mers of the read, for the median and for the count
    noisy, quals = [], []
    for s in seqs:
        b, q = bytearray(s), bytearray(b"I" * len(s))
        for _ in range(rnd.randrange(0, 3)):
            b[rnd.randrange(len(b))] = ord("N")
        for _ in range(rnd.randrange(0, 3)):
            q[rnd.randrange(len(q))] = ord("#")
        noisy.append(bytes(b)); quals.append(bytes(q))
    ruled, tot = check(T, fastq(noisy, quals), 21, 4, 16, tmp_path, acgt_only=True, minq=ord("5"))
    assert 0 < tot["kept"] < 200 and tot["kmers_seen"] < sum(len(s) - 20 for s in noisy)
    keep, tot = check(T, fasta(seqs), 21, 4, 16, tmp_path, lpr=2)
    assert 0 < tot["kept"] < 200


@pytest.mark.gpu
def test_record_shapes(T, tmp_path):
    k = 21
    seqs = drawn_reads(11, k, n=120, templates=3)
    rep = random_bases(random.Random(3), 30)
    seqs[5] = b"A" * 90                                       # a homopolymer: one run of equal k-mers
    seqs[6] = rep + rep + rep                                 # a k-mer repeated inside the read: the LDS dedup
    seqs[40] = seqs[5]; seqs[41] = seqs[6]; seqs[80] = seqs[5]; seqs[81] = seqs[6]
    seqs[10] = seqs[0][:k - 1]; seqs[11] = b"AC"; seqs[12] = seqs[0][:k]   # shorter than k: median 0, kept, nothing added; exactly k
    seqs[50] = random_bases(random.Random(4), 9000)           # a record that spans three tiles
    seqs[100] = seqs[50]; seqs[110] = seqs[50]
    body = fastq(seqs)
    texts = {"whole": body,
             "empty_lines": b"\n\n" + body.replace(b"\n@r7\n", b"\n\n\n@r7\n").replace(b"\n@r60\n", b"\n\n@r60\n") + b"\n\n",
             "open": body[:-1],
             "open_incomplete": body + b"@tail\n" + seqs[1]}
    for name, text in texts.items():
        keep, tot = check(T, text, k, 2, 4, tmp_path)
        assert keep[10] and keep[11], name
        assert keep[5] and not keep[40] and not keep[80], name    # the later copies of the homopolymer meet a count of 70
        assert keep[6] and not keep[41], name
        assert keep[50] and keep[100] and not keep[110], name      # the long record: its third copy's tiles are skipped
        assert any(keep[i] != keep[i + 1] for i in range(119)), name   # kept and dropped records share tiles (some 15 a tile)
        assert 0 < tot["kept"] < tot["records"], name
    keep, _ = check(T, fasta(seqs), k, 2, 4, tmp_path, lpr=2)


@pytest.mark.gpu
def test_seams_change_nothing(T, tmp_path, monkeypatch):
    k = 21
    seqs = drawn_reads(13, k, n=300)
    seqs[150] = random_bases(random.Random(5), 6000)          # a record longer than a piece and a window
    text = fastq(seqs)
    want = {R: check(T, text, k, 4, R, tmp_path) for R in (1, 5, 64)}
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "700")
    monkeypatch.setenv("TSX_HIP_DEV_WINDOW", "4096")
    monkeypatch.setenv("TSX_HIP_MEDIAN_LONG", "64")
    for R in (1, 5, 64):
        assert check(T, text, k, 4, R, tmp_path, chunks=(0, 300, 5000)) == want[R], R
    monkeypatch.delenv("TSX_HIP_PIECE_BYTES")
    monkeypatch.delenv("TSX_HIP_MEDIAN_LONG")
    assert check(T, text, k, 4, 64, tmp_path, chunks=(900, 20000)) == want[64]   # chunk_bytes alone, below a round of records


@pytest.mark.gpu
def test_extreme_cutoffs(T, tmp_path):
    k = 21
    text = fastq(drawn_reads(15, k, n=200))
    keep, tot = check(T, text, k, U64, 16, tmp_path)
    assert all(keep) and tot["kmers_added"] == tot["kmers_seen"]
    a, b = new_map(T, k), new_map(T, k)
    a.normalizeReads(text, None, cutoff=U64, round_records=16)
    b.countFastq(text)
    (ka, ca), (kb, cb) = a.getAllKmers(), b.getAllKmers()
    assert sorted(zip(map(tuple, np.asarray(ka).reshape(len(ca), -1).tolist()), ca.tolist())) == \
           sorted(zip(map(tuple, np.asarray(kb).reshape(len(cb), -1).tolist()), cb.tolist()))
    a.close(); b.close()
    keep, tot = check(T, text, k, 0, 16, tmp_path, prefill=fastq(drawn_reads(16, k, n=50)))
    assert not any(keep) and tot["kmers_added"] == 0 and tot["kmers_seen"] > 0


@pytest.mark.gpu
def test_on_a_table_that_is_not_empty(T, tmp_path):
    k = 21
    seqs = drawn_reads(17, k, n=200)
    empty, _ = check(T, fastq(seqs[100:]), k, 4, 8, tmp_path, device=False)
    filled, tot = check(T, fastq(seqs[100:]), k, 4, 8, tmp_path, prefill=fastq(seqs[:100]))
    assert sum(filled) < sum(empty) and 0 < tot["kept"]


@pytest.mark.gpu
def test_more_records_than_keep_cap(T):
    import ctypes
    k = 21
    text = fastq(drawn_reads(19, k, n=100))
    keep, _, tot, table = normalize(text, k, 4, 4, 8)
    m = new_map(T, k)
    flags = np.full(40, 9, dtype=np.uint8)
    rule, got = T.normalize_rule(4, 8), T.NormalizeTotals()
    rc = m._lib.tsx_hip_normalize_host(m.handle, text, len(text), ctypes.byref(rule), -1, flags.ctypes.data_as(ctypes.c_void_p), 30,
                                       0, ctypes.byref(got))
    assert rc == T.ERANGE and got.as_dict() == tot
    assert flags[:30].astype(bool).tolist() == keep[:30] and (flags[30:] == 9).all()
    check_table(m, k, table)                                  # the table is complete
    m.close()
    import torch
    m = new_map(T, k)
    dev, dkeep = to_device(text), torch.full((40,), 9, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(T.TSXException) as e:
        m.normalizeReadsDevice(dev.data_ptr(), len(text), dkeep.data_ptr(), 30, cutoff=4, round_records=8)
    assert e.value.code == T.ERANGE
    hk = dkeep.cpu().numpy()
    assert hk[:30].astype(bool).tolist() == keep[:30] and (hk[30:] == 9).all()
    check_table(m, k, table)
    m.close()


@pytest.mark.gpu
def test_refusals_on_the_device(T):
    text = fastq(drawn_reads(21, 21, n=10))
    m = T.TSXHashMapHIP(16, 0, 21, shard_bits=1, shard_index=0)
    with pytest.raises(T.TSXException) as e:
        m.normalizeReads(text)
    assert e.value.code == T.EINVAL and "shard_bits" in str(e.value)
    m.close()
    m = new_map(T, 21)
    m.prefilter(text, 16)
    m.armPrefilter(True)
    with pytest.raises(T.TSXException) as e:
        m.normalizeReads(text)
    assert e.value.code == T.EINVAL and "prefilter" in str(e.value)
    m.armPrefilter(False)
    assert m.normalizeReads(text)["kept"] == 10 and m.stats()["kmers_added"] > 0
    m.close()


@pytest.mark.gpu
def test_cli_end_to_end(T, tmp_path):
    k, cutoff, R = 14, 3, 100
    src = os.path.join(GOLDEN, "small_t7.1000.fastq")
    text = open(src, "rb").read()
    keep, out, tot, table = normalize(text, k, 4, cutoff, R)
    assert 0 < tot["kept"] < tot["records"]
    kept_path, db, histo = tmp_path / "kept.fastq", tmp_path / "n.db", tmp_path / "n.histo"
    base = ("--input=" + src, "--k=%d" % k, "--l=20", "--normalize-cutoff=%d" % cutoff, "--normalize-round=%d" % R)
    code, stdout, err = run_cli(*base, "--normalize=" + str(kept_path), "--save=" + str(db), "--histo=" + str(histo))
    assert code == 0, err
    line = [ln for ln in stdout.splitlines() if ln.startswith("normalize\t")]
    assert line == ["normalize\t" + "\t".join(str(tot[f]) for f in TOT_KEYS)]
    assert kept_path.read_bytes() == out
    want_h = {}
    for c in table.values():
        want_h[c] = want_h.get(c, 0) + 1
    got_h = {int(a): int(b) for a, b in (ln.split("\t") for ln in histo.read_text().splitlines()) if int(b)}
    assert got_h == want_h
    # on top of the saved table fewer reads stay below the cutoff: exactly the definition's number
    keep2, out2, tot2, _ = normalize(text, k, 4, cutoff, R, counts=table)
    assert tot2["kept"] < tot["kept"]
    again = tmp_path / "again.fastq"
    code, stdout, err = run_cli(*base, "--load=" + str(db), "--normalize=" + str(again))
    assert code == 0, err
    assert [ln for ln in stdout.splitlines() if ln.startswith("normalize\t")] == ["normalize\t" + "\t".join(str(tot2[f]) for f in TOT_KEYS)]
    assert again.read_bytes() == out2
