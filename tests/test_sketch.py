"""Table sizing on the GPU: the HyperLogLog sketch of a text (tsx_hip_sketch_*), its estimate against the table's own
distinct count, and the sizing end to end, through the C ABI, Python and the tsxCount CLI.

Registers and totals are compared EXACTLY with the model of test_sketch_cpu.py (model_sketch: the window rule of
test_base_rule, encode_np, tsxcount_amd.sketch_registers in numpy).  Never with the library under test."""
import ctypes
import gzip
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from test_base_rule import RULES, edited_text
from test_read_query import EDGE_FASTQ, fasta_of, fastq_of, random_seqs, rc, run_cli
from test_sketch_cpu import U8P, model_sketch, sigma5


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def probe(T, k, lpr=4, l=None, **kw):
    if l is None:
        l = 12 if k > 120 else min(10, 2 * k - 1)                 # (k = 127 has no layout below l = 11)
    m = T.TSXHashMapHIP(l, 0, k, **kw)
    if lpr != 4:
        m.set_record_lines(lpr)
    return m


def to_device(text):
    import torch
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    if text:
        dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    return dev


def device_sketch(m, text, p=14, regs=None, totals=True):
    """(registers as uint8, totals) of the device call; the words behind the registers and the totals stay untouched."""
    import torch
    dev = to_device(text)
    dregs = torch.zeros((1 << p) + 4, dtype=torch.int32, device="cuda:0")
    dregs[1 << p:] = 77
    if regs is not None:
        dregs[:1 << p] = torch.from_numpy(regs.astype(np.int32)).to("cuda:0")
    dtot = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    dtot[2] = -5
    torch.cuda.synchronize()                                     # (the map's stream does not wait for torch's)
    m.sketchKmersDevice(dev.data_ptr(), len(text), dregs.data_ptr(), precision=p, totals_ptr=dtot.data_ptr() if totals else None)
    torch.cuda.synchronize()
    m.sync()
    r, t = dregs.cpu().numpy(), dtot.cpu().numpy()
    assert (r[1 << p:] == 77).all() and t[2] == -5 and r[:1 << p].max() <= 64 - p + 1
    return r[:1 << p].astype(np.uint8), {"kmers": int(t[0]), "records": int(t[1])}


def abi_sketch(T, m, text, p=14):
    regs = np.zeros(1 << p, dtype=np.uint8)
    tot = T.SketchTotals()
    assert T.lib().tsx_hip_sketch_host(m.handle, text, len(text), p, regs.ctypes.data_as(U8P), ctypes.byref(tot), 0) == T.OK
    return regs, tot.as_dict()


def check_all_forms(T, m, text, want, tot, p=14):
    """sketchKmers, the C ABI host call and the device call against the model."""
    for name, (regs, t) in (("python", m.sketchKmers(text, precision=p)), ("abi", abi_sketch(T, m, text, p)),
                            ("device", device_sketch(m, text, p))):
        assert regs.dtype == np.uint8 and np.array_equal(regs, want), (name, np.flatnonzero(regs != want)[:8])
        assert t == tot, (name, t, tot)


def reads_for(rnd, k, n=150):
    seqs = random_seqs(rnd, n, 60, 300) + random_seqs(rnd, 6, 1, max(1, k - 1)) + random_seqs(rnd, 2, k, k)
    rnd.shuffle(seqs)
    return seqs


@pytest.mark.gpu
@pytest.mark.parametrize("lpr", [4, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,p", [(5, 14), (21, 14), (21, 10), (32, 14), (33, 14), (64, 14), (65, 14), (96, 14), (127, 14), (127, 10)])
def test_every_key_width(T, k, p, canonical, lpr):
    rnd = random.Random(1000 * k + 10 * p + lpr + canonical)
    text = (fastq_of if lpr == 4 else fasta_of)(reads_for(rnd, k))
    want, tot, distinct = model_sketch(text, k, lpr, canonical=canonical, precision=p)
    assert tot["records"] == 158 and tot["kmers"] > (1000 if k == 127 else 10000) and np.count_nonzero(want) > 200
    m = probe(T, k, lpr, canonical=canonical)
    try:
        check_all_forms(T, m, text, want, tot, p)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_base_rules(T, k):
    text = edited_text(700 + k, 120, k)
    plain, plain_tot, _ = model_sketch(text, k)
    m = probe(T, k)
    try:
        check_all_forms(T, m, text, plain, plain_tot)
        for acgt_only, min_qual in RULES:
            m.set_base_rule(acgt_only, min_qual)
            want, tot, _ = model_sketch(text, k, 4, acgt_only, min_qual)
            assert tot["kmers"] < plain_tot["kmers"] and not np.array_equal(want, plain)   # the rule drops windows
            check_all_forms(T, m, text, want, tot)
    finally:
        m.close()


@pytest.mark.gpu
def test_record_rule_edges(T):
    k = 7
    m = probe(T, k)
    try:
        for text in (EDGE_FASTQ, EDGE_FASTQ[:-5] + b"@x\nACGTACGTAAA", EDGE_FASTQ[:-5] + b"\n\n"):
            want, tot, _ = model_sketch(text, k)
            assert tot["kmers"] > 20
            check_all_forms(T, m, text, want, tot)
        for text, nrec in ((b"", 0), (b"\n\n\n", 0), (b"@a\nACGTAC\n+\nIIIIII\n@b\nAC\n+\nII\n", 2), (b"@a", 1)):
            want, tot, _ = model_sketch(text, k)
            assert not want.any() and tot == {"kmers": 0, "records": nrec}
            check_all_forms(T, m, text, want, tot)
            assert T.sketch_estimate(m.sketchKmers(text)[0]) == 0.0
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 127])
def test_long_record_and_identical_reads(T, k):
    rnd = random.Random(k)
    long_rec = b">chr\n" + random_seqs(rnd, 1, 120000, 120000)[0] + b"\n"   # tiles and workgroups, one line
    read = random_seqs(rnd, 1, 150, 150)[0]
    same = fasta_of([read] * 3000)                                          # run-length leaders, hot registers
    homo = fasta_of([b"A" * 200] * 40 + [b"ACAC" * 50] * 40)                 # equal neighbouring windows
    m = probe(T, k, 2)
    try:
        for text in (long_rec, same, homo):
            want, tot, _ = model_sketch(text, k, 2)
            check_all_forms(T, m, text, want, tot)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,min_qual", [(31, "5"), (127, None)])
def test_seams(T, k, min_qual, monkeypatch):
    rnd = random.Random(77 + k)
    seqs = random_seqs(rnd, 560, 100, 250)
    quals = [bytes(rnd.choice(b"+5I") for _ in s) for s in seqs]
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(seqs, quals)))
    assert 190000 < len(text) < 260000
    want, tot, _ = model_sketch(text, k, 4, False, min_qual)
    if min_qual:
        assert tot["kmers"] < model_sketch(text, k)[1]["kmers"]
    m = probe(T, k, min_qual_char=min_qual)
    try:
        one, t1 = m.sketchKmers(text)
        assert np.array_equal(one, want) and t1 == tot
        for chunk in (4096, 5000, 65536):
            regs, t = m.sketchKmers(text, chunk_bytes=chunk)
            assert np.array_equal(regs, want) and t == tot, chunk
        for win in (4096, 5000):
            monkeypatch.setenv("TSX_HIP_DEV_WINDOW", str(win))
            regs, t = device_sketch(m, text)
            assert np.array_equal(regs, want) and t == tot, win
        monkeypatch.delenv("TSX_HIP_DEV_WINDOW")
        monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")                 # (the smallest batch the library takes: 128 KiB)
        for block in (1000, 65280):
            regs, t = m.sketchKmersBgzf(T.bgzf_compress(text, block=block))
            assert np.array_equal(regs, want) and t == tot, block
    finally:
        m.close()
    for piece in (4096, 5000):
        monkeypatch.setenv("TSX_HIP_PIECE_BYTES", str(piece))
        m = probe(T, k, min_qual_char=min_qual)
        try:
            regs, t = m.sketchKmers(text)
            assert np.array_equal(regs, want) and t == tot, piece
        finally:
            m.close()


@pytest.mark.gpu
def test_accumulation_and_independence(T):
    k = 31
    rnd = random.Random(12)
    sa, sb = random_seqs(rnd, 60, 80, 200), random_seqs(rnd, 60, 80, 200)
    A, B = fastq_of(sa, b"a"), fastq_of(sb, b"b")
    wa, ta, _ = model_sketch(A, k)
    wb, tb, _ = model_sketch(B, k)
    wab, tab, _ = model_sketch(A + B, k)
    assert np.array_equal(T.merge_sketches(wa, wb), wab) and not np.array_equal(wa, wb)
    m = probe(T, k)
    try:
        ra, _ = m.sketchKmers(A)
        rab, t2 = m.sketchKmers(B, registers=ra)
        assert np.array_equal(ra, wa) and np.array_equal(rab, wab) and t2 == tb       # ra is not written to
        assert np.array_equal(T.merge_sketches(ra, m.sketchKmers(B)[0]), wab)
        assert np.array_equal(m.sketchKmers(A + B)[0], wab)
        da, dta = device_sketch(m, A)
        dab, dtab = device_sketch(m, B, regs=da)
        assert np.array_equal(dab, wab) and dta == ta and dtab == tb
        assert np.array_equal(device_sketch(m, A, totals=False)[0], wa)               # the totals are optional
        st = m.stats()
        assert st["distinct"] == 0 and st["kmers_added"] == 0                         # an empty map stays empty
    finally:
        m.close()
    # the registers depend on neither l, s nor the seed
    for l, s, seed in ((4, 0, 1), (18, 8, 99), (22, 4, 5)):
        m = T.TSXHashMapHIP(l, s, k, hash_seed=seed)
        try:
            assert np.array_equal(m.sketchKmers(A)[0], wa), (l, s, seed)
        finally:
            m.close()
    # a filled map is neither read nor written
    m = T.TSXHashMapHIP(16, 0, k)
    try:
        m.countFastq(A)
        kept = sorted(set(s[i:i + k] for s in sa for i in range(len(s) - k + 1)))[:1000]
        enc = T.encode_many([x.decode() for x in kept], k)
        before, counts = m.stats(), m.getKmerCounts(enc)
        assert before["distinct"] > 5000 and (counts >= 1).all()
        assert np.array_equal(m.sketchKmers(B)[0], wb) and np.array_equal(device_sketch(m, B)[0], wb)
        assert m.stats() == before and np.array_equal(m.getKmerCounts(enc), counts)
    finally:
        m.close()
    # a canonical map: either strand of a read gives the same registers
    R = fastq_of([rc(s) for s in sa], b"a")
    wc, _, _ = model_sketch(A, k, canonical=True)
    m = probe(T, k, canonical=True)
    try:
        assert np.array_equal(m.sketchKmers(A)[0], wc) and np.array_equal(m.sketchKmers(R)[0], wc)
    finally:
        m.close()
    assert not np.array_equal(model_sketch(R, k)[0], wa)


def genome_fasta(n, seed):
    return b">g\n" + random_seqs(random.Random(seed), 1, n, n)[0] + b"\n"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3000, 45000, 200000])
def test_estimate_against_the_table(T, n):
    """|E / distinct - 1| <= 5 * 1.04 / sqrt(2^14) = 0.0406.  Measured on an MI355X: -0.0005 (3 000 bases), +0.0269
    (45 000: the classic estimator's bias bump just above the switch to linear counting), -0.0063 (200 000)."""
    k = 31
    text = genome_fasta(n, n)
    m = T.TSXHashMapHIP(20, 0, k)
    try:
        m.set_record_lines(2)
        m.countFastq(text)
        st = m.stats()
        regs, tot = m.sketchKmers(text)
        assert st["kmers_added"] == tot["kmers"] == n - k + 1 and st["distinct"] > 0.99 * (n - k + 1)
        e = T.sketch_estimate(regs)
        print("bases=%d distinct=%d estimate=%.1f E/distinct-1=%+.4f bound=%.4f" % (n, st["distinct"], e, e / st["distinct"] - 1, sigma5(14)))
        assert abs(e / st["distinct"] - 1) <= sigma5(14)
    finally:
        m.close()


@pytest.mark.gpu
def test_sized_for_end_to_end(T):
    k = 31
    text = genome_fasta(200000, 200000)
    want, tot, distinct = model_sketch(text, k, 2)
    est = T.sketch_estimate(want)
    m = T.TSXHashMapHIP.sizedFor(text, k, lines=2)
    try:
        assert m.l == T.suggest_l(est, k) == 19
        assert m.size_estimate == {"kmers": tot["kmers"], "distinct": est, "l": m.l, "load": est / (1 << m.l)}
        m.countFastq(text)                                       # no EFULL
        st = m.stats()
        assert st["distinct"] == distinct and st["distinct"] / (1 << m.l) <= 0.9
    finally:
        m.close()
    # k = 127 has no layout below l = 11: the probe map and the sized one take the smallest l that has one
    m = T.TSXHashMapHIP.sizedFor(fasta_of([genome_fasta(400, 4)[3:-1]]), 127, lines=2)
    try:
        assert m.l == 11 and T.suggest_l(m.size_estimate["distinct"], 127) == 9 and m.size_estimate["kmers"] == 274
        m.countFastq(fasta_of([genome_fasta(400, 4)[3:-1]]))
        assert m.stats()["distinct"] == 274
    finally:
        m.close()
    m = T.TSXHashMapHIP.sizedFor(fastq_of([b"ACGT" * 20]), k, load=0.5, canonical=True)
    try:
        assert m.l == 4 and m.canonical and m.size_estimate["kmers"] == 50       # (a period of 4: at most 4 distinct windows)
    finally:
        m.close()


def estimate_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("estimate\t")]
    assert len(lines) == 1, out
    f = lines[0].split("\t")
    assert len(f) == 5
    return int(f[1]), int(f[2]), int(f[3]), f[4]


@pytest.mark.gpu
def test_cli_auto_and_estimate(T, tmp_path, golden_counts):
    k = 14
    text = open(os.path.join(GOLDEN, "small_t7.1000.fastq"), "rb").read()
    fq = tmp_path / "small_t7.1000.fastq"
    fq.write_bytes(text)
    with gzip.open(os.path.join(GOLDEN, "small_t7.1000.fastq.14.count.gz"), "rb") as f:
        (tmp_path / "small_t7.1000.fastq.14.count").write_bytes(f.read())
    want, tot, distinct = model_sketch(text, k)
    est = T.sketch_estimate(want)
    l = T.suggest_l(est, k)
    assert tot["kmers"] == sum(golden_counts.values()) and distinct == len(golden_counts)
    line = (tot["kmers"], int(round(est)), l, "%.3f" % (est / (1 << l)))
    code, out, err = run_cli("--input=" + str(fq), "--k=14", "--l=auto", "--mode=HIP", "--check")
    assert code == 0, err
    assert estimate_line(out) == line and "l=%d" % l in err
    assert "total errors0" in out and "tsxCount kmer count: %d" % distinct in out
    before = sorted(os.listdir(tmp_path))
    code, out, err = run_cli("--input=" + str(fq), "--k=14", "--estimate", "--l=3", "--output=" + str(tmp_path / "o.tsv"))
    assert code == 0 and estimate_line(out) == line and "Added a total" not in out, err
    assert sorted(os.listdir(tmp_path)) == before                # nothing counted, nothing written
    # .gz through zlib and BGZF through the device inflate, canonical
    wc, _, _ = model_sketch(text, k, canonical=True)
    ec = T.sketch_estimate(wc)
    lc = T.suggest_l(ec, k)
    cline = (tot["kmers"], int(round(ec)), lc, "%.3f" % (ec / (1 << lc)))
    gz, bg = tmp_path / "plain.fastq.gz", tmp_path / "blocked.fastq.gz"
    gz.write_bytes(gzip.compress(text))
    bg.write_bytes(T.bgzf_compress(text, block=20000))
    for path in (gz, bg):
        code, out, err = run_cli("--input=" + str(path), "--k=14", "--estimate", "--canonical")
        assert code == 0 and estimate_line(out) == cline, (path, err)
        assert ("Input is BGZF" in err) == (path == bg)
    code, out, err = run_cli("--input=" + str(fq), "--k=14", "--estimate", "--load-factor=0.3")
    assert code == 0 and estimate_line(out)[2] == T.suggest_l(est, k, load=0.3) == l + 1


@pytest.mark.gpu
def test_cli_auto_counts_what_overflows_a_guessed_table(T, tmp_path):
    k = 21
    text = genome_fasta(20000, 5)                                # 19 980 distinct k-mers: more than the 4 096 slots of l = 12
    fa = tmp_path / "genome.fa"
    fa.write_bytes(text)
    code, out, err = run_cli("--input=" + str(fa), "--k=21", "--l=12")
    assert code == 42, err
    code, out, err = run_cli("--input=" + str(fa), "--k=21", "--l=auto")
    assert code == 0, err
    kmers, distinct, l, _ = estimate_line(out)
    assert kmers == 20000 - k + 1 and l == 15 and abs(distinct / kmers - 1) <= sigma5(14)
    assert "Added a total of %d different kmers" % kmers in out
