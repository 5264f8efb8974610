"""Coverage tracks on the GPU: tsxcount_amd.track.sequence_track and its BGZF, device and file forms against track_bins
(CPU) over conftest.python_counts of the text the table was filled from.  Every integer matches exactly; names, stats and
offsets are those of querySequences on the same text; on every case the bins of a sequence sum to its stats row.

Shapes are the smallest that cross each border of csrc/tsx_track.h: a lane is 16 bytes, a wave row 64 start positions, a
tile 4096 bytes, the fold 256 bin rows.  The text of test_seq.make_case has a sequence of three tiles, a tile packed with
100 short sequences and records of 0 .. 400 bases at every wrap width."""
import os
import random

import pytest

from conftest import python_counts
from test_seq import T, case, counts_for, filled, rand_seq, wrap, substitute, TILE  # noqa: F401 -- T is the module's fixture

WINDOWS = [64, 100, 4096, 5000, 1 << 20]


@pytest.fixture(scope="module")
def track(T):
    from tsxcount_amd import track
    return track


_models = {}


def model(track, key, recs, D, k, W, lower=1, upper=None, canonical=False, acgt_only=False):
    """track_bins, made once per case and window."""
    key = (key, k, W, lower, upper, canonical, acgt_only)
    if key not in _models:
        _models[key] = track.track_bins(recs, D, k, W, lower, upper, canonical, acgt_only)
    return _models[key]


def rows_of(a):
    return [tuple(int(v) for v in r) for r in a]


def check_result(got, want, recs, query):
    """One (names, stats, first, bins) against the model (first, bins) and against querySequences (names, stats)."""
    names, stats, first, bins = got
    assert names == [n for n, _ in recs] and names == query[0]
    assert stats.dtype == query[1].dtype and rows_of(stats) == rows_of(query[1])
    assert [int(v) for v in first] == want[0]
    have = rows_of(bins)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(have, want[1])) if g != w]
    assert len(have) == len(want[1]) and not bad, (len(have), len(want[1]), bad[:5])
    for i, s in enumerate(rows_of(stats)):                                          # the bins sum to the stats row
        rows = have[int(first[i]):int(first[i + 1])]
        assert sum(r[0] for r in rows) == s[1] and sum(r[1] for r in rows) == s[2]
        assert sum(r[4] for r in rows) % (1 << 64) == s[4]
        assert min([r[2] for r in rows if r[0]], default=0) == s[3]


def check(T, track, m, key, text, recs, D, k, W, lower=1, upper=None, canonical=False, acgt_only=False, chunk_bytes=0):
    want = model(track, key, recs, D, k, W, lower, upper, canonical, acgt_only)
    got = track.sequence_track(m, text, W, lower, upper, chunk_bytes)
    check_result(got, want, recs, m.querySequences(text, lower, upper))
    return got


# ---- windows, widths and modes ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_every_window_at_k31(T, track, W):
    k = 31
    text, table, recs, D = case(T, k)
    m = filled(T, k, table)
    names, stats, first, bins = check(T, track, m, "case", text, recs, D, k, W)
    if W == 64:
        check(T, track, m, "case", text, recs, D, k, W, lower=2, upper=5)
    m.close()
    i = [n for n, _ in recs].index(b"long")
    rows = bins[int(first[i]):int(first[i + 1])]
    assert len(rows) == (3 * TILE + 5 + W - 1) // W
    assert int(rows["max_count"].max()) >= 2 and int(bins["min_count"].min()) == 0
    if W == 64:
        assert int(rows[-1]["kmers"]) == 0 and int(rows[0]["kmers"]) == 64         # a tail bin without k-mers, a full bin
    if W == 5000:
        assert [int(v) for v in rows["kmers"]] == [5000, 5000, 3 * TILE + 5 - 10000 - k + 1]   # bins fed by two tiles
    if W == 1 << 20:                                                                # one bin per sequence: the stats row
        assert len(bins) == sum(1 for _, s in recs if s) == len(stats)
        assert [(r[0], r[1], r[2], r[4]) for r in rows_of(bins)] == [r[1:] for r in rows_of(stats)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,kw", [(40, {}), (65, {"n_records": 30})])
def test_two_and_three_limb_keys(T, track, k, kw):
    text, table, recs, D = case(T, k, **kw)
    m = filled(T, k, table)
    for W in (64, 100):
        check(T, track, m, ("case", tuple(kw.items())), text, recs, D, k, W)
    m.close()


@pytest.mark.gpu
def test_canonical(T, track):
    k = 31
    text, table, recs, D = case(T, k)
    m = filled(T, k, table, canonical=True)
    for W in (64, 100):
        check(T, track, m, "case", text, recs, D, k, W, canonical=True)
    m.close()


@pytest.mark.gpu
def test_acgt_only_with_runs_of_n(T, track):
    k = 31
    text, table, recs, D = case(T, k, seed=2, n_runs=True)
    m = filled(T, k, table, acgt_only=True)
    for W in (64, 100):
        _, stats, first, bins = check(T, track, m, "case2n", text, recs, counts_for(D, True), k, W, acgt_only=True)
    m.close()
    i = [n for n, _ in recs].index(b"plant_tile")
    assert int(stats[i]["kmers"]) < int(stats[i]["length"]) - k + 1               # the N run lowers kmers


# ---- seams -----------------------------------------------------------------------------------------------------------------

def seam_case(T, k):
    """A text of its own: a 1000-base sequence on ONE line behind a 3-byte header (byte 3 + s of the text is base s), a
    sequence behind a long header line, a short one; the table holds them with a substitution every ~100 bases, the
    first twice."""
    rng = random.Random(21)
    a, b, c = rand_seq(rng, 1000), rand_seq(rng, 700), rand_seq(rng, 130)
    head = b">second with a header line of some length\n"
    text = b">h\n" + a + b"\n" + head + wrap(b, 60) + b"\n>c\n" + wrap(c, 50)
    mut = []
    for s in (a, b, c, a):
        for at in range(50, len(s), 100):
            s = substitute(s, at + rng.randrange(20), at + rng.randrange(20) + 1) if s is not a else s
        mut.append(s)
    mut[0] = substitute(a, 500, 501)
    table = b"".join(b">t\n" + wrap(s, 70) for s in mut)
    return text, table, T.fasta_records(text), python_counts(T.join_fasta(table), k, 2), text.index(head)


@pytest.mark.gpu
def test_host_pieces_cut_inside_a_bin_on_a_bin_border_in_a_header_and_in_the_carry(T, track):
    k, W = 31, 64
    text, table, recs, D, head_at = seam_case(T, k)
    m = filled(T, k, table, l=16)
    whole = check(T, track, m, "seam", text, recs, D, k, W)
    assert int(whole[3]["max_count"].max()) == 2
    on_border = 3 + 4 * W                                                           # the first seam: base 256 of sequence 0
    in_header = head_at + 10
    assert (on_border - 3) % W == 0 and (2 * on_border - 3) % W != 0                # on a border, then inside a bin
    assert text[head_at:head_at + 1] == b">" and b"\n" not in text[head_at:in_header + 1]
    for chunk in (on_border, in_header, k - 2, 16, 1000):                          # k - 2, 16: pieces shorter than the carry
        got = check(T, track, m, "seam", text, recs, D, k, W, chunk_bytes=chunk)
        assert got[3].tobytes() == whole[3].tobytes()
    for chunk in (3 + 100, 257):
        check(T, track, m, "seam", text, recs, D, k, 100, chunk_bytes=chunk)        # W = 100: a seam on base 100, then inside
    m.close()


@pytest.mark.gpu
def test_piece_bytes_of_256(T, track, monkeypatch):
    k = 31
    text, table, recs, D = case(T, k)
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "256")
    m = filled(T, k, table)
    for W in (64, 5000):
        check(T, track, m, "case", text, recs, D, k, W)
    m.close()


@pytest.mark.gpu
def test_device_windows_of_4096_bytes(T, track, monkeypatch):
    import torch
    k = 31
    text, table, recs, D = case(T, k)
    m = filled(T, k, table)
    buf = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    uncut = track.sequence_track_device(m, buf.data_ptr(), len(text), 100)
    monkeypatch.setenv("TSX_HIP_DEV_WINDOW", "4096")
    query = m.querySequences(text)
    for W in (64, 100, 5000):
        got = track.sequence_track_device(m, buf.data_ptr(), len(text), W)
        check_result(got, model(track, "case", recs, D, k, W), recs, query)
        if W == 100:
            assert got[3].tobytes() == uncut[3].tobytes() and got[2].tobytes() == uncut[2].tobytes()
    m.close()


@pytest.mark.gpu
def test_bgzf_batches(T, track, monkeypatch):
    k, W = 31, 100
    text, table, recs, D = case(T, k)
    big = text * 5                                                                  # (more than one batch of 128 KiB)
    assert len(big) > 2 * 131072
    z = T.bgzf_compress(big, level=1)
    m = filled(T, k, table)
    uncut = track.sequence_track_bgzf(m, z, W)
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "131072")
    got = track.sequence_track_bgzf(m, z, W)
    query = m.querySequences(big)
    m.close()
    # five copies of the text: each copy's first record (lines without a header) goes on with the copy before it
    want = model(track, "case5", T.fasta_records(big), D, k, W)
    check_result(got, want, T.fasta_records(big), query)
    assert got[3].tobytes() == uncut[3].tobytes() and got[2].tobytes() == uncut[2].tobytes()


# ---- more bin rows in a tile than the fold has slots -------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_tile_of_more_bin_rows_than_the_fold_has_slots(T, track):
    """600 sequences of 7 .. 9 bases on single lines, 10 .. 12 bytes each of the unwrapped text: a 4096-byte tile holds
    more than 340 of them, one bin row each, so the rows past the 256th of a tile take the direct atomics."""
    k, W = 7, 64
    rng = random.Random(17)
    seqs = [rand_seq(rng, 7 + i % 3) for i in range(600)]
    text = b"".join(b">q%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    assert TILE // 12 > 256
    recs = T.fasta_records(text)
    D = python_counts(T.join_fasta(text), k, 2)
    m = filled(T, k, text, l=13)
    names, stats, first, bins = check(T, track, m, "tiny", text, recs, D, k, W)
    check(T, track, m, "tiny", text, recs, D, k, W, chunk_bytes=1000)
    m.close()
    assert len(bins) == 600 and [int(v) for v in bins["kmers"]] == [len(s) - k + 1 for s in seqs]
    assert int(bins["min_count"].min()) >= 1 and int(bins["max_count"].max()) >= 2


# ---- the file and the refusals -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_written_track_is_format_track(T, track, tmp_path):
    k, W = 31, 100
    text, table, recs, D = case(T, k)
    m = filled(T, k, table)
    names, stats, first, bins = track.sequence_track(m, text, W)
    want = track.format_track(names, first, bins, W, stats["length"])
    path = str(tmp_path / "t.tsv")
    assert track.write_sequence_track(m, text, path, W) == len(bins)
    fd = os.open(str(tmp_path / "t2.tsv"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        assert track.write_sequence_track(m, text, fd, W) == len(bins)
    finally:
        os.close(fd)
    m.close()
    assert open(path, "rb").read() == want and open(str(tmp_path / "t2.tsv"), "rb").read() == want
    lines = want.split(b"\n")[:-1]
    assert len(lines) == len(bins) and any(l.startswith(b"*\t") for l in lines) and any(l.endswith(b"\tNA") for l in lines)
    model_first, model_bins = model(track, "case", recs, D, k, W)
    assert want == track.format_track([n for n, _ in recs], model_first, model_bins, W, [len(s) for _, s in recs])


@pytest.mark.gpu
def test_refusals(T, track, tmp_path):
    text = b">a\n" + b"ACGT" * 30 + b"\n"
    m = T.TSXHashMapHIP(16, 0, 21)
    for W in (63, (1 << 32) + 1, 0):
        for call in (lambda: track.sequence_track(m, text, W), lambda: track.sequence_track_bgzf(m, T.bgzf_compress(text), W),
                     lambda: track.sequence_track_device(m, 0, 0, W)):
            with pytest.raises(T.TSXException) as e:
                call()
            assert e.value.code == T.EINVAL and "window" in str(e.value)
    with pytest.raises(T.TSXException) as e:
        track.sequence_track(m, text, 64, lower=3, upper=2)
    assert e.value.code == T.EINVAL and "lower" in str(e.value)
    names, stats, first, bins = track.sequence_track(m, text, 1 << 32)            # the largest window is taken
    assert names == [b"a"] and [int(v) for v in first] == [0, 1] and rows_of(bins) == [(100, 0, 0, 0, 0)]
    # a result without a track has no bins and is not written
    L = T.lib()
    fd = os.open(str(tmp_path / "none.tsv"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        rc = m._seq_call(L.tsx_hip_seq_stats_host, (text, len(text), 1, (1 << 64) - 1, 0),
                         lambda res: (L.tsx_hip_seq_write_track(res, fd), L.tsx_hip_seq_result_window(res), L.tsx_hip_seq_result_bins(res, None, None)))
    finally:
        os.close(fd)
    assert rc == (T.EINVAL, 0, 0) and os.path.getsize(str(tmp_path / "none.tsv")) == 0
    m.close()
    m = T.TSXHashMapHIP(16, 0, 21, min_qual_char="5")
    with pytest.raises(T.TSXException) as e:
        track.sequence_track(m, text, 64)
    assert e.value.code == T.EINVAL and "quality" in str(e.value)
    m.close()
