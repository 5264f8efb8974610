"""The inputs of tests/test_seq_widths.py (tests/seq_design.py) are sharp, shown on the CPU reference alone: the cut
text holds every scenario the host-side carry of sequence identity tells apart and a cut offset for each of them, a
table whose lookups ignore part of the key answers otherwise on the sibling contigs, and the alternating contig emits
exactly the 2048 fragments per tile that SEQ_TILE_FRAGS (csrc/tsx_seq.h) allows while no other text emits more.  No GPU,
and no kernel is made wrong: the defects are stated on dictionaries."""
import pytest

import seq_design as S
import tsxcount_amd as T
import width_design as W
from conftest import python_counts

GPU_KS = [31, 32, 63, 64, 65, 80, 96, 97, 127]       # every k test_seq_widths.py runs sibling contigs at


def counts_of(table, k):
    return python_counts(T.join_fasta(table), k, 2)


# ---- the cut text --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 127])
def test_cut_text_holds_every_scenario(k):
    text, table = S.cut_text(k)
    recs = T.fasta_records(text)
    names = [n for n, _ in recs]
    assert names == S.cut_names(k)
    assert names[0] == b"" and names[1] == b"" and b"vanishes" not in names and b"after" in names
    assert S.TAB_NAME in names and S.LONG_NAME[:255] in names and len(S.LONG_NAME) > 255
    assert names[-2] == b"cr\r" and not text.endswith(b"\n") and text[:1] != b">"
    by = {n: s for n, s in recs[1:]}
    assert len(by[b"short"]) < k - 1 == len(by[S.LONG_NAME[:255]]) and len(by[b"exact"]) == k
    assert len(by[b"long"]) == 2 * k + 40 and b"\r" in by[b"cr\r"] and b">" in by[b"cr\r"]
    assert b">blank x\n\n\n\n" in text and b">vanishes\n>after\n" in text
    assert max(len(ln) for ln in text.split(b"\n") if ln[:1] != b">") <= max(60, k // 2 + 1)
    D = counts_of(table, k)
    stats = T.sequence_stats(recs, D, k)
    iv = T.missing_intervals(recs, D, k)
    assert any(s[1] == 0 for s in stats) and any(0 < s[2] < s[1] for s in stats) and any(s[1] and s[2] == s[1] for s in stats)
    assert any(s == 0 for _, s, _ in iv) and any(s > 0 for _, s, _ in iv)
    assert {s[3] for s in stats} >= {0, 1, 3, 5} and 2 in D.values()                # counts above 1 occur
    sib = names.index(b"sib")
    assert [(e - s) for r, s, e in iv if r == sib] == [2 * k - 1]                  # a run of exactly k windows
    assert stats[sib][2] == stats[sib][1] - k
    # another run pattern under lower = 2, upper = 3 and under a canonical table
    assert T.missing_intervals(recs, D, k, 2, 3) != iv and T.sequence_stats(recs, D, k, 2, 3) != stats
    assert any(0 < s[2] for s in T.sequence_stats(recs, D, k, 2, 3))


@pytest.mark.parametrize("k", [31, 127])
def test_every_cut_class_has_an_offset(k):
    text, table = S.cut_text(k)
    recs = T.fasta_records(text)
    iv = T.missing_intervals(recs, counts_of(table, k), k)
    classes = S.cut_classes(k, text, iv)
    assert len(classes) >= 20
    for name, at in classes.items():
        hits = [o for o in range(1, len(text) + 1) if at(o)]
        assert hits, name
        assert len(hits) < len(text) * 2 // 3, name                               # (a class, not everything)


def test_byte_map_follows_the_record_rules():
    text = b"AC\nG\n>a b\n\nTT\n>v\n>w\nC>\rA\n"
    recs = T.fasta_records(text)
    assert recs == [(b"", b"ACG"), (b"a", b"TT"), (b"w", b"C>\rA")]
    bm = S.byte_map(text)
    seq = {}
    for o, (kind, _, rec, nb) in enumerate(bm):
        assert (kind == "n") == (text[o:o + 1] == b"\n")
        if kind == "s":
            seq.setdefault(rec, []).append((nb, text[o:o + 1]))
    assert {r: b"".join(b for _, b in v) for r, v in seq.items()} == {i: s for i, (_, s) in enumerate(recs)}
    assert all([nb for nb, _ in v] == list(range(len(v))) for v in seq.values())


# ---- sibling contigs: sharp under every truncation ------------------------------------------------------------------------

def answers(recs, lookup, k, lower, upper):
    """sequence_stats and missing_intervals over a window lookup of its own (ACGT texts, no strand folding)."""
    stats, iv = [], []
    for r, (_, seq) in enumerate(recs):
        cs = [lookup(seq[i:i + k]) for i in range(len(seq) - k + 1)]
        stats.append((len(seq), len(cs), sum(lower <= c <= upper for c in cs), min(cs) if cs else 0, sum(cs)))
        start = None
        for i, c in enumerate(cs + [None]):
            miss = c is not None and not lower <= c <= upper
            if miss and start is None:
                start = i
            elif not miss and start is not None:
                iv.append((r, start, i - 1 + k))
                start = None
    return stats, iv


@pytest.mark.parametrize("k", GPU_KS)
def test_sibling_contigs_are_what_the_design_says(k):
    sib = S.sibling_contigs(k)
    wk = (2 * k + 63) // 64
    assert len(sib.cross) == len(sib.within) == wk + (1 if (2 * k) % 64 else 0)
    assert len(S.limb_positions(k)) == wk and all(32 * i <= o < min(32 * (i + 1), k) for i, o in enumerate(S.limb_positions(k)))
    for canonical in (False, True):
        text = sib.query(canonical)
        recs = T.fasta_records(text)
        cs = sib.contigs(canonical)
        assert [n for n, _ in recs] == [c.name for c in cs] and [s for _, s in recs] == [c.seq for c in cs]
        assert max(len(ln) for ln in text.split(b"\n")) <= 60
        D = counts_of(sib.table_canonical if canonical else sib.table, k)
        # a tile border of the unwrapped text among the start positions of cross pair 0's covering windows
        b, p0 = sib.border_offset(canonical), cs[1].p
        assert cs[1].kind == "cross" and p0 - k + 1 < b <= p0
        assert T.join_fasta(text).index(cs[1].seq) + b == S.TILE
        for lo, up in ((1, None), (2, 2), (5, 5)):
            stats = T.sequence_stats(recs, D, k, lo, up, canonical)
            iv = T.missing_intervals(recs, D, k, lo, up, canonical)
            for r, c in enumerate(cs):
                mine = [(s, e) for rr, s, e in iv if rr == r]
                n = len(c.seq) - k + 1
                assert stats[r][:2] == (len(c.seq), n)
                if c.kind == "filler":
                    assert stats[r][2:4] == ((n, 1) if lo == 1 else (0, 1))
                elif c.kind == "cross" and lo == 1:
                    assert mine == [(c.p - k + 1, c.p + k)] and stats[r][2] == n - k and stats[r][3] == 0
                elif c.kind in ("within2", "within5"):
                    own = int(c.kind[-1])
                    assert stats[r][3] == own and stats[r][4] == 7 * (n - k) + own * k
                    assert stats[r][2] == (n if lo == 1 else k if lo == own else 0)
                    if lo == own:                                             # only the covering windows are in range
                        assert mine == [(0, c.p), (c.p + 1, len(c.seq))]
                elif c.kind == "pal":
                    assert stats[r][3] == 3 and stats[r][1] == 3
        if canonical:
            assert sum(c.name.endswith(b"_rc") for c in cs) >= len(cs) // 2 - 1
            assert (sib.pal is not None) == (k % 2 == 0) == (cs[-1].kind == "pal")


@pytest.mark.parametrize("k", GPU_KS)
def test_a_truncated_key_answers_otherwise_on_the_sibling_contigs(k):
    sib = S.sibling_contigs(k)
    recs = T.fasta_records(sib.query())
    kinds = [c.kind for c in sib.contigs()]
    D = counts_of(sib.table, k)
    cuts = W.truncations(k)
    assert cuts and all(0 < n < k for n in cuts.values())
    U = (1 << 64) - 1
    for lo, up in ((1, U), (2, 2), (5, 5)):
        exact = answers(recs, lambda x: D.get(x, 0), k, lo, up)
        assert exact == (T.sequence_stats(recs, D, k, lo, up), T.missing_intervals(recs, D, k, lo, up))
        for label, n in cuts.items():
            Dn = W.truncated(D, n)
            stats, iv = answers(recs, lambda x: Dn.get(x[:n], 0), k, lo, up)
            want = "cross" if lo == 1 else "within%d" % lo
            for r, kind in enumerate(kinds):
                if kind == want:                                               # every such contig, not one by chance
                    assert stats[r] != exact[0][r], (label, lo, r)
                    assert [v for v in iv if v[0] == r] != [v for v in exact[1] if v[0] == r], (label, lo, r)


@pytest.mark.parametrize("k", [63, 65, 127])
def test_runs_of_n_cut_and_split_the_missing_intervals(k):
    sib = S.sibling_contigs(k)
    text, table, contigs, doubles = S.with_n_runs(sib)
    recs = T.fasta_records(text)
    assert [n for n, _ in recs] == [c[0] for c in contigs]
    D = counts_of(table, k)
    on = T.missing_intervals(recs, D, k, acgt_only=True)
    off = T.missing_intervals(recs, D, k, acgt_only=False)
    s_on, s_off = T.sequence_stats(recs, D, k, acgt_only=True), T.sequence_stats(recs, D, k)
    assert on != off and s_on != s_off
    cross = [r for r, c in enumerate(contigs) if c[2] == "cross"]
    for i, r in enumerate(cross):
        p = sib.cross[i][2]
        assert [(s, e) for rr, s, e in on if rr == r] == [(p - 3, p + k)]         # cut short by the run in front of p
        assert s_on[r][1] == s_off[r][1] - (p - 4 - max(p - 5 - k + 1, 0) + 1)    # the windows over the run of 2
    dbl = [r for r, c in enumerate(contigs) if c[2] == "double"]
    for r, (_, p) in zip(dbl, doubles):
        assert [(s, e) for rr, s, e in on if rr == r] == [(p - k + 1, p + 1), (p + 3, p + 2 * k)]   # split in two
    low = [c[0] for c in contigs].index(b"lower")
    assert s_on[low] == s_off[low] and s_on[low][2] == s_on[low][1] - k           # lower case is a base under both rules
    iu = [c[0] for c in contigs].index(b"iupac")
    assert s_on[iu][1] == s_off[iu][1] - k and s_off[iu][2] < s_off[iu][1] - k    # R: dropped, or looked up as its stand-in
    assert any(0x4E in s for _, s in recs)


# ---- the fragment bound --------------------------------------------------------------------------------------------------

def test_the_alternating_contig_reaches_the_fragment_bound_exactly():
    k, n_tiles = 31, 3
    contig, kmers, counts = S.alternating(k, n_tiles)
    assert len(S.alternating_limbs(kmers, k)) == len(kmers) == len(counts)
    D = dict(zip(kmers, counts))
    recs = T.fasta_records(S.fasta(b"alt", contig))
    n = len(contig) - k + 1
    iv = T.missing_intervals(recs, D, k)
    assert iv == [(0, i, i + k) for i in range(1, n, 2)]                          # every odd start, none merged
    assert T.sequence_stats(recs, D, k)[0][1:3] == (n, (n + 1) // 2)
    tiles = S.fragments_per_tile(recs, D, k)
    assert tiles[0] == S.TILE_FRAGS - 1                                           # (tile 0 begins with ">\n")
    assert tiles[1:n_tiles + 1] == [S.TILE_FRAGS] * n_tiles and len(tiles) == n_tiles + 2
    assert sum(tiles) == len(iv)


def test_no_text_of_the_suite_passes_the_fragment_bound():
    import test_seq
    texts = []
    for k in (31, 127):
        text, table = S.cut_text(k)
        texts.append((text, table, k, {}))
        texts.append((text, table, k, dict(lower=2, upper=3)))
    for k in (31, 65, 127):
        sib = S.sibling_contigs(k)
        texts.append((sib.query(), sib.table, k, {}))
        texts.append((sib.query(), sib.table, k, dict(lower=5, upper=5)))
        texts.append((sib.query(True), sib.table_canonical, k, dict(canonical=True)))
    text, table, _, _ = S.with_n_runs(S.sibling_contigs(65))
    texts.append((text, table, 65, dict(acgt_only=True)))
    text, table = test_seq.make_case(1, 31)
    texts.append((text, table, 31, {}))
    texts.append((text, b">a\n" + b"ACGT" * 20 + b"\n", 31, {}))                # nothing present: one run per sequence
    for text, table, k, kw in texts:
        tiles = S.fragments_per_tile(T.fasta_records(text), counts_of(table, k), k, **kw)
        assert tiles and 0 < max(tiles) <= S.TILE_FRAGS, (k, kw, max(tiles))


def test_the_fragment_model_on_a_text_counted_by_hand():
    k = 4
    seq = b"A" * 70 + b"C" * 70                                                    # windows 0 .. 66 AAAA, 67 .. 69 mixed, 70 .. CCCC
    recs = [(b"a", seq), (b"b", b"G" * 10)]
    D = {b"CCCC": 1}
    assert T.missing_intervals(recs, D, k) == [(0, 0, 73), (1, 0, 10)]
    # run 1: text positions 2 .. 71 (rows 0 and 1); run 2: starts 0 .. 6 of record b at 2 + 140 + 3 .. (row 2)
    assert S.fragments_per_tile(recs, D, k) == [3]
