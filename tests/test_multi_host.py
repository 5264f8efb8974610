"""The C++ multi-GPU host (csrc/tsx_multi.cpp, tsx_hip_group_*): record cuts on the CPU; on the GPU the group with
its collective as device copies (2 and 8 ranks sharing cuda:0 -- RCCL wants one GPU per rank) and through the RCCL
API with the one rank a one-GPU box can give it; the minimizer exchange in many rounds (small pieces and shares through
TSX_HIP_MZ_PIECE / TSX_HIP_MZ_SHARE); the CLI's --gpus."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, python_counts


KIB = 1 << 10
MIB = 1 << 20


def _mini_rounds(max_len, piece, share):
    """pieces x shares of the C++ minimizer exchange for a longest shard of max_len bytes (mini_geometry in
    csrc/tsx_multi.cpp): TSX_HIP_MZ_PIECE rounded up to 4096, never more than the shard needs; 1 .. 4 shares."""
    piece = min(max(4096, (piece + 4095) & ~4095), 2 << 30)
    piece_bytes = min(piece, max(4096, (max_len + 4095) & ~4095))
    pieces = max(1, -(-max_len // piece_bytes))
    parts = max(1, min(4, piece_bytes // share))
    return pieces * parts, piece_bytes


def _fasta_of(fastq_text):
    lines = fastq_text.split(b"\n")
    return b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))


def _random_bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


@functools.lru_cache(maxsize=None)
def _uneven_fasta():
    """Two-line FASTA texts for 4 ranks, a piece of 32 KiB: (one record of 300 000 bases among six of 500: a shard of many
    pieces whose seams are all inside one line, a shard shorter than a piece, empty shards in between; two records only:
    two of the four shards are empty and still take part in every round)."""
    rng = np.random.default_rng(41)
    small = [b">s%d\n" % i + _random_bases(rng, 500) + b"\n" for i in range(6)]
    long_rec = b">long\n" + _random_bases(rng, 300000) + b"\n"
    two = b">a\n" + _random_bases(rng, 40000) + b"\n>b\n" + _random_bases(rng, 30000) + b"\n"
    return b"".join(small[:2]) + long_rec + b"".join(small[2:]), two


UNEVEN_RANKS, UNEVEN_PIECE, UNEVEN_SHARE = 4, 32 * KIB, 8 * KIB


def _check_uneven_fixture():
    """The preconditions of the uneven texts, from cut_records alone; returns the shard sizes of both."""
    import tsxcount_amd as T
    text, two = _uneven_fasta()
    sizes = np.diff(T.cut_records(text, UNEVEN_RANKS, 2))
    assert sizes.max() >= 4 * UNEVEN_PIECE                                  # one shard spans >= 4 pieces
    assert any(0 < s < UNEVEN_PIECE for s in sizes)                         # a non-empty shard shorter than a piece
    assert max(len(l) for l in text.split(b"\n")) > 4 * UNEVEN_PIECE        # and its seams are inside one line
    sizes2 = np.diff(T.cut_records(two, UNEVEN_RANKS, 2))
    assert (sizes2 == 0).sum() >= 2 and (sizes2 > 0).sum() == 2             # two records: at least two ranks have nothing
    return sizes, sizes2


POLY_K, POLY_PIECE, POLY_SHARE, POLY_READ = 31, MIB, 512 * KIB, 1000
POLY_PLAN = int(4096 * 10 * 6 * 1.2) + 65536     # est_total of a rank that received nothing in round 0 of 6


@functools.lru_cache(maxsize=None)
def _polyfirst_fasta(ranks):
    """`ranks` shards of two-line FASTA records of 1 000 bases, each just below 3 MiB (3 pieces of 1 MiB x 2 shares = 6
    rounds): 1 044 poly-A records (more than 1 MiB + 4 KiB), then 2 073 random reads, about 2e6 distinct k-mers.  The
    headers have one width, so every shard has the same length and cut_records cuts exactly between them."""
    rng = np.random.default_rng(43)
    recs = []
    for r in range(ranks):
        for i in range(3117):
            seq = b"A" * POLY_READ if i < 1044 else _random_bases(rng, POLY_READ)
            recs.append(b">%d%05d\n" % (r, i) + seq + b"\n")
    return b"".join(recs)


def _check_polyfirst_fixture(ranks):
    """Every shard runs 6 rounds, and its first piece (and 4 KiB more) holds only headers, 'A' and newlines."""
    import tsxcount_amd as T
    text = _polyfirst_fasta(ranks)
    cuts = T.cut_records(text, ranks, 2)
    sizes = np.diff(cuts)
    assert sizes.min() > 2 * POLY_PIECE and sizes.max() <= 3 * POLY_PIECE
    assert _mini_rounds(int(sizes.max()), POLY_PIECE, POLY_SHARE) == (6, POLY_PIECE)
    for r in range(ranks):
        head = text[cuts[r]:cuts[r] + POLY_PIECE + 4 * KIB]
        assert len(head) == POLY_PIECE + 4 * KIB
        assert all(l[:1] == b">" or l.strip(b"A") == b"" for l in head.split(b"\n")), r
        assert head[:1] == b">"
    return cuts


def test_minimizer_round_fixtures():
    """The texts of the multi-round exchange tests keep exercising what they are for: shard sizes against the piece, the
    empty shards, the poly-A-only first pieces -- from cut_records alone, so a change of the cuts shows on a CPU run."""
    import tsxcount_amd as T
    sizes, sizes2 = _check_uneven_fixture()
    assert _mini_rounds(int(sizes.max()), UNEVEN_PIECE, UNEVEN_SHARE)[0] >= 4 * 4
    assert _mini_rounds(int(sizes2.max()), UNEVEN_PIECE, UNEVEN_SHARE)[0] >= 4
    for text in _uneven_fasta():
        cuts = T.cut_records(text, UNEVEN_RANKS, 2)
        assert all(_is_record_boundary(text, c, 2) for c in cuts)
        whole = python_counts(text, 31, 2)
        got = sum((python_counts(text[cuts[i]:cuts[i + 1]], 31, 2) for i in range(UNEVEN_RANKS)), type(whole)())
        assert got == whole
    for ranks in (1, 2):
        cuts = _check_polyfirst_fixture(ranks)
        text = _polyfirst_fasta(ranks)
        # every record is one read of POLY_READ bases: with k = POLY_READ a k-mer is a whole read, and the shards hold
        # every read of the text exactly once (which is the same statement for every smaller k)
        whole = python_counts(text, POLY_READ, 2)
        assert sum(whole.values()) == 3117 * ranks and whole[b"A" * POLY_READ] == 1044 * ranks
        got = sum((python_counts(text[cuts[i]:cuts[i + 1]], POLY_READ, 2) for i in range(ranks)), type(whole)())
        assert got == whole
    # the geometry the tests expect of the library: clamps and rounding of the piece, 1 .. 4 shares
    assert _mini_rounds(700000, 128 * KIB, 32 * KIB) == (6 * 4, 128 * KIB)
    assert _mini_rounds(100000, 1, 1) == (25 * 4, 4096)
    assert _mini_rounds(100000, 5000, 5000) == (13, 8192)
    assert _mini_rounds(100000, 2 << 30, 32 << 20) == (1, 102400)


def _is_record_boundary(text, cut, lines_per_record):
    """cut is 0, len(text), or right behind the terminator of the last line of a record (reference rules:
    empty lines do not count, FastXReader.h:365-370)."""
    if cut in (0, len(text)):
        return True
    if text[cut - 1:cut] != b"\n":
        return False
    lines = [l for l in text[:cut].split(b"\n") if l]
    return len(lines) % lines_per_record == 0


@pytest.mark.parametrize("lines", [4, 2])
def test_record_cuts_are_record_boundaries(lines):
    import tsxcount_amd as T
    from tsxcount_amd import synth
    rng = np.random.default_rng(3)
    fq = synth.fastq(7, 0, 61)
    if lines == 2:
        ls = fq.split(b"\n")
        fq = b"".join(b">" + ls[i][1:] + b"\n" + ls[i + 1] + b"\n" for i in range(0, len(ls) - 1, 4))
    # empty lines sprinkled in (they are dropped by the reader and must not shift the record count), no final newline
    parts = fq.split(b"\n")
    for _ in range(25):
        parts.insert(int(rng.integers(0, len(parts))), b"")
    messy = b"\n".join(parts).rstrip(b"\n")
    for text in (fq, messy, b"", b"\n\n\n", fq[:200]):
        for n in (1, 2, 3, 8, 64):
            cuts = T.cut_records(text, n, lines)
            assert cuts[0] == 0 and cuts[-1] == len(text) and cuts == sorted(cuts)
            assert all(_is_record_boundary(text, c, lines) for c in cuts), (n, cuts)
            # the shards together hold every k-mer of the text exactly once
            whole = python_counts(text, 21, lines)
            got = sum((python_counts(text[cuts[i]:cuts[i + 1]], 21, lines) for i in range(n)), type(whole)())
            assert got == whole
    # a balanced text gives balanced shards
    cuts = T.cut_records(fq, 8, lines)
    sizes = np.diff(cuts)
    assert sizes.min() > 0.5 * len(fq) / 8 and sizes.max() < 1.5 * len(fq) / 8


@pytest.mark.gpu
@pytest.mark.parametrize("ranks,k,l,s", [(2, 31, 18, 0), (8, 31, 17, 0), (4, 63, 17, 0), (8, 127, 16, 2), (3, 21, 17, 4)])
def test_group_counts_equal_the_oracle(ranks, k, l, s):
    """N tables on cuda:0, the collective as device copies behind a barrier: record shards, per-GPU counts, the merge
    (partition by owner, all-to-all, clear, re-insert with counts), lookups at the owner.  Any N, any k (config 5's
    k = 127 with --s=2 counters: every hot k-mer carries into the secondary array before and after the merge)."""
    import tsxcount_amd as T
    from oracle.oracle import Oracle
    from tsxcount_amd import synth
    text = synth.fastq(91, 0, 90 if k < 100 else 40)
    o = Oracle(k, 20, 4, seed=1)
    n = o.count_fastq(text)
    kmers, counts = o.dump()
    g = T.TSXHashMapHIPGroup(ranks, l, s, k, devices=[0] * ranks, comm="copy")
    assert g.comm_name() == "copy"
    for rep in (1, 2):      # a second count after clear(): the same tables, the same answer
        g.countFastq(text)
        st = g.stats()
        assert st["distinct"] == len(kmers) and st["count_sum"] == n and st["insert_failures"] == 0
        assert np.array_equal(g.getKmerCounts(kmers), counts)
        per = [g.rank_stats(r)["distinct"] for r in range(ranks)]
        assert sum(per) == len(kmers) and min(per) > 0.5 * len(kmers) / ranks      # every k-mer on one GPU, spread evenly
        assert 0 < g.exchanged_entries() <= sum(per) * 2
        g.clear()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ranks,k,l", [(2, 31, 23), (3, 20, 23), (8, 31, 23), (5, 32, 23), (1, 26, 23)])
def test_group_minimizer_exchange_equals_the_oracle(ranks, k, l):
    """The C++ group with the minimizer exchange (tsx_hip_group_set_exchange 1): record shards, every GPU describes and
    splits its own, the lists travel (device copies behind a barrier here), every GPU walks what it owns, one build; the
    homopolymer totals on their owners.  Every k-mer on the rank tsx_hip_mini_owner_host names and only there; a second
    count doubles everything; FASTA; outside 20 <= k <= 32 the mode is refused."""
    import tsxcount_amd as T
    from tsxcount_amd import distributed as TD
    text, n, kmers, counts = _synth_oracle(k, 700)
    owner = TD.owner_of(kmers, k, ranks)
    g = T.TSXHashMapHIPGroup(ranks, l, 0, k, devices=[0] * ranks, comm="copy", exchange="mini")
    for rep in (1, 2):
        g.countFastq(text)
        st = g.stats()
        assert st["distinct"] == len(kmers) and st["count_sum"] == rep * n and st["insert_failures"] == 0
        assert np.array_equal(g.getKmerCounts(kmers), rep * counts)
        for r in range(ranks):
            assert g.rank_stats(r)["distinct"] == int((owner == r).sum())
    g.clear()
    g.set_record_lines(2)
    lines = text.split(b"\n")
    fasta = b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 4))
    g.countFastq(fasta)
    assert np.array_equal(g.getKmerCounts(kmers), counts)
    g.close()
    with pytest.raises(T.TSXException):
        T.TSXHashMapHIPGroup(2, 19, 0, 63, devices=[0, 0], comm="copy", exchange="mini")


@functools.lru_cache(maxsize=None)
def _synth_oracle(k, reads):
    """(text, k-mer occurrences, k-mers, counts) of synth.fastq(93, 0, reads) from the oracle, counted once per (k, reads)
    and shared by the tests of the minimizer exchange; the arrays are read-only."""
    from oracle.oracle import Oracle
    from tsxcount_amd import synth
    text = synth.fastq(93, 0, reads)
    o = Oracle(k, 21, 4, seed=1)
    n = o.count_fastq(text)
    kmers, counts = o.dump()
    o.close()
    assert len(kmers) < 0.5 * (1 << 21)
    kmers.setflags(write=False)
    counts.setflags(write=False)
    return text, n, kmers, counts


@functools.lru_cache(maxsize=None)
def _polyfirst_oracles():
    """ranks -> (k-mer occurrences, k-mers, counts) of _polyfirst_fasta(ranks), ranks 1 and 2, from ONE oracle table: the
    text of two ranks is the text of one rank and one more shard, so the table is dumped, counts the second shard on top
    and is dumped again -- every shard goes through the oracle once."""
    from oracle.oracle import Oracle
    one, two = _polyfirst_fasta(1), _polyfirst_fasta(2)
    assert two[:len(one)] == one
    o = Oracle(POLY_K, 24, 4, seed=1)
    out, n = {}, 0
    for ranks, more in ((1, one), (2, two[len(one):])):
        n += o.count_fastq(more, 2)
        kmers, counts = o.dump()
        assert len(kmers) < 0.5 * (1 << 24)
        kmers.setflags(write=False)
        counts.setflags(write=False)
        out[ranks] = (n, kmers, counts)
    o.close()
    return out


def _set_geometry(monkeypatch, piece, share):
    if piece is None:
        monkeypatch.delenv("TSX_HIP_MZ_PIECE", raising=False)
        monkeypatch.delenv("TSX_HIP_MZ_SHARE", raising=False)
    else:
        monkeypatch.setenv("TSX_HIP_MZ_PIECE", str(piece))
        monkeypatch.setenv("TSX_HIP_MZ_SHARE", str(share))


def _rank_kmers(g, rank):
    """(k-mers, counts) of one rank's table: tsx_hip_dump_host on tsx_hip_group_map(rank); order unspecified."""
    import ctypes
    import tsxcount_amd as T
    L = T.lib()
    n = max(g.rank_stats(rank)["distinct"], 1)
    kmers, counts = np.zeros((n, g.wk), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    got = ctypes.c_size_t(0)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    rc = L.tsx_hip_dump_host(L.tsx_hip_group_map(g._h, rank), kmers.ctypes.data_as(u64p), counts.ctypes.data_as(u64p), n, ctypes.byref(got))
    assert rc == T.OK
    return kmers[:got.value], counts[:got.value]


def _rank_dumps(g, ranks):
    """rank -> (sorted k-mers, their counts)."""
    out = []
    for r in range(ranks):
        dk, dc = _rank_kmers(g, r)
        order = np.argsort(dk[:, 0], kind="stable")
        out.append((dk[order, 0].copy(), dc[order].copy()))
    return out


def _exact_against_oracle(g, ranks, k, kmers, counts, n, times=1):
    from tsxcount_amd import distributed as TD
    owner = TD.owner_of(kmers, k, ranks)
    st = g.stats()
    assert st["distinct"] == len(kmers) and st["count_sum"] == times * n and st["insert_failures"] == 0
    assert np.array_equal(g.getKmerCounts(kmers), times * counts)
    for r in range(ranks):
        assert g.rank_stats(r)["distinct"] == int((owner == r).sum())
    return owner


def _one_round_dumps(monkeypatch, ranks, l, k, texts):
    """lines -> the per-rank tables of the same count with the geometry left alone (one round), for every (lines, text);
    one group, cleared between the texts."""
    import tsxcount_amd as T
    _set_geometry(monkeypatch, None, None)
    g = T.TSXHashMapHIPGroup(ranks, l, 0, k, devices=[0] * ranks, comm="copy", exchange="mini")
    dumps = {}
    for lines, text in texts:
        g.clear()
        g.set_record_lines(lines)
        g.countFastq(text)
        assert g.exchange_rounds() == 1
        dumps[lines] = _rank_dumps(g, ranks)
    g.close()
    return dumps


def _same_dumps(a, b):
    assert len(a) == len(b)
    for r, ((ka, ca), (kb, cb)) in enumerate(zip(a, b)):
        assert np.array_equal(ka, kb) and np.array_equal(ca, cb), "rank %d" % r


@pytest.mark.gpu
@pytest.mark.parametrize("ranks,k,reads,piece,share", [(2, 31, 700, 128 * KIB, 32 * KIB), (3, 20, 700, 64 * KIB, 21 * KIB),
                                                       (8, 31, 700, 32 * KIB, 8 * KIB), (5, 32, 200, 4096, 1024),
                                                       (1, 26, 300, 64 * KIB, 64 * KIB), (4, 24, 300, 4096, 4096)])
def test_group_minimizer_exchange_over_many_rounds(monkeypatch, ranks, k, reads, piece, share):
    """The minimizer exchange of the C++ group with small pieces and shares (TSX_HIP_MZ_PIECE, TSX_HIP_MZ_SHARE): what only
    happens from the second round on -- a split behind a walk, appending walks, a describe at an offset with a cut inside
    a line or a record, a receive buffer that grows, a level-1 plan fixed in round 0, homopolymer totals summed over
    rounds, ranks whose shard ended pieces ago.  Exactly the oracle's counts, every k-mer on its owner, a second count
    doubles, FASTA; the number of rounds is the one the geometry asks for; and every rank's table is the one a single
    round gives."""
    import tsxcount_amd as T
    l = 23
    text, n, kmers, counts = _synth_oracle(k, reads)
    fasta = _fasta_of(text)
    want = {}
    for lines, t in ((4, text), (2, fasta)):
        want[lines] = _mini_rounds(int(max(np.diff(T.cut_records(t, ranks, lines)))), piece, share)[0]
        assert want[lines] >= 4
    one = _one_round_dumps(monkeypatch, ranks, l, k, ((4, text), (2, fasta)))
    _set_geometry(monkeypatch, piece, share)
    g = T.TSXHashMapHIPGroup(ranks, l, 0, k, devices=[0] * ranks, comm="copy", exchange="mini")
    for rep in (1, 2):
        g.countFastq(text)
        assert g.exchange_rounds() == want[4]
        _exact_against_oracle(g, ranks, k, kmers, counts, n, rep)
        if rep == 1:
            _same_dumps(_rank_dumps(g, ranks), one[4])
    g.clear()
    g.set_record_lines(2)
    g.countFastq(fasta)
    assert g.exchange_rounds() == want[2]
    _exact_against_oracle(g, ranks, k, kmers, counts, n)
    _same_dumps(_rank_dumps(g, ranks), one[2])
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_group_minimizer_exchange_uneven_and_empty_shards(monkeypatch, which):
    """Shards of very different length in one exchange: a record of 300 000 bases (ten pieces, every seam inside the
    line) beside a shard shorter than a piece and empty ones; and two records on four ranks.  A rank without text
    describes nothing (len 0) in every round and still walks what the others send."""
    import tsxcount_amd as T
    from oracle.oracle import Oracle
    ranks, k, l = UNEVEN_RANKS, 31, 23
    sizes = _check_uneven_fixture()[which]
    text = _uneven_fasta()[which]
    o = Oracle(k, 20, 4, seed=1)
    n = o.count_fastq(text, 2)
    kmers, counts = o.dump()
    assert len(kmers) < 0.5 * (1 << 20)
    want = _mini_rounds(int(sizes.max()), UNEVEN_PIECE, UNEVEN_SHARE)[0]
    assert want >= 4
    one = _one_round_dumps(monkeypatch, ranks, l, k, ((2, text),))[2]
    _set_geometry(monkeypatch, UNEVEN_PIECE, UNEVEN_SHARE)
    g = T.TSXHashMapHIPGroup(ranks, l, 0, k, devices=[0] * ranks, comm="copy", exchange="mini")
    g.set_record_lines(2)
    g.countFastq(text)
    assert g.exchange_rounds() == want
    _exact_against_oracle(g, ranks, k, kmers, counts, n)
    _same_dumps(_rank_dumps(g, ranks), one)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [1, 2])
def test_group_minimizer_exchange_first_piece_yields_nothing(monkeypatch, ranks):
    """Every shard opens with more than a piece of poly-A records (asserted on the text).  The sender counts homopolymer
    k-mers itself and takes them out of the descriptions, so every rank should receive 0 descriptions in the rounds of
    the first piece: its receive buffer then starts at its floor and must grow, and the level-1 plan made in round 0 is
    POLY_PLAN keys, several times too small for the 2e6 keys per shard that follow.  That the plan on the device is
    POLY_PLAN is inferred from the text and from mini_rank's formula, not observed: the library reports neither the
    descriptions of a round nor its plan.  What is observed: 6 rounds, more distinct k-mers on every rank than POLY_PLAN,
    the oracle's counts exactly, no insert failure (the slack of the level-1 lists, the overflow queues and the
    deferred list take the excess), the poly-A k-mer with the oracle's count on its owner and nowhere else."""
    import tsxcount_amd as T
    k, l = POLY_K, 23
    _check_polyfirst_fixture(ranks)
    text = _polyfirst_fasta(ranks)
    n, kmers, counts = _polyfirst_oracles()[ranks]
    _set_geometry(monkeypatch, POLY_PIECE, POLY_SHARE)
    g = T.TSXHashMapHIPGroup(ranks, l, 0, k, devices=[0] * ranks, comm="copy", exchange="mini")
    g.set_record_lines(2)
    g.countFastq(text)
    assert g.exchange_rounds() == 6
    owner = _exact_against_oracle(g, ranks, k, kmers, counts, n)
    assert min(g.rank_stats(r)["distinct"] for r in range(ranks)) > POLY_PLAN
    # the poly-A k-mer (code 0): the oracle's count, on the rank tsx_hip_mini_owner_host names and nowhere else
    polya = np.zeros(1, dtype=np.uint64)
    at = np.flatnonzero(kmers[:, 0] == 0)
    assert len(at) == 1 and int(counts[at[0]]) == 1044 * ranks * (POLY_READ - k + 1)
    assert int(g.getKmerCounts(polya)[0]) == int(counts[at[0]])
    home = int(owner[at[0]])
    for r in range(ranks):
        dk, dc = _rank_kmers(g, r)
        hit = np.flatnonzero(dk[:, 0] == 0)
        assert len(hit) == (1 if r == home else 0)
        if r == home:
            assert int(dc[hit[0]]) == int(counts[at[0]])
    g.close()


@pytest.mark.gpu
def test_group_of_one_through_the_rccl_api():
    """ncclCommInitAll with the one GPU of this box, the merge's all-to-all as grouped ncclSend/ncclRecv from rank 0
    to rank 0: the RCCL leg of the C++ host through its API (N > 1 needs one GPU per rank)."""
    import tsxcount_amd as T
    from oracle.oracle import Oracle
    from tsxcount_amd import synth
    text = synth.fastq(92, 0, 120)
    o = Oracle(31, 20, 4, seed=1)
    n = o.count_fastq(text)
    kmers, counts = o.dump()
    g = T.TSXHashMapHIPGroup(1, 19, 0, 31, comm="rccl")
    assert g.comm_name() == "rccl"
    g.countFastq(text)
    st = g.stats()
    assert st["distinct"] == len(kmers) and st["count_sum"] == n
    assert np.array_equal(g.getKmerCounts(kmers), counts)
    g.close()
    # the minimizer exchange's lists (pieces that are not neighbours in memory) through the same grouped send / recv
    g = T.TSXHashMapHIPGroup(1, 23, 0, 31, comm="rccl", exchange="mini")
    g.countFastq(text)
    st = g.stats()
    assert st["distinct"] == len(kmers) and st["count_sum"] == n
    assert np.array_equal(g.getKmerCounts(kmers), counts)
    g.close()
    with pytest.raises(T.TSXException):       # RCCL refuses two ranks on one GPU: reported, not attempted
        T.TSXHashMapHIPGroup(2, 19, 0, 31, devices=[0, 0], comm="rccl")


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["--gpus=2", "--comm=copy", "--devices=0,0"], ["--gpus=8", "--comm=copy", "--devices=0,0,0,0,0,0,0,0", "--exchange=merge"],
                                  ["--gpus=1"]])
def test_cli_gpus_check_passes_on_golden(tmp_path, args):
    """tsxCount --mode=HIP --gpus=N --check on the reference's own fixture: one command runs the job
    (src/mains/main.cpp:404-507), the reference's console lines, `total errors0`."""
    text = open(os.path.join(GOLDEN, "small_t7.1000.fastq"), "rb").read()
    fq = tmp_path / "small_t7.1000.fastq"
    fq.write_bytes(text)
    with gzip.open(os.path.join(GOLDEN, "small_t7.1000.fastq.14.count.gz"), "rb") as f:
        (tmp_path / "small_t7.1000.fastq.14.count").write_bytes(f.read())
    exe = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
    p = subprocess.run([exe, "--input=%s" % fq, "--mode=HIP", "--l=20", "--check", "--checkabort"] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, out + err
    assert "Added a total of 194697 different kmers" in out and "total errors0" in out
    assert "entries moved between GPUs by the merge" in err and "exchange: per-GPU tables merged" in err


@pytest.mark.gpu
@pytest.mark.parametrize("args,how", [(["--gpus=4", "--comm=copy", "--devices=0,0,0,0"], "minimizer"), (["--gpus=2", "--comm=copy", "--devices=0,0"], "merged"),
                                      (["--gpus=3", "--comm=copy", "--devices=0,0,0", "--exchange=mini"], "minimizer")])
def test_cli_gpus_exchange_choice(tmp_path, args, how):
    """tsxCount --mode=HIP --gpus=N at k = 31: the minimizer exchange from 4 GPUs on (or on request), the table merge below;
    the number of different k-mers it reports is the oracle's."""
    from oracle.oracle import Oracle
    from tsxcount_amd import synth
    text = synth.fastq(95, 0, 600)
    o = Oracle(31, 21, 4, seed=1)
    o.count_fastq(text)
    kmers, _ = o.dump()
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(text)
    exe = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
    p = subprocess.run([exe, "--input=%s" % fq, "--mode=HIP", "--k=31", "--l=23"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, out + err
    assert "Added a total of %d different kmers" % len(kmers) in out, out + err
    assert ("exchange: minimizer owners" in err) == (how == "minimizer"), err


@pytest.mark.gpu
def test_cli_gpus_exchange_over_many_rounds(tmp_path):
    """tsxCount --gpus=4 --check on the reference's fixture at k = 31 with TSX_HIP_MZ_PIECE / TSX_HIP_MZ_SHARE in its
    environment: the minimizer exchange in many rounds, every k-mer of the check file at its owner, and the line that
    names the exchange's traffic names the rounds."""
    import re
    text = open(os.path.join(GOLDEN, "small_t7.1000.fastq"), "rb").read()
    fq = tmp_path / "small_t7.1000.fastq"
    fq.write_bytes(text)
    ref = python_counts(text, 31)
    (tmp_path / "small_t7.1000.fastq.31.count").write_bytes(b"".join(b"%s\t%d\n" % kv for kv in ref.items()))
    exe = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
    env = dict(os.environ, TSX_HIP_MZ_PIECE="8192", TSX_HIP_MZ_SHARE="2048")
    p = subprocess.run([exe, "--input=%s" % fq, "--mode=HIP", "--k=31", "--l=23", "--gpus=4", "--comm=copy", "--devices=0,0,0,0",
                        "--check", "--checkabort"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, out + err
    assert "exchange: minimizer owners" in err, err
    assert "Added a total of %d different kmers" % len(ref) in out and "total errors0" in out, out + err
    rounds = re.search(r"exchange rounds: (\d+)", err)
    assert rounds and int(rounds.group(1)) > 1, err
