"""The CPU statement of the coverage track (tsxcount_amd.track.track_bins) against a loop over start positions written
out here, its sums against sequence_stats, the text of format_track, and the new prototypes of the header against the
signature table.  No library, no GPU."""
import random

import pytest

import tsxcount_amd as T
from tsxcount_amd import track
from tsxcount_amd._abi import SIGNATURES
from conftest import python_counts

K = 9
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def small_text(seed=5):
    """A wrapped text with blank lines, an empty record, a sequence shorter than k, one of exactly k bases, runs of N and
    lower case, sequences of 64, 100 and 200 bases (whole bins at W = 64 and W = 100) and one of 333."""
    rng = random.Random(seed)
    long = rand_seq(rng, 333)
    with_n = rand_seq(rng, 70) + b"NNN" + rand_seq(rng, 40).lower() + b"N" + rand_seq(rng, 60)
    text = wrap(rand_seq(rng, 30), 7)                                   # lines in front of the first header
    text += b">long one\n" + wrap(long, 60) + b"\n\n"
    text += b">empty\n\n>short\n" + rand_seq(rng, K - 1) + b"\n>exact\n" + rand_seq(rng, K) + b"\n"
    text += b">\n" + wrap(with_n, 50) + b"\n"                           # an empty name
    for n in (64, 100, 200, 65):
        text += b">s%d\n" % n + wrap(rand_seq(rng, n), 13) + b"\n" * rng.choice([0, 2])
    table = b">t\n" + long[:150] + b"\n>t\n" + long[100:] + b"\n>t\n" + with_n + b"\n>t\n" + long[200:260][::-1].translate(COMP) + b"\n"
    return text, table


def brute(records, D, k, W, lower, upper, canonical, acgt_only):
    """The definition, position by position: the bin of a start position is position // W."""
    fold = bytes(b"ACGT"[((b >> 1) ^ (b >> 2)) & 3] for b in range(256))
    tab = {}
    for x, c in D.items():
        x = x.translate(fold)
        if canonical:
            x = min(x, x[::-1].translate(COMP))
        tab[x] = tab.get(x, 0) + c
    first, bins = [0], []
    for _, seq in records:
        rows = [[] for _ in range((len(seq) + W - 1) // W)]
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if acgt_only and any(b not in b"ACGTacgt" for b in w):
                continue
            x = w.translate(fold)
            if canonical:
                x = min(x, x[::-1].translate(COMP))
            rows[i // W].append(tab.get(x, 0))
        for c in rows:
            bins.append((len(c), sum(1 for v in c if lower <= v <= upper), min(c, default=0), max(c, default=0), sum(c)))
        first.append(len(bins))
    return first, bins


@pytest.mark.parametrize("W", [64, 100, 1 << 20])
@pytest.mark.parametrize("canonical,acgt_only", [(False, False), (True, False), (False, True)])
def test_track_bins_is_the_loop_over_start_positions(W, canonical, acgt_only):
    text, table = small_text()
    recs = T.fasta_records(text)
    assert [len(s) for _, s in recs[:4]] == [30, 333, K - 1, K] and recs[4][0] == b""       # the empty record vanished
    D = python_counts(T.join_fasta(table), K, 2)
    if acgt_only:
        D = {x: c for x, c in D.items() if all(b in b"ACGTacgt" for b in x)}
    for lower, upper in ((1, None), (2, 2)):
        first, bins = track.track_bins(recs, D, K, W, lower, upper, canonical, acgt_only)
        want = brute(recs, D, K, W, lower, (1 << 64) - 1 if upper is None else upper, canonical, acgt_only)
        assert (first, bins) == want
        assert [b - a for a, b in zip(first, first[1:])] == [(len(s) + W - 1) // W for _, s in recs]
        # the bins of a sequence sum to its stats row; the min over its bins with k-mers is the row's min
        stats = T.sequence_stats(recs, D, K, lower, upper, canonical, acgt_only)
        for i, (length, kmers, present, mn, total) in enumerate(stats):
            rows = bins[first[i]:first[i + 1]]
            assert sum(r[0] for r in rows) == kmers and sum(r[1] for r in rows) == present
            assert sum(r[4] for r in rows) % (1 << 64) == total
            assert min([r[2] for r in rows if r[0]], default=0) == mn
            assert all(r[2] <= r[3] for r in rows) and all(r[0] or r[2:] == (0, 0, 0) for r in rows)
    if W == 64:
        by = {n: i for i, (n, _) in enumerate(recs)}
        assert bins[first[by[b"s64"] + 1] - 1][0] == 64 - K + 1 and first[by[b"s64"] + 1] - first[by[b"s64"]] == 1
        assert bins[first[by[b"s65"] + 1] - 1][0] == 0                   # a tail bin without k-mers
        assert sum(r[1] for r in bins) > 0 and (canonical or acgt_only or max(r[3] for r in bins) >= 2)
    if W == 1 << 20:
        assert [(r[0], r[1], r[2], r[4]) for r in bins] == [s[1:] for s in T.sequence_stats(recs, D, K, 2, 2, canonical, acgt_only)]


def test_track_bins_refuses_a_window_out_of_range():
    for W in (63, (1 << 32) + 1, 0):
        with pytest.raises(ValueError):
            track.track_bins([(b"a", b"ACGT")], {}, 3, W)
    assert track.track_bins([(b"a", b"ACGT")], {b"ACG": 3}, 3, 1 << 32) == ([0, 1], [(2, 1, 0, 3, 3)])


def test_format_track():
    names = [b"one", b"", b"none"]
    first = [0, 2, 3, 3]
    bins = [(100, 90, 0, 7, 333), (3, 3, 2, 2, 6), (0, 0, 0, 0, 0)]
    got = track.format_track(names, first, bins, 100, [112, 8, 0])
    assert got == (b"one\t0\t100\t100\t90\t0\t7\t3.3300\n"
                   b"one\t100\t112\t3\t3\t2\t2\t2.0000\n"
                   b"*\t0\t8\t0\t0\t0\t0\tNA\n")
    assert track.format_track([b"x"], [0, 1], [(3, 0, 0, 1, 2)], 64, [70]).endswith(b"\t0.6667\n")
    assert track.format_track([], [0], [], 64, []) == b""


def test_the_package_surface_does_not_grow():
    assert T.track is track and track.SEQ_BIN_DTYPE.itemsize == 40
    for name in ("sequence_track", "track_bins", "format_track", "SEQ_BIN_DTYPE", "write_sequence_track"):
        assert hasattr(track, name) and not hasattr(T, name)
    assert not hasattr(T.TSXHashMapHIP, "sequenceTrack")


def test_header_and_signature_table_agree_on_the_track_calls():
    from test_abi_signatures_cpu import PROTOS, ctypes_kind
    names = ["tsx_hip_seq_track_host", "tsx_hip_seq_track_bgzf_host", "tsx_hip_seq_track_device", "tsx_hip_seq_result_bins",
             "tsx_hip_seq_result_window", "tsx_hip_seq_write_track"]
    for name in names:
        assert name in PROTOS and name in SIGNATURES, name
        want_ret, want_args = PROTOS[name]
        restype, argtypes = SIGNATURES[name]
        assert ctypes_kind(restype) == want_ret and [ctypes_kind(a) for a in argtypes] == want_args, name
    assert len(PROTOS["tsx_hip_seq_track_host"][1]) == 8 and PROTOS["tsx_hip_seq_result_window"][0] is T.ctypes.c_uint64
    text = open(T.HEADER_PATH).read()
    assert "uint64_t kmers, present, min_count, max_count, sum_count;" in text          # tsx_hip_seq_bin as SEQ_BIN_DTYPE
    assert [n for n, _ in track.SEQ_BIN_DTYPE.descr] == ["kmers", "present", "min_count", "max_count", "sum_count"]
