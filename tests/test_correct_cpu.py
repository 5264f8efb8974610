"""Read correction without a GPU: the CPU model (tsxcount_amd.correct.correct_model) on hand-made cases of every clause
of the rule in include/tsxcount_hip.h, the signature-table entries, and the submodule's place in the package."""
import ctypes
import random
from collections import Counter

import pytest

import tsxcount_amd as T
from tsxcount_amd import _abi
from tsxcount_amd.correct import CORRECTION_DTYPE, correct_model, correct_rule

K = 9
_rnd = random.Random(4107)
GENOME = bytes(_rnd.choice(b"ACGT") for _ in range(400))


def counts_of(seq, k=K, times=2):
    c = Counter()
    for i in range(len(seq) - k + 1):
        c[seq[i:i + k]] += times
    return c


COUNTS = counts_of(GENOME)
assert max(COUNTS.values()) == 2   # every k-mer of the genome is unique: a substituted window is never solid by chance


def sub(read, at, to=None):
    r = bytearray(read)
    for p in at:
        r[p] = to if to is not None else b"CGTA"[b"ACGT".index(bytes([r[p] & 0xDF]))] | (r[p] & 0x20)
    return bytes(r)


def fastq(seqs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def model(seqs, counts=COUNTS, **kw):
    text = fastq(seqs)
    out, fixes, tot = correct_model(text, counts, K, **kw)
    assert len(out) == len(text) and tot["bytes"] == len(text) and tot["records"] == len(seqs)
    assert tot["sites"] == tot["corrected"] + tot["ambiguous"] + tot["unfixable"] and tot["corrected"] == len(fixes)
    diff = [i for i in range(len(text)) if text[i] != out[i]]
    assert len(diff) == len(fixes)
    return out, fixes, tot


READ = GENOME[100:160]   # L = 60, n = 52


@pytest.mark.parametrize("p", [0, 1, K - 2, K - 1, K, 30, 60 - K - 1, 60 - K, 58, 59])
def test_a_single_substitution_is_undone_head_interior_and_tail(p):
    bad = sub(READ, [p])
    out, fixes, tot = model([READ, bad])
    assert out == fastq([READ, READ])
    w = min(p + 1, K, 60 - p)   # the windows that hold base p
    assert fixes == [(1, p, bad[p], READ[p], w)]
    assert tot["sites"] == 1 and tot["corrected"] == 1


def test_two_substitutions_far_apart_and_close():
    far, close, edge = sub(READ, [20, 20 + K + 1]), sub(READ, [20, 20 + K - 1]), sub(READ, [20, 20 + K])
    out, fixes, tot = model([far, close, edge])
    # K + 1 apart: a solid window between the runs, two interior sites.  Closer, or exactly K apart: one run longer than k
    assert out == fastq([READ, close, edge])
    assert [f[:2] for f in fixes] == [(0, 20), (0, 20 + K + 1)] and tot["sites"] == 2


def test_what_is_no_site():
    noise = bytes(_rnd.choice(b"ACGT") for _ in range(60))
    hole = Counter(COUNTS)
    del hole[READ[30:30 + K]]          # an interior run of one window: shorter than k
    for seqs, counts in (([noise], COUNTS), ([READ], hole), ([READ[:K]], COUNTS), ([READ[:K - 2]], COUNTS)):
        out, fixes, tot = model(seqs, counts)
        assert out == fastq(seqs) and fixes == [] and tot["sites"] == 0
    # L == k + 1: two windows, so the head and the tail clause both apply
    short = sub(READ[:K + 1], [0])
    out, fixes, tot = model([short])
    assert out == fastq([READ[:K + 1]]) and fixes == [(0, 0, short[0], READ[0], 1)]
    # a head run longer than k (two errors K apart, the first at base 0)
    two = sub(READ, [0, K])
    assert model([two])[2]["sites"] == 0


def test_min_windows():
    bad = sub(READ, [59])   # a tail run of one window
    assert model([bad], min_windows=1)[2]["corrected"] == 1
    assert model([bad], min_windows=2)[2]["sites"] == 0
    mid = sub(READ, [30])
    assert model([mid], min_windows=K)[2]["corrected"] == 1


def test_unfixable_ambiguous_and_bytes_that_are_no_base():
    hole = Counter(COUNTS)
    del hole[READ[0:K]]                 # window 0 missing: a head site whose three alternatives are missing too
    out, fixes, tot = model([READ], hole)
    assert fixes == [] and (tot["sites"], tot["unfixable"]) == (1, 1)
    # two alternatives at base 59 are in the table: ambiguous, untouched
    bad = sub(READ, [59])
    both = Counter(COUNTS)
    third = sub(READ, [59], to=[b for b in b"ACGT" if b not in (READ[59], bad[59])][0])
    both[third[51:60]] = 2
    out, fixes, tot = model([bad], both)
    assert out == fastq([bad]) and (tot["sites"], tot["ambiguous"]) == (1, 1)
    # an N at the suspect position: its windows hold the k-mer base_code makes of it, the site is unfixable
    n_read = sub(READ, [30], to=ord("N"))
    for acgt_only in (False, True):
        out, fixes, tot = model([n_read], acgt_only=acgt_only)
        assert out == fastq([n_read]) and (tot["sites"], tot["unfixable"]) == (1, 1)
    # a second N in an interior site's reach: under acgt_only its dropped windows join the run, which is then longer than k
    two = sub(sub(READ, [30]), [33], to=ord("N"))
    assert model([two], acgt_only=True)[2]["sites"] == 0
    # a second N INSIDE a site (a head run holds it), where the read has an A, the code of an N: the default rule does not
    # see it and undoes the error; under acgt_only windows 0..2 are dropped whatever stands at base 5: unfixable
    at = next(i for i in range(K, 300) if GENOME[i + 2] == ord("A") and GENOME[i + 57] == ord("A"))
    read = GENOME[at:at + 60]
    head = sub(sub(read, [5]), [2], to=ord("N"))
    out, fixes, tot = model([head])
    assert fixes == [(0, 5, head[5], read[5], 6)] and out == fastq([sub(read, [2], to=ord("N"))])
    out, fixes, tot = model([head], acgt_only=True)
    assert out == fastq([head]) and (tot["sites"], tot["unfixable"]) == (1, 1)
    tail = sub(sub(read, [54]), [57], to=ord("N"))   # the mirror case: a tail run of six windows, the N in the last three
    assert model([tail], acgt_only=True)[2]["unfixable"] == 1 and model([tail])[2]["corrected"] == 1


def test_lower_case_is_kept_and_upper_bounds_a_repeat():
    low = READ[:20] + READ[20:40].lower() + READ[40:]
    bad = sub(low, [30])
    assert bad[30:31].islower()
    out, fixes, _ = model([bad])
    assert out == fastq([low]) and fixes == [(0, 30, bad[30], low[30], K)]
    high = Counter(COUNTS)
    high[READ[30:30 + K]] = 50
    assert model([READ], high, upper=40)[2]["sites"] == 0          # one window: shorter than k
    assert model([READ], high)[2]["sites"] == 0


def test_canonical_counts_fold_the_strands():
    rc = READ[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    bad = sub(rc, [25])
    assert model([bad])[2]["corrected"] == 0
    out, fixes, tot = model([bad], canonical=True)
    assert out == fastq([rc]) and tot["corrected"] == 1


def test_fasta_records_empty_lines_and_an_open_last_line():
    bad = sub(READ, [30])
    text = b"\n>a\n" + bad + b"\n\n\n>b\n" + sub(READ, [5])
    out, fixes, tot = correct_model(text, COUNTS, K, lines_per_record=2)
    assert out == b"\n>a\n" + READ + b"\n\n\n>b\n" + READ and tot["records"] == 2
    assert [f[:2] for f in fixes] == [(0, 30), (1, 5)]


def test_the_signature_table_and_the_structures():
    for name in ("tsx_hip_correct_sites_device", "tsx_hip_correct_sites_host", "tsx_hip_correct_reads_device",
                 "tsx_hip_correct_reads_host"):
        assert name in _abi.SIGNATURES, name
        assert name + "(" in open(T.HEADER_PATH).read(), name
    assert ctypes.sizeof(_abi.CorrectRule) == 24 and ctypes.sizeof(_abi.CorrectTotals) == 48 and CORRECTION_DTYPE.itemsize == 16
    with pytest.raises(ValueError):
        correct_rule(lower=3, upper=2)


def test_the_submodule_is_reached_by_name_and_not_re_exported():
    assert T.correct.correct_model is correct_model
    for name in ("correct_model", "correct_reads", "correction_sites", "correct_reads_device", "CORRECTION_DTYPE", "CorrectRule"):
        assert not hasattr(T, name), name
