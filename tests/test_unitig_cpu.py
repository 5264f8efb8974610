"""Unitigs on the CPU: tsxcount_amd.unitig.unitig_model (the definition with strings and sets) against check_unitigs (an
independent property check) and both against the hand-written expectations of tests/unitig_cases.py; the checker must
reject every mutation of a right answer; format_unitigs; the rule's ValueErrors.  No library, no GPU."""
import pytest

from tsxcount_amd import unitig as U
from unitig_cases import CASES, K, kmers_of, rc, same_unitigs


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_gives_the_hand_written_unitigs(name, canonical):
    counts, lower, upper, plain, canon = CASES[name]
    want = canon if canonical else plain
    got, tot = U.unitig_model(counts, K, lower, upper, canonical)
    U.check_unitigs(got, counts, K, lower, upper, canonical)
    U.check_unitigs(want, counts, K, lower, upper, canonical)        # the expectation itself passes the checker
    same_unitigs(got, want, K, canonical)
    assert tot["unitigs"] == len(want) and tot["circular"] == sum(1 for u in want if u[3])
    assert tot["nodes"] == sum(u[1] for u in want) and tot["sum_count"] == sum(u[2] for u in want)
    assert tot["bases"] == sum(len(u[0]) for u in want) and tot["longest"] == max(len(u[0]) for u in want)
    assert sum(tot["degree"]) == tot["nodes"]
    assert tot["isolated"] == tot["degree"][0]


def test_the_reverse_complement_of_a_path_gives_the_same_canonical_output():
    a = U.unitig_model(CASES["path"][0], K, canonical=True)
    b = U.unitig_model(CASES["path_rc"][0], K, canonical=True)
    assert a == b
    assert U.unitig_model(CASES["path"][0], K)[0] != U.unitig_model(CASES["path_rc"][0], K)[0]


def test_totals_of_the_y():
    _, tot = U.unitig_model(CASES["y"][0], K)
    deg = tot["degree"]
    assert (tot["tips"], tot["branching"], tot["isolated"]) == (3, 1, 0)
    assert deg[0 * 5 + 1] == 1 and deg[1 * 5 + 0] == 2 and deg[1 * 5 + 2] == 1 and deg[1 * 5 + 1] == 10


def test_counts_of_both_strands_are_summed_on_a_canonical_table():
    d = {b"ACGTA": 2, rc(b"ACGTA"): 3}
    assert U.unitig_model(d, K, canonical=True)[0] == [(b"ACGTA", 1, 5, False)]
    assert U.unitig_model(d, K, lower=3, canonical=True)[0] == [(b"ACGTA", 1, 5, False)]
    assert U.unitig_model(d, K)[0] == [(b"TACGTA", 2, 5, False)]      # two nodes on a plain table, and they overlap


MUTATIONS = {
    "a dropped k-mer": lambda u: [(u[0][0][:-1], u[0][1] - 1, u[0][2] - 1, False)] + u[1:],
    "a unitig split in two": lambda u: [(u[0][0][:K + 1], 2, 2, False), (u[0][0][2:], u[0][1] - 2, u[0][2] - 2, False)] + u[1:],
    "a wrong sum": lambda u: [(u[0][0], u[0][1], u[0][2] + 1, False)] + u[1:],
    "a wrong number of k-mers": lambda u: [(u[0][0], u[0][1] + 1, u[0][2], False)] + u[1:],
    "a k-mer twice": lambda u: u + [(u[0][0][:K], 1, 1, False)],
    "a k-mer that is no node": lambda u: u + [(b"TTTTT", 1, 1, False)],
}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
@pytest.mark.parametrize("canonical", [False, True])
def test_checker_rejects_a_mutated_path(what, canonical):
    counts = CASES["path"][0]
    good = [(CASES["path"][3][0])]
    U.check_unitigs(good, counts, K, canonical=canonical)
    with pytest.raises(AssertionError):
        U.check_unitigs(MUTATIONS[what](list(good)), counts, K, canonical=canonical)


def test_checker_rejects_two_unitigs_joined_over_a_branch():
    counts, _, _, plain, canon = CASES["y"]
    joined = [(b"TCAATACGGTTCA", 9, 13, False), (b"TACGATGCC", 5, 5, False)]    # stem + one arm in one piece
    with pytest.raises(AssertionError, match="compactable|lies in"):
        U.check_unitigs(joined, counts, K)
    joined = [(b"TCAATACGGTTCA", 9, 13, False), (b"ACGATGCC", 4, 4, False)]     # every k-mer once, still wrong
    with pytest.raises(AssertionError, match="no compactable edge"):
        U.check_unitigs(joined, counts, K)


def test_checker_rejects_the_greater_strand_and_a_cycle_that_does_not_close():
    counts, _, _, _, canon = CASES["y"]
    flipped = [(rc(canon[0][0]),) + canon[0][1:]] + canon[1:]
    U.check_unitigs(canon, counts, K, canonical=True)
    with pytest.raises(AssertionError, match="greater strand"):
        U.check_unitigs(flipped, counts, K, canonical=True)
    counts = CASES["path"][0]
    with pytest.raises(AssertionError, match="does not close"):
        U.check_unitigs([(CASES["path"][3][0][0], 8, 8, True)], counts, K)
    cyc = CASES["cycle"]
    with pytest.raises(AssertionError, match="extends"):                      # a cycle reported as a path
        U.check_unitigs([(cyc[3][0][0], 9, 9, False)], cyc[0], K)


def test_checker_catches_a_model_that_stops_early():
    """Every k-mer its own unitig covers the nodes once and has the right sums: only the ends' rule catches it."""
    counts = CASES["path"][0]
    with pytest.raises(AssertionError, match="extends"):
        U.check_unitigs([(s, 1, c, False) for s, c in counts.items()], counts, K)


def test_any_cut_and_strand_of_a_cycle_passes():
    counts = CASES["cycle"][0]
    seq = CASES["cycle"][3][0][0]
    ring = seq[:9]
    for cut in range(9):
        r = ring[cut:] + ring[:cut]
        U.check_unitigs([(r + r[:K - 1], 9, 9, True)], counts, K)
        rr = rc(r)
        U.check_unitigs([(rr + rr[:K - 1], 9, 9, True)], counts, K, canonical=True)


def test_format_unitigs_bytes():
    text = U.format_unitigs([(b"ACGTACG", 3, 10, False), (b"AGGCGTGATAGGC", 9, 9, True), (b"AAAAA", 1, 1 << 40, False)])
    assert text == (b">0 LN:i:7 KC:i:10 km:f:3.3\nACGTACG\n"
                    b">1 LN:i:13 KC:i:9 km:f:1.0 CL:i:1\nAGGCGTGATAGGC\n"
                    b">2 LN:i:5 KC:i:1099511627776 km:f:1099511627776.0\nAAAAA\n")
    assert U.format_unitigs([]) == b""


def test_rule_value_errors():
    with pytest.raises(ValueError, match="lower 3 > upper 2"):
        U.unitig_rule(3, 2)
    with pytest.raises(ValueError, match="lower"):
        U.unitig_model({b"ACGTA": 1}, K, lower=3, upper=2)
    with pytest.raises(ValueError, match="even k"):
        U.unitig_model({b"ACGT": 1}, 4, canonical=True)
    with pytest.raises(ValueError, match="even k"):
        U.check_unitigs([], {b"ACGT": 1}, 4, canonical=True)
    with pytest.raises(ValueError, match="no 5-mer"):
        U.unitig_model({b"ACGT": 1}, K)
    r = U.unitig_rule()
    assert (r.lower, r.upper, r.flags, r.reserved) == (1, (1 << 64) - 1, 0, 0)
    assert U.unitig_model({b"ACGT": 1, b"CGTA": 1}, 4)[0] == [(b"ACGTA", 2, 2, False)]   # even k is fine on a plain table
    assert U.UNITIG_DTYPE.names == ("offset", "length", "kmers", "sum_count", "circular") and U.UNITIG_DTYPE.itemsize == 40


def test_empty_table():
    got, tot = U.unitig_model({}, K, canonical=True)
    assert got == [] and tot["nodes"] == 0 and tot["unitigs"] == 0 and tot["longest"] == 0
    U.check_unitigs([], {}, K)


def test_a_larger_random_graph_model_against_checker():
    import random
    rng = random.Random(11)
    genome = bytes(rng.choice(b"ACGT") for _ in range(400))
    genome = genome[:200] + genome[50:90] + genome[200:]            # a repeat longer than k
    counts = kmers_of([genome], 7)
    for canonical in (False, True):
        for lower in (1, 2):
            got, tot = U.unitig_model(counts, 7, lower, None, canonical)
            U.check_unitigs(got, counts, 7, lower, None, canonical)
            assert tot["unitigs"] == len(got) > 1
