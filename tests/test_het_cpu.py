"""Heterozygous k-mer pairs, the part that needs no GPU: the CPU statement of the definition (tsxcount_amd.het_pairs and
het_histogram) on hand cases."""
import numpy as np
import pytest

STAT_NAMES = ("kmers_in_range", "paired", "pairs", "families_2", "families_3plus")


def het(D, k=5, **kw):
    import tsxcount_amd as T
    pairs, st = T.het_pairs(D, k, **kw)
    assert tuple(st) == STAT_NAMES and st["pairs"] == len(pairs) and pairs == sorted(pairs)
    return pairs, st


def test_families_of_one_two_three_and_four():
    #    alone         two                     three                                four
    D = {"AAAAA": 3, "CCACC": 5, "CCGCC": 9, "GGAGG": 1, "GGCGG": 2, "GGTGG": 4, "TTATT": 1, "TTCTT": 2, "TTGTT": 3, "TTTTT": 4}
    pairs, st = het(D)
    assert pairs == [("CCACC", 5, "CCGCC", 9)]
    assert st == {"kmers_in_range": 10, "paired": 2, "pairs": 1, "families_2": 1, "families_3plus": 2}
    pairs, st = het(D, mode="all")
    assert len(pairs) == 1 + 3 + 6 and ("CCACC", 5, "CCGCC", 9) in pairs
    assert ("GGAGG", 1, "GGTGG", 4) in pairs and ("TTCTT", 2, "TTTTT", 4) in pairs and ("TTATT", 1, "TTCTT", 2) in pairs
    assert len(set(pairs)) == len(pairs) and all(a != b for a, _, b, _ in pairs)
    assert st == {"kmers_in_range": 10, "paired": 9, "pairs": 10, "families_2": 1, "families_3plus": 2}
    # a variant at another position is no partner
    assert het({"AAAAA": 1, "AAAAC": 1, "CAAAA": 2, "ACAAA": 2})[0] == []


def test_the_range_turns_a_family_of_three_into_a_pair():
    D = {"GGAGG": 1, "GGCGG": 20, "GGTGG": 40}
    assert het(D)[0] == [] and het(D)[1]["families_3plus"] == 1
    pairs, st = het(D, lower=2)
    assert pairs == [("GGCGG", 20, "GGTGG", 40)]
    assert st == {"kmers_in_range": 2, "paired": 2, "pairs": 1, "families_2": 1, "families_3plus": 0}
    pairs, st = het(D, upper=20)
    assert pairs == [("GGAGG", 1, "GGCGG", 20)] and st["kmers_in_range"] == 2
    assert het(D, lower=2, upper=20)[1] == {"kmers_in_range": 1, "paired": 0, "pairs": 0, "families_2": 0, "families_3plus": 0}
    assert het(D, lower=0)[1]["kmers_in_range"] == 3       # a count of 0 is an absent k-mer, whatever the range says
    assert het({"GGAGG": 0, "GGCGG": 2, "GGTGG": 3}, lower=0)[0] == [("GGCGG", 2, "GGTGG", 3)]


def test_minor_major_and_the_tie_rule():
    assert het({"CCGCC": 2, "CCACC": 7})[0] == [("CCGCC", 2, "CCACC", 7)]      # the lower count is the minor
    assert het({"CCGCC": 7, "CCACC": 2})[0] == [("CCACC", 2, "CCGCC", 7)]
    assert het({"CCTCC": 4, "CCGCC": 4})[0] == [("CCGCC", 4, "CCTCC", 4)]      # a tie: the smaller k-mer
    assert het({b"CCTCC": 4, b"CCGCC": 4})[0] == [("CCGCC", 4, "CCTCC", 4)]    # (bytes keys, as a dump's names)


def test_canonical_partner_on_the_other_strand():
    # AAAGG is the smaller strand of CCTTT; the variant CCGTT of CCTTT is reported as AACGG, the other strand
    D = {"AAAGG": 6, "CCGTT": 2}
    assert het(D)[0] == []                                                      # not canonical: unrelated k-mers
    pairs, st = het(D, canonical=True)
    assert pairs == [("AACGG", 2, "AAAGG", 6)]
    assert st == {"kmers_in_range": 2, "paired": 2, "pairs": 1, "families_2": 1, "families_3plus": 0}
    # a dict given by the other strands is the same table
    assert het({"CCTTT": 6, "AACGG": 2}, canonical=True)[0] == pairs
    assert het({"CCTTT": 6, "CCGTT": 2}, canonical=True)[0] == pairs
    assert het({"CCTTT": 6, "CCGTT": 2})[0] == [("CCGTT", 2, "CCTTT", 6)]


def test_palindromic_flanks_have_two_keys_and_one_pair():
    import tsxcount_amd as T
    # AC?GT: ACAGT / ACTGT are one strand pair, ACCGT / ACGGT the other
    assert T.revcomp("ACAGT") == "ACTGT" and T.revcomp("ACCGT") == "ACGGT"
    D = {"ACAGT": 3, "ACCGT": 8}
    for mode in ("unique", "all"):
        pairs, st = het(D, canonical=True, mode=mode)
        assert pairs == [("ACAGT", 3, "ACCGT", 8)]
        assert st == {"kmers_in_range": 2, "paired": 2, "pairs": 1, "families_2": 1, "families_3plus": 0}
    # not canonical: four different k-mers, a family of four
    D4 = {"ACAGT": 1, "ACCGT": 2, "ACGGT": 3, "ACTGT": 4}
    assert het(D4)[1]["families_3plus"] == 1 and het(D4, mode="all")[1]["pairs"] == 6


def test_histogram_clips_at_the_last_bin():
    import tsxcount_amd as T
    pairs = [("A", 1, "C", 2), ("A", 1, "G", 2), ("A", 3, "C", 4), ("A", 4, "C", 4), ("A", 5, "C", 900), ("A", 70, "C", 80)]
    m = T.het_histogram(pairs, 5, 6)
    assert m.dtype == np.uint64 and m.shape == (5, 6)
    want = np.zeros((5, 6), dtype=np.uint64)
    want[1, 2], want[3, 4], want[4, 4], want[4, 5] = 2, 1, 1, 2
    assert np.array_equal(m, want)
    assert T.het_histogram(pairs, 2, 2)[1, 1] == len(pairs) and T.het_histogram(pairs, 2, 2).sum() == len(pairs)
    assert T.het_histogram(pairs).shape == (1002, 1002) and T.het_histogram(pairs)[5, 900] == 1
    assert not T.het_histogram([], 3, 3).any()
    for bad in ((1, 5), (5, 1), (4097, 4096)):
        with pytest.raises(ValueError):
            T.het_histogram(pairs, *bad)


def test_even_k_and_bad_arguments_are_refused():
    import tsxcount_amd as T
    with pytest.raises(ValueError):
        T.het_pairs({"ACGT": 1}, 4)
    with pytest.raises(ValueError):
        T.het_pairs({}, 30, canonical=True)
    with pytest.raises(ValueError):
        T.het_pairs({"ACGTA": 1}, 5, mode="some")
    with pytest.raises(ValueError):
        T.het_pairs({"ACGTAAA": 1}, 5)
    assert T.het_pairs({}, 5) == ([], dict.fromkeys(STAT_NAMES, 0))
