"""The small de Bruijn graphs of the unitig tests, k = 5, with hand-written expectations: shared by tests/test_unitig_cpu.py
(the model and the checker) and tests/test_unitig.py (the device).  Nothing here imports the library.

A case is (counts, lower, upper, expected plain, expected canonical); an expectation is a sorted list of (sequence, kmers,
sum_count, circular).  Circular ones are compared as sets of k-mers by the tests (cut and strand are free), so the
sequence given for them is one of the valid spellings."""
K = 5


def rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def kmers_of(seqs, k=K, circular=False, count=1):
    """{k-mer: occurrences * count} of the windows of the sequences (circular: read round the end)."""
    d = {}
    for s in seqs:
        s = s + s[:k - 1] if circular else s
        for i in range(len(s) - k + 1):
            d[s[i:i + k]] = d.get(s[i:i + k], 0) + count
    return d


def windows(seq, k):
    seq = bytes(seq)
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def node_set(seq, k, canonical):
    return frozenset(min(s, rc(s)) if canonical else s for s in windows(seq, k))


PATH = b"CCTGAGTCCGAG"
Y = (b"TCAATACGGTTCA", b"TCAATACGATGCC")
BUBBLE = (b"TCCACAGCATCATTGTA", b"TCCACAGCGTCATTGTA")
TIP = (b"AACTCTGGAAAACT", b"GAAAC")
CYCLE = b"GGCGTGATA"
BRANCH = b"GAACGGCG"     # runs into the cycle at GGCG


def _with(d, **more):
    d = dict(d)
    d.update({k.encode(): v for k, v in more.items()})
    return d


def _cycle_branch():
    d = kmers_of([CYCLE], circular=True)
    d.update(kmers_of([BRANCH]))
    return d


CASES = {
    "one_kmer": ({b"ACGTA": 7}, 1, None, [(b"ACGTA", 1, 7, False)], [(b"ACGTA", 1, 7, False)]),
    "path": (kmers_of([PATH]), 1, None, [(PATH, 8, 8, False)], [(PATH, 8, 8, False)]),
    # the same path given as its reverse complement: a plain table spells that strand, a canonical one the same as above
    "path_rc": (kmers_of([rc(PATH)]), 1, None, [(rc(PATH), 8, 8, False)], [(PATH, 8, 8, False)]),
    "y": (kmers_of(Y), 1, None,
          [(b"TACGATGCC", 5, 5, False), (b"TACGGTTCA", 5, 5, False), (b"TCAATACG", 4, 8, False)],
          [(b"CGTATTGA", 4, 8, False), (b"GGCATCGTA", 5, 5, False), (b"TACGGTTCA", 5, 5, False)]),
    "bubble": (kmers_of(BUBBLE), 1, None,
               [(b"CAGCATCAT", 5, 5, False), (b"CAGCGTCAT", 5, 5, False), (b"TCATTGTA", 4, 8, False), (b"TCCACAGC", 4, 8, False)],
               [(b"ATGACGCTG", 5, 5, False), (b"ATGATGCTG", 5, 5, False), (b"GCTGTGGA", 4, 8, False), (b"TACAATGA", 4, 8, False)]),
    "tip": (_with(kmers_of([TIP[0]]), GAAAC=1), 1, None,
            [(b"AAACTCTGGAAA", 8, 8, False), (b"GAAAAC", 2, 2, False), (b"GAAAC", 1, 1, False)],
            [(b"AAACTCTGGAAA", 8, 8, False), (b"GAAAAC", 2, 2, False), (b"GAAAC", 1, 1, False)]),
    # AAAAA -> AAAAA is no compactable edge: one unitig of one k-mer, not circular
    "self_loop": ({b"AAAAA": 3}, 1, None, [(b"AAAAA", 1, 3, False)], [(b"AAAAA", 1, 3, False)]),
    # AACGT -> ACGTT = rc(AACGT): on a canonical table the path ends at the hairpin
    "hairpin": (kmers_of([b"GGAACGT"]), 1, None, [(b"GGAACGT", 3, 3, False)], [(b"ACGTTCC", 3, 3, False)]),
    "cycle": (kmers_of([CYCLE], circular=True), 1, None, [(b"AGGCGTGATAGGC", 9, 9, True)], [(b"ACGCCTATCACGC", 9, 9, True)]),
    # a path that runs into the cycle: the cycle is cut at the branch and is no longer circular
    "cycle_branch": (_cycle_branch(), 1, None,
                     [(b"GAACGGCG", 4, 4, False), (b"GGCGTGATAGGCG", 9, 9, False)],
                     [(b"CGCCGTTC", 4, 4, False), (b"CGCCTATCACGCC", 9, 9, False)]),
    # the count range removes the mid-path k-mer AGTCC (count 5 > upper 4): two unitigs
    "range_mid": (_with(kmers_of([PATH]), AGTCC=5), 1, 4,
                  [(b"CCTGAGTC", 4, 4, False), (b"GTCCGAG", 3, 3, False)],
                  [(b"CCTGAGTC", 4, 4, False), (b"CTCGGAC", 3, 3, False)]),
    # the count range removes the branch k-mer TACGA (count 1 < lower 2): the stem and the other arm merge
    "range_branch": (_with(kmers_of(Y, count=2), TACGA=1), 2, None,
                     [(b"ACGATGCC", 4, 8, False), (b"TCAATACGGTTCA", 9, 26, False)],
                     [(b"ACGATGCC", 4, 8, False), (b"TCAATACGGTTCA", 9, 26, False)]),
}


def split(unitigs):
    """(sorted non-circular (sequence, kmers, sum_count), the circular ones as a sorted list of (sorted k-mer windows
    as found, kmers, sum_count)) -- the caller folds the windows to node sets."""
    lin = sorted((bytes(s), int(m), int(c)) for s, m, c, circ in unitigs if not circ)
    cyc = [(bytes(s), int(m), int(c)) for s, m, c, circ in unitigs if circ]
    return lin, cyc


def same_unitigs(got, want, k, canonical):
    """got and want hold the same unitigs: the non-circular ones as sorted lists, the circular ones as sets of nodes."""
    gl, gc = split(got)
    wl, wc = split(want)
    assert gl == wl, (gl[:3], wl[:3])
    fold = lambda cyc: sorted((sorted(node_set(s, k, canonical)), m, c) for s, m, c in cyc)   # noqa: E731
    for s, m, _ in gc:
        assert len(s) == m + k - 1
    assert fold(gc) == fold(wc)
