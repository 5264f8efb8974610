"""Read medians without a GPU: the symbols, the convention of median_count, the refusals of the entry points and of the
CLI -- and the Python restatement that tests/test_median.py compares the library with.

The restatement (expected_medians) is the window rule of test_trim.solid_flags over a Counter of the counted text, the
count of every window that is a k-mer written at its byte of the text, and sorted(values)[m // 2] per record.  Never
the library under test."""
import ctypes
import random

import numpy as np
import pytest

from test_read_query import _CODE, U64, line_spans, rc, records, run_cli
from test_trim import solid_flags

NO = 0xFFFFFFFF
SAT = 0xFFFFFFFE

NEW_SYMBOLS = ("tsx_hip_count_profile_device", "tsx_hip_count_profile_host", "tsx_hip_median_reads_device",
               "tsx_hip_median_reads_host", "tsx_hip_filter_median_host")


def expected_medians(query, counts, k, lpr, canonical=False, acgt_only=False, minq=0):
    """(profile as uint32[len(query)], [(kmers, median)] per record)."""
    sp = line_spans(query)
    prof = np.full(len(query), NO, dtype=np.uint32)
    meds = []
    for i in range(0, len(sp), lpr):
        grp = sp[i:i + lpr]
        seq = query[grp[1][0]:grp[1][1]] if len(grp) > 1 else b""
        qual = query[grp[3][0]:grp[3][1]] if len(grp) > 3 else b""
        is_kmer = solid_flags(seq, qual, counts, k, 0, U64, canonical, acgt_only, minq)
        s = seq.translate(_CODE)
        vals = []
        for j, ok in enumerate(is_kmer):
            if ok:
                x = s[j:j + k]
                v = min(counts.get(min(x, rc(x)) if canonical else x, 0), SAT)
                prof[grp[1][0] + j] = v
                vals.append(v)
        meds.append((len(vals), sorted(vals)[len(vals) // 2] if vals else 0))
    return prof, meds


def expected_median_filter(query, meds, lpr, lower=0, upper=U64, invert=False):
    recs = records(query, lpr)
    assert len(recs) == len(meds)
    keep = [(lower <= md <= upper) != invert for _, md in meds]
    return sum(keep), b"".join(r for (_, r), kp in zip(recs, keep) if kp)


def test_median_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    for name in ("tsx_hip_read_median", "tsx_hip_median_rule", "#define TSX_HIP_NO_KMER 0xFFFFFFFFu", "TSX_HIP_MEDIAN_LONG"):
        assert name in hdr, name
    assert ctypes.sizeof(T.MedianRule) == 24 and T.READ_MEDIAN_DTYPE.itemsize == 16
    assert T.READ_MEDIAN_DTYPE.names == ("kmers", "median") and T.NO_KMER == NO
    for name in ("countProfile", "medianReads", "filterReadsByMedian"):
        assert callable(getattr(T.TSXHashMapHIP, name)), name


def test_median_count_states_the_convention():
    import tsxcount_amd as T
    mc = T.median_count
    assert mc([]) == 0 and mc([7]) == 7
    assert mc([1, 9]) == 9 and mc([9, 1]) == 9              # m = 2: the upper middle
    assert mc([5, 1, 9]) == 5                                # m = 3
    assert mc([4, 1, 3, 2]) == 3 and mc([1, 2, 3, 4, 5]) == 3
    assert mc([6] * 10) == 6 and mc([6] * 11) == 6
    assert mc([SAT, SAT, 1]) == SAT and mc([SAT, 0]) == SAT and mc([SAT]) == SAT
    assert mc([NO, NO]) == 0 and mc([NO, 3, NO, 1]) == 3     # NO_KMER entries are no values
    assert mc(np.array([2, 0, NO, 1], dtype=np.uint32)) == 1
    rnd = random.Random(5)
    for _ in range(300):
        v = [rnd.choice((0, 1, 2, 300, 70000, SAT)) for _ in range(rnd.randint(0, 40))]
        assert mc(v) == (sorted(v)[len(v) // 2] if v else 0)


def test_the_restatement_on_a_text_worked_by_hand():
    k = 3
    counts = {b"ACG": 5, b"CGT": 1, b"GTA": 2 ** 33, b"AAA": 4}
    #        0         1         2
    #        0123456789012345678901234
    text = b"@a\nACGTA\n+\nIIIII\n\n@b\nAC\n+"
    prof, meds = expected_medians(text, counts, k, 4)
    assert meds == [(3, 5), (0, 0)]                          # sorted 1, 5, SAT -> the middle; a line shorter than k
    assert prof.tolist() == [NO] * 3 + [5, 1, SAT] + [NO] * (len(text) - 6)
    prof, meds = expected_medians(b">n\nACGNA\n", counts, k, 2, acgt_only=True)
    assert meds == [(1, 5)] and prof.tolist() == [NO] * 3 + [5] + [NO] * 5
    _, meds = expected_medians(b">n\nACGNA\n", counts, k, 2)   # N takes the code of A: ACG, CGA, GAA
    assert meds == [(3, 0)]
    assert expected_median_filter(b">x\nACGTA\n\n>y\nTT", [(3, 5), (0, 0)], 2, lower=1) == (1, b">x\nACGTA\n")
    assert expected_median_filter(b">x\nACGTA\n\n>y\nTT", [(3, 5), (0, 0)], 2, lower=1, invert=True) == (1, b">y\nTT\n")


def test_median_entry_points_refuse_bad_arguments_without_a_gpu():
    import tsxcount_amd as T
    with pytest.raises(ValueError):
        T.median_rule(lower=5, upper=4)
    assert tuple(getattr(T.median_rule(), f) for f in ("lower", "upper", "invert", "reserved")) == (0, U64, 0, 0)
    m = T.TSXHashMapHIP.__new__(T.TSXHashMapHIP)   # no table behind it: the checks come first
    with pytest.raises(ValueError):
        m.filterReadsByMedian(b"@a\nACGT\n", 1, lower=3, upper=2)
    L = T.lib()
    text = b"@a\nACGT\n"
    n = ctypes.c_size_t(7)
    out = np.zeros(4, dtype=T.READ_MEDIAN_DTYPE)
    prof = np.zeros(len(text), dtype=np.uint32)
    vp = ctypes.c_void_p
    assert L.tsx_hip_median_reads_host(None, text, len(text), out.ctypes.data_as(vp), 4, ctypes.byref(n), 0) == T.EINVAL
    assert n.value == 0
    n = ctypes.c_size_t(7)
    assert L.tsx_hip_median_reads_device(None, None, 0, None, 0, ctypes.byref(n), None) == T.EINVAL and n.value == 0
    assert L.tsx_hip_count_profile_host(None, text, len(text), prof.ctypes.data_as(vp), 0) == T.EINVAL
    assert L.tsx_hip_count_profile_device(None, None, 0, None, None) == T.EINVAL
    kept, nbytes = ctypes.c_uint64(9), ctypes.c_uint64(9)
    for rule in (T.median_rule(), T.MedianRule(3, 2, 0, 0), T.MedianRule(0, U64, 0, 1)):
        assert L.tsx_hip_filter_median_host(None, text, len(text), ctypes.byref(rule), 1, 0, ctypes.byref(kept),
                                            ctypes.byref(nbytes)) == T.EINVAL
        assert kept.value == 0 and nbytes.value == 0
    assert L.tsx_hip_filter_median_host(None, text, len(text), None, 1, 0, None, None) == T.EINVAL


def test_cli_usage_errors_of_the_median_options(tmp_path):
    code, _, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--read-medians=FILE", "--filter-median-lower=N", "--filter-median-upper=N"):
        assert flag in err, flag
    out, tsv = tmp_path / "f.out", tmp_path / "m.tsv"
    base = ("--input=x.fastq", "--k=15", "--l=18")
    # the median rule does not mix with the share rule's options
    for other in ("--filter-lower=3", "--filter-upper=9", "--filter-min=1", "--filter-fraction=0.5"):
        code, _, err = run_cli(*base, "--filter=" + str(out), "--filter-median-lower=2", other, timeout=30)
        assert code == 1 and "Usage" in err and "median rule" in err, other
    code, _, err = run_cli(*base, "--filter=" + str(out), "--filter-median-lower=5", "--filter-median-upper=4", timeout=30)
    assert code == 1 and "Usage" in err
    code, _, err = run_cli(*base, "--filter-median-upper=4", timeout=30)
    assert code == 1 and "--filter=OUT" in err
    # paired input, in both spellings
    for args in (("--filter-input=a.fastq,b.fastq", "--filter=o1,o2", "--filter-median-lower=2"),
                 ("--filter-input=a.fastq", "--filter-interleaved", "--filter=" + str(out), "--filter-median-upper=9"),
                 ("--filter-input=a.fastq", "--filter-interleaved", "--read-medians=" + str(tsv))):
        code, _, err = run_cli(*base, *args, timeout=30)
        assert code == 1 and "paired" in err and "median" in err, args
    # several GPUs
    for args in (("--read-medians=" + str(tsv),), ("--filter=" + str(out), "--filter-median-lower=2")):
        code, _, err = run_cli(*base, "--gpus=2", *args, timeout=30)
        assert code == 1 and "one GPU" in err and "median" in err, args
    # a wrapped FASTA as the queried file
    for args in (("--read-medians=" + str(tsv),), ("--filter=" + str(out), "--filter-median-lower=2"),
                 ("--read-medians=" + str(tsv), "--filter-input=x.fa")):
        code, _, err = run_cli("--input=x.fa", "--format=fasta-wrapped", "--k=15", "--l=18", *args, timeout=30)
        assert code == 1 and "wrapped" in err and "median" in err, args
    assert not out.exists() and not tsv.exists()
