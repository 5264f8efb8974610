"""Digital normalization without a GPU: the symbols, the refusals of the entry points and of the CLI, and self-checks of
the plain Python definition (tests/normalize_ref.py) that tests/test_normalize.py compares the library with."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from normalize_ref import normalize
from test_read_query import U64, coded_counts, run_cli

NEW_SYMBOLS = ("tsx_hip_normalize_host", "tsx_hip_normalize_device")
K = 5
READ = b"ACGTTGCAAGGCTA"                      # length k + 9, ten distinct k-mers
COPIES = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, READ, b"I" * len(READ)) for i in range(50))


def test_normalize_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    for name in ("tsx_hip_normalize_rule", "tsx_hip_normalize_totals", "#define TSX_HIP_NORMALIZE_ROUND 65536u"):
        assert name in hdr, name
    assert ctypes.sizeof(T.NormalizeRule) == 24 and ctypes.sizeof(T.NormalizeTotals) == 40
    assert T.NORMALIZE_ROUND == 65536
    for name in ("normalizeReads", "normalizeReadsDevice"):
        assert callable(getattr(T.TSXHashMapHIP, name)), name


def test_normalize_entry_points_refuse_bad_arguments_without_a_gpu():
    import tsxcount_amd as T
    with pytest.raises(ValueError):
        T.normalize_rule(round_records=0)
    with pytest.raises(ValueError):
        T.normalize_rule(cutoff=-1)
    r = T.normalize_rule()
    assert (r.cutoff, r.round_records, tuple(r.reserved)) == (20, 65536, (0, 0))
    m = T.TSXHashMapHIP.__new__(T.TSXHashMapHIP)   # no table behind it: the checks come first
    with pytest.raises(ValueError):
        m.normalizeReads(b"@a\nACGT\n", round_records=0)
    L = T.lib()
    text = b"@a\nACGT\n"
    for dev in (False, True):
        tot = T.NormalizeTotals(9, 9, 9, 9, 9)
        if dev:
            rc = L.tsx_hip_normalize_device(None, None, 0, ctypes.byref(r), None, 0, ctypes.byref(tot), None)
        else:
            rc = L.tsx_hip_normalize_host(None, text, len(text), ctypes.byref(r), -1, None, 0, 0, ctypes.byref(tot))
        assert rc == T.EINVAL and tot.as_dict() == dict.fromkeys(("records", "kept", "kmers_seen", "kmers_added", "rounds"), 0)


def test_cli_usage_errors_of_the_normalize_options(tmp_path):
    code, _, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--normalize=OUT", "--normalize-cutoff=20", "--normalize-round=65536"):
        assert flag in err, flag
    out = tmp_path / "n.out"
    base = ("--input=x.fastq", "--k=15", "--l=18", "--normalize=" + str(out))
    for args, word in ((("--check",), "--check"), (("--gpus=2",), "one GPU"), (("--min-count=2",), "--min-count=2"),
                       (("--l=auto",), "--l=auto"), (("--estimate",), "--estimate"),
                       (("--format=fasta-wrapped",), "wrapped"), (("--filter-interleaved", "--filter=f"), "paired"),
                       (("--filter-input=a.fq,b.fq", "--filter=f,g"), "paired"), (("--trim-interleaved", "--trim=f"), "paired")):
        code, _, err = run_cli(*base, *args, timeout=30)
        assert code == 1 and "Usage" in err and "--normalize" in err.split("Usage")[0] and word in err.split("Usage")[0], args
    code, _, err = run_cli("--load=x.db", "--normalize=" + str(out), timeout=30)
    assert code == 1 and "--input" in err.split("Usage")[0]
    code, _, err = run_cli("--input=x.fastq", "--k=15", "--l=18", "--normalize-cutoff=5", timeout=30)
    assert code == 1 and "--normalize=OUT" in err.split("Usage")[0]
    for bad in ("--normalize-round=0", "--normalize-round=x", "--normalize-cutoff=-3", "--normalize-cutoff="):
        code, _, err = run_cli(*base, bad, timeout=30)
        assert code == 1 and "Usage" in err, bad
    assert not out.exists()


@pytest.mark.parametrize("R,kept", [(1, 5), (4, 8), (64, 50)])
def test_reference_on_copies_of_one_read(R, kept):
    """50 copies of a read with distinct k-mers, C = 5: a copy is kept while every count is below 5 when its round starts.
    R = 1: five copies.  R = 4: rounds 0 and 1 start at counts 0 and 4 and keep four each.  R = 64: one round, all."""
    keep, out, tot, table = normalize(COPIES, K, 4, 5, R)
    assert sum(keep) == kept == tot["kept"] and keep == [True] * kept + [False] * (50 - kept)
    assert tot == {"records": 50, "kept": kept, "kmers_seen": 500, "kmers_added": 10 * kept, "rounds": (50 + R - 1) // R}
    assert len(table) == 10 and set(table.values()) == {kept}
    assert out == b"".join(b"@r%d\n%s\n+\n%s\n" % (i, READ, b"I" * len(READ)) for i in range(kept))


def test_reference_at_the_extreme_cutoffs():
    keep, out, tot, table = normalize(COPIES, K, 4, 0, 3)
    assert not any(keep) and out == b"" and not table and tot["kmers_added"] == 0 and tot["kmers_seen"] == 500
    before = Counter({b"ACGTT": 7})
    keep, _, _, table = normalize(COPIES, K, 4, 0, 3, counts=before)
    assert not any(keep) and table == before
    rnd = np.random.RandomState(4)
    text = b"".join(b">s%d\n%s\n" % (i, bytes(rnd.choice(list(b"ACGTN"), rnd.randint(1, 40)).tolist())) for i in range(60))
    for R in (1, 7, 1000):
        keep, out, tot, table = normalize(text, K, 2, U64, R)
        assert all(keep) and out == text and table == coded_counts(text, K, 2)
        assert tot["kmers_added"] == tot["kmers_seen"] == sum(table.values())
    _, _, _, table = normalize(text, K, 2, U64, 5, canonical=True)
    assert table == coded_counts(text, K, 2, canonical=True)
