"""Paired reads, what needs no GPU: the symbols and the error code, the argument checks of tsx_hip_filter_pairs_host /
tsx_hip_trim_pairs_host (made before any HIP call), the name rule on the CPU, and what the CLI refuses."""
import ctypes

import pytest

import tsxcount_amd as T
from test_read_query import U64, run_cli

TEXT = b"@a/1\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n"


def test_pair_symbols_declared_and_exported():
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in ("tsx_hip_filter_pairs_host", "tsx_hip_trim_pairs_host"):
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    for name in ("tsx_hip_pair_io", "tsx_hip_pair_totals", "TSX_HIP_PAIR_BOTH", "TSX_HIP_PAIR_ANY", "TSX_HIP_EPAIR = -11",
                 "check_names", "fd_single1", "fd_single2"):
        assert name in hdr, name
    assert ctypes.sizeof(T.PairIO) == 16 and ctypes.sizeof(T.PairTotals) == 80
    assert T.PAIR_MODES == {"both": 0, "any": 1}


def test_epair_has_a_text():
    L = T.lib()
    assert T.EPAIR == -11
    msg = L.tsx_hip_strerror(T.EPAIR).decode()
    assert msg != "unknown" and "pair" in msg
    assert L.tsx_hip_strerror(T.EPAIR - 1).decode() == "unknown"   # EPAIR took the next free value


def test_pair_argument_checks_need_no_gpu():
    L = T.lib()
    tot = T.PairTotals()
    tot.pairs = 7

    def filt(m, t2, n2, rule, mode, io):
        return L.tsx_hip_filter_pairs_host(m, TEXT, len(TEXT), t2, n2, ctypes.byref(rule) if rule else None, mode, 0,
                                           ctypes.byref(io) if io else None, 0, ctypes.byref(tot))

    def trim(m, t2, n2, rule, io):
        return L.tsx_hip_trim_pairs_host(m, TEXT, len(TEXT), t2, n2, ctypes.byref(rule) if rule else None, 0,
                                         ctypes.byref(io) if io else None, 0, ctypes.byref(tot))

    two, one = T.PairIO(1, 2, -1, -1), T.PairIO(1, -1, -1, -1)
    # no map: refused first, and the totals are cleared
    assert filt(None, TEXT, len(TEXT), T.filter_rule(), 0, two) == T.EINVAL and tot.pairs == 0
    assert trim(None, TEXT, len(TEXT), T.trim_rule(), two) == T.EINVAL
    assert filt(None, None, 0, T.filter_rule(), 0, one) == T.EINVAL
    assert trim(None, None, 0, T.trim_rule(), one) == T.EINVAL
    # every case below is refused without a GPU too; test_pairs.py repeats them with a real map behind the call, where
    # each one is the only thing wrong
    check_with_map(T, None, filt, trim, two, one)


def check_with_map(T, h, filt, trim, two, one):
    """Every EINVAL case of the pair calls, with map handle h."""
    ok_f, ok_t = T.filter_rule(), T.trim_rule()
    for rule in (T.FilterRule(3, 2, 0, 1000000, 0), T.FilterRule(1, U64, 0, 1000001, 0), None):
        assert filt(h, TEXT, len(TEXT), rule, 0, two) == T.EINVAL
    for rule in (T.TrimRule(3, 2, 0, 0, 0), T.TrimRule(1, U64, 0, 2, 0), T.TrimRule(1, U64, 0, 0, 1), None):
        assert trim(h, TEXT, len(TEXT), rule, two) == T.EINVAL
    for mode in (-1, 2):
        assert filt(h, TEXT, len(TEXT), ok_f, mode, two) == T.EINVAL
    for io in (None, T.PairIO(-1, 2, -1, -1), T.PairIO(1, -1, -1, -1)):           # two texts: fd1 and fd2 are required
        assert filt(h, TEXT, len(TEXT), ok_f, 0, io) == T.EINVAL
        assert trim(h, TEXT, len(TEXT), ok_t, io) == T.EINVAL
    for io in (None, T.PairIO(-1, -1, -1, -1), T.PairIO(1, 2, -1, -1), T.PairIO(1, -1, 3, 4)):   # interleaved: fd2, fd_single2 = -1
        assert filt(h, None, 0, ok_f, 0, io) == T.EINVAL
        assert trim(h, None, 0, ok_t, io) == T.EINVAL
    assert filt(h, None, 5, ok_f, 0, one) == T.EINVAL    # no text behind a length


def test_python_argument_checks_need_no_gpu():
    m = T.TSXHashMapHIP.__new__(T.TSXHashMapHIP)   # no table behind it: the checks come first
    with pytest.raises(ValueError):
        m.filterPairs(TEXT, TEXT, 1, 2, pairs="either")
    with pytest.raises(ValueError):
        m.trimPairs(TEXT, TEXT, 1, 2, mode="suffix")
    with pytest.raises(ValueError):
        m.trimPairs(TEXT, TEXT, 1, 2, lower=3, upper=2)
    with pytest.raises(ValueError):
        m.filterPairs(TEXT, None, 1, 2, lower=1)               # interleaved: one output
    with pytest.raises(ValueError):
        m.filterPairs(TEXT, None, 1, singles=(None, 3), lower=1)
    with pytest.raises(ValueError):
        m.trimPairs(TEXT, TEXT, 1, None, lower=1)              # two texts: two outputs


def test_pair_name():
    assert T.pair_name(b"@read7/1") == b"read7"
    assert T.pair_name(b"@read7/2") == b"read7"
    assert T.pair_name(b"@read7/1 1:N:0:ACGT") == b"read7"
    assert T.pair_name(b"@read7 2:N:0:ACGT/2") == b"read7"
    assert T.pair_name(b">read7/2\tlength=100") == b"read7"
    assert T.pair_name(b"@read7") == b"read7"
    assert T.pair_name("@read7/1\nACGT\n") == b"read7"        # only the first line counts
    assert T.pair_name(b"@read7/1/2") == b"read7/1"           # one suffix is removed
    assert T.pair_name(b"@read7/3") == b"read7/3"
    assert T.pair_name(b"@/1") == b"" and T.pair_name(b"@") == b"" and T.pair_name(b"@ x") == b""


def refused(*args):
    code, _, err = run_cli("--input=x.fastq", "--k=15", "--l=18", *args, timeout=30)
    assert code != 0, args
    return err


def test_cli_pair_options_and_refusals(tmp_path):
    code, _, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--filter-input=R1,R2", "--filter=O1,O2", "--filter-singles=S1,S2", "--filter-pairs=both|any", "--filter-interleaved",
                 "--trim-input=R1,R2", "--trim=O1,O2", "--trim-singles=S1,S2", "--trim-interleaved", "--pair-names",
                 "pairs<TAB>seen<TAB>kept<TAB>single1<TAB>single2"):
        assert flag in err, flag
    o = str(tmp_path / "o")
    # comma counts that do not match
    assert "two files each" in refused("--filter-input=a,b", "--filter=" + o)
    assert "two files each" in refused("--trim-input=a,b", "--trim=" + o)
    assert "two files each" in refused("--filter-input=a,b", "--filter=%s,%s2" % (o, o), "--filter-singles=s")
    assert "two files each" in refused("--trim-input=a,b,c", "--trim=%s,%s2" % (o, o))
    assert "one file each" in refused("--filter-interleaved", "--filter-input=a", "--filter=%s,%s2" % (o, o))
    assert "one file each" in refused("--trim-interleaved", "--trim-input=a", "--trim=" + o, "--trim-singles=s,t")
    assert "one file each" in refused("--trim-interleaved", "--trim-input=a,b", "--trim=" + o)
    # per-record outputs have no paired form
    assert "--read-stats" in refused("--filter-input=a,b", "--filter=%s,%s2" % (o, o), "--read-stats=" + o)
    assert "--trim-spans" in refused("--trim-input=a,b", "--trim=%s,%s2" % (o, o), "--trim-spans=" + o)
    # one GPU, no wrapped FASTA
    assert "one GPU" in refused("--gpus=2", "--filter-input=a,b", "--filter=%s,%s2" % (o, o))
    assert "one GPU" in refused("--gpus=2", "--trim-interleaved", "--trim-input=a", "--trim=" + o)
    code, _, err = run_cli("--input=x.fa", "--format=fasta-wrapped", "--trim-input=x.fa,b", "--trim=%s,%s2" % (o, o), timeout=30)
    assert code != 0 and "wrapped" in err
    code, _, err = run_cli("--input=x.fa", "--format=fasta-wrapped", "--filter-interleaved", "--filter-input=x.fa", "--filter=" + o,
                           timeout=30)
    assert code != 0 and "wrapped" in err
    assert "Usage" in refused("--filter-input=a,b", "--filter=%s,%s2" % (o, o), "--filter-pairs=neither")
    assert "paired input" in refused("--filter=" + o, "--filter-singles=s")
    assert not (tmp_path / "o").exists()
