"""Read binning by two tables, the part that needs no GPU: the class rule on the CPU (tsxcount_amd.bin_class), the
exported C ABI and its structures, the argument checks the library makes before it touches a device, and what the CLI
lists and refuses from the options alone."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from kmerdb import pack_header as header

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
A, B, AMB, NONE = 0, 1, 2, 3


def run_cli(*args, timeout=120):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


# (hits_a, hits_b, min_hits, ratio_milli) -> class, worked out by hand from the rule:
#   q = hits >= min_hits; a side wins when q, more hits than the other, and hits * 1000 >= ratio_milli * the other's;
#   nobody qualifies: NONE; nobody wins: AMBIGUOUS.
CASES = [
    # ties win nothing; a tie of hits that qualify is ambiguous, a tie below min_hits is none
    (5, 5, 1, 1000, AMB), (0, 0, 1, 1000, NONE), (1, 1, 1, 1000, AMB), (3, 3, 4, 1000, NONE), (4, 4, 4, 1000, AMB),
    # the plain rule: more hits wins
    (2, 1, 1, 1000, A), (1, 2, 1, 1000, B), (1, 0, 1, 1000, A), (0, 1, 1, 1000, B),
    # min_hits met by one side only: the side that has more but does not qualify cannot win; the other has fewer
    (5, 3, 4, 1000, A), (3, 5, 4, 1000, B), (3, 2, 3, 1000, A), (2, 3, 3, 1000, B),
    (3, 5, 6, 1000, NONE), (5, 9, 6, 1000, B), (9, 5, 6, 1000, A),
    (10, 4, 11, 1000, NONE), (4, 10, 5, 1000, B),
    # ratio 1500: 3 : 2 is exactly 1.5 (wins), 29 : 20 is below (ambiguous)
    (3, 2, 1, 1500, A), (2, 3, 1, 1500, B), (29, 20, 1, 1500, AMB), (20, 29, 1, 1500, AMB), (30, 20, 1, 1500, A),
    (31, 20, 1, 1500, A), (14, 10, 1, 1500, AMB),
    # ratio 10^6: only a thousandfold lead, or an opponent without hits, wins
    (999, 1, 1, 1000000, AMB), (1000, 1, 1, 1000000, A), (1, 1000, 1, 1000000, B), (1999, 2, 1, 1000000, AMB),
    (2000, 2, 1, 1000000, A),
    # hits_b = 0: any ratio is met by a side that has hits at all
    (1, 0, 1, 1000000, A), (7, 0, 1, 1500, A), (7, 0, 8, 1500, NONE), (0, 7, 1, 1000000, B),
    # min_hits = 0: every record qualifies, so nothing is NONE
    (0, 0, 0, 1000, AMB), (0, 0, 0, 1000000, AMB), (1, 0, 0, 1000, A), (0, 1, 0, 1000, B), (2, 2, 0, 1500, AMB),
    # hits near 2^32 (a sequence line is shorter than 4 GiB): the products need more than 32 and fit 64 bits
    (2 ** 32 - 1, 2 ** 32 - 2, 1, 1000, A), (2 ** 32 - 2, 2 ** 32 - 1, 1, 1000, B), (2 ** 32 - 1, 2 ** 32 - 1, 1, 1000, AMB),
    (2 ** 32 - 1, 2 ** 32 - 2, 1, 1001, AMB), (2 ** 32 - 1, 4294968, 1, 1000000, AMB), (2 ** 32 - 1, 4294967, 1, 1000000, A),
    (2 ** 32 - 1, 2 ** 31, 2 ** 32 - 1, 1000, A), (2 ** 32 - 2, 2 ** 31, 2 ** 32 - 1, 1000, NONE),
]


@pytest.mark.parametrize("ha,hb,min_hits,ratio,want", CASES)
def test_bin_class_cases(ha, hb, min_hits, ratio, want):
    import tsxcount_amd as T
    assert (T.BIN_A, T.BIN_B, T.BIN_AMBIGUOUS, T.BIN_NONE) == (A, B, AMB, NONE)
    assert T.bin_class(ha, hb, min_hits, ratio) == want
    # the mirror image swaps A and B and nothing else
    mirror = {A: B, B: A, AMB: AMB, NONE: NONE}[want]
    assert T.bin_class(hb, ha, min_hits, ratio) == mirror


def test_bin_class_defaults_and_bounds():
    import tsxcount_amd as T
    assert T.bin_class(2, 1) == A and T.bin_class(1, 1) == AMB and T.bin_class(0, 0) == NONE
    for bad in (999, 0, 1000001):
        with pytest.raises(ValueError):
            T.bin_class(1, 0, 1, bad)


def test_symbols_structs_and_constants():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in ("tsx_hip_bin_stats_device", "tsx_hip_bin_stats_host", "tsx_hip_bin_reads_host"):
        assert name + "(" in hdr and hasattr(L, name), name
    for word in ("tsx_hip_bin_stats", "tsx_hip_bin_rule", "tsx_hip_bin_io", "tsx_hip_bin_totals", "TSX_HIP_BIN_A = 0",
                 "TSX_HIP_BIN_B = 1", "TSX_HIP_BIN_AMBIGUOUS = 2", "TSX_HIP_BIN_NONE = 3"):
        assert word in hdr, word
    assert ctypes.sizeof(T.BinRule) == 48 and T.BIN_STATS_DTYPE.itemsize == 32
    assert ctypes.sizeof(T.BinIO) == 16 and ctypes.sizeof(T.BinTotals) == 72
    assert T.BIN_STATS_DTYPE.names == ("kmers", "hits_a", "hits_b", "hits_both")
    for method in ("binStats", "binStatsDevice", "binReads"):
        assert hasattr(T.TSXHashMapHIP, method), method
    r = T.bin_rule((0, None), (2, 9), 3, 1.5)
    assert (r.a_lower, r.a_upper, r.b_lower, r.b_upper, r.min_hits, r.ratio_milli, r.reserved) == (0, 2 ** 64 - 1, 2, 9, 3, 1500, 0)


def bin_calls(L, T, rule, io):
    """The three entry points with NULL maps: [(name, rc, last error)]."""
    n = ctypes.c_size_t(7)
    tot = T.BinTotals()
    out = []
    rp = ctypes.byref(rule) if rule is not None else None
    out.append(("device", L.tsx_hip_bin_stats_device(None, None, None, 0, rp, None, 0, ctypes.byref(n), None),
                L.tsx_hip_last_error().decode()))
    assert n.value == 0
    out.append(("host", L.tsx_hip_bin_stats_host(None, None, b"", 0, rp, None, None, 0, None, 0), L.tsx_hip_last_error().decode()))
    out.append(("reads", L.tsx_hip_bin_reads_host(None, None, b"", 0, rp, ctypes.byref(io) if io is not None else None, 0,
                                                  ctypes.byref(tot)), L.tsx_hip_last_error().decode()))
    return out


def test_einval_before_any_device_call():
    """No map exists here (and on a CPU-only machine no device): every refusal below is made from the arguments alone."""
    import tsxcount_amd as T
    L = T.lib()
    top = 2 ** 64 - 1
    good_io = T.BinIO(1, -1, -1, -1)
    # NULL maps, everything else in order
    for name, rc, why in bin_calls(L, T, T.BinRule(1, top, 1, top, 1, 1000, 0), good_io):
        assert rc == T.EINVAL and "a and b are needed" in why, (name, why)
    # a NULL rule
    for name, rc, why in bin_calls(L, T, None, good_io):
        assert rc == T.EINVAL and "no rule" in why, (name, why)
    # the rule's own fields are looked at before the maps
    bad_rules = [
        (T.BinRule(5, 4, 1, top, 1, 1000, 0), "a_lower > a_upper"),
        (T.BinRule(1, 0, 1, top, 1, 1000, 0), "a_lower > a_upper"),     # (a lower bound of 0 is taken as 1)
        (T.BinRule(1, top, 9, 8, 1, 1000, 0), "b_lower > b_upper"),
        (T.BinRule(1, top, 0, 0, 1, 1000, 0), "b_lower > b_upper"),
        (T.BinRule(1, top, 1, top, 1, 999, 0), "ratio_milli"),
        (T.BinRule(1, top, 1, top, 1, 0, 0), "ratio_milli"),
        (T.BinRule(1, top, 1, top, 1, 1000001, 0), "ratio_milli"),
        (T.BinRule(1, top, 1, top, 1, 1000, 1), "reserved"),
        (T.BinRule(1, top, 1, top, 1, 1000, -1), "reserved"),
    ]
    for rule, word in bad_rules:
        for name, rc, why in bin_calls(L, T, rule, good_io):
            assert rc == T.EINVAL and word in why, (name, word, why)
    # io == NULL and an io without an output: bin_reads_host only
    rule = T.BinRule(1, top, 1, top, 1, 1000, 0)
    assert bin_calls(L, T, rule, None)[2][1:] == (T.EINVAL, "bin: no outputs (io is NULL)")
    name, rc, why = bin_calls(L, T, rule, T.BinIO(-1, -1, -1, -1))[2]
    assert rc == T.EINVAL and "every output of io is -1" in why
    # the totals of a refused call are zeroed
    tot = T.BinTotals(9, (9, 9, 9, 9), (9, 9, 9, 9))
    assert L.tsx_hip_bin_reads_host(None, None, b"", 0, ctypes.byref(rule), ctypes.byref(good_io), 0, ctypes.byref(tot)) == T.EINVAL
    assert tot.as_dict() == {"records": 0, "n": [0, 0, 0, 0], "bytes": [0, 0, 0, 0]}


BIN_OPTIONS = ("--bin-a=OUT", "--bin-b=OUT", "--bin-ambiguous=OUT", "--bin-none=OUT", "--bin-input=FILE", "--bin-stats=FILE",
               "--bin-min-hits=N", "--bin-ratio=R")


def test_cli_usage_lists_the_bin_options():
    rc, _, err = run_cli("--help")
    assert rc != 0
    for o in BIN_OPTIONS:
        assert o in err, o
    assert "bin<TAB>records<TAB>a<TAB>b<TAB>ambiguous<TAB>none" in err
    assert "index<TAB>kmers<TAB>hits_a<TAB>hits_b<TAB>hits_both<TAB>class" in err


def test_cli_refusals_without_gpu(tmp_path):
    a, b = tmp_path / "a.db", tmp_path / "b.db"
    a.write_bytes(header(k=14, l=20, F=8, C=4))
    b.write_bytes(header(k=14, l=20, F=8, C=4))
    q = tmp_path / "q.fastq"
    q.write_bytes(b"@r\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    outs = {n: tmp_path / ("out_%s.fq" % n) for n in ("a", "b", "ambiguous", "none", "stats")}
    load, wth, inp = "--load=%s" % a, "--with=%s" % b, "--bin-input=%s" % q
    oa, ob = "--bin-a=%s" % outs["a"], "--bin-b=%s" % outs["b"]

    def refused(what, *args):
        rc, _, err = run_cli(*args)
        assert rc != 0 and what in err and "Creating" not in err, (args, err[-400:])
        for p in outs.values():
            assert not p.exists(), p

    # every --bin-* option on its own needs --with
    for o in (oa, ob, "--bin-ambiguous=%s" % outs["ambiguous"], "--bin-none=%s" % outs["none"], "--bin-stats=%s" % outs["stats"],
              inp, "--bin-min-hits=2", "--bin-ratio=2"):
        refused("need a second table: --with=", load, o)
    # the rule options and the input without an output or --bin-stats
    refused("go with --bin-a, --bin-b, --bin-ambiguous, --bin-none or --bin-stats", load, wth, "--compare", "--bin-min-hits=2")
    refused("go with --bin-a, --bin-b, --bin-ambiguous, --bin-none or --bin-stats", load, wth, "--compare", "--bin-ratio=1.5")
    refused("go with --bin-a, --bin-b, --bin-ambiguous, --bin-none or --bin-stats", load, wth, "--compare", inp)
    # one GPU
    refused("one GPU only", load, wth, inp, oa, ob, "--gpus=2")
    # a wrapped FASTA as the binned file
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">g\nACGTACGTAC\nGTACGTACGT\n")
    refused("do not read wrapped FASTA", wth, "--input=%s" % fa, "--format=fasta-wrapped", "--k=14", oa, ob)
    refused("do not read wrapped FASTA", wth, "--input=%s" % fa, "--format=fasta-wrapped", "--k=14", oa, "--bin-input=%s" % fa)
    # pairs are out of scope
    refused("--bin-input takes one file", load, wth, oa, ob, "--bin-input=%s,%s" % (q, q))
    # the ratio: a decimal 1 .. 1000
    for bad in ("0.999", "0", "1000.001", "1001", "-2", "two", "1.5x", "", ".5", "1.", "1e2"):
        refused("--bin-ratio takes a decimal 1 .. 1000" if bad else "Usage", load, wth, inp, oa, ob, "--bin-ratio=%s" % bad)
    refused("--bin-min-hits takes a number", load, wth, inp, oa, ob, "--bin-min-hits=many")
    # nothing to bin
    refused("need --bin-input=FILE", load, wth, oa, ob)
    # --with alone still says what it needs, the bin outputs now among them
    rc, _, err = run_cli(load, wth)
    assert rc != 0 and "--with needs --op, --compare, --joint-histo or a --bin-a" in err and "Creating" not in err
