"""Table set operations, the part that needs no GPU: the C ABI is declared and exported, the ctypes mirrors have the
structs' sizes, the CLI knows the options and refuses what the options and database headers already tell, and the
pure-Python statement of the operations (tests/combine_ref.py) says what the issue's table says."""
import ctypes
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT, python_counts
from combine_ref import MODES, OPS, combine_expect, jaccard
from kmerdb import pack_header as header

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")


def run_cli(*args, timeout=120):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_combine_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    assert "tsx_hip_combine(" in hdr and hasattr(L, "tsx_hip_combine")
    for name in ("tsx_hip_combine_rule", "tsx_hip_combine_stats", "TSX_HIP_OP_INTERSECT = 0", "TSX_HIP_OP_UNION = 1",
                 "TSX_HIP_OP_SUBTRACT = 2", "TSX_HIP_OP_DIFF = 3", "TSX_HIP_CNT_MIN = 0", "TSX_HIP_CNT_MAX = 1",
                 "TSX_HIP_CNT_SUM = 2", "TSX_HIP_CNT_LEFT = 3", "TSX_HIP_CNT_RIGHT = 4"):
        assert name in hdr, name
    assert T.COMBINE_OPS == {o: i for i, o in enumerate(OPS)}
    assert T.COMBINE_COUNTS == {m: i for i, m in enumerate(MODES)}


def test_struct_sizes_match_the_ctypes_mirrors(tmp_path):
    import tsxcount_amd as T
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsxcount_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(tsx_hip_combine_rule), sizeof(tsx_hip_combine_stats),\n'
                   ' offsetof(tsx_hip_combine_rule, a_lower), offsetof(tsx_hip_combine_rule, b_upper),\n'
                   ' offsetof(tsx_hip_combine_stats, out_count_sum)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.dirname(T.HEADER_PATH), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(T.CombineRule), ctypes.sizeof(T.CombineStats), T.CombineRule.a_lower.offset,
                   T.CombineRule.b_upper.offset, T.CombineStats.out_count_sum.offset]
    assert got[:2] == [40, 56]


def test_combine_rule_helper():
    import tsxcount_amd as T
    r = T.combine_rule("diff", "right", a_range=(2, 9), b_range=(0, None))
    assert (r.op, r.count_mode, r.a_lower, r.a_upper, r.b_lower, r.b_upper) == (3, 4, 2, 9, 0, (1 << 64) - 1)
    r = T.combine_rule()
    assert (r.op, r.count_mode, r.a_lower, r.a_upper) == (0, 0, 1, (1 << 64) - 1)


def test_cli_usage_lists_the_set_operation_options():
    rc, _, err = run_cli("--help")
    assert rc != 0
    for o in ("--with=DB", "--op=intersect|union|subtract|diff", "--op-count=min|max|sum|left|right", "--a-lower=N",
              "--a-upper=N", "--b-lower=N", "--b-upper=N", "--compare"):
        assert o in err, o


def test_cli_refusals_without_gpu(tmp_path):
    a, b = tmp_path / "a.db", tmp_path / "b.db"
    a.write_bytes(header(k=14, l=20, F=8, C=4))
    b.write_bytes(header(k=14, l=20, F=8, C=4))
    rc, _, err = run_cli("--load=%s" % a, "--op=subtract")
    assert rc != 0 and "--with" in err
    rc, _, err = run_cli("--load=%s" % a, "--compare")
    assert rc != 0 and "--with" in err
    rc, _, err = run_cli("--load=%s" % a, "--with=%s" % b, "--op=symdiff")
    assert rc != 0 and "--op is" in err
    rc, _, err = run_cli("--load=%s" % a, "--with=%s" % b, "--op=union", "--op-count=avg")
    assert rc != 0 and "--op-count is" in err
    rc, _, err = run_cli("--load=%s" % a, "--with=%s" % b, "--op=union", "--gpus=2")
    assert rc != 0 and "one GPU" in err
    rc, _, err = run_cli("--load=%s" % a, "--with=%s" % b, "--op=union", "--a-lower=5", "--a-upper=4")
    assert rc != 0
    rc, _, err = run_cli("--load=%s" % a, "--with=%s" % (tmp_path / "missing.db"), "--op=union")
    assert rc != 0 and "--with=" in err


@pytest.mark.parametrize("other", [dict(k=15, F=10), dict(canonical=1), dict(acgt=1), dict(minq=53)])
def test_cli_with_refuses_a_mismatched_database_without_gpu(tmp_path, other):
    a, b = tmp_path / "a.db", tmp_path / "b.db"
    a.write_bytes(header(k=14, l=20, F=8, C=4))
    kw = dict(k=14, l=20, F=8, C=4)
    kw.update(other)
    b.write_bytes(header(**kw))
    rc, _, err = run_cli("--load=%s" % a, "--with=%s" % b, "--op=intersect")
    assert rc != 0 and "--with=%s was counted with" % b in err and "Creating" not in err


# ---- the Python statement itself ----------------------------------------------------------------------------------------

A = {b"AA": 1, b"AC": 5, b"AG": 2, b"AT": 9}
B = {b"AC": 3, b"AG": 2, b"CC": 4, b"AT": 1}


def test_statement_full_ranges():
    assert combine_expect(A, B, "intersect", "min")[0] == {b"AC": 3, b"AG": 2, b"AT": 1}
    assert combine_expect(A, B, "intersect", "max")[0] == {b"AC": 5, b"AG": 2, b"AT": 9}
    assert combine_expect(A, B, "intersect", "sum")[0] == {b"AC": 8, b"AG": 4, b"AT": 10}
    assert combine_expect(A, B, "intersect", "left")[0] == {b"AC": 5, b"AG": 2, b"AT": 9}
    assert combine_expect(A, B, "intersect", "right")[0] == {b"AC": 3, b"AG": 2, b"AT": 1}
    assert combine_expect(A, B, "union", "min")[0] == {b"AA": 1, b"AC": 3, b"AG": 2, b"AT": 1, b"CC": 4}
    assert combine_expect(A, B, "union", "right")[0] == {b"AA": 1, b"AC": 3, b"AG": 2, b"AT": 1, b"CC": 4}
    assert combine_expect(A, B, "subtract")[0] == {b"AA": 1}
    assert combine_expect(A, B, "diff")[0] == {b"AA": 1, b"AC": 2, b"AT": 8}
    out, st = combine_expect(A, B, "union", "sum")
    assert st == dict(a_in_range=4, b_in_range=4, both=3, a_sum_both=16, b_sum_both=6, out_entries=5, out_count_sum=27)
    assert jaccard(st) == 3 / 5


def test_statement_ranges_cut_before_the_op():
    # a' drops AA (1) and AT (9); b' drops CC (4)
    kw = dict(a_range=(2, 5), b_range=(0, 3))
    assert combine_expect(A, B, "intersect", "sum", **kw)[0] == {b"AC": 8, b"AG": 4}
    assert combine_expect(A, B, "union", "left", **kw)[0] == {b"AC": 5, b"AG": 2, b"AT": 1}
    assert combine_expect(A, B, "subtract", **kw)[0] == {}
    assert combine_expect(A, B, "diff", **kw)[0] == {b"AC": 2}
    # a k-mer of A whose count is out of range is absent: B's count survives a subtract the other way round
    assert combine_expect(B, A, "subtract", a_range=(1, None), b_range=(2, 5))[0] == {b"CC": 4, b"AT": 1}
    _, st = combine_expect(A, B, "intersect", "min", **kw)
    assert (st["a_in_range"], st["b_in_range"], st["both"], st["a_sum_both"], st["b_sum_both"]) == (2, 3, 2, 7, 5)


def test_statement_on_the_golden_reads():
    text = open(os.path.join(GOLDEN, "small_t7.1000.fastq"), "rb").read()
    recs = text.split(b"\n")
    half = (len(recs) // 8) * 4
    lo, hi = b"\n".join(recs[:half + 200]) + b"\n", b"\n".join(recs[half - 200:])
    a, b, whole = python_counts(lo, 14), python_counts(hi, 14), python_counts(text, 14)
    inter, st = combine_expect(a, b, "intersect", "min")
    assert 0 < len(inter) < min(len(a), len(b))
    # |A and B| + |A minus B| = |A|;  sum of min + sum of max = both tables' sums over the shared k-mers
    assert len(inter) + len(combine_expect(a, b, "subtract")[0]) == len(a)
    mx = combine_expect(a, b, "intersect", "max")[0]
    assert sum(inter.values()) + sum(mx.values()) == st["a_sum_both"] + st["b_sum_both"]
    assert set(combine_expect(a, b, "union", "sum")[0]) == set(whole)
