"""The joint spectrum of two tables, the part that needs no GPU: the CPU statement of the definition
(tsxcount_amd.joint_histogram), the exported C ABI, the argument checks the library makes before it touches a device,
and what the CLI lists and refuses from the options alone."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kmerdb import pack_header as header

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")


def run_cli(*args, timeout=120):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def histogram(d, nbins):
    h = np.zeros(nbins, dtype=np.uint64)
    for c in d.values():
        h[min(c, nbins - 1)] += 1
    return h


#      only A      only B      both
A = {b"AA": 1, b"AC": 7,               b"AG": 2, b"AT": 9, b"CA": 3, b"CC": 4, b"CG": 1}
B = {              b"GG": 4, b"GT": 1, b"AG": 2, b"AT": 1, b"CA": 4, b"CC": 9, b"CG": 1, b"GA": 3}


def test_only_a_only_b_and_both():
    import tsxcount_amd as T
    m = T.joint_histogram(A, B, 16, 16)
    assert m.dtype == np.uint64 and m.shape == (16, 16)
    want = {(1, 0): 1, (7, 0): 1, (0, 4): 1, (0, 1): 1, (0, 3): 1, (2, 2): 1, (9, 1): 1, (3, 4): 1, (4, 9): 1, (1, 1): 1}
    got = {(int(i), int(j)): int(m[i, j]) for i, j in zip(*np.nonzero(m))}
    assert got == want
    assert m[0, 0] == 0 and m.sum() == len(set(A) | set(B))


def test_counts_at_below_and_above_the_last_bin():
    import tsxcount_amd as T
    # na = 5: the last bin of A is 4; counts 3 (below), 4 (at), 7 and 9 (above) -- nb = 3: the last bin of B is 2
    m = T.joint_histogram(A, B, 5, 3)
    assert m.shape == (5, 3)
    assert m[3, 2] == 1                 # CA: (3, 4) -> (3, 2)
    assert m[4, 2] == 1                 # CC: (4, 9) -> (4, 2)
    assert m[4, 1] == 1                 # AT: (9, 1) -> (4, 1)
    assert m[4, 0] == 1                 # AC: (7, 0) -> (4, 0)
    assert m[0, 2] == 2 and m[0, 1] == 1   # GG (4) and GA (3) pooled, GT (1)
    assert m[2, 2] == 1 and m[1, 1] == 1 and m[1, 0] == 1
    assert m[0, 0] == 0 and m.sum() == 10


def test_two_bins_each_is_presence():
    import tsxcount_amd as T
    m = T.joint_histogram(A, B, 2, 2)
    assert m.tolist() == [[0, 3], [2, 5]]


@pytest.mark.parametrize("na,nb", [(16, 16), (5, 3), (3, 200), (2, 2)])
def test_row_and_column_sums_are_the_histograms(na, nb):
    import tsxcount_amd as T
    m = T.joint_histogram(A, B, na, nb)
    assert np.array_equal(m.sum(axis=1)[1:], histogram(A, na)[1:])
    assert np.array_equal(m.sum(axis=0)[1:], histogram(B, nb)[1:])
    assert m[0].sum() == len(set(B) - set(A)) and m[:, 0].sum() == len(set(A) - set(B))


def test_a_count_of_zero_is_an_absent_kmer_and_empty_inputs():
    import tsxcount_amd as T
    m = T.joint_histogram({b"AA": 0, b"AC": 2}, {b"AA": 0, b"GG": 0}, 4, 4)
    assert m.sum() == 1 and m[2, 0] == 1 and m[0, 0] == 0
    assert not T.joint_histogram({}, {}, 2, 7).any()
    assert T.joint_histogram({}, B, 3, 3)[0].sum() == len(B)
    assert np.array_equal(np.diag(np.diag(T.joint_histogram(A, A, 12, 12))), T.joint_histogram(A, A, 12, 12))
    for bad in ((1, 5), (5, 1), (4097, 4096)):
        with pytest.raises(ValueError):
            T.joint_histogram(A, B, *bad)


def test_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in ("tsx_hip_joint_histogram_device", "tsx_hip_joint_histogram_host"):
        assert name + "(" in hdr and hasattr(L, name), name
    assert hasattr(T.TSXHashMapHIP, "jointHistogram") and T.JOINT_MAX_CELLS == 1 << 24


def test_null_maps_are_refused_before_any_device_call():
    import tsxcount_amd as T
    L = T.lib()
    out = np.zeros(4, dtype=np.uint64)
    assert L.tsx_hip_joint_histogram_host(None, None, T._p(out), 2, 2) == T.EINVAL
    assert b"joint histogram" in L.tsx_hip_last_error()
    assert L.tsx_hip_joint_histogram_device(None, None, 2, 2, None, None) == T.EINVAL
    assert not out.any()


def test_cli_usage_lists_the_joint_options():
    rc, _, err = run_cli("--help")
    assert rc != 0
    for o in ("--joint-histo=FILE", "--joint-max-a=H", "--joint-max-b=H", "--joint-format=sparse|matrix"):
        assert o in err, o


def test_cli_refusals_without_gpu(tmp_path):
    a, b = tmp_path / "a.db", tmp_path / "b.db"
    a.write_bytes(header(k=14, l=20, F=8, C=4))
    b.write_bytes(header(k=14, l=20, F=8, C=4))
    j = "--joint-histo=%s" % (tmp_path / "j.tsv")
    load, wth = "--load=%s" % a, "--with=%s" % b

    def refused(what, *args):
        rc, _, err = run_cli(*args)
        assert rc != 0 and what in err and "Creating" not in err, (args, err[-300:])
        assert not (tmp_path / "j.tsv").exists()

    refused("--joint-histo needs a second table", load, j)
    refused("one GPU only", load, wth, j, "--gpus=2")
    for side in ("a", "b"):
        refused("1 .. 4094", load, wth, j, "--joint-max-%s=0" % side)
        refused("1 .. 4094", load, wth, j, "--joint-max-%s=4095" % side)      # (H + 2)^2 > 2^24
        refused("1 .. 4094", load, wth, j, "--joint-max-%s=-3" % side)
        refused("1 .. 4094", load, wth, j, "--joint-max-%s=ten" % side)
    refused("--joint-format is sparse or matrix", load, wth, j, "--joint-format=dense")
    refused("go with --joint-histo", load, wth, "--compare", "--joint-max-a=10")
    refused("--with needs", load, wth)
