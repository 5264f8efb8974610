"""Unitigs on the GPU: tsx_hip_unitig_stats, tsx_hip_unitigs_host / _device and tsx_hip_write_unitigs_host through
tsxcount_amd.unitig, against unitig_model and check_unitigs over the table's own dump (getAllKmers -> dict).

Non-circular unitigs are compared as sorted lists with the model's (sequence, kmers, sum_count), circular ones as sets of
(canonical) k-mers -- their cut and strand are the library's choice -- and everything goes through check_unitigs."""
import ctypes
import os

import numpy as np
import pytest

from test_het import from_dict, random_names, table_dict
from unitig_cases import CASES, K, kmers_of, same_unitigs

pytestmark = pytest.mark.gpu


def device_unitigs(m, lower=1, upper=None):
    """unitigs() of m as the model's tuples, and the totals."""
    from tsxcount_amd import unitig as U
    seq, rec, tot = U.unitigs(m, lower, upper)
    assert rec.dtype == U.UNITIG_DTYPE and len(rec) == tot["unitigs"] and len(seq) == tot["bases"]
    # the records tile the sequence buffer
    spans = sorted((int(r["offset"]), int(r["length"])) for r in rec)
    assert [a for a, _ in spans] == [0] + list(np.cumsum([n for _, n in spans])[:-1]) if spans else not seq
    strings = U.unitig_strings(seq, rec)
    return [(s, int(r["kmers"]), int(r["sum_count"]), bool(r["circular"])) for s, r in zip(strings, rec)], tot


def check(m, lower=1, upper=None, model=True):
    """The device's unitigs of m against check_unitigs and (model) unitig_model over the table's dump; returns them."""
    from tsxcount_amd import unitig as U
    d = table_dict(m)
    d = {bytes(s): c for s, c in d.items()}
    got, tot = device_unitigs(m, lower, upper)
    U.check_unitigs(got, d, m.k, lower, upper, m.canonical)
    if model:
        want, wtot = U.unitig_model(d, m.k, lower, upper, m.canonical)
        same_unitigs(got, want, m.k, m.canonical)
        assert tot == wtot
    assert U.unitig_stats(m, lower, upper) == tot
    return got, tot, d


def random_genome(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))


# ---- 1. the hand-written cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_written_cases(name, canonical):
    counts, lower, upper, plain, canon = CASES[name]
    m = from_dict(counts, K, l=8, canonical=canonical, hash_seed=3)
    got, tot, _ = check(m, lower, upper)
    same_unitigs(got, canon if canonical else plain, K, canonical)
    m.close()


# ---- 2. random graphs with repeats and errors -----------------------------------------------------------------------------

def reads_graph(rng, k, length=3000):
    g = random_genome(rng, length)
    g = g[:1000] + g[200:200 + 2 * k] + g[1000:2000] + g[400:400 + k + 7] + g[2000:]      # two repeats longer than k
    reads = [g[a:a + 150] for a in range(0, len(g) - 150, 40)]
    for j in (3, 11, 19, 30):                                                            # reads with substitutions
        r = bytearray(reads[j])
        for p in (20, 75, 149 - j):
            r[p] = b"ACGT"[(b"ACGT".index(r[p]) + 1 + j % 3) % 4]
        reads[j] = bytes(r)
    return kmers_of(reads, k)


@pytest.mark.parametrize("lower", [1, 2])
@pytest.mark.parametrize("k,canonical", [(21, True), (20, False)])
def test_random_graph(k, canonical, lower):
    counts = reads_graph(np.random.default_rng(100 + k), k)
    m = from_dict(counts, k, l=14, canonical=canonical, hash_seed=k)
    got, tot, _ = check(m, lower)
    assert tot["unitigs"] > 4 and tot["branching"] > 0 and tot["nodes"] > 2500
    if lower == 1:
        assert tot["tips"] > 0
    m.close()


# ---- 3. every key width ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 31, 33, 63, 65, 127])
def test_every_key_width(k):
    rng = np.random.default_rng(200 + k)
    g = random_genome(rng, 1500 if k > 5 else 300)      # (k = 5 has 512 canonical k-mers and at most 2^9 slots)
    if k > 5:
        g = g[:700] + g[100:100 + k + 20] + g[700:]
    m = from_dict(kmers_of([g], k), k, l=12 if k > 5 else 9, canonical=True, hash_seed=k)
    got, tot, _ = check(m)
    assert tot["nodes"] > (1300 if k > 5 else 150) and tot["unitigs"] >= 3
    m.close()


# ---- 4. long chains, wave seams, a long cycle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("canonical", [False, True])
def test_long_chain_isolated_kmers_and_a_cycle(canonical):
    k = 31
    rng = np.random.default_rng(31)
    counts = kmers_of([random_genome(rng, 6000)], k)
    assert len(counts) == 5970
    for s in random_names(rng, 500, k):
        counts[s] = counts.get(s, 0) + 3
    counts.update(kmers_of([random_genome(rng, 700)], k, circular=True, count=2))
    m = from_dict(counts, k, l=15, canonical=canonical, hash_seed=9)
    got, tot, _ = check(m)
    assert tot["longest"] == 6000 and tot["circular"] == 1 and tot["isolated"] == 500 and tot["unitigs"] == 502
    assert sorted(u[1] for u in got)[-2:] == [700, 5970]
    m.close()


# ---- 5. carried counts ----------------------------------------------------------------------------------------------------------

def test_carried_counts_sum_exactly():
    k = 31
    g = random_genome(np.random.default_rng(5), 200)
    counts = kmers_of([g], k)
    counts[g[50:50 + k]] = 1 << 20
    counts[g[120:120 + k]] = (1 << 33) + 5
    m = from_dict(counts, k, l=12, s=3, canonical=True, hash_seed=2)
    assert m.stats()["overflow_carries"] > 0
    got, tot, d = check(m)
    assert len(got) == 1 and got[0][2] == sum(d.values()) == 168 + (1 << 20) + (1 << 33) + 5
    got, tot, _ = check(m, lower=1, upper=1 << 20)          # the greater one leaves the range: two unitigs
    assert len(got) == 2 and sum(u[2] for u in got) == 168 + (1 << 20)
    m.close()


# ---- 6. caps and entry points -------------------------------------------------------------------------------------------------

def test_caps_streams_and_files(tmp_path):
    import torch
    import tsxcount_amd as T
    from tsxcount_amd import unitig as U
    k = 21
    m = from_dict(reads_graph(np.random.default_rng(6), k), k, l=14, canonical=True, hash_seed=6)
    want, tot, d = check(m)
    n, nbytes = tot["unitigs"], tot["bases"]
    assert n > 4
    fill = 0x5A
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for rec_cap, seq_cap, st in ((n - 1, nbytes, None), (n, nbytes - 1, None), (n, nbytes, None), (n, nbytes, stream.cuda_stream)):
        seq = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device="cuda:0")
        rec = torch.full(((n + 2) * 5,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        if rec_cap < n or seq_cap < nbytes:
            with pytest.raises(T.TSXException) as e:
                U.unitigs_device(m, seq.data_ptr(), seq_cap, rec.data_ptr(), rec_cap, stream=st)
            assert e.value.code == T.ERANGE and e.value.needed == (n, nbytes)
            assert (seq.cpu().numpy() == fill).all()                                   # nothing is spelled
            assert (rec.cpu().numpy()[rec_cap * 5:] == -1).all()                       # nothing behind the cap
            continue
        assert U.unitigs_device(m, seq.data_ptr(), seq_cap, rec.data_ptr(), rec_cap, stream=st) == (n, nbytes, tot)
        host_seq, host_rec = seq.cpu().numpy(), rec.cpu().numpy()
        assert (host_seq[nbytes:] == fill).all() and (host_rec[n * 5:] == -1).all()
        r = host_rec[:n * 5].view(U.UNITIG_DTYPE)
        got = [(s, int(x["kmers"]), int(x["sum_count"]), bool(x["circular"])) for s, x in zip(U.unitig_strings(host_seq[:nbytes].tobytes(), r), r)]
        assert sorted(got) == sorted(want)
    # the file, to a path and to a descriptor: its records, without their index, are format_unitigs of the model's
    model, _ = U.unitig_model(d, k, canonical=True)
    assert not any(u[3] for u in model)

    def records(text):
        lines = text.split(b"\n")
        assert lines[-1] == b"" and len(lines) % 2 == 1
        heads = lines[0:-1:2]
        assert [h.split(b" ")[0] for h in heads] == [b">%d" % i for i in range(len(heads))]
        return sorted(h.split(b" ", 1)[1] + b"\n" + s for h, s in zip(heads, lines[1::2]))
    path = str(tmp_path / "u.fa")
    assert U.write_unitigs(m, path) == tot
    fd = os.open(str(tmp_path / "v.fa"), os.O_WRONLY | os.O_CREAT, 0o644)
    assert U.write_unitigs(m, fd) == tot
    os.close(fd)
    text = open(path, "rb").read()
    assert records(text) == records(open(str(tmp_path / "v.fa"), "rb").read()) == records(U.format_unitigs(model))
    assert U.unitig_stats(m, 2) == U.unitig_model(d, k, 2, canonical=True)[1]
    m.close()


def test_cycles_in_the_file_carry_the_mark(tmp_path):
    from tsxcount_amd import unitig as U
    counts = dict(CASES["cycle"][0])
    counts.update(CASES["one_kmer"][0])
    m = from_dict(counts, K, l=8, hash_seed=4)
    path = str(tmp_path / "c.fa")
    U.write_unitigs(m, path)
    got, _ = device_unitigs(m)
    lines = open(path, "rb").read().split(b"\n")
    heads = lines[0:-1:2]
    assert sorted(h.split(b" ")[0] for h in heads) == [b">0", b">1"]
    assert sorted(h.split(b" ", 1)[1] for h in heads) == [b"LN:i:13 KC:i:9 km:f:1.0 CL:i:1", b"LN:i:5 KC:i:7 km:f:7.0"]
    assert sorted(lines[1::2]) == sorted(u[0] for u in got)
    assert open(path, "rb").read() == U.format_unitigs([u for h in heads for u in got if len(u[0]) == int(h.split(b":")[2].split()[0])])
    m.close()


# ---- 7. refusals, the empty table -------------------------------------------------------------------------------------------------

def test_refusals_and_the_empty_table():
    import tsxcount_amd as T
    from tsxcount_amd import unitig as U
    L = T.lib()
    m = from_dict({b"ACGTACGTACGTACG": 1}, 15, l=10)
    tot = T._abi.UnitigTotals()
    n, nb = ctypes.c_size_t(7), ctypes.c_size_t(7)
    good = U.unitig_rule()

    def refused(rc, what):
        assert rc == T.EINVAL
        msg = L.tsx_hip_last_error().decode()
        assert msg and what in msg, msg

    stats = lambda h, rule: L.tsx_hip_unitig_stats(h, ctypes.byref(rule) if rule else None, ctypes.byref(tot))   # noqa: E731
    refused(stats(None, good), "map")
    refused(stats(m.handle, None), "rule")
    refused(L.tsx_hip_unitig_stats(m.handle, ctypes.byref(good), None), "no totals")
    refused(stats(m.handle, T._abi.UnitigRule(5, 4, 0, 0)), "lower > upper")
    refused(stats(m.handle, T._abi.UnitigRule(1, 4, 1, 0)), "flags")
    refused(stats(m.handle, T._abi.UnitigRule(1, 4, 0, 1)), "reserved")
    refused(L.tsx_hip_unitigs_host(m.handle, ctypes.byref(good), None, 4, None, 0, ctypes.byref(n), ctypes.byref(nb), None), "no output")
    refused(L.tsx_hip_unitigs_device(m.handle, ctypes.byref(good), None, 0, None, 4, ctypes.byref(n), ctypes.byref(nb), None, None), "no output")
    refused(L.tsx_hip_unitigs_device(m.handle, ctypes.byref(good), None, 0, None, 0, None, ctypes.byref(nb), None, None), "no output")
    refused(L.tsx_hip_write_unitigs_host(m.handle, ctypes.byref(good), -1, None), "no output")
    even = from_dict({b"ACGTACGTACGTAC": 1}, 14, l=10, canonical=True)
    shard = T.TSXHashMapHIP(14, 0, 15, shard_bits=1, shard_index=0)
    for x, what in ((even, "even k"), (shard, "shard_bits")):
        refused(stats(x.handle, good), what)
        refused(L.tsx_hip_write_unitigs_host(x.handle, ctypes.byref(good), 1, None), what)
        with pytest.raises(T.TSXException) as e:
            U.unitigs(x)
        assert e.value.code == T.EINVAL and what in str(e.value)
    with pytest.raises(ValueError, match="lower 3 > upper 2"):      # before any GPU call: the map is not even looked at
        U.unitig_stats(None, 3, 2)
    with pytest.raises(ValueError):
        U.unitigs(None, 3, 2)
    # zero caps on a table with a unitig: the sizes come back with ERANGE
    rc = L.tsx_hip_unitigs_device(m.handle, ctypes.byref(good), None, 0, None, 0, ctypes.byref(n), ctypes.byref(nb), None, None)
    assert rc == T.ERANGE and (n.value, nb.value) == (1, 15)
    # an even k is fine on a plain table, an empty table gives nothing, also while it is lazily cleared
    plain_even = from_dict({b"ACGTACGTACGTAC": 2}, 14, l=10)
    assert device_unitigs(plain_even)[0] == [(b"ACGTACGTACGTAC", 1, 2, False)]
    for x in (from_dict({}, 15, l=10, canonical=True), m):
        x.clear()
        got, t = device_unitigs(x)
        assert got == [] and not any(v for f, v in t.items() if f != "degree") and not any(t["degree"])
        assert U.unitig_stats(x) == t
    for x in (m, even, shard, plain_even):
        x.close()


# ---- 8. long probe chains -------------------------------------------------------------------------------------------------------

def test_a_table_filled_above_four_fifths():
    k = 31
    rng = np.random.default_rng(8)
    g = random_genome(rng, 3000)
    counts = kmers_of([g[:1500] + g[300:300 + 50] + g[1500:]], k)
    for s in random_names(rng, 440, k):
        counts[s] = 2
    m = from_dict(counts, k, l=12, canonical=True, hash_seed=8)
    assert m.stats()["distinct"] > 0.8 * 4096
    got, tot, _ = check(m, model=False)
    assert tot["nodes"] == m.stats()["distinct"] and tot["unitigs"] > 440
    m.close()


# ---- 9. the sizing walk of the host and file forms ------------------------------------------------------------------------------

def test_sizing_walk_gives_the_same_unitigs(tmp_path, monkeypatch):
    """Above a record room of 256 MiB the host and file forms walk once for the number of unitigs and once more for the
    records; TSX_HIP_UNITIG_SIZING_BYTES = 0 takes that way on a small table with paths, isolated k-mers and a cycle."""
    from tsxcount_amd import unitig as U
    k = 21
    rng = np.random.default_rng(9)
    counts = reads_graph(rng, k)
    counts.update(kmers_of([random_genome(rng, 90)], k, circular=True, count=4))
    m = from_dict(counts, k, l=14, canonical=True, hash_seed=9)
    want, tot, _ = check(m)
    U.write_unitigs(m, str(tmp_path / "a.fa"))
    monkeypatch.setenv("TSX_HIP_UNITIG_SIZING_BYTES", "0")
    got, tot2, _ = check(m)
    same_unitigs(got, want, k, True)
    assert tot2 == tot and tot["circular"] == 1
    assert U.write_unitigs(m, str(tmp_path / "b.fa")) == tot
    body = lambda name: sorted(open(str(tmp_path / name), "rb").read().split(b"\n")[1::2], key=len)   # noqa: E731
    assert [len(x) for x in body("a.fa")] == [len(x) for x in body("b.fa")] and len(body("b.fa")) == tot["unitigs"]
    assert sorted(body("a.fa")) == sorted(body("b.fa"))      # (one cycle, cut at its lowest slot either way)
    m.close()
