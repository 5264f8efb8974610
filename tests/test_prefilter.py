"""Counting only the k-mers seen twice, on the GPU: pass 1 (the prefilter's two filters), pass 2 (the armed count) and the
contract between them, through Python, the C ABI and the tsxCount CLI.

The yardstick is a Python Counter over the text's windows (test_base_rule.oracle: the reference's record rules, the base
rule, canonical form) and tsxcount_amd.prefilter_masks, which is numpy alone -- never the library's own unfiltered count,
except in the CLI test, where the comparison of the two runs is the point."""
import ctypes
import functools
import random

import numpy as np
import pytest

from test_base_rule import edited_text, encode_np, oracle, records
from test_prefilter_cpu import model_filters
from test_read_query import fastq_of, random_seqs, run_cli

L_TABLE = 16


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


@functools.lru_cache(maxsize=None)
def reads_text(k):
    """300 reads drawn from a 2 000-base random genome with a repeat, 1 % substitutions: thousands of k-mers seen once
    (every error makes up to k of them) and thousands seen again.  100 bases a read; k + 60 where k leaves no window."""
    rnd = random.Random(4000 + k)
    unit = random_seqs(rnd, 1, 300, 300)[0]
    genome = random_seqs(rnd, 1, 700, 700)[0] + unit + random_seqs(rnd, 1, 700, 700)[0] + unit
    n = 100 if k < 64 else k + 60
    seqs = []
    for _ in range(300):
        at = rnd.randrange(len(genome) - n + 1)
        s = bytearray(genome[at:at + n])
        for i in range(n):
            if rnd.random() < 0.01:
                s[i] = rnd.choice(b"ACGT".replace(bytes([s[i]]), b""))
        seqs.append(bytes(s))
    return fastq_of(seqs)


@functools.lru_cache(maxsize=None)
def truth(text, k, canonical=False, acgt_only=False, min_qual=None):
    """(Counter of coded k-mers, their encoded limbs in sorted order, their counts)."""
    kept, _ = oracle(text, k, acgt_only, min_qual, canonical)
    keys = sorted(kept)
    return kept, encode_np(keys, k), np.array([kept[x] for x in keys], dtype=np.uint64)


def as_dict(kmers, counts):
    return {tuple(int(x) for x in row): int(c) for row, c in zip(np.asarray(kmers).reshape(len(counts), -1), counts)}


def new_map(T, k, canonical=False, **kw):
    return T.TSXHashMapHIP(L_TABLE, 0, k, canonical=canonical, **kw)


def to_device(text):
    import torch
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()                                     # (the map's stream does not wait for torch's)
    return dev


def check_filters(T, m, enc, counts, k, bits, kmers):
    """A is exact; B holds every k-mer seen twice and nothing that is no k-mer's; the pass-1 totals."""
    A, lo, hi = model_filters(T, (enc, counts), k, bits)
    a, b = m.prefilterWords("a"), m.prefilterWords("b")
    assert a.dtype == np.uint64 and a.shape == A.shape and b.shape == lo.shape
    assert np.array_equal(a, A), np.flatnonzero(a != A)[:8]
    assert not (lo & ~b).any(), "a k-mer seen twice is not in B"
    assert not (b & ~hi).any(), "a bit of B that belongs to no k-mer"
    st = m.prefilter_stats
    assert st["bits"] == bits and st["seen"] == kmers and st["admitted"] == 0 and st["skipped"] == 0
    assert st["seen_again"] >= kmers - len(counts)               # every occurrence after the first (+ false positives)
    assert st["set_bits_a"] == sum(bin(int(x)).count("1") for x in A) and st["set_bits_b"] == sum(bin(int(x)).count("1") for x in b)


def check_contract(m, kept_enc_counts, kmers, bits=None):
    """The table after pass 2 against the Counter; returns (entries of count 1, the text's singletons)."""
    enc, counts = kept_enc_counts
    want = as_dict(enc, counts)
    got = as_dict(*m.getAllKmers())
    for key, c in want.items():
        if c >= 2:
            assert got.get(key) == c, (key, c, got.get(key))     # every k-mer seen twice, with its exact count
    for key, c in got.items():
        assert want.get(key) == c, (key, c, want.get(key))       # every entry is a k-mer of the text, with its exact count
    st, pst = m.stats(), m.prefilter_stats
    assert pst["admitted"] + pst["skipped"] == kmers == pst["seen"]
    assert st["kmers_added"] == pst["admitted"] == sum(got.values()) and st["distinct"] == len(got)
    ones, singles = sum(1 for c in got.values() if c == 1), sum(1 for c in want.values() if c == 1)
    print("bits=%s entries=%d of %d distinct, count-1 entries=%d of %d singletons" % (bits, len(got), len(want), ones, singles))
    return ones, singles


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [20, 12])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [15, 31, 33, 63, 127])
def test_filter_a_is_exact_and_b_is_bounded(T, k, canonical, bits):
    text = reads_text(k)
    kept, enc, counts = truth(text, k, canonical)
    assert (counts == 1).sum() > 3000 and (counts >= 2).sum() > 1000
    m = new_map(T, k, canonical)
    try:
        m.prefilter(text, bits=bits)
        check_filters(T, m, enc, counts, k, bits, int(counts.sum()))
        st = m.stats()
        assert st["distinct"] == 0 and st["kmers_added"] == 0    # pass 1 writes no table
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,canonical", [(31, True), (127, False)])
def test_pieces_device_windows_and_the_c_abi(T, k, canonical, monkeypatch):
    text = reads_text(k)
    kept, enc, counts = truth(text, k, canonical)
    kmers = int(counts.sum())
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "4096")            # (read when a map is created)
    assert len(text) > 15 * 4096
    m = new_map(T, k, canonical)
    try:
        m.prefilter(text, bits=20)
        check_filters(T, m, enc, counts, k, 20, kmers)
        # chunk_bytes of the call, through the C ABI: a second filter replaces the first
        assert T.lib().tsx_hip_prefilter_create(m.handle, 18) == T.OK
        assert T.lib().tsx_hip_prefilter_add_host(m.handle, text, len(text), 5000) == T.OK
        check_filters(T, m, enc, counts, k, 18, kmers)
        # the device call, in windows of 4 096 and 5 008 bytes
        dev = to_device(text)
        for win in (4096, 5000):
            monkeypatch.setenv("TSX_HIP_DEV_WINDOW", str(win))
            m.prefilterDevice(dev.data_ptr(), len(text), bits=20)
            m.sync()
            check_filters(T, m, enc, counts, k, 20, kmers)
        assert T.lib().tsx_hip_prefilter_add_device(m.handle, ctypes.c_void_p(dev.data_ptr() + 8), 16, None) == T.EINVAL
        # pass 2 through the device call, the windows still small
        m.armPrefilter()
        m.countFastqDevice(dev.data_ptr(), len(text))
        m.sync()
        check_contract(m, (enc, counts), kmers, 20)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pass1", ["device", "host"])
def test_caller_streams(T, pass1):
    """Pass 1 and pass 2 on streams of the caller's, with nothing between them but the library's own ordering: the filter
    is created (32 MiB + 8 MiB zeroed on the map's stream) and filled on one stream in ONE call, the armed count runs on
    another.  A is exact -- no bit was wiped by the zeroing -- and the contract holds."""
    import torch
    k, bits = 31, 28
    text = reads_text(k)
    kept, enc, counts = truth(text, k)
    dev = to_device(text)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    m = new_map(T, k)
    try:
        if pass1 == "device":
            m.prefilterDevice(dev.data_ptr(), len(text), bits=bits, stream=s1.cuda_stream)
        else:
            m.prefilter(text, bits=bits)
        assert m.prefilter_bits == bits
        m.armPrefilter()
        m.countFastqDevice(dev.data_ptr(), len(text), stream=s2.cuda_stream)
        s2.synchronize()
        m.sync()
        wa, _, mk = T.prefilter_masks(enc, k, bits)
        A = np.zeros(1 << (bits - 6), dtype=np.uint64)
        np.bitwise_or.at(A, wa.astype(np.int64), mk)
        assert np.array_equal(m.prefilterWords("a"), A)
        ones, singles = check_contract(m, (enc, counts), int(counts.sum()), bits)
        assert ones <= singles // 100
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [20, 12])
@pytest.mark.parametrize("k,canonical,path", [(31, False, 0), (31, True, 2), (33, True, 0), (63, False, 0), (127, True, 0), (15, False, 0)])
def test_the_contract(T, k, canonical, path, bits):
    """bits = 20: the entries of count 1 are at most 1 % of the text's singletons (a CPU simulation of the definition with
    20 000 keys admitted 1 of 15 038; this text has fewer keys).  bits = 12: the filters are saturated, the table may
    equal the full count, and every assertion on counts holds all the same."""
    text = reads_text(k)
    kept, enc, counts = truth(text, k, canonical)
    m = new_map(T, k, canonical)
    try:
        m.set_path(path)                                         # (armed: the atomic path whatever this says)
        m.prefilter(text, bits=bits)
        m.armPrefilter()
        m.countFastq(text)
        m.armPrefilter(False)
        ones, singles = check_contract(m, (enc, counts), int(counts.sum()), bits)
        assert singles > 3000
        if bits == 20:
            assert ones <= singles // 100
        else:
            assert m.prefilter_stats["set_bits_a"] >= 4000       # A's 64 words: (nearly) every bit
        # not gated, armed or not: the read calls and addKmers
        m.armPrefilter()
        idx = np.flatnonzero(counts >= 2)[:3]
        m.addKmers(enc[idx], np.array([5, 5, 5], dtype=np.uint64))
        assert np.array_equal(m.getKmerCounts(enc[idx]), counts[idx] + np.uint64(5))
    finally:
        m.close()


@pytest.mark.gpu
def test_count_twice_and_default_bits(T):
    k = 31
    text = reads_text(k)
    kept, enc, counts = truth(text, k)
    m = new_map(T, k)
    try:
        st = m.countTwice(text)
        assert st["bits"] == L_TABLE + 6 and st == m.prefilter_stats
        ones, singles = check_contract(m, (enc, counts), int(counts.sum()), st["bits"])
        assert ones <= singles // 100
        m.freePrefilter()
        assert m.prefilter_stats == dict.fromkeys(st, 0)
        with pytest.raises(T.TSXException):
            m.armPrefilter()
    finally:
        m.close()
    m = T.TSXHashMapHIP(4, 0, k)                                 # l + 6 below the range: clamped to 12
    try:
        m.prefilter(b"")
        assert m.prefilter_stats["bits"] == 12 == m.prefilter_bits
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 40])
def test_runs_of_equal_neighbours(T, k, monkeypatch):
    rnd = random.Random(k)
    noise = random_seqs(rnd, 60, 90, 110)
    poly = lambda base, n: bytes([base]) * n                     # noqa: E731
    for run, n in ((poly(65, k + 1), 2), (poly(65, 200), 201 - k)):   # one wave; across the lane 63 / lane 0 boundary
        text = fastq_of(noise[:20] + [run] + noise[20:])
        kept, enc, counts = truth(text, k)
        assert kept[poly(65, k)] == n
        m = new_map(T, k)
        try:
            m.prefilter(text, bits=20)
            m.armPrefilter()
            m.countFastq(text)
            check_contract(m, (enc, counts), int(counts.sum()))
            assert int(m.getKmerCounts(encode_np([poly(65, k)], k))[0]) == n
        finally:
            m.close()
    # one k-mer, two occurrences that are no neighbours: in two pieces of one call, and in two calls
    twin = random_seqs(rnd, 1, k, k)[0]
    one, two = fastq_of([twin + b"C"] + noise[:30], b"a"), fastq_of(noise[30:] + [b"G" + twin], b"b")
    kept, enc, counts = truth(one + two, k)
    assert kept[twin] == 2 and len(one) > 4096 and len(two) > 4096
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "4096")
    for calls in ((one + two,), (one, two)):
        m = new_map(T, k)
        try:
            m.createPrefilter(20)
            for part in calls:
                m.prefilter(part)                                # several calls accumulate
            m.armPrefilter()
            for part in calls:
                m.countFastq(part)
            check_contract(m, (enc, counts), int(counts.sum()))
            assert int(m.getKmerCounts(encode_np([twin], k))[0]) == 2
        finally:
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("acgt_only,min_qual", [(True, None), (False, "5"), (True, "5")])
def test_base_rule(T, acgt_only, min_qual):
    """Windows the rule drops reach neither filter nor table."""
    k = 21
    text = edited_text(3100, 60, k)
    text = b"".join(rec for _, _, rec in records(text)[:20]) + text   # (its reads share no k-mers: twenty of them twice)
    kept, enc, counts = truth(text, k, False, acgt_only, min_qual)
    plain = truth(text, k)[0]
    assert len(kept) < len(plain) and (counts >= 2).sum() > 300 and (counts == 1).sum() > 300
    m = new_map(T, k, acgt_only=acgt_only, min_qual_char=min_qual)
    try:
        m.prefilter(text, bits=20)
        check_filters(T, m, enc, counts, k, 20, int(counts.sum()))
        m.armPrefilter()
        m.countFastq(text)
        check_contract(m, (enc, counts), int(counts.sum()), 20)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("min_qual", [None, "5"])
def test_bgzf(T, min_qual, monkeypatch):
    """prefilterBgzf + countFastqBgzf against the host-text path on the same records.  bits = 26: with 2^20 words for
    these few thousand keys no k-mer seen once has its four bits set by others, so that the dumps are equal whatever the
    order of the windows was (at a small filter the entries of count 1 may depend on it)."""
    k = 31
    text = edited_text(77, 200, k) if min_qual else reads_text(k)
    kept, enc, counts = truth(text, k, False, False, min_qual)
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")                # (the smallest batch the library takes: 128 KiB)
    dumps, words = [], []
    for block in (None, 1000, 65280):
        m = new_map(T, k, min_qual_char=min_qual)
        try:
            if block is None:
                m.prefilter(text, bits=26)
                m.armPrefilter()
                m.countFastq(text)
            else:
                gz = T.bgzf_compress(text, block=block)
                m.prefilterBgzf(gz, bits=26)
                m.armPrefilter()
                m.countFastqBgzf(gz)
            check_contract(m, (enc, counts), int(counts.sum()), 26)
            words.append(m.prefilterWords("a"))
            dumps.append(as_dict(*m.getAllKmers()))
        finally:
            m.close()
    A = model_filters(T, (enc, counts), k, 26)[0]
    assert all(np.array_equal(w, A) for w in words)
    assert dumps[0] == dumps[1] == dumps[2] and len(dumps[0]) == int((counts >= 2).sum())


@pytest.mark.gpu
def test_refusals_leave_the_table_alone(T):
    k = 31
    L = T.lib()
    text = reads_text(k)
    m = new_map(T, k)
    try:
        m.countFastq(text)
        before = m.stats()
        one = np.zeros(64, dtype=np.uint64)
        p64 = one.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        # without a filter: arm, add, read
        assert L.tsx_hip_prefilter_arm(m.handle, 1) == T.EINVAL and L.tsx_hip_prefilter_arm(m.handle, 0) == T.OK
        assert L.tsx_hip_prefilter_add_host(m.handle, text, len(text), 0) == T.EINVAL
        assert L.tsx_hip_prefilter_add_bgzf_host(m.handle, text, len(text)) == T.EINVAL
        assert L.tsx_hip_prefilter_add_device(m.handle, ctypes.c_void_p(0x1000), 16, None) == T.EINVAL
        assert L.tsx_hip_prefilter_read(m.handle, 0, p64, 64) == T.EINVAL
        for bits in (11, 39):
            assert L.tsx_hip_prefilter_create(m.handle, bits) == T.EINVAL
            assert L.tsx_hip_prefilter_armed(m.handle) == 0 and m.prefilter_stats["bits"] == 0
        # with one: the wrong size of a read, wrapped FASTA while armed
        m.createPrefilter(12)
        assert L.tsx_hip_prefilter_read(m.handle, 0, p64, 63) == T.ERANGE and L.tsx_hip_prefilter_read(m.handle, 2, p64, 64) == T.EINVAL
        assert L.tsx_hip_prefilter_read(m.handle, 0, p64, 64) == T.OK and L.tsx_hip_prefilter_read(m.handle, 1, p64, 16) == T.OK
        m.armPrefilter()
        assert L.tsx_hip_prefilter_armed(m.handle) == 1
        fa = b">x\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\nACGTACGTACGT\n"
        for call in (lambda: m.countFasta(fa), lambda: m.countFastaBgzf(T.bgzf_compress(fa))):
            with pytest.raises(T.TSXException) as ei:
                call()
            assert ei.value.code == T.EINVAL and "prefilter" in str(ei.value)
        assert m.stats() == before and not m.prefilterWords("a").any()
        m.armPrefilter(False)
        m.countFasta(fa)                                         # disarmed: counted
        assert m.stats()["kmers_added"] == before["kmers_added"] + 48 - k + 1
    finally:
        m.close()
    # a shard map: the filter may be filled, the armed count is refused
    m = T.TSXHashMapHIP(L_TABLE, 0, k, shard_bits=1, shard_index=0)
    try:
        m.prefilter(text, bits=20)
        m.armPrefilter()
        assert L.tsx_hip_count_fastq_host(m.handle, text, len(text)) == T.EINVAL
        assert L.tsx_hip_count_fastq_bgzf_host(m.handle, text, len(text)) == T.EINVAL
        assert "prefilter" in L.tsx_hip_last_error().decode()
        st = m.stats()
        assert st["distinct"] == 0 and st["kmers_added"] == 0
    finally:
        m.close()
    # a group: refused while one of its maps is armed
    g = T.TSXHashMapHIPGroup(2, L_TABLE, 0, k, devices=[0, 0], comm="copy")
    try:
        h = ctypes.c_void_p(L.tsx_hip_group_map(g._h, 1))
        assert L.tsx_hip_prefilter_create(h, 12) == T.OK and L.tsx_hip_prefilter_arm(h, 1) == T.OK
        with pytest.raises(T.TSXException) as ei:
            g.countFastq(text)
        assert ei.value.code == T.EINVAL and "prefilter" in str(ei.value) and g.stats()["distinct"] == 0
        assert L.tsx_hip_prefilter_arm(h, 0) == T.OK
        g.countFastq(text)
        assert g.stats()["distinct"] == len(truth(text, k)[0])
    finally:
        g.close()


@pytest.mark.gpu
def test_disarmed_is_untouched(T):
    k = 31
    text = reads_text(k)
    kept, enc, counts = truth(text, k, True)
    m = new_map(T, k, True)
    try:
        m.prefilter(text, bits=20)
        m.armPrefilter()
        m.armPrefilter(False)
        m.countFastq(text)
        assert as_dict(*m.getAllKmers()) == as_dict(enc, counts)
        st = m.prefilter_stats
        assert st["admitted"] == 0 and st["skipped"] == 0 and m.stats()["kmers_added"] == int(counts.sum())
    finally:
        m.close()


def tsv(path):
    return sorted(open(path).read().split("\n")[:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "bgzf-canonical"])
def test_cli_min_count(T, form, tmp_path):
    k = 31
    text = reads_text(k)
    kept, enc, counts = truth(text, k, form != "plain")
    fq = tmp_path / ("reads.fastq" if form == "plain" else "reads.fastq.gz")
    fq.write_bytes(text if form == "plain" else T.bgzf_compress(text, block=20000))
    mode = [] if form == "plain" else ["--canonical"]
    outs = {}
    for name, extra in (("all", []), ("twice", ["--min-count=2"]), ("small", ["--min-count=2", "--prefilter-bits=12"])):
        f, h = tmp_path / (name + ".tsv"), tmp_path / (name + ".histo")
        code, out, err = run_cli("--input=" + str(fq), "--k=%d" % k, "--l=%d" % L_TABLE, "--output=" + str(f), "--lower=2",
                                 "--histo=" + str(h), *mode, *extra)
        assert code == 0, err
        outs[name] = (tsv(f), {ln.split()[0]: ln.split()[1] for ln in tsv(h)}, out)
    lines, histo, out = outs["all"]
    assert len(lines) == int((counts >= 2).sum()) > 1000 and "prefilter\t" not in out
    for name, bits in (("twice", L_TABLE + 6), ("small", 12)):
        got_lines, got_histo, got_out = outs[name]
        assert got_lines == lines                                # --lower=2: the same set of lines
        assert {c: n for c, n in got_histo.items() if int(c) >= 2} == {c: n for c, n in histo.items() if int(c) >= 2}
        pf = [ln.split("\t") for ln in got_out.splitlines() if ln.startswith("prefilter\t")]
        assert len(pf) == 1 and len(pf[0]) == 6, got_out
        _, b, kmers, again, admitted, skipped = pf[0][0], *map(int, pf[0][1:])
        assert b == bits and kmers == int(counts.sum()) and admitted + skipped == kmers and again >= kmers - len(counts)
        assert admitted >= int(counts[counts >= 2].sum())
    # fewer slots: the distinct k-mers of the filtered run are those seen twice (+ at most 1 % of the singletons)
    distinct = int(outs["twice"][2].split("Added a total of ")[1].split()[0])
    assert int((counts >= 2).sum()) <= distinct <= int((counts >= 2).sum()) + int((counts == 1).sum()) // 100
