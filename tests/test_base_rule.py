"""The base rule (tsx_hip_set_base_rule): acgt_only drops every window with a byte outside ACGTacgt, min_qual_char every
window with a base whose quality byte is below it or missing.  Checked against a dictionary count with the reference's
record rules plus the two rules, on texts with N runs, lowercase and IUPAC bytes, short and long quality lines, '+'
lines that repeat the header, empty lines and an unterminated last record."""
import os
import random
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
HEADER = os.path.join(ROOT, "include", "tsxcount_hip.h")
U64 = (1 << 64) - 1
_CODE = bytes(b"ACGT"[((b >> 1) ^ (b >> 2)) & 3] for b in range(256))   # base_code as a byte table
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = frozenset(b"ACGTacgt")
KS = [5, 14, 21, 31, 32, 33, 47, 63, 64, 96, 127]
RULES = [(True, None), (False, "5"), (True, "5")]


# ---- the oracle --------------------------------------------------------------------------------------------------

def records(text, lpr=4):
    """[(sequence line, quality line, record bytes as the filter writes them)]: empty lines dropped, lpr lines a record."""
    spans, pos = [], 0
    for part in text.split(b"\n"):
        if part:
            spans.append((pos, pos + len(part)))
        pos += len(part) + 1
    out = []
    for i in range(0, len(spans), lpr):
        g = spans[i:i + lpr]
        seq = text[g[1][0]:g[1][1]] if len(g) > 1 else b""
        qual = text[g[3][0]:g[3][1]] if lpr == 4 and len(g) > 3 else b""
        out.append((seq, qual, text[g[0][0]:g[-1][1]] + b"\n"))
    return out


def windows(seq, qual, k, acgt_only, min_qual):
    """(start, kept) of every window of k bytes of a sequence line."""
    q = ord(min_qual) if min_qual else 0
    for i in range(len(seq) - k + 1):
        ok = True
        if acgt_only and any(b not in ACGT for b in seq[i:i + k]):
            ok = False
        if q and any(j >= len(qual) or qual[j] < q for j in range(i, i + k)):
            ok = False
        yield i, ok


def oracle(text, k, acgt_only=False, min_qual=None, canonical=False):
    """(kept: Counter of coded k-mers, dropped: coded k-mers that occur only in dropped windows)."""
    kept, seen = Counter(), set()
    for seq, qual, _ in records(text):
        s = seq.translate(_CODE)
        for i, ok in windows(seq, qual, k, acgt_only, min_qual):
            x = s[i:i + k]
            if canonical:
                x = min(x, x[::-1].translate(_COMP))
            if ok:
                kept[x] += 1
            else:
                seen.add(x)
    return kept, seen - set(kept)


def oracle_stats(query, counts, k, acgt_only, min_qual, lower, upper):
    out = []
    for seq, qual, _ in records(query):
        s = seq.translate(_CODE)
        cs = [counts.get(s[i:i + k], 0) for i, ok in windows(seq, qual, k, acgt_only, min_qual) if ok]
        out.append((len(cs), sum(lower <= c <= upper for c in cs), min(cs) if cs else 0, sum(cs) % (1 << 64)))
    return out


def encode_np(kmers, k):
    """tsx_hip_encode of coded k-mers (ACGT only), vectorised: base i in bits 2i, 2i + 1 of limb i / 32."""
    wk = (2 * k + 63) // 64
    if not kmers:
        return np.zeros((0, wk), dtype=np.uint64)
    a = np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(-1, k)
    codes = (((a >> 1) ^ (a >> 2)) & 3).astype(np.uint64)
    out = np.zeros((a.shape[0], wk), dtype=np.uint64)
    for i in range(k):
        out[:, i // 32] |= codes[:, i] << np.uint64(2 * (i % 32))
    return out


# ---- texts -------------------------------------------------------------------------------------------------------

def edited_text(seed, n_reads=120, k=31):
    """synth.fastq reads with edits: N runs, IUPAC and lowercase bytes, random qualities of shifting length, empty lines,
    '+' lines with the header, reads shorter than k, an unterminated last record."""
    from tsxcount_amd import synth
    rnd = random.Random(seed)
    base = [ln for ln in synth.fastq(seed, 0, n_reads).split(b"\n") if ln]
    alphabet = b"ACG" if k < 8 else b"ACGT"   # k = 5: few enough distinct k-mers for a 2^9-slot table
    seqs = [bytearray(base[i].translate(bytes.maketrans(b"T", b"G")) if k < 8 else base[i]) for i in range(1, len(base), 4)]
    seqs += [bytearray(rnd.choice(alphabet) for _ in range(rnd.randint(1, k - 1))) for _ in range(6)]   # shorter than k
    parts = []
    for r, s in enumerate(seqs):
        kind = r % 9
        if kind == 0 and len(s) > 2:
            for _ in range(3):
                s[rnd.randrange(len(s))] = ord("N")
        elif kind == 1:
            run = rnd.randint(k, k + 40)
            at = rnd.randrange(len(s) + 1)
            s[at:at] = b"N" * run
        elif kind == 2 and s:
            s[0] = ord("N")
            s[-1] = ord("n")
        elif kind == 3 and len(s) > 10:
            a = rnd.randrange(len(s) - 8)
            s[a:a + 8] = bytes(s[a:a + 8]).lower()
        elif kind == 4 and s:
            for _ in range(2):
                s[rnd.randrange(len(s))] = ord(rnd.choice("RYKM"))
        # '!' .. 'J', 3 % of them below '5' (the rule's threshold in these tests): long k-mers survive too
        qual = bytearray(rnd.randint(53, 74) if rnd.random() < 0.97 else rnd.randint(33, 52) for _ in range(len(s)))
        if r % 7 == 3:
            qual = qual[:rnd.randint(0, len(qual))]                   # shorter than the sequence
        elif r % 7 == 5:
            qual += bytes(rnd.randint(33, 74) for _ in range(rnd.randint(1, 30)))   # longer
        head = b"@read%d" % r
        plus = b"+" + head[1:] if r % 5 == 2 else b"+"
        parts.append(head + b"\n" + bytes(s) + b"\n" + plus + b"\n" + bytes(qual) + b"\n")
        if r % 11 == 4:
            parts.append(b"\n\n")
    text = b"".join(parts)
    return text[:-1]   # the last record without its '\n'


def max_record(text):
    return max(len(r) for _, _, r in records(text))


# ---- CPU ---------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("tsx_hip_set_base_rule", "tsx_hip_get_base_rule", "tsx_hip_group_set_base_rule")


def test_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tsxcount_amd", "lib", "libtsxcount_hip.so")],
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name
    # no map: EINVAL, nothing dereferenced
    a, q = T.ctypes.c_int(7), T.ctypes.c_int(7)
    assert L.tsx_hip_set_base_rule(None, 1, 0) == T.EINVAL
    assert L.tsx_hip_get_base_rule(None, T.ctypes.byref(a), T.ctypes.byref(q)) == T.EINVAL
    assert L.tsx_hip_group_set_base_rule(None, 1, 0) == T.EINVAL


def test_python_argument_checks():
    import tsxcount_amd as T
    assert T.min_qual_code(None) == 0 and T.min_qual_code(0) == 0
    assert T.min_qual_code("5") == 53 and T.min_qual_code(b"I") == 73 and T.min_qual_code(40) == 40
    for bad in ("", "55", 256, -1):
        with pytest.raises(ValueError):
            T.min_qual_code(bad)
    for bad in (1.5, True, [5]):
        with pytest.raises(TypeError):
            T.min_qual_code(bad)
    # refused before anything is allocated: no device needed
    with pytest.raises(ValueError):
        T.TSXHashMapHIP(16, 0, 21, min_qual_char="ab")
    with pytest.raises(ValueError):
        T.TSXHashMapHIPGroup(2, 16, 0, 21, devices=[0, 0], comm="copy", min_qual_char=300)


def test_oracle_rules():
    text = b"@a\nACGTNACGTA\n+\nIIIII!IIII\n\n@b\nacgtRa\n+a\nIII\n@c\nAC"
    (s1, q1, _), (s2, q2, _), (s3, q3, _) = records(text)
    assert (s1, q1, s2, q2, s3, q3) == (b"ACGTNACGTA", b"IIIII!IIII", b"acgtRa", b"III", b"AC", b"")
    assert [ok for _, ok in windows(s1, q1, 4, True, None)] == [True, False, False, False, False, True, True]
    assert [ok for _, ok in windows(s1, q1, 4, False, "5")] == [True, True, False, False, False, False, True]
    assert [ok for _, ok in windows(s2, q2, 2, False, "5")] == [True, True, False, False, False]
    assert [ok for _, ok in windows(s2, q2, 2, True, None)] == [True, True, True, False, False]
    kept, dropped = oracle(text, 4, True, None)
    assert kept == Counter({b"ACGT": 3, b"CGTA": 1})
    assert b"GTAA" in dropped   # "GTNA": N as A, a window the rule drops
    import tsxcount_amd as T
    xs = [b"ACGT" * 8 + b"GA", b"T" * 33, b"CAGT" * 31 + b"ACG"]
    for x in xs:
        assert np.array_equal(encode_np([x], len(x))[0], T.encode(x, len(x)))


@pytest.mark.parametrize("args,msg", [
    (["--input=x.fasta", "--format=fasta", "--min-qual-char=5"], "--min-qual-char needs FASTQ"),
    (["--input=x.fastq", "--gpus=2", "--comm=copy", "--devices=0,0", "--exchange=mini", "--acgt-only"], "--exchange=mini has no base rule"),
    (["--input=x.fastq", "--min-qual-char=55"], "--min-qual-char takes one character"),
])
def test_cli_refusals(args, msg):
    p = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and msg in p.stderr.decode(), p.stderr.decode()


def test_cli_usage_lists_the_options():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    err = p.stderr.decode()
    assert "--acgt-only" in err and "--min-qual-char=C" in err


# ---- GPU ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def check_table(m, k, kept, dropped, canonical=False):
    keys = sorted(kept)
    got = m.getKmerCounts(encode_np(keys, k))
    want = np.array([kept[x] for x in keys], dtype=np.uint64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(keys[i], int(got[i]), int(want[i])) for i in bad[:5]]
    st = m.stats()
    assert st["distinct"] == len(kept) and st["kmers_added"] == sum(kept.values()), (st, len(kept), sum(kept.values()))
    if dropped:
        assert not m.getKmerCounts(encode_np(sorted(dropped), k)).any()


def dump(m):
    km, c = m.getAllKmers()
    i = np.lexsort(km.T[::-1])
    return km[i], c[i]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_exact_counts(T, k):
    text = edited_text(100 + k, k=k)
    for path in (1, 2):
        for acgt, mq in RULES:
            kept, dropped = oracle(text, k, acgt, mq)
            assert kept and dropped
            m = T.TSXHashMapHIP(20 if k > 10 else 2 * k - 1, 0, k, acgt_only=acgt, min_qual_char=mq)
            m.set_path(path)
            assert m.base_rule == (acgt, mq)
            m.countFastq(text)
            check_table(m, k, kept, dropped)
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31, 63])
def test_poly_n_is_not_poly_a(T, k):
    """With acgt_only a text with long N runs gives the poly-A k-mer exactly its real count; without the rule N still
    counts as A (the default stand-in code, unchanged)."""
    reads = [b"N" * 200, b"ACGT" * 10 + b"N" * 80 + b"A" * (k + 3) + b"N" * 50, b"n" * 150, b"A" * (k + 1)]
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads))
    poly_a = encode_np([b"A" * k], k)
    for path in (1, 2):
        m = T.TSXHashMapHIP(18, 0, k, acgt_only=True)
        m.set_path(path)
        m.countFastq(text)
        assert int(m.getKmerCounts(poly_a)[0]) == 4 + 2
        check_table(m, k, *oracle(text, k, True, None))
        m.set_base_rule()        # off again: the same table now also gets N as A
        m.clear()
        m.countFastq(text)
        kept, _ = oracle(text, k)
        assert int(m.getKmerCounts(poly_a)[0]) == kept[b"A" * k] > 200
        check_table(m, k, kept, set())
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 63])
def test_seams_host_pieces(T, k, monkeypatch):
    text = edited_text(7 + k, n_reads=200, k=k)
    mr = max_record(text)
    for acgt, mq in RULES:
        kept, dropped = oracle(text, k, acgt, mq)
        for piece in (mr + 1, mr + 17, 4096, 5000, 1 << 20):
            monkeypatch.setenv("TSX_HIP_PIECE_BYTES", str(max(piece, 256)))
            for path in (1, 2):
                m = T.TSXHashMapHIP(20, 0, k, acgt_only=acgt, min_qual_char=mq)
                m.set_path(path)
                m.countFastq(text)
                check_table(m, k, kept, dropped)
                m.close()
    # a record longer than a piece: ERANGE under a quality rule, not a silent miscount
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "256")
    long_rec = b"@x\n" + b"ACGT" * 100 + b"\n+\n" + b"I" * 400 + b"\n"
    m = T.TSXHashMapHIP(18, 0, k, min_qual_char="5")
    with pytest.raises(T.TSXException) as e:
        m.countFastq(long_rec * 3)
    assert e.value.code == T.ERANGE
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 63])
def test_seams_device_windows(T, k, monkeypatch):
    import torch
    text = edited_text(31 + k, n_reads=200, k=k)
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(text + b"\n" * 64), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    for acgt, mq in RULES:
        kept, dropped = oracle(text, k, acgt, mq)
        for win in (None, 4096, 4112, 20000):
            if win:
                monkeypatch.setenv("TSX_HIP_DEV_WINDOW", str(win))
            else:
                monkeypatch.delenv("TSX_HIP_DEV_WINDOW", raising=False)
            for path in (1, 2):
                m = T.TSXHashMapHIP(20, 0, k, acgt_only=acgt, min_qual_char=mq)
                m.set_path(path)
                m.countFastqDevice(d_text.data_ptr(), len(text))
                check_table(m, k, kept, dropped)
                m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,block", [(31, 65280), (63, 700)])
def test_seams_bgzf_batches(T, k, block, monkeypatch):
    text = edited_text(57 + k, n_reads=900, k=k)
    assert len(text) > 3 * (128 << 10)      # several batches of the smallest size
    z = T.bgzf_compress(text, level=1, block=block)
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")      # clamped to the minimum, 128 KiB
    for acgt, mq in RULES:
        kept, dropped = oracle(text, k, acgt, mq)
        a = T.TSXHashMapHIP(21, 0, k, acgt_only=acgt, min_qual_char=mq)
        b = T.TSXHashMapHIP(21, 0, k, acgt_only=acgt, min_qual_char=mq)
        a.countFastq(text)
        b.countFastqBgzf(z)
        check_table(b, k, kept, dropped)
        ka, ca = dump(a)
        kb, cb = dump(b)
        assert np.array_equal(ka, kb) and np.array_equal(ca, cb)
        a.close(); b.close()


def long_record_text(seed=2024):
    """About 40 short records, one record of 300 000 bases with a few qualities below '5', about 40 short records."""
    rnd = random.Random(seed)

    def rec(name, n, low):
        qual = bytearray(b"I" * n)
        for i in low:
            qual[i] = ord("+")
        return b"@%s\n%s\n+\n%s\n" % (name, bytes(rnd.choices(b"ACGT", k=n)), bytes(qual))

    def short(tag):
        return b"".join(rec(b"%s%d" % (tag, i), rnd.randint(60, 150), (rnd.randrange(60),) if i % 5 == 0 else ())
                        for i in range(40))

    return short(b"a") + rec(b"long", 300000, (7, 99999, 100010, 250000, 299990)) + short(b"b")


@pytest.mark.gpu
def test_bgzf_record_longer_than_a_batch(T, monkeypatch):
    """A record that spans several of the smallest BGZF batches: the middle batches hold no whole record and are carried
    whole under a quality rule (the count and the sketch); without the rule the long lines cross the double-buffered
    batches.  Both give what the plain text gives on the host path, which sees the record whole."""
    k, block = 31, 65280
    text = long_record_text()
    z = T.bgzf_compress(text, level=1, block=block)
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")      # clamped to the minimum, 128 KiB: two members a batch
    monkeypatch.delenv("TSX_HIP_PIECE_BYTES", raising=False)
    batch = 2 * block
    nbatch = (len(text) + batch - 1) // batch
    ends, pos = set(), 0
    for _, _, r in records(text):
        pos += len(r)
        ends.add((pos - 1) // batch)
    assert nbatch >= 5 and len(set(range(nbatch - 1)) - ends) >= 2      # middle batches without a record end
    for mq in ("5", None):
        kept, dropped = oracle(text, k, False, mq)
        assert kept and bool(dropped) == bool(mq)
        a = T.TSXHashMapHIP(21, 0, k, min_qual_char=mq)
        b = T.TSXHashMapHIP(21, 0, k, min_qual_char=mq)
        a.countFastq(text)
        b.countFastqBgzf(z)
        check_table(b, k, kept, dropped)
        ka, ca = dump(a)
        kb, cb = dump(b)
        assert np.array_equal(ka, kb) and np.array_equal(ca, cb)
        ra, ta = a.sketchKmers(text)
        rb, tb = b.sketchKmersBgzf(z)
        assert np.array_equal(ra, rb) and ta == tb and ta["kmers"] == sum(kept.values()), (ta, tb)
        a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 32, 64])
def test_canonical_and_rule_changes(T, k):
    t1, t2 = edited_text(300 + k, 60, k), edited_text(400 + k, 60, k)
    for path in (1, 2):
        m = T.TSXHashMapHIP(20, 0, k, canonical=True, acgt_only=True, min_qual_char="5")
        m.set_path(path)
        m.countFastq(t1)
        kept, dropped = oracle(t1, k, True, "5", canonical=True)
        check_table(m, k, kept, set())
        # the rule changes between two calls on one table: each call counts under its own rule
        m.set_base_rule(acgt_only=True)
        assert m.base_rule == (True, None)
        m.countFastq(t2)
        k2, _ = oracle(t2, k, True, None, canonical=True)
        both = kept + k2
        check_table(m, k, both, set())
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [19, 31, 47])
def test_queries(T, k, tmp_path):
    import torch
    text = edited_text(500 + k, 150, k)
    for acgt, mq in RULES:
        kept, _ = oracle(text, k, acgt, mq)
        m = T.TSXHashMapHIP(20, 0, k, acgt_only=acgt, min_qual_char=mq)
        m.countFastq(text)
        added = m.stats()["kmers_added"]
        want = oracle_stats(text, kept, k, acgt, mq, 2, U64)
        assert sum(w[0] for w in want) == added
        for chunk in (0, 4096, 5000):
            got = [tuple(int(v) for v in r) for r in m.queryReads(text, 2, chunk_bytes=chunk)]
            assert got == want, chunk
        assert sum(g[0] for g in got) == added
        dev = torch.device("cuda", 0)
        d_text = torch.frombuffer(bytearray(text + b"\n" * 64), dtype=torch.uint8).to(dev)
        stats = torch.zeros((len(want) + 3) * 4, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for win in (None, 4096):
            if win:
                os.environ["TSX_HIP_DEV_WINDOW"] = str(win)
            try:
                n = m.queryReadsDevice(d_text.data_ptr(), len(text), stats.data_ptr(), len(want) + 3, lower=2)
            finally:
                os.environ.pop("TSX_HIP_DEV_WINDOW", None)
            got = [tuple(int(v) for v in r) for r in stats.cpu().numpy().view(np.uint64).reshape(-1, 4)[:n]]
            assert got == want, win
        # the filter keeps what the oracle's stats select (a record with no k-mer left passes a fraction rule)
        out = tmp_path / "kept.fq"
        nk, nb = m.filterReads(text, str(out), lower=2, fraction=0.5, chunk_bytes=4096)
        recs = records(text)
        sel = [r for (_, _, r), (km, inr, _, _) in zip(recs, want) if inr * 1000000 >= 500000 * km]
        assert nk == len(sel) and out.read_bytes() == b"".join(sel)
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_merge_and_exchange_refusals(T, ranks):
    k = 31
    text = edited_text(77, 200, k)
    for acgt, mq in RULES:
        kept, dropped = oracle(text, k, acgt, mq)
        g = T.TSXHashMapHIPGroup(ranks, 20, 0, k, devices=[0] * ranks, comm="copy", acgt_only=acgt, min_qual_char=mq)
        assert g.base_rule == (acgt, mq)
        g.countFastq(text)
        st = g.stats()
        assert st["distinct"] == len(kept) and st["count_sum"] == sum(kept.values())
        keys = sorted(kept)
        assert np.array_equal(g.getKmerCounts(encode_np(keys, k)), np.array([kept[x] for x in keys], dtype=np.uint64))
        g.close()
    # the minimizer exchange refuses a rule, in either order
    with pytest.raises(T.TSXException):
        T.TSXHashMapHIPGroup(ranks, 23, 0, k, devices=[0] * ranks, comm="copy", exchange="mini", acgt_only=True)
    g = T.TSXHashMapHIPGroup(ranks, 23, 0, k, devices=[0] * ranks, comm="copy", exchange="mini")
    with pytest.raises(T.TSXException):
        g.set_base_rule(min_qual_char="5")
    g.close()
    # the sharded entry points refuse a table with a rule (as a canonical one), and answer "not supported"
    m = T.TSXHashMapHIP(20, 0, k, acgt_only=True)
    L, sz = T.lib(), T.ctypes.c_size_t(0)
    assert L.tsx_hip_shard_send_capacity(m.handle, 1 << 20, T.ctypes.byref(sz)) == T.EINVAL
    assert L.tsx_hip_shard_desc_capacity(m.handle, 1 << 20, 0, T.ctypes.byref(sz)) == T.EINVAL
    assert L.tsx_hip_mini_capacity(m.handle, 1 << 20, 2, T.ctypes.byref(sz)) == T.EINVAL
    assert L.tsx_hip_shard_l1_supported(m.handle) == 0 and L.tsx_hip_mini_supported(m.handle) == 0
    assert b"base rule" in L.tsx_hip_last_error()
    m.set_base_rule()
    assert L.tsx_hip_shard_desc_capacity(m.handle, 1 << 20, 0, T.ctypes.byref(sz)) == T.OK
    # FASTA with a quality rule: EINVAL from the count and the query calls
    m.set_record_lines(2)
    L.tsx_hip_set_base_rule(m.handle, 0, 53)
    fasta = b">a\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n"
    assert L.tsx_hip_count_fastq_host(m.handle, fasta, len(fasta)) == T.EINVAL
    assert b"FASTA" in L.tsx_hip_last_error()
    with pytest.raises(T.TSXException):
        m.queryReads(fasta)
    m.close()


def run_cli(*args, timeout=600):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.gpu
def test_cli_output_and_histo(T, tmp_path):
    k = 21
    text = edited_text(901, 300, k)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(text)
    kept, _ = oracle(text, k, True, "5")
    assert len(kept) > 1000
    want_h = Counter(min(c, 10001) for c in kept.values())   # (--histo-max 10000: one line for everything above)
    for extra in ([], ["--gpus=2", "--comm=copy", "--devices=0,0", "--exchange=merge"]):
        out, histo = tmp_path / "out.count", tmp_path / "out.histo"
        rc, so, se = run_cli("--input=%s" % fq, "--k=%d" % k, "--l=20", "--s=0", "--acgt-only", "--min-qual-char=5",
                             "--output=%s" % out, "--histo=%s" % histo, *extra)
        assert rc == 0, se
        assert "AcgtOnly=Yes" in se and "MinQualChar=5" in se
        got = {}
        for line in out.read_text().splitlines():
            a, b = line.split("\t")
            got[a.encode()] = int(b)
        assert got == dict(kept)
        h = {}
        for line in histo.read_text().splitlines():
            a, b = line.split("\t")
            h[int(a)] = int(b)
        assert {c: n for c, n in h.items() if n} == dict(want_h)
