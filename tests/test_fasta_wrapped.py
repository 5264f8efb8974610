"""Wrapped (multi-line) FASTA on the GPU: the device transform byte for byte against join_fasta, and the tables of
countFasta / countFastaDevice / countFastaBgzf and the command line against a dictionary count of join_fasta(text) read as
two-line records (conftest.python_counts) and against the reference's recorded result for the golden reads.

Shapes are the smallest that cross each boundary of csrc/tsx_fasta.h: a lane is 16 bytes, a wave 1 KiB, a tile 4096 bytes,
a scan chunk 1024 tiles (4 MiB)."""
import ctypes
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN, python_counts
from test_fasta_wrapped_cpu import LITERALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
_CODE = bytes(b"ACGT"[((b >> 1) ^ (b >> 2)) & 3] for b in range(256))   # the stand-in code of every byte, as a base
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = frozenset(b"ACGTacgt")
TILE = 4096


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


# ---- texts and expectations --------------------------------------------------------------------------------------

def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def expected(T, text, k, canonical=False, acgt_only=False):
    """{coded k-mer: count} of the wrapped text: the dictionary count of its canonical two-line form."""
    out = Counter()
    for x, c in python_counts(T.join_fasta(text), k, 2).items():
        if acgt_only and any(b not in ACGT for b in x):
            continue
        y = x.translate(_CODE)
        if canonical:
            y = min(y, y[::-1].translate(_COMP))
        out[y] += c
    return out


def encode_np(keys, k):
    a = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, k)
    code = (((a >> 1) ^ (a >> 2)) & 3).astype(np.uint64)
    out = np.zeros((len(keys), (2 * k + 63) // 64), dtype=np.uint64)
    for i in range(k):
        out[:, i // 32] |= code[:, i] << np.uint64(2 * (i % 32))
    return out


def check_table(m, k, want):
    keys = sorted(want)
    st = m.stats()
    assert st["kmers_added"] == sum(want.values()) and st["distinct"] == len(want), (st, sum(want.values()), len(want))
    if keys:
        got = m.getKmerCounts(encode_np(keys, k))
        exp = np.array([want[x] for x in keys], dtype=np.uint64)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, [(keys[i], int(got[i]), int(exp[i])) for i in bad[:5]]


def records_text(seed, k, n_records=300, alphabet=b"ACGT", n_runs=False):
    """A few hundred records of 0 - 400 bases (k - 1, k and k + 1 among them), each wrapped at a width from 1 .. k - 1, 60 or
    80 -- every window of a record wrapped below k spans a break -- with blank lines and headers of all sorts between."""
    rng = random.Random(seed)
    parts = [wrap(rand_seq(rng, 2 * k, alphabet), 7)]                 # lines in front of the first header
    lens = [k - 1, k, k + 1, 0, 1, 400] + [rng.randrange(0, 401) for _ in range(n_records - 6)]
    widths = [1, k - 1, 60, 80]
    for i, n in enumerate(lens):
        seq = rand_seq(rng, n, alphabet)
        if n_runs and n > 40:                                         # runs of N and lower-case stretches
            a, b = sorted(rng.randrange(n) for _ in range(2))
            seq = seq[:a] + b"N" * min(b - a, rng.randrange(1, 30)) + seq[a:].lower()
            seq = seq[:n]
        w = widths[i % 4] if i < 8 else rng.choice([rng.randrange(1, k), 60, 80])
        parts.append(b">r%d %s\n" % (i, b"x" * rng.randrange(0, 40)) + wrap(seq, w) + b"\n" * rng.choice([0, 0, 0, 1, 3]))
    return b"".join(parts)


_cache = {}


def cached(T, key, make, k, **kw):
    if key not in _cache:
        text = make()
        _cache[key] = (text, expected(T, text, k, **kw))
    return _cache[key]


# ---- 1. the transform, byte for byte -----------------------------------------------------------------------------------

def boundary_text():
    rng = random.Random(5)
    t = bytearray()

    def rec(header, seq, width):
        t.extend(b">" + header + b"\n" + wrap(seq, width))

    def pad_to(target, mod=TILE):
        """A record whose header is sized so that the text is target (mod TILE) bytes long behind it."""
        fill = (target - len(t) - 2 - 11) % mod
        t.extend(b">" + b"p" * fill + b"\n" + b"ACGTACGTAC\n")
        assert len(t) % mod == target % mod

    for w in (1, 15, 16, 17, 60, 61, 80):
        rec(b"w%d" % w, rand_seq(rng, 5 * w + 3), w)
    for w in (4095, 4096, 4097):
        rec(b"w%d" % w, rand_seq(rng, 2 * w + 5), w)
    rec(b"one line of three tiles", rand_seq(rng, 3 * TILE + 77), 1 << 20)
    rec(b"h" * 5000, rand_seq(rng, 100), 60)                          # a header longer than a tile
    pad_to(TILE - 7)
    rec(b"ends!", rand_seq(rng, 50), 60)                              # a header whose '\n' is the last byte of a tile
    assert len(t) % TILE == 51 and t[len(t) - 51 - 1:len(t) - 51] == b"\n"
    pad_to(0)
    assert len(t) % TILE == 0 and t[-1:] == b"\n"
    rec(b"first byte of a tile, at a line start", rand_seq(rng, 70), 60)
    pad_to(TILE - 6)
    t.extend(b">x\nAAC>GGT\n")                                        # '>' first byte of a tile, not at a line start
    assert (len(t) - 5) % TILE == 0 and t[len(t) - 8:len(t) - 4] == b"AAC>"
    t.extend(b"\n\n\n>blank\n\n\nACGT\n\n\n\nTTGA\n\n>e1\n\n>e2\n\n\n")  # runs of newlines
    rec(b"last", rand_seq(rng, 333), 61)
    return bytes(t)


@pytest.mark.gpu
def test_unwrap_boundaries_byte_exact(T):
    text = boundary_text()
    assert len(text) > 8 * TILE
    for t in (text, text[:-1], text.rstrip(b"\n"), b"\n" * 5 + text, text[7:]):
        assert T.unwrap_fasta(t) == T.join_fasta(t)


@pytest.mark.gpu
@pytest.mark.parametrize("text,want", LITERALS)
def test_unwrap_literals(T, text, want):
    assert T.unwrap_fasta(text) == want


@pytest.mark.gpu
def test_unwrap_across_a_scan_chunk(T):
    """A little over 4 MiB (more than 1024 tiles) in 60-column lines: bytes, and the counters of countFasta against the
    two-line path on the joined text (no dictionary of it)."""
    rng = np.random.default_rng(11)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(4 << 20) + 300000)].tobytes()
    cuts = [0] + sorted(int(x) for x in rng.integers(1, len(bases), size=40)) + [len(bases)]
    text = b"".join(b">chr%d some words\n" % i + wrap(bases[a:b], 60) for i, (a, b) in enumerate(zip(cuts, cuts[1:])))
    assert len(text) > 1025 * TILE
    joined = T.join_fasta(text)
    assert T.unwrap_fasta(text) == joined
    stats = []
    for wrapped in (True, False):
        m = T.TSXHashMapHIP(24, 0, 31)
        if wrapped:
            m.countFasta(text)
        else:
            m.set_record_lines(2)
            m.countFastq(joined)
        st = m.stats()
        stats.append((st["kmers_added"], st["distinct"]))
        m.close()
    assert stats[0] == stats[1] and stats[0][0] == sum(max(0, b - a - 30) for a, b in zip(cuts, cuts[1:]))


# ---- 2. counts ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("k", [21, 31, 63, 127])
def test_counts(T, k, path):
    text, want = cached(T, ("plain", k), lambda: records_text(k, k), k)
    m = T.TSXHashMapHIP(20, 0, k)
    m.set_path(path)
    m.countFasta(text)
    check_table(m, k, want)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_counts_canonical(T, k):
    text, _ = cached(T, ("plain", k), lambda: records_text(k, k), k)
    want = expected(T, text, k, canonical=True)
    for path in (1, 2):
        m = T.TSXHashMapHIP(20, 0, k, canonical=True)
        m.set_path(path)
        m.countFasta(text)
        check_table(m, k, want)
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 63])
def test_counts_acgt_only(T, k):
    text = records_text(900 + k, k, alphabet=b"ACGTacgt", n_runs=True)
    want, every = expected(T, text, k, acgt_only=True), expected(T, text, k)
    assert 0 < sum(want.values()) < sum(every.values())
    for path in (1, 2):
        m = T.TSXHashMapHIP(20, 0, k, acgt_only=True)
        m.set_path(path)
        m.countFasta(text)
        check_table(m, k, want)
        m.close()


@pytest.mark.gpu
def test_record_lines_setting_is_left_alone(T):
    """The wrapped entry points count two-line records under either setting, and the setting still holds afterwards."""
    k = 21
    text, want = cached(T, ("plain", k), lambda: records_text(k, k), k)
    fq = b"@r\nACGTACGTACGTACGTACGTACGTA\n+\nIIIIIIIIIIIIIIIIIIIIIIIII\n"
    m = T.TSXHashMapHIP(20, 0, k)          # 4 lines per record
    m.countFasta(text)
    check_table(m, k, want)
    m.clear()
    m.countFastq(fq)
    assert m.stats()["kmers_added"] == 5   # still FASTQ: the quality line is not a sequence
    m.close()


# ---- 3. seams ----------------------------------------------------------------------------------------------------------

def seam_text(seed, k, mod):
    """Records placed so that multiples of `mod` (piece or window seams) fall inside a header, directly after its '>',
    directly after its newline, between a newline and a '>', and inside sequence lines; one record spans three pieces."""
    rng = random.Random(seed)
    t = bytearray()

    def pad_to(target):
        fill = (target - len(t) - 2 - 11) % mod
        t.extend(b">" + b"p" * fill + b"\n" + b"ACGTACGTAC\n")

    def rec(header, n, width=60):
        t.extend(b">" + header + b"\n" + wrap(rand_seq(rng, n), width))

    rec(b"first", 2 * k + 9)
    pad_to(mod - 20); rec(b"h" * 60, 3 * k)                # a seam inside a header
    pad_to(mod - 1); rec(b"after the >", 3 * k)            # ... directly after its '>'
    pad_to(mod - 6); rec(b"abcd", 3 * k)                   # ... directly after its '\n' (6 = len(">abcd\n"))
    pad_to(mod); rec(b"at a line start", 3 * k)            # ... between a '\n' and the '>'
    rec(b"three pieces", 3 * mod + 100)                    # a record across at least three pieces
    rec(b"one long line", 2 * mod + 50, 1 << 20)
    pad_to(mod - 3); t.extend(b">e\n>f\n"); rec(b"g", k + 1, 5)
    text = bytes(t)
    seams = range(mod, len(text), mod)
    assert any(text[s - 1:s] == b">" and text[s - 2:s - 1] == b"\n" for s in seams)
    assert any(text[s - 1:s] == b"\n" and text.rfind(b"\n", 0, s - 1) + 1 < s - 1 and text[text.rfind(b"\n", 0, s - 1) + 1:][:1] == b">" for s in seams)
    assert any(text[s - 1:s] == b"\n" and text[s:s + 1] == b">" for s in seams)
    assert any(text[text.rfind(b"\n", 0, s) + 1:][:1] == b">" and text[s - 1:s] not in (b">", b"\n") for s in seams)
    return text


def long_header_text(seed, k):
    """200-byte headers and 60-column lines: most 256-byte pieces add fewer than k - 1 bases to the open record, many none."""
    rng = random.Random(seed)
    return b"".join(b">" + b"h" * 199 + b"\n" + wrap(rand_seq(rng, rng.randrange(100, 500)), 60) for _ in range(40))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 127])
def test_seams_host_pieces(T, k, monkeypatch):
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "256")
    texts = [seam_text(3 + k, k, 256), records_text(40 + k, k, n_records=60)]
    if k == 127:
        texts.append(long_header_text(9, k))
    for text in texts:
        want = expected(T, text, k)
        for path in (1, 2):
            m = T.TSXHashMapHIP(20, 0, k)
            m.set_path(path)
            m.countFasta(text)
            check_table(m, k, want)
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 127])
def test_seams_device_windows(T, k, monkeypatch):
    import torch
    monkeypatch.setenv("TSX_HIP_DEV_WINDOW", "4096")
    for text in (seam_text(5 + k, k, 4096), b"".join(long_header_text(s, k) for s in range(3))):
        assert len(text) > 3 * 4096
        want = expected(T, text, k)
        d_text = torch.frombuffer(bytearray(text + b"\n" * 64), dtype=torch.uint8).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        for path in (1, 2):
            m = T.TSXHashMapHIP(20, 0, k)
            m.set_path(path)
            m.countFastaDevice(d_text.data_ptr(), len(text))
            m.sync()
            check_table(m, k, want)
            m.close()


# ---- 4. golden ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_golden_reads_as_wrapped_fasta(T, golden_fastq, golden_counts):
    """The reads of the golden FASTQ as FASTA wrapped at 60 columns: the joined sequences are the reads, so the table is the
    reference's recorded one."""
    lines = [l for l in golden_fastq.split(b"\n") if l]
    text = b"".join(b">" + h[1:] + b"\n" + wrap(s, 60) for h, s in zip(lines[0::4], lines[1::4]))
    m = T.TSXHashMapHIP(20, 4, 14)
    m.countFasta(text)
    st = m.stats()
    assert st["kmers_added"] == sum(golden_counts.values()) and st["distinct"] == len(golden_counts)
    kmers = T.encode_many(list(golden_counts.keys()), 14)
    assert np.array_equal(m.getKmerCounts(kmers), np.array(list(golden_counts.values()), dtype=np.uint64))
    m.close()


# ---- 5. BGZF -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_bgzf_batches(T, monkeypatch):
    k = 31
    rng = random.Random(77)
    text = b"".join(b">contig%d len=%d\n" % (i, n) + wrap(rand_seq(rng, n), 70)
                    for i, n in enumerate(rng.randrange(10, 30000) for _ in range(27)))
    assert len(text) > 3 * 131072
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "131072")
    z = T.bgzf_compress(text, level=1)
    want = expected(T, text, k)
    m = T.TSXHashMapHIP(21, 0, k)
    m.countFastaBgzf(z)
    check_table(m, k, want)
    with pytest.raises(T.TSXException) as e:
        m.countFastaBgzf(b"not a gzip file at all")
    assert e.value.code == T.EINVAL
    m.close()


# ---- 6. the command line -----------------------------------------------------------------------------------------------

def run_cli(*args):
    p = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.gpu
def test_cli(T, tmp_path):
    k = 21
    rng = random.Random(8)
    contam = [rand_seq(rng, n) for n in (500, 90, 20, 700)]
    text = b"".join(b">c%d\n" % i + wrap(s, 60) for i, s in enumerate(contam))
    want = expected(T, text, k)
    fa = tmp_path / "contam.fa"
    fa.write_bytes(text)
    (tmp_path / ("contam.fa.%d.count" % k)).write_bytes(b"".join(x + b"\t%d\n" % c for x, c in want.items()))
    out = tmp_path / "out.count"
    rc, so, se = run_cli("--input=%s" % fa, "--format=fasta-wrapped", "--k=%d" % k, "--l=18", "--output=%s" % out, "--check")
    assert rc == 0, (so, se)
    assert "Format=FASTA (wrapped, lines joined)" in se and "total errors0" in so
    got = dict(l.split(b"\t") for l in out.read_bytes().splitlines())
    assert {x: int(c) for x, c in got.items()} == dict(want)
    # without the option the file name means two-line FASTA, as before: no k-mer across a line break
    rc, so, se = run_cli("--input=%s" % fa, "--k=%d" % k, "--l=18")
    assert rc == 0 and "Format=FASTA (2 lines per record)" in se
    # the screening example: reads that share k-mers with the contaminants, from a FASTQ --filter-input
    reads = [contam[0][100:250], rand_seq(rng, 150), contam[3][400:550], rand_seq(rng, 150)]
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads)))
    hits = tmp_path / "hits.fastq"
    rc, so, se = run_cli("--input=%s" % fa, "--format=fasta-wrapped", "--k=%d" % k, "--l=18", "--filter=%s" % hits,
                         "--filter-input=%s" % fq, "--filter-lower=1", "--filter-fraction=0.5")
    assert rc == 0, (so, se)
    kept = [l for l in hits.read_bytes().split(b"\n") if l][0::4]
    assert kept == [b"@r0", b"@r2"]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(T):
    text = b">a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\nACGT\n"
    m = T.TSXHashMapHIP(18, 0, 21, shard_bits=1, shard_index=0)
    with pytest.raises(T.TSXException) as e:
        m.countFasta(text)
    assert e.value.code == T.EINVAL and "shard_bits" in str(e.value)
    m.close()
    m = T.TSXHashMapHIP(18, 0, 21, min_qual_char="5")
    for call in (lambda: m.countFasta(text), lambda: m.countFastaBgzf(T.bgzf_compress(text))):
        with pytest.raises(T.TSXException) as e:
            call()
        assert e.value.code == T.EINVAL and "min_qual_char" in str(e.value)
    assert m.stats()["kmers_added"] == 0
    m.close()
    # a buffer too small for the two-line form: ERANGE, and the size it needs
    form = T.join_fasta(text)
    L, got = T.lib(), ctypes.c_size_t(0)
    small = ctypes.create_string_buffer(len(form) - 1)
    assert L.tsx_hip_unwrap_fasta_host(0, text, len(text), small, len(form) - 1, ctypes.byref(got)) == T.ERANGE
    assert got.value == len(form)
    exact = ctypes.create_string_buffer(len(form))
    assert L.tsx_hip_unwrap_fasta_host(0, text, len(text), exact, len(form), ctypes.byref(got)) == T.OK
    assert exact.raw == form and got.value == len(form)
