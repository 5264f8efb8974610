"""Read trimming: the kept span of every record (tsx_hip_trim_spans_*) and the records cut to it (tsx_hip_trim_reads_*),
through the C ABI, Python and the tsxCount CLI.

Expectations come from a Python restatement only: a Counter over the counted text (bytes through base_code, strands
folded for canonical tables), the window rule of the table's base rule, then runs, span and output bytes as
include/tsxcount_hip.h states them.  Never from the library under test.  Spans and bytes are compared exactly."""
import ctypes
import gzip
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from test_read_query import _CODE, U64, coded_counts, line_spans, rc, run_cli

K = 21
ACGT = b"ACGTacgt"


def solid_flags(seq, qual, counts, k, lower, upper, canonical, acgt_only, minq):
    s = seq.translate(_CODE)
    out = []
    for i in range(len(s) - k + 1):
        ok = True
        if acgt_only and any(b not in ACGT for b in seq[i:i + k]):
            ok = False
        if minq and any(j >= len(qual) or qual[j] < minq for j in range(i, i + k)):
            ok = False
        x = s[i:i + k]
        c = counts.get(min(x, rc(x)) if canonical else x, 0)
        out.append(ok and lower <= c <= upper)
    return out


def pick_span(flags, k, mode):
    runs, i = [], 0
    while i < len(flags):
        if flags[i]:
            j = i
            while j + 1 < len(flags) and flags[j + 1]:
                j += 1
            runs.append((i, j - i + k))
            i = j + 1
        else:
            i += 1
    if mode == "prefix":
        runs = [r for r in runs if r[0] == 0]
    if not runs:
        return (0, 0)
    best = max(r[1] for r in runs)
    return next(r for r in runs if r[1] == best)   # the leftmost among equals


def expected_trim(query, counts, k, lpr, lower=1, upper=U64, mode="longest", min_len=0, canonical=False, acgt_only=False,
                  minq=0):
    """(spans, output bytes, totals) of a text."""
    sp = line_spans(query)
    spans, out, kept, bases_in, bases_kept = [], b"", 0, 0, 0
    for i in range(0, len(sp), lpr):
        grp = [query[a:b] for a, b in sp[i:i + lpr]]
        seq = grp[1] if len(grp) > 1 else b""
        qual = grp[3] if len(grp) > 3 else b""
        start, length = pick_span(solid_flags(seq, qual, counts, k, lower, upper, canonical, acgt_only, minq), k, mode)
        spans.append((start, length))
        bases_in += len(seq)
        if length > 0 and length >= (min_len or k):
            kept += 1
            bases_kept += length
            out += grp[0] + b"\n" + seq[start:start + length] + b"\n"
            if lpr == 4 and len(grp) > 2:
                out += grp[2] + b"\n"
            if lpr == 4 and len(grp) > 3:
                out += qual[min(start, len(qual)):min(start + length, len(qual))] + b"\n"
    return spans, out, dict(records=len(spans), kept=kept, bases_in=bases_in, bases_kept=bases_kept, bytes=len(out))


def as_pairs(sp):
    return [(int(a), int(b)) for a, b in sp]


def sub(read, positions):
    r = bytearray(read)
    for p in positions:
        r[p] = b"CGTA"[b"ACGT".index(r[p])]
    return bytes(r)


def fastq(seqs, pad=0):
    return b"".join(b"@r%d%s\n%s\n+\n%s\n" % (i, b"x" * (pad if i == 0 else 0), s, b"I" * len(s)) for i, s in enumerate(seqs))


def fasta(seqs, pad=0):
    return b"".join(b">r%d%s\n%s\n" % (i, b"x" * (pad if i == 0 else 0), s) for i, s in enumerate(seqs))


_rnd = random.Random(20250)
GENOME = bytes(_rnd.choice(b"ACGT") for _ in range(20000))
COUNTED = b">g\n" + GENOME + b"\n"
COUNTS = coded_counts(COUNTED, K, 2)
# substitutions of a 150-base read: none, base 0, base 149, the middle, two at distance < k, = k and > k
PLANTS = ([], [0], [149], [75], [60, 70], [60, 60 + K], [40, 100], [20, 21, 130], [10, 139])


def planted_reads(rnd, copies=1):
    seqs = []
    for _ in range(copies):
        for pl in PLANTS:
            at = rnd.randrange(0, len(GENOME) - 151)
            seqs.append(sub(GENOME[at:at + 150], pl))
        at = rnd.randrange(0, len(GENOME) - 151)
        seqs.append(sub(GENOME[at:at + 151], [75]))                       # a tie: 55 solid windows on either side
        seqs.append(GENOME[at:at + 15])                                   # shorter than k
        seqs.append(bytes(rnd.choice(b"ACGT") for _ in range(150)))       # no solid window
        seqs.append(GENOME[at:at + 150])                                  # all solid
    return seqs


def closed_fd(tmp_path):
    fd = os.open(str(tmp_path / "closed"), os.O_WRONLY | os.O_CREAT, 0o644)
    os.close(fd)
    return fd


def write_out(m, text, tmp_path, **kw):
    p = str(tmp_path / "trim.out")
    tot = m.trimReads(text, p, **kw)
    return open(p, "rb").read(), tot


# ---- CPU --------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("tsx_hip_trim_spans_device", "tsx_hip_trim_spans_host", "tsx_hip_trim_reads_device", "tsx_hip_trim_reads_host")


def test_trim_symbols_declared_and_exported():
    import tsxcount_amd as T
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    for name in ("tsx_hip_trim_rule", "tsx_hip_trim_span", "tsx_hip_trim_totals", "TSX_HIP_TRIM_LONGEST", "TSX_HIP_TRIM_PREFIX"):
        assert name in hdr, name
    assert ctypes.sizeof(T.TrimRule) == 32 and T.TRIM_SPAN_DTYPE.itemsize == 16 and ctypes.sizeof(T.TrimTotals) == 40


def test_trim_argument_checks_need_no_gpu():
    import tsxcount_amd as T
    with pytest.raises(ValueError):
        T.trim_rule(mode="shortest")
    with pytest.raises(ValueError):
        T.trim_rule(lower=5, upper=4)
    m = T.TSXHashMapHIP.__new__(T.TSXHashMapHIP)   # no table behind it: the checks come first
    with pytest.raises(ValueError):
        m.trimSpans(b"@a\nACGT\n", mode="suffix")
    with pytest.raises(ValueError):
        m.trimReads(b"@a\nACGT\n", 1, lower=3, upper=2)
    L = T.lib()
    rule = T.trim_rule()
    n = ctypes.c_size_t(7)
    assert L.tsx_hip_trim_spans_host(None, b"@a\nACGT\n", 8, ctypes.byref(rule), None, 0, ctypes.byref(n), 0) == T.EINVAL
    assert n.value == 0
    assert L.tsx_hip_trim_spans_device(None, None, 0, ctypes.byref(rule), None, 0, None, None) == T.EINVAL
    assert L.tsx_hip_trim_reads_host(None, b"", 0, ctypes.byref(rule), 1, 0, None) == T.EINVAL
    assert L.tsx_hip_trim_reads_device(None, None, 0, ctypes.byref(rule), None, 0, None, None) == T.EINVAL


def test_cli_refuses_trim_on_several_gpus(tmp_path):
    code, _, err = run_cli("--help", timeout=30)
    assert code == 1
    for flag in ("--trim=OUT", "--trim-spans=FILE", "--trim-input=FILE", "--trim-lower=N", "--trim-upper=N",
                 "--trim-mode=longest|prefix", "--trim-min-len=N"):
        assert flag in err, flag
    code, _, err = run_cli("--input=x.fastq", "--k=15", "--l=18", "--gpus=2", "--trim=" + str(tmp_path / "t.out"), timeout=30)
    assert code != 0 and "one GPU" in err
    assert not (tmp_path / "t.out").exists()
    code, _, err = run_cli("--input=x.fastq", "--trim=o", "--trim-mode=middle", timeout=30)
    assert code == 1 and "Usage" in err
    code, _, err = run_cli("--input=x.fa", "--format=fasta-wrapped", "--trim=o", timeout=30)
    assert code == 1 and "wrapped" in err


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def genome_map(T, k=K, l=18, counted=COUNTED, s=0, path=1, **kw):
    m = T.TSXHashMapHIP(l, s, k, **kw)
    m.set_path(path)
    m.set_record_lines(2)
    m.countFastq(counted)
    return m


@pytest.fixture(scope="module")
def gmap(T):
    m = genome_map(T)
    yield m
    m.close()


def check_text(m, text, lpr, tmp_path, counts=COUNTS, k=K, modes=("longest", "prefix"), chunks=(0,), **kw):
    """Spans, bytes and totals of every mode and piece size against the restatement; returns the spans of modes[0]."""
    m.set_record_lines(lpr)
    first = None
    for mode in modes:
        spans, out, tot = expected_trim(text, counts, k, lpr, mode=mode, **kw)
        first = spans if first is None else first
        lib_kw = dict(lower=kw.get("lower", 1), upper=None if kw.get("upper", U64) == U64 else kw["upper"], mode=mode)
        for chunk in chunks:
            assert as_pairs(m.trimSpans(text, chunk_bytes=chunk, **lib_kw)) == spans, (mode, chunk)
            got, gtot = write_out(m, text, tmp_path, min_len=kw.get("min_len", 0), chunk_bytes=chunk, **lib_kw)
            assert got == out, (mode, chunk)
            assert gtot == tot, (mode, chunk)
    return first


@pytest.mark.gpu
@pytest.mark.parametrize("lpr", [4, 2])
def test_planted_errors(T, gmap, lpr, tmp_path):
    seqs = planted_reads(random.Random(11))
    text = (fastq if lpr == 4 else fasta)(seqs)
    want, _, _ = expected_trim(text, COUNTS, K, lpr)
    n = len(PLANTS)
    assert want[0] == (0, 150) and want[1] == (1, 149) and want[2] == (0, 149) and want[3] == (0, 75)
    assert want[n] == (0, 75) and want[n + 1] == (0, 0) and want[n + 2] == (0, 0) and want[n + 3] == (0, 150)   # tie, short, none, all
    pre, _, _ = expected_trim(text, COUNTS, K, lpr, mode="prefix")
    assert pre[1] == (0, 0) and pre[3] == (0, 75)
    check_text(gmap, text, lpr, tmp_path)


@pytest.mark.gpu
def test_seams_of_words_rounds_tiles_and_workgroups(T, gmap, tmp_path):
    """The first header grows by 0..70 bytes: every run boundary of a 10 KiB text moves over every offset of a 64-position
    word, and with them the boundaries near the 2048-position rounds, the 4 KiB tiles and the workgroups."""
    seqs = planted_reads(random.Random(12), copies=3)
    for pad in range(71):
        text = fastq(seqs, pad)
        assert len(text) > 2 * 4096
        check_text(gmap, text, 4, tmp_path, modes=("longest",) if pad % 8 else ("longest", "prefix"))
    check_text(gmap, fasta(seqs, 33), 2, tmp_path)


@pytest.mark.gpu
def test_windows_and_pieces_equal_one_piece(T, gmap, tmp_path, monkeypatch):
    import torch
    seqs = planted_reads(random.Random(13), copies=7)
    text = fastq(seqs, 5)
    assert len(text) >= 5 * 4096 + 64
    gmap.set_record_lines(4)
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    for mode in ("longest", "prefix"):
        spans, out, tot = expected_trim(text, COUNTS, K, 4, mode=mode)
        rule = T.trim_rule(1, None, mode)
        for win in (None, "4096"):
            if win:
                monkeypatch.setenv("TSX_HIP_DEV_WINDOW", win)   # >= 5 windows
            else:
                monkeypatch.delenv("TSX_HIP_DEV_WINDOW", raising=False)
            dsp = torch.full((len(spans) + 3, 2), -1, dtype=torch.int64, device="cuda:0")
            assert gmap.trimSpansDevice(dev.data_ptr(), len(text), dsp.data_ptr(), len(spans) + 3, rule) == len(spans)
            got = dsp.cpu().numpy()
            assert [tuple(r) for r in got[:len(spans)].tolist()] == spans, (mode, win)
            assert (got[len(spans):] == 0).all()
            dout = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
            dtot = gmap.trimReadsDevice(dev.data_ptr(), len(text), dout.data_ptr(), len(text) + 64, rule)
            assert dtot == tot
            assert bytes(dout[:tot["bytes"]].cpu().numpy()) == out, (mode, win)
        monkeypatch.delenv("TSX_HIP_DEV_WINDOW", raising=False)
    check_text(gmap, text, 4, tmp_path, chunks=(0, 4000, 700))   # 4000: >= 5 pieces


@pytest.mark.gpu
def test_a_long_record(T, gmap, tmp_path):
    long = GENOME[3000:15000]
    bad = sub(long, [2000, 2500, 9000])
    text = b">clean\n" + long + b"\n>three\n" + bad + b"\n" + fasta([GENOME[100:250]])
    spans = check_text(gmap, text, 2, tmp_path, chunks=(0, 5000))
    assert spans[0] == (0, 12000) and spans[1] == (2501, 6499)   # more than 64 bitmap words; the longest run is the third
    want, _, _ = expected_trim(text, COUNTS, K, 2, mode="prefix")
    assert want[1] == (0, 2000)


def _line_texts():
    a, b, c, d, e = (GENOME[i:i + 90] for i in (500, 1500, 2500, 3500, 4500))
    a, c = sub(a, [30]), sub(c, [5, 80])
    body = (b"\n\n@a\n" + a + b"\n\n+\n" + b"I" * 90 + b"\n\n\n"
            b"@shortq\n" + b + b"\n+\n" + b"J" * 40 + b"\n"
            b"@longq\n" + c + b"\n+plus\n" + b"K" * 120 + b"\n\n"
            b"@crlf\r\n" + d + b"\r\n+\r\n" + b"L" * 90 + b"\r\n")
    return {"whole": body,
            "unterminated": body + b"@u\n" + sub(e, [60]) + b"\n+\n" + b"M" * 90,
            "incomplete": body + b"@tail\n" + sub(e, [10]) + b"\n",
            "incomplete_open": body + b"@tail\n" + sub(e, [10]),
            "header_only": body + b"@tail"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["whole", "unterminated", "incomplete", "incomplete_open", "header_only"])
def test_line_rules(T, gmap, name, tmp_path):
    text = _line_texts()[name]
    spans = check_text(gmap, text, 4, tmp_path, chunks=(0, 1, 150, 333))
    assert spans[0] == (31, 59) and spans[1] == (0, 90) and spans[2] == (6, 74)
    assert spans[3] == (0, 90)   # '\r' is a byte of the line: the windows that hold it are not solid, the rest is
    _, out, _ = expected_trim(text, COUNTS, K, 4)
    assert b"\n" + b"J" * 40 + b"\n" in out and b"\n" + b"K" * 74 + b"\n" in out and b"\n\n" not in out
    two = text.replace(b"\r", b"")
    check_text(gmap, b"\n".join(two.split(b"\n")[:5]) + b"\n>x\n" + GENOME[7000:7100], 2, tmp_path, chunks=(0, 64))


@pytest.mark.gpu
def test_canonical_table_reads_from_either_strand(T, tmp_path):
    counts = coded_counts(COUNTED, K, 2, canonical=True)
    m = genome_map(T, canonical=True)
    seqs = planted_reads(random.Random(14))
    text = fastq([rc(s) for s in seqs] + seqs[:4])
    spans = check_text(m, text, 4, tmp_path, counts=counts, canonical=True)
    assert spans[1] == (0, 149) and spans[2] == (1, 149)   # the plants at base 0 and base 149, seen from the other strand
    m.close()


@pytest.mark.gpu
def test_base_rules_break_runs(T, tmp_path):
    at = GENOME.index(b"A", 8070) - 70
    read = GENOME[at:at + 150]
    withn = read[:70] + b"N" + read[71:]      # N takes the code of A: solid throughout unless the rule drops the windows
    text = fastq([withn, read])
    m = genome_map(T, acgt_only=True)
    spans = check_text(m, text, 4, tmp_path, acgt_only=True)
    assert spans == [(71, 79), (0, 150)]
    m.close()
    m = genome_map(T)
    assert check_text(m, text, 4, tmp_path) == [(0, 150), (0, 150)]
    m.set_base_rule(min_qual_char="5")
    q = bytearray(b"I" * 150)
    q[50] = ord("#")
    text = b"@low\n" + read + b"\n+\n" + bytes(q) + b"\n" + fastq([read])
    assert check_text(m, text, 4, tmp_path, minq=ord("5"), chunks=(0, 400)) == [(51, 99), (0, 150)]
    m.close()


@pytest.mark.gpu
def test_upper_excludes_a_repeat(T, tmp_path):
    rep = GENOME[5000:5060]
    counted = COUNTED + fasta([rep] * 5)
    counts = coded_counts(counted, K, 2)
    m = genome_map(T, counted=counted)
    text = fastq([GENOME[4900:5050], GENOME[4990:5140], GENOME[6000:6150]])
    assert check_text(m, text, 4, tmp_path, counts=counts, upper=3) == [(0, 120), (50, 100), (0, 150)]
    assert check_text(m, text, 4, tmp_path, counts=counts, lower=2) == [(100, 50), (10, 60), (0, 0)]
    m.close()


@pytest.mark.gpu
def test_min_len_and_error_returns(T, gmap, tmp_path):
    import torch
    seqs = planted_reads(random.Random(15))
    text = fastq(seqs)
    spans, out, tot = expected_trim(text, COUNTS, K, 4, min_len=100)
    assert 0 < tot["kept"] < sum(1 for s in spans if s[1]) and tot["bases_kept"] < sum(s[1] for s in spans)
    check_text(gmap, text, 4, tmp_path, min_len=100, chunks=(0, 1000))
    check_text(gmap, text, 4, tmp_path, min_len=1)
    L, rule = T.lib(), T.trim_rule(1)
    n = ctypes.c_size_t(0)
    few = np.zeros(5, dtype=T.TRIM_SPAN_DTYPE)
    for chunk in (0, 600):
        few[:] = 0
        assert L.tsx_hip_trim_spans_host(gmap.handle, text, len(text), ctypes.byref(rule), few.ctypes.data_as(ctypes.c_void_p), 4,
                                         ctypes.byref(n), chunk) == T.ERANGE
        assert n.value == len(spans) and as_pairs(few[:4]) == spans[:4] and as_pairs(few[4:]) == [(0, 0)]
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    dsp = torch.zeros((5, 2), dtype=torch.int64, device="cuda:0")
    with pytest.raises(T.TSXException) as e:
        gmap.trimSpansDevice(dev.data_ptr(), len(text), dsp.data_ptr(), 4, rule)
    assert e.value.code == T.ERANGE
    assert [tuple(r) for r in dsp.cpu().tolist()] == spans[:4] + [(0, 0)]
    dout = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(T.TSXException) as e:
        gmap.trimReadsDevice(dev.data_ptr(), len(text), dout.data_ptr(), len(text) + 63, rule)
    assert e.value.code == T.ERANGE
    for bad in (T.TrimRule(3, 2, 0, 0, 0), T.TrimRule(1, U64, 0, 2, 0), T.TrimRule(1, U64, 0, 0, 1)):
        assert L.tsx_hip_trim_spans_host(gmap.handle, text, len(text), ctypes.byref(bad), few.ctypes.data_as(ctypes.c_void_p), 5,
                                         ctypes.byref(n), 0) == T.EINVAL
        assert L.tsx_hip_trim_reads_device(gmap.handle, dev.data_ptr(), len(text), ctypes.byref(bad), dout.data_ptr(),
                                           len(text) + 64, None, None) == T.EINVAL
    shard = T.TSXHashMapHIP(18, 0, K, shard_bits=1, shard_index=0)
    with pytest.raises(T.TSXException) as e:
        shard.trimSpans(text, lower=1)
    assert e.value.code == T.EINVAL
    tot_s = T.TrimTotals()
    assert L.tsx_hip_trim_reads_host(shard.handle, text, len(text), ctypes.byref(rule), 1, 0, ctypes.byref(tot_s)) == T.EINVAL
    shard.close()
    with pytest.raises(T.TSXException) as e:
        gmap.trimReads(text, closed_fd(tmp_path), lower=1)
    assert e.value.code == T.EIO


@pytest.mark.gpu
def test_calls_leave_the_owner_counters(T, gmap, tmp_path):
    import torch
    L = T.lib()
    L.tsx_hip_debug_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]

    def counters():
        out = (ctypes.c_uint64 * 8)()
        assert L.tsx_hip_debug_counters(gmap.handle, out) == 0
        return tuple(int(x) for x in out[:3])

    text = fastq(planted_reads(random.Random(16), copies=2))
    gmap.set_record_lines(4)
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    dsp = torch.zeros((64, 2), dtype=torch.int64, device="cuda:0")
    dout = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
    rule = T.trim_rule(1)

    def one_pass():
        gmap.trimSpans(text, lower=1, chunk_bytes=3000)
        gmap.trimReads(text, str(tmp_path / "o"), lower=1, chunk_bytes=3000)
        gmap.trimSpansDevice(dev.data_ptr(), len(text), dsp.data_ptr(), 64, rule)
        gmap.trimReadsDevice(dev.data_ptr(), len(text), dout.data_ptr(), len(text) + 64, rule)
        for call in (lambda: gmap.trimSpansDevice(dev.data_ptr(), len(text), dsp.data_ptr(), 3, rule),          # ERANGE
                     lambda: gmap.trimReadsDevice(dev.data_ptr(), len(text), dout.data_ptr(), 100, rule),       # ERANGE
                     lambda: gmap.trimReads(text, closed_fd(tmp_path), lower=1, chunk_bytes=3000)):             # EIO
            with pytest.raises(T.TSXException):
                call()

    one_pass()   # warm-up: the map's grow-only line scratch grows here
    warm = counters()
    one_pass()
    assert counters() == warm


@pytest.mark.gpu
def test_golden_cli_trim(T, tmp_path):
    k = 14
    inp = os.path.join(GOLDEN, "small_t7.1000.fastq")
    text = open(inp, "rb").read()
    counts = coded_counts(text, k, 4)
    with gzip.open(str(tmp_path / "q.fastq.gz"), "wb") as f:
        f.write(text)

    def trim_line(so):
        return [ln for ln in so.splitlines() if ln.startswith("trim\t")]

    for mode in ("longest", "prefix"):
        spans, data, tot = expected_trim(text, counts, k, 4, lower=2, mode=mode)
        assert 0 < tot["bases_kept"] < tot["bases_in"]
        line = "trim\t%d\t%d\t%d\t%d" % (tot["records"], tot["kept"], tot["bases_in"], tot["bases_kept"])
        for qin in (inp, str(tmp_path / "q.fastq.gz")):
            out, sp = tmp_path / "t.fq", tmp_path / "t.tsv"
            code, so, se = run_cli("--input=" + inp, "--k=14", "--l=20", "--trim=" + str(out), "--trim-spans=" + str(sp),
                                   "--trim-input=" + qin, "--trim-mode=" + mode)
            assert code == 0, so + se
            assert out.read_bytes() == data, (mode, qin)
            assert [tuple(int(v) for v in ln.split("\t")) for ln in sp.read_text().splitlines()] == \
                [(i,) + s for i, s in enumerate(spans)]
            assert trim_line(so) == [line]
    # the counted input is the trimmed one by default; a saved table trims without --input
    db = tmp_path / "t.kmerdb"
    _, data, tot = expected_trim(text, counts, k, 4, lower=3, min_len=40)
    line = "trim\t%d\t%d\t%d\t%d" % (tot["records"], tot["kept"], tot["bases_in"], tot["bases_kept"])
    code, so, se = run_cli("--input=" + inp, "--k=14", "--l=20", "--save=" + str(db), "--trim=" + str(tmp_path / "a.fq"),
                           "--trim-lower=3", "--trim-min-len=40")
    assert code == 0, so + se
    assert (tmp_path / "a.fq").read_bytes() == data and trim_line(so) == [line]
    code, so, se = run_cli("--load=" + str(db), "--trim=" + str(tmp_path / "b.fq"), "--trim-input=" + inp, "--trim-lower=3",
                           "--trim-min-len=40")
    assert code == 0, so + se
    assert (tmp_path / "b.fq").read_bytes() == data and trim_line(so) == [line]
