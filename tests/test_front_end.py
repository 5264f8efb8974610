"""Every text kernel sees the same windows.

The kernels that walk a text tile by tile share one front end (csrc/tsx_kernels.h: tile_load, tile_stage, window_valid,
run_leader) and, three of them, one lookup schedule (csrc/tsx_query.h).  The other tests check each kernel against its
own oracle; this one checks that five calls, each through a kernel of its own, agree on ONE number -- how many windows
of a text are k-mers -- for texts whose line ends, windows and text ends fall on the first and second tile seam (bytes
4096 and 8192):

    count on the atomic path (count_fastq_kernel)    stats()["kmers_added"]
    sketchKmers (sketch_windows_kernel)              totals["kmers"]
    prefilter (prefilter_windows_kernel)             prefilter_stats["seen"]
    queryReads (query_reads_kernel)                  the sum of kmers over the records
    countProfile (window_counts_kernel)              the entries that are not TSX_HIP_NO_KMER

The yardstick is the oracle's count_fastq total (oracle/tsx_oracle.c).  The C oracle knows no base rule: under acgt_only
the yardstick is a run count over the sequence lines of test_base_rule.records, which is first checked against the C
oracle on the same text with the rule off.  A window may reach 126 bytes into the halo at most (k = 127 from a tile's last
byte), so "the last byte of the halo" is read as: the window that starts at a tile's last byte is the last of its line.
"""
import random

import numpy as np
import pytest

from test_base_rule import ACGT, records
from test_prefilter import to_device
from test_read_query import random_seqs

TILE = 4096
KS = (31, 32, 33, 64, 65, 127)
NO_KMER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def record(name, seq, lpr):
    if lpr == 2:
        return b">" + name + b"\n" + seq + b"\n"
    return b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"


def text_with(rnd, lpr, marks, tail=b""):
    """Records of 100-base reads, and for every (p, kind) of marks one record of 300 bases whose name is as long as it
    takes to put the '\n' of its sequence line (kind "seq") or of its last line ("rec") at byte p; then tail."""
    out = bytearray()
    for p, kind in marks:
        seq = random_seqs(rnd, 1, 300, 300)[0]
        fixed = len(record(b"", seq, lpr)) if kind == "rec" else 2 + len(seq) + 1   # bytes up to and with that '\n'
        while p + 1 - len(out) - fixed > 500:
            out += record(b"r%d" % len(out), random_seqs(rnd, 1, 100, 100)[0], lpr)
        name = b"x" * (p + 1 - len(out) - fixed)
        out += record(name, seq, lpr)
        nl = len(out) - 1 if kind == "rec" else len(out) - len(record(name, seq, lpr)) + 2 + len(name) + len(seq)
        assert nl == p and out[p] == 0x0A, (p, kind, nl)
    return bytes(out) + tail


def texts(k, lpr):
    """{name: text}, every text under 3 tiles."""
    rnd = random.Random(100 * k + lpr)
    open_rec = lambda n: (b">" if lpr == 2 else b"@") + b"u\n" + random_seqs(rnd, 1, n, n)[0]   # no '\n' at the end
    out = {
        # a sequence line's end as the last byte of tile 0 and as the first byte of tile 2
        "line_end_at_seams": text_with(rnd, lpr, [(TILE - 1, "seq"), (2 * TILE, "seq")]),
        # the window at a tile's last byte is the last of its line; the window at the next tile's last byte needs one more
        "window_in_halo": text_with(rnd, lpr, [(TILE - 1 + k, "seq"), (2 * TILE - 2 + k, "seq")]),
        # an empty line between records: its '\n' is the first byte of tile 1, the record's own the last byte of tile 0;
        # a sequence line over the second seam for the planted N
        "empty_line": text_with(rnd, lpr, [(TILE - 1, "rec")]) + b"\n" +
                      text_with(rnd, lpr, [(TILE + 50 - 1, "seq")], tail=b"\n\n" + record(b"last", b"ACGT" * 40, lpr)),
        "shorter_than_k": record(b"s", b"ACGTACGTAC", lpr)[:k - 1],
    }
    assert out["empty_line"][TILE - 1:TILE + 1] == b"\n\n" and out["empty_line"][2 * TILE - 3] in ACGT
    for d in (-1, 0, 1):   # an unterminated sequence line that ends 1 byte before the end of tile 0, at it, 1 byte after
        head = text_with(rnd, lpr, [(TILE - 400, "rec")])
        out["open_end%+d" % d] = head + open_rec(TILE + d - len(head) - 3)
        assert len(out["open_end%+d" % d]) == TILE + d
    assert all(len(t) < 3 * TILE for t in out.values())
    return out


def plant_n(text, lpr):
    """The text with an N three bases before the first seam that has a sequence line there (none: the text as it is)."""
    pos, seq_at = 0, set()
    kept = 0
    for l in text.split(b"\n"):
        if l:
            if kept % lpr == 1:
                seq_at.update(range(pos, pos + len(l)))
            kept += 1
        pos += len(l) + 1
    for seam in (TILE, 2 * TILE):
        if seam - 3 in seq_at:
            return text[:seam - 3] + b"N" + text[seam - 2:]
    return text


def oracle_total(text, k, lpr):
    from oracle.oracle import Oracle
    o = Oracle(k, 16, 4, seed=1)
    try:
        return o.count_fastq(text, lpr)
    finally:
        o.close()


def run_total(text, k, lpr, acgt_only):
    """Windows of k bytes inside the sequence lines (under acgt_only: of ACGTacgt alone)."""
    total = 0
    for seq, _, _ in records(text, lpr):
        run = 0
        for b in seq:
            run = run + 1 if (b in ACGT or not acgt_only) else 0
            total += run >= k
    return total


def five_totals(m, text):
    m.clear()
    m.countFastq(text)
    count = m.stats()["kmers_added"]
    sketch = m.sketchKmers(text, precision=10)[1]["kmers"]
    m.prefilter(text, bits=12)
    seen = m.prefilter_stats["seen"]
    m.freePrefilter()
    query = int(m.queryReads(text)["kmers"].sum())
    profile = int((m.countProfile(text) != NO_KMER).sum())
    return {"count": count, "sketch": sketch, "prefilter": seen, "query": query, "profile": profile}


def cases(k):
    for lpr in (4, 2):
        for name, text in texts(k, lpr).items():
            want = oracle_total(text, k, lpr)
            assert want == run_total(text, k, lpr, False), (name, lpr)   # the two yardsticks agree where both apply
            yield lpr, False, name, text, want
            with_n = plant_n(text, lpr)
            assert (with_n != text) == (name != "shorter_than_k"), name
            assert oracle_total(with_n, k, lpr) == run_total(with_n, k, lpr, False)
            yield lpr, True, name, with_n, run_total(with_n, k, lpr, True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_every_text_kernel_sees_the_same_windows(T, k):
    m = T.TSXHashMapHIP(16, 0, k)
    m.set_path("atomic")
    seen = 0
    try:
        for lpr, acgt_only, name, text, want in cases(k):
            seen += want
            m.set_record_lines(lpr)
            m.set_base_rule(acgt_only=acgt_only)
            got = five_totals(m, text)
            print(k, lpr, acgt_only, name, want, got)
            assert set(got.values()) == {want}, (k, lpr, acgt_only, name, want, got)
        assert seen > 0
    finally:
        m.close()


@pytest.mark.gpu
def test_pieces_and_device_windows_of_one_tile(T, monkeypatch):
    """One case again in host pieces of 4 096 bytes (a piece that starts inside a line: head_open = 1) and, for the
    device calls, in windows of 4 096 bytes (the byte before the window is read: head_open < 0)."""
    import torch
    k, lpr = 33, 4
    text = plant_n(texts(k, lpr)["window_in_halo"], lpr)
    want = run_total(text, k, lpr, True)
    assert want > 0
    monkeypatch.setenv("TSX_HIP_PIECE_BYTES", "4096")            # (read when a map is created)
    monkeypatch.setenv("TSX_HIP_DEV_WINDOW", "4096")
    m = T.TSXHashMapHIP(16, 0, k)
    m.set_path("atomic")
    m.set_base_rule(acgt_only=True)
    try:
        got = five_totals(m, text)
        assert set(got.values()) == {want}, (want, got)
        dev = to_device(text)
        nrec = len(records(text, lpr))
        m.clear()
        m.countFastqDevice(dev.data_ptr(), len(text))
        m.sync()
        got = {"count": m.stats()["kmers_added"]}
        regs = torch.zeros(1 << 10, dtype=torch.int32, device="cuda:0")
        totals = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        m.sketchKmersDevice(dev.data_ptr(), len(text), regs.data_ptr(), precision=10, totals_ptr=totals.data_ptr())
        m.prefilterDevice(dev.data_ptr(), len(text), bits=12)
        stats = torch.zeros((nrec + 3) * 4, dtype=torch.int64, device="cuda:0")
        profile = torch.zeros(len(text), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert m.queryReadsDevice(dev.data_ptr(), len(text), stats.data_ptr(), nrec + 3) == nrec
        m.countProfileDevice(dev.data_ptr(), len(text), profile.data_ptr())
        m.sync()
        got["prefilter"] = m.prefilter_stats["seen"]
        got["sketch"] = int(totals.cpu()[0])
        got["query"] = int(stats.cpu().numpy().view(np.uint64).reshape(-1, 4)[:nrec, 0].sum())
        got["profile"] = int((profile.cpu().numpy().view(np.uint32) != NO_KMER).sum())
        assert set(got.values()) == {want}, (want, got)
    finally:
        m.close()
