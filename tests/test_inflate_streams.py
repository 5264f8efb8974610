"""The device inflate (tsxcount_amd/csrc/tsx_inflate.h) on deflate streams that zlib's encoder with its default settings
never writes: crafted members from tests/deflate_writer.py (tests/inflate_cases.py holds the families) and zlib's other
strategies, memory levels and flushes.  The expectation is always zlib's DECODER on the same compressed bytes, byte for
byte; test_inflate_streams_cpu.py shows without a GPU that this is also what the writer meant.

The cases of a family are the members of one BGZF image: a lane takes a member, so a wave sits in 64 unrelated streams
and a launch costs about what its longest member costs.  The comparison is member by member and names the case."""
import random
import re
import zlib
from functools import lru_cache

import numpy as np
import pytest

import inflate_cases as C
from deflate_writer import bgzf_file, bgzf_member

EMPTY = bgzf_member(b"\x03\x00", b"")


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def reference(cases):
    """(names, what zlib's decoder reads from each stream, the members with the trailer of that text)."""
    want = [zlib.decompress(c.raw, -15) for c in cases]
    return [c.name for c in cases], want, [bgzf_member(c.raw, w) for c, w in zip(cases, want)]


def check(T, ref, order=None, between=()):
    """Inflate the members (in `order`, `between` behind each) as one image and compare member by member."""
    names, want, members = ref
    order = range(len(members)) if order is None else order
    parts, index = [], []                    # index: the member of the image -> the case
    for i in order:
        parts.append(members[i]); index.append(i)
        for e in between:
            parts.append(e); index.append(None)
    try:
        got = T.bgzf_inflate(bgzf_file(parts))
    except T.TSXException as e:
        m = re.match(r"BGZF member (\d+): ", str(e))
        who = index[int(m.group(1))] if m and int(m.group(1)) < len(index) else None
        pytest.fail("%s -- %s" % (e, "an empty member in between" if who is None else names[who]))
    if got == b"".join(want[i] for i in order):
        return
    wrong, at = [], 0
    for i in order:
        if got[at:at + len(want[i])] != want[i]:
            w, g = want[i], got[at:at + len(want[i])]
            first = next(j for j in range(len(w)) if j >= len(g) or g[j] != w[j])
            wrong.append("%s: byte %d of %d" % (names[i], first, len(w)))
        at += len(want[i])
    pytest.fail("%d of %d members differ from zlib: %s" % (len(wrong), len(names), "; ".join(wrong[:8])))


@lru_cache(maxsize=None)
def matrix(kind):
    return reference(C.match_matrix(kind))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fixed", "dynamic"])
def test_match_matrix(T, kind):
    """One match between literals, over distance x length x position x what is left of the member: the pattern stores of
    distances below 8, the 32-byte step and its remainder, the 8-byte step and its landing store (distances 8..31 read
    what the step before stored), the byte loop in the first 8 and the last 64 or 8 bytes; distances up to 32768."""
    check(T, matrix(kind))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fixed", "dynamic"])
def test_neighbours_do_not_matter(T, kind):
    """The same members in another order, and with an empty member between every two: a store that runs past its
    member, or a lane that depends on the lanes beside it, changes somebody's bytes."""
    ref = matrix(kind)
    order = list(range(len(ref[0])))
    random.Random(11).shuffle(order)
    check(T, ref, order)
    check(T, ref, None, (EMPTY,))


@pytest.mark.gpu
def test_match_after_match_and_literal_runs(T):
    check(T, reference(C.match_runs()))
    check(T, reference(C.block_end_runs()))


@pytest.mark.gpu
def test_code_shapes(T):
    cases = C.code_shapes()
    check(T, reference(cases))
    both = [zlib.decompress(c.raw, -15) for c in cases if "length 258 as symbol" in c.name]
    assert len(both) == 4 and set(both) == {b"A" * 259 + b"B"}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stored", "fixed", "dynamic"])
def test_member_sizes(T, kind):
    """Sizes 0..130, 65535 and 65536: the CRC's 32-byte steps, the prefetch of the 32 behind them, the byte tail, and the
    byte-wise end of the literal store."""
    check(T, reference(C.member_sizes(kind)))


@lru_cache(maxsize=None)
def encoder_texts():
    return C.encoder_texts()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [700, 4000, 65280])
def test_zlibs_other_encoders(T, size):
    """Every strategy x memLevel 1, 8, 9 x level 1, 6, 9 of zlib's encoder (memLevel 1: many blocks per member; Z_FIXED,
    Z_RLE, Z_HUFFMAN_ONLY: codes and matches the default never picks), and sync and full flushes inside a member."""
    check(T, reference(C.encoder_cases(size, encoder_texts())))


def same_table(a, b):
    sa, sb = a.stats(), b.stats()
    assert sa["kmers_added"] == sb["kmers_added"] > 0 and sa["distinct"] == sb["distinct"]
    ka, ca = a.getAllKmers()
    assert np.array_equal(b.getKmerCounts(ka), ca)


@pytest.mark.gpu
def test_empty_members_and_batch_seams_through_the_count(T, monkeypatch):
    """Members of 1..5000 bytes, crafted three-block members among them, and runs of 1, 2 and 70 empty members in the
    middle of the file, inflated and counted in the smallest batches (128 KiB of text)."""
    from tsxcount_amd import synth
    from test_fasta_wrapped import records_text
    monkeypatch.setenv("TSX_HIP_BGZF_BATCH", "1")
    k = 21
    text = synth.fastq(31, 0, 175)
    members = C.irregular_members(text, 5)
    assert 300000 < len(text) < 400000 and sum(m == EMPTY for m in members) == 73
    z = bgzf_file(members)
    assert T.bgzf_index(z) == (len(members) + 1, len(text))
    assert T.bgzf_inflate(z) == text
    a, b = T.TSXHashMapHIP(21, 0, k), T.TSXHashMapHIP(21, 0, k)
    a.countFastq(text)
    b.countFastqBgzf(z)
    same_table(a, b)
    a.close(); b.close()
    fasta = records_text(77, k, n_records=1500)
    assert len(fasta) > 2 * (128 << 10)
    z = bgzf_file(C.irregular_members(fasta, 6))
    assert T.bgzf_inflate(z) == fasta
    a, b = T.TSXHashMapHIP(21, 0, k), T.TSXHashMapHIP(21, 0, k)
    a.countFasta(fasta)
    b.countFastaBgzf(z)
    same_table(a, b)
    a.close(); b.close()


@pytest.mark.gpu
def test_refusals(T):
    """One minimal member per way the kernel refuses a stream (inflate_cases.malformed).  Alone, and as member 70 of 131, in
    the middle of the second wave, where 63 lanes decode on while one leaves: the message names the member and the
    reason; without it the image inflates; afterwards the match matrix still does."""
    names, want, members = reference(C.member_sizes("fixed")[1:131])
    assert len(members) == 130
    for b in C.malformed():
        bad = C.bad_member(b)
        with pytest.raises(T.TSXException) as e:
            T.bgzf_inflate(bgzf_file([bad]))
        assert str(e.value) == "BGZF member 0: " + b.reason, b.name
        with pytest.raises(T.TSXException) as e:
            T.bgzf_inflate(bgzf_file(members[:70] + [bad] + members[70:]))
        assert str(e.value) == "BGZF member 70: " + b.reason, b.name
        assert T.bgzf_inflate(bgzf_file(members)) == b"".join(want), b.name
    m = T.TSXHashMapHIP(18, 0, 21)
    for count in (m.countFastqBgzf, m.countFastaBgzf):       # the counting entry points say the same
        with pytest.raises(T.TSXException) as e:
            count(bgzf_file(members[:70] + [C.bad_member(C.malformed()[-1])] + members[70:]))
        assert str(e.value) == "BGZF member 70: " + C.CRC
    m.close()
    check(T, matrix("fixed"))
