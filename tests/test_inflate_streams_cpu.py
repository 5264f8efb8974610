"""The expectations of test_inflate_streams.py, fixed without a GPU: every crafted deflate stream (tests/deflate_writer.py,
tests/inflate_cases.py) means to zlib's decoder exactly what the writer meant, every malformed one is refused by zlib (or,
where only the trailer is wrong, by gzip), and the host's BGZF member index (bgzf_index) reads headers as it should."""
import gzip
import struct
import zlib

import pytest

import inflate_cases as C
from deflate_writer import EOF_MEMBER, bgzf_file, bgzf_member


def agree_with_zlib(cases):
    for c in cases:
        assert zlib.decompress(c.raw, -15) == c.text, c.name
    image = bgzf_file([C.member_of(c) for c in cases])
    assert gzip.decompress(image) == b"".join(c.text for c in cases)


@pytest.mark.parametrize("kind", ["fixed", "dynamic"])
def test_writer_match_matrix(kind):
    cases = C.match_matrix(kind)
    assert len(cases) == 112 * 16 * 10 + 2          # (dist, p) pairs x lengths x tails, and the two far members
    agree_with_zlib(cases)


def test_writer_match_runs_and_block_ends():
    agree_with_zlib(C.match_runs())
    agree_with_zlib(C.block_end_runs())


def test_writer_code_shapes():
    cases = C.code_shapes()
    agree_with_zlib(cases)
    by_name = {c.name: c for c in cases}
    hclen = lambda raw: 4 + ((int.from_bytes(raw[:3], "little") >> 13) & 15)
    assert hclen(by_name["literal code of 1..15 bits, HCLEN 19"].raw) == 19
    assert hclen(by_name["HCLEN 5, the smallest of a valid block"].raw) == 5
    for kind in ("fixed", "dynamic"):               # 284 + 31 and 285 are two spellings of the same 258 bytes
        a, b = by_name[kind + " length 258 as symbol 284 + 31"], [c for c in cases if c.name.startswith(kind + " length 258 as symbol 285")][0]
        assert a.raw != b.raw and zlib.decompress(a.raw, -15) == zlib.decompress(b.raw, -15) == b"A" * 259 + b"B"
    assert sorted(int(c.name[-1]) for c in cases if c.name.startswith("a stored block of length 0")) == list(range(8))


@pytest.mark.parametrize("kind", ["stored", "fixed", "dynamic"])
def test_writer_member_sizes(kind):
    cases = C.member_sizes(kind)
    assert [len(c.text) for c in cases] == list(range(131)) + [65535, 65536]
    agree_with_zlib(cases)


@pytest.mark.parametrize("size", [700, 4000, 65280])
def test_encoder_cases_are_what_zlib_reads(size):
    agree_with_zlib(C.encoder_cases(size, C.encoder_texts()))


def test_malformed_cases_are_malformed():
    bad = C.malformed()
    assert len({b.reason for b in bad}) == 8            # every status of the kernel but "ok"
    for b in bad:
        image = bgzf_file([C.bad_member(b)])
        if b.crc is None and b.isize is None:
            with pytest.raises(zlib.error):
                zlib.decompress(b.raw, -15)
        else:                                           # a good stream, a wrong trailer
            assert zlib.decompress(b.raw, -15) == b.text, b.name
        with pytest.raises((zlib.error, OSError, EOFError)):
            gzip.decompress(image)


# ---- the host's member index ----------------------------------------------------------------------------------------

TEXT = b"@r\nACGT\n+\nIIII\n" * 40
_C = zlib.compressobj(6, zlib.DEFLATED, -15)
RAW = _C.compress(TEXT) + _C.flush()
SUB_A, SUB_B = b"XY" + struct.pack("<H", 3) + b"abc", b"ZZ" + struct.pack("<H", 1) + b"q"


def index(image):
    import tsxcount_amd as T
    return T.bgzf_index(image)


def test_index_other_subfields_around_bc():
    image = bgzf_file([bgzf_member(RAW, TEXT, before=SUB_A, after=SUB_B)])
    assert gzip.decompress(image) == TEXT
    assert index(image) == (2, len(TEXT))


def test_index_xlen_larger_than_its_subfields():
    """Three bytes behind the last subfield, too few for another one: every gzip reader skips XLEN bytes and so does the
    index.  The same for a last subfield whose length runs past XLEN."""
    image = bgzf_file([bgzf_member(RAW, TEXT, after=b"\0\0\0")])
    assert gzip.decompress(image) == TEXT
    assert index(image) == (2, len(TEXT))
    assert index(bgzf_file([bgzf_member(RAW, TEXT, after=b"QQ" + struct.pack("<H", 500) + b"z")])) == (2, len(TEXT))
    assert index(bgzf_file([bgzf_member(RAW, TEXT, before=b"QQ" + struct.pack("<H", 500))])) is None   # BC inside it: not found


def test_index_isize_limit():
    assert index(bgzf_file([bgzf_member(RAW, TEXT, isize=65536)])) == (2, 65536)
    assert index(bgzf_file([bgzf_member(RAW, TEXT, isize=65537)])) is None


@pytest.mark.parametrize("flag", [2, 8, 16])
def test_index_refuses_fhcrc_fname_fcomment(flag):
    assert index(bgzf_file([bgzf_member(RAW, TEXT, flags=4 | flag)])) is None


def test_index_bsize_out_of_range():
    total = 18 + len(RAW) + 8
    assert index(bgzf_file([bgzf_member(RAW, TEXT, bsize=total + len(EOF_MEMBER))])) is None     # one byte past the end
    assert index(bgzf_member(RAW, TEXT, bsize=total)) is None                                    # the same without an EOF member
    assert index(bgzf_file([bgzf_member(RAW, TEXT, bsize=18 + 8 - 2)])) is None                  # less than header + trailer
    assert index(bgzf_file([bgzf_member(RAW, TEXT, before=SUB_A, bsize=18 + 8 - 1)])) is None    # ... of THIS header
    assert index(bgzf_file([bgzf_member(RAW, TEXT, bsize=total - 1)])) == (2, len(TEXT))


def test_index_only_the_eof_member():
    assert index(EOF_MEMBER) == (1, 0)


def test_index_empty_members_between_data_members():
    one, empty = bgzf_member(RAW, TEXT), bgzf_member(b"\x03\x00", b"")
    image = bgzf_file([empty, one, empty, empty, one, empty])
    assert gzip.decompress(image) == TEXT * 2
    assert index(image) == (7, 2 * len(TEXT))
