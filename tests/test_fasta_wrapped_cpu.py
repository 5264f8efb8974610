"""Wrapped (multi-line) FASTA without a GPU: join_fasta -- the CPU statement of the record rules -- against hand-written
literals, the command line's refusals, and the new symbols of the C ABI."""
import os
import re
import subprocess

import pytest

import tsxcount_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")
NEW_SYMBOLS = ["tsx_hip_count_fasta_host", "tsx_hip_count_fasta_device", "tsx_hip_count_fasta_bgzf_host", "tsx_hip_unwrap_fasta_host"]

# (wrapped text, its canonical two-line form): one case per record rule
LITERALS = [
    (b"", b""),                                                                 # an empty text
    (b"\n\n\n", b""),
    (b">a\n>b\n>c\n", b""),                                                     # a text that holds only headers
    (b">a", b""),
    (b">a\nACGT\nTTGA\n", b">\nACGTTTGA\n"),                                    # the lines of a record are joined
    (b">a\nACGT\nTTGA", b">\nACGTTTGA\n"),                                      # no trailing newline
    (b"ACGT\nGG\n>a\nTT\n", b">\nACGTGG\n>\nTT\n"),                             # leading headerless lines: a record of their own
    (b"\n\nACGT", b">\nACGT\n"),
    (b">a\nAC\n>empty\n>b\nGT\n", b">\nAC\n>\nGT\n"),                           # an empty record in the middle
    (b">a\nAC\n>empty\n", b">\nAC\n"),                                          # ... and at the end
    (b">a\nAC\n>empty", b">\nAC\n"),
    (b">a\nAC\n\n\nGT\n\n>b\n\nTT\n", b">\nACGT\n>\nTT\n"),                     # blank lines inside a sequence
    (b">a\nAC>GT\nA>\n>b\nT\n", b">\nAC>GTA>\n>\nT\n"),                         # a '>' inside a line is an ordinary byte
    (b">a b c\nAC\r\nGT\r\n", b">\nAC\rGT\r\n"),                                # '\r' gets no special treatment
    (b">a\nA\n>b\nC\n>c\nG\n>d\nT\n", b">\nA\n>\nC\n>\nG\n>\nT\n"),             # width 1
    (b">>\n>\nA\n", b">\nA\n"),                                                 # headers that are only '>'
    (b">a\nNNNN\nnnnn\n", b">\nNNNNnnnn\n"),
]


@pytest.mark.parametrize("text,want", LITERALS)
def test_join_fasta_literals(text, want):
    got = T.join_fasta(text)
    assert got == want
    assert len(got) <= len(text) + 2
    assert T.join_fasta(got) == got          # the canonical form is a fixed point


def test_join_fasta_gives_two_line_records():
    """Read as two-line records (empty lines dropped, every second line a sequence) the form gives the joined sequences."""
    text = b"AC\n>r1 x\nACGT\nAC\n\n>r2\n>r3\nTTTT\nT"
    form = T.join_fasta(text)
    lines = [l for l in form.split(b"\n") if l]
    assert lines[0::2] == [b">"] * 3 and lines[1::2] == [b"AC", b"ACGTAC", b"TTTTT"]


@pytest.mark.parametrize("args,msg", [
    (["--input=x.fa", "--format=fasta-wrapped", "--gpus=2"], "--format=fasta-wrapped runs on one GPU only"),
    (["--input=x.fa", "--format=fasta-wrapped", "--min-qual-char=5"], "--min-qual-char needs FASTQ"),
    (["--input=x.fa", "--format=fasta-wrapped", "--filter=out.fa"], "--filter and --read-stats do not read wrapped FASTA"),
    (["--input=x.fa", "--format=fasta-wrapped", "--read-stats=out.tsv"], "--filter and --read-stats do not read wrapped FASTA"),
    (["--input=x.fa", "--format=fasta-wrapped", "--filter=out.fa", "--filter-input=x.fa"], "--filter and --read-stats do not read wrapped FASTA"),
])
def test_cli_refusals(args, msg):
    """Refused before any device is touched (the input does not even exist), with the exit code of the other conflicts."""
    p = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    conflict = subprocess.run([EXE, "--input=x.fasta", "--format=fasta", "--min-qual-char=5"], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, timeout=60)
    assert msg in p.stderr.decode(), p.stderr.decode()
    assert p.returncode == conflict.returncode != 0
    assert "Creating TSXHashMap" not in p.stderr.decode()


def test_cli_usage_lists_the_format():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert "--format=fastq|fasta|fasta-wrapped" in p.stderr.decode()


def test_new_symbols_declared_and_exported():
    L = T.lib()
    hdr = open(T.HEADER_PATH).read()
    out = subprocess.run(["nm", "-D", "--defined-only", T.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
    # no map, no text: EINVAL, nothing dereferenced
    assert L.tsx_hip_count_fasta_host(None, b"", 0) == T.EINVAL
    assert L.tsx_hip_count_fasta_device(None, None, 0, None) == T.EINVAL
    assert L.tsx_hip_count_fasta_bgzf_host(None, None, 0) == T.EINVAL
    assert L.tsx_hip_unwrap_fasta_host(0, b"", 0, None, 0, None) == T.EINVAL


def test_bindings_exist():
    for name in ("countFasta", "countFastaBgzf", "countFastaDevice"):
        assert callable(getattr(T.TSXHashMapHIP, name))
        assert not hasattr(T.TSXHashMapHIPGroup, name)
    assert callable(T.unwrap_fasta) and callable(T.join_fasta)
