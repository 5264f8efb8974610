#!/usr/bin/env python3
"""Regenerates tests/golden/cli_refusals.json and tests/golden/cli_usage.txt:

    python tests/golden/make_cli_refusals.py tsxcount_amd/bin/tsxCount

Every command line of CASES ends in main() before a table is created, so the binary needs no GPU: an option the
parser turns down, a combination the refusals turn down, a database header that cannot be read or does not match, or
an input --l=auto cannot read.  For each one the argument list, the exit status, stdout and stderr are recorded.  The
usage block is pinned once, verbatim, in cli_usage.txt (from --help); in the recorded stderr it is the token {USAGE}.
Paths are written with two placeholders, {GOLDEN} (this directory) and {TMP} (where write_fixtures put the database
headers); tests/test_cli_refusals_cpu.py substitutes them both ways.
"""
import json
import os
import subprocess
import sys
import tempfile

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(GOLDEN))
from kmerdb import pack_header  # noqa: E402

USAGE_FILE = os.path.join(GOLDEN, "cli_usage.txt")
CASES_FILE = os.path.join(GOLDEN, "cli_refusals.json")

FQ = "--input={GOLDEN}/small_t7.1000.fastq"
DB = "--load={GOLDEN}/small_t7.first8.k14.v1.db"          # k=14, plain counting mode
WITH = "--with={GOLDEN}/small_t7.first8.k14.v1.db"
WRAPPED = "--format=fasta-wrapped"
O = "{TMP}/out"                                            # an output no case lives long enough to write
U64 = 2 ** 64


def write_fixtures(tmp):
    """Database headers the mismatch and read refusals need (a header is all main() reads before the GPU)."""
    def put(name, data):
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(data)
    put("plain.db", pack_header(k=14, l=20, F=8, C=4))
    put("k15.db", pack_header(k=15, l=18, F=12, C=6, seed=99))
    put("canon.db", pack_header(k=14, l=20, F=8, C=4, canonical=1))
    put("acgt.db", pack_header(k=14, l=20, F=8, C=4, acgt=1))
    put("minq.db", pack_header(k=14, l=20, F=8, C=4, minq=ord("5")))
    put("all.db", pack_header(k=14, l=20, F=8, C=4, canonical=1, acgt=1, minq=ord("I")))
    put("short.db", pack_header(k=14, l=20, F=8, C=4)[:40])
    bad = bytearray(pack_header(k=14, l=20, F=8, C=4))
    bad[124] ^= 0x10                                       # the header's own checksum no longer holds
    put("badsum.db", bytes(bad))
    put("notadb.db", b"@read\nACGT\n+\nIIII\n" * 16)       # long enough, wrong magic


def strict_cases():
    """The strict number options: each bound and its neighbour, an empty value, trailing junk, a leading '-', a value
    above 2^64 (some copies refuse the saturated value, some take it), and what strtoull skips in front."""
    out = []

    def both(opt, values):
        out.extend([["%s=%s" % (opt, v)] for v in values])
    odd = ["", "12x", "x", "-3", "-0", str(U64), str(U64 * 10), "+5", " 5", "5 ", "0x10", " -%d" % (U64 - 5)]
    for opt in ("--joint-max-a", "--joint-max-b", "--het-max"):
        both(opt, ["1", "4094", "0", "4095", str(U64 - 1)] + odd)
    for opt in ("--het-lower", "--het-upper", "--bin-min-hits", "--normalize-cutoff"):
        both(opt, ["0", "1", str(U64 - 1)] + odd)
    both("--normalize-round", ["1", "0", "00", str(U64 - 1)] + odd)
    both("--prefilter-bits", ["12", "38", "11", "39", "", "13x", "x", "-13", "-0", str(2 ** 63), str(U64), "+13", " 13",
                              "13 ", "0x10", " -%d" % (U64 - 13)])
    both("--bin-ratio", ["1", "1000", "1.000", "1000.000", "1000.0009", "1000.001", "0.999", "0", "1001", "", ".5", "1.",
                         "1.5x", "-2", "1e2", "2.5", "99999999999999999999"])
    return out


PARSER = [
    [], ["--help"], ["--help=me"], ["--bogus"], ["--bogus=1", "--help"], ["-k=5"], ["--"], ["--=3"], ["--k"], ["--kk=3"],
    ["word"], ["word", "input=x"], ["word", "--bogus"], ["--check=anything"], ["--check=anything", DB],
    ["--min-count=3"], ["--min-count="], ["--min-count"], ["--min-count=02"], ["--min-count=1"], ["--min-count=two"],
    ["--min-count=3", "--bogus"], ["--bogus", "--min-count=3"],
    ["--save="], ["--save"], ["--load="], ["--load"], ["--load=a,,b"], ["--load=,a"], ["--load=a,"], ["--with="],
    ["--with=x,"], ["--op="], ["--op"], ["--joint-histo="], ["--bin-a="], ["--bin-b="], ["--bin-ambiguous="],
    ["--bin-none="], ["--bin-input="], ["--bin-stats="], ["--het-histo="], ["--het-pairs="], ["--filter="],
    ["--read-medians="], ["--normalize="], ["--trim="], ["--trim-spans="], ["--read-stats="], ["--read-stats"],
    ["--min-qual-char="], ["--min-qual-char=ab"], ["--min-qual-char"], ["--min-qual-char=5"],
    ["--joint-format=dense"], ["--joint-format="], ["--joint-format=matrix"], ["--het-format=dense"],
    ["--het-format=sparse"], ["--het-mode=some"], ["--het-mode=all"], ["--het-mode=ALL"],
]

REFUSALS = [
    # digital normalization
    ["--normalize-cutoff=5"], ["--normalize-round=7", FQ], ["--normalize=" + O], [FQ, "--normalize=" + O, "--check"],
    [FQ, "--normalize=" + O, "--gpus=2"], [FQ, "--normalize=" + O, "--min-count=2"], [FQ, "--normalize=" + O, "--l=auto"],
    [FQ, "--normalize=" + O, "--estimate"], [FQ, "--normalize=" + O, WRAPPED], [FQ, "--normalize=" + O, "--filter-interleaved"],
    [FQ, "--normalize=" + O, "--trim-interleaved"], [FQ, "--normalize=" + O, "--filter-input=a,b"],
    [FQ, "--normalize=" + O, "--trim-input=a,b"], ["--input=a,b", "--normalize=" + O],
    # table sizing
    ["--estimate", FQ], ["--l=auto"], ["--estimate", "--k=14"], ["--l=20", "--l=auto"], ["--l=auto", FQ, "--gpus=2"],
    ["--estimate", "--k=14", FQ, "--gpus=3"], ["--l=auto", FQ, DB], ["--l=auto", FQ, WITH], ["--l=auto", FQ, WRAPPED],
    ["--l=auto", FQ, "--load-factor=0.95"], ["--l=auto", FQ, "--load-factor=0"], ["--l=auto", FQ, "--load-factor=abc"],
    ["--estimate", "--k=14", FQ, "--load-factor=1"], ["--l=auto", FQ, "--load-factor=nan"],
    ["--l=auto", "--input={TMP}/missing.fastq"], ["--estimate", "--k=21", "--input={TMP}/missing.fastq.gz"],
    ["--l=auto", "--input={TMP}/missing.fa", "--canonical", "--acgt-only", "--load-factor=0.9"],
    # the two-pass count
    ["--min-count=2"], [FQ, "--min-count=2", "--gpus=2"], [FQ, "--min-count=2", WRAPPED], [FQ, "--min-count=2", "--check"],
    [FQ, "--min-count=2", DB], [FQ, "--min-count=2", "--l=auto"], [FQ, "--min-count=2", "--estimate", "--k=14"],
    [FQ, "--prefilter-bits=20"], [FQ, "--prefilter-bits=20", "--min-count=1"], [FQ, "--min-count=2", "--min-count=1", "--prefilter-bits=12"],
    # --load headers
    ["--load={TMP}/missing.db"], ["--load={TMP}/short.db"], ["--load={TMP}/badsum.db"], ["--load={TMP}/notadb.db"],
    ["--load={TMP}"], ["--load={TMP}/k15.db", "--k=14"], ["--load={TMP}/canon.db"], ["--load={TMP}/acgt.db"],
    ["--load={TMP}/minq.db"], ["--load={TMP}/all.db"], ["--load={TMP}/plain.db", "--canonical"],
    ["--load={TMP}/plain.db", "--acgt-only"], ["--load={TMP}/plain.db", "--min-qual-char=5"],
    ["--load={TMP}/minq.db", "--min-qual-char=6"], ["--load={TMP}/plain.db,{TMP}/k15.db"],
    ["--load={TMP}/plain.db,{TMP}/missing.db"], ["--load={TMP}/k15.db,{TMP}/plain.db"],
    ["--load={TMP}/k15.db", "--mode=CAS"], ["--load={TMP}/k15.db", "--mode=CAS", "--l=9", "--s=3", "--seed=5"],
    ["--load={TMP}/all.db", "--canonical", "--acgt-only", "--min-qual-char=I", "--mode=serial", "--save=" + O],
    # set operations, joint spectrum, het pairs, binning: what the options alone tell
    [DB, WITH, "--op=bogus"], [DB, WITH, "--op=union", "--op-count=avg"], [DB, "--op-count="], [DB, "--op=union"],
    [DB, "--compare"], [DB, "--joint-histo=" + O], [DB, "--joint-max-a=5"], [DB, "--joint-format=sparse"],
    [DB, WITH, "--compare", "--joint-format=matrix"], [DB, WITH, "--compare", "--joint-max-b=7"], [DB, "--het-max=5"],
    [DB, "--het-format=matrix"], [DB, "--het-mode=all"], [DB, "--het-lower=2"], [DB, "--het-upper=2"],
    [FQ, "--het-histo=" + O, "--gpus=2"], [FQ, "--het-pairs=" + O, "--gpus=4"],
    [DB, "--het-histo=" + O, "--het-lower=5", "--het-upper=4"], [DB, WITH, "--joint-histo=" + O, "--gpus=2"],
    [DB, "--bin-a=" + O], [FQ, "--bin-stats=" + O], [FQ, "--bin-min-hits=2"], [DB, WITH, "--compare", "--bin-input=" + O],
    [DB, WITH, "--compare", "--bin-ratio=2"], [DB, WITH, "--compare", "--bin-min-hits=3"], [DB, WITH, "--bin-a=" + O, "--gpus=2"],
    [DB, WITH, "--bin-b=" + O, "--bin-input=a,b"], [FQ, WRAPPED, WITH, "--bin-none=" + O],
    [FQ, WRAPPED, WITH, "--bin-ambiguous=" + O, "--bin-input={GOLDEN}/small_t7.1000.fastq"], [DB, WITH, "--bin-stats=" + O],
    [DB, WITH], [FQ, WITH], [DB, WITH, "--compare", "--gpus=2"], [DB, WITH, "--compare", "--a-lower=5", "--a-upper=4"],
    [DB, WITH, "--compare", "--b-lower=9", "--b-upper=3"], [DB, WITH, "--compare", "--a-lower=0", "--a-upper=0"],
    [FQ, "--b-upper=0"], [FQ, "--a-upper=abc"],
    # --with headers
    [DB, "--with={TMP}/missing.db", "--compare"], [DB, "--with={TMP}/short.db", "--compare"],
    [DB, "--with={TMP}/badsum.db", "--op=union"], [DB, "--with={TMP}/k15.db", "--compare"],
    [DB, "--with={TMP}/canon.db", "--compare"], [DB, "--with={TMP}/acgt.db", "--compare"],
    [DB, "--with={TMP}/minq.db", "--compare"], [DB, "--with={TMP}/all.db", "--compare"],
    [DB, "--with={TMP}/plain.db,{TMP}/k15.db", "--compare"], [DB, "--with={TMP}/plain.db,{TMP}/missing.db", "--compare"],
    ["--load={TMP}/canon.db", "--canonical", "--with={TMP}/plain.db", "--compare"],
    ["--load={TMP}/all.db", "--canonical", "--acgt-only", "--min-qual-char=I", "--with={TMP}/minq.db", "--compare"],
    [FQ, "--k=15", "--with={TMP}/plain.db", "--op=subtract"], [FQ, "--acgt-only", WITH, "--compare"],
    # behind the banner
    [FQ, "--mode=CAS"], [FQ, "--mode=cas", "--check", "--canonical", "--acgt-only", "--min-qual-char=5", "--threads=3"],
    [FQ, "--mode="], [DB, WITH, "--op=diff", "--op-count=sum", "--save=" + O, "--mode=omp"], [FQ, "--l=auto", "--mode=TSX"],
    [FQ, "--estimate", "--k=9", "--mode=TSX"], [FQ, "--k=abc", "--l=-3", "--s=1x", "--threads=z", "--mode=x"],
    [FQ, "--exchange=ring"], [FQ, "--exchange="], [FQ, "--lower=5", "--upper=4"], [FQ, "--lower=5", "--upper=abc"],
    [FQ, "--histo-max=0"], [FQ, "--histo-max=4294967297"], [FQ, "--histo-max=x"],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini"], [FQ, "--gpus=2", "--acgt-only", "--exchange=mini"],
    [FQ, "--gpus=2", "--min-qual-char=5", "--exchange=mini"],
    ["--input={TMP}/x.fa", "--min-qual-char=5"], ["--input={TMP}/x.fasta.gz", "--min-qual-char=5"],
    ["--input={TMP}/x.fna", "--min-qual-char=5"], [FQ, "--format=fasta", "--min-qual-char=5"],
    [FQ, "--filter=" + O, "--filter-median-lower=2", "--filter-lower=3"], [FQ, "--filter=" + O, "--filter-median-upper=2", "--filter-fraction=0.5"],
    [FQ, "--filter-median-lower=2"], [FQ, "--filter=" + O, "--filter-median-lower=5", "--filter-median-upper=4"],
    [FQ, "--read-medians=" + O, "--filter-interleaved"], [FQ, "--read-medians=" + O, "--filter-input=a,b"],
    [FQ, "--read-medians=" + O, "--gpus=2"], [FQ, WRAPPED, "--read-medians=" + O],
    [FQ, WRAPPED, "--filter=" + O, "--filter-median-lower=1", "--filter-input={GOLDEN}/small_t7.1000.fastq"],
    [FQ, WRAPPED, "--gpus=2"], [FQ, WRAPPED, "--min-qual-char=5"], [FQ, WRAPPED, "--filter=" + O], [FQ, WRAPPED, "--read-stats=" + O],
    [FQ, WRAPPED, "--read-stats=" + O, "--filter-input={GOLDEN}/small_t7.1000.fastq"], [FQ, WRAPPED, "--trim=" + O],
    [FQ, WRAPPED, "--trim-spans=" + O, "--trim-input={GOLDEN}/small_t7.1000.fastq"],
    [FQ, "--filter-pairs=all"], [FQ, "--filter-pairs="],
    # paired reads: the filter's form, then the trim's
    [FQ, "--read-stats=" + O, "--filter-interleaved"], [FQ, "--filter-interleaved"], [FQ, "--filter-input=a,b"],
    [FQ, "--filter-interleaved", "--filter-input=a"], [FQ, "--filter-input=a,b", "--filter=" + O],
    [FQ, "--filter-input=a,b,c", "--filter=o1,o2"], [FQ, "--filter-input=a,b", "--filter=o1,o2", "--filter-singles=s"],
    [FQ, "--filter-interleaved", "--filter-input=a", "--filter=o1,o2"],
    [FQ, "--filter-interleaved", "--filter-input=a", "--filter=o", "--filter-singles=s1,s2"],
    [FQ, "--filter-input=a,", "--filter=o1,o2"], [FQ, "--filter-input=a,b", "--filter=,o2"],
    [FQ, "--filter-input=a,b", "--filter=o1,o2", "--gpus=2"], [FQ, "--filter-singles=s"],
    ["--input={TMP}/w.fa", WRAPPED, "--filter-input={TMP}/w.fa,b", "--filter=o1,o2"],
    [FQ, "--trim-spans=" + O, "--trim-interleaved"], [FQ, "--trim-interleaved"], [FQ, "--trim-input=a,b"],
    [FQ, "--trim-input=a,b", "--trim=" + O], [FQ, "--trim-input=a,b", "--trim=o1,o2", "--trim-singles=s"],
    [FQ, "--trim-interleaved", "--trim-input=a", "--trim=o1,o2"], [FQ, "--trim-input=a,b", "--trim=o1,", "--trim-singles=s1,s2"],
    [FQ, "--trim-input=a,b", "--trim=o1,o2", "--gpus=2"], [FQ, "--trim-singles=s"],
    ["--input={TMP}/w.fa", WRAPPED, "--trim-input=b,{TMP}/w.fa", "--trim=o1,o2"],
    # the rest of the list
    [FQ, "--gpus=0"], [FQ, "--gpus=-1"], [FQ, "--gpus=abc"], [FQ, "--comm=mpi"], [FQ, "--comm="],
    [FQ, "--devices=0", "--gpus=2"], [FQ, "--devices=0,1"], [FQ, "--devices=0,1,", "--gpus=3"], [FQ, "--devices=,", "--gpus=2"],
    [FQ, "--filter-lower=5", "--filter-upper=4"], [FQ, "--filter-fraction=2"], [FQ, "--filter-fraction=-0.1"],
    [FQ, "--filter-fraction=nan"], [FQ, "--filter=" + O, "--gpus=2"], [FQ, "--read-stats=" + O, "--gpus=2"],
    [FQ, "--trim-lower=5", "--trim-upper=4"], [FQ, "--trim-mode=suffix"], [FQ, "--trim-mode="],
    [FQ, "--trim=" + O, "--gpus=2"], [FQ, "--trim-spans=" + O, "--gpus=2"], [DB, "--trim=" + O], [DB, "--trim-spans=" + O],
    [FQ, "--save=" + O, "--gpus=2"], [DB, "--gpus=2"], [FQ, DB, "--check"], [DB, "--filter=" + O], [DB, "--read-stats=" + O],
    [DB, "--read-medians=" + O], [FQ, "--het-histo=" + O], [DB, "--het-pairs=" + O], [FQ, "--k=16", "--het-histo=" + O, "--het-max=9"],
]

# Two refusals apply: which one speaks.  (A refusal before the "Running with parameters" banner leaves stdout empty.)
ORDER = [
    ["--normalize-cutoff=5", "--bogus"], ["--prefilter-bits=20"], ["--l=auto", "--min-count=2"],
    [FQ, "--normalize=" + O, "--check", "--min-count=2"], [FQ, "--normalize=" + O, "--l=auto", "--gpus=2"],
    [FQ, "--l=auto", "--gpus=2", "--min-count=2"], [FQ, "--min-count=2", "--gpus=2", "--load={TMP}/missing.db"],
    [FQ, "--prefilter-bits=20", "--load={TMP}/missing.db"], ["--load={TMP}/missing.db", "--op=bogus"],
    ["--load={TMP}/k15.db", "--k=14", "--op=bogus"], ["--load={TMP}/k15.db,{TMP}/missing.db", "--k=14"],
    [DB, "--op=bogus", "--compare"], [DB, "--compare", "--joint-histo=" + O], [DB, "--het-max=5", "--joint-histo=" + O],
    [DB, WITH, "--compare", "--joint-max-a=5", "--het-max=5"], [DB, WITH, "--joint-histo=" + O, "--het-histo=" + O, "--gpus=2"],
    [DB, WITH, "--joint-histo=" + O, "--bin-a=" + O, "--gpus=2"], [DB, "--het-histo=" + O, "--het-lower=5", "--het-upper=4", "--bin-a=" + O],
    [DB, "--with={TMP}/missing.db", "--compare", "--a-lower=5", "--a-upper=4"], [DB, "--with={TMP}/missing.db", "--gpus=2", "--compare"],
    [DB, "--with={TMP}/missing.db"], [DB, "--with={TMP}/missing.db", "--compare", "--mode=CAS"],
    [DB, "--with={TMP}/k15.db", "--compare", "--mode=CAS"], [DB, WITH, "--compare", "--mode=CAS", "--exchange=ring"],
    [FQ, "--mode=CAS", "--lower=5", "--upper=4"], [FQ, "--exchange=ring", "--bin-a=" + O], [FQ, "--lower=5", "--upper=4", "--b-upper=0"],
    [FQ, "--exchange=ring", "--gpus=1", "--canonical"], [FQ, "--gpus=1", "--canonical", "--acgt-only", "--exchange=mini"],
    [FQ, "--format=fasta", "--min-qual-char=5", "--gpus=1", "--exchange=mini"],
    # --gpus=1 --canonical --exchange=mini: refused while the run still counts as a group.  --save, --load, --with and
    # wrapped FASTA take the run off the group path only behind that refusal; --min-count=2, --l=auto, --normalize and
    # the het outputs do so in front of it, and the run passes on (here: to the bare usage of --comm=bogus)
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", "--save=" + O], [FQ, "--gpus=1", "--canonical", "--exchange=mini", DB],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", WITH, "--compare"], [FQ, "--gpus=1", "--canonical", "--exchange=mini", WRAPPED],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", "--comm=bogus"],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", "--min-count=2", "--comm=bogus"],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", "--l=auto", "--comm=bogus"],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", "--normalize=" + O, "--comm=bogus"],
    [FQ, "--gpus=1", "--canonical", "--exchange=mini", "--k=15", "--het-pairs=" + O, "--comm=bogus"],
    [FQ, "--gpus=1", "--min-qual-char=5", "--exchange=mini", "--min-count=2", "--comm=bogus"],
    [FQ, "--canonical", "--exchange=mini", "--comm=bogus"],
    [FQ, "--filter=" + O, "--gpus=2", "--filter-median-lower=1"], [FQ, WRAPPED, "--gpus=2", "--read-medians=" + O],
    [FQ, WRAPPED, "--gpus=2", "--filter=" + O], [FQ, WRAPPED, "--filter=" + O, "--trim=" + O], [FQ, WRAPPED, "--trim=" + O, "--filter-pairs=all"],
    [FQ, "--filter-pairs=all", "--filter-singles=s"], [FQ, "--filter-singles=s", "--trim-interleaved"],
    [FQ, "--trim-singles=s", "--gpus=0"], [FQ, "--filter=" + O, "--gpus=2", "--filter-fraction=2"],
    [FQ, "--trim=" + O, "--gpus=2", "--trim-mode=bogus"], [FQ, "--filter=" + O, "--trim=" + O, "--gpus=2"],
    [DB, "--filter=" + O, "--trim=" + O], [FQ, "--save=" + O, "--gpus=2", "--filter=" + O], [FQ, DB, "--check", "--gpus=2"],
    [DB, "--check", "--filter=" + O], [DB, "--het-histo=" + O, "--filter=" + O], [FQ, "--het-histo=" + O, "--trim-mode=bogus"],
]

CASES = PARSER + strict_cases() + REFUSALS + ORDER


def run(exe, argv):
    p = subprocess.run([exe] + argv, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def fill(arg, tmp):
    return arg.replace("{GOLDEN}", GOLDEN).replace("{TMP}", tmp)


def blank(text, tmp, usage):
    """Recorded form of an output: the usage block and the two directories as tokens."""
    return text.replace(usage, "{USAGE}\n").replace(GOLDEN, "{GOLDEN}").replace(tmp, "{TMP}")


def run_case(exe, args, tmp, usage):
    rc, out, err = run(exe, [fill(x, tmp) for x in args])
    return {"args": args, "exit": rc, "stdout": blank(out, tmp, usage), "stderr": blank(err, tmp, usage)}


def main():
    exe = os.path.abspath(sys.argv[1])
    rc, out, usage = run(exe, ["--help"])
    assert rc == 1 and out == "" and usage.startswith("Usage: tsxCount") and usage.endswith("\n"), (rc, out, usage[:80])
    with open(USAGE_FILE, "w") as f:
        f.write(usage)
    runs = []
    with tempfile.TemporaryDirectory(prefix="cli_refusals_") as tmp:
        tmp = os.path.realpath(tmp)
        write_fixtures(tmp)
        for args in CASES:
            r = run_case(exe, args, tmp, usage)
            # a case that reaches a table belongs to the GPU tests, not here
            assert r["exit"] in (1, 2, 3) and "TSXException" not in r["stderr"] and "Creating" not in r["stderr"], r
            runs.append(r)
    assert len({json.dumps(r["args"]) for r in runs}) == len(runs), "a command line is listed twice"
    with open(CASES_FILE, "w") as f:
        json.dump({"generator": "tests/golden/make_cli_refusals.py", "runs": runs}, f, indent=1)
        f.write("\n")
    print("%d command lines -> %s" % (len(runs), CASES_FILE))


if __name__ == "__main__":
    main()
