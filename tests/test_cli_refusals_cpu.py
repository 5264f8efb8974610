"""What the command line does before it touches a GPU, pinned byte for byte: tests/golden/cli_refusals.json holds the
exit status, stdout and stderr of command lines that end in main() before a table is created (an option the parser turns
down, a refusal, a database header that cannot be read or does not match, an input --l=auto cannot read), and
tests/golden/cli_usage.txt the usage block.  tests/golden/make_cli_refusals.py wrote both and says how."""
import importlib.util
import json
from concurrent.futures import ThreadPoolExecutor
import os
import re

import pytest

from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "tsxcount_amd", "bin", "tsxCount")

_spec = importlib.util.spec_from_file_location("make_cli_refusals", os.path.join(GOLDEN, "make_cli_refusals.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.CASES_FILE) as _f:
    RUNS = json.load(_f)["runs"]
with open(gen.USAGE_FILE) as _f:
    USAGE = _f.read()


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    tmp = os.path.realpath(str(tmp_path_factory.mktemp("cli")))
    gen.write_fixtures(tmp)
    return tmp


def test_the_usage_block_is_the_pinned_one():
    assert gen.run(EXE, ["--help"]) == (1, "", USAGE)


def test_the_corpus_is_the_generators_list():
    assert [r["args"] for r in RUNS] == gen.CASES


@pytest.fixture(scope="module")
def reruns(fixtures):
    """Every recorded command line run again, once for the module (a process start each, a few at a time)."""
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda r: gen.run_case(EXE, r["args"], fixtures, USAGE), RUNS))


@pytest.mark.parametrize("i", range(len(RUNS)), ids=lambda i: "%03d" % i)
def test_case_reproduces_byte_for_byte(i, reruns):
    want = RUNS[i]
    assert want["exit"] in (1, 2, 3) and "TSXException" not in want["stderr"]     # (ends before a table is created)
    assert reruns[i] == want


def test_every_option_of_the_usage_text_is_known_to_the_parser():
    words = sorted(set(re.findall(r"--[a-z][a-z0-9]*(?:-[a-z0-9]+)*", USAGE)))
    assert len(words) > 80 and "--min-count" in words and "--het-mode" in words
    # alone and with a value, without --input: main returns at a refusal, at a --load it cannot open or at "no
    # --input and no --load" (--input itself is given a mode this binary refuses, so that it stops there)
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(lambda w: gen.run(EXE, [w + "=1"] + (["--mode=CAS"] if w == "--input" else [])), words))
    for w, (rc, out, err) in zip(words, got):
        assert rc in (1, 2, 3) and "unknown option" not in err, (w, err[:200])
        assert "Creating" not in err and "TSXException" not in err, (w, err[:200])
        assert (rc == 1) == err.endswith(USAGE) and (out == "" or w == "--input"), (w, rc, err[:200])
