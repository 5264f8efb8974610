"""The importable surface of the package -- public names and their kinds, signatures of the functions and of the two
classes' methods, structure fields, dtypes -- is the one tests/golden/python_api.json recorded before the package was
split into modules.  tests/golden/make_python_api.py wrote the file and says what it holds.  No library, no GPU."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_python_api", os.path.join(GOLDEN, "make_python_api.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.API_FILE) as _f:
    RECORDED = json.load(_f)
WANT = RECORDED["surface"]


@pytest.fixture(scope="module")
def live():
    return gen.surface()


def test_the_record_names_its_commit_and_is_not_empty():
    assert len(RECORDED["source_commit"]) >= 7
    assert (len(WANT["names"]), len(WANT["functions"]), len(WANT["structures"]), len(WANT["dtypes"])) == (106, 42, 21, 7)
    assert len(WANT["classes"]["TSXHashMapHIP"]) == 91 and len(WANT["classes"]["TSXHashMapHIPGroup"]) == 15
    assert sorted(WANT) == ["classes", "dtypes", "functions", "names", "private", "structures"]


def test_public_names_and_kinds_are_the_recorded_ones(live):
    assert sorted(live["names"]) == sorted(WANT["names"])     # none gone, none new
    assert live["names"] == WANT["names"]
    assert live["private"] == WANT["private"]


@pytest.mark.parametrize("section", ["functions", "structures", "dtypes"])
def test_section_is_the_recorded_one(section, live):
    for name in WANT[section]:
        assert live[section].get(name) == WANT[section][name], name
    assert live[section] == WANT[section]


@pytest.mark.parametrize("cls", sorted(WANT["classes"]))
def test_class_members_are_the_recorded_ones(cls, live):
    for name in WANT["classes"][cls]:
        assert live["classes"][cls].get(name) == WANT["classes"][cls][name], cls + "." + name
    assert live["classes"][cls] == WANT["classes"][cls]
