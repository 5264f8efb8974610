"""The ctypes signature table of the package (tsxcount_amd._abi.SIGNATURES) against the prototypes of
include/tsxcount_hip.h: the same functions in both, the same number of parameters, and per parameter and return value
the same kind -- a pointer in the header is any ctypes pointer type, int / size_t / uint64_t / uint32_t / double are
c_int / c_size_t / c_uint64 / c_uint32 / c_double, a void return is None.  A width that differs (c_int where the header
says size_t) would cut an argument short without a word; nothing else checks it.  Every prototype is compared: none
is left out, and a type this file does not know fails the test.  Reads the header and the table only: no library, no GPU."""
import ctypes
import re

import pytest

import tsxcount_amd as T
from tsxcount_amd._abi import SIGNATURES
from test_abi import declared_symbols

SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
           "double": ctypes.c_double}
POINTER = "pointer"


def c_kind(decl, is_return=False):
    """What a parameter declaration (or a return type) of the header is: POINTER, a ctypes scalar, or None for void."""
    if "*" in decl or "[" in decl:
        return POINTER
    words = [w for w in decl.split() if w != "const"]
    if not is_return and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    assert len(words) == 1, "not understood: %r" % decl
    if is_return and words[0] == "void":
        return None
    assert words[0] in SCALARS, "a type this test does not know: %r" % decl
    return SCALARS[words[0]]


def prototypes():
    """{name: (return kind, [parameter kinds])} of every function the header declares."""
    text = open(T.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(tsx_hip_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, "declared twice: " + name
        plist = [p.strip() for p in params.split(",")]
        out[name] = (c_kind(ret.strip(), is_return=True), [] if plist == ["void"] else [c_kind(p) for p in plist])
    return out


PROTOS = prototypes()


def ctypes_kind(t):
    if t is None:
        return None
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return POINTER
    return t


def test_every_prototype_is_parsed():
    syms = declared_symbols()
    assert len(PROTOS) == len(syms) and sorted(PROTOS) == syms      # nothing the header declares is skipped
    assert len(PROTOS) >= 156


def test_the_table_and_the_header_name_the_same_functions():
    assert sorted(set(PROTOS) - set(SIGNATURES)) == [], "declared, no signature"
    assert sorted(set(SIGNATURES) - set(PROTOS)) == [], "a signature for what the header does not declare"


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_signature_matches_the_prototype(name):
    want_ret, want_args = PROTOS[name]
    restype, argtypes = SIGNATURES[name]
    assert len(argtypes) == len(want_args), "%s: %d parameters, the header has %d" % (name, len(argtypes), len(want_args))
    assert ctypes_kind(restype) == want_ret, "%s: return type %r" % (name, restype)
    for i, (have, want) in enumerate(zip(argtypes, want_args)):
        assert ctypes_kind(have) == want, "%s: parameter %d is %r" % (name, i, have)


def test_the_checker_tells_widths_apart():
    """c_int for a size_t, a scalar for a pointer, a missing parameter: each is a difference this file sees."""
    assert ctypes_kind(ctypes.c_int) != c_kind("size_t n") and ctypes_kind(ctypes.c_uint32) != c_kind("uint64_t seed")
    assert ctypes_kind(ctypes.c_uint64) != c_kind("const uint64_t *kmers") == ctypes_kind(ctypes.POINTER(ctypes.c_uint64))
    assert c_kind("const char *", is_return=True) == POINTER and c_kind("void", is_return=True) is None
    assert ctypes_kind(ctypes.c_char_p) == ctypes_kind(ctypes.c_void_p) == POINTER
    with pytest.raises(AssertionError):
        c_kind("unsigned long n")
