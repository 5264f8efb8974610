#!/usr/bin/env python3
"""Writes tests/golden/python_api.json, the importable surface of the tsxcount_amd package:

    python tests/golden/make_python_api.py <commit the tree is checked out at>

The file was recorded once, from the commit named in its "source_commit", before the package was split into
modules; tests/test_python_api_cpu.py compares the live package to it with surface() below.  It is not regenerated
when code moves between modules: a difference is then a change of the surface, to be made on purpose, by hand.

Recorded, for `import tsxcount_amd as T`:
  names       every public (no leading underscore) attribute of T but the package's own submodules, with its kind --
              function, class, structure, dtype, module (ctypes, os, np: tests reach them as T.ctypes) or constant --
              and, for a constant of a plain type, its repr
  private     the kind of the underscore names that tests, scripts and the benchmark reach for
  functions   str(inspect.signature(f)) of every public function
  classes     of every public class that is no Structure: __init__ and each public method with its signature, each
              property as "property"
  structures  of every ctypes.Structure: the (field name, ctypes type name) pairs and the public methods
  dtypes      the descr of every numpy dtype constant
Neither the built library nor a GPU is needed: importing the package loads nothing.
"""
import ctypes
import inspect
import json
import os
import sys
import types

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
API_FILE = os.path.join(GOLDEN, "python_api.json")
PRIVATE = ("_check", "_p")   # underscore names used outside the package (tests/, scripts/)


def kind_of(v):
    import numpy as np
    if isinstance(v, types.ModuleType):
        return "module " + v.__name__
    if isinstance(v, type):
        return "structure" if issubclass(v, ctypes.Structure) else "class"
    if isinstance(v, types.FunctionType):
        return "function"
    if isinstance(v, np.dtype):
        return "dtype"
    return "constant"


def members(cls):
    """The public members a class has in Python code, its own or inherited (and __init__): signature, or "property"."""
    out = {}
    for name in dir(cls):
        if name.startswith("_") and name != "__init__":
            continue
        v = inspect.getattr_static(cls, name)
        if isinstance(v, property):
            out[name] = "property"
        elif isinstance(v, (classmethod, staticmethod)):
            out[name] = type(v).__name__ + str(inspect.signature(v.__func__))
        elif isinstance(v, types.FunctionType):
            out[name] = str(inspect.signature(v))
    return out


def descr(dt):
    return json.loads(json.dumps(dt.descr))   # tuples as lists, the way the file holds them


def surface():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import tsxcount_amd as T
    public = {n: v for n, v in vars(T).items()
              if not n.startswith("_") and not getattr(v, "__name__", "").startswith(T.__name__ + ".")}
    s = {"names": {}, "private": {n: kind_of(getattr(T, n)) for n in PRIVATE}, "functions": {}, "classes": {},
         "structures": {}, "dtypes": {}}
    for n in sorted(public):
        v, k = public[n], kind_of(public[n])
        if isinstance(v, str) and os.path.isabs(v):
            v = os.path.relpath(v, ROOT)   # LIB_PATH, HEADER_PATH: where they point inside the tree
        s["names"][n] = k if k != "constant" or not isinstance(v, (int, str, tuple, dict, range)) else k + " " + repr(v)
        if k == "function":
            s["functions"][n] = str(inspect.signature(v))
        elif k == "class":
            s["classes"][n] = members(v)
        elif k == "structure":
            s["structures"][n] = {"fields": [[f[0], f[1].__name__] for f in v._fields_], "methods": members(v)}
        elif k == "dtype":
            s["dtypes"][n] = descr(v)
    return s


def main():
    with open(API_FILE, "w") as f:
        json.dump({"generator": "tests/golden/make_python_api.py", "source_commit": sys.argv[1], "surface": surface()},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print("-> %s" % API_FILE)


if __name__ == "__main__":
    main()
