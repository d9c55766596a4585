"""The ctypes tables of cimrgp_amd/_lib.py against the prototypes of include/*.h, type for type.  A table entry that
says c_int where the header says int64_t loads and runs, and truncates silently; the per-feature
``..._exported_and_registered`` tests compare argument counts only.  No GPU is needed: the headers are read as text."""
import ctypes
import glob
import os
import re

from cimrgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

#: the headers held 87 prototypes when this test was written; fewer found means the pattern below stopped matching
MIN_PROTOTYPES = 87

SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "uint64_t": ctypes.c_uint64}


def prototypes(header):
    """[(name, return type, [parameter type, ...])] of a header's ``int|size_t|const char* cimrgp_...(...);`` declarations,
    comments and preprocessor lines stripped; a type is the declaration without the parameter's name."""
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    found = []
    for ret, name, params in re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(cimrgp_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        types = []
        if params != "void":
            for p in params.split(","):
                m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p)      # "<type> <name>", the type ending in a blank or a *
                assert m, "%s: cannot read parameter %r of %s" % (header, p, name)
                types.append(m.group(1).replace("const", "").replace(" ", ""))
        found.append((name, ret.replace("const", "").replace(" ", ""), types))
    return found


def agrees(ctype, decl):
    """Whether the ctypes type stands for the C type ``decl`` (blanks and const removed)."""
    if decl.endswith("*"):
        return ctype in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(ctype, type(ctypes.POINTER(ctypes.c_int)))
    return decl in SCALARS and ctype is SCALARS[decl]


def test_every_header_is_registered_once():
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "*.h")))
    assert sorted(_lib.HEADERS) == headers
    tables = list(_lib.HEADERS.values())
    assert len(set(map(id, tables))) == len(tables), "one table registered under two headers"
    # the registry follows the include order of the umbrella header
    main = open(os.path.join(INCLUDE, "cimrgp.h")).read()
    assert list(_lib.HEADERS) == ["cimrgp.h"] + re.findall(r'^#include "(cimrgp_\w+\.h)"', main, re.M)


def test_tables_agree_with_the_prototypes_type_for_type():
    total = 0
    for header, table in _lib.HEADERS.items():
        protos = prototypes(header)
        total += len(protos)
        names = [name for name, _, _ in protos]
        assert len(set(names)) == len(names), "%s declares a name twice" % header
        assert sorted(table) == sorted(names), "%s: table and prototypes differ: %s" % (
            header, sorted(set(table) ^ set(names)))
        for other, other_table in _lib.HEADERS.items():
            if other != header:
                assert not set(names) & set(other_table), "%s: also registered under %s: %s" % (
                    header, other, sorted(set(names) & set(other_table)))
        for name, ret, types in protos:
            restype, argtypes = table[name]
            assert agrees(restype, ret), "%s: restype %r, declared %s" % (name, restype, ret)
            assert len(argtypes) == len(types), "%s: %d argtypes, %d parameters" % (name, len(argtypes), len(types))
            for i, (ctype, decl) in enumerate(zip(argtypes, types)):
                assert agrees(ctype, decl), "%s: argument %d is %r, declared %s" % (name, i, ctype, decl)
    assert total >= MIN_PROTOTYPES, "only %d prototypes found" % total
    merged = _lib.signatures()
    assert len(merged) == total == sum(len(t) for t in _lib.HEADERS.values())


def test_load_applies_the_merged_view():
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.signatures().items():
        fn = getattr(lib, name)
        assert fn.restype == restype and fn.argtypes == argtypes, name
