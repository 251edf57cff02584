"""lumahdrv_amd/capi.py's _ABI table against include/lumahip.h, declaration by declaration: the names, the number of parameters, the
class of every parameter's type and the class of the return type.  Needs neither a GPU nor the built library: the header is parsed
as text and capi is imported without lib()."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"float": C.c_float, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t, "uint64_t": C.c_uint64,
           "uint32_t": C.c_uint32, "long": C.c_long, "double": C.c_double}


def _split_top_level(params):
    """the parameter list cut at the commas outside any parentheses (a function-pointer parameter holds some inside)"""
    out, depth, cur = [], 0, ""
    for ch in params:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return [] if out in ([""], ["void"]) else out


def _declarations():
    """{name: (return type text, [parameter texts])} of every `lumahip_x(...);` in the header"""
    hdr = open(os.path.join(ROOT, "include", "lumahip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", " ", hdr, flags=re.M)
    decls = {}
    for m in re.finditer(r"([A-Za-z_][\w \t\n*]*?)\b(lumahip_\w+)\s*\(((?:[^()]|\([^()]*\))*)\)\s*;", hdr):
        assert m.group(2) not in decls, m.group(2)
        decls[m.group(2)] = (" ".join(m.group(1).split()), _split_top_level(" ".join(m.group(3).split())))
    return decls


def _is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, (C._Pointer, C._CFuncPtr)))


def _scalar_of(text):
    """the c_* type of a scalar parameter or return type: its type words without qualifiers and without the parameter's name"""
    words = [wd for wd in text.split() if wd != "const"]
    hits = [wd for wd in words if wd in SCALARS]
    assert len(hits) == 1, "no known scalar type in %r" % text
    return SCALARS[hits[0]]


@pytest.fixture(scope="module")
def decls():
    return _declarations()


def test_the_table_names_what_the_header_declares(decls):
    from lumahdrv_amd import capi
    assert len(decls) == 126
    assert set(decls) == set(capi.SYMBOLS)
    assert len(capi.SYMBOLS) == len(set(capi.SYMBOLS))
    assert capi.SYMBOLS == tuple(capi._ABI)


def test_every_parameter_agrees_with_the_header(decls):
    from lumahdrv_amd import capi
    bad = []
    for name, (_, params) in sorted(decls.items()):
        argtypes = capi._ABI[name][1]
        if len(argtypes) != len(params):
            bad.append("%s: %d argtypes, %d parameters" % (name, len(argtypes), len(params)))
            continue
        for k, (text, ctype) in enumerate(zip(params, argtypes)):
            if "*" in text or "[" in text:
                ok = _is_pointer(ctype)
                if "(" in text:                                  # a function pointer takes the callback type, not a data pointer
                    ok = ctype is capi.PROBE_FN
            else:
                ok = ctype is _scalar_of(text)
            if not ok:
                bad.append("%s: parameter %d `%s` is %r" % (name, k, text, ctype))
    assert not bad, "\n".join(bad)


def test_every_return_type_agrees_with_the_header(decls):
    from lumahdrv_amd import capi
    bad = []
    for name, (ret, _) in sorted(decls.items()):
        restype = capi._ABI[name][0]
        if "*" in ret:
            ok = restype is not None and _is_pointer(restype)
        elif ret == "void":
            ok = restype is None
        else:
            ok = restype is _scalar_of(ret)
        if not ok:
            bad.append("%s: returns `%s`, restype %r" % (name, ret, restype))
    assert not bad, "\n".join(bad)


def test_the_parser_sees_drift():
    """the comparison's own pieces on hand-made input: nested commas, array and function-pointer parameters, void lists"""
    assert _split_top_level("int n, double (*probe)(int i, int r, void *user), void *user") == \
        ["int n", "double (*probe)(int i, int r, void *user)", "void *user"]
    assert _split_top_level("void") == [] and _split_top_level("") == []
    assert _scalar_of("unsigned w") is C.c_uint and _scalar_of("const size_t n") is C.c_size_t and _scalar_of("int") is C.c_int
    assert _is_pointer(C.POINTER(C.c_int)) and _is_pointer(C.c_char_p) and _is_pointer(C.CFUNCTYPE(C.c_int))
    assert not _is_pointer(C.c_size_t) and not _is_pointer(None)
