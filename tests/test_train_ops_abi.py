"""The ctypes signatures of sgrl_amd/train_ops.py against the prototypes of include/sgrl_train.h: every argument kind and return
type of every entry point, and the layout of the weight-gradient descriptor.  A wrong letter in the signature table is a kernel
writing through a truncated pointer, not a Python error -- so the header is parsed here and the table held to it."""
import ctypes
import os
import re

import pytest

from sgrl_amd import _lib
from test_abi import REPO, _declared

ARG = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
RES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


def _header():
    text = open(os.path.join(REPO, "include", "sgrl_train.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//.*$", "", text, flags=re.M)
    return re.sub(r"^\s*#.*$", "", text, flags=re.M)


def _prototypes():
    """{name: (return type, [parameter type or "*" for any pointer])} of every function the header declares."""
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", _header(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(sgrl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        kinds = []
        for prm in (p.strip() for p in params.split(",")):
            if prm == "void" and "," not in params:
                continue
            if "*" in prm:
                kinds.append("*")
            else:
                words = prm.split()
                assert len(words) == 2, (name, prm)          # "<type> <name>"
                kinds.append(words[0])
        assert name not in protos, name
        protos[name] = (ret, kinds)
    return protos


@pytest.fixture(scope="module")
def L():
    _lib.build()
    from sgrl_amd import train_ops
    return train_ops._L()


def test_every_signature_matches_the_header(L):
    protos = _prototypes()
    declared = _declared("sgrl_train.h")
    assert sorted(protos) == declared and len(protos) == len(declared) >= 46     # no prototype the parser could not read
    for name, (ret, kinds) in sorted(protos.items()):
        fn = getattr(L, name)
        want = [ctypes.c_void_p if k == "*" else ARG[k] for k in kinds]
        assert fn.argtypes is not None and list(fn.argtypes) == want, name
        assert fn.restype is RES[ret], name


def test_the_descriptor_dtype_is_the_headers_struct():
    from sgrl_amd import train_ops
    body = re.search(r"typedef\s+struct\s+sgrl_wgrad_desc\s*\{(.*?)\}\s*sgrl_wgrad_desc\s*;", _header(), flags=re.S).group(1)
    fields, offset = [], 0
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        if "*" in decl:                                          # "const float* dy": one pointer per declaration
            names, kind, size = [decl.replace("*", " ").split()[-1]], "u", 8
        else:                                                    # "int32_t lddy, ldy, ..."
            ctype, rest = decl.split(None, 1)
            assert ctype == "int32_t", decl
            names, kind, size = [n.strip() for n in rest.split(",")], "i", 4
        for n in names:
            offset = (offset + size - 1) // size * size          # natural alignment
            fields.append((n, kind, size, offset))
            offset += size
    D = train_ops._DESC
    assert list(D.names) == [f[0] for f in fields] and len(fields) == 14
    for n, kind, size, off in fields:
        dt, at = D.fields[n][:2]
        assert (dt.kind, dt.itemsize, at) == (kind, size, off), n
    assert D.itemsize == (offset + 7) // 8 * 8 == 80
