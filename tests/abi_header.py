"""include/sfmwarp.h as the CPU tests read it: the declared entry points, their prototypes and the layout of its descriptors, so
that every test holds the binding (_lib.py) against the ONE header in the same way.  A plain module: no fixtures, no device."""
import ctypes as C
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
HEADER = os.path.join(ROOT, "include", "sfmwarp.h")
CONSTANTS = {"SFM_MAX_SCALES": _lib.SFM_MAX_SCALES, "SFM_MAX_SRC": _lib.SFM_MAX_SRC}

with open(HEADER) as _f:
    TEXT = re.sub(r"/\*.*?\*/", "", _f.read(), flags=re.S)      # the header without its comments


def declared():
    """the sorted names of the functions the header declares"""
    return sorted(set(re.findall(r"\b(sfm_[a-z0-9_]+)\s*\(", TEXT)))


def prototypes():
    """name -> parameter list (text) of every function the header declares"""
    code = re.sub(r"^\s*#.*$", "", TEXT, flags=re.M)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(sfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}


def parameters(name):
    """the parameters of one prototype, as texts ([] for `void`)"""
    params = prototypes()[name].strip()
    return [] if params in ("", "void") else [p.strip() for p in params.split(",")]


def struct_fields(name):
    """[(field, element size, count)] of `typedef struct name {...} name;` in declaration order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), TEXT, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float \*|float \*|int32_t |float )(.*)$", decl)
        assert m, decl
        size = C.sizeof(C.c_void_p) if m.group(1).endswith("*") else 4
        for item in m.group(2).split(","):
            a = re.match(r"(\w+)(?:\[(\w+)\])?$", item.strip().lstrip("*"))
            assert a, item
            fields.append((a.group(1), size, CONSTANTS[a.group(2)] if a.group(2) else 1))
    return fields


def assert_layout(struct, name):
    """the ctypes Structure `struct` is `name` of the header: the same members in the same order, each at the offset the C layout
    rule gives it (a multiple of its element size) with its size, and the same total size"""
    fields = struct_fields(name)
    assert [f[0] for f in fields] == [f[0] for f in struct._fields_], name
    off, align = 0, 1
    for field, size, count in fields:
        off = -(-off // size) * size
        assert getattr(struct, field).offset == off, (name, field)
        assert getattr(struct, field).size == size * count, (name, field)
        off += size * count
        align = max(align, size)
    assert C.sizeof(struct) == -(-off // align) * align, name
