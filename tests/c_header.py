"""The prototypes of include/eigenexa_amd.h as text, for the tests that hold the ctypes table against the header."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eigenexa_amd.h")


def _declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def prototype(name):
    """the parameters of the int-valued entry ``name``, one string each, blanks squeezed"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _declarations())
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def all_prototypes():
    """{name: (return type, [parameter, ...])} of every eigx_* entry; ``(void)`` is an empty list"""
    out = {}
    for ret, name, params in re.findall(r"\b(int|double|int64_t|void\s*\*)\s+(eigx_\w+)\s*\(([^)]*)\)\s*;", _declarations()):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (ret.replace(" ", ""), [] if params == ["void"] else params)
    return out
