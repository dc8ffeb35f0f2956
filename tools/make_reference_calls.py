"""Writes tests/golden/reference_calls.json: which eigen_libs_mod / eigen_blacs_mod entities the reference's own benchmark
sources (benchmark/main2.f, mat_set.f, w_test.f, ev_test.f) call, and the keyword arguments they pass to each.

The sources are read as TEXT (fixed form: comment lines and column-6 continuations handled); only the names are kept.
tests/test_host.py::test_reference_benchmark_sources_find_their_symbols_in_the_module checks them against
eigenexa_amd/fortran/eigen_libs_mod.F90.
Run:  python tools/make_reference_calls.py <reference source tree>
"""
import json
import os
import re
import sys

FILES = ("main2.f", "mat_set.f", "w_test.f", "ev_test.f")


def scan(bench_dir):
    used, kw = set(), {}
    for fn in FILES:
        text = open(os.path.join(bench_dir, fn), errors="replace").read()
        lines = []
        for ln in text.splitlines():
            if not ln or ln[0] in "cC*!":          # fixed-form comment lines
                continue
            ln = ln.split("!")[0]
            if len(ln) > 5 and ln[5] not in " 0" and lines:   # continuation line (column 6)
                lines[-1] += ln[6:]
            else:
                lines.append(ln)
        for ln in lines:
            low = ln.lower()
            for m in re.finditer(r"\b(eigen_[a-z0-9_]+|get_constant_[a-z0-9_]+)\s*\(([^)]*)\)", low):
                name = m.group(1)
                used.add(name)
                for k in re.findall(r"\b([a-z_][a-z0-9_]*)\s*=", m.group(2)):
                    kw.setdefault(name, set()).add(k)
            for m in re.finditer(r"call\s+(eigen_[a-z0-9_]+)\b", low):
                used.add(m.group(1))
    used -= {"eigen_libs_mod", "eigen_blacs_mod"}
    return {"sources": ["benchmark/" + f for f in FILES], "used": sorted(used),
            "keywords": {k: sorted(v) for k, v in sorted(kw.items())}}


if __name__ == "__main__":
    out = scan(os.path.join(sys.argv[1], "benchmark"))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "reference_calls.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
