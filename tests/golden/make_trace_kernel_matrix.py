#!/usr/bin/env python3
"""Generates tests/golden/trace_kernel_matrix.json: which ft_trace_kernel* handle ft_trace_kernel_for (kernels.hip) returns for a fixed grid of
keys — variant x carveKind x ext x libm x views x shade, keys() below — and the kernel handles the library exports.  No GPU is needed: the
function only returns a handle's address, which is named by comparing it with the addresses of the library's exported ft_trace_kernel*
data symbols ("null" for nullptr).

The table pins what the lookup answered before it was generated from the table of builds, so it is recorded from the library of the commit
whose behaviour is to be kept, not from the code under test.  That commit keeps the function `static`; the one change to the scratch copy it
is built from is `static` -> `extern "C"` on that function, so that it can be called at all:

    python tests/golden/make_trace_kernel_matrix.py SCRATCH/fraytracer_amd/libfraytracer_hip.so --commit <commit>

tests/test_trace_kernel_table.py replays the same grid against the library in the tree.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "trace_kernel_matrix.json")

VARIANTS = (0, 1, 2, 3, 4)                   # 4: no such family
CARVE_KINDS = (0, 1, 2, 3, 4, 7, 9)          # FtPrim sphere .. triangle, box (no carved build of its own), FT_CARVE_MIXED, a value that is no kind
SHADES = (0, 1, 2, 3)                        # 3: no such form


def keys():
    """[(variant, carveKind, ext, libm, views, shade)] in the order of the recorded answers"""
    return list(itertools.product(VARIANTS, CARVE_KINDS, (0, 1), (0, 1), (0, 1), SHADES))


def key_name(k):
    return "variant=%d kind=%d ext=%d libm=%d views=%d shade=%d" % k


def exported_handles(path):
    """names of the library's exported kernel handles (global data symbols; the host stubs are functions under other names)"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(set(re.findall(r"\b[DBR] (ft_trace_kernel[a-z0-9_]*)\b", out)) - {"ft_trace_kernel_for"})


def run(lib):
    """{key name: kernel name or "null"} for every key of the grid, asked of a ctypes.CDLL"""
    by_address = {C.addressof(C.c_char.in_dll(lib, n)): n for n in exported_handles(lib._name)}
    fn = lib.ft_trace_kernel_for
    fn.restype = C.c_void_p
    fn.argtypes = [C.c_uint, C.c_uint, C.c_bool, C.c_bool, C.c_bool, C.c_uint]
    out = {}
    for k in keys():
        p = fn(*k)
        out[key_name(k)] = "null" if not p else by_address[p]         # KeyError: a handle that is no exported ft_trace_kernel*
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--commit", required=True)
    args = ap.parse_args()
    answers = run(C.CDLL(args.lib))
    kernels = exported_handles(args.lib)
    unreachable = sorted(set(kernels) - set(answers.values()))
    assert not unreachable, f"kernels no key of the grid reaches: {unreachable}"
    table = {
        "header": "ft_trace_kernel_for's answers as recorded from commit %s built in a scratch copy whose only change is `static` -> "
                  "`extern \"C\"` on ft_trace_kernel_for (tests/golden/make_trace_kernel_matrix.py)" % args.commit,
        "recorded_from_commit": args.commit,
        "kernels": kernels,
        "answers": answers,
    }
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print(f"{len(answers)} keys, {len(kernels)} kernels, {sum(1 for v in answers.values() if v == 'null')} null -> {TABLE}")


if __name__ == "__main__":
    main()
