#!/usr/bin/env python3
"""Record the digests of every registry model's plan for tests/golden/model_plan_digests.json (tests/test_model_plan_host.py).

    python tools/record_model_plan.py --commit <id> [--hook-lib LIB] [--out FILE]

A plan is everything gmr_amd/csrc/model_plan.h derives from a blob: the two DevModels, both LdsLayouts, the scalars and every table of
the model image with its offset (the dump format is in tests/model_plan_host.cpp).  One SHA-256 per case: every packed
``params.IK_CONFIG_DICT`` config x force_generic in {0, 1} x min_nvp in {0, 64}.  Each case is planned twice and must dump the same bytes.

Without --hook-lib the plans come from the stand-alone program built from this tree.  To pin the digests to a commit from before
model_plan.h existed, give that commit's library a temporary export

    int gmr_debug_plan_dump(const void *blob, size_t bytes, int min_nvp, int force_generic, const char *path)

that runs the model build up to its first device call (with the DevModel images zeroed by memset before they are filled, as
model_plan.h does) and writes the same dump, and pass the library as --hook-lib.  No device is needed either way.  The commit id is
stored in the file; nothing else identifies the build.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import model_plan_cases as mp  # noqa: E402


def hook_digests(lib_path, cases, workdir):
    lib = C.CDLL(lib_path)
    f = lib.gmr_debug_plan_dump
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_char_p]
    out = {}
    for key, blob, nvp, fg in cases:
        path = os.path.join(workdir, "hook.dump")
        rc = f(blob, len(blob), nvp, fg, path.encode())
        assert rc == 0, (key, rc)
        with open(path, "rb") as fh:
            out[key] = hashlib.sha256(fh.read()).hexdigest()
        os.remove(path)
    return out


def program_digests(exe, cases, workdir):
    res = mp.run_cases(exe, cases, workdir)
    assert all(r["code"] == 0 for r in res.values()), {k: r["message"] for k, r in res.items() if r["code"]}
    return {k: r["digest"] for k, r in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit whose plans are recorded")
    ap.add_argument("--hook-lib", help="a library of that commit with the temporary gmr_debug_plan_dump export")
    ap.add_argument("--out", default=mp.GOLDEN)
    args = ap.parse_args()
    cases = mp.registry_cases()
    assert len(cases) >= 4 * 12
    with tempfile.TemporaryDirectory() as tmp:
        if args.hook_lib:
            runs = [hook_digests(args.hook_lib, cases, tmp) for _ in range(2)]
        else:
            cxx, rocm = mp.toolchain()
            assert cxx and rocm, "needs a C++ compiler and the ROCm headers"
            exe = mp.build_program(cxx, os.path.join(tmp, "model_plan_host"), ["-O1"])
            runs = [program_digests(exe, cases, tmp) for _ in range(2)]
    assert runs[0] == runs[1], "the dumps are not reproducible"
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "source": "hook" if args.hook_lib else "program", "digests": runs[0]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(runs[0])} cases, {os.path.getsize(args.out)} bytes, commit {args.commit}")


if __name__ == "__main__":
    main()
