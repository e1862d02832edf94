"""gmr_amd/csrc/slice_plan.h without a GPU: tests/slice_plan_host.cpp (its own main, built with the host compiler under
AddressSanitizer and UBSan, never loaded into Python) makes the schedule of a sliced IK launch for every longest item T in 1..600,
slice length L in 1..70 and 256 and taper floor f in 0..40 and checks, for each: the boundaries rise strictly from 0 to T in slices
of at most L; the three uniform cases are the fixed-length schedule r L; a taper never grows, ends under 2 f and adds at most
ceil(log2(L / f)) + 2 rounds; the form the kernel reads gives the same slices as the boundary list; and for every item length
n <= T the clipped slices tile [0, n), exactly one ends the item, and every later ticket leaves at once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmr_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "slice_plan_host.cpp")


def build_slice_plan_host(out_dir, sanitize=True):
    """The stand-alone program, or None without a host compiler.  sanitize=False: a plain build, for the GPU tests that only ask it
    for a schedule (tests/test_gpu_ik_slice_taper.py): sanitizer builds stay with the tests that need no GPU."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        return None
    exe = os.path.join(str(out_dir), "slice_plan_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [f"-I{CSRC}", SOURCE, "-o", exe])
    return exe


def slice_lengths(exe, T, L, f):
    """[slice lengths] of the schedule for (T, L, f), as slice_plan.h makes it on the host."""
    out = subprocess.run([exe, str(T), str(L), str(f)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    rounds, lens = int(out[0]), [int(v) for v in out[1:]]
    assert rounds == len(lens) and sum(lens) == T
    return lens


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = build_slice_plan_host(tmp_path_factory.mktemp("slice_plan"))
    if path is None:
        pytest.skip("no C++ compiler")
    return path


def test_every_schedule_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    schedules, tapered, lengths = (int(v) for v in r.stdout.split()[1:4])
    assert schedules == 600 * 71 * 41
    assert tapered > schedules // 10 and lengths > 10 * schedules


def test_worked_examples(exe):
    assert slice_lengths(exe, 3000, 256, 32) == [256] * 10 + [184, 128, 64, 32, 32]  # the headline batch: 15 rounds against 12
    assert slice_lengths(exe, 3000, 256, 0) == [256] * 11 + [184]
    assert slice_lengths(exe, 45, 16, 1) == [16, 13, 8, 4, 2, 1, 1]
    assert slice_lengths(exe, 45, 16, 4) == [16, 13, 8, 4, 4]
    assert slice_lengths(exe, 45, 16, 9) == [16, 16, 13]  # ceil(L / 2) < f: uniform
    assert slice_lengths(exe, 16, 16, 2) == [16]          # T <= L: uniform
    assert slice_lengths(exe, 71, 7, 1)[-4:] == [1, 4, 2, 1]


def test_slice_plan_header_is_plain_cxx():
    """No HIP include: the stand-alone build above and the kernel share the header."""
    text = open(os.path.join(CSRC, "slice_plan.h")).read()
    assert "hip" not in "\n".join(ln for ln in text.split("\n") if ln.lstrip().startswith("#include"))
