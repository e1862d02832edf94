"""What tests/test_model_plan_host.py and tools/record_model_plan.py share: the cases (every packed registry config x force_generic x
min_nvp), the build of the stand-alone program tests/model_plan_host.cpp, and one run of it over a list of cases."""
import hashlib
import os
import shutil
import subprocess

from gmr_amd import params
from tests.util import compiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmr_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "model_plan_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_plan_digests.json")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SANITIZE = ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def registry_configs():
    """(src, robot) of every ``params.IK_CONFIG_DICT`` entry whose pack exists (the registry names more configs than have been packed)."""
    return [(src, robot) for src, robots in params.IK_CONFIG_DICT.items() for robot, path in robots.items() if os.path.exists(path)]


def registry_cases():
    """(key, blob, min_nvp, force_generic) per case."""
    return [(f"{src}/{robot}/generic{fg}/min_nvp{nvp}", compiled(src, robot).blob, nvp, fg)
            for src, robot in registry_configs() for fg in (0, 1) for nvp in (0, 64)]


def toolchain():
    """The host compiler, or None; and whether the ROCm headers (<hip/hip_vector_types.h>) are there."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    return cxx, os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_vector_types.h"))


def build_program(cxx, exe, extra=()):
    subprocess.check_call([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INCLUDE}", f"-I{CSRC}", "-Wall", "-Wextra", "-Werror", *extra,
                           PROGRAM, "-o", str(exe)])
    return str(exe)


def run_cases(exe, cases, workdir, dump=True):
    """Plan every (key, blob, min_nvp, force_generic) with the program.  Returns {key: result}: code, message, shape, name, fields
    (the 15 ints, empty on an error) and digest (SHA-256 of the dump, None without one)."""
    workdir = str(workdir)
    lines, dumps = [], []
    for i, (_, blob, nvp, fg) in enumerate(cases):
        blob_path, dump_path = os.path.join(workdir, f"case{i}.blob"), os.path.join(workdir, f"case{i}.dump")
        with open(blob_path, "wb") as f:
            f.write(blob)
        dumps.append(dump_path)
        lines.append(f"{blob_path} {nvp} {fg} {dump_path if dump else '-'}")
    env = dict(os.environ)
    env.pop("GMR_DEBUG_PLAN", None)
    # a plan is half a second of hill climbing (more under the sanitizers): a few processes, every nth case each
    nproc = max(1, min(8, os.cpu_count() or 1, len(cases) // 4))
    procs = []
    for k in range(nproc):
        manifest = os.path.join(workdir, f"manifest{k}.txt")
        with open(manifest, "w") as f:
            f.write("\n".join(lines[k::nproc]) + "\n")
        procs.append(subprocess.Popen([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    out = [None] * len(cases)
    for k, proc in enumerate(procs):
        stdout, stderr = proc.communicate(timeout=600)
        assert proc.returncode == 0 and not stderr, stdout[-2000:] + stderr[-4000:]
        part = stdout.splitlines()
        assert len(part) == len(lines[k::nproc]), stdout[-2000:]
        out[k::nproc] = part
    results = {}
    for (key, _, _, _), line, dump_path in zip(cases, out, dumps):
        code, message, shape, name, fields = line.split("|")
        digest = None
        if os.path.exists(dump_path):
            with open(dump_path, "rb") as f:
                digest = hashlib.sha256(f.read()).hexdigest()
            os.remove(dump_path)
        results[key] = dict(code=int(code), message=message, shape=int(shape), name=name, fields=[int(x) for x in fields.split(",")] if fields else [],
                            digest=digest)
    return results
