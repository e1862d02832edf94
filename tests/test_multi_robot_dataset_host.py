"""The multi-robot dataset output, the parts that need no GPU: the two epilogue exports and their ctypes layout, the --robots flag of
the dataset scripts and its per-robot target planning."""
import argparse
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmr_motion_epilogue", "gmr_group_motion_epilogue")


def test_motion_epilogue_exports_are_declared_and_bound():
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+gmr_motion_epilogue\s*\(gmr_model \*m, const gmr_motion_input \*in, void \*stream\)", src)
    assert re.search(r"\bint\s+gmr_group_motion_epilogue\s*\(gmr_group \*g, const gmr_motion_input \*inputs, void \*stream\)", src)
    assert re.search(r"#define GMR_MOTION_HEIGHT_ADJUST 1\b", src) and re.search(r"#define GMR_MOTION_ROOT_ORIGIN 2\b", src)
    assert _native.MOTION_HEIGHT_ADJUST == 1 and _native.MOTION_ROOT_ORIGIN == 2
    for name in NEW:
        assert name in _native.EXPORTS
    lib = _native.load()
    assert lib.gmr_abi_version() == 5
    # null handles are refused before anything else (no device needed)
    mi = _native.MotionInput()
    assert lib.gmr_motion_epilogue(None, ctypes.byref(mi), None) == -1
    assert lib.gmr_group_motion_epilogue(None, ctypes.byref(mi), None) == -1


def test_motion_input_layout_matches_the_c_struct():
    """ctypes.sizeof / offsets of MotionInput against the struct as a C compiler lays it out (x86-64 SysV, like the library)."""
    from gmr_amd import _native
    M = _native.MotionInput
    assert ctypes.sizeof(M) == 80
    want = {"qpos": 0, "n_frames": 8, "seq_offsets": 16, "n_seq": 24, "flags": 28, "ground_offset": 32, "root_pos_out": 40,
            "root_rot_out": 48, "dof_pos_out": 56, "local_body_pos_out": 64, "min_z_out": 72}
    for k, off in want.items():
        assert getattr(M, k).offset == off, k


def _parser():
    from gmr_amd.scripts._walk import add_common_flags
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default=None)
    add_common_flags(ap)
    return ap


def _resolve(argv):
    from gmr_amd.scripts._walk import resolve_robots
    ap = _parser()
    args = ap.parse_args(argv)
    resolve_robots(ap, args)
    return args


def test_robots_flag_parsing():
    a = _resolve([])
    assert a.robot == "unitree_g1" and a.robot_list is None
    a = _resolve(["--robot", "booster_t1"])
    assert a.robot == "booster_t1" and a.robot_list is None
    a = _resolve(["--robots", "unitree_g1, booster_t1,fourier_n1"])
    assert a.robot_list == ["unitree_g1", "booster_t1", "fourier_n1"]
    for bad in (["--robot", "unitree_g1", "--robots", "booster_t1"], ["--robots", ","], ["--robots", "unitree_g1,unitree_g1"]):
        with pytest.raises(SystemExit):
            _resolve(bad)


def test_robots_flag_in_both_scripts_refuses_robot_and_robots(tmp_path):
    from gmr_amd.scripts import bvh_to_robot_dataset, smplx_to_robot_dataset
    for script in (bvh_to_robot_dataset, smplx_to_robot_dataset):
        with pytest.raises(SystemExit):
            script.main(["--src_folder", str(tmp_path), "--tgt_folder", str(tmp_path / "o"), "--robot", "unitree_g1", "--robots", "booster_t1"])


def test_per_robot_target_planning(tmp_path):
    from gmr_amd.scripts._walk import plan
    src, tgt = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(os.path.join(src, "sub"))
    for n in ("a.bvh", "b.bvh", os.path.join("sub", "c.bvh"), "notes.txt"):
        open(os.path.join(src, n), "w").write("x")
    args = _resolve(["--robots", "unitree_g1,booster_t1"])
    args.src_folder, args.tgt_folder = src, tgt
    srcs, tgts, skipped = plan(args, ".bvh", lambda n: n.endswith(".bvh"))
    assert [os.path.relpath(s, src) for s in srcs] == ["a.bvh", "b.bvh", os.path.join("sub", "c.bvh")] and skipped == 0
    assert tgts[2] == (os.path.join(tgt, "unitree_g1", "sub", "c.pkl"), os.path.join(tgt, "booster_t1", "sub", "c.pkl"))
    # a.bvh: both robots have it -> skipped; b.bvh: one robot lacks it -> converted
    for r in ("unitree_g1", "booster_t1"):
        os.makedirs(os.path.join(tgt, r), exist_ok=True)
        open(os.path.join(tgt, r, "a.pkl"), "w").write("x")
    open(os.path.join(tgt, "unitree_g1", "b.pkl"), "w").write("x")
    srcs, tgts, skipped = plan(args, ".bvh", lambda n: n.endswith(".bvh"))
    assert [os.path.relpath(s, src) for s in srcs] == ["b.bvh", os.path.join("sub", "c.bvh")] and skipped == 1
    args.override = True
    srcs, _, skipped = plan(args, ".bvh", lambda n: n.endswith(".bvh"))
    assert len(srcs) == 3 and skipped == 0
    # --robot keeps the single-robot layout
    one = _resolve(["--robot", "unitree_g1"])
    one.src_folder, one.tgt_folder = src, tgt
    srcs, tgts, _ = plan(one, ".bvh", lambda n: n.endswith(".bvh"))
    assert tgts[0] == os.path.join(tgt, "a.pkl")
