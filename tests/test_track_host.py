"""The tracking export, the parts that need no GPU: the resampling plan against a plain loop, the two exports and the ctypes
layout of their input struct, the .npz round trip with its route through MotionWriter, and the two flags of the dataset scripts."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmr_motion_track", "gmr_group_motion_track")
RATES = [(30.0, 50.0), (120.0, 30.0), (30.0, 30.0), (29.97, 50.0)]
LENGTHS = [0, 1, 2, 3, 4, 121]


def _plan_loop(lengths, fps_in, fps_out):
    """The contract's plan, clip by clip."""
    offs, ratios = [0], []
    for T, fin in zip(lengths, fps_in):
        ratio = fin / fps_out
        M = 0 if T == 0 else int(math.floor((T - 1) / ratio + 1e-6)) + 1
        offs.append(offs[-1] + M)
        ratios.append(ratio)
    return offs, ratios


@pytest.mark.parametrize("fps_in,fps_out", RATES)
def test_track_plan_matches_the_plain_loop(fps_in, fps_out):
    from gmr_amd.schedule import track_plan
    lengths = LENGTHS + [5, 0, 7]  # ... and an empty clip between two that are not
    offs = np.concatenate([[0], np.cumsum(lengths)])
    out, ratio = track_plan(offs, fps_in, fps_out)
    want_offs, want_ratio = _plan_loop(lengths, [fps_in] * len(lengths), fps_out)
    assert out.dtype == np.int64 and ratio.dtype == np.float64 and out.shape == (len(lengths) + 1,) and ratio.shape == (len(lengths),)
    assert out.tolist() == want_offs and ratio.tolist() == want_ratio
    M = np.diff(out)
    for T, m, r in zip(lengths, M, ratio):
        assert (m == 0) == (T == 0)
        if m:
            assert (m - 1) * r <= T - 1 + 1e-6  # the last output frame reads no source frame past the clip's last
    if fps_in == fps_out:
        assert M.tolist() == lengths
    if (fps_in, fps_out) == (120.0, 30.0):
        assert M[LENGTHS.index(121)] == 31 and 30 * ratio[0] == 120.0  # the last source frame is an output frame


def test_track_plan_takes_per_clip_rates_and_refuses_bad_ones():
    from gmr_amd.schedule import track_plan
    lengths, fin = [10, 0, 121, 1], [30.0, 60.0, 120.0, 29.97]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    out, ratio = track_plan(offs, fin, 50)
    want_offs, want_ratio = _plan_loop(lengths, fin, 50.0)
    assert out.tolist() == want_offs and ratio.tolist() == want_ratio
    assert np.array_equal(track_plan(offs, np.float32(30), 50)[0], track_plan(offs, [30.0] * 4, 50)[0])
    for bad in ((30, 0), (30, -1.0), (0, 50), ([30, 30, -2, 30], 50), (30, float("nan")), ([30, 30], 50)):
        with pytest.raises(ValueError):
            track_plan(offs, *bad)
    with pytest.raises(ValueError):
        track_plan([0, 5, 3], 30, 50)


def test_track_exports_are_declared_and_bound():
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+gmr_motion_track\s*\(gmr_model \*m, const gmr_track_input \*in, void \*stream\)", src)
    assert re.search(r"\bint\s+gmr_group_motion_track\s*\(gmr_group \*g, const gmr_track_input \*inputs, void \*stream\)", src)
    assert re.search(r"#define GMR_ABI_VERSION 5\b", src)
    for name in NEW:
        assert name in _native.EXPORTS
    lib = _native.load()
    assert lib.gmr_abi_version() == 5
    for name in NEW:
        assert hasattr(lib, name)
    # null handles are refused before anything else (no device needed)
    ti = _native.TrackInput()
    assert lib.gmr_motion_track(None, ctypes.byref(ti), None) == -1
    assert lib.gmr_group_motion_track(None, ctypes.byref(ti), None) == -1


def test_track_input_layout_matches_the_c_struct(tmp_path):
    """ctypes.sizeof and the offsets of TrackInput against the struct as a C compiler lays it out from the header."""
    from gmr_amd import _native
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    T = _native.TrackInput
    fields = [name for name, _ in T._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gmr_track_input));\n'
                   + "".join(f'  printf(" %zu", offsetof(gmr_track_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert ctypes.sizeof(T) == got[0] == 136
    assert [getattr(T, n).offset for n in fields] == got[1:]
    assert fields[-10:] == [k + "_out" for k in _native.TRACK_OUTPUTS]


def _fake_track(M=7, nd=5, nb=3, seed=0):
    from gmr_amd import dataset
    rng = np.random.default_rng(seed)
    shapes = {"joint_pos": (M, nd), "joint_vel": (M, nd), "root_pos": (M, 3), "root_rot": (M, 4), "root_lin_vel": (M, 3),
              "root_ang_vel": (M, 3), "body_pos_w": (M, nb, 3), "body_quat_w": (M, nb, 4), "body_lin_vel_w": (M, nb, 3),
              "body_ang_vel_w": (M, nb, 3)}
    assert tuple(shapes) == dataset.TRACK_ARRAYS
    d = {"fps": 50.0}
    for k, sh in shapes.items():
        d[k] = rng.normal(size=sh).astype(np.float32 if k.startswith("body_") else np.float64)
    d.update(body_names=[f"b{i}" for i in range(nb)], joint_names=[f"joint_{i}" for i in range(nd)], quat_order="xyzw")
    return d, shapes


def test_save_tracking_round_trip_and_the_writer_route(tmp_path):
    from gmr_amd import dataset
    d, shapes = _fake_track()
    p = str(tmp_path / "sub" / "clip.npz")
    assert dataset.save_tracking(p, d) is True and os.path.exists(p)
    got = dataset.load_tracking(p)
    assert set(got) == set(d) == set(dataset.TRACK_ARRAYS) | {"fps", "body_names", "joint_names", "quat_order"}
    for k, sh in shapes.items():
        assert got[k].shape == sh and got[k].dtype == d[k].dtype and np.array_equal(got[k], d[k]), k
    assert got["fps"] == 50.0 and got["body_names"] == d["body_names"] and got["joint_names"] == d["joint_names"]
    assert got["quat_order"] == "xyzw"
    with np.load(p) as z:  # uncompressed, and nothing that needs pickle
        assert all(info.compress_type == 0 for info in z.zip.infolist())
    # skipped when the file exists, unless override
    other, _ = _fake_track(seed=1)
    assert dataset.save_tracking(p, other) is False
    assert np.array_equal(dataset.load_tracking(p)["root_pos"], d["root_pos"])
    assert dataset.save_tracking(p, other, override=True) is True
    assert np.array_equal(dataset.load_tracking(p)["root_pos"], other["root_pos"])
    # MotionWriter: a .npz path takes a tracking dict, a .pkl path beside it a motion dict as before
    motion = {"fps": 30, "root_pos": np.zeros((4, 3)), "root_rot": np.tile([0.0, 0, 0, 1], (4, 1)), "dof_pos": np.zeros((4, 5)),
              "local_body_pos": np.zeros((4, 3, 3), np.float32), "link_body_list": ["a", "b", "c"]}
    paths = [str(tmp_path / "w" / "a.npz"), str(tmp_path / "w" / "a.pkl"), p]
    with dataset.MotionWriter(workers=2) as w:
        w.submit([d, motion, d], paths)
    assert (w.written, w.skipped) == (2, 1)
    assert np.array_equal(dataset.load_tracking(paths[0])["body_quat_w"], d["body_quat_w"])
    assert np.array_equal(dataset.load_robot_motion(paths[1])[2], motion["root_pos"])


@pytest.mark.parametrize("script", ["bvh_to_robot_dataset", "smplx_to_robot_dataset"])
def test_dataset_scripts_take_the_two_track_flags_together(script, tmp_path, capsys):
    import importlib
    mod = importlib.import_module("gmr_amd.scripts." + script)
    src, tgt, trk = str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "trk")
    os.makedirs(src)
    base = ["--src_folder", src, "--tgt_folder", tgt] + (["--hard_motions"] if script.startswith("smplx") else [])
    # both flags: accepted (an empty folder: nothing to convert, no device touched); neither: as before
    assert mod.main(base + ["--track_fps", "50", "--track_folder", trk]) == 0
    assert mod.main(base) == 0
    for one in (["--track_fps", "50"], ["--track_folder", trk], ["--track_fps", "0", "--track_folder", trk]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.main(base + one)
        assert e.value.code == 2 and "--track_f" in capsys.readouterr().err


def test_track_path_mirrors_the_target_below_the_track_folder():
    import argparse
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    args = ap.parse_args(["--track_fps", "50", "--track_folder", "/trk"])
    assert args.track_fps == 50.0 and args.track_folder == "/trk"
    args.tgt_folder = "/out"
    assert _walk.track_path(args, "/out/sub/clip_1.pkl") == "/trk/sub/clip_1.npz"
    assert _walk.track_path(args, "/out/unitree_g1/sub/clip_1.pkl") == "/trk/unitree_g1/sub/clip_1.npz"
    none = ap.parse_args([])
    assert none.track_fps is None and none.track_folder is None
