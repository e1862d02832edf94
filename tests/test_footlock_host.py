"""Foot locking without a GPU: the header, the export and the binding of gmr_motion_footlock, the layout of its struct, the static
stream check of its launches, the chain derivation, the ramp weights, the tiled bit-mask formulation of the runs against the plain
loop (tests/footlock_reference.py), the reference on the GPU test's inputs (tests/footlock_inputs.py), the .npz round trip of the
new keys and the flag of the dataset scripts.

The rounding floor.  The reference run in float64 and in numpy.longdouble (x87 extended, 64-bit mantissa) on the GPU test's inputs
differs by at most (measured here, x86-64):

    case    qpos (rad)   pos (m)    shift (m)
    main    2.98e-15     3.30e-16   2.47e-16
    one     1.95e-15     3.21e-16   2.47e-16
    w0      2.98e-15     3.30e-16   2.47e-16
    limit   7.81e-16     6.51e-17   0

ROUNDING_FLOOR = 3.0e-15 is the worst of them, rounded up; the GPU test allows 16 times that.  (Where numpy.longdouble is no wider
than float64 the measured floor is 0 and the recorded one stands.)"""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import footlock_inputs as fi
from tests import footlock_reference as ref
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units
from tests.util import compiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDING_FLOOR = 3.0e-15   # rad or m: float64 against longdouble, worst over the GPU test's cases (module docstring)


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------ 1: header, export, binding, layout
def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_footlock\s*\(gmr_model \*m, const gmr_footlock_input \*in\);", code)
    assert "gmr_motion_footlock" in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert "gmr_motion_footlock" not in stream_prototypes() and len(stream_prototypes()) == 27         # the stream travels in the struct
    lib = _native.load()
    assert lib.gmr_motion_footlock.restype == C.c_int and len(lib.gmr_motion_footlock.argtypes) == 2
    assert lib.gmr_motion_footlock.argtypes[1]._type_ is _native.FootlockInput
    assert lib.gmr_motion_footlock(None, C.byref(_native.FootlockInput())) == -1   # a null handle is refused before anything else
    assert _native.FOOTLOCK_OUTPUTS == ref.FIELDS
    from gmr_amd import engine
    assert engine.FOOTLOCK_DEFAULTS == ref.DEFAULTS == {"blend_frames": 5, "min_run": 2, "iterations": 8, "damping": 1e-6, "step_cap": 0.2}


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.FootlockInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_footlock_input")].rindex("Layout (LP64)"):]   # (the listing nearest above the struct)
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct gmr_footlock_input \{(.*?)\} gmr_footlock_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_footlock_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 152
    assert listing == {k: getattr(T, k).offset for k in fields}
    assert fields[-8:] == [k + "_out" for k in _native.FOOTLOCK_OUTPUTS] and fields[-9] == "stream"
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_footlock_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_footlock_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_launches_are_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=["gmr_motion_footlock"])
    assert not problems, "\n".join(problems)
    assert syncs == {"gmr_motion_footlock": False}
    us = units()
    r = reachable(us, "gmr_motion_footlock")
    assert {"footlock_plan", "footlock_run"} <= r and "scratch_alloc" not in r and "CallScratch" not in r   # no allocation
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 3                         # three kernels
    assert len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us["footlock_run"])) == 3
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                       # no copy, no memset
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us["gmr_motion_footlock"])


# ------------------------------------------------------------------ 2: chains
def _names(rob, paths, chains):
    return [[rob.jnt_names[p[i]] for i in c] for p, c in zip(paths, chains)]


def test_chains_of_the_g1_feet_are_the_six_leg_hinges():
    rob = fi.robot()
    paths, chains = ref.paths_and_chains(rob, fi.feet_ids())
    for side, got in zip(("left", "right"), _names(rob, paths, chains)):
        assert got == [f"{side}_{j}_joint" for j in ("hip_pitch", "hip_roll", "hip_yaw", "knee", "ankle_pitch", "ankle_roll")]
    assert [rob.body_names[j] for j in paths[0]][-1] == "left_ankle_roll_link" and all(rob.parent[p[0]] == 0 for p in paths)


def test_chains_leave_out_a_joint_two_feet_share():
    """booster_t1's legs hang off the Waist body, not off the root: its hinge lies on both feet's paths and belongs to neither chain."""
    rob = compiled("smplx", "booster_t1").robot
    ids = [list(rob.body_names).index(b) for b in ("left_foot_link", "right_foot_link")]
    paths, chains = ref.paths_and_chains(rob, ids)
    assert [rob.body_names[p[0]] for p in paths] == ["Waist", "Waist"] and rob.jnt_type[paths[0][0]] == ref.JNT_HINGE
    assert all(0 not in c and len(c) == 6 and len(p) == 7 for p, c in zip(paths, chains))
    alone, solo = ref.paths_and_chains(rob, ids[:1])
    assert solo[0] == [0, 1, 2, 3, 4, 5, 6]            # one foot alone: the waist is its own
    with pytest.raises(ValueError, match="EINVAL"):
        ref.paths_and_chains(rob, [ids[0], ids[0]])
    with pytest.raises(ValueError, match="EINVAL"):
        ref.paths_and_chains(rob, [ids[0], rob.nbody])
    with pytest.raises(ValueError, match="EINVAL"):   # the toe hangs off the foot: the foot's chain would be empty
        ref.paths_and_chains(rob, [ids[0], list(rob.body_names).index("left_toe_link")])
    with pytest.raises(ValueError, match="EUNSUPPORTED"):
        r1 = compiled("smplx", "galaxea_r1pro").robot
        ref.paths_and_chains(r1, [r1.nbody - 1])


def test_chain_and_path_limits_on_synthetic_trees(tmp_path):
    """No registry robot reaches the limits: a floating base with one limb of 17 hinges (a chain of more than 16), and one of 3
    hinges and 30 jointless bodies (the tip 33 bodies below the root, more than a path's 32).  One less of either is accepted."""
    for hinges, fixed, word in ((17, 0, "chain of more than 16"), (3, 30, "path longer than 32")):
        rob = fi.synthetic_limb(tmp_path, hinges, fixed, f"over_{hinges}_{fixed}").robot
        assert rob.nbody == hinges + fixed + 1 <= 64
        with pytest.raises(ValueError, match="EUNSUPPORTED: .*" + word):
            ref.paths_and_chains(rob, [rob.nbody - 1])
    for hinges, fixed in ((16, 0), (3, 29)):
        rob = fi.synthetic_limb(tmp_path, hinges, fixed, f"at_{hinges}_{fixed}").robot
        paths, chains = ref.paths_and_chains(rob, [rob.nbody - 1])
        assert len(paths[0]) == hinges + fixed and chains[0] == list(range(hinges))
    rob = fi.synthetic_limb(tmp_path, 17, 0, "mid").robot
    paths, chains = ref.paths_and_chains(rob, [10])          # a body half way down the same limb: ten hinges, fine
    assert len(chains[0]) == 10
    with pytest.raises(ValueError, match="EINVAL"):          # two hinges only
        ref.paths_and_chains(rob, [2])


# ------------------------------------------------------------------ 3: ramps and runs
def test_ramp_weights_on_hand_cases():
    S = ref.smooth
    assert S(0.0) == 0.0 and S(1.0) == 1.0 and S(0.5) == 0.5
    W = 5
    assert ref.ramp_weights(11, 10, None, W) == (S(1.0 - 1 / 6), 0.0)
    assert ref.ramp_weights(15, 10, None, W) == (S(1.0 - 5 / 6), 0.0) and S(1.0 - 5 / 6) > 0
    assert ref.ramp_weights(16, 10, None, W) == (0.0, 0.0)                  # k - e = W + 1: outside
    assert ref.ramp_weights(9, None, 10, W) == (0.0, S(1.0 - 1 / 6))
    assert ref.ramp_weights(3, None, None, W) == (0.0, 0.0)
    assert ref.ramp_weights(11, 10, 12, 0) == (0.0, 0.0)                    # W = 0: no ramp at all
    wm, wp = ref.ramp_weights(12, 10, 14, W)                                # the middle of a gap of three frames
    assert wm == wp == S(1.0 - 2 / 6) and wm + wp > 1.0


def test_a_gap_shorter_than_two_ramps_is_normalised():
    """Two runs with constant shifts (1, 0) and (3, 0) cm around a gap of three frames: the weights add up to more than one there
    and the shift is their weighted mean; at a lone run's side the weight falls to zero and the shift with it."""
    n = 40
    p = np.zeros((n, 3))
    L = np.zeros(n, bool)
    L[10:20] = L[23:30] = True
    p[10:20, 0] = np.where(np.arange(10) % 2 == 0, 0.0, 0.02)      # anchor 0.01: shifts +-0.01
    p[23:30, 0] = 0.0
    p[23, 0] = 0.07                                               # anchor 0.01: the first frame's shift is -0.06
    d, solve, runs = ref.shifts(p, L, np.ones(n, bool), 5, 2)
    assert runs == [(10, 19), (23, 29)]
    S = ref.smooth
    de, df = d[19, 0], d[23, 0]
    assert de == pytest.approx(-0.01) and df == pytest.approx(-0.06)
    for k in (20, 21, 22):
        wm, wp = S(1.0 - (k - 19) / 6), S(1.0 - (23 - k) / 6)
        assert wm + wp > 1.0 and d[k, 0] == (wm * de + wp * df) / (wm + wp) and solve[k]
    assert d[9, 0] == S(1.0 - 1 / 6) * d[10, 0] and d[5, 0] == S(1.0 - 5 / 6) * d[10, 0] and not d[4].any() and not solve[4]
    assert d[34, 0] == S(1.0 - 5 / 6) * d[29, 0] and not solve[35]
    assert not d[:, 2].any()


def test_tiled_masks_equal_the_loop_on_random_sequences():
    rnd = random.Random(11)
    lengths = set()
    for i in range(1500):
        n = rnd.randint(0, 200) if i >= 201 else i   # every length 0 .. 200 once, then random ones
        lengths.add(n)
        p = rnd.choice([0.1, 0.5, 0.9, 0.99])
        L = [rnd.random() < p for _ in range(n)]
        for min_run in (1, 2, 5):
            assert ref.runs_tiled(L, min_run) == ref.runs_loop(L, min_run), (i, n, min_run)
    assert lengths == set(range(201))


def test_tiled_masks_on_the_tile_edges():
    def seq(n, *runs):
        L = [False] * n
        for a, b in runs:
            L[a:b + 1] = [True] * (b - a + 1)
        return L
    for runs in ([(60, 70)], [(63, 63)], [(63, 64)], [(64, 64)], [(0, 63)], [(0, 64)], [(0, 199)], [(10, 150)], [(62, 62), (64, 65)],
                 [(0, 0), (199, 199)], [(127, 128)], [(5, 63), (65, 127), (129, 191)]):
        L = seq(200, *runs)
        assert ref.runs_tiled(L, 1) == ref.runs_loop(L, 1) == list(runs)
    L = seq(130, (63, 64))
    assert ref.runs_tiled(L, 3) == ref.runs_loop(L, 3) == []            # too short, across the edge
    assert ref.runs_tiled([], 1) == ref.runs_loop([], 1) == []
    assert ref.runs_tiled([True] * 64, 1) == [(0, 63)] and ref.runs_tiled([True] * 128, 1) == [(0, 127)]


def test_anchor_is_the_tiled_tree_sum():
    rng = np.random.default_rng(3)
    x, y = rng.normal(size=200), rng.normal(size=200)
    ax, ay = ref.anchor(x, y, 60, 70)
    assert abs(ax - x[60:71].mean()) < 1e-15 and abs(ay - y[60:71].mean()) < 1e-15
    assert ref.anchor(x, y, 5, 5) == (x[5], y[5])
    assert ref.tree_sum([1.0] * 64) == 64.0
    big = [1e16, 1.0] + [0.0] * 62
    assert ref.tree_sum(big) == 1e16 and ref.tree_sum(big[::-1]) == 1e16      # neighbours first: the order is the tree's


# ------------------------------------------------------------------ 4: the reference on the GPU test's inputs
def test_inputs_keep_the_reference_converged():
    """Knees of at least 0.3 rad, shifts of at most 1 cm: the reference's own residual stays below 5e-7 m."""
    rob = fi.robot()
    q = fi.qpos()
    knees = [rob.qpos_adr[b] for b in rob.hinge_bodies() if "knee" in rob.jnt_names[b]]
    assert len(knees) == 2 and q[:, knees].min() >= 0.3
    for b in rob.hinge_bodies():
        if rob.jnt_limited[b]:
            assert rob.jnt_range[b, 0] < q[:, rob.qpos_adr[b]].min() and q[:, rob.qpos_adr[b]].max() < rob.jnt_range[b, 1], rob.jnt_names[b]
    for case in ("main", "one", "w0", "nan"):
        r = fi.reference(case)
        assert float(r["shift_max"].max()) <= 0.01 and float(r["residual_max"].max()) <= 5e-7, case
        assert not r["limit_frames"].any()
    r = fi.reference("limit")
    assert r["limit_frames"][0, 0] > 0 and r["locked_frames"][0, 0] == fi.LIMIT_FRAMES


def test_the_rounding_floor_is_the_recorded_one():
    worst = 0.0
    for case in ("main", "one", "w0", "limit"):
        a, b = fi.reference(case), fi.reference(case, "longdouble")
        for k in ("runs", "locked_frames", "limit_frames"):
            assert np.array_equal(a[k], b[k]), (case, k)
        for k in ("qpos", "pos", "shift"):
            d = np.abs(a[k].astype(np.longdouble) - b[k])
            d = float(np.nanmax(d)) if d.size else 0.0
            print(f"{case:6s} {k:6s} {d:.3e}")
            worst = max(worst, d)
    print(f"rounding floor: measured {worst:.3e}, recorded {ROUNDING_FLOOR:.3e}")
    assert worst <= ROUNDING_FLOOR
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert worst >= ROUNDING_FLOOR / 4    # the recorded figure is not a loose one


# ------------------------------------------------------------------ 5: the .npz round trip and the scripts' flag
def test_save_and_load_tracking_round_trip_the_footlock_stats(tmp_path):
    from gmr_amd import dataset
    from tests.test_contact_host import _fake_track
    assert dataset.FOOTLOCK_STATS == ("runs", "locked_frames", "shift_max", "residual_max", "limit_frames")
    plain = _fake_track()
    d = dict(plain)
    rng = np.random.default_rng(4)
    stats = {"runs": np.array([3, 1], np.int32), "locked_frames": np.array([40, 7], np.int32), "shift_max": rng.random(2),
             "residual_max": rng.random(2) * 1e-9, "limit_frames": np.array([0, 2], np.int32)}
    d["footlock_stats"] = stats
    p, q = str(tmp_path / "with.npz"), str(tmp_path / "plain.npz")
    assert dataset.save_tracking(p, d) and dataset.save_tracking(q, plain)
    got = dataset.load_tracking(p)
    assert set(got) == set(d) and "footlock_stats" not in dataset.load_tracking(q)
    for k, v in stats.items():
        assert np.array_equal(got["footlock_stats"][k], v) and got["footlock_stats"][k].dtype == v.dtype, k
    with np.load(p) as z:
        assert z.files[:14] == ["fps", "body_names", "joint_names", "quat_order"] + list(dataset.TRACK_ARRAYS)


@pytest.mark.parametrize("script", ["bvh_to_robot_dataset", "smplx_to_robot_dataset"])
def test_dataset_scripts_take_lock_feet(script, tmp_path, capsys):
    import argparse
    import importlib
    from gmr_amd.scripts import _walk
    mod = importlib.import_module("gmr_amd.scripts." + script)
    src, tgt, trk = str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "trk")
    os.makedirs(src)
    base = ["--src_folder", src, "--tgt_folder", tgt] + (["--hard_motions"] if script.startswith("smplx") else [])
    track = ["--track_fps", "50", "--track_folder", trk]
    feet = ",".join(fi.FEET)
    assert mod.main(base + track + ["--contact_bodies", feet, "--lock_feet"]) == 0   # (an empty folder: nothing to convert)
    for flags in (track + ["--lock_feet"], ["--lock_feet"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.main(base + flags)
        assert e.value.code == 2 and "--contact_bodies" in capsys.readouterr().err, flags
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    off = ap.parse_args(["--track_fps", "50", "--track_folder", "/trk", "--contact_bodies", "a,b"])
    off.robot_list = None
    _walk.resolve_track(ap, off)
    assert "lock_feet" not in off.contact_kw             # without the flag nothing is passed on
    on = ap.parse_args(["--track_fps", "50", "--track_folder", "/trk", "--contact_bodies", "a,b", "--lock_feet"])
    on.robot_list = None
    _walk.resolve_track(ap, on)
    assert on.contact_kw["lock_feet"] is True and on.contact_kw["contact_bodies"] == ["a", "b"]
