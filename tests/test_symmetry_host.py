"""Mirror augmentation without a GPU: the symmetry plan of gmr_amd/symmetry.py on every robot pack, the numpy FK identity it
promises, its refusals, the header, the export and the binding of gmr_motion_mirror, the layout of its struct, the static stream check
of its launch, the numpy reference against its 50-digit evaluator (tests/mirror_reference.py, tests/mirror_inputs.py) and the dataset
scripts' flags."""
import copy
import ctypes as C
import dataclasses
import glob
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gmr_amd import symmetry as SY
from gmr_amd.mjcf import ROOT_DOFS_FREE, RobotModel
from tests import dynamics_reference as R
from tests import mirror_inputs as mi
from tests import mirror_reference as MR
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gmr_motion_mirror"
PACKS = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(ROOT, "gmr_amd", "packs", "robots", "*.json")))

# Per robot and tolerance (all three tolerances alike): ("paired", unpaired bodies, residual_pos, residual_axis, range_mismatch,
# worst FK mismatch of the mirror over 2000 poses) or ("refused", the body the error names, the mismatch it reports: position in
# metres or axis components).  Recorded figures are rounded up; the tests re-measure them and fail if one is smaller than the measured.
EXACT = ("paired", [], 0.0, 0.0, 0.0, 0.0)
BERKELEY = ("paired", [], 7e-14, 8e-13, 7e-13, 1.6e-13)
TABLE = {
    "booster_k1": {1e-6: EXACT, 1e-3: EXACT},
    "booster_t1": {1e-6: EXACT, 1e-3: EXACT},
    "fourier_n1": {1e-6: ("paired", ["camera_link"], 0.0, 0.0, 0.0, 0.0), 1e-3: ("paired", ["camera_link"], 0.0, 0.0, 0.0, 0.0)},
    "berkeley_humanoid_lite": {1e-6: BERKELEY, 1e-3: BERKELEY},
    "unitree_g1": {1e-6: ("refused", "left_shoulder_pitch_link", "pos", 1.0001e-5), 1e-3: ("paired", ["imu_in_torso"], 1.0001e-5, 0.0, 0.0, 1.0001e-5)},
    "unitree_g1_with_hands": {1e-6: ("refused", "left_shoulder_pitch_link", "pos", 1.0001e-5), 1e-3: ("paired", [], 1.0001e-5, 0.0, 0.0, 1.0001e-5)},
    "engineai_pm01": {1e-6: ("refused", "LINK_HIP_ROLL_L", "pos", 1.0001e-6), 1e-3: ("refused", "LINK_ELBOW_PITCH_L", "axis", 5.5e-3)},
    "kuavo_s45": {1e-6: ("refused", "leg_l3_link", "pos", 1.0001e-3), 1e-3: ("refused", "leg_l3_link", "pos", 1.0001e-3)},
    "galaxea_r1pro": {1e-6: ("refused", "torso_link3", "pos", 2.02e-4), 1e-3: ("refused", "left_arm_link2", "pos", 1.03e-3)},   # (its planar base taken as free)
    "hightorque_hi": {1e-6: ("refused", "head_pitch_link", "pos", 3.1e-2), 1e-3: ("refused", "head_pitch_link", "pos", 3.1e-2)},
    "stanford_toddy": {1e-6: ("refused", "hip_yaw_link", "pos", 3.9e-2), 1e-3: ("refused", "hip_yaw_link", "pos", 3.9e-2)},
}
EXACT_ROBOTS = ["booster_k1", "booster_t1", "fourier_n1", "berkeley_humanoid_lite"]
PLANNED = [r for r in PACKS if TABLE[r][1e-3][0] == "paired"]
POSES = 2000


def pack(robot):
    with open(os.path.join(ROOT, "gmr_amd", "packs", "robots", robot + ".json")) as f:
        return json.load(f)


def model(robot, free=True):
    rob = RobotModel.from_dict(pack(robot))
    return dataclasses.replace(rob, root_dofs=ROOT_DOFS_FREE) if free and rob.planar_base else rob


def poses(rob, n=POSES, seed=0):
    rng = np.random.default_rng(seed)
    q = np.zeros((n, rob.nq))
    q[:, :3] = rng.normal(size=(n, 3))
    q[:, 3:7] = rng.normal(size=(n, 4))
    q[:, 7:] = rng.uniform(-np.pi, np.pi, size=(n, rob.nq - 7))
    return q


def fk_mismatch(rob, plan, q):
    """max |M X[b] - X'[partner[b]]| over the paired bodies: the FK of the mirrored poses against the reflected FK of the poses."""
    X, _ = R.fk(rob, q)
    X2, _ = R.fk(rob, SY.mirror_rows(plan, q))
    ok = plan.body_partner >= 0
    return float(np.abs(X[:, ok] * SY.M - X2[:, plan.body_partner[ok]]).max())


# ------------------------------------------------------------------ 1: the plan on every pack robot
def test_the_table_names_every_pack_robot():
    assert sorted(TABLE) == PACKS and len(PACKS) == 11


@pytest.mark.parametrize("tol", [1e-6, 1e-3])
@pytest.mark.parametrize("robot", PACKS)
def test_every_pack_robot_is_planned_or_refused_as_recorded(robot, tol):
    want = TABLE[robot][tol]
    rob = model(robot)
    if want[0] == "refused":
        with pytest.raises(SY.SymmetryError) as e:
            SY.plan_symmetry(rob, tol, tol, tol)
        text = str(e.value)
        print(text)
        if want[1] is not None:
            assert f"body {want[1]!r} has no mirror partner" in text
        got = float(re.search(r"position mismatch ([0-9.e+-]+) m" if want[2] == "pos" else r"axis mismatch ([0-9.e+-]+) ", text).group(1))
        assert tol * (1.0 - 1e-3) <= got <= want[3], (got, want[3])   # (printed with four digits) the recorded figure covers the measured one
        assert got > 0.9 * want[3]                            # ... and is that figure, not a loose one
        return
    plan = SY.plan_symmetry(rob, tol, tol, tol)
    print(f"{robot} at {tol:g}: residual_pos {plan.residual_pos:.3e} residual_axis {plan.residual_axis:.3e} range_mismatch {plan.range_mismatch:.3e} "
          f"fk_bound {plan.fk_bound:.3e} unpaired {plan.unpaired}")
    assert plan.unpaired == want[1]
    assert plan.residual_pos <= want[2] and plan.residual_axis <= want[3] and plan.range_mismatch <= want[4]
    assert plan.residual_pos <= tol and plan.residual_axis <= tol and plan.range_mismatch <= tol
    for b, n in enumerate(plan.body_names):                   # an unpaired body carries no qpos column, nor does anything below it
        if plan.body_partner[b] < 0:
            assert n in plan.unpaired and rob.qpos_adr[b] < 0
    assert sorted(plan.col_src[7:].tolist()) == list(range(7, rob.nq))   # a permutation of the hinge columns


def test_a_planar_base_is_refused_as_not_implemented():
    rob = model("galaxea_r1pro", free=False)
    assert rob.planar_base
    with pytest.raises(NotImplementedError):
        SY.plan_symmetry(rob)


@pytest.mark.parametrize("robot", PLANNED)
def test_fk_of_the_mirrored_pose_is_the_reflected_fk_within_fk_bound(robot):
    rob = model(robot)
    plan = SY.plan_symmetry(rob)
    got = fk_mismatch(rob, plan, poses(rob))
    print(f"{robot}: worst FK mismatch of the mirror {got:.3e} m over {POSES} poses, fk_bound {plan.fk_bound:.3e} m")
    assert got <= plan.fk_bound
    assert got <= TABLE[robot][1e-3][5]                       # the recorded figure is not smaller than the measured one
    if robot in EXACT_ROBOTS:
        assert plan.fk_bound <= 2e-12
    else:
        assert 5e-6 < got and plan.fk_bound < 2e-4            # G1: the shoulders' 1e-5 m shows, and the bound is not vacuous


def test_the_pairing_is_what_the_names_say_on_g1_and_k1():
    for robot in ("unitree_g1", "booster_k1"):
        rob = model(robot)
        plan = SY.plan_symmetry(rob)
        names = plan.body_names
        for b, n in enumerate(names):
            p = int(plan.body_partner[b])
            if p < 0:
                continue
            swapped = n.replace("left", "@").replace("right", "left").replace("@", "right").replace("Left", "@").replace("Right", "Left").replace("@", "Right")
            if swapped in names:
                assert names[p] == swapped, (n, names[p])
    g1 = SY.plan_symmetry(model("unitree_g1"))
    rob = model("unitree_g1")
    col = {rob.jnt_names[b]: int(rob.qpos_adr[b]) for b in rob.hinge_bodies()}
    sign_of = lambda j: float(g1.col_sign[col[j]])            # noqa: E731
    assert g1.col_src[col["left_hip_roll_joint"]] == col["right_hip_roll_joint"]
    assert sign_of("left_hip_pitch_joint") == 1.0 and sign_of("left_knee_joint") == 1.0       # pitch axes (y) copy the angle
    assert sign_of("left_hip_roll_joint") == -1.0 and sign_of("left_hip_yaw_joint") == -1.0   # roll (x) and yaw (z) negate it
    assert g1.col_src[col["waist_yaw_joint"]] == col["waist_yaw_joint"] and sign_of("waist_yaw_joint") == -1.0   # on the plane: its own image


# ------------------------------------------------------------------ 2: involution, determinism, JSON, names
@pytest.mark.parametrize("robot", PLANNED)
def test_involution_determinism_and_json_round_trip(robot, tmp_path):
    rob = model(robot)
    plan, again = SY.plan_symmetry(rob), SY.plan_symmetry(rob)
    assert plan == again and plan is not again
    p = plan.body_partner
    for b in range(rob.nbody):
        if p[b] >= 0:
            assert p[p[b]] == b
    src, sg = plan.col_src, plan.col_sign
    assert np.array_equal(src[src], np.arange(rob.nq)) and np.array_equal(sg[src], sg) and set(np.abs(sg).tolist()) == {1.0}
    q = poses(rob, 16, seed=3)
    assert np.array_equal(SY.mirror_rows(plan, SY.mirror_rows(plan, q)), q)                   # mirroring twice: the input, bit for bit
    back = SY.SymmetryPlan.from_json(json.loads(json.dumps(plan.to_json())))
    assert back == plan and back.fk_bound == plan.fk_bound and np.array_equal(back.col_sign, plan.col_sign)
    assert SY.SymmetryPlan.from_json(json.dumps(plan.to_json())) == plan                      # (the text is accepted too)
    SY.save_plan(str(tmp_path / "plan.json"), plan)
    assert SY.load_plan(str(tmp_path / "plan.json")) == plan
    plan.check_robot(rob)
    with pytest.raises(SY.SymmetryError):
        plan.check_robot(model("booster_t1" if robot != "booster_t1" else "booster_k1"))


def test_from_json_checks_the_involution_and_the_column_bounds_again():
    plan = SY.plan_symmetry(model("booster_k1"))
    d = plan.to_json()
    nq = len(d["col_src"])
    for edit, what in [(lambda e: e["col_src"].__setitem__(8, nq), "col_src must hold"), (lambda e: e["col_src"].__setitem__(8, 3), "col_src must hold"),
                       (lambda e: e["col_src"].__setitem__(7, e["col_src"][8]), "not an involution"),
                       (lambda e: e["col_sign"].__setitem__(nq - 1, 0.5), "col_sign must hold"),
                       (lambda e: e["col_sign"].__setitem__(int(np.flatnonzero(np.array(e["col_src"]) != np.arange(nq))[0]), -1.0 * e["col_sign"][int(np.flatnonzero(np.array(e["col_src"]) != np.arange(nq))[0])]), "not an involution"),
                       (lambda e: e["body_partner"].__setitem__(1, 2 if e["body_partner"][2] != 1 else 3), "not an involution"),
                       (lambda e: e["body_partner"].__setitem__(0, 1), "root is its own partner"),
                       (lambda e: e["col_src"].__setitem__(2, 1), "root columns"),
                       (lambda e: e.__setitem__("format", "other"), "not a gmr_amd symmetry plan")]:
        e = copy.deepcopy(d)
        edit(e)
        with pytest.raises(SY.SymmetryError, match=what):
            SY.SymmetryPlan.from_json(e)


def test_mirror_names_swaps_sides_and_refuses_an_unpaired_body():
    g1 = SY.plan_symmetry(model("unitree_g1"))
    feet = ["left_ankle_roll_link", "right_ankle_roll_link", "pelvis"]
    assert g1.mirror_names(feet) == ["right_ankle_roll_link", "left_ankle_roll_link", "pelvis"]
    assert g1.mirror_names(g1.mirror_names(feet)) == feet
    with pytest.raises(SY.SymmetryError, match="imu_in_torso"):
        g1.mirror_names(["imu_in_torso"])
    with pytest.raises(KeyError):
        g1.mirror_names(["no_such_body"])


# ------------------------------------------------------------------ 3: the refusals, on packs edited in memory
def _edited(robot, edit):
    d = pack(robot)
    edit({b["name"]: b for b in d["bodies"]})
    return RobotModel.from_dict(d)


def test_a_hinge_bearing_body_moved_off_the_plane_is_refused_with_both_mismatches():
    def move(bodies):
        bodies["left_knee_link"]["pos"][1] += 0.01
    with pytest.raises(SY.SymmetryError) as e:
        SY.plan_symmetry(_edited("unitree_g1", move))
    text = str(e.value)
    assert "'left_knee_link' has no mirror partner" in text and "nearest candidate is 'right_knee_link'" in text
    assert "position mismatch 1.000e-02 m" in text and "axis mismatch 0.000e+00" in text
    SY.plan_symmetry(_edited("unitree_g1", move), tol_pos=0.011)          # a looser tolerance is the user's way out


def test_a_tilted_axis_is_refused():
    def tilt(bodies):
        bodies["left_knee_link"]["joint"]["axis"] = [0.0, float(np.cos(0.01)), float(np.sin(0.01))]
    with pytest.raises(SY.SymmetryError, match=r"'left_knee_link' has no mirror partner.*axis mismatch 1\.000e-02"):
        SY.plan_symmetry(_edited("unitree_g1", tilt))


def test_a_one_sided_range_is_refused_and_nothing_is_clamped():
    def widen(bodies):
        bodies["left_knee_link"]["joint"]["range"][1] += 0.1
    with pytest.raises(SY.SymmetryError, match=r"range of 'left_knee_link'.*mismatch 1\.000e-01 rad"):
        SY.plan_symmetry(_edited("unitree_g1", widen))
    plan = SY.plan_symmetry(_edited("unitree_g1", widen), tol_range=0.2)
    assert abs(plan.range_mismatch - 0.1) < 1e-12
    q = poses(model("unitree_g1"), 4)
    assert np.array_equal(np.sort(np.abs(SY.mirror_rows(plan, q)[:, 7:]), axis=1), np.sort(np.abs(q[:, 7:]), axis=1))   # values far outside any range pass

    def unlimit(bodies):
        bodies["left_knee_link"]["joint"]["limited"] = False
    with pytest.raises(SY.SymmetryError, match="'left_knee_link' is unlimited and its partner 'right_knee_link' is not"):
        SY.plan_symmetry(_edited("unitree_g1", unlimit))


def test_a_hinge_free_leaf_off_the_plane_stays_unpaired_and_a_missing_limb_is_refused():
    def shift(bodies):
        bodies["imu_in_torso"]["pos"][1] = 0.5
    assert SY.plan_symmetry(_edited("unitree_g1", shift)).unpaired == ["imu_in_torso"]
    d = pack("booster_k1")
    rob = RobotModel.from_dict(d)
    leaf = max(b for b in range(rob.nbody) if rob.jnt_type[b] == 1 and b not in set(rob.parent.tolist()))   # the last hinge leaf
    del d["bodies"][leaf]
    d["nq"], d["nv"] = d["nq"] - 1, d["nv"] - 1
    assert all(b["parent"] < leaf for b in d["bodies"])
    with pytest.raises(SY.SymmetryError, match="has no free child with the same joint type|has no mirror partner"):
        SY.plan_symmetry(RobotModel.from_dict(d))


# ------------------------------------------------------------------ 4: header, export, binding, layout
def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_mirror\s*\(gmr_model \*m, const gmr_mirror_input \*in\);", code)
    assert ENTRY in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert ENTRY not in stream_prototypes() and len(stream_prototypes()) == 27                        # the stream travels in the struct
    assert re.search(r"^ \*   gmr_motion_mirror\s+\(no counterpart in the reference\)", src, flags=re.M)
    assert re.search(r"^#define GMR_MIRROR_WORLD 0$", src, flags=re.M) and re.search(r"^#define GMR_MIRROR_CLIP_START 1$", src, flags=re.M)
    assert _native.MIRROR_MODES == {"world": 0, "start": 1} and _native.MIRROR_MAX_NQ == 64
    lib = _native.load()
    assert lib.gmr_motion_mirror.restype == C.c_int and len(lib.gmr_motion_mirror.argtypes) == 2
    assert lib.gmr_motion_mirror.argtypes[1]._type_ is _native.MirrorInput
    assert lib.gmr_motion_mirror(None, C.byref(_native.MirrorInput())) == -1   # a null handle is refused before anything else
    assert lib.gmr_abi_version() == 5


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.MirrorInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_mirror_input")].rindex("Layout (LP64)"):]
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*#define GMR_MIRROR_WORLD 0\s*#define GMR_MIRROR_CLIP_START 1\s*"
                 r"typedef struct gmr_mirror_input \{(.*?)\} gmr_mirror_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_mirror_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 72
    assert listing == {k: getattr(T, k).offset for k in fields}
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_mirror_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_mirror_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_launch_is_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=[ENTRY])
    assert not problems, "\n".join(problems)
    assert syncs == {ENTRY: False}
    us = units()
    r = reachable(us, ENTRY)
    assert "mirror_run" in r and "scratch_alloc" not in r and "CallScratch" not in r                      # no allocation
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 1                      # one launch
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                    # no copy, no memset
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us[ENTRY])
    body = us[ENTRY]
    assert "hipLaunchKernelGGL" not in body and "hipSetDevice" not in body                                # the entry only checks ...
    assert body.index("in->n_frames == 0 || in->n_seq == 0") < body.index("in->qpos_out == in->qpos") < body.index("mirror_run(")   # ... and refuses first


def test_the_kernel_file_has_no_atomics_no_lds_no_barrier_and_contraction_is_off():
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "mirror_kernel.hip.h")) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic", code, flags=re.I) and "__syncthreads" not in code and "__shared__" not in code
    body = code[code.index("motion_mirror_kernel(MirrorArgs A)"):]
    assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1
    assert not re.search(r"\b(sin|cos|atan2|sincos)\s*\(", code)                                          # no trigonometric function


# ------------------------------------------------------------------ 5: the numpy reference
@pytest.mark.parametrize("robot", mi.ROBOTS)
def test_the_recorded_floor_covers_the_gpu_cases_own_rows(robot):
    got = MR.measure_floor(mi.plan(robot), mi.qpos(robot), mi.OFFS)
    print(f"{robot}: worst |numpy - 50 digits| on the root columns: {got}, recorded {MR.FLOAT_WORST[robot]}")
    for k, v in got.items():
        assert v <= MR.FLOAT_WORST[robot][k] <= 4.0 * max(v, 1e-16), k     # covered, and not by a loose figure
    q, offs = mi.vertical(robot)
    up = MR.measure_floor(mi.plan(robot), q, offs)                          # the psi = 0 branch agrees with the 50-digit evaluator's
    assert up["pos"] <= MR.FLOAT_WORST[robot]["pos"] and up["quat"] <= MR.FLOAT_WORST[robot]["quat"]
    cp, sp, c2, s2 = MR.heading(q[[0, 5], 3:7])
    assert cp.tolist() == [1.0, 1.0] and sp.tolist() == [0.0, 0.0] and c2.tolist() == [1.0, 1.0] and s2.tolist() == [0.0, 0.0]


def test_the_reference_modes_agree_with_the_host_mirror_and_with_each_other():
    robot = "booster_k1"
    plan, q = mi.plan(robot), mi.qpos(robot)
    w = mi.reference(robot, "world")
    assert np.array_equal(w, SY.mirror_rows(plan, q))                       # OFFS covers every row
    assert np.array_equal(MR.world_clips(plan, w, mi.OFFS), q)              # an involution, bit for bit
    s = mi.reference(robot, "start")
    assert np.array_equal(s[:, 7:], w[:, 7:]) and np.array_equal(s[:, 2], q[:, 2])
    for k, T in enumerate(mi.LENS):                                         # a mirrored clip starts where the original does, facing the same way
        if T:
            a = int(mi.OFFS[k])
            assert np.abs(s[a, :3] - q[a, :3]).max() <= MR.bound(robot, "pos")
            h0, h1 = MR.heading(q[a:a + 1, 3:7]), MR.heading(s[a:a + 1, 3:7])
            assert abs(h0[0][0] - h1[0][0]) <= 1e-15 and abs(h0[1][0] - h1[1][0]) <= 1e-15
    # gaps: rows outside every clip keep the fill
    gaps = np.array([2, 5, 5, 40], np.int64)
    out = MR.clip_start(plan, q, gaps, fill=7.0)
    assert np.all(out[:2] == 7.0) and np.all(out[40:] == 7.0) and not np.any(out[2:40] == 7.0)


# ------------------------------------------------------------------ 6: the scripts' flags
def _parser():
    import argparse
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default=None)
    _walk.add_common_flags(ap)
    return ap, _walk


def test_the_dataset_scripts_flags_parse_and_plan_on_the_host(tmp_path):
    ap, _walk = _parser()
    off = ap.parse_args([])
    _walk.resolve_robots(ap, off)
    _walk.resolve_track(ap, off)
    assert off.mirror is False and off.mirror_about == "start" and off.mirror_plan is None and off.mirror_kw == {}
    on = ap.parse_args(["--mirror", "--mirror_about", "world"])
    _walk.resolve_robots(ap, on)
    _walk.resolve_track(ap, on)
    kw = on.mirror_kw["mirror"]
    assert kw["about"] == "world" and kw["plan"] == SY.plan_symmetry(model("unitree_g1"))
    both = ap.parse_args(["--mirror", "--robots", "unitree_g1,booster_k1"])
    _walk.resolve_robots(ap, both)
    _walk.resolve_track(ap, both)
    assert sorted(both.mirror_kw["mirror"]["plan"]) == ["booster_k1", "unitree_g1"] and both.mirror_kw["mirror"]["about"] == "start"
    SY.save_plan(str(tmp_path / "k1.json"), SY.plan_symmetry(model("booster_k1")))
    filed = ap.parse_args(["--mirror", "--robot", "booster_k1", "--mirror_plan", str(tmp_path / "k1.json")])
    _walk.resolve_robots(ap, filed)
    _walk.resolve_track(ap, filed)
    assert filed.mirror_kw["mirror"]["plan"] == SY.plan_symmetry(model("booster_k1"))
    assert _walk.mirror_path("out/a/walk.pkl") == "out/a/walk_mirror.pkl"
    for bad in (["--mirror_plan", "x.json"], ["--mirror", "--robot", "unitree_g1", "--mirror_plan", str(tmp_path / "k1.json")],
                ["--mirror", "--mirror_about", "sideways"]):
        args = None
        with pytest.raises(SystemExit):
            args = ap.parse_args(bad)
            _walk.resolve_robots(ap, args)
            _walk.resolve_track(ap, args)


@pytest.mark.parametrize("script", ["smplx_to_robot_dataset", "bvh_to_robot_dataset"])
def test_a_refused_robot_ends_the_script_before_a_file_is_read(script, tmp_path, capsys):
    import importlib
    mod = importlib.import_module("gmr_amd.scripts." + script)
    src = tmp_path / "in"
    src.mkdir()
    (src / "clip.npz").write_bytes(b"not a file anyone could read")
    (src / "clip.bvh").write_text("not a file anyone could read")
    with pytest.raises(SystemExit) as e:
        mod.main(["--src_folder", str(src), "--tgt_folder", str(tmp_path / "out"), "--robot", "stanford_toddy", "--mirror"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "stanford_toddy: body 'hip_yaw_link' has no mirror partner" in err and "position mismatch 3.800e-02 m" in err
    assert not (tmp_path / "out").exists()
