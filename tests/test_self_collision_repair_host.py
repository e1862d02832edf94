"""Self-collision repair without a GPU: the header, the export and the binding of gmr_motion_self_collision_repair, the layout of its
struct, the static stream check of its launches, `collision.movable_mask`, the gradient of the contract's step 5 against central
differences of the reference's own clearance, the reference's float64-against-extended floor, and the conditions of the issue on
the reference (tests/self_collision_repair_reference.py, tests/self_collision_repair_inputs.py).

`unitree_g1_with_hands` and the thin synthetic chains are not cases here (tests/self_collision_repair_inputs.py says why)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gmr_amd import collision
from tests import self_collision_inputs as ci
from tests import self_collision_reference as SR
from tests import self_collision_repair_inputs as ri
from tests import self_collision_repair_reference as RR
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gmr_motion_self_collision_repair"
STRUCT = "gmr_self_collision_repair_input"


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------ 1: header, export, binding, layout
def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native, engine
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint " + ENTRY + r"\s*\(gmr_model \*m, const " + STRUCT + r" \*in\);", code)
    assert ENTRY in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert ENTRY not in stream_prototypes() and len(stream_prototypes()) == 27                        # the stream travels in the struct
    assert re.search(r"^ \*   " + ENTRY + r"\s+\(no counterpart in the reference\)", src, flags=re.M)
    lib = _native.load()
    f = getattr(lib, ENTRY)
    assert f.restype == C.c_int and len(f.argtypes) == 2 and f.argtypes[1]._type_ is _native.SelfCollisionRepairInput
    assert f(None, C.byref(_native.SelfCollisionRepairInput())) == -1     # a null handle is refused before anything else
    assert engine.SELF_COLLISION_REPAIR_FIELDS == _native.SELF_COLLISION_REPAIR_FRAME_OUTPUTS + _native.SELF_COLLISION_REPAIR_STATS
    assert engine.SELF_COLLISION_REPAIR_DEFAULTS == {"iterations": RR.ITERATIONS, "damping": RR.DAMPING, "step_cap": RR.STEP_CAP,
                                                     "resolve_tol": RR.RESOLVE_TOL}


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.SelfCollisionRepairInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct " + STRUCT)].rindex("Layout (LP64)"):]   # (the listing nearest above the struct)
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct " + STRUCT + r" \{(.*?)\} " + STRUCT + ";", src, flags=re.S)
    assert m, "the layout listing in front of " + STRUCT
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 200
    assert listing == {k: getattr(T, k).offset for k in fields}
    n_out = len(_native.SELF_COLLISION_REPAIR_OUTPUTS)
    assert fields[-n_out:] == [k + "_out" for k in _native.SELF_COLLISION_REPAIR_OUTPUTS] and fields[-n_out - 1] == "stream"
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    f'  printf("%zu", sizeof({STRUCT}));\n'
                    + "".join(f'  printf(" %zu", offsetof({STRUCT}, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_launches_are_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=[ENTRY])
    assert not problems, "\n".join(problems)
    assert syncs == {ENTRY: False}
    us = units()
    r = reachable(us, ENTRY)
    assert "self_collision_repair_run" in r and "scratch_alloc" not in r and "CallScratch" not in r      # no allocation
    run = us["self_collision_repair_run"]
    # three launch statements, two launches: the two instances of kernel a are the arms of one if / else
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 3 == len(re.findall(r"\bhipLaunchKernelGGL\s*\(", run))
    assert re.search(r"if \(lds\) hipLaunchKernelGGL\(gmr::self_collision_repair_kernel<true>.*\n\s*else hipLaunchKernelGGL\(gmr::self_collision_repair_kernel<false>", run)
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                    # no copy, no memset
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us[ENTRY])


def test_the_kernel_file_has_no_atomics_no_block_barrier_and_contraction_is_off():
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "self_collision_repair_kernel.hip.h")) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic", code, flags=re.I) and "__syncthreads" not in code
    for kern in ("self_collision_repair_kernel", "self_collision_repair_stats_kernel"):
        body = code[code.index(f"{kern}(const SelfCollisionRepairArgs a)"):]
        assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1, kern
    assert not re.search(r'#include "(self_collision_kernel|footlock_kernel)', code)      # the pose step is copied, the headers stay apart


# ------------------------------------------------------------------ 2: the hinge mask
def test_movable_mask_freezes_joints_and_the_paths_of_bodies():
    rob = ci.robot_model("unitree_g1")
    hb = RR.hinge_bodies(rob)
    names = [rob.jnt_names[b] for b in hb]
    nh = len(hb)
    assert collision.movable_mask(rob) == (1 << nh) - 1
    one = collision.movable_mask(rob, freeze_joints=[names[3]])
    assert one == ((1 << nh) - 1) & ~(1 << 3)
    # a frozen body freezes every hinge on its path to the root and nothing else
    ankle = next(b for b in range(rob.nbody) if "left_ankle_roll" in rob.body_names[b])
    got = collision.movable_mask(rob, freeze_bodies=[rob.body_names[ankle]])
    A = RR.ancestor_matrix(rob)
    assert [(got >> i) & 1 for i in range(nh)] == [0 if A[ankle, i] else 1 for i in range(nh)] and A[ankle].sum() == 6
    assert got == collision.movable_mask(rob, freeze_bodies=[ankle])
    assert np.array_equal(RR.mask_array(rob, got), ~A[ankle])
    with pytest.raises(ValueError):
        collision.movable_mask(rob, freeze_joints=["no_such_joint"])
    with pytest.raises(ValueError):
        collision.movable_mask(rob, freeze_bodies=["no_such_body"])
    legs = ri.hinge_mask("g1_frozen")
    assert [n for i, n in enumerate(names) if not (legs >> i) & 1] == [n for n in names if "hip" in n or "knee" in n or "ankle" in n]
    assert bin(legs).count("1") == nh - 12


# ------------------------------------------------------------------ 3: the gradient of step 5
def test_closest_points_give_the_reports_distance_bit_for_bit():
    rng = np.random.default_rng(2)
    p = rng.normal(size=(4, 2000, 3))
    p[1, ::7] = p[0, ::7]                    # spheres first, second, both
    p[3, ::5] = p[2, ::5]
    a, b = RR.closest(*p)
    w = a - b
    assert np.array_equal(np.sqrt(RR._dot(w, w)), SR.segment_distance(*p))


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_k1"])
def test_gradient_equals_central_differences_of_the_references_clearance(robot):
    """On random poses inside the joint ranges: d c_p / d q_i by central differences (h = 1e-6 rad) of the reference's own clearance
    against g_pi, for every pair and hinge.  g holds the closest-point parameters fixed, which is exact wherever the closest points
    are differentiable in the pose: the pairs whose s or t sits within 1e-4 of a clamp edge's switch are left out (a kink there
    makes a central difference the mean of two slopes), and so are pairs with parallel axes (den near 0).  The truncation error of
    the difference is O(h^2 |c'''|) ~ 1e-10 and its rounding error eps |c| / h ~ 1e-10: 1e-6 is four orders above both."""
    rob = ci.robot_model(robot)
    caps, pairs = ci.tables(robot)
    rng = np.random.default_rng(5)
    n = 6
    q = np.array(ci.qpos(robot)[int(ci.OFFS[8]):int(ci.OFFS[8]) + n])
    lo, hi = RR.limits(rob)
    cols = np.array([int(rob.qpos_adr[b]) for b in RR.hinge_bodies(rob)])
    span = np.where(np.isfinite(lo), lo, -1.0), np.where(np.isfinite(hi), hi, 1.0)
    q[:, cols] = rng.uniform(span[0], span[1], (n, cols.size))
    ev = RR.Evaluation(rob, caps, pairs, q, ri.ALL)
    h = 1e-6
    worst, used = 0.0, 0
    for i, col in enumerate(cols):
        qp, qm = q.copy(), q.copy()
        qp[:, col] += h
        qm[:, col] -= h
        cp, cm = RR.Evaluation(rob, caps, pairs, qp, ri.ALL, gradient=False), RR.Evaluation(rob, caps, pairs, qm, ri.ALL, gradient=False)
        fd = (cp.c - cm.c) / (2.0 * h)
        # smooth where the one-sided differences agree (no clamp switch between q - h and q + h) and the segments are not near touching
        fwd, bwd = (cp.c - ev.c) / h, (ev.c - cm.c) / h
        smooth = (np.abs(fwd - bwd) < 1e-4) & (ev.nw > 1e-3)
        err = np.abs(fd - ev.g[:, :, i])[smooth]
        used += int(smooth.sum())
        worst = max(worst, float(err.max()))
        # outside the moving set the clearance does not depend on the hinge at all
        still = ~(ev.in_x[:, i] | ev.in_y[:, i])
        assert np.abs(fd[:, still]).max() < 1e-9 and not ev.g[:, still, i].any()
    print(f"{robot}: worst |central difference - g| {worst:.2e} over {used} (frame, pair, hinge) entries")
    assert worst < 1e-6 and used > 0.9 * n * len(pairs) * cols.size


# ------------------------------------------------------------------ 4: the floor and the conditions
@pytest.mark.parametrize("case", list(ri.CASES))
def test_recorded_floor_is_not_smaller_than_the_measured_one(case):
    got = ri.measure_floor(case)
    print(f"{case}: |float64 - long double| qpos {got['qpos']:.2e} rad, clearance {got['clearance']:.2e} m")
    assert np.finfo(np.longdouble).nmant >= 63, "the extended evaluator needs a long double wider than float64"
    for k, v in got.items():
        assert v <= RR.FLOAT_WORST[case][k], (case, k, v)
        assert RR.FLOAT_WORST[case][k] <= 4.0 * max(v, 1e-16), (case, k, v)      # nor much larger: the recorded figure is the measured one, rounded up
    assert RR.bound(case, "qpos") <= RR.QPOS_BOUND_MIN


# (colliding frames before, of them with a movable hinge, the largest move in rad, the smallest nw in m): the issue's table
CONDITIONS = {"g1": (24, 24, 0.23, 3.7e-4), "g1_margin": (33, 33, 0.25, 3.7e-4), "g1_frozen": (33, 25, 0.25, 3.7e-4),
              "k1": (54, 54, 0.45, 0.086), "k1_margin": (146, 146, 0.66, 0.086), "reach": (1, 1, 0.10, 0.026)}


@pytest.mark.parametrize("case", list(ri.CASES))
def test_the_reference_reproduces_the_conditions_of_the_issue(case):
    """unresolved_frames == 0 at resolve_tol = 1e-4 on every case, and nw >= 1e-4 m for every active pair in every pass.  With the
    legs frozen, 8 of G1's 33 colliding frames collide in pairs between the legs alone (V = 0: no movable hinge changes them) and
    stay as they are: there the cap holds for the 25 frames that have a movable hinge, and exactly the other 8 are unresolved."""
    ref = ri.reference(case)
    m = ri.margin(case)
    before, movable, move, nw = CONDITIONS[case]
    hit = ref["clearance_before"] < m
    assert int(hit.sum()) == before and int(ref["violating"].sum()) == movable and not (ref["violating"] & ~hit).any()
    assert ref["nw_min"] >= ri.NW_MIN and abs(ref["nw_min"] - nw) <= 0.05 * nw
    assert abs(float(ref["move"].max()) - move) <= 0.01
    low = ref["clearance_after"] < m - RR.RESOLVE_TOL
    assert not (low & ref["violating"]).any()
    assert int(ref["unresolved_frames"].sum()) == int(low.sum()) == before - movable
    assert int(ref["repaired_frames"].sum()) == movable and np.array_equal(ref["move"] > 0.0, ref["violating"])
    q, _ = ri.rows(case)
    assert np.array_equal(ref["qpos"][~ref["violating"]].view(np.uint64), np.asarray(q)[~ref["violating"]].view(np.uint64))
    assert np.array_equal(ref["qpos"][:, :7].view(np.uint64), np.asarray(q)[:, :7].view(np.uint64))
    frozen = ~RR.mask_array(ci.robot_model(ri.robot_of(case)), ri.hinge_mask(case))
    assert np.array_equal(ref["qpos"][:, 7:][:, frozen].view(np.uint64), np.asarray(q)[:, 7:][:, frozen].view(np.uint64))
    assert frozen.sum() == (12 if case == "g1_frozen" else 0)
    if case == "g1":
        assert ref["clearance_after"].min() > -2e-5
        r8 = ri.reference(case, iterations=8)
        assert int((r8["clearance_after"] < -1e-4).sum()) == 2 and not (r8["clearance_after"] < -1e-3).any()
    if case == "reach":
        assert ref["clearance_before"].min() < -0.03 and ref["clearance_after"].min() >= 0.0


def test_the_dataset_scripts_flag_turns_into_retarget_clips_argument(tmp_path):
    import argparse
    import inspect
    from gmr_amd import dataset
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    off = ap.parse_args([])
    assert off.resolve_collisions is False and _walk.resolve_collisions_kw(off) == {}
    assert _walk.resolve_collisions_kw(ap.parse_args(["--resolve_collisions"])) == {"resolve_collisions": True}
    args = ap.parse_args(["--resolve_collisions", "--collision_radius", "0.04"])
    assert _walk.resolve_collisions_kw(args) == {"resolve_collisions": {"radius": 0.04}} and not _walk.wants_collision(args)
    rob = ci.robot_model("booster_k1")
    caps, pairs = ci.tables("booster_k1")
    collision.save_proxies(str(tmp_path / "k1.json"), caps, pairs)
    filed = ap.parse_args(["--resolve_collisions", "--collision_proxies", str(tmp_path / "k1.json")])
    kw = _walk.resolve_collisions_kw(filed, model=rob)["resolve_collisions"]
    assert np.array_equal(kw["capsules"].p1, caps.p1) and np.array_equal(kw["pairs"].pairs, pairs.pairs)
    sig = inspect.signature(dataset.retarget_clips)
    assert sig.parameters["resolve_collisions"].default is False
    assert set(kw) | {"radius"} <= set(inspect.signature(dataset.resolve_self_collisions).parameters)


def test_statistics_of_the_reference_on_hand_made_frames():
    after = np.array([0.1, -0.2, np.nan, 0.004, 0.0049, 1.0])
    move = np.array([0.0, 0.3, 0.0, 0.1, 0.0, 5.0])
    got = RR.statistics(after, move, [0, 0, 5, 9], 0.005, 1e-4)
    assert got["repaired_frames"].tolist() == [0, 2, 1] and got["unresolved_frames"].tolist() == [0, 2, 0]
    assert got["nonfinite_frames"].tolist() == [0, 1, 0] and got["move_max"].tolist() == [0.0, 0.3, 5.0]
    assert got["clearance_min_after"].tolist() == [np.inf, -0.2, 1.0]
