"""Self-collision without a GPU: the header, the export and the binding of gmr_motion_self_collision, the layout of its struct, the
static stream check of its launches, the proxy and pair builders of gmr_amd/collision.py, the clearance formula against brute-force
sampling, the reductions of the numpy reference, and that reference against its 50-digit evaluator
(tests/self_collision_reference.py, tests/self_collision_inputs.py)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gmr_amd import collision
from tests import self_collision_inputs as ci
from tests import self_collision_reference as SR
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gmr_motion_self_collision"


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------ 1: header, export, binding, layout
def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native, engine
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_self_collision\s*\(gmr_model \*m, const gmr_self_collision_input \*in\);", code)
    assert ENTRY in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert ENTRY not in stream_prototypes() and len(stream_prototypes()) == 27                        # the stream travels in the struct
    assert re.search(r"^ \*   gmr_motion_self_collision\s+\(no counterpart in the reference\)", src, flags=re.M)   # "what it replaces"
    lib = _native.load()
    assert lib.gmr_motion_self_collision.restype == C.c_int and len(lib.gmr_motion_self_collision.argtypes) == 2
    assert lib.gmr_motion_self_collision.argtypes[1]._type_ is _native.SelfCollisionInput
    assert lib.gmr_motion_self_collision(None, C.byref(_native.SelfCollisionInput())) == -1   # a null handle is refused before anything else
    assert engine.SELF_COLLISION_FIELDS == _native.SELF_COLLISION_FRAME_OUTPUTS + _native.SELF_COLLISION_STATS
    assert (_native.SELF_COLLISION_MAX_CAPS, _native.SELF_COLLISION_MAX_PAIRS) == (collision.MAX_CAPSULES, collision.MAX_PAIRS) == (256, 32768)


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.SelfCollisionInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_self_collision_input")].rindex("Layout (LP64)"):]   # (the listing nearest above the struct)
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct gmr_self_collision_input \{(.*?)\} gmr_self_collision_input;",
                 src, flags=re.S)
    assert m, "the layout listing in front of gmr_self_collision_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 176
    assert listing == {k: getattr(T, k).offset for k in fields}
    n_out = len(_native.SELF_COLLISION_OUTPUTS)
    assert fields[-n_out:] == [k + "_out" for k in _native.SELF_COLLISION_OUTPUTS] and fields[-n_out - 1] == "stream"
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_self_collision_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_self_collision_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
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
    assert "self_collision_run" in r and "scratch_alloc" not in r and "CallScratch" not in r              # no allocation
    # three launch statements, two launches: the two instances of kernel a are the arms of one if / else
    run = us["self_collision_run"]
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 3 == len(re.findall(r"\bhipLaunchKernelGGL\s*\(", run))
    assert re.search(r"if \(lds\) hipLaunchKernelGGL\(gmr::motion_self_collision_kernel<true>.*\n\s*else hipLaunchKernelGGL\(gmr::motion_self_collision_kernel<false>", run)
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                    # no copy, no memset
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us[ENTRY])


def test_the_kernel_file_has_no_atomics_no_block_barrier_and_contraction_is_off():
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "self_collision_kernel.hip.h")) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic", code, flags=re.I) and "__syncthreads" not in code
    for kern in ("motion_self_collision_kernel", "motion_self_collision_stats_kernel"):
        body = code[code.index(f"{kern}(const SelfCollisionArgs a)"):]
        assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1, kern


# ------------------------------------------------------------------ 2: proxies and pairs
# (capsules, kept pairs).  A capsule-against-sphere formula that ignores the capsule's length when the sphere comes second keeps one
# pair more on G1 and two more on K1 (870, 298): those pairs do overlap at rest.
EXPECT = {"unitree_g1": (45, 869), "booster_k1": (27, 296), "unitree_g1_with_hands": (59, 1633)}


def _mirror(name):
    for a, b in (("left", "right"), ("Left", "Right")):     # (K1 writes both: Left_Arm_1, left_hand_link)
        name = name.replace(a, "\0").replace(b, a).replace("\0", b)
    return name


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_builder_invariants(robot):
    rob = ci.robot_model(robot)
    caps, pairs = ci.tables(robot)
    kept, dropped = collision.default_pairs(rob, caps)
    C = len(caps)
    assert np.array_equal(kept.pairs, pairs.pairs) and (C, len(pairs)) == EXPECT[robot]
    # every body has a capsule, a leaf exactly one sphere, and the anchors are the bodies whose origins lie on the segment
    children = [[c for c in range(rob.nbody) if rob.parent[c] == b] for b in range(rob.nbody)]
    assert C == sum(max(1, len(ch)) for ch in children) and sorted(set(caps.body.tolist())) == list(range(rob.nbody))
    for i in range(C):
        b = int(caps.body[i])
        assert not caps.p0[i].any() and caps.radius[i] == ci.RADIUS[robot]
        if len(caps.anchors[i]) == 1:
            assert caps.anchors[i] == (b,) and not children[b] and not caps.p1[i].any() and caps.names[i] == rob.body_names[b]
        else:
            c = caps.anchors[i][1]
            assert caps.anchors[i][0] == b and rob.parent[c] == b and np.array_equal(caps.p1[i], rob.body_pos[c])
    # kept and dropped partition all unordered pairs, both in lexicographic order, every dropped pair with one of the three reasons
    everything = sorted([tuple(p) for p in kept.pairs.tolist()] + [p for p, _ in dropped])
    assert everything == [(a, b) for a in range(C) for b in range(a + 1, C)]
    assert [tuple(p) for p in kept.pairs.tolist()] == sorted(tuple(p) for p in kept.pairs.tolist()) and [p for p, _ in dropped] == sorted(p for p, _ in dropped)
    assert {w for _, w in dropped} <= {collision.SAME_BODY, collision.ALWAYS_OVERLAP, collision.REST_OVERLAP}
    P, Q = collision.rest_ends(rob, caps)
    rr = lambda a, b: caps.radius[a] + caps.radius[b]   # noqa: E731
    clr = lambda a, b: float(collision.segment_distance(P[a], Q[a], P[b], Q[b]) - rr(a, b))   # noqa: E731
    for (a, b), why in dropped:
        if why == collision.SAME_BODY:
            assert caps.body[a] == caps.body[b]
        elif why == collision.ALWAYS_OVERLAP:
            assert caps.body[a] != caps.body[b] and clr(a, b) <= 1e-12      # (it overlaps in every pose, the rest pose included)
        else:
            assert caps.body[a] != caps.body[b] and clr(a, b) <= 0.0
    assert all(clr(a, b) > 0.0 for a, b in kept.pairs.tolist())             # no kept pair overlaps at rest
    # an always-overlapping pair does overlap in random poses too
    rng = np.random.default_rng(0)
    q = np.zeros((8, rob.nq)); q[:, 3] = 1.0
    q[:, 7:] = rng.uniform(-1.0, 1.0, (8, rob.nq - 7))
    always = collision.PairTable(np.array([p for p, w in dropped if w == collision.ALWAYS_OVERLAP], np.int32))
    assert SR.pair_clearance(rob, caps, always, q).max() <= 1e-12
    # mirror symmetry under left <-> right
    names = set(collision.pair_names(caps, kept))
    assert all((_mirror(a), _mirror(b)) in names or (_mirror(b), _mirror(a)) in names for a, b in names)
    # with a rest margin the third kind grows and nothing else changes
    tightest = min(clr(a, b) for a, b in kept.pairs.tolist())
    kept2, dropped2 = collision.default_pairs(rob, caps, rest_margin=tightest)
    assert len(kept2) < len(kept) and all(clr(a, b) > tightest for a, b in kept2.pairs.tolist()) and sum(w != collision.REST_OVERLAP for _, w in dropped2) == sum(w != collision.REST_OVERLAP for _, w in dropped)


def test_json_round_trip_is_exact_and_a_file_can_name_bodies(tmp_path):
    rob = ci.robot_model("unitree_g1")
    caps = collision.skeleton_capsules(rob, {"default": 0.03, "pelvis": 0.1234567890123456789, "head_mocap": 1.0 / 3.0})
    pairs = collision.default_pairs(rob, caps)[0]
    d = json.loads(json.dumps({**caps.to_dict(), **pairs.to_dict()}))
    c2, p2 = collision.CapsuleTable.from_dict(d), collision.PairTable.from_dict(d)
    for k in ("body", "p0", "p1", "radius"):
        assert np.array_equal(getattr(caps, k), getattr(c2, k)) and getattr(caps, k).dtype == getattr(c2, k).dtype, k
    assert caps.names == c2.names and caps.anchors == c2.anchors and np.array_equal(pairs.pairs, p2.pairs) and p2.pairs.dtype == np.int32
    assert caps.radius[caps.names.index("head_mocap")] == 1.0 / 3.0 and set(caps.radius[caps.body == 0].tolist()) == {0.1234567890123456789}
    path = tmp_path / "proxies.json"
    collision.save_proxies(str(path), caps, pairs)
    c3, p3 = collision.load_proxies(str(path))
    assert np.array_equal(c3.p1, caps.p1) and np.array_equal(p3.pairs, pairs.pairs)
    path.write_text(json.dumps({"capsules": [{"name": "fist", "body": "right_rubber_hand", "p0": [0, 0, 0], "radius": 0.05},
                                             {"name": "skull", "body": "head_mocap", "p0": [0, 0, 0.05], "p1": [0, 0, 0.1], "radius": 0.09}]}))
    c4, p4 = collision.load_proxies(str(path), rob)
    assert p4 is None and c4.body.tolist() == [rob.body_names.index("right_rubber_hand"), rob.body_names.index("head_mocap")]
    assert np.array_equal(c4.p0[0], c4.p1[0]) and len(collision.default_pairs(rob, c4)[0]) == 1
    with pytest.raises(ValueError):
        collision.PairTable(np.array([[1, 1]]))
    with pytest.raises(ValueError):
        collision.skeleton_capsules(rob, {"no_such_body": 0.1})


# ------------------------------------------------------------------ 3: the clearance formula against brute force
def _brute(p1, q1, p2, q2, n=401):
    u = np.linspace(0.0, 1.0, n)
    a = p1[None] + u[:, None] * (q1 - p1)[None]
    b = p2[None] + u[:, None] * (q2 - p2)[None]
    return float(np.sqrt(((a[:, None] - b[None]) ** 2).sum(-1)).min())


def test_segment_distance_against_brute_force_sampling():
    rng = np.random.default_rng(5)
    cases = [tuple(rng.uniform(-1, 1, 3) for _ in range(4)) for _ in range(40)]
    p, q, d = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    cases += [(p, p, q, q), (p, p, q, q + d), (q, q + d, p, p),                       # sphere-sphere, sphere-capsule (either order)
              (p, p + d, q, q + d), (p, p + d, q, q - 2 * d), (p, p + d, p + 3 * d, p + 5 * d), (p, p + d, p + 0.5 * d, p + 2 * d),   # parallel, collinear
              (p - d, p + d, p - np.cross(d, q), p + np.cross(d, q)),                  # crossing: distance 0
              (p, q, p, p + d), (p, q, q + d, q), (p, p, p, p)]                       # a shared endpoint, coincident spheres
    for p1, q1, p2, q2 in cases:
        got = float(SR.segment_distance(p1, q1, p2, q2))
        want = _brute(p1, q1, p2, q2)
        lens = np.linalg.norm(q1 - p1) + np.linalg.norm(q2 - p2)
        assert got <= want + 1e-12 and want - got <= lens / 400.0 + 1e-12, (got, want)
        assert got == float(collision.segment_distance(p1, q1, p2, q2))               # the builder's copy is the same formula
        assert abs(got - float(SR.segment_distance(p2, q2, p1, q1))) <= 1e-12        # symmetric to rounding
    assert SR.segment_distance(p - d, p + d, p - np.cross(d, q), p + np.cross(d, q)) <= 1e-15
    assert SR.segment_distance(p, q, p, p + d) == 0.0 and SR.segment_distance(p, p, p, p) == 0.0
    assert np.isnan(SR.segment_distance(p * np.nan, q, p, p + d))


# ------------------------------------------------------------------ 4: the reductions
def test_frame_reduction_lowest_index_on_ties_and_the_nan_rule():
    cl = np.array([[0.3, -0.1, -0.1, 0.2], [0.5, 0.5, 0.5, 0.5], [0.1, np.nan, -0.4, 0.0], [-0.2, -0.3, 0.0, -0.3]])
    f = SR.frames(cl, 0.0)
    assert f["pair"].tolist() == [1, 0, -1, 1] and f["hits"].tolist() == [2, 0, 0, 3]
    assert f["clearance"][[0, 1, 3]].tolist() == [-0.1, 0.5, -0.3] and np.isnan(f["clearance"][2])
    assert SR.frames(cl, 0.25)["hits"].tolist() == [3, 0, 0, 4] and f["pair"].dtype == f["hits"].dtype == np.int32


def test_clip_statistics_longest_run_earliest_frame_and_the_empty_clip():
    nan = np.nan
    #            clip 0 (empty) | clip 1                                      | clip 2
    clearance = np.array([0.2, -0.1, -0.3, nan, -0.3, -0.2, -0.1, 0.4, -0.5, nan, nan])
    hits = np.array([0, 1, 2, 0, 3, 1, 1, 0, 4, 0, 0], np.int32)
    pair = np.array([7, 5, 6, -1, 9, 5, 5, 7, 2, -1, -1], np.int32)
    st = SR.statistics(clearance, pair, hits, [0, 0, 9, 11])
    assert st["clearance_min"].tolist() == [np.inf, -0.5, np.inf] and st["worst_frame"].tolist() == [-1, 8, -1] and st["worst_pair"].tolist() == [-1, 2, -1]
    assert st["colliding_frames"].tolist() == [0, 6, 0] and st["longest_run"].tolist() == [0, 3, 0]      # the NaN frame ends the run of two
    assert st["hits_sum"].tolist() == [0, 12, 0] and st["nonfinite_frames"].tolist() == [0, 1, 2] and st["hits_sum"].dtype == np.int64
    st = SR.statistics(clearance[:8], pair[:8], hits[:8], [0, 8])
    assert st["worst_frame"].tolist() == [2] and st["worst_pair"].tolist() == [6]                         # the earlier of the two frames at -0.3
    long = np.where(np.arange(200) % 70 == 69, 0, 1).astype(np.int32)                                     # runs of 69 across the 64-frame tiles
    st = SR.statistics(np.where(long > 0, -0.1, 0.1), np.zeros(200, np.int32), long, [0, 200])
    assert st["longest_run"].tolist() == [69] and st["colliding_frames"].tolist() == [198]


def test_the_cases_have_both_kinds_of_frame_and_stay_clear_of_the_margin():
    """A precondition of asking the GPU for equal hit counts, a condition on the reference, not a measurement: every pair clearance of
    every frame is farther from the margin than a thousand times the bound."""
    for robot, colliding in (("unitree_g1", 24), ("booster_k1", 54), ("unitree_g1_with_hands", 167)):
        ref = ci.reference(robot)
        assert int((ref["hits"] > 0).sum()) == colliding == int(ref["colliding_frames"].sum())
        assert ci.margin_distance(robot) > 1000.0 * SR.bound(robot)
        assert ref["clearance_min"][0] == np.inf and ref["worst_frame"][0] == -1                          # the empty clip
    assert int((ci.reference("unitree_g1")["colliding_frames"] > 0).sum()) == 3                          # spread over three clips
    assert (ci.second_gap(ci.reference("unitree_g1")["pair_clearance"]) == 0.0).any()                    # exact ties between pairs do occur


def test_the_hand_built_clip_puts_the_right_hand_into_the_head():
    rob = ci.robot_model("unitree_g1")
    caps, pairs = ci.tables("unitree_g1")
    q = ci.reach_pose()
    ref = SR.self_collision(rob, caps, pairs, q, [0, q.shape[0]])
    a, b = collision.pair_names(caps, pairs)[int(ref["worst_pair"][0])]
    assert ref["worst_frame"].tolist() == [5] and ref["colliding_frames"].tolist() == [1] and ref["clearance_min"][0] < -0.01
    assert "head" in a and (b.startswith("right_wrist") or b.startswith("right_rubber_hand"))


# ------------------------------------------------------------------ 5: the bound
@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_the_recorded_floor_covers_the_gpu_cases_own_rows(robot):
    """|numpy reference - 50-digit evaluator| over all pairs of the cases' hardest rows, re-measured."""
    rows = ci.floor_rows(robot)
    worst = ci.measure_floor(robot, rows)
    print(f"{robot}: {len(rows)} rows x {len(ci.tables(robot)[1])} pairs: worst |numpy - 50 digits| {worst:.2e} (recorded {SR.FLOAT_WORST[robot]:.0e})")
    assert 8 <= len(rows) <= 32
    assert worst <= SR.FLOAT_WORST[robot], f"the recorded floor {SR.FLOAT_WORST[robot]:.1e} is below the measured {worst:.2e}"
    assert SR.FLOAT_WORST[robot] <= 64 * np.finfo(float).eps          # and the floor is rounding, not a modelling difference


# ------------------------------------------------------------------ 6: the report's CSV, the threshold and the script flags
def test_collision_csv_names_the_worst_pair_and_the_threshold_marks_the_clip(tmp_path):
    from gmr_amd import dataset
    rep = {"clearance_min": np.array([0.01, -0.04]), "penetration_max": np.array([0.0, 0.04]), "worst_frame": np.array([3, 17], np.int32),
           "worst_pair": np.array([5, 9], np.int32), "colliding_frames": np.array([0, 6], np.int32), "longest_run": np.array([0, 4], np.int32),
           "hits_sum": np.array([0, 11], np.int64), "nonfinite_frames": np.array([0, 0], np.int32),
           "worst_pair_names": [("a", "b"), ("hand", "head")]}
    p = tmp_path / "col.csv"
    dataset.write_collision_csv(str(p), ["walk", "wave"], rep)
    rows = [r.split(",") for r in p.read_text().strip().splitlines()]
    assert rows[0] == ["clip", *dataset.COLLISION_CSV_FIELDS, "worst_capsule_a", "worst_capsule_b"]
    assert rows[1] == ["walk", "0.01", "0.0", "3", "0", "0", "0", "0", "a", "b"] and rows[2] == ["wave", "-0.04", "0.04", "17", "6", "4", "11", "0", "hand", "head"]
    assert dataset.collision_hard_mask(rep, 0.02).tolist() == [False, True] and dataset.collision_hard_mask(rep, 0.05).tolist() == [False, False]


def test_the_dataset_scripts_flags_ask_for_the_report_and_the_sink_writes_both_files(tmp_path):
    import argparse
    from gmr_amd import dataset
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    off = ap.parse_args([])
    assert off.collision_csv is None and off.max_penetration is None and not _walk.wants_collision(off) and not _walk.wants_sink(off)
    assert _walk.collision_kw(off) == {}
    args = ap.parse_args(["--collision_csv", str(tmp_path / "col.csv"), "--max_penetration", "0.02", "--hard_out", str(tmp_path / "hard.txt"),
                          "--collision_radius", "0.04"])
    assert _walk.wants_collision(args) and _walk.wants_report(args) and not _walk.wants_dynamics(args)
    assert _walk.collision_kw(args) == {"collision": {"radius": 0.04}}
    assert _walk.report_path(args.collision_csv, "unitree_g1", 2).endswith("col.unitree_g1.rank2.csv")

    class Report:   # what dataset.report_hard_mask and report_difficulty read of a ClipReport
        task_pos_max = np.array([[0.01], [0.02]])
        dof_step_max = np.array([[0.1], [0.2]])
        err_max = np.array([[0.1, 0.1], [0.2, 0.2]])
        last_table = 1

        def __len__(self):
            return 2

    col = {"clearance_min": np.array([0.01, -0.04]), "penetration_max": np.array([0.0, 0.04]), "worst_frame": np.array([3, 17], np.int32),
           "worst_pair": np.array([5, 9], np.int32), "colliding_frames": np.array([0, 6], np.int32), "longest_run": np.array([0, 4], np.int32),
           "hits_sum": np.array([0, 11], np.int64), "nonfinite_frames": np.array([0, 0], np.int32), "worst_pair_names": [("a", "b"), ("hand", "head")]}
    sink = _walk.ReportSink(args)
    kept, targets = sink.take(dataset, ["out/walk.pkl", "out/wave.pkl"], ["m0", "m1"], Report(), None, col)
    assert kept == ["m0"] and targets == ["out/walk.pkl"] and sink.withheld == 1
    assert (tmp_path / "col.csv").read_text().splitlines()[2].startswith("wave,-0.04,")
    assert "wave.pkl" in (tmp_path / "hard.txt").read_text() and "walk.pkl" not in (tmp_path / "hard.txt").read_text()
    alone = ap.parse_args(["--collision_csv", str(tmp_path / "only.csv")])
    assert _walk.wants_collision(alone) and _walk.wants_sink(alone) and not _walk.wants_report(alone) and _walk.collision_kw(alone) == {"collision": True}
    sink = _walk.ReportSink(alone)
    kept, targets = sink.take(dataset, ["out/walk.pkl", "out/wave.pkl"], ["m0", "m1"], None, None, col)
    assert kept == ["m0", "m1"] and sink.withheld == 0 and len((tmp_path / "only.csv").read_text().splitlines()) == 3
    # a proxies file replaces the skeleton
    rob = ci.robot_model("booster_k1")
    caps, pairs = ci.tables("booster_k1")
    collision.save_proxies(str(tmp_path / "k1.json"), caps, pairs)
    filed = ap.parse_args(["--collision_csv", "x.csv", "--collision_proxies", str(tmp_path / "k1.json")])
    kw = _walk.collision_kw(filed, model=rob)["collision"]
    assert np.array_equal(kw["capsules"].p1, caps.p1) and np.array_equal(kw["pairs"].pairs, pairs.pairs)
