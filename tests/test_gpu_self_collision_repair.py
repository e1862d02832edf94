"""gmr_motion_self_collision_repair on the GPU against the numpy reference (tests/self_collision_repair_reference.py; inputs:
tests/self_collision_repair_inputs.py).

The bound.  self_collision_repair_reference.bound: 16 times (foot locking's margin over its floor) the numpy reference's own distance
to its long-double evaluator, measured per case on every row (FLOAT_WORST; tests/test_self_collision_repair_host.py re-measures
it), for qpos_out never looser than 1e-9 rad.  Nothing in the bound was measured on a kernel.  The synthetic tables have no
recorded floor: theirs is measured here, on the rows of the test, by the same two evaluators.

`unitree_g1_with_hands` and the thin synthetic chains are not agreement cases (tests/self_collision_repair_inputs.py says why).

Measured on an MI355X (worst |GPU - numpy| per case as a fraction of its bound): see DESIGN.md 4.21."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import collision  # noqa: E402
from tests import self_collision_inputs as ci  # noqa: E402
from tests import self_collision_repair_inputs as ri  # noqa: E402
from tests import self_collision_repair_reference as RR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402

FILL = 0xA5
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
FRAME = ("qpos", "clearance_before", "clearance_after", "move")
STATS = ("repaired_frames", "unresolved_frames", "move_max", "clearance_min_after", "nonfinite_frames")
COUNTS = ("repaired_frames", "unresolved_frames", "nonfinite_frames")
EINVAL, EUNSUPPORTED = -1, -3
G1 = "unitree_g1"


def shapes(robot=G1, rows=ri.N, clips=ri.S):
    nq = ci.robot_model(robot).nq
    return {"qpos": ((rows, nq), F64), "clearance_before": ((rows,), F64), "clearance_after": ((rows,), F64), "move": ((rows,), F64),
            "repaired_frames": ((clips,), I32), "unresolved_frames": ((clips,), I32), "move_max": ((clips,), F64),
            "clearance_min_after": ((clips,), F64), "nonfinite_frames": ((clips,), I32)}


def sentinel_out(names=None, **kw):
    out = {}
    for k, (sh, dt) in shapes(**kw).items():
        if names is None or k in names:
            out[k] = torch.empty(sh, dtype=dt, device=DEV())
            if out[k].numel():
                out[k].view(U8).fill_(FILL)
    return out


def run(robot, q, offs, caps, pairs, out=None, **kw):
    res = engine(robot).motion_self_collision_repair(_dev(q), offs, caps, pairs, out=out, **kw)
    return {k: t.cpu().numpy() for k, t in res.items()}


def run_case(case, out=None, **kw):
    q, offs = ri.rows(case)
    caps, pairs = ri.tables(case)
    return run(ri.robot_of(case), q, offs, caps, pairs, out=out, margin=ri.margin(case), movable=ri.hinge_mask(case), **kw)


@functools.lru_cache(maxsize=None)
def gpu(case):
    """The GPU's answer to a case into pre-filled caller-owned outputs: computed once, shared."""
    q, offs = ri.rows(case)
    return run_case(case, out=sentinel_out(robot=ri.robot_of(case), rows=q.shape[0], clips=len(offs) - 1))


def same(a, b):
    return np.array_equal(_bytes(a), _bytes(b))


def check(got, ref, bq, bc, what, margin, resolve_tol=RR.RESOLVE_TOL):
    """The comparison of the issue: qpos_out within bq, both clearances within bc with equal NaN patterns, move within bq, counts
    equal, every statistic bit for bit the reference reduction of the GPU's own per-frame arrays.  Returns the worst differences."""
    worst = {"qpos": float(np.abs(got["qpos"] - ref["qpos"]).max(initial=0.0))}
    assert worst["qpos"] <= bq, (what, worst, bq)
    worst["clearance"] = 0.0
    for k in ("clearance_before", "clearance_after"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (what, k)
        ok = ~np.isnan(ref[k])
        worst["clearance"] = max(worst["clearance"], float(np.abs(got[k][ok] - ref[k][ok]).max(initial=0.0)))
    assert worst["clearance"] <= bc, (what, worst, bc)
    worst["move"] = float(np.abs(got["move"] - ref["move"]).max(initial=0.0))
    assert worst["move"] <= bq, (what, worst, bq)
    if "repaired_frames" in got:
        offs = ref["offs"]
        own = RR.statistics(got["clearance_after"], got["move"], offs, margin, resolve_tol)
        for k in STATS:
            assert got[k].dtype == own[k].dtype and same(got[k], own[k]), (what, k)
        for k in COUNTS:
            assert np.array_equal(got[k], ref[k]), (what, k)
    return worst


def reference(rob, caps, pairs, q, offs, margin=0.0, **kw):
    ref = RR.repair(rob, caps, pairs, q, offs, margin, **kw)
    ref["offs"] = np.asarray(offs)
    return ref


def measured_bounds(rob, caps, pairs, q, offs, margin=0.0, **kw):
    """(reference, qpos bound, clearance bound) of a table without a recorded floor: GPU_FACTOR times the distance of the numpy
    reference to its long-double evaluator on these very rows, and never below the recorded bounds of the G1 case (whose rows
    these are), which a subset of its table cannot undercut by more than luck."""
    ref = reference(rob, caps, pairs, q, offs, margin, **kw)
    ext = RR.repair(rob, caps, pairs, q, offs, margin, dtype=np.longdouble, **kw)
    fq = float(np.abs(ref["qpos"] - ext["qpos"]).max())
    fc = float(max(np.abs(ref[k] - ext[k]).max() for k in ("clearance_before", "clearance_after")))
    return ref, min(max(RR.GPU_FACTOR * fq, RR.bound("g1", "qpos")), RR.QPOS_BOUND_MIN), max(RR.GPU_FACTOR * fc, RR.bound("g1", "clearance"))


@functools.lru_cache(maxsize=None)
def busy_rows():
    """(qpos, seq_offsets) of G1: the 24 colliding rows of the `g1` case and the 16 rows in front of the first, as clips of 0, 3
    and 37 frames."""
    ref = ri.reference("g1")
    hit = np.flatnonzero(ref["violating"])
    free = np.flatnonzero(~ref["violating"])[:16]
    q = np.array(ci.qpos(G1))[np.concatenate([free, hit])]
    q.setflags(write=False)
    return q, np.array([0, 0, 3, q.shape[0]], np.int64)


# ------------------------------------------------------------------ 1: accuracy
@pytest.mark.parametrize("case", list(ri.CASES))
def test_cases_equal_the_reference(case):
    got, ref = gpu(case), dict(ri.reference(case))
    q, offs = ri.rows(case)
    ref["offs"] = offs
    m = ri.margin(case)
    # the precondition of equal counts (conditions on the reference): no frame near the unresolved threshold, no tiny move
    assert np.abs(ref["clearance_after"] - (m - RR.RESOLVE_TOL)).min() > 1000.0 * RR.bound(case, "clearance")
    assert ref["move"][ref["move"] > 0.0].min() > 1000.0 * RR.bound(case, "qpos") and ref["nw_min"] >= ri.NW_MIN
    worst = check(got, ref, RR.bound(case, "qpos"), RR.bound(case, "clearance"), case, m)
    print(f"{case}: worst |GPU - numpy| qpos {worst['qpos']:.2e} rad ({worst['qpos'] / RR.bound(case, 'qpos'):.3f} of its bound), "
          f"clearance {worst['clearance']:.2e} m ({worst['clearance'] / RR.bound(case, 'clearance'):.3f}), move {worst['move']:.2e}; "
          f"{int(got['repaired_frames'].sum())} frames repaired, {int(got['unresolved_frames'].sum())} unresolved, largest move {got['move_max'].max():.3f} rad")
    # the cap of the issue: nothing that a movable hinge can reach stays below margin - 1e-4
    low = got["clearance_after"] < m - RR.RESOLVE_TOL
    assert not (low & ref["violating"]).any()
    assert int(got["unresolved_frames"].sum()) == (8 if case == "g1_frozen" else 0)
    assert got["repaired_frames"].sum() > 0 and got["qpos"].dtype == np.float64
    if len(offs) > 2:
        assert got["clearance_min_after"][0] == np.inf and got["move_max"][0] == 0.0 and got["repaired_frames"][0] == 0     # the empty clip


@pytest.mark.parametrize("case", ["g1", "g1_frozen", "k1_margin"])
def test_untouched_entries_are_the_inputs_bytes(case):
    got, ref = gpu(case), ri.reference(case)
    q = np.asarray(ri.rows(case)[0])
    assert same(got["qpos"][:, :7], q[:, :7])                                            # the root never moves
    still = ~ref["violating"]
    assert same(got["qpos"][still], q[still]) and not got["move"][still].any() and still.sum() > 100
    assert same(got["clearance_before"][still], got["clearance_after"][still])           # one evaluation, reported twice
    frozen = ~RR.mask_array(ci.robot_model(ri.robot_of(case)), ri.hinge_mask(case))
    assert same(got["qpos"][:, 7:][:, frozen], q[:, 7:][:, frozen]) and frozen.sum() == (12 if case == "g1_frozen" else 0)
    for k, t in got.items():
        assert not bool((_bytes(t) == FILL).all()) or t.size == 0, k                    # every element of a non-NULL output was written
    moved = ref["violating"]
    assert (np.abs(got["qpos"][moved] - q[moved]).max(axis=1) > 0.0).all()


def test_two_calls_wavefront_counts_and_where_the_pairs_live_change_no_byte(monkeypatch):
    case = "k1_margin"          # (146 of 332 frames are repaired)
    base = gpu(case)
    again = run_case(case)      # without out the call allocates the same answer
    for k in base:
        assert same(again[k], base[k]), k
    for env in ({"GMR_AMD_COLLISION_REPAIR_WAVES": "1"}, {"GMR_AMD_COLLISION_REPAIR_WAVES": "7"}, {"GMR_AMD_COLLISION_REPAIR_PAIRS": "global"},
                {"GMR_AMD_COLLISION_REPAIR_PAIRS": "global", "GMR_AMD_COLLISION_REPAIR_WAVES": "3"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = run_case(case)
        for k in got:
            assert same(got[k], base[k]), (env, k)
    q, offs = ri.rows(case)
    a = int(offs[8])
    caps, pairs = ri.tables(case)
    alone = run(ri.robot_of(case), np.asarray(q)[a:a + 130], [0, 130], caps, pairs, margin=ri.margin(case))   # a clip alone and in the batch
    for k in FRAME:
        assert same(alone[k], base[k][a:a + 130]), k
    for k in STATS:
        assert same(alone[k][0], base[k][8]), k
    eng = engine(ri.robot_of(case))
    assert eng.collision_device(caps, pairs) is eng.collision_device(caps, pairs)       # uploaded once per (capsules, pairs)


def test_outputs_left_out_and_rows_outside_every_clip():
    case = "k1"
    q, offs = ri.rows(case)
    full = gpu(case)
    only = run_case(case, out=sentinel_out(names=("qpos",), robot=ri.robot_of(case)))
    assert list(only) == ["qpos"] and same(only["qpos"], full["qpos"])
    nostats = run_case(case, stats=False)
    assert sorted(nostats) == sorted(FRAME) and all(same(nostats[k], full[k]) for k in FRAME)
    for k in STATS:
        some = run_case(case, out=sentinel_out(names=FRAME + (k,), robot=ri.robot_of(case)))
        assert sorted(some) == sorted(FRAME + (k,)) and same(some[k], full[k]), k
    short = np.array(offs)
    short[-1] -= 7                                                                       # the last clip ends seven rows early
    caps, pairs = ri.tables(case)
    got = run(ri.robot_of(case), q, short, caps, pairs, out=sentinel_out(robot=ri.robot_of(case)))
    for k in FRAME:
        assert bool((_bytes(got[k][-7:]) == FILL).all()) and same(got[k][:-7], full[k][:-7]), k
    own = RR.statistics(got["clearance_after"][:-7], got["move"][:-7], short, 0.0, RR.RESOLVE_TOL)
    for k in STATS:
        assert same(got[k], own[k]), k
    with pytest.raises(Exception, match="clearance_before, clearance_after and move"):
        run_case(case, out=sentinel_out(names=("qpos", "clearance_after", "move_max"), robot=ri.robot_of(case)))
    with pytest.raises(Exception, match="qpos"):
        run_case(case, out=sentinel_out(names=("clearance_after",), robot=ri.robot_of(case)))


# ------------------------------------------------------------------ 2: table passes
def test_a_table_of_65_pairs():
    """65 pairs of G1's table -- the deepest of the rows in use, the two deepest of all last, so that the one pair of the second
    pass over the pairs is an active one."""
    rob = ci.robot_model(G1)
    caps, pairs = ci.tables(G1)
    q, offs = busy_rows()
    cl = ci.reference(G1)["pair_clearance"].min(axis=0)
    idx = np.argsort(cl)[:65]
    table = collision.PairTable(pairs.pairs[np.concatenate([np.sort(idx[2:]), idx[1::-1]])].copy())
    ref, bq, bc = measured_bounds(rob, caps, table, q, offs)
    assert len(table) == 65 and ref["violating"].sum() >= 20 and ref["nw_min"] >= ri.NW_MIN
    got = run(G1, q, offs, caps, table)
    w = check(got, ref, bq, bc, "65 pairs", 0.0)
    without = RR.repair(rob, caps, collision.PairTable(table.pairs[:64].copy()), q, offs)
    assert np.abs(without["qpos"] - ref["qpos"]).max() > 1e-3                             # the 65th pair matters
    print(f"65 pairs: worst qpos {w['qpos']:.2e} (bound {bq:.1e}), clearance {w['clearance']:.2e} (bound {bc:.1e})")


def test_a_table_of_more_than_64_capsules():
    """70 capsules on random bodies, ends within 0.2 m of the body's origin, every fifth a sphere, all 2 415 pairs of them: two
    passes over the capsules, 38 over the pairs.  Random capsules overlap in ways no pose resolves and their axes come close (nw
    down to 1.7e-5 m), so this is a test of agreement over two passes, with the floor measured on these rows, not of success."""
    n_caps = 70
    rob = ci.robot_model(G1)
    rng = np.random.default_rng(n_caps)
    body = rng.integers(0, rob.nbody, n_caps)
    p0, p1 = rng.uniform(-0.2, 0.2, (n_caps, 3)), rng.uniform(-0.2, 0.2, (n_caps, 3))
    p1[::5] = p0[::5]
    caps = collision.CapsuleTable(body, p0, p1, rng.uniform(0.002, 0.01, n_caps), [str(i) for i in range(n_caps)])
    table = collision.PairTable(np.array([(a, b) for a in range(n_caps) for b in range(a + 1, n_caps)], np.int32))
    q = np.array(ci.qpos(G1)[int(ci.OFFS[6]):int(ci.OFFS[6]) + 40])
    offs = np.array([0, 0, 3, 40], np.int64)
    ref, bq, bc = measured_bounds(rob, caps, table, q, offs, iterations=2)
    assert ref["violating"].all() and ref["nw_min"] > 1e-5
    got = run(G1, q, offs, caps, table, iterations=2)
    w = check(got, ref, bq, bc, "70 capsules", 0.0)
    print(f"70 capsules: worst qpos {w['qpos']:.2e} (bound {bq:.1e}), clearance {w['clearance']:.2e} (bound {bc:.1e})")


# ------------------------------------------------------------------ 3: the hinge mask and the pass count
def test_hinge_mask_none_set_one_bit_and_all_set():
    rob = ci.robot_model(G1)
    caps, pairs = ci.tables(G1)
    q, offs = busy_rows()
    nh = rob.nq - 7
    none = run(G1, q, offs, caps, pairs, movable=0)
    assert same(none["qpos"], q) and not none["repaired_frames"].any() and not none["move"].any()
    assert same(none["clearance_before"], none["clearance_after"]) and none["unresolved_frames"].sum() > 0
    names = [rob.jnt_names[b] for b in RR.hinge_bodies(rob)]
    bit = names.index("right_shoulder_pitch_joint")
    ref, bq, bc = measured_bounds(rob, caps, pairs, q, offs, hinge_mask=1 << bit)
    one = run(G1, q, offs, caps, pairs, movable=1 << bit)
    check(one, ref, bq, bc, "one bit", 0.0)
    others = np.arange(rob.nq) != 7 + bit
    assert same(one["qpos"][:, others], q[:, others]) and one["repaired_frames"].sum() > 0
    all_set = run(G1, q, offs, caps, pairs, movable=(1 << 64) - 1)                          # (bits past the last hinge are ignored)
    default = run(G1, q, offs, caps, pairs)
    exact = run(G1, q, offs, caps, pairs, movable=(1 << nh) - 1)
    for k in all_set:
        assert same(all_set[k], default[k]) and same(exact[k], default[k]), k
    base, hit = gpu("g1"), np.flatnonzero(ri.reference("g1")["violating"])
    assert same(default["qpos"][16:], base["qpos"][hit])                                  # a frame's answer does not depend on its clip


@pytest.mark.parametrize("iterations", [1, 32])
def test_one_pass_and_thirty_two(iterations):
    rob = ci.robot_model(G1)
    caps, pairs = ci.tables(G1)
    q, offs = busy_rows()
    ref, bq, bc = measured_bounds(rob, caps, pairs, q, offs, iterations=iterations)
    got = run(G1, q, offs, caps, pairs, iterations=iterations)
    w = check(got, ref, bq, bc, iterations, 0.0)
    print(f"I = {iterations}: worst qpos {w['qpos']:.2e} (bound {bq:.1e}), {int(got['unresolved_frames'].sum())} unresolved")
    if iterations == 1:
        assert got["move"].max() <= RR.STEP_CAP + 1e-12 and got["unresolved_frames"].sum() > 0
    else:
        assert not got["unresolved_frames"].any()


def test_the_step_cap_and_the_joint_limits_hold():
    rob = ci.robot_model(G1)
    caps, pairs = ci.tables(G1)
    q, offs = busy_rows()
    got = run(G1, q, offs, caps, pairs, iterations=3, step_cap=0.01)
    assert 0.0 < got["move"].max() <= 3 * 0.01 + 1e-12
    lo, hi = RR.limits(rob)
    full = run(G1, q, offs, caps, pairs)["qpos"][:, 7:]
    assert (full >= np.minimum(lo, q[:, 7:])).all() and (full <= np.maximum(hi, q[:, 7:])).all()


# ------------------------------------------------------------------ 4: errors and empty calls
def raw_call(eng, q, offs, tab, out, **kw):
    """The entry itself, from device tensors: (return code, message)."""
    from gmr_amd import _native
    st = _native.SelfCollisionRepairInput()
    st.qpos, st.n_frames, st.seq_offsets, st.n_seq = q.data_ptr(), int(q.shape[0]), offs.data_ptr(), int(offs.shape[0]) - 1
    st.n_caps, st.n_pairs, st.margin = int(tab["cap_body"].shape[0]), int(tab["pairs"].shape[0]), 0.0
    st.iterations, st.damping, st.step_cap, st.resolve_tol, st.hinge_mask = RR.ITERATIONS, RR.DAMPING, RR.STEP_CAP, RR.RESOLVE_TOL, ri.ALL
    for k, t in tab.items():
        setattr(st, k, t.data_ptr())
    for k, t in out.items():
        setattr(st, k + "_out", t.data_ptr())
    for k, v in kw.items():
        setattr(st, k, v)
    st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    rc = eng._lib.gmr_motion_self_collision_repair(eng._h, C.byref(st))
    return rc, eng._lib.gmr_last_error(eng._h)


def test_bad_arguments_are_refused_with_their_code_and_empty_calls_return_ok():
    case = "k1"
    robot = ri.robot_of(case)
    eng = engine(robot)
    caps, pairs = ri.tables(case)
    tab = eng.collision_device(caps, pairs)
    q, offs = _dev(ri.rows(case)[0]), _dev(ri.rows(case)[1])
    out = sentinel_out(robot=robot)
    nan, inf = float("nan"), float("inf")
    bad = [({"iterations": 0}, EINVAL, b"iterations"), ({"iterations": 33}, EINVAL, b"iterations"), ({"iterations": -1}, EINVAL, b"iterations"),
           ({"damping": 0.0}, EINVAL, b"damping"), ({"damping": -1.0}, EINVAL, b"damping"), ({"damping": nan}, EINVAL, b"damping"),
           ({"damping": inf}, EINVAL, b"damping"), ({"step_cap": 0.0}, EINVAL, b"step_cap"), ({"step_cap": nan}, EINVAL, b"step_cap"),
           ({"step_cap": inf}, EINVAL, b"step_cap"), ({"resolve_tol": -1e-9}, EINVAL, b"resolve_tol"), ({"resolve_tol": nan}, EINVAL, b"resolve_tol"),
           ({"resolve_tol": inf}, EINVAL, b"resolve_tol"), ({"margin": nan}, EINVAL, b"margin"), ({"margin": inf}, EINVAL, b"margin"),
           ({"qpos_out": q.data_ptr()}, EINVAL, b"alias"), ({"qpos_out": None}, EINVAL, b"null"), ({"qpos": None}, EINVAL, b"null"),
           ({"seq_offsets": None}, EINVAL, b"null"), ({"cap_body": None}, EINVAL, b"null"), ({"cap_p0": None}, EINVAL, b"null"),
           ({"cap_p1": None}, EINVAL, b"null"), ({"cap_radius": None}, EINVAL, b"null"), ({"pairs": None}, EINVAL, b"null"),
           ({"clearance_before_out": None}, EINVAL, b"all three"), ({"clearance_after_out": None}, EINVAL, b"all three"),
           ({"move_out": None}, EINVAL, b"all three"), ({"n_frames": -1}, EINVAL, b"negative"), ({"n_seq": -1}, EINVAL, b"negative"),
           ({"n_caps": -1}, EINVAL, b"negative"), ({"n_pairs": -2}, EINVAL, b"negative"), ({"n_caps": 0}, EINVAL, b"at least 1"),
           ({"n_pairs": 0}, EINVAL, b"at least 1"), ({"n_caps": 257}, EUNSUPPORTED, b"capsules"), ({"n_pairs": 32769}, EUNSUPPORTED, b"pairs")]
    for kw, code, word in bad:
        rc, msg = raw_call(eng, q, offs, tab, out, **kw)
        assert rc == code and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k       # nothing was launched
    for kw in ({"n_frames": 0}, {"n_seq": 0}, {"n_frames": 0, "qpos": None, "pairs": None, "n_caps": 0, "qpos_out": None},
               {"n_seq": 0, "seq_offsets": None, "n_pairs": 0}):
        rc, msg = raw_call(eng, q, offs, tab, out, **kw)
        assert rc == 0, (kw, msg)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k
    empty = eng.motion_self_collision_repair(torch.zeros((0, eng.nq), dtype=F64, device=DEV()), [0, 0, 0], caps, pairs)
    assert empty["qpos"].shape == (0, eng.nq) and empty["clearance_min_after"].tolist() == [inf, inf] and not empty["repaired_frames"].any()
    assert raw_call(eng, q, offs, tab, out)[0] == 0
    torch.cuda.synchronize()
    assert same(out["qpos"].cpu().numpy(), gpu(case)["qpos"])
    # a planar base is refused: the qpos its caller holds is not in free-joint layout.  (No model of the registry has more than 64
    # bodies or a body in front of its parent: those two refusals are not exercised.)
    from gmr_amd.engine import Engine, EngineError
    from tests.util import compiled
    planar = Engine(compiled("smplx", "galaxea_r1pro"), device=0)
    prob = planar.cm.robot
    pc = collision.skeleton_capsules(prob, 0.03)
    pp = collision.default_pairs(prob, pc)[0]
    ptab = planar.collision_device(pc, pp)
    pq = torch.zeros((4, planar.nq), dtype=F64, device=DEV())
    pout = {k: torch.zeros(sh, dtype=dt, device=DEV()) for k, (sh, dt) in shapes(rows=4, clips=1).items() if k != "qpos"}
    pout["qpos"] = torch.zeros_like(pq)
    rc, msg = raw_call(planar, pq, _dev(np.array([0, 4], np.int64)), ptab, pout)
    assert rc == EUNSUPPORTED and b"planar" in msg, (rc, msg)
    with pytest.raises(NotImplementedError):
        planar.motion_self_collision_repair(pq, [0, 4], pc, pp)
    for kw in ({"iterations": 0}, {"damping": 0.0}, {"step_cap": nan}, {"resolve_tol": -1.0}, {"margin": inf}, {"movable": -1}, {"movable": 1 << 64}):
        with pytest.raises(ValueError):
            eng.motion_self_collision_repair(q, offs, caps, pairs, **kw)
    with pytest.raises(EngineError, match="qpos"):
        eng.motion_self_collision_repair(q.float(), offs, caps, pairs)
    with pytest.raises(EngineError, match="must not be qpos"):
        eng.motion_self_collision_repair(q, offs, caps, pairs, out={"qpos": q})


# ------------------------------------------------------------------ 5: the Python layers
def test_the_report_shows_a_colliding_frame_before_the_repair_and_none_after():
    from gmr_amd import GeneralMotionRetargeting, dataset
    g = GeneralMotionRetargeting("smplx", G1, verbose=False)
    q = ci.reach_pose()
    offs = [0, q.shape[0]]
    before = g.self_collision_report(q, offs)
    assert before["colliding_frames"].tolist() == [1] and before["worst_frame"].tolist() == [5] and before["clearance_min"][0] < -0.03
    fixed, info = g.resolve_self_collisions(q, offs)
    after = g.self_collision_report(fixed, offs)
    assert after["colliding_frames"].tolist() == [0] and after["clearance_min"][0] >= 0.0
    assert info["repaired_frames"].tolist() == [1] and info["unresolved_frames"].tolist() == [0] and 0.05 < info["move_max"][0] < 0.2
    assert same(fixed.cpu().numpy(), gpu("reach")["qpos"]) and same(info["clearance_after"], gpu("reach")["clearance_after"])
    keep = np.arange(q.shape[0]) != 5
    assert same(fixed.cpu().numpy()[keep], q[keep])
    # a margin takes the rest_margin table: the pair that rests 0.27 mm apart at the right hip is not in it, so nothing stays unresolved
    wide, winfo = dataset.resolve_self_collisions(g, _dev(q), offs, margin=0.005)
    assert winfo["unresolved_frames"].tolist() == [0] and winfo["clearance_min_after"][0] >= 0.005 - RR.RESOLVE_TOL
    assert same(wide.cpu().numpy(), run("unitree_g1", q, offs, *ri.tables("g1_margin"), margin=0.005)["qpos"])
    # frozen arms: the hand stays in the head
    arms = [n for n in g.model.body_names if "shoulder" in n or "elbow" in n or "wrist" in n]
    stuck, sinfo = g.resolve_self_collisions(q, offs, freeze_bodies=arms)
    assert sinfo["unresolved_frames"].tolist() == [1] and same(stuck.cpu().numpy(), q)
