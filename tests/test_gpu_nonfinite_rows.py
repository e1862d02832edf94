"""Non-finite qpos rows through every kernel that takes a solved qpos (the cases, sets and predictor of tests/nonfinite_cases.py).

For every call the clean input runs once; then every case of the table -- ONE coordinate of ONE frame replaced by +NaN, -NaN, +inf
or -inf -- and
  (a) outside the case's dependency set every output is byte for byte the clean run's: a poisoned row stays in its own frame, through
      the LDS stages, the tile overlays, the halo lanes and the wave-wide decisions;
  (b) inside the set the non-finite mask is the predictor's (the oracle / numpy on the same input), listed exceptions included;
  (c) +NaN and -NaN give the same mask: nothing hangs on the sign bit of a NaN.
Outputs the caller owns are pre-filled with a finite sentinel, so that "not written" and "written as NaN" differ.  A non-finite
float in a data array is ordinary input: no index, offset or loop bound of these kernels is computed from data.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import nonfinite_cases as NF  # noqa: E402
from tests.util import compiled  # noqa: E402

SENTINEL = 12345.0
ROBOTS2 = ["unitree_g1", "unitree_g1_with_hands"]   # the epilogue and the tracking export also on the largest LDS image
GROUP = ["unitree_g1_with_hands", "booster_k1"]     # the largest tree next to a small one in one grid; member 0 is poisoned
_ENGINES, _GROUPS = {}, {}


def _engine(robot):
    from gmr_amd.engine import Engine
    if robot not in _ENGINES:
        _ENGINES[robot] = Engine(compiled("smplx", robot), device=0)
    return _ENGINES[robot]


def _group():
    from gmr_amd.engine import EngineGroup
    if "g" not in _GROUPS:
        _GROUPS["g"] = EngineGroup([compiled("smplx", r) for r in GROUP], device=0)
    return _GROUPS["g"]


def _up(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the tables' clean arrays are read-only)


def _full(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _sweep(call, cases, run, clean_in, poisoned, dep, pred):
    """run(input) -> {name: array} on the GPU; poisoned(case) -> input; dep(case) / pred(input) -> {name: mask / values}."""
    clean = run(clean_in)
    for k, v in clean.items():
        assert not (v == SENTINEL).any(), (call, k, "an element the clean run did not write")
    masks = {}
    for case in cases:
        x = poisoned(case)
        got, d, p = run(x), dep(case), pred(x)
        for k in got:
            assert got[k].shape == d[k].shape == p[k].shape and got[k].dtype == clean[k].dtype, (call, case, k)
            out = ~d[k]
            assert np.array_equal(_bits(got[k])[out], _bits(clean[k])[out]), \
                (call, case, k, "(a) changed outside the set", np.argwhere(out & (_bits(got[k]) != _bits(clean[k])))[:8].tolist())
            m, pm = NF.nonfinite(got[k]), NF.listed_mask(call, case, k, NF.nonfinite(p[k]))
            assert np.array_equal(m[d[k]], pm[d[k]]), \
                (call, case, k, "(b) mask differs from the predicted one", NF.exception_for(call, case, k), np.argwhere(d[k] & (m != pm))[:8].tolist())
            masks[case, k] = m
    twins = 0
    for (case, k), m in masks.items():
        twin = case._replace(value="-nan")
        if case.value == "+nan" and (twin, k) in masks:
            assert np.array_equal(m, masks[twin, k]), (call, case, k, "(c) +NaN and -NaN differ", np.argwhere(m != masks[twin, k])[:8].tolist())
            twins += 1
    assert twins
    return clean


# ------------------------------------------------------------------ gmr_fk, gmr_fk_shape, gmr_fk_min_height
def _fk_run(robot, want_rot, shape=None):
    eng = _engine(robot)
    t = NF.robot_tree(robot)
    sh = None if shape is None else _up(shape)

    def run(q):
        rp, rr, dof = (_up(x) for x in NF.fk_inputs(q))
        bp = _full((NF.N, t.nb, 3), torch.float32)
        br = _full((NF.N, t.nb, 4), torch.float32) if want_rot else None
        eng.fk(rp, rr, dof, want_rot=want_rot, out_pos=bp, out_rot=br, fitted_shape=sh)
        return _host({"pos": bp, "rot": br} if want_rot else {"pos": bp})
    return run


@pytest.mark.parametrize("want_rot", [True, False])   # fk_kernel<0> and fk_pos_kernel
def test_fk_rows_stay_in_their_frame(want_rot):
    robot = "unitree_g1"
    _sweep("fk", NF.TABLE, _fk_run(robot, want_rot), NF.clean_qpos(robot), lambda c: NF.poisoned_qpos(robot, c),
           lambda c: NF.dep_fk(robot, c), lambda q: NF.pred_fk(robot, q))


def test_fk_shape_rows_stay_in_their_frame():
    robot = "unitree_g1"
    sh = NF.fitted_shape(robot)
    _sweep("fk", NF.TABLE, _fk_run(robot, True, sh), NF.clean_qpos(robot), lambda c: NF.poisoned_qpos(robot, c),
           lambda c: NF.dep_fk(robot, c), lambda q: NF.pred_fk(robot, q, sh))


def test_fk_min_height_follows_torch_min():
    """low_s is NaN when any body height of the clip is NaN -- for a NaN of either sign --, +-inf take part as values, and the other
    clips keep their minimum to the bit.  (Before the rule was written down, the key of a negative NaN sorted below -inf and won, the
    key of a positive NaN above +inf and lost, and fminf dropped every NaN that was not the root's own height.)"""
    robot = "unitree_g1"
    eng = _engine(robot)

    def run(q):
        rp, rr, dof = (_up(x) for x in NF.fk_inputs(q))
        return _host({"min_z": eng.fk_min_height(rp, rr, dof, NF.OFFS)})
    clean = _sweep("min_height", NF.TABLE, run, NF.clean_qpos(robot), lambda c: NF.poisoned_qpos(robot, c),
                   lambda c: NF.dep_min_height(robot, c), lambda q: NF.pred_min_height(robot, q))
    assert np.array_equal(clean["min_z"], NF.pred_min_height(robot, NF.clean_qpos(robot))["min_z"])   # (the chains agree to the bit)


# ------------------------------------------------------------------ gmr_motion_epilogue, gmr_group_motion_epilogue
def _epilogue_shapes(robot):
    t = NF.robot_tree(robot)
    return {"root_pos": ((NF.N, 3), torch.float64), "root_rot": ((NF.N, 4), torch.float64), "dof_pos": ((NF.N, t.ndof), torch.float64),
            "local_body_pos": ((NF.N, t.nb, 3), torch.float32), "min_z": ((NF.S,), torch.float32)}


@pytest.mark.parametrize("height,origin", NF.EPILOGUE_FLAGS)
@pytest.mark.parametrize("robot", ROBOTS2)
def test_epilogue_rows_stay_in_their_frame(robot, height, origin):
    eng = _engine(robot)

    def run(q):
        o = {k: _full(*sd) for k, sd in _epilogue_shapes(robot).items()}
        eng.motion_epilogue(_up(q), NF.OFFS, height_adjust=height, root_origin_offset=origin, ground_offset=NF.GROUND,
                            out=tuple(o[k] for k in NF.EPILOGUE_KEYS[:4]), min_z=o["min_z"])
        return _host(o)
    _sweep("epilogue", NF.TABLE, run, NF.clean_qpos(robot), lambda c: NF.poisoned_qpos(robot, c),
           lambda c: NF.dep_epilogue(robot, c, height, origin), lambda q: NF.pred_epilogue(robot, q, height, origin))


def test_group_epilogue_poison_stays_in_its_member():
    g = _group()
    other = _up(NF.clean_qpos(GROUP[1]))

    def call(q):
        mz = [_full((NF.S,), torch.float32) for _ in GROUP]
        res = g.motion_epilogue([(_up(q), NF.OFFS), (other, NF.OFFS)], ground_offset=NF.GROUND, min_z=mz)
        return [_host(dict(zip(NF.EPILOGUE_KEYS, tuple(r) + (z,)))) for r, z in zip(res, mz)]
    state = {}

    def run(q):
        state["all"] = call(q)
        if "other" in state:   # the member whose input is clean: every byte of every output
            for k, v in state["all"][1].items():
                assert np.array_equal(_bits(v), _bits(state["other"][k])), ("group epilogue", k, "the clean member changed")
        else:
            state["other"] = state["all"][1]
        return state["all"][0]
    _sweep("epilogue", NF.TABLE, run, NF.clean_qpos(GROUP[0]), lambda c: NF.poisoned_qpos(GROUP[0], c),
           lambda c: NF.dep_epilogue(GROUP[0], c, True, True), lambda q: NF.pred_epilogue(GROUP[0], q, True, True))


# ------------------------------------------------------------------ gmr_motion_track, gmr_group_motion_track
def _track_shapes(robot, rate):
    t, M = NF.robot_tree(robot), NF.plan(rate).M
    sh = {"root_pos": (M, 3), "root_rot": (M, 4), "joint_pos": (M, t.ndof), "root_lin_vel": (M, 3), "root_ang_vel": (M, 3),
          "joint_vel": (M, t.ndof), "body_pos_w": (M, t.nb, 3), "body_quat_w": (M, t.nb, 4), "body_lin_vel_w": (M, t.nb, 3),
          "body_ang_vel_w": (M, t.nb, 3)}
    return {k: (sh[k], torch.float32 if k.startswith("body") else torch.float64) for k in NF.TRACK_KEYS}


@pytest.mark.parametrize("rate", list(NF.TRACK_RATES))
@pytest.mark.parametrize("robot", ROBOTS2)
def test_tracking_rows_stay_in_their_frames(robot, rate):
    eng = _engine(robot)
    p = NF.plan(rate)

    def run(q):
        o = {k: _full(*sd) for k, sd in _track_shapes(robot, rate).items()}
        res = eng.motion_track(_up(q), NF.OFFS, p.fps_in, p.fps_out, out=o, bodies=True)
        assert np.array_equal(res.out_offsets, p.out_offs)
        return _host(o)
    _sweep("track", NF.track_table(rate), run, NF.clean_qpos(robot), lambda c: NF.poisoned_qpos(robot, c),
           lambda c: NF.dep_track(robot, c, rate), lambda q: NF.pred_track(robot, q, rate))


def test_group_tracking_poison_stays_in_its_member():
    g, rate = _group(), "30to50"
    p = NF.plan(rate)
    other = _up(NF.clean_qpos(GROUP[1]))
    state = {}

    def run(q):
        res = g.motion_track([(_up(q), NF.OFFS, p.fps_in), (other, NF.OFFS, p.fps_in)], p.fps_out, bodies=True)
        both = [_host(dict(r)) for r in res]
        if "other" in state:
            for k, v in both[1].items():
                assert np.array_equal(_bits(v), _bits(state["other"][k])), ("group tracking", k, "the clean member changed")
        else:
            state["other"] = both[1]
        return both[0]
    _sweep("track", NF.track_table(rate), run, NF.clean_qpos(GROUP[0]), lambda c: NF.poisoned_qpos(GROUP[0], c),
           lambda c: NF.dep_track(GROUP[0], c, rate), lambda q: NF.pred_track(GROUP[0], q, rate))


# ------------------------------------------------------------------ gmr_evaluate
def test_evaluate_rows_stay_in_their_frame():
    robot = "unitree_g1"
    eng = _engine(robot)
    pos, quat, sc = NF.keypoints(robot)
    dpos, dquat = _up(pos), _up(quat)

    def run(q):
        err, xp, xq, terr = eng.evaluate(_up(q), dpos, dquat, sc, want_errors=True, want_poses=True, want_task_errors=True)
        return _host({"err": err, "task_err": terr, "xpos": xp, "xquat": xq})
    _sweep("evaluate", NF.TABLE, run, NF.clean_qpos(robot), lambda c: NF.poisoned_qpos(robot, c),
           lambda c: NF.dep_evaluate(robot, c), lambda q: NF.pred_evaluate(robot, q))


# ------------------------------------------------------------------ gmr_dof_to_rot, gmr_rot_to_dof, gmr_local_rot_to_global
@pytest.mark.parametrize("op", ["dof_to_rot", "rot_to_dof", "local_rot_to_global"])
def test_kin_op_rows_stay_in_their_frame(op):
    robot = "unitree_g1"
    eng = _engine(robot)
    x0, cases = NF.kin_setup(robot, op)
    shape = NF.pred_kin(robot, op, x0)["out"].shape

    def run(x):
        out = _full(shape, torch.float32)
        getattr(eng, op)(_up(x), out=out)
        return _host({"out": out})
    _sweep(op, cases, run, x0, lambda c: NF.kin_poisoned(robot, op, c), lambda c: NF.dep_kin(robot, op, c), lambda x: NF.pred_kin(robot, op, x))
