"""Every rotation kernel on the deterministic edge tables of tests/rotation_edges.py, against the 50-digit reference.

Bound: |kernel - reference| <= max(GPU_FACTOR x FLOAT_WORST[family][output], 8 epsilons x |output|) -- ten times what plain numpy
does on the same table (the kernels chain ~1-ulp fast_rcp / fast_rsqrt where numpy chains correctly rounded operations), nothing
measured on a kernel.  Every case of every table is compared; each test prints its measured maximum (`-s`), DESIGN.md holds them.
Quaternions of the two adapters are compared up to overall sign (their consumers are sign-blind and the API fixes none); the
tracking export's root_rot and the kin-ops outputs are compared as they are.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native  # noqa: E402
from tests import rotation_edges as E  # noqa: E402

vp = C.c_void_p


def _dev():
    return torch.device("cuda", 0)


def _compare(fam, out, got, eps=E.EPS64, sign_free=False):
    """Assert the bound element by element over all input sets of the family; returns (measured maximum, largest ratio to the bound)."""
    ref = E.reference(fam)[out]
    assert len(got) == len(ref)
    worst, ratio = 0.0, 0.0
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
        d = np.abs(g - r)
        if sign_free:
            d = np.minimum(d.max(-1), np.abs(g + r).max(-1))
            b = E.bound(fam, out, 1.0, eps)
        else:
            b = E.bound(fam, out, r, eps)
        worst, ratio = max(worst, float(d.max())), max(ratio, float((d / b).max()))
    print(f"GPU_MAX {fam:24s} {out:14s} measured {worst:.3e}  FLOAT_WORST {E.FLOAT_WORST[fam][out]:.3e}  worst / bound {ratio:.3f}")
    assert ratio <= 1.0, (fam, out, worst, ratio)
    return worst, ratio


# ------------------------------------------------------------------ a. gmr_smplx_keypoints_cols / _in
@functools.lru_cache(maxsize=None)
def _g1_columns():
    from gmr_amd import params
    from gmr_amd.ik_config import load_ik_config
    from gmr_amd.smplx_adapter import SMPLX_JOINT_NAMES, SMPLX_PARENTS
    assert list(SMPLX_PARENTS) == E.SMPLX_PARENTS
    cfg = load_ik_config(params.IK_CONFIG_DICT["smplx"]["unitree_g1"])
    names = sorted({t.human for t in list(cfg.table1) + list(cfg.table2)})
    return [SMPLX_JOINT_NAMES.index(n) for n in names]


def _smplx_call(inp, cols):
    lib, dev = _native.load(), _dev()
    go, fp, parents = inp["go"], inp["fp"], inp["parents"]
    T, J = fp.shape[:2]
    resample = inp["T_out"] is not None
    T_out = inp["T_out"] if resample else T
    jt = np.zeros((T, J, 3), dtype=fp.dtype)
    d_go, d_fp, d_jt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (go, fp, jt))
    B = J if cols is None else len(cols)
    pos = torch.full((T_out, B, 3), float("nan"), dtype=torch.float64, device=dev)
    quat = torch.full((T_out, B, 4), float("nan"), dtype=torch.float64, device=dev)
    oc = None if cols is None else np.asarray(cols, np.int32)
    dt = _native.GMR_DTYPE_F64 if fp.dtype == np.float64 else _native.GMR_DTYPE_F32
    rc = lib.gmr_smplx_keypoints_in(parents.ctypes.data_as(vp), J, J, vp(d_go.data_ptr()), vp(d_fp.data_ptr()), vp(d_jt.data_ptr()), dt, T, T_out,
                                    int(resample), oc.ctypes.data_as(vp) if oc is not None else None, B, vp(pos.data_ptr()), vp(quat.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
    return quat.cpu().numpy()


@pytest.mark.parametrize("fam", ["smplx_chain3", "smplx_small_chain3", "smplx_tree55", "smplx_resample_chain3", "smplx_resample_tree55"])
def test_smplx_keypoints_on_the_edge_tables(fam):
    ins = E.family_inputs(fam)
    full = [_smplx_call(i, None) for i in ins]
    _compare(fam, "quat", full, sign_free=True)
    if fam.endswith("tree55"):   # the 14 columns an IK config reads: 22 live joints, two frames per wavefront -- the same bytes
        cols = _g1_columns()
        assert len(cols) == 14
        for i, f in zip(ins, full):
            assert np.array_equal(_smplx_call(i, cols), f[:, cols])
    if fam in ("smplx_chain3", "smplx_small_chain3"):
        # sincos_n: a lane's result does not depend on what its neighbours hold -- the edge rotation of joint 0 (the root: its
        # output is its local quaternion) among 0.3-rad neighbours and among neighbours that all hold the edge value
        n = ins[0]["n_single"]
        assert np.array_equal(full[0][:n, 0], full[0][n:, 0])


# ------------------------------------------------------------------ b. gmr_bvh_fk_rows
def _bvh_call(inp, layout):
    lib, dev = _native.load(), _dev()
    eul, lpos, offsets, parents = inp["eul"], inp["lpos"], inp["offsets"], inp["parents"]
    T, J = eul.shape[:2]
    if layout == 3:
        rows = np.concatenate([lpos[:, 0], eul.reshape(T, -1)], axis=1)
    else:
        rows = np.concatenate([lpos, eul], axis=2).reshape(T, -1)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets)).to(dev)
    pos = torch.full((T, J, 3), float("nan"), dtype=torch.float64, device=dev)
    quat = torch.full((T, J, 4), float("nan"), dtype=torch.float64, device=dev)
    od = np.asarray(inp["order"], np.int32)
    rc = lib.gmr_bvh_fk_rows(parents.ctypes.data_as(vp), J, od.ctypes.data_as(vp), None, None, 0, layout, vp(d_off.data_ptr()), vp(d_rows.data_ptr()),
                             rows.shape[1], T, inp["scale"], None, J, vp(pos.data_ptr()), vp(quat.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
    return pos.cpu().numpy(), quat.cpu().numpy()


@pytest.mark.parametrize("layout", [3, 6])
@pytest.mark.parametrize("fam", ["bvh_chain3", "bvh_tree33"])
def test_bvh_fk_rows_on_the_edge_tables(fam, layout):
    res = [_bvh_call(i, layout) for i in E.family_inputs(fam)]   # one launch per axis order
    _compare(fam, "quat", [r[1] for r in res], sign_free=True)
    _compare(fam, "pos", [r[0] for r in res])


# ------------------------------------------------------------------ c, d: unitree_g1
@functools.lru_cache(maxsize=None)
def _engine():
    from gmr_amd import GeneralMotionRetargeting
    return GeneralMotionRetargeting("smplx", "unitree_g1", device=0)._engine


def test_dof_to_rot_on_the_angle_grid():
    dof = E.family_inputs("dof_to_rot")[0]["dof"]
    got = _engine().dof_to_rot(torch.from_numpy(dof).to(_dev())).cpu().numpy().astype(np.float64)
    _compare("dof_to_rot", "quat", [got], eps=E.EPS32)


def test_rot_to_dof_on_the_threshold_and_clamp_table():
    rot = E.family_inputs("rot_to_dof")[0]["rot"]
    got = _engine().rot_to_dof(torch.from_numpy(rot).to(_dev())).cpu().numpy().astype(np.float64)
    _compare("rot_to_dof", "dof", [got], eps=E.EPS32)


def test_motion_track_on_the_pair_grid():
    i = E.family_inputs("track")[0]
    tr = _engine().motion_track(torch.from_numpy(i["qpos"]).to(_dev()), i["offs"], i["fps_in"], E.TRACK_FPS_OUT, bodies=False)
    assert np.array_equal(np.asarray(tr.out_offsets), i["out_offs"])
    rot, vel = tr["root_rot"].cpu().numpy(), tr["root_ang_vel"].cpu().numpy()
    _compare("track", "root_rot", [rot])
    # the velocities against log(p (x) conj(q)) / h of the call's OWN rows k +- 1
    _, want = E.track_reference(E.MP, i["qpos"], i["offs"], i["out_offs"], i["ratio"], E.TRACK_FPS_OUT, rows=rot)
    d = np.abs(vel - want)
    b = E.bound("track", "root_ang_vel", want)
    print(f"GPU_MAX {'track':24s} {'root_ang_vel':14s} measured {d.max():.3e}  FLOAT_WORST {E.FLOAT_WORST['track']['root_ang_vel']:.3e}  "
          f"worst / bound {(d / b).max():.3f}")
    assert (d <= b).all(), (float(d.max()), float((d / b).max()))
    # the standing clip: every velocity exactly zero, every row the source row
    a, e = int(i["out_offs"][-2]), int(i["out_offs"][-1])
    assert e - a == 33
    for k in ("root_lin_vel", "root_ang_vel", "joint_vel"):
        assert not tr[k][a:e].cpu().numpy().any(), k
    assert np.array_equal(rot[a:e], np.repeat(i["qpos"][-1:, [4, 5, 6, 3]], e - a, axis=0))


# ------------------------------------------------------------------ e. gmr_evaluate: task_err_out, xpos_out / xquat_out
@pytest.mark.parametrize("robot", ["unitree_g1", "galaxea_r1pro"])
def test_evaluate_task_errors_and_poses_on_the_turn_table(robot):
    """so3_log_factor, the V^-1 block and the sign rule of task_residual (ik_kernel.hip.h) at turns of 0 .. pi + 1e-9 about every body
    axis, one task at a time, 0.1 m beside the body; sincos_fk's ballot with hinge angles up to 3.2 rad and one ulp beyond."""
    from gmr_amd import GeneralMotionRetargeting
    fam = "evaluate_" + robot
    s = E.family_inputs(fam)[0]
    ref = E.reference(fam)
    g = GeneralMotionRetargeting("smplx", robot, device=0)
    eng, cols = g._engine, g._columns(list(s["names"]))
    N = len(s["frames"])
    qpos = torch.from_numpy(np.repeat(s["qpos"][None], N, axis=0)).cuda()
    _, _, _, terr = eng.evaluate(qpos, torch.from_numpy(s["pos"]).cuda(), torch.from_numpy(s["quat"]).cuda(), cols, want_task_errors=True)
    terr = terr.cpu().numpy()
    got = np.stack([terr[f, fr["row"]] for f, fr in enumerate(s["frames"])])
    assert np.isfinite(got).all()
    want = ref["task_err"][0]
    d = E.deviation(fam, "task_err", [got], ref)[0]
    b = E.bound(fam, "task_err", want)
    print(f"GPU_MAX {fam:24s} {'task_err':14s} measured {d.max():.3e}  FLOAT_WORST {E.FLOAT_WORST[fam]['task_err']:.3e}  worst / bound {(d / b).max():.3f}")
    assert (d <= b).all(), (float(d.max()), float((d / b).max()), s["frames"][int(np.argmax((d / b).max(axis=1)))])
    # exactly pi: |omega| = pi, omega = +- the axis; which of the two is decided by a w that is zero to rounding (|w| < 4e-16 at
    # 50 digits), so the sign is printed, not asserted -- the turns of pi -+ 2e-11 above, with |w| = 1e-11 < kLieEps and a sign that
    # is a number, are where mink's rule (w > 0 ? + : -) is asserted, as part of the signed comparison
    tol = float(E.bound(fam, "task_err", np.pi))
    plus = 0
    for f, fr in enumerate(s["frames"]):
        if fr["angle"] == E.TURN_PI:
            om = got[f, 3:]
            assert abs(np.linalg.norm(om) - np.pi) <= tol
            ax = np.zeros(3)
            ax[fr["axis"]] = np.pi
            assert min(np.abs(om - ax).max(), np.abs(om + ax).max()) <= tol, (fr, om)
            plus += om[fr["axis"]] > 0
    print(f"turns of exactly pi on {robot}: omega = +axis in {plus} frames, -axis in {sum(fr['angle'] == E.TURN_PI for fr in s['frames']) - plus}")
    # the hinge-angle run
    _, xp, xq = eng.evaluate(torch.from_numpy(s["hinge_qpos"]).cuda(), want_errors=False, want_poses=True)
    _compare(fam, "xpos", [xp.cpu().numpy()])
    _compare(fam, "xquat", [xq.cpu().numpy()], sign_free=True)


# ------------------------------------------------------------------ f. non-finite key-points stay where they are
def test_non_finite_keypoints_stay_in_their_frame():
    """The bit-31 contract of include/gmr_amd.h through Engine.ik_solve (unitree_g1 / smplx, nine clips, float32): a NaN or an
    inf in a consumed column marks its own frame, leaves every other clip and the frames before it byte for byte as they were, and
    bit 31 of iters says exactly which qpos rows are non-finite; a non-finite value in a column no slot reads changes nothing."""
    from gmr_amd import synth
    from gmr_amd.engine import Engine
    from gmr_amd.schedule import make_items
    from tests.util import compiled
    cm = compiled("smplx", "unitree_g1")
    eng = Engine(cm, 0)
    lens = [40, 7, 33, 21, 35, 12, 28, 9, 16]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos, quat, names, _, _ = synth.synth_clips(cm, 1, int(offs[-1]), seed=23, hard=True, dtype=np.float32, pad_to=55)
    sc = cm.slot_columns(names)
    unused = next(c for c in range(pos.shape[1]) if c not in set(int(v) for v in sc))
    items = make_items(offs)
    clip, frame = 3, 5
    f = int(offs[clip]) + frame

    def run(p):
        q, it, _ = eng.ik_solve(torch.from_numpy(p).cuda(), torch.from_numpy(quat).cuda(), sc, items, launch_order=None)
        torch.cuda.synchronize()
        q, it = q.cpu().numpy(), it.cpu().numpy()
        bad_row = ~np.isfinite(q).all(axis=1)
        assert np.array_equal((it.view(np.uint32) >> 31).astype(bool), bad_row)   # bit 31 <=> a non-finite coordinate in the row
        return q, it

    q0, it0 = run(pos)
    assert np.isfinite(q0).all() and not (it0.view(np.uint32) & 0x40000000).any()   # clean: no bit 30, no bit 31
    for value in (np.nan, np.inf):
        p = pos.copy()
        p[f, int(sc[3]), 1] = value
        q, it = run(p)
        a, e = int(offs[clip]), int(offs[clip + 1])
        assert np.array_equal(q[:a].view(np.uint64), q0[:a].view(np.uint64)) and np.array_equal(it[:a], it0[:a])
        assert np.array_equal(q[e:].view(np.uint64), q0[e:].view(np.uint64)) and np.array_equal(it[e:], it0[e:])
        assert np.array_equal(q[a:f].view(np.uint64), q0[a:f].view(np.uint64)) and np.array_equal(it[a:f], it0[a:f])
        assert it.view(np.uint32)[f] >> 31 and not np.isfinite(q[f]).all()
    p = pos.copy()
    p[f, unused] = np.nan
    q, it = run(p)
    assert np.array_equal(q.view(np.uint64), q0.view(np.uint64)) and np.array_equal(it, it0)
    eng.close()
