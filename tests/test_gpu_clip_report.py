"""The clip report kernel (gmr_clip_report / gmr_group_clip_report) on the GPU, against an independent float64 numpy reference
built on tests/ik_certificate.IKCertificate (fk, prepare_targets, task_errors), and against gmr_evaluate for the stage errors.

Tolerance of the task statistics and of root_turn_max.  The kernel and the certificate take different sincos / sqrt / atan2
paths, so these fields are compared within ten times the largest difference that gmr_evaluate's own task_err_out / xpos_out
(code that predates the report, same device functions) shows against the certificate ON THE SAME INPUTS; the bound is measured
in the test run itself (`_eval_gap`), never taken from the report.  Measured on one MI355X for the cases below:
gmr_evaluate is within 1.1e-15 .. 1.2e-14 of the certificate (hightorque_hi the largest), which makes the bound 1.1e-14 .. 1.2e-13
at the margin of 10; the report's maxima then differ from the certificate by at most 1.8e-15 (task_pos_max, task_rot_max) and
4.4e-16 (root_turn_max), its per-clip sums by at most 8.5e-14 (65 frames).  DESIGN 4.6 holds the same figures.
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd.engine import CLIP_REPORT_LIMIT_EPS, CLIP_REPORT_SEGMENT  # noqa: E402
from tests import ik_certificate as ikc  # noqa: E402
from tests.util import compiled  # noqa: E402

OFFS = np.array([0, 0, 1, 3, 7, 11, 12, 21], dtype=np.int64)  # lengths 0, 1, 2, 4, 4, 1, 9
ROBOTS = ["unitree_g1", "unitree_g1_with_hands", "hightorque_hi", "galaxea_r1pro"]
GROUP = ["unitree_g1", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01"]
MAX_FIELDS = ("err_max", "task_pos_max", "task_rot_max", "dof_step_max", "root_step_max", "root_turn_max")
COUNT_FIELDS = ("near_lo", "near_hi", "nonfinite_frames", "solves_max", "solves_sum")
SUM_FIELDS = ("err_sum", "task_pos_sum", "task_rot_sum")
_GMR = {}


def _gmr(robot):
    from gmr_amd import GeneralMotionRetargeting
    if robot not in _GMR:
        _GMR[robot] = GeneralMotionRetargeting("smplx", robot, device=0)
    return _GMR[robot]


def _random_qpos(robot, N, seed):
    """Hinges uniform within the joint ranges, unit root quaternions (wxyz), root positions around a standing height
    (test_gpu_motion_epilogue._random_qpos); a planar base gets a heading-only quaternion."""
    r = compiled("smplx", robot).robot
    rng = np.random.default_rng(seed)
    hb = sorted(r.hinge_bodies(), key=lambda b: r.qpos_adr[b])
    lim = np.array(r.jnt_range, dtype=np.float64)[hb]
    lo = np.where(lim[:, 0] < lim[:, 1], lim[:, 0], -1.0)
    hi = np.where(lim[:, 0] < lim[:, 1], lim[:, 1], 1.0)
    q = np.empty((N, r.nq))
    q[:, :3] = rng.normal(size=(N, 3)) * [2.0, 2.0, 0.2] + [0.0, 0.0, 0.8]
    w = rng.normal(size=(N, 4))
    if r.planar_base:
        w[:, 1:3] = 0.0
    q[:, 3:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
    q[:, 7:] = rng.uniform(lo, hi, size=(N, len(hb)))
    return q


def _random_keypoints(robot, N, seed, dtype=np.float64):
    """Random key-points for the robot's slots plus one column nothing consumes (first) -- (pos, quat, names)."""
    g = _gmr(robot)
    names = ["_unused"] + list(g.ik_columns)
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(N, len(names), 3)) * 0.5 + [0.0, 0.0, 0.9]).astype(dtype)
    w = rng.normal(size=(N, len(names), 4))
    quat = (w / np.linalg.norm(w, axis=-1, keepdims=True)).astype(dtype)
    return pos, quat, names


# ------------------------------------------------------------------ the reference: numpy float64 on the certificate
def _hinges(robot):
    hb = sorted((int(b) for b in robot.hinge_bodies()), key=lambda b: int(robot.qpos_adr[b]))
    lo = np.array([robot.jnt_range[b][0] if robot.jnt_limited[b] else -np.inf for b in hb], dtype=np.float64)
    hi = np.array([robot.jnt_range[b][1] if robot.jnt_limited[b] else np.inf for b in hb], dtype=np.float64)
    return [int(robot.qpos_adr[b]) for b in hb], lo, hi


def reference_report(robot_name, qpos, pos, quat, names, offs, heights=None, iters=None, limit_eps=CLIP_REPORT_LIMIT_EPS):
    """Every field of the report from its definition; returns a dict of numpy arrays."""
    cm = compiled("smplx", robot_name)
    cert = ikc.IKCertificate(cm.robot, cm.config)
    qadr, lo, hi = _hinges(cm.robot)
    cols = np.unique(cm.slot_columns(names))
    nt0, nt = len(cm.tasks[0]), len(cm.tasks[0]) + len(cm.tasks[1])
    S, nh = len(offs) - 1, len(qadr)
    out = {k: np.zeros((S, 2)) for k in ("err_max", "err_sum")}
    out.update({k: np.zeros((S, nt)) for k in ("task_pos_max", "task_pos_sum", "task_rot_max", "task_rot_sum")})
    out.update(near_lo=np.zeros((S, nh), np.int64), near_hi=np.zeros((S, nh), np.int64), dof_step_max=np.zeros((S, nh)),
               root_step_max=np.zeros(S), root_turn_max=np.zeros(S), solves_max=np.zeros(S, np.int64), solves_sum=np.zeros(S, np.int64),
               nonfinite_frames=np.zeros(S, np.int64))
    qpos, pos, quat = np.asarray(qpos, np.float64), np.asarray(pos, np.float64), np.asarray(quat, np.float64)
    for s in range(S):
        prev = None
        for f in range(int(offs[s]), int(offs[s + 1])):
            q = qpos[f]
            if not (np.isfinite(q).all() and np.isfinite(pos[f, cols]).all() and np.isfinite(quat[f, cols]).all()):
                out["nonfinite_frames"][s] += 1
                prev = None
                continue
            if iters is not None:
                it = int(iters[f]) & 0x3FFFFFFF
                out["solves_max"][s] = max(out["solves_max"][s], it)
                out["solves_sum"][s] += it
            th = q[qadr]
            out["near_lo"][s] += (th - lo <= limit_eps)
            out["near_hi"][s] += (hi - th <= limit_eps)
            if prev is not None:
                out["dof_step_max"][s] = np.maximum(out["dof_step_max"][s], np.abs(th - prev[qadr]))
                d = q[:3] - prev[:3]
                step = np.sqrt(d[0] * d[0] + d[1] * d[1]) if cert.planar else np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                out["root_step_max"][s] = max(out["root_step_max"][s], step)
                if cert.planar:  # wrapped difference of the headings 2 atan2(qz, qw), sign-blind
                    rel = np.array([prev[3] * q[3] + prev[6] * q[6], 0.0, 0.0, prev[3] * q[6] - prev[6] * q[3]])
                else:
                    rel = ikc._qmul(ikc._qconj(prev[3:7]), q[3:7])
                turn = float(np.linalg.norm(ikc.so3_log(ikc._unit(rel))))
                out["root_turn_max"][s] = max(out["root_turn_max"][s], turn)
            prev = q
            targets = cert.prepare_targets(pos[f], quat[f], names, None if heights is None else heights[s])
            xpos, _ = cert.fk(q)
            for k in cert.used_tables():
                e = cert.task_errors(k, q, targets)
                rows = slice(k * nt0, k * nt0 + len(cert.tables[k]))
                dp = np.array([np.linalg.norm(targets[h][0] - xpos[b]) for b, h, _, _ in cert.tables[k]])
                dr = np.linalg.norm(e[:, 3:], axis=1)
                err = np.sqrt(np.sum(e * e))
                out["err_max"][s, k] = max(out["err_max"][s, k], err)
                out["err_sum"][s, k] += err
                out["task_pos_max"][s, rows] = np.maximum(out["task_pos_max"][s, rows], dp)
                out["task_pos_sum"][s, rows] += dp
                out["task_rot_max"][s, rows] = np.maximum(out["task_rot_max"][s, rows], dr)
                out["task_rot_sum"][s, rows] += dr
    return out


def _eval_gap(robot_name, qpos, pos, quat, names, offs, heights=None):
    """The largest difference between gmr_evaluate's task_err_out / xpos_out and the certificate on these inputs (finite frames)."""
    g = _gmr(robot_name)
    cm = compiled("smplx", robot_name)
    cert = ikc.IKCertificate(cm.robot, cm.config)
    cols = g._columns(list(names))
    lens = np.diff(offs)
    hs = None
    if heights is not None:
        hs = torch.from_numpy(np.repeat(np.asarray(heights) / cm.config.human_height_assumption / cm.ratio, lens)).cuda()
    ok = np.isfinite(qpos).all(axis=1) & np.isfinite(pos[:, np.unique(cols)]).all(axis=(1, 2)) & np.isfinite(quat[:, np.unique(cols)]).all(axis=(1, 2))
    _, xp, _, terr = g._engine.evaluate(torch.from_numpy(qpos).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda(), cols,
                                        want_poses=True, want_task_errors=True, height_scale=hs)
    xp, terr = xp.cpu().numpy(), terr.cpu().numpy()
    clip = np.repeat(np.arange(len(lens)), lens)
    nt0 = len(cm.tasks[0])
    gap = 0.0
    for f in np.nonzero(ok)[0]:
        q = np.asarray(qpos[f], np.float64)
        gap = max(gap, float(np.abs(cert.fk(q)[0] - xp[f]).max()))
        targets = cert.prepare_targets(pos[f], quat[f], names, None if heights is None else heights[clip[f]])
        for k in cert.used_tables():
            e = cert.task_errors(k, q, targets)
            gap = max(gap, float(np.abs(e - terr[f, k * nt0:k * nt0 + len(e)]).max()))
    return gap


def _evaluate_errors(robot_name, qpos, pos, quat, names, offs, heights=None, offset_to_ground=False):
    """Per-frame stage errors [N, 2] of gmr_evaluate, on the host."""
    g = _gmr(robot_name)
    cm = compiled("smplx", robot_name)
    hs = None
    if heights is not None:
        hs = torch.from_numpy(np.repeat(np.asarray(heights) / cm.config.human_height_assumption / cm.ratio, np.diff(offs))).cuda()
    err, _, _ = g._engine.evaluate(torch.from_numpy(qpos).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda(),
                                   g._columns(list(names)), height_scale=hs, offset_to_ground=offset_to_ground)
    return err.cpu().numpy()


def _report(robot_name, qpos, pos, quat, names, offs, **kw):
    return _gmr(robot_name).clip_report(qpos, pos, quat, names, offs, **kw).numpy()


def _check_against_evaluate(rep, err, offs, finite=None):
    """err_max bitwise the per-clip max of gmr_evaluate's err_out; err_sum within len * 2^-52 * sum of its sum."""
    for s in range(len(offs) - 1):
        e = err[offs[s]:offs[s + 1]]
        if finite is not None:
            e = e[finite[offs[s]:offs[s + 1]]]
        want_max = e.max(axis=0) if len(e) else np.zeros(2)
        assert np.array_equal(rep.err_max[s], want_max), (s, rep.err_max[s], want_max)
        want_sum = e.sum(axis=0) if len(e) else np.zeros(2)
        assert (np.abs(rep.err_sum[s] - want_sum) <= len(e) * 2.0 ** -52 * want_sum).all(), (s, rep.err_sum[s], want_sum)


def _check_against_reference(rep, ref, offs, tol, what=""):
    lens = np.diff(offs)
    for k in COUNT_FIELDS:
        got = getattr(rep, k)
        if got is not None:
            assert np.array_equal(got.astype(np.int64), ref[k]), (what, k)
    assert np.array_equal(rep.dof_step_max, ref["dof_step_max"]), what
    assert np.array_equal(rep.root_step_max, ref["root_step_max"]), what
    print(f"{what}: tolerance {tol:.3e}; differences "
          + ", ".join(f"{k} {np.abs(getattr(rep, k) - ref[k]).max(initial=0.0):.3e}" for k in ("task_pos_max", "task_rot_max", "root_turn_max", "task_pos_sum", "task_rot_sum")))
    for k in ("task_pos_max", "task_rot_max", "root_turn_max"):
        assert np.abs(getattr(rep, k) - ref[k]).max(initial=0.0) <= tol, (what, k)
    for k in ("task_pos_sum", "task_rot_sum"):
        assert (np.abs(getattr(rep, k) - ref[k]) <= lens[:, None] * tol).all(), (what, k)
    # the certificate's own stage errors, to the same bound (sqrt of a sum over <= 32 tasks x 6 of squares)
    assert np.abs(rep.err_max - ref["err_max"]).max() <= 14 * tol, what


@functools.lru_cache(maxsize=None)
def _random_case(robot):
    N = int(OFFS[-1])
    seed = 100 + ROBOTS.index(robot) if robot in ROBOTS else 200 + GROUP.index(robot)
    qpos = _random_qpos(robot, N, seed)
    pos, quat, names = _random_keypoints(robot, N, seed + 50, np.float32 if robot == "hightorque_hi" else np.float64)
    heights = [1.6, 1.8, 1.75, 1.7, 1.66, 1.9, 1.72]
    iters = np.random.default_rng(seed).integers(2, 20, size=N).astype(np.int32)
    ref = reference_report(robot, qpos, pos, quat, names, OFFS, heights, iters)
    return qpos, pos, quat, names, heights, iters, ref


def test_reference_is_not_vacuous():
    """(CPU part) The random cases exercise every statistic: the reference itself holds non-zero entries."""
    for robot in ROBOTS:
        ref = _random_case(robot)[-1]
        assert ref["dof_step_max"].max() > 0 and ref["root_step_max"].max() > 0 and ref["root_turn_max"].max() > 0, robot
        assert ref["task_pos_max"].max() > 0 and ref["task_rot_max"].max() > 0 and ref["solves_sum"].sum() > 0, robot
        assert (ref["dof_step_max"][[0, 1, 5]] == 0).all() and (ref["root_step_max"][[0, 1, 5]] == 0).all()  # clips of 0 / 1 frames
    assert _random_case("galaxea_r1pro")[-1]["err_max"][:, 1].max() == 0  # table 2 unused


@pytest.mark.parametrize("robot", ROBOTS)
def test_random_qpos_matches_reference_for_every_segment_length(robot):
    qpos, pos, quat, names, heights, iters, ref = _random_case(robot)
    tol = 10.0 * _eval_gap(robot, qpos, pos, quat, names, OFFS, heights)
    assert 0 < tol < 1e-9, tol
    err = _evaluate_errors(robot, qpos, pos, quat, names, OFFS, heights)
    reps = {}
    for seg in (4, 1, 3, 64):
        reps[seg] = rep = _report(robot, qpos, pos, quat, names, OFFS, human_heights=heights, iters=iters, segment_frames=seg)
        assert rep.frames.tolist() == np.diff(OFFS).tolist()
        _check_against_reference(rep, ref, OFFS, tol, f"{robot} segment {seg}")
        _check_against_evaluate(rep, err, OFFS)
        for k in MAX_FIELDS + COUNT_FIELDS + SUM_FIELDS:
            assert (getattr(rep, k)[0] == 0).all(), k  # the empty clip
    lens = np.diff(OFFS)
    for seg in (1, 3, 64):
        for k in MAX_FIELDS + COUNT_FIELDS:
            assert np.array_equal(getattr(reps[seg], k), getattr(reps[4], k)), (seg, k)
        for k in SUM_FIELDS:
            a, b = getattr(reps[seg], k), getattr(reps[4], k)
            assert (np.abs(a - b) <= lens.reshape((-1,) + (1,) * (a.ndim - 1)) * 2.0 ** -52 * np.maximum(a, b)).all(), (seg, k)
    again = _report(robot, qpos, pos, quat, names, OFFS, human_heights=heights, iters=iters, segment_frames=4)
    for k in MAX_FIELDS + COUNT_FIELDS + SUM_FIELDS:
        assert np.array_equal(getattr(again, k), getattr(reps[4], k)), k  # the same call twice: bitwise


def test_offset_to_ground_errors_equal_evaluate():
    qpos, pos, quat, names, heights, _, _ = _random_case("unitree_g1")
    err = _evaluate_errors("unitree_g1", qpos, pos, quat, names, OFFS, heights, offset_to_ground=True)
    rep = _report("unitree_g1", qpos, pos, quat, names, OFFS, human_heights=heights, offset_to_ground=True, segment_frames=4)
    _check_against_evaluate(rep, err, OFFS)
    assert not np.array_equal(err, _evaluate_errors("unitree_g1", qpos, pos, quat, names, OFFS, heights))


def test_one_long_clip_with_the_default_segment():
    robot, N = "unitree_g1", 2 * CLIP_REPORT_SEGMENT + 1
    offs = np.array([0, N], dtype=np.int64)
    qpos = _random_qpos(robot, N, 7)
    pos, quat, names = _random_keypoints(robot, N, 8, np.float32)
    iters = np.arange(N, dtype=np.int32) % 11 + 1
    ref = reference_report(robot, qpos, pos, quat, names, offs, None, iters)
    tol = 10.0 * _eval_gap(robot, qpos, pos, quat, names, offs)
    rep = _report(robot, qpos, pos, quat, names, offs, iters=iters)
    _check_against_reference(rep, ref, offs, tol, "one long clip")
    _check_against_evaluate(rep, _evaluate_errors(robot, qpos, pos, quat, names, offs), offs)
    whole = _report(robot, qpos, pos, quat, names, offs, iters=iters, segment_frames=N)
    for k in MAX_FIELDS + COUNT_FIELDS:
        assert np.array_equal(getattr(whole, k), getattr(rep, k)), k


def test_hand_made_limits_jumps_and_nonfinite_frames():
    robot, eps = "unitree_g1", 1e-3
    cm = compiled("smplx", robot)
    qadr, lo, hi = _hinges(cm.robot)
    offs = np.array([0, 12, 20], dtype=np.int64)
    N = 20
    lim = [j for j in range(len(qadr)) if np.isfinite(lo[j]) and hi[j] - lo[j] > 0.5]
    a, b, c, d, e = lim[:5]
    q0 = np.zeros(cm.robot.nq)
    q0[:7] = [0.1, -0.2, 0.8, 1.0, 0.0, 0.0, 0.0]
    q0[7:] = np.where(np.isfinite(lo), 0.5 * (lo + hi), 0.0)
    qpos = np.tile(q0, (N, 1))
    qpos[2:4, 7 + a] = lo[a] + eps / 2      # counted twice
    qpos[2, 7 + b] = lo[b] + 2 * eps        # not counted
    qpos[5, 7 + c] = hi[c] - eps / 2        # counted
    qpos[5, 7 + d] = hi[d] - 2 * eps        # not counted
    qpos[7:12, 7 + e] += 0.25               # one jump of 0.25 rad between frames 6 and 7
    qpos[9:12, :3] += [0.3, 0.4, 0.0]       # one root jump of 0.5 m between frames 8 and 9
    qpos[10:12, 3:7] = [np.cos(0.5), 0.0, 0.0, np.sin(0.5)]  # one root turn of 1 rad between frames 9 and 10
    qpos[4, 7 + lim[6]] = np.nan            # a non-finite qpos frame mid-clip: the steps 3 -> 4 and 4 -> 5 do not count
    qpos[14:20, 7 + e] += 0.125             # second clip: one jump of 0.125 rad between frames 13 and 14
    pos, quat, names = _random_keypoints(robot, N, 9)
    pos[16, 1 + 3, 1] = np.nan              # one non-finite consumed key-point in the second clip
    pos[17, 0] = np.nan                     # the column nothing consumes: not counted
    ref = reference_report(robot, qpos, pos, quat, names, offs, limit_eps=eps)
    # the reference itself, on the CPU: no vacuous pass
    assert ref["near_lo"][0, a] == 2 and ref["near_lo"][0, b] == 0 and ref["near_hi"][0, c] == 1 and ref["near_hi"][0, d] == 0
    assert ref["near_lo"].sum() == 2 and ref["near_hi"].sum() == 1
    assert abs(ref["dof_step_max"][0, e] - 0.25) < 1e-15 and abs(ref["dof_step_max"][1, e] - 0.125) < 1e-15
    assert ref["dof_step_max"][0, a] > 0 and ref["dof_step_max"][0, lim[6]] == 0
    assert abs(ref["root_step_max"][0] - 0.5) < 1e-15 and ref["root_step_max"][1] == 0
    assert abs(ref["root_turn_max"][0] - 1.0) < 1e-15 and ref["root_turn_max"][1] == 0
    assert ref["nonfinite_frames"].tolist() == [1, 1]
    tol = 10.0 * _eval_gap(robot, qpos, pos, quat, names, offs)
    finite = np.ones(N, bool)
    finite[[4, 16]] = False
    err = _evaluate_errors(robot, np.where(np.isfinite(qpos), qpos, 0.0), np.where(np.isfinite(pos), pos, 0.0), quat, names, offs)
    for seg in (4, 0, 1):
        rep = _report(robot, qpos, pos, quat, names, offs, limit_eps=eps, segment_frames=seg)
        _check_against_reference(rep, ref, offs, tol, f"hand-made, segment {seg}")
        _check_against_evaluate(rep, err, offs, finite)
        assert rep.solves_max is None and rep.solves_sum is None  # no iters: untouched


def test_real_retarget_result_on_hard_clips():
    robot = "unitree_g1"
    g, cm = _gmr(robot), compiled("smplx", robot)
    pos, quat, names, offs, _ = synth.synth_clips(cm, 3, 40, seed=5, hard=True, dtype=np.float32)
    offs = np.asarray(offs, dtype=np.int64)
    qpos, iters = g.retarget_batch(pos, quat, names, seq_offsets=offs, return_iters=True)
    ref = reference_report(robot, qpos, pos, quat, names, offs, None, iters)
    assert ref["solves_sum"].min() >= 40 and ref["dof_step_max"].max() > 0
    tol = 10.0 * _eval_gap(robot, qpos, pos.astype(np.float32), quat, names, offs)
    rep = _report(robot, qpos, pos, quat, names, offs, iters=iters)
    _check_against_reference(rep, ref, offs, tol, "retarget_batch result")
    _check_against_evaluate(rep, _evaluate_errors(robot, qpos, pos, quat, names, offs), offs)
    assert rep.task_pos_max.max() < 0.5 and np.allclose(rep.solves_mean, ref["solves_sum"] / 40.0)


def test_group_report_is_bitwise_the_members_single_reports():
    from gmr_amd import MultiRobotRetargeting
    mr = MultiRobotRetargeting("smplx", GROUP, device=0)
    N = int(OFFS[-1])
    names = ["_unused"] + list(mr.ik_columns)
    rng = np.random.default_rng(77)
    pos = rng.normal(size=(N, len(names), 3)) * 0.5 + [0.0, 0.0, 0.9]
    w = rng.normal(size=(N, len(names), 4))
    quat = w / np.linalg.norm(w, axis=-1, keepdims=True)
    qpos = {r: _random_qpos(r, N, 300 + i) for i, r in enumerate(GROUP)}
    iters = {r: rng.integers(1, 12, size=N).astype(np.int32) for r in GROUP}
    heights = [1.6, 1.8, 1.75, 1.7, 1.66, 1.9, 1.72]
    got = mr.clip_report(qpos, pos, quat, names, OFFS, human_heights=heights, iters=iters, segment_frames=4)
    tp, tq = torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda()
    for r, eng, cm in zip(GROUP, mr.engines, mr._cms):
        hs = np.asarray(heights) / cm.config.human_height_assumption / cm.ratio
        one = eng.clip_report(torch.from_numpy(qpos[r]).cuda(), OFFS, tp, tq, cm.slot_columns(names), height_scale=hs,
                              iters=torch.from_numpy(iters[r]).cuda(), segment_frames=4).numpy()
        g = got[r].numpy()
        for k in MAX_FIELDS + COUNT_FIELDS + SUM_FIELDS:
            assert np.array_equal(getattr(g, k), getattr(one, k)), (r, k)
        assert g.task_names == one.task_names and g.hinge_names == one.hinge_names and len(g.hinge_names) == eng.nq - 7
        assert g.dof_step_max.max() > 0 and g.err_max.max() > 0
    # a member without work
    some = mr.group.clip_report([None, {"qpos": torch.from_numpy(qpos[GROUP[1]]).cuda(), "seq_offsets": OFFS}, None, None, None])
    assert some[0] is None and some[1].err_max is None
    assert np.array_equal(some[1].numpy().dof_step_max, reference_report(GROUP[1], qpos[GROUP[1]], pos, quat, names, OFFS)["dof_step_max"])
    mr.close()


def test_null_outputs_refusals_and_the_empty_batch():
    import ctypes as C
    from gmr_amd import _native
    from gmr_amd.engine import EngineError, _report_input
    robot = "unitree_g1"
    g = _gmr(robot)
    eng = g._engine
    qpos, pos, quat, names, heights, iters, _ = _random_case(robot)
    cols = g._columns(list(names))
    tq, tp, tqu = torch.from_numpy(qpos).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda()
    full = eng.clip_report(tq, OFFS, tp, tqu, cols, segment_frames=4).numpy()
    # without key-points the error fields are not computed, the others are the same
    bare = eng.clip_report(tq, OFFS, segment_frames=4).numpy()
    assert bare.err_max is None and bare.task_pos_sum is None and bare.solves_max is None
    for k in ("near_lo", "near_hi", "dof_step_max", "root_step_max", "root_turn_max", "nonfinite_frames"):
        assert np.array_equal(getattr(bare, k), getattr(full, k)), k
    lib, stream = eng._lib, eng._stream()
    prm = _native.ClipReportParams(CLIP_REPORT_LIMIT_EPS, 4, 0)
    # any output pointer may be NULL
    ri, rep, keep = _report_input(eng, tq, tp, tqu, cols, OFFS, None, None)
    ri.err_sum_out = ri.task_rot_max_out = ri.near_hi_out = ri.root_step_max_out = ri.nonfinite_frames_out = None
    for t in (rep.err_sum, rep.task_rot_max, rep.near_hi, rep.root_step_max, rep.nonfinite_frames):
        t.fill_(7)
    assert lib.gmr_clip_report(eng._h, C.byref(ri), C.byref(prm), stream) == 0
    part = rep.numpy()
    for k in ("err_max", "task_pos_max", "task_pos_sum", "task_rot_sum", "near_lo", "dof_step_max", "root_turn_max"):
        assert np.array_equal(getattr(part, k), getattr(full, k)), k
    for k in ("err_sum", "task_rot_max", "near_hi", "root_step_max", "nonfinite_frames"):
        assert (getattr(part, k) == 7).all(), k

    def refused(change, params=prm):
        ri, rep, keep = _report_input(eng, tq, tp, tqu, cols, OFFS, None, None)
        extra = change(ri)
        for k in MAX_FIELDS + SUM_FIELDS + ("near_lo", "near_hi", "nonfinite_frames"):
            getattr(rep, k).fill_(7)
        assert lib.gmr_clip_report(eng._h, C.byref(ri), C.byref(params), stream) == -1
        torch.cuda.synchronize()
        for k in MAX_FIELDS + SUM_FIELDS + ("near_lo", "near_hi", "nonfinite_frames"):
            assert (getattr(rep, k) == 7).all(), k  # nothing was launched
        assert lib.gmr_last_error(eng._h)
        return extra

    short = np.array(OFFS.tolist()[:-1] + [int(OFFS[-1]) - 1], dtype=np.int64)
    refused(lambda ri: setattr(ri, "seq_offsets", short.ctypes.data))
    late = OFFS + 1
    refused(lambda ri: setattr(ri, "seq_offsets", late.ctypes.data))
    down = np.array([0, 0, 1, 7, 3, 11, 12, 21], dtype=np.int64)
    refused(lambda ri: setattr(ri, "seq_offsets", down.ctypes.data))
    refused(lambda ri: None, _native.ClipReportParams(CLIP_REPORT_LIMIT_EPS, -1, 0))

    def no_keypoints(ri):
        ri.human_pos = ri.human_quat = None
    refused(no_keypoints)
    with pytest.raises(ValueError):
        eng.clip_report(tq, [0, 5])
    with pytest.raises(EngineError):
        eng.clip_report(tq.to(torch.float32), OFFS)
    with pytest.raises(EngineError):
        eng.clip_report(tq, OFFS, tp, None, cols)
    with pytest.raises(EngineError):
        eng.clip_report(tq, OFFS, iters=torch.zeros(3, dtype=torch.int32, device="cuda"))
    # an empty batch
    empty = eng.clip_report(tq[:0], [0, 0, 0], tp[:0], tqu[:0], cols, iters=torch.zeros(0, dtype=torch.int32, device="cuda")).numpy()
    for k in MAX_FIELDS + COUNT_FIELDS + SUM_FIELDS:
        assert getattr(empty, k).shape[0] == 2 and (getattr(empty, k) == 0).all(), k
    assert np.isnan(empty.err_mean).all()


def _jump_clips():
    """Three short smooth clips; the second one's key-points jump to another pose half way."""
    cm = compiled("smplx", "unitree_g1")
    pos, quat, names, offs, _ = synth.synth_clips(cm, 3, 30, seed=12, hard=False, dtype=np.float64)
    other = synth.synth_clips(cm, 1, 30, seed=99, hard=False, dtype=np.float64, amp=0.9)
    rs = cm.root_slot
    pos[45:60, :, :] = other[0][15:30] - other[0][15:16, rs:rs + 1] + pos[44:45, rs:rs + 1]  # the other motion, brought to this root position
    quat[45:60] = other[1][15:30]
    return pos, quat, names, np.asarray(offs, dtype=np.int64)


def test_retarget_clips_with_report_returns_the_same_motions():
    from gmr_amd import MultiRobotRetargeting, dataset
    g = _gmr("unitree_g1")
    pos, quat, names, offs = _jump_clips()
    plain = dataset.retarget_clips(g, pos, quat, names, offs)
    motions, rep = dataset.retarget_clips(g, pos, quat, names, offs, report=True)
    for m, w in zip(motions, plain):
        assert all(np.array_equal(m[k], w[k]) for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"))
    assert len(rep) == 3 and rep.solves_sum.min() >= 30 and rep.nonfinite_frames.sum() == 0
    assert rep.dof_step_max[1].max() > 2 * max(rep.dof_step_max[0].max(), rep.dof_step_max[2].max())
    mr = MultiRobotRetargeting("smplx", ["unitree_g1", "booster_t1"], device=0)
    mplain = mr.retarget_clips(pos, quat, names, offs)
    mm, mrep = mr.retarget_clips(pos, quat, names, offs, report=True)
    for r in mr.robots:
        for m, w in zip(mm[r], mplain[r]):
            assert all(np.array_equal(m[k], w[k]) for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"))
    for k in MAX_FIELDS + COUNT_FIELDS + SUM_FIELDS:
        assert np.array_equal(getattr(mrep["unitree_g1"], k), getattr(rep, k)), k
    mr.close()


def test_dataset_script_withholds_and_lists_the_jump_clip(tmp_path):
    from gmr_amd import dataset
    from gmr_amd.scripts import smplx_to_robot_dataset
    from gmr_amd.scripts._walk import hard_motion_names
    pos, quat, names, offs = _jump_clips()
    src = str(tmp_path / "in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, torch.from_numpy(pos), torch.from_numpy(quat), names, offs, fps=30.0)
    files = sorted(os.listdir(src))
    assert len(files) == 3
    # what the script will see: the report of the files as it loads them, without any flag
    base = ["--src_folder", src, "--num_cpus", "2", "--hard_motions"]
    plain, csv_path, hard_path = str(tmp_path / "plain"), str(tmp_path / "rep" / "report.csv"), str(tmp_path / "rep" / "hard.txt")
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", plain, "--report_csv", csv_path]) == 0
    assert sorted(os.listdir(plain)) == [f.replace(".npz", ".pkl") for f in files]  # nothing withheld without a bound
    import csv
    with open(csv_path, newline="") as f:
        rows = list(csv.DictReader(f))
    steps = [max(float(v) for k, v in row.items() if k.endswith(":step_max")) for row in rows]
    assert [row["clip"] for row in rows] == [f.split(".")[0] for f in files]
    jump = steps[1]
    assert jump > 2 * max(steps[0], steps[2])
    out = str(tmp_path / "out")
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", out, "--hard_out", hard_path, "--max_dof_step", repr(0.5 * jump)]) == 0
    assert sorted(os.listdir(out)) == [files[0].replace(".npz", ".pkl"), files[2].replace(".npz", ".pkl")]
    assert hard_motion_names([hard_path]) == [files[1].split(".")[0]]
    for f in os.listdir(out):  # what is written is what the plain run writes
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(plain, f), "rb").read()
    # the list feeds the next run's --hard_motions
    again = str(tmp_path / "again")
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--num_cpus", "2", "--tgt_folder", again, "--hard_motions", hard_path]) == 0
    assert sorted(os.listdir(again)) == sorted(os.listdir(out))
