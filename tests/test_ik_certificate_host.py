"""The IK certificate (tests/ik_certificate.py) pinned on the CPU, and the oracle put under it.

Three things happen here.  (1) The certificate's pieces are cross-checked against the oracle's -- two restatements that share no
code and no data path (the oracle reads the compiled blob, the certificate the Python-side robot and config): FK, target
preparation, the error norm and the gradient.  (2) The oracle solves the certificate's cases and has to pass them; the values it
reaches are where the thresholds of tests/test_gpu_ik_certificate.py come from (ik_certificate.ORACLE_WORST).  (3) Negative
controls: the oracle's result judged by a certificate whose model is wrong on purpose has to fail by a wide margin -- otherwise
passing would mean nothing.
"""
import numpy as np
import pytest

from oracle.oracle import IKParams, Oracle, WORK_ITEM_DTYPE
from tests import ik_certificate as ikc
from tests import ik_certificate_cases as cases
from tests.util import make_items

CONTROL_FACTOR = 100.0  # a negative control has to miss a threshold by at least this factor


def _random_qpos(robot, rng, spread=2.0):
    q = rng.uniform(-spread, spread, robot.nq)
    q[3:7] = rng.normal(size=4)
    if robot.planar_base:  # what the planar base can reach: its own height, a turn about z
        q[2], q[4:6] = robot.body_pos[0, 2], 0.0
    q[3:7] /= np.linalg.norm(q[3:7])
    return q


def _setup(robot_name, src="smplx", height=None):
    robot, config = cases._registry(src, robot_name)
    cm = cases.compile_model(robot, config, height)
    return robot, config, cm, ikc.IKCertificate(robot, config, height), Oracle(cm.blob)


def _frame(cm, seed=5):
    pos, quat, names, _, _ = cases.synth.synth_clips(cm, 1, 6, seed=seed, hard=True, dtype=np.float64)
    return pos[3], quat[3], names


def _slot_targets(cm, targets):
    return np.array([targets[n][0] for n in cm.slot_names]), np.array([targets[n][1] for n in cm.slot_names])


# ------------------------------------------------------------------ (1) cross-checks
@pytest.mark.parametrize("robot_name", cases.REACHABLE_ROBOTS)
def test_fk_matches_oracle(robot_name):
    robot, _, _, cert, orc = _setup(robot_name)
    rng = np.random.default_rng(1)
    qs = np.stack([_random_qpos(robot, rng, 3.0) for _ in range(8)] + [robot.qpos0])
    xpos, xquat = cert.fk(qs)  # a batch and single rows are the same code
    for q, p, r in zip(qs, xpos, xquat):
        op, oq = orc.fk_mj(q)
        assert np.abs(p - op).max() < 1e-12 and np.abs(r - oq).max() < 1e-12


@pytest.mark.parametrize("robot_name,src,height", [(r, "smplx", None) for r in cases.REACHABLE_ROBOTS] +
                         [("unitree_g1", "smplx", 1.52), ("unitree_g1", "fbx", 1.75), ("booster_t1", "bvh", 1.9)])
def test_prepare_targets_matches_oracle(robot_name, src, height):
    robot, config, cm, cert, orc = _setup(robot_name, src, height)
    pos, quat, names = _frame(cm)
    # columns in another order and one body no table names: the certificate goes by name
    order = np.random.default_rng(2).permutation(len(names))
    pos = np.concatenate([pos[order], [[9.0, 9.0, 9.0]]])
    quat = np.concatenate([quat[order] * 1.7, [[1.0, 0.0, 0.0, 0.0]]])  # un-normalised on purpose
    names = [names[i] for i in order] + ["_nobody_"]
    sc = cm.slot_columns(names)
    tp, tq = orc.prepare_targets(pos[sc], quat[sc])
    targets = cert.prepare_targets(pos, quat, names)
    assert set(targets) == set(cm.slot_names)
    cp, cq = _slot_targets(cm, targets)
    assert np.abs(cp - tp).max() < 1e-12 and np.abs(cq - tq).max() < 1e-12


@pytest.mark.parametrize("robot_name", cases.REACHABLE_ROBOTS)
def test_unit_weight_cost_is_the_stage_error(robot_name):
    """Oracle.stage_error returns the reference's error1() / error2(): the 2-norm of the concatenated UNWEIGHTED 6-vectors of a
    table's tasks (oracle/gmr_oracle.c, stage_error).  That is sqrt(2 cost) with every weight 1 -- and the 6-vectors themselves
    agree one by one."""
    robot, _, cm, cert, orc = _setup(robot_name)
    pos, quat, names = _frame(cm)
    targets = cert.prepare_targets(pos, quat, names)
    tp, tq = _slot_targets(cm, targets)
    rng = np.random.default_rng(3)
    for q in [_random_qpos(robot, rng, 1.0) for _ in range(4)]:
        for k in cert.used_tables():
            assert [(b, h) for b, h, _, _ in cert.tables[k]] == [(b, cm.slot_names[s]) for b, s in zip(cm.task_body[k], cm.task_slot[k])]
            norm, e = orc.stage_error(k, q, tp, tq, len(cert.tables[k]))
            assert np.abs(cert.task_errors(k, q, targets) - e).max() < 1e-12
            assert abs(np.sqrt(2.0 * cert.cost(k, q, targets, unit_weights=True)) - norm) < 1e-12 * max(1.0, norm)


@pytest.mark.parametrize("robot_name", cases.REACHABLE_ROBOTS)
def test_gradient_is_the_linear_term_of_the_oracles_qp(robot_name):
    """c of the QP the oracle builds (sum of (W J)' (W e), analytic Jacobians) is the gradient of the certificate's cost; the
    central difference reproduces it to its own accuracy (FD_STEP: 1e-10 of the cost, relative to a gradient of 1e3 .. 1e5)."""
    robot, _, cm, cert, orc = _setup(robot_name)
    pos, quat, names = _frame(cm)
    targets = cert.prepare_targets(pos, quat, names)
    tp, tq = _slot_targets(cm, targets)
    q = _random_qpos(robot, np.random.default_rng(4), 1.0)
    dof = [0, 1, 5] + list(range(6, robot.nv)) if robot.planar_base else list(range(robot.nv))
    assert len(dof) == len(cert.dofs)
    for k in cert.used_tables():
        _, c, _, _ = orc.build_qp(k, q, tp, tq)
        g = cert.gradient(k, q, targets)
        assert np.abs(g - c[dof]).max() < 1e-8 * np.abs(c).max()


def test_log_series_branches_join():
    """The series arms of the SE(3) log near zero angle against the closed form evaluated just outside them, and the log of
    exp on both sides of the switch."""
    rng = np.random.default_rng(5)
    for ang in (0.0, 1e-12, 3e-9, 0.99e-4, 1.01e-4, 1e-3, 0.5, 3.1):
        axis = rng.normal(size=3)
        w = ang * axis / np.linalg.norm(axis)
        t = rng.normal(size=3)
        e = ikc.se3_log(ikc._qexp(w), t)
        assert np.abs(e[3:] - w).max() < 1e-15 * max(1.0, ang / 1e-3)
        # V(w) e_pos = t, with V = I + (1 - cos a) / a^2 K + (a - sin a) / a^3 K^2 (series below 1e-3: the closed form cancels)
        a = ang
        c1, c3 = (0.5 - a * a / 24.0, 1.0 / 6.0 - a * a / 120.0) if a < 1e-3 else ((1.0 - np.cos(a)) / a ** 2, (a - np.sin(a)) / a ** 3)
        back = e[:3] + c1 * np.cross(w, e[:3]) + c3 * np.cross(w, np.cross(w, e[:3]))
        assert np.abs(back - t).max() < 1e-12
    assert np.abs(ikc.so3_log(-ikc._qexp(np.array([0.3, -0.2, 0.1]))) - np.array([0.3, -0.2, 0.1])).max() < 1e-15  # q and -q


def test_projection_signs():
    """The sign branch on a problem small enough to read: one hinge pushed against its upper bound."""
    robot, config = cases._registry("smplx", "unitree_g1")
    cert = ikc.IKCertificate(robot, config)
    b = int(robot.hinge_bodies()[3])
    k = [i for i, (kind, bb) in enumerate(cert.dofs) if kind == "hinge" and bb == b][0]
    cm = cases.compile_model(robot, config)
    pos, quat, names = _frame(cm)
    targets = cert.prepare_targets(pos, quat, names)
    q = np.array(robot.qpos0)
    g_free = cert.gradient(1, q, targets)
    assert g_free[k] != 0.0
    for side in (0, 1):
        q[int(robot.qpos_adr[b])] = robot.jnt_range[b, side]
        g = cert.gradient(1, q, targets)
        pg = cert.projected_gradient(1, q, targets)
        state, feasible = cert.bound_state(q)
        assert feasible and state[k] == (-1, 1)[side] and np.count_nonzero(state) == 1
        explained = g[k] > 0 if side == 0 else g[k] < 0  # the cost falls only beyond the bound
        assert pg[k] == (0.0 if explained else g[k]) and np.array_equal(np.delete(pg, k), np.delete(g, k))
    q[int(robot.qpos_adr[b])] = robot.jnt_range[b, 1] + 1e-6
    assert np.all(np.isinf(cert.projected_gradient(1, q, targets))) and not cert.bound_state(q)[1]


# ------------------------------------------------------------------ (2) + (3) the oracle under the certificate
def _oracle_final(case, **solver):
    pos, quat, offs = case.held_input()
    prm = IKParams(**{**case.solver, **solver})
    q, it, _ = Oracle(case.cm.blob).ik_solve(pos, quat, case.cm.slot_columns(case.names), make_items(offs, WORK_ITEM_DTYPE), params=prm)
    assert not np.isnan(q).any()
    return q[case.final_rows()]


def _assert_passes(case, got, family):
    print(f"[certificate] oracle {case.name}: {got}")
    for key, bound in ikc.thresholds(family, case.tables).items():
        assert got[key] <= bound, (case.name, key, got[key], bound)


def _assert_controls_fail(case, q_final, family, controls):
    bounds = ikc.thresholds(family, case.tables)
    for control in controls:
        got = cases.certify(case, q_final, control(case, q_final[0]))
        print(f"[certificate] control {control.__name__} on {case.name}: {got}")
        key = f"stat{case.tables[-1]}"
        assert got[key] >= CONTROL_FACTOR * bounds[key], (case.name, control.__name__, got[key], bounds[key])
        ckey = f"cost{case.tables[-1]}"
        if ckey in bounds and np.isfinite(got[key]):
            assert got[ckey] >= CONTROL_FACTOR * bounds[ckey], (case.name, control.__name__, got[ckey], bounds[ckey])


@pytest.mark.parametrize("robot_name", cases.REACHABLE_ROBOTS)
def test_oracle_reachable_targets(robot_name):
    """(a).  The weight control is absent here on purpose: where the residual is zero the gradient is zero under ANY weights, so
    a reachable case cannot see a wrong weight -- that is what the unreachable cases below are for."""
    case = cases.reachable_case(robot_name)
    q_final = _oracle_final(case)
    _assert_passes(case, cases.certify(case, q_final), "reachable")
    _assert_controls_fail(case, q_final, "reachable", [cases.wrong_axis, cases.wrong_offset, cases.wrong_range])


def test_oracle_reachable_targets_with_the_callers_constants():
    """(a) as the class API runs it (tol = 1e-3, max_iter = 10: one or two solves per stage and frame once the error stops
    falling), hence many more held frames; the GPU twin goes through MultiRobotRetargeting.retarget_batch.  unitree_g1_with_hands
    uses unitree_g1's config, so one input is reachable for both."""
    for robot_name in cases.PAIR_ROBOTS:
        case = cases.pair_case(robot_name)
        q_final = _oracle_final(case)
        _assert_passes(case, cases.certify(case, q_final), "reachable_default")
        _assert_controls_fail(case, q_final, "reachable_default", [cases.wrong_axis, cases.wrong_offset, cases.wrong_range])


ALL_CONTROLS = [cases.wrong_axis, cases.wrong_offset, cases.wrong_weight, cases.wrong_range]


def test_oracle_held_reference_frame(golden_dir):
    """(b) 1."""
    case = cases.held_reference_frame_case(golden_dir)
    t1, t2 = case.config.table1, case.config.table2
    assert [(t.frame, t.human) for t in t1] == [(t.frame, t.human) for t in t2]  # the same map ...
    assert [(t.pos_weight, t.rot_weight) for t in t1] != [(t.pos_weight, t.rot_weight) for t in t2]  # ... with other weights
    q_final = _oracle_final(case)
    got = cases.certify(case, q_final)
    assert got["active"] >= 1, "no joint limit active: the sign branch of the projection is not exercised"
    _assert_passes(case, got, "limits")
    _assert_controls_fail(case, q_final, "limits", ALL_CONTROLS)
    # with the caller's constants the frame's last stage is one or two solves after table 1 pulled the robot elsewhere: the
    # result is not stationary for table 2, and the certificate says so (why this case runs its stages long)
    loose = cases.certify(case, _oracle_final(case, max_iter=10, tol=1e-3))
    assert loose["stat1"] > CONTROL_FACTOR * ikc.thresholds("limits", case.tables)["stat1"]


def test_oracle_synthetic_robot_at_its_limits(tmp_path):
    """(b) 2."""
    case = cases.synthetic_limits_case(tmp_path)
    w = lambda tab: [(t.frame, t.human, t.pos_weight, t.rot_weight) for t in tab]  # noqa: E731
    assert w(case.config.table1) == w(case.config.table2)
    q_final = _oracle_final(case)
    got = cases.certify(case, q_final)
    assert got["active"] >= 1, "no joint limit active: the sign branch of the projection is not exercised"
    _assert_passes(case, got, "limits")
    _assert_controls_fail(case, q_final, "limits", ALL_CONTROLS)
    # a limit the model does not know of: the range of one active joint widened -- its gradient component is no longer explained
    import dataclasses
    cert = case.cert()
    state, _ = cert.bound_state(q_final[0])
    b = cert.dofs[int(np.nonzero(state)[0][0])][1]
    rng = case.robot.jnt_range.copy()
    rng[b] = (rng[b, 0] - 0.5, rng[b, 1] + 0.5)
    wide = cases.certify(case, q_final, ikc.IKCertificate(dataclasses.replace(case.robot, jnt_range=rng), case.config))
    assert wide["stat1"] >= CONTROL_FACTOR * ikc.thresholds("limits", case.tables)["stat1"]
