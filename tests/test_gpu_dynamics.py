"""gmr_motion_dynamics on the GPU against the numpy reference (tests/dynamics_reference.py; inputs: tests/dynamics_inputs.py).

The bound.  dynamics_reference.bound: ten times the numpy reference's own distance to its 50-digit evaluator, measured per robot on
the frames of the explicit case themselves (FLOAT_WORST; tests/test_dynamics_host.py re-measures it), as an absolute figure with no
other factor.  Nothing in the bound was measured on a kernel.

Measured on an MI355X (worst |GPU - numpy| over the three robots, explicit qvel / qacc | differenced): see DESIGN.md 4.14."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dynamics_inputs as di  # noqa: E402
from tests import dynamics_reference as R  # noqa: E402
from tests.util import compiled  # noqa: E402

FILL = 0xA5
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
EPS = float(np.finfo(np.float64).eps)
FRAME, STATS = ("tau", "root_wrench", "com", "zmp"), ("tau_abs_max", "tau_rms", "tau_ratio_max", "frames_over_limit",
                                                        "frames_any_over_limit", "fz_ratio_max", "fz_ratio_min", "unloaded_frames", "nonfinite_frames")
COUNTS = ("frames_over_limit", "frames_any_over_limit", "unloaded_frames", "nonfinite_frames")


def DEV():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def engine(robot):
    """The engine of the robot pack (of a synthetic tree: tests/synthetic_trees.py), checked to be the tree the reference reads from
    the MJCF file."""
    from gmr_amd.engine import Engine
    from tests import synthetic_trees
    cm = synthetic_trees.compiled(robot) if synthetic_trees.is_tree(robot) else compiled("smplx", robot)
    rob = R.model(robot)[0]
    assert cm.robot.to_dict() == rob.to_dict()
    return Engine(cm, device=0)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV())   # (a copy: the shared inputs are read-only)


def shapes(robot, rows=di.N, clips=di.S):
    rob = R.model(robot)[0]
    nh, nv = rob.nq - 7, rob.nv
    return {"tau": ((rows, nh), F64), "root_wrench": ((rows, 6), F64), "com": ((rows, 3), F64), "zmp": ((rows, 2), F64),
            "qvel": ((rows, nv), F64), "qacc": ((rows, nv), F64), "tau_abs_max": ((clips, nh), F64), "tau_rms": ((clips, nh), F64),
            "tau_ratio_max": ((clips, nh), F64), "frames_over_limit": ((clips, nh), I32), "frames_any_over_limit": ((clips,), I32),
            "fz_ratio_max": ((clips,), F64), "fz_ratio_min": ((clips,), F64), "unloaded_frames": ((clips,), I32),
            "nonfinite_frames": ((clips,), I32)}


def sentinel_out(robot, names=None, **kw):
    out = {}
    for k, (sh, dt) in shapes(robot, **kw).items():
        if names is None or k in names:
            out[k] = torch.empty(sh, dtype=dt, device=DEV())
            if out[k].numel():
                out[k].view(U8).fill_(FILL)
    return out


def run(robot, q, offs, v=None, a=None, table=None, out=None, **kw):
    tab = R.model(robot)[1] if table is None else table
    res = engine(robot).motion_dynamics(_dev(q), offs, kw.pop("fps", di.FPS), qvel=None if v is None else _dev(v),
                                        qacc=None if a is None else _dev(a), table=tab, out=out, **kw)
    return {k: t.cpu().numpy() for k, t in res.items()}


@functools.lru_cache(maxsize=None)
def gpu(robot, case):
    """The GPU's answer to a named case into pre-filled caller-owned outputs: computed once, shared."""
    if case == "explicit":
        q, v, a = di.explicit(robot)
        return run(robot, q, di.OFFS, v, a, out=sentinel_out(robot))
    return run(robot, di.quantised(robot), di.OFFS, out=sentinel_out(robot))


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------ 1: accuracy
def check_frames(robot, case):
    """The per-frame comparison of a named case: equal shapes and NaN patterns, every output within its bound of the numpy
    reference.  Prints the worst |GPU - numpy| per output and its share of the bound."""
    got, ref = gpu(robot, case), di.reference(robot, case)
    bounds = {k: R.bound(robot, k) for k in FRAME}
    report = []
    for k in FRAME:
        assert got[k].shape == ref[k].shape and np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        with np.errstate(all="ignore"):
            err = np.abs(got[k] - ref[k])
        worst = float(np.nanmax(err)) if np.isfinite(err).any() else 0.0     # (tau of a model without a hinge has no column)
        report.append(f"{k} {worst:.2e} ({worst / bounds[k] if bounds[k] else 0.0:.2f} of its bound)")
    print(f"{robot} {case}: worst |GPU - numpy|: " + ", ".join(report))
    for k in FRAME:
        with np.errstate(all="ignore"):
            assert not np.any(np.abs(got[k] - ref[k]) > bounds[k]), k
    return got, ref


@pytest.mark.parametrize("case", ["explicit", "diff"])
@pytest.mark.parametrize("robot", di.ROBOTS)
def test_frames_equal_the_reference(robot, case):
    assert R.model(robot)[0].nbody == {"unitree_g1": 38, "booster_k1": 23, "unitree_g1_with_hands": 52}[robot]
    _, ref = check_frames(robot, case)
    assert np.isnan(ref["zmp"]).any() and not np.isnan(ref["zmp"]).all()     # both kinds of frame are in the case


def check_pass_through(robot):
    got = gpu(robot, "explicit")
    _, v, a = di.explicit(robot)
    assert np.array_equal(_bytes(got["qvel"]), _bytes(v)) and np.array_equal(_bytes(got["qacc"]), _bytes(a))


@pytest.mark.parametrize("robot", di.ROBOTS)
def test_explicit_velocities_pass_through_bit_for_bit(robot):
    check_pass_through(robot)


def check_differences(robot):
    """On rows that are multiples of 2^-16 at 64 Hz every difference of the linear and hinge parts is exact, so there is one correct
    value and the kernel must give its bits.  The angular part goes through atan2 of two different libraries: it is held to 8
    epsilons of the rate (velocity), and for the acceleration -- a difference of two rates over h -- to 16 epsilons of the rate
    over h."""
    got, ref = gpu(robot, "diff"), di.reference(robot, "diff")
    nv = ref["qvel"].shape[1]
    cols = [0, 1, 2] + list(range(6, nv))
    for k in ("qvel", "qacc"):
        assert np.array_equal(_bytes(got[k][:, cols]), _bytes(ref[k][:, cols])), k
    w = np.abs(ref["qvel"][:, 3:6]).max()
    ev, ea = np.abs(got["qvel"][:, 3:6] - ref["qvel"][:, 3:6]).max(), np.abs(got["qacc"][:, 3:6] - ref["qacc"][:, 3:6]).max()
    print(f"{robot}: angular differences: velocity {ev:.2e} (bound {8 * EPS * w:.2e}), acceleration {ea:.2e} (bound {16 * EPS * w * di.FPS:.2e})")
    assert ev <= 8 * EPS * w and ea <= 16 * EPS * w * di.FPS and w > 1.0
    for s, T in enumerate(di.LENS):   # the short clips: nothing, zero velocity, zero acceleration
        rows = slice(int(di.OFFS[s]), int(di.OFFS[s + 1]))
        if T == 1:
            assert not got["qvel"][rows].any()
        if T in (1, 2):
            assert not got["qacc"][rows].any()


@pytest.mark.parametrize("robot", di.ROBOTS)
def test_differences_are_the_numpy_restatements_bit_for_bit(robot):
    check_differences(robot)


# ------------------------------------------------------------------ 2: statistics
def check_statistics(robot, case):
    """Counts equal the numpy reference's (its own values keep a relative distance of more than 1e-9 from every threshold, asserted
    here).  Maxima and counts are exactly the reference reduction of the GPU's own tau and root_wrench rows, and within the frames'
    bound of the numpy reference.  tau_rms: its sum is added frame by frame in both, so it differs by the rows' own error (the rms
    is 1-Lipschitz in the largest row error) plus n epsilons of itself for the order of the additions."""
    got, ref = gpu(robot, case), di.reference(robot, case)
    tab = R.model(robot)[1]
    m_tau, m_fz = di.margins(robot, ref)
    assert m_tau > 1e-9 and m_fz > 1e-9
    own = R.statistics(tab, got["tau"], got["root_wrench"], di.OFFS)
    for k in COUNTS:
        assert np.array_equal(got[k], ref[k]) and got[k].dtype == np.int32, k
    for k in ("tau_abs_max", "tau_ratio_max", "fz_ratio_max", "fz_ratio_min"):
        assert np.array_equal(_bytes(got[k]), _bytes(own[k])), k
    n = np.array(di.LENS, dtype=np.float64)[:, None]
    slack = R.bound(robot, "tau") + n * EPS * ref["tau_rms"]
    print(f"{robot} {case}: tau_rms worst {np.abs(got['tau_rms'] - ref['tau_rms']).max(initial=0.0):.2e}, against its own rows "
          f"{np.abs(got['tau_rms'] - own['tau_rms']).max(initial=0.0):.2e}")
    assert np.all(np.abs(got["tau_rms"] - ref["tau_rms"]) <= slack) and np.all(np.abs(got["tau_rms"] - own["tau_rms"]) <= n * EPS * own["tau_rms"])
    assert np.all(np.abs(got["tau_abs_max"] - ref["tau_abs_max"]) <= R.bound(robot, "tau"))
    assert not got["tau_abs_max"][:1].any() and not got["tau_rms"][:1].any()     # the empty clip reports 0
    return got, ref


@pytest.mark.parametrize("case", ["explicit", "diff"])
@pytest.mark.parametrize("robot", di.ROBOTS)
def test_statistics_equal_the_reference(robot, case):
    """check_statistics, on a case that has frames over a torque limit and unloaded frames."""
    _, ref = check_statistics(robot, case)
    if robot != "booster_k1":   # (its MJCF gives no torque limits: nothing can be over)
        assert ref["frames_any_over_limit"].sum() > 0
    assert ref["unloaded_frames"].sum() > 0


def test_one_push_over_the_limit_raises_that_clips_counters_only():
    q, v, a, offs, table, (clip, row, j) = di.push_case()
    ref = di.with_statistics("unitree_g1", q, v, a, offs, table)
    assert ref["frames_over_limit"].sum() == 1 and ref["frames_over_limit"][clip, j] == 1 and min(di.margins("unitree_g1", ref, table)) > 1e-9
    got = run("unitree_g1", q, offs, v, a, table=table)
    assert np.array_equal(got["frames_over_limit"], ref["frames_over_limit"]) and got["frames_any_over_limit"].tolist() == [0, 1, 0]
    assert abs(got["tau_ratio_max"][clip, j] - 2.0) <= 1e-12 and np.all(got["tau_ratio_max"][[0, 2]] < 1.0)
    assert np.array_equal(_bytes(got["tau"][0:5]), _bytes(got["tau"][10:15]))    # the clips at rest are the same rows
    assert got["unloaded_frames"].tolist() == [0, 0, 0] and got["nonfinite_frames"].tolist() == [0, 0, 0]
    weight = table.total_mass * 9.81
    assert np.abs(got["root_wrench"][0:5, :3] - [0.0, 0.0, weight]).max() <= 16 * EPS * weight      # statics: the weight
    # another table on the same engine is another upload: the first one's limits are not reused
    again = run("unitree_g1", q, offs, v, a)
    assert np.array_equal(_bytes(again["tau"]), _bytes(got["tau"])) and not np.array_equal(again["tau_ratio_max"], got["tau_ratio_max"])


def test_free_fall_is_unloaded_and_has_no_zmp():
    """root z = z0 - 9.81 t^2 / 2 with fixed hinges: the second difference is -9.81 in every interior frame, so F = 0 there to the
    rounding of z over h^2 (1e-10 N), those T - 2 frames are unloaded and have a NaN ZMP.  By the contract the first and the last
    frame take their neighbour's acceleration, so they fall too: unloaded_frames is T, not T - 2."""
    T = 12
    q, offs = di.free_fall(frames=T)
    got = run("unitree_g1", q, offs)
    interior = slice(1, T - 1)
    assert np.abs(got["root_wrench"][interior]).max() <= 1e-8
    assert np.isnan(got["zmp"][interior]).all() and int(np.isnan(got["zmp"][interior]).all(axis=1).sum()) == T - 2
    assert np.isnan(got["zmp"]).all() and got["unloaded_frames"].tolist() == [T] and got["nonfinite_frames"].tolist() == [0]
    assert np.abs(got["tau"]).max() <= 1e-8 and np.abs(got["fz_ratio_max"]).max() <= 1e-10
    assert np.abs(got["qacc"][:, 2] + 9.81).max() <= 1e-9 and not got["qacc"][:, [0, 1]].any()


# ------------------------------------------------------------------ 3: robustness
def test_a_nan_row_stays_in_its_clip_and_is_counted():
    """A NaN hinge in row 2 of the middle clip of three (6 frames each, differenced): the frames whose stencil reads that row are
    0 .. 3 (frame 0 takes frame 1's acceleration); clips 0 and 2 keep every byte."""
    robot = "unitree_g1"
    q0 = np.array(di.quantised(robot)[int(di.OFFS[8]):int(di.OFFS[8]) + 18])
    offs = np.array([0, 6, 12, 18], np.int64)
    clean = run(robot, q0, offs)
    q1 = q0.copy()
    q1[8, 7 + 3] = np.nan
    got = run(robot, q1, offs)
    ref = di.with_statistics(robot, q1, *R.differences(q1, offs, di.FPS), offs=offs)
    for k, t in got.items():
        per_clip = t.shape[0] == 3
        for s in (0, 2):
            rows = slice(s, s + 1) if per_clip else slice(6 * s, 6 * s + 6)
            assert np.array_equal(_bytes(t[rows]), _bytes(clean[k][rows])), (k, s)
    assert got["nonfinite_frames"].tolist() == ref["nonfinite_frames"].tolist() == [0, 4, 0]
    bad = ~(np.isfinite(got["tau"]).all(axis=1) & np.isfinite(got["root_wrench"]).all(axis=1))
    assert np.flatnonzero(bad).tolist() == [6, 7, 8, 9]
    for k in ("tau", "root_wrench"):
        assert np.array_equal(np.isfinite(got[k]), np.isfinite(ref[k])), k
    for k in ("tau", "root_wrench", "com"):   # the two clean frames of the middle clip, and its statistics over them
        assert np.array_equal(_bytes(got[k][10:12]), _bytes(clean[k][10:12])), k
    own = R.statistics(R.model(robot)[1], got["tau"], got["root_wrench"], offs)
    for k in ("tau_abs_max", "frames_over_limit", "unloaded_frames", "fz_ratio_max", "fz_ratio_min"):
        assert np.array_equal(got[k], own[k]), k
    inf = q0.copy()
    inf[8, 0] = np.inf
    got = run(robot, inf, offs)
    assert got["nonfinite_frames"].tolist() == [0, 4, 0]      # an infinite root x reaches the same four frames
    for k in ("tau", "root_wrench", "zmp", "tau_abs_max", "unloaded_frames"):
        t = got[k]
        for s in (0, 2):
            rows = slice(s, s + 1) if t.shape[0] == 3 else slice(6 * s, 6 * s + 6)
            assert np.array_equal(_bytes(t[rows]), _bytes(clean[k][rows])), (k, s)


@pytest.mark.parametrize("robot", di.ROBOTS)
def test_two_calls_give_identical_bytes(robot):
    q = di.quantised(robot)
    a, b = run(robot, q, di.OFFS, out=sentinel_out(robot)), gpu(robot, "diff")
    for k in a:
        assert np.array_equal(_bytes(a[k]), _bytes(b[k])), k
    c = run(robot, q, di.OFFS)                     # without out the call allocates the same answer
    for k in a:
        assert np.array_equal(_bytes(a[k]), _bytes(c[k])), k


def test_outputs_left_out_are_not_computed_and_rows_outside_every_clip_are_not_written():
    robot = "booster_k1"
    q, v, a = di.explicit(robot)
    full = gpu(robot, "explicit")
    some = run(robot, q, di.OFFS, v, a, out=sentinel_out(robot, names=("tau", "root_wrench", "nonfinite_frames")))
    assert sorted(some) == ["nonfinite_frames", "root_wrench", "tau"]
    for k in some:
        assert np.array_equal(_bytes(some[k]), _bytes(full[k])), k
    only = run(robot, q, di.OFFS, v, a, out=sentinel_out(robot, names=("zmp",)))
    assert np.array_equal(_bytes(only["zmp"]), _bytes(full["zmp"]))
    offs = di.OFFS.copy()
    offs[-1] -= 7                                  # the last clip ends seven rows early
    out = sentinel_out(robot)
    got = run(robot, q, offs, v, a, out=out)
    for k in ("tau", "root_wrench", "com", "zmp", "qvel", "qacc"):
        assert bool((_bytes(got[k][-7:]) == FILL).all()) and np.array_equal(_bytes(got[k][:-7]), _bytes(full[k][:-7])), k
    with pytest.raises(Exception, match="tau and root_wrench"):
        run(robot, q, di.OFFS, v, a, out=sentinel_out(robot, names=("tau", "tau_rms")))


def test_bad_arguments_are_refused_with_their_code():
    from gmr_amd import _native
    robot = "booster_k1"
    eng = engine(robot)
    keep = [_dev(di.quantised(robot)), _dev(di.OFFS)]
    table = eng.inertial_device(R.model(robot)[1])
    out = sentinel_out(robot)

    def call(**kw):
        st = _native.DynamicsInput()
        st.qpos, st.n_frames, st.seq_offsets, st.n_seq = keep[0].data_ptr(), di.N, keep[1].data_ptr(), di.S
        st.nbody, st.fps, st.gravity_z, st.fz_min = eng.nbody, di.FPS, -9.81, 0.05
        for k in _native.DYNAMICS_TABLE:
            setattr(st, k, table[k].data_ptr())
        for k, t in out.items():
            setattr(st, k + "_out", t.data_ptr())
        for k, val in kw.items():
            setattr(st, k, val)
        rc = eng._lib.gmr_motion_dynamics(eng._h, C.byref(st))
        return rc, eng._lib.gmr_last_error(eng._h)

    EINVAL, EUNSUPPORTED = -1, -3
    for kw, code, word in (({"fps": 0.0}, EINVAL, b"fps"), ({"fps": float("nan")}, EINVAL, b"fps"), ({"gravity_z": 0.0}, EINVAL, b"zero"),
                           ({"gravity_x": float("inf")}, EINVAL, b"finite"), ({"fz_min": -0.1}, EINVAL, b"fz_min"),
                           ({"n_frames": -1}, EINVAL, b"negative"), ({"body_mass": None}, EINVAL, b"null"),
                           ({"armature": None}, EINVAL, b"null"), ({"torque_limit": None}, EINVAL, b"null"),   # (NULL only without a hinge)
                           ({"tau_out": None}, EINVAL, b"tau_out"), ({"nbody": eng.nbody - 1}, EUNSUPPORTED, b"bodies")):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k       # nothing was launched
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bytes(out["tau"].cpu().numpy()), _bytes(gpu(robot, "diff")["tau"]))


def test_a_planar_base_is_refused():
    from gmr_amd import GeneralMotionRetargeting, dataset
    from gmr_amd.engine import Engine, EngineError
    cm = compiled("smplx", "galaxea_r1pro")
    assert cm.robot.planar_base
    eng = Engine(cm, device=0)
    tab = R.model("galaxea_r1pro")[1]
    q = torch.zeros((4, eng.nq), dtype=F64, device=DEV())
    q[:, 3] = 1.0
    with pytest.raises(EngineError, match="not supported by the kernels.*planar"):
        eng.motion_dynamics(q, [0, 4], 30.0, table=tab)
    g = GeneralMotionRetargeting("smplx", "galaxea_r1pro", verbose=False)
    with pytest.raises(NotImplementedError):
        dataset.dynamics_from_qpos(g, q, [0, 4], 30.0)
    with pytest.raises(NotImplementedError):
        g.dynamics_report(q, [0, 4], 30.0)


# ------------------------------------------------------------------ 4: the Python layers
def test_dataset_functions_return_the_engines_answer_per_clip():
    from gmr_amd import GeneralMotionRetargeting, dataset
    robot = "unitree_g1"
    g = GeneralMotionRetargeting("smplx", robot, verbose=False)
    tab = R.model(robot)[1]
    q = _dev(di.quantised(robot))
    want = gpu(robot, "diff")
    clips = dataset.dynamics_from_qpos(g, q, di.OFFS, di.FPS, table=tab)
    assert len(clips) == di.S and [c["tau"].shape[0] for c in clips] == di.LENS
    for s, c in enumerate(clips):
        a, b = int(di.OFFS[s]), int(di.OFFS[s + 1])
        for k in ("tau", "root_wrench", "com", "zmp", "qvel", "qacc"):
            assert np.array_equal(_bytes(c[k]), _bytes(want[k][a:b])), k
        for k in STATS:
            assert np.array_equal(_bytes(c[k]), _bytes(want[k][s])), k
        assert c["joint_names"][0] == "left_hip_pitch_joint" and c["fps"] == di.FPS and np.array_equal(c["torque_limit"], tab.torque_limit)
    rep = dataset.dynamics_report(g, q, di.OFFS, di.FPS, table=tab)
    assert sorted(rep) == sorted(STATS + ("joint_names", "torque_limit"))
    for k in STATS:
        assert np.array_equal(_bytes(rep[k]), _bytes(want[k])), k
    smooth = dataset.dynamics_report(g, q, di.OFFS, di.FPS, lowpass_hz=6.0, table=tab)
    qs = dataset.smooth_qpos(g, q, di.OFFS, di.FPS, 6.0)
    direct = g._engine.motion_dynamics(qs, di.OFFS, di.FPS, table=tab)
    assert np.array_equal(_bytes(smooth["tau_abs_max"]), _bytes(direct["tau_abs_max"].cpu().numpy()))
    assert not np.array_equal(smooth["tau_abs_max"], rep["tau_abs_max"])


def test_the_default_table_is_the_robots_own_mjcf_and_a_group_loops_over_its_members(monkeypatch):
    """With the MJCF files at hand (GMR_ROOT) no table has to be passed: the engine reads its robot's own, once.  The multi-robot
    object answers per member with one call each, and ``retarget_clips(dynamics=True)`` appends the same report."""
    import os
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting
    monkeypatch.setenv("GMR_ROOT", os.path.join(R.ROOT, "tests", "golden", "gmr_root"))
    robots = ["unitree_g1", "booster_k1"]
    q = {r: _dev(di.quantised(r)) for r in robots}
    g = GeneralMotionRetargeting("smplx", "unitree_g1", verbose=False)
    assert g.model.xml_path and g.model.xml_path.endswith("g1_mocap_29dof.xml")
    rep = g.dynamics_report(q["unitree_g1"], di.OFFS, di.FPS)
    for k in STATS:
        assert np.array_equal(_bytes(rep[k]), _bytes(gpu("unitree_g1", "diff")[k])), k
    assert g._engine.inertial_device() is g._engine.inertial_device()          # uploaded once per engine
    mr = MultiRobotRetargeting("smplx", robots)
    reps = mr.dynamics_report(q, di.OFFS, di.FPS)
    assert sorted(reps) == sorted(robots)
    for r in robots:
        for k in STATS:
            assert np.array_equal(_bytes(reps[r][k]), _bytes(gpu(r, "diff")[k])), (r, k)
        assert len(reps[r]["joint_names"]) == reps[r]["tau_abs_max"].shape[1]
