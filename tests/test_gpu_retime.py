"""gmr_motion_retime_plan and gmr_motion_retime_apply on the GPU against the numpy restatement (tests/retime_reference.py; inputs:
tests/retime_inputs.py).

Everything is bit for bit -- need, ticks, cum, out_len, clip_stats, need_max, src_time and every column of every output row -- except
the root quaternion of the rows that go through the slerp (u != 0 and two different source quaternions), where acos / sin belong to
two libms: there the rotation between the two answers is at most compose_reference.SLERP_RAD, the project's slerp bound, the norm
is 1 within 4 eps and the sign is the same.  The velocity property is asserted on the GPU's output with the bound derived in
retime_reference.bound.  Nothing in a bound was measured on a kernel."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import compose_reference as CR  # noqa: E402
from tests import retime_inputs as ri  # noqa: E402
from tests import retime_reference as RR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.util import compiled  # noqa: E402

F64, I64, U8 = torch.float64, torch.int64, torch.uint8
EPS = RR.EPS
G1, K1 = "unitree_g1", "booster_k1"
PLAN_KEYS = ("need", "ticks", "cum", "out_len", "clip_stats", "need_max")
ALL_CASES = [(r, n) for r in ri.ROBOTS for n in ri.CASES if n != "striding" or r == G1]


def sentinel(shape, dtype=F64):
    t = torch.empty(shape, dtype=dtype, device=DEV())
    if t.numel():
        t.view(U8).fill_(ri.FILL)
    return t


def plan_out(n, s):
    return {"need": sentinel((n,)), "ticks": sentinel((n,), I64), "cum": sentinel((n,), I64), "out_len": sentinel((s,), I64),
            "clip_stats": sentinel((s, 4), I64), "need_max": sentinel((s,))}


def run(robot, c, out_offsets=None, n_out=None):
    """Both calls into pre-filled caller-owned outputs, as host arrays: (plan dict, qpos_out, src_time, out_offsets)."""
    eng = engine(robot)
    q = _dev(c.q)
    out = plan_out(c.q.shape[0], len(c.offs) - 1)
    plan = eng.motion_retime_plan(q, c.offs, c.fps, c.vmax, c.window, c.max_stretch, out=out)
    assert all(plan[k] is out[k] for k in PLAN_KEYS)
    p = {k: plan[k].cpu().numpy() for k in PLAN_KEYS}
    oo = np.concatenate([[0], np.cumsum(p["out_len"])]).astype(np.int64) if out_offsets is None else np.asarray(out_offsets, dtype=np.int64)
    m = int(oo[-1]) if n_out is None else n_out
    res = {"qpos": sentinel((m, eng.nq)), "src_time": sentinel((m,))}
    a, b, back = eng.motion_retime_apply(q, c.offs, plan, oo, out=res)
    assert a is res["qpos"] and b is res["src_time"] and np.array_equal(back, oo)
    return p, a.cpu().numpy(), b.cpu().numpy(), oo


@functools.lru_cache(maxsize=None)
def gpu(robot, name):
    """The GPU's answer to a named case: computed once, shared, read-only."""
    p, out, st, oo = run(robot, ri.case(robot, name))
    for a in list(p.values()) + [out, st, oo]:
        a.setflags(write=False)
    return p, out, st, oo


def compare_rows(got, st, ref, ref_st, slerped, what):
    """The comparison of an apply's outputs with the restatement's."""
    assert got.shape == ref.shape and np.array_equal(_bytes(st), _bytes(ref_st)), f"{what}: src_time differs"
    exact = np.ones(got.shape, bool)
    exact[slerped, 3:7] = False
    same = _bytes(got).reshape(got.shape + (8,)) == _bytes(ref).reshape(ref.shape + (8,))
    bad = np.argwhere(~np.all(same, axis=-1) & exact)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ from the restatement, first (row, column) {bad[:6].tolist()}"
    ang = float(CR.quat_angle(got[slerped, 3:7], ref[slerped, 3:7]).max()) if slerped.any() else 0.0
    norm = float(np.abs(np.linalg.norm(got[slerped, 3:7], axis=1) - 1.0).max()) if slerped.any() else 0.0
    print(f"{what}: {int(slerped.sum())} slerped rows of {got.shape[0]}, worst slerp angle to the restatement {ang:.2e} rad, | |q| - 1 | {norm:.1e}")
    assert ang <= CR.SLERP_RAD and norm <= 4 * EPS
    if slerped.any():
        assert np.all(np.sum(got[slerped, 3:7] * ref[slerped, 3:7], axis=1) > 0.0)          # and the same sign


def check(robot, name, got=None):
    """The comparison every case gets; returns (plan, qpos_out, src_time, out_offsets, case)."""
    c = ri.case(robot, name)
    p, out, st, oo = gpu(robot, name) if got is None else got
    rp, rout, rst, roo, sl = ri.reference(robot, name)
    for k in PLAN_KEYS:
        assert np.array_equal(_bytes(p[k]), _bytes(rp[k])), f"{robot} {name}: {k} differs at {np.argwhere(p[k] != rp[k])[:6].tolist()}"
    assert np.array_equal(oo, roo)
    compare_rows(out, st, rout, rst, sl, f"{robot} {name}")
    return p, out, st, oo, c


# ------------------------------------------------------------------ a .. g against the restatement
@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_a_limits_nothing_reaches_give_the_input_back(robot):
    p, out, st, oo, c = check(robot, "identity")
    assert engine(robot).nq == {G1: 36, K1: 29}[robot]
    assert p["out_len"].tolist() == ri.LENS and np.array_equal(_bytes(out), _bytes(c.q))
    assert np.all(p["ticks"][p["ticks"] != 0] == 1024) and np.array_equal(st, np.floor(st))


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_b_a_uniform_limit_without_a_window(robot):
    p, out, st, oo, c = check(robot, "uniform")
    if robot == G1:
        assert p["clip_stats"][list(ri.LONG), 0].tolist() == [51, 63, 59, 108]
    else:
        assert p["out_len"][ri.C130] == 130
    assert np.array_equal(_bytes(run(robot, c)[1]), _bytes(out))                            # two calls: identical bytes


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_c_per_column_limits_window_four(robot):
    p, out, st, oo, c = check(robot, "columns")
    if robot == G1:
        assert p["out_len"].tolist() == [0, 1, 3, 5, 7, 125, 127, 129, 251]
    assert np.abs(p["need_max"][list(ri.LONG)] - 2.0).max() <= 4 * EPS


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_d_the_widest_window_crosses_the_tile_edges_and_covers_the_short_clips(robot):
    p, out, st, oo, c = check(robot, "wide")
    assert c.window == 32 and np.array_equal(p["need"], gpu(robot, "uniform")[0]["need"])


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_e_a_cap_that_binds(robot):
    p, out, st, oo, c = check(robot, "cap")
    assert np.all(p["clip_stats"][list(ri.LONG), 1] > 0) and p["ticks"].max() == 1536


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_f_a_burst_on_the_tile_edge(robot):
    p, out, st, oo, c = check(robot, "burst")
    assert p["out_len"].tolist() == [171] and p["clip_stats"][0, :3].tolist() == [1, 0, 0] and int(np.argmax(p["ticks"])) == 63


def with_waves(value, f):
    old = os.environ.get("GMR_AMD_RETIME_WAVES")
    try:
        os.environ["GMR_AMD_RETIME_WAVES"] = value
        return f()
    finally:
        os.environ.pop("GMR_AMD_RETIME_WAVES", None)
        if old is not None:
            os.environ["GMR_AMD_RETIME_WAVES"] = old


def test_g_one_wavefront_per_clip_strides_over_the_long_clip():
    c = ri.case(G1, "striding")
    got = with_waves("1", lambda: run(G1, c))
    p, out, st, oo, _ = check(G1, "striding", got)
    assert p["out_len"][ri.STRIDING_CLIPS // 2] > 1000
    check(G1, "striding")                                                                   # and the grid rule's own choice
    assert np.array_equal(_bytes(gpu(G1, "striding")[1]), _bytes(out))


def test_the_result_does_not_depend_on_the_wavefronts_per_clip():
    for name in ("columns", "wide"):
        for waves in ("1", "2", "7"):
            p, out, st, oo = with_waves(waves, lambda: run(G1, ri.case(G1, name)))
            base = gpu(G1, name)
            assert all(np.array_equal(_bytes(p[k]), _bytes(base[0][k])) for k in PLAN_KEYS), (name, waves)
            assert np.array_equal(_bytes(out), _bytes(base[1])) and np.array_equal(_bytes(st), _bytes(base[2])), (name, waves)


# ------------------------------------------------------------------ the property, on the GPU's output
@pytest.mark.parametrize("robot,name", ALL_CASES)
def test_no_hinge_of_the_output_exceeds_its_limit_beyond_one_lerps_rounding(robot, name):
    c = ri.case(robot, name)
    p, out, _, oo = gpu(robot, name)
    b = RR.bound(c.fps, float(np.abs(c.q[:, 7:]).max()), float(c.vmax.min()), c.window, c.max_stretch)
    worst = 0.0
    for s, r in enumerate(RR.ratios(out, oo, c.fps, c.vmax)):
        if r.size and not p["clip_stats"][s, 1:3].any():
            worst = max(worst, float(r.max()))
    print(f"{robot} {name}: worst |dq| fps / vmax = 1 + {worst - 1.0:.2e}, b = {b:.2e}")
    assert worst <= 1.0 + b


# ------------------------------------------------------------------ other output offsets than out_len's
def test_fewer_rows_truncate_more_rows_repeat_the_last_row_and_rows_outside_every_clip_keep_their_bytes():
    robot = K1
    c = ri.case(robot, "columns")
    p0 = gpu(robot, "columns")[0]
    lens = p0["out_len"].copy()
    lens[ri.C63] -= 20                                                                      # truncated
    lens[ri.C64] += 70                                                                      # its last row, 70 times more: past a tile
    lens[1] += 3                                                                            # a one-frame clip: four copies
    oo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + 5                        # a gap in front ...
    n_out = int(oo[-1]) - 9                                                                 # ... and the last clip runs past the array
    p, out, st, _ = run(robot, c, oo, n_out)
    fill = np.frombuffer(bytes([ri.FILL]) * 8, dtype=np.float64)[0]
    ref, ref_st, sl = RR.apply(c.q, c.offs, p["ticks"], p["cum"], oo, n_out, fill=fill)
    assert np.all(_bytes(out[:5]) == ri.FILL) and np.all(_bytes(st[:5]) == ri.FILL)
    compare_rows(out, st, ref, ref_st, sl, "other offsets")
    a, b = int(oo[ri.C64]), int(oo[ri.C64 + 1])
    last = c.q[int(ri.OFFS[ri.C64 + 1]) - 1]
    assert np.array_equal(_bytes(out[b - 71:b]), _bytes(np.tile(last, (71, 1)))) and np.all(st[b - 71:b] == 63.0)
    assert np.array_equal(_bytes(out[int(oo[1]):int(oo[2])]), _bytes(np.tile(c.q[0], (4, 1))))


def test_wrong_ticks_and_cum_take_every_row_from_its_own_clip():
    """Garbage in the hand-over arrays -- a cum in no order, ticks of 2^62, so that |u| < 2^-20 -- and every output row still lies within
    1e-5 of a row of its own clip (the clips follow different trajectories: a row of another clip is tenths of a radian away).  That
    nothing outside the arrays is touched is tests/test_gpu_retime_guard_band.py's business."""
    robot = K1
    c = ri.case(robot, "columns")
    eng = engine(robot)
    oo = gpu(robot, "columns")[3]
    rng = np.random.default_rng(5)
    n = c.q.shape[0]
    bad = {"ticks": _dev(np.full(n, 2 ** 62, dtype=np.int64)), "cum": _dev(rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64))}
    res = {"qpos": sentinel((int(oo[-1]), eng.nq)), "src_time": sentinel((int(oo[-1]),))}
    eng.motion_retime_apply(_dev(c.q), c.offs, bad, oo, out=res)
    out, st = res["qpos"].cpu().numpy(), res["src_time"].cpu().numpy()
    for s in range(ri.S):
        a, b, o0, o1 = int(ri.OFFS[s]), int(ri.OFFS[s + 1]), int(oo[s]), int(oo[s + 1])
        if o1 > o0:
            d = np.abs(out[o0:o1, None, 7:] - c.q[None, a:b, 7:]).max(axis=2).min(axis=1)
            assert d.max() <= 1e-5, s
            assert np.all(st[o0:o1] > -1e-5) and np.all(st[o0:o1] <= b - a - 1)


# ------------------------------------------------------------------ no work, the refusals
def _structs(robot, c, q, out, oo, res):
    from gmr_amd import _native
    eng = engine(robot)
    offs, vmax = _dev(c.offs), _dev(c.vmax)
    ps = _native.RetimePlanInput()
    ps.qpos, ps.n_frames, ps.seq_offsets, ps.n_seq, ps.window = q.data_ptr(), int(q.shape[0]), offs.data_ptr(), len(c.offs) - 1, c.window
    ps.fps, ps.vmax, ps.max_stretch = c.fps, vmax.data_ptr(), c.max_stretch
    for k in PLAN_KEYS:
        setattr(ps, k, out[k].data_ptr())
    ood = _dev(oo)
    st = _native.RetimeApplyInput()
    st.qpos, st.n_frames, st.seq_offsets, st.n_seq = q.data_ptr(), int(q.shape[0]), offs.data_ptr(), len(c.offs) - 1
    st.ticks, st.cum, st.out_offsets, st.n_out_frames = out["ticks"].data_ptr(), out["cum"].data_ptr(), ood.data_ptr(), int(oo[-1])
    st.qpos_out, st.src_time = res["qpos"].data_ptr(), res["src_time"].data_ptr()
    ps.stream = st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    return eng, ps, st, (offs, vmax, ood)


def test_h_no_work_returns_without_a_launch_and_every_refusal_returns_its_code():
    robot = K1
    c = ri.case(robot, "columns")
    oo = gpu(robot, "columns")[3]
    eng = engine(robot)
    q, out = _dev(c.q), plan_out(c.q.shape[0], ri.S)
    res = {"qpos": sentinel((int(oo[-1]), eng.nq)), "src_time": sentinel((int(oo[-1]),))}
    plan_call = lambda e, s: e._lib.gmr_motion_retime_plan(e._h, C.byref(s))     # noqa: E731
    apply_call = lambda e, s: e._lib.gmr_motion_retime_apply(e._h, C.byref(s))   # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -3
    eng, ps, st, keep = _structs(robot, c, q, out, oo, res)
    assert plan_call(eng, ps) == 0 and apply_call(eng, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bytes(res["qpos"].cpu().numpy()), _bytes(gpu(robot, "columns")[1]))   # the structs by hand give the tests' answer
    for t in list(out.values()) + list(res.values()):
        t.view(U8).fill_(ri.FILL)
    null = lambda name: (lambda s: setattr(s, name, None))                       # noqa: E731
    put = lambda name, v: (lambda s: setattr(s, name, v))                        # noqa: E731
    plan_edits = [(null(k), "null") for k in ("qpos", "seq_offsets", "vmax") + PLAN_KEYS] \
        + [(put("n_frames", -1), "negative"), (put("n_seq", -1), "negative"), (put("window", -1), "window"), (put("window", 33), "window"),
           (put("max_stretch", 0.5), "max_stretch"), (put("max_stretch", 64.5), "max_stretch"), (put("max_stretch", float("nan")), "max_stretch"),
           (put("fps", 0.0), "fps"), (put("fps", float("inf")), "fps"), (put("fps", float("nan")), "fps"), (put("fps", -30.0), "fps")]
    for edit, text in plan_edits:
        eng, ps, st, keep = _structs(robot, c, q, out, oo, res)
        edit(ps)
        assert plan_call(eng, ps) == EINVAL and text in eng._lib.gmr_last_error(eng._h).decode(), text
    apply_edits = [(null(k), "null") for k in ("qpos", "seq_offsets", "ticks", "cum", "out_offsets", "qpos_out", "src_time")] \
        + [(put(k, -1), "negative") for k in ("n_frames", "n_seq", "n_out_frames")] + [(lambda s: setattr(s, "qpos_out", s.qpos), "must not be qpos")]
    for edit, text in apply_edits:
        eng, ps, st, keep = _structs(robot, c, q, out, oo, res)
        edit(st)
        assert apply_call(eng, st) == EINVAL and text in eng._lib.gmr_last_error(eng._h).decode(), text
    # no work: GMR_OK without a launch, NULL arrays and all
    eng, ps, st, keep = _structs(robot, c, q, out, oo, res)
    ps.n_seq = 0
    ps.qpos = ps.seq_offsets = ps.vmax = ps.need = ps.out_len = None
    assert plan_call(eng, ps) == 0
    for field in ("n_seq", "n_frames", "n_out_frames"):
        eng, ps, st, keep = _structs(robot, c, q, out, oo, res)
        setattr(st, field, 0)
        st.qpos = st.qpos_out = st.src_time = st.ticks = st.out_offsets = None
        assert apply_call(eng, st) == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(U8) == ri.FILL).all()) for t in list(out.values()) + list(res.values()))   # none of them wrote a byte
    assert bool(torch.equal(q.cpu(), torch.from_numpy(np.array(c.q))))
    # a call without frames still reports its clips: zeros
    empty = eng.motion_retime_plan(q[:0], [0, 0, 0], c.fps, c.vmax, c.window, c.max_stretch, out=plan_out(0, 2))
    assert empty["out_len"].tolist() == [0, 0] and not empty["clip_stats"].any().item() and empty["need_max"].tolist() == [0.0, 0.0]
    a, b, back = eng.motion_retime_apply(q[:0], [0, 0, 0], empty)                            # and through the Python layer's read-back
    assert tuple(a.shape) == (0, eng.nq) and tuple(b.shape) == (0,) and back.tolist() == [0, 0, 0]
    # a planar base: GMR_EUNSUPPORTED from the library, NotImplementedError from the engine
    from gmr_amd.engine import Engine
    planar = Engine(compiled("smplx", "galaxea_r1pro"), device=0)
    assert planar.cm.robot.planar_base
    eng, ps, st, keep = _structs(robot, c, q, out, oo, res)                                 # (refused before an array is looked at)
    for rc in (plan_call(planar, ps), apply_call(planar, st)):
        assert rc == EUNSUPPORTED and "planar base" in planar._lib.gmr_last_error(planar._h).decode()
    with pytest.raises(NotImplementedError):
        planar.motion_retime_plan(torch.zeros((4, planar.nq), dtype=F64, device=DEV()), [0, 4], 30.0, np.ones(planar.nq - 7), 4, 8.0)


# ------------------------------------------------------------------ the layers above
@functools.lru_cache(maxsize=None)
def retargeter(robot):
    from gmr_amd import GeneralMotionRetargeting
    return GeneralMotionRetargeting("smplx", robot, device=0, verbose=False)


def test_retime_to_limits_end_to_end():
    import gmr_amd
    from gmr_amd import dataset
    g = retargeter(K1)
    c = ri.case(K1, "uniform")
    limit = float(c.vmax[0])
    q = _dev(c.q)
    out, offs, info = dataset.retime_to_limits(g, q, ri.OFFS, ri.FPS, limit)
    assert gmr_amd.retime_to_limits is dataset.retime_to_limits
    p, rout, rst, roo, sl = RR.retime(c.q, c.offs, c.fps, c.vmax, dataset.RETIME_WINDOW, dataset.RETIME_MAX_STRETCH)
    assert np.array_equal(offs, roo) and offs.dtype == np.int64                             # seq_offsets_out is the prefix sum of out_len
    compare_rows(out.cpu().numpy(), info["src_time"].cpu().numpy(), rout, rst, sl, "retime_to_limits")
    assert np.array_equal(_bytes(info["need"].cpu().numpy()), _bytes(p["need"])) and np.array_equal(info["need_max"], p["need_max"])
    for k, col in (("stretched_intervals", 0), ("capped_intervals", 1), ("nonfinite_intervals", 2)):
        assert np.array_equal(info[k], p["clip_stats"][:, col])
    lens = np.diff(ri.OFFS)
    want = np.where(lens > 1, (np.diff(roo) - 1) / np.maximum(lens - 1, 1), 1.0)
    assert np.array_equal(info["stretch"], want) and info["stretch"].max() > 1.2 and info["stretch"].min() == 1.0
    # ordinary (qpos, seq_offsets): the tracking export and the clip report take it
    tracks = dataset.tracking_from_qpos(g, out, offs, ri.FPS, ri.FPS)
    assert len(tracks) == ri.S
    host = out.cpu().numpy()
    for s, tr in enumerate(tracks):
        a, b = int(offs[s]), int(offs[s + 1])
        assert np.asarray(tr["root_pos"]).shape == (b - a, 3) and np.all(np.isfinite(np.asarray(tr["joint_vel"])))
    rep = g._engine.clip_report(out, offs).numpy()
    bound = RR.bound(c.fps, float(np.abs(c.q[:, 7:]).max()), limit, dataset.RETIME_WINDOW, dataset.RETIME_MAX_STRETCH)
    step = np.asarray(rep.dof_step_max)
    assert step.shape == (ri.S, host.shape[1] - 7) and step.max() * ri.FPS / limit <= 1.0 + bound   # the report's own finding is gone
    assert np.asarray(g._engine.clip_report(q, ri.OFFS).numpy().dof_step_max).max() * ri.FPS / limit > 1.5
    # two rates in one call: one call pair per rate, the same clips
    fps = np.where(np.arange(ri.S) % 2 == 0, ri.FPS, 2.0 * ri.FPS)
    out2, offs2, info2 = dataset.retime_to_limits(g, q, ri.OFFS, fps, limit)
    for s in range(ri.S):
        a, b = int(ri.OFFS[s]), int(ri.OFFS[s + 1])
        one = RR.retime(c.q[a:b], np.array([0, b - a]), fps[s], c.vmax, dataset.RETIME_WINDOW, dataset.RETIME_MAX_STRETCH)
        assert int(offs2[s + 1] - offs2[s]) == int(one[3][-1])
        compare_rows(out2[int(offs2[s]):int(offs2[s + 1])].cpu().numpy(), info2["src_time"][int(offs2[s]):int(offs2[s + 1])].cpu().numpy(),
                     one[1], one[2], one[4], f"two rates, clip {s}")
    # None: the default table on every limited hinge
    out3, offs3, info3 = dataset.retime_to_limits(g, q, ri.OFFS, ri.FPS)
    ref3 = RR.retime(c.q, c.offs, c.fps, dataset.retime_vmax(g.model), dataset.RETIME_WINDOW, dataset.RETIME_MAX_STRETCH)
    assert np.array_equal(offs3, ref3[3])
