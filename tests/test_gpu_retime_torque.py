"""gmr_motion_retime_plan_torque and the cubic resampling of gmr_motion_retime_apply on the GPU against the numpy restatement
(tests/retime_torque_reference.py; inputs: tests/retime_torque_inputs.py).

  plan    static_over bit for bit; need within 1 ulp (a quotient and a square root per row: whether this build rounds them correctly
          is printed, and recorded in DESIGN 4.20); ticks, cum, out_len, clip_stats and need_max bit for bit against the restatement
          evaluated on the GPU's own need -- everything behind need is the velocity plan's kernels and integers.
  apply   src_time, root position and hinges bit for bit; the root quaternion within 2 eps per component (a square root and four
          quotients behind bit-for-bit sums), and whether it was in fact bit for bit is printed.
  loop    dataset.retime_to_torque_limits on the four G1 clips of tests/test_retime_torque_host.py and a quiet one: converged within
          four passes -- the condition the host test establishes on the CPU.  Lengths are not compared with the CPU's: the GPU's
          torques differ from numpy's by 1e-13 and a ceil may flip.

Nothing in a bound was measured on a kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import retime_inputs as ri  # noqa: E402
from tests import retime_reference as RR  # noqa: E402
from tests import retime_torque_inputs as ti  # noqa: E402
from tests import retime_torque_reference as TR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402

F64, I64, I32, U8 = torch.float64, torch.int64, torch.int32, torch.uint8
EPS = RR.EPS
KEYS = ("need", "ticks", "cum", "out_len", "clip_stats", "need_max", "static_over")
TAIL = ("ticks", "cum", "out_len", "clip_stats", "need_max")
G1, K1 = "unitree_g1", "booster_k1"
EINVAL, EUNSUPPORTED = -1, -3


def sentinel(shape, dtype=F64):
    t = torch.empty(shape, dtype=dtype, device=DEV())
    if t.numel():
        t.view(U8).fill_(ti.FILL)
    return t


def plan_out(n, s):
    return {"need": sentinel((n,)), "ticks": sentinel((n,), I64), "cum": sentinel((n,), I64), "out_len": sentinel((s,), I64),
            "clip_stats": sentinel((s, 4), I64), "need_max": sentinel((s,)), "static_over": sentinel((n,), I32)}


def run_plan(model, c, offs=None, rows=None):
    """The call into pre-filled caller-owned outputs, as host arrays."""
    eng = engine(model)
    offs = c.offs if offs is None else offs
    n = c.tau.shape[0] if rows is None else rows
    out = plan_out(n, len(offs) - 1)
    tau, g = np.zeros((n, c.tau.shape[1])), np.zeros((n, c.tau.shape[1]))
    tau[:c.tau.shape[0]], g[:c.tau.shape[0]] = c.tau, c.tau_static
    fl = None
    if c.floor is not None:
        fl = np.zeros(n)
        fl[:c.floor.size] = c.floor
    plan = eng.motion_retime_plan_torque(_dev(tau), _dev(g), offs, c.limit, c.scale, c.window, c.max_stretch,
                                         None if fl is None else _dev(fl), c.align, out=out)
    assert all(plan[k] is out[k] for k in KEYS)
    return {k: plan[k].cpu().numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def gpu_plan(model, layout, floor, align):
    p = run_plan(model, ti.case(model, layout, floor, align))
    for a in p.values():
        a.setflags(write=False)
    return p


def ulps(a, b):
    """The largest distance in units of the last place between two arrays whose NaN patterns are the same bits."""
    ia, ib = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)) and np.array_equal(ia[nan], ib[nan])
    return int(np.abs(ia[~nan] - ib[~nan]).max()) if (~nan).any() else 0


def check_plan(p, ref, c, offs, what):
    assert np.array_equal(_bytes(p["static_over"]), _bytes(ref["static_over"])), f"{what}: static_over differs"
    d = ulps(p["need"], ref["need"])
    print(f"{what}: need differs from the restatement by at most {d} ulp ({'bit for bit' if d == 0 else 'NOT bit for bit'})")
    assert d <= 1
    tail = TR.plan_tail(p["need"], offs, c.window, c.max_stretch, c.align)
    for k in TAIL:
        assert np.array_equal(_bytes(p[k]), _bytes(tail[k])), f"{what}: {k} differs at {np.argwhere(p[k] != tail[k])[:6].tolist()}"
    return d


# ------------------------------------------------------------------ the plan against the restatement
@pytest.mark.parametrize("floor,align", ti.VARIANTS)
@pytest.mark.parametrize("layout", sorted(ti.LAYOUTS))
@pytest.mark.parametrize("model", list(ti.MODELS))
def test_plan_equals_the_restatement(model, layout, floor, align):
    c = ti.case(model, layout, floor, align)
    assert engine(model).nq - 7 == ti.MODELS[model]
    p = gpu_plan(model, layout, floor, align)
    check_plan(p, ti.reference(model, layout, floor, align), c, c.offs, f"{model} {layout} floor={floor} align={align}")
    if align:
        assert np.all(p["clip_stats"][:, 3] % 1024 == 0) and np.array_equal(p["out_len"], np.where(np.diff(c.offs) > 0, p["clip_stats"][:, 3] // 1024 + 1, 0))
    if ti.MODELS[model] >= 29 and layout == "lens":
        assert p["clip_stats"][:, 0].sum() > 50 and p["clip_stats"][:, 1].sum() > 0 and p["static_over"].max() >= 1


def test_two_calls_give_identical_bytes_and_the_wavefronts_per_clip_do_not_matter():
    from tests.test_gpu_retime import with_waves
    for model in (G1, "unitree_g1_with_hands"):
        c = ti.case(model, "lens", True, True)
        base = gpu_plan(model, "lens", True, True)
        for waves in (None, "1", "2", "7"):
            p = run_plan(model, c) if waves is None else with_waves(waves, lambda: run_plan(model, c))
            assert all(np.array_equal(_bytes(p[k]), _bytes(base[k])) for k in KEYS), (model, waves)


def test_rows_outside_every_clip_are_untouched():
    c = ti.case(G1, "ragged", True, True)
    offs = c.offs + 5                                                                       # a gap in front ...
    offs[-1] -= 3                                                                           # ... the last clip three rows shorter ...
    n = int(c.offs[-1]) + 9                                                                 # ... and rows behind it
    p = run_plan(G1, c, offs, n)
    tau, g, fl = np.zeros((n, 29)), np.zeros((n, 29)), np.zeros(n)
    tau[:310], g[:310], fl[:310] = c.tau, c.tau_static, c.floor
    ref = TR.plan(tau, g, offs, c.limit, c.scale, c.window, c.max_stretch, fl, True)
    inside = np.zeros(n, bool)
    inside[int(offs[0]):int(offs[-1])] = True
    for k in ("need", "ticks", "cum", "static_over"):
        assert np.all(_bytes(p[k][~inside]) == ti.FILL), k
        p[k][~inside] = 0                                                                    # (the restatement holds 0 there)
    check_plan(p, ref, c, offs, "shifted offsets")
    clamped = run_plan(G1, c, np.array([-4, 37, 37, 38, 101, 400]), None)                    # offsets outside [0, N] are clamped into it
    assert all(np.array_equal(_bytes(clamped[k]), _bytes(gpu_plan(G1, "ragged", True, True)[k])) for k in KEYS)


# ------------------------------------------------------------------ the cubic resampling
def run_apply(robot, c, plan, oo, n_out=None, interp="cubic"):
    eng = engine(robot)
    m = int(oo[-1]) if n_out is None else n_out
    res = {"qpos": sentinel((m, eng.nq)), "src_time": sentinel((m,))}
    eng.motion_retime_apply(_dev(c.q), c.offs, {"ticks": _dev(plan["ticks"]), "cum": _dev(plan["cum"])}, oo, out=res, interp=interp)
    return res["qpos"].cpu().numpy(), res["src_time"].cpu().numpy()


def compare_cubic(got, st, ref, ref_st, what):
    assert got.shape == ref.shape and np.array_equal(_bytes(st), _bytes(ref_st)), f"{what}: src_time differs"
    same = np.all(_bytes(got).reshape(got.shape + (8,)) == _bytes(ref).reshape(ref.shape + (8,)), axis=-1)
    quat = np.zeros(got.shape[1], bool)
    quat[3:7] = True
    bad = np.argwhere(~same[:, ~quat])
    assert bad.size == 0, f"{what}: {len(bad)} elements outside the quaternion differ from the restatement, first {bad[:6].tolist()}"
    fin = np.isfinite(ref[:, 3:7])
    assert np.array_equal(fin, np.isfinite(got[:, 3:7]))
    worst = float(np.abs(np.where(fin, got[:, 3:7] - ref[:, 3:7], 0.0)).max()) if fin.any() else 0.0
    exact = bool(same[:, quat].all())
    print(f"{what}: quaternion {'bit for bit' if exact else 'NOT bit for bit'}, worst component difference {worst / EPS:.2f} eps")
    assert worst <= 2 * EPS
    return exact


@pytest.mark.parametrize("name", ["uniform", "columns", "wide", "burst", "cap"])
@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_cubic_apply_equals_the_restatement(robot, name):
    c = ri.case(robot, name)
    p, _, _, oo, _ = ri.reference(robot, name)                                               # the velocity plan of the existing cases
    out, st = run_apply(robot, c, p, oo)
    ref, ref_st, curved = TR.apply_cubic(c.q, c.offs, p["ticks"], p["cum"], oo, int(oo[-1]))
    compare_cubic(out, st, ref, ref_st, f"{robot} {name}")
    assert curved.any() and np.array_equal(_bytes(out[~curved]), _bytes(ref[~curved]))        # the copies: all columns
    again = run_apply(robot, c, p, oo)[0]
    assert np.array_equal(_bytes(again), _bytes(out))                                        # two calls: identical bytes


def test_cubic_other_offsets_truncate_repeat_and_leave_the_rest():
    robot = K1
    c = ri.case(robot, "columns")
    p = ri.reference(robot, "columns")[0]
    lens = p["out_len"].copy()
    lens[ri.C63] -= 20
    lens[ri.C64] += 70
    lens[1] += 3
    oo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + 5
    n_out = int(oo[-1]) - 9
    out, st = run_apply(robot, c, p, oo, n_out)
    fill = np.frombuffer(bytes([ti.FILL]) * 8, dtype=np.float64)[0]
    ref, ref_st, _ = TR.apply_cubic(c.q, c.offs, p["ticks"], p["cum"], oo, n_out, fill=fill)
    assert np.all(_bytes(out[:5]) == ti.FILL) and np.all(_bytes(st[:5]) == ti.FILL)
    compare_cubic(out, st, ref, ref_st, "other offsets")


@pytest.mark.parametrize("name", ["uniform", "columns", "wide", "burst", "cap"])
@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_linear_through_the_new_argument_is_the_existing_kernels_answer(robot, name):
    from tests.test_gpu_retime import compare_rows, gpu
    c = ri.case(robot, name)
    p, out0, st0, oo = gpu(robot, name)                                                      # the default path of the existing tests
    out, st = run_apply(robot, c, p, oo, interp="linear")
    assert np.array_equal(_bytes(out), _bytes(out0)) and np.array_equal(_bytes(st), _bytes(st0))
    rp, rout, rst, roo, sl = ri.reference(robot, name)
    compare_rows(out, st, rout, rst, sl, f"{robot} {name} interp=linear")


def test_wrong_ticks_and_cum_take_every_cubic_row_from_its_own_clip():
    robot = K1
    c = ri.case(robot, "columns")
    oo = ri.reference(robot, "columns")[3]
    rng = np.random.default_rng(5)
    n = c.q.shape[0]
    bad = {"ticks": np.full(n, 2 ** 62, dtype=np.int64), "cum": rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)}
    out, st = run_apply(robot, c, bad, oo)
    for s in range(ri.S):
        a, b, o0, o1 = int(ri.OFFS[s]), int(ri.OFFS[s + 1]), int(oo[s]), int(oo[s + 1])
        if o1 > o0:
            d = np.abs(out[o0:o1, None, 7:] - c.q[None, a:b, 7:]).max(axis=2).min(axis=1)
            assert d.max() <= 1e-5, s


# ------------------------------------------------------------------ no work, the refusals
def _struct(model, c, out):
    from gmr_amd import _native
    eng = engine(model)
    keep = [_dev(c.tau), _dev(c.tau_static), _dev(c.offs), _dev(c.limit), _dev(c.floor)]
    st = _native.RetimeTorqueInput()
    st.tau, st.tau_static, st.seq_offsets, st.torque_limit, st.need_floor = (t.data_ptr() for t in keep)
    st.n_frames, st.n_seq, st.window, st.limit_scale, st.max_stretch, st.align_end = c.tau.shape[0], len(c.offs) - 1, c.window, c.scale, c.max_stretch, 1
    for k in KEYS:
        setattr(st, k, out[k].data_ptr())
    st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    return eng, st, keep


def test_no_work_returns_without_a_launch_and_every_refusal_returns_its_code():
    from gmr_amd import _native
    c = ti.case(G1, "ragged", True, True)
    out = plan_out(310, 5)
    call = lambda e, s: e._lib.gmr_motion_retime_plan_torque(e._h, C.byref(s))   # noqa: E731
    eng, st, keep = _struct(G1, c, out)
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    base = gpu_plan(G1, "ragged", True, True)
    assert all(np.array_equal(_bytes(out[k].cpu().numpy()), _bytes(base[k])) for k in KEYS)   # the struct by hand gives the tests' answer
    st.static_over = None                                                                    # static_over may be NULL
    for t in out.values():
        t.view(U8).fill_(ti.FILL)
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    assert all(np.array_equal(_bytes(out[k].cpu().numpy()), _bytes(base[k])) for k in KEYS[:-1]) and bool((out["static_over"].view(U8) == ti.FILL).all())
    for t in out.values():
        t.view(U8).fill_(ti.FILL)
    null = lambda name: (lambda s: setattr(s, name, None))                       # noqa: E731
    put = lambda name, v: (lambda s: setattr(s, name, v))                        # noqa: E731
    edits = [(null(k), "null") for k in ("tau", "tau_static", "seq_offsets", "torque_limit") + KEYS[:-1]] \
        + [(put("n_frames", -1), "negative"), (put("n_seq", -1), "negative"), (put("window", -1), "window"), (put("window", 33), "window"),
           (put("max_stretch", 0.5), "max_stretch"), (put("max_stretch", 64.5), "max_stretch"), (put("max_stretch", float("nan")), "max_stretch"),
           (put("limit_scale", 0.0), "limit_scale"), (put("limit_scale", 1.0001), "limit_scale"), (put("limit_scale", float("nan")), "limit_scale"),
           (put("limit_scale", -0.5), "limit_scale"), (put("align_end", 2), "align_end"), (put("align_end", -1), "align_end")]
    for edit, text in edits:
        eng, st, keep = _struct(G1, c, out)
        edit(st)
        assert call(eng, st) == EINVAL and text in eng._lib.gmr_last_error(eng._h).decode(), text
    eng, st, keep = _struct(G1, c, out)                                                     # no work: GMR_OK without a launch, NULL arrays and all
    st.n_seq = 0
    st.tau = st.tau_static = st.seq_offsets = st.torque_limit = st.need = st.out_len = None
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(U8) == ti.FILL).all()) for t in out.values())                    # none of them wrote a byte
    # the apply's interp: anything but 0 and 1 is refused
    ai = _native.RetimeApplyInput()
    ai.interp = 2
    assert eng._lib.gmr_motion_retime_apply(eng._h, C.byref(ai)) == EINVAL and "interp" in eng._lib.gmr_last_error(eng._h).decode()
    # a call without frames still reports its clips: zeros
    empty = eng.motion_retime_plan_torque(torch.zeros((0, 29), dtype=F64, device=DEV()), torch.zeros((0, 29), dtype=F64, device=DEV()), [0, 0, 0],
                                          c.limit, 0.95, 12, 8.0, out=plan_out(0, 2))
    assert empty["out_len"].tolist() == [0, 0] and not empty["clip_stats"].any().item() and empty["need_max"].tolist() == [0.0, 0.0]
    # a planar base: GMR_EUNSUPPORTED before an array is looked at
    eng, st, keep = _struct(G1, c, out)
    from gmr_amd.engine import Engine
    from tests.util import compiled
    planar = Engine(compiled("smplx", "galaxea_r1pro"), device=0)
    assert call(planar, st) == EUNSUPPORTED and "planar base" in planar._lib.gmr_last_error(planar._h).decode()
    with pytest.raises(NotImplementedError):
        t = torch.zeros((4, planar.nq - 7), dtype=F64, device=DEV())
        planar.motion_retime_plan_torque(t, t, [0, 4], np.ones(planar.nq - 7), 0.95, 12, 8.0)


def test_a_row_of_more_than_64_columns_is_refused_before_any_array_is_read():
    """A chain of 64 bodies with a hinge on every one but the base has nq 70: GMR_EUNSUPPORTED from the plan and from the apply, linear
    and cubic, with pointers that would fault if they were read; nothing is written."""
    from gmr_amd import _native
    from gmr_amd.engine import Engine
    wide = Engine(ti.wide_model(), device=0)
    assert wide.nq == ti.WIDE_NQ == 70
    lib, stream = wide._lib, torch.cuda.current_stream(DEV()).cuda_stream
    guard = sentinel((64,))
    st = _native.RetimeTorqueInput()
    for k in ("tau", "tau_static", "seq_offsets", "torque_limit", "need_floor") + KEYS:
        setattr(st, k, 8)                                                                    # (not NULL, and not memory)
    st.out_len = st.clip_stats = st.need_max = guard.data_ptr()
    st.n_frames, st.n_seq, st.window, st.limit_scale, st.max_stretch, st.align_end, st.stream = 100, 1, 12, 0.95, 8.0, 1, stream
    assert lib.gmr_motion_retime_plan_torque(wide._h, C.byref(st)) == EUNSUPPORTED
    assert "a row of 70 columns does not fit one wavefront" in lib.gmr_last_error(wide._h).decode()
    for interp in (0, 1):
        ai = _native.RetimeApplyInput()
        for k in ("qpos", "seq_offsets", "ticks", "cum", "out_offsets", "src_time"):
            setattr(ai, k, 8)
        ai.qpos_out = 16
        ai.n_frames, ai.n_seq, ai.n_out_frames, ai.interp, ai.stream = 100, 1, 100, interp, stream
        assert lib.gmr_motion_retime_apply(wide._h, C.byref(ai)) == EUNSUPPORTED
        assert "does not fit one wavefront" in lib.gmr_last_error(wide._h).decode()
    torch.cuda.synchronize()
    assert bool((guard.view(U8) == ti.FILL).all())


# ------------------------------------------------------------------ the loop, end to end
def test_retime_to_torque_limits_end_to_end():
    import gmr_amd
    from gmr_amd import dataset
    from tests.test_gpu_retime import retargeter
    g = retargeter(G1)
    rob, tab, q, offs = ti.loop_clips(quiet=True)
    qd = _dev(q)
    out, oo, info = dataset.retime_to_torque_limits(g, qd, offs, ti.LOOP_FPS, table=tab)     # (the MJCF file's table: real limits)
    assert gmr_amd.retime_to_torque_limits is dataset.retime_to_torque_limits
    host, st = out.cpu().numpy(), info["src_time"].cpu().numpy()
    print("passes", info["passes"], "ratio before", np.round(info["tau_ratio_before"], 4), "after", np.round(info["tau_ratio_after"], 4),
          "rows", np.diff(oo), "stretched per pass", info["stretched_intervals"].tolist())
    assert info["converged"].all() and np.all(info["passes"] <= 4) and info["passes"].tolist()[4] == 0
    assert np.round(info["tau_ratio_before"][:4], 2).tolist() == [2.08, 1.70, 1.07, 1.40]
    assert not info["capped_intervals"].any() and not info["nonfinite_intervals"].any() and not info["static_over_frames"].any()
    rep = dataset.dynamics_report(g, out, oo, ti.LOOP_FPS, table=tab)
    ratio = np.asarray(rep["tau_ratio_max"]).max(axis=1)
    assert np.all(ratio <= 1.0) and np.array_equal(ratio, info["tau_ratio_after"])
    assert oo.dtype == np.int64 and np.all(np.diff(oo)[:4] > 120) and int(oo[-1]) == host.shape[0] == st.shape[0]
    a, b = int(oo[4]), int(oo[5])
    assert b - a == 40 and np.array_equal(_bytes(host[a:b]), _bytes(q[int(offs[4]):]))        # the quiet clip is bitwise its input
    for s in range(5):
        o0, o1, a0, a1 = int(oo[s]), int(oo[s + 1]), int(offs[s]), int(offs[s + 1])
        assert np.array_equal(_bytes(host[o0]), _bytes(q[a0])) and np.array_equal(_bytes(host[o1 - 1]), _bytes(q[a1 - 1]))
        assert st[o0] == 0.0 and st[o1 - 1] == a1 - a0 - 1 and np.all(np.diff(st[o0:o1]) >= 0.0)
    assert np.abs(np.linalg.norm(host[:, 3:7], axis=1) - 1.0).max() <= 4 * EPS
    # a velocity floor in the same warp: the torque side still converges, no clip gets shorter, and the worst hinge speed over 4 rad/s
    # comes down.  How far a cubic may carry a hinge over the limit the plan was made for is not bounded by the contract (the header
    # says so), so no such bound is asserted: the figure is printed.
    out2, oo2, info2 = dataset.retime_to_torque_limits(g, qd, offs, ti.LOOP_FPS, table=tab, velocity_limits=4.0)
    assert info2["converged"].all() and np.all(np.diff(oo2) >= np.diff(offs))
    vmax = dataset.retime_vmax(g.model, 4.0)
    before = max(float(r.max()) for r in RR.ratios(q, offs, ti.LOOP_FPS, vmax) if r.size)
    after = max(float(r.max()) for r in RR.ratios(out2.cpu().numpy(), oo2, ti.LOOP_FPS, vmax) if r.size)
    print(f"velocity floor at 4 rad/s: worst |dq| fps / vmax {before:.3f} going in, {after:.3f} coming out")
    assert before > 1.0 and after < before
    # ordinary (qpos, seq_offsets): the tracking export takes it
    tracks = dataset.tracking_from_qpos(g, out, oo, ti.LOOP_FPS, ti.LOOP_FPS)
    assert len(tracks) == 5 and all(np.all(np.isfinite(np.asarray(tr["joint_vel"]))) for tr in tracks)
