"""gmr_motion_compose on the GPU against the numpy restatement (tests/compose_reference.py; inputs: tests/compose_inputs.py).

Everything is bit for bit -- seg_transform, and every column of every output row -- except the root quaternion of blended rows, where
the slerp's acos / sin belong to two libms: there the rotation between the two answers is at most 1e-12 rad, the project's slerp
bound.  Nothing in a bound was measured on a kernel."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd.compose import ComposePlan, Segment  # noqa: E402
from tests import compose_inputs as ci  # noqa: E402
from tests import compose_reference as CR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.util import compiled  # noqa: E402

F64, U8 = torch.float64, torch.uint8
EPS = CR.EPS


def sentinel(shape):
    t = torch.empty(shape, dtype=F64, device=DEV())
    if t.numel():
        t.view(U8).fill_(ci.FILL)
    return t


def run(robot, q, plan):
    """One call into pre-filled caller-owned outputs, as host arrays: (qpos_out, seg_transform)."""
    eng = engine(robot)
    out, tr = sentinel((plan.n_out_frames, eng.nq)), sentinel((plan.n_seg, 6))
    a, b = eng.motion_compose(_dev(q), plan, out=out, transform_out=tr)
    assert a is out and b is tr
    return out.cpu().numpy(), tr.cpu().numpy()


@functools.lru_cache(maxsize=None)
def gpu(robot, name):
    """The GPU's answer to a named case: computed once, shared, read-only."""
    res = run(robot, *ci.case(robot, name))
    for a in res:
        a.setflags(write=False)
    return res


def check(robot, name):
    """The comparison every case gets; returns (got, transforms, plan, q)."""
    q, plan = ci.case(robot, name)
    (got, T), (ref, T_ref) = gpu(robot, name), ci.reference(robot, name)
    assert np.array_equal(_bytes(T), _bytes(T_ref)), f"{name}: seg_transform differs at segments {np.flatnonzero(np.any(T != T_ref, axis=1))[:8].tolist()}"
    bl = plan.blended_rows()
    exact = np.ones(got.shape, bool)
    exact[bl, 3:7] = False
    same = _bytes(got).reshape(got.shape + (8,)) == _bytes(ref).reshape(ref.shape + (8,))
    bad = np.argwhere(~np.all(same, axis=-1) & exact)
    assert bad.size == 0, f"{name}: {len(bad)} elements differ from the restatement, first (row, column) {bad[:6].tolist()}"
    ang = float(CR.quat_angle(got[bl, 3:7], ref[bl, 3:7]).max()) if bl.any() else 0.0
    norm = float(np.abs(np.linalg.norm(got[bl, 3:7], axis=1) - 1.0).max()) if bl.any() else 0.0
    print(f"{robot} {name}: {int(bl.sum())} blended rows of {got.shape[0]}, worst slerp angle to the restatement {ang:.2e} rad, | |q| - 1 | {norm:.1e}")
    assert ang <= CR.SLERP_RAD and norm <= 4 * EPS
    if bl.any():
        assert np.all(np.sum(got[bl, 3:7] * ref[bl, 3:7], axis=1) > 0.0)                    # and the same sign
    return got, T, plan, q


# ------------------------------------------------------------------ a .. g against the restatement
@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_a_whole_clips_come_back_as_their_bytes(robot):
    got, T, plan, q = check(robot, "whole")
    assert engine(robot).nq == {"unitree_g1": 36, "booster_k1": 29}[robot]
    assert np.array_equal(_bytes(got), _bytes(q)) and plan.n_seg == 8
    assert np.array_equal(T, np.tile(CR.IDENTITY, (8, 1)))


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_b_two_segments_blend_one(robot):
    got, T, plan, q = check(robot, "blend1")
    a = int(ci.OFFS[ci.C63])
    assert np.array_equal(_bytes(got[:62]), _bytes(q[a:a + 62]))                            # the first segment outside the overlap: copied
    assert plan.blended_rows().sum() == 2 and plan.n_out_frames == 63 + 64 - 1 + 1


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_c_blend_eight_across_the_tile_and_batch_edges(robot):
    got, T, plan, q = check(robot, "blend8")
    assert plan.seg_len.tolist() == [63, 64, 65, 130, 40, 60, 30] and plan.blended_rows().sum() == 5 * 8
    assert np.array_equal(_bytes(run(robot, q, plan)[0]), _bytes(got))                      # two calls: identical bytes


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_d_a_segment_that_is_all_overlap_and_a_blend_as_long_as_the_segment_before(robot):
    got, T, plan, q = check(robot, "overlap")
    assert plan.seg_blend[1] + plan.seg_blend[2] == plan.seg_len[1] and plan.seg_blend[4] == plan.seg_len[3] and plan.seg_blend[6] == plan.seg_len[6] == 64
    assert plan.blended_rows()[int(plan.out_offsets[1])]                                    # an output clip whose first row is a blend


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_e_a_turn_of_pi_headings_across_pi_and_a_vertical_root(robot):
    got, T, plan, q = check(robot, "edges")
    assert T[1].tolist()[:2] == [-1.0, 0.0] and abs(T[1, 4]) == 0.0 and abs(T[1, 5]) == 1.0   # the turn of pi: exact
    assert (T[:, 0] < 0.0).sum() >= 3                                                      # the c < 0 branch was taken
    # across +-pi the relative turn is 2e-3, not 2 pi - 2e-3: the segment keeps the heading of the one before it to 0.03
    c = T[2, 0] * T[3, 0] + T[2, 1] * T[3, 1]
    assert c > np.cos(0.03)
    # the vertical anchor row: psi = 0, so D's rotation is the previous anchor's heading itself
    ca, sa = (float(v) for v in CR.heading(q[60 + 20 - 4 + 2, 3:7]))
    cd, sd = T[3, 0] * T[4, 0] + T[3, 1] * T[4, 1], T[3, 0] * T[4, 1] - T[3, 1] * T[4, 0]
    assert abs(cd - ca) <= 8 * EPS and abs(sd - sa) <= 8 * EPS


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_f_a_negated_source_clip_gives_the_same_bytes_and_no_sign_jump(robot):
    got, T, plan, q = check(robot, "negated")
    assert np.all(np.sum(got[1:, 3:7] * got[:-1, 3:7], axis=1) > 0.0)                       # every consecutive pair, the anchor rows among them
    plain, T0 = run(robot, ci.qpos(robot), plan)
    assert np.array_equal(_bytes(got), _bytes(plain))                                      # (-h) (x) (-r) = h (x) r, bit for bit
    assert np.array_equal(T[1, 4:], -T0[1, 4:]) and np.array_equal(T[:, :4], T0[:, :4])


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_g_a_chain_of_130_segments_beside_an_empty_clip_and_a_one_frame_clip(robot):
    got, T, plan, q = check(robot, "long")
    assert plan.clip_segs.tolist() == [0, 130, 130, 131] and plan.out_offsets.tolist() == [0, 1173, 1173, 1174]
    assert np.array_equal(_bytes(got[-1]), _bytes(q[int(ci.OFFS[1])]))
    assert not np.array_equal(T[63], T[64]) and not np.array_equal(T[64], T[65])            # the carry past 64 lanes went somewhere


# ------------------------------------------------------------------ properties of the kernel's output alone
@pytest.mark.parametrize("name", ["blend8", "overlap", "edges", "long"])
@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_properties_of_the_output_alone(robot, name):
    q, plan = ci.case(robot, name)
    got, T = gpu(robot, name)
    bl = plan.blended_rows()
    L = float(max(np.abs(got[:, :2]).max(), np.abs(q[:, :2]).max()))
    for o in range(plan.n_out):
        for k in range(int(plan.clip_segs[o]), int(plan.clip_segs[o + 1])):
            B, nxt = int(plan.seg_blend[k]), int(plan.seg_blend[k + 1]) if k + 1 < int(plan.clip_segs[o + 1]) else 0
            n = int(plan.seg_len[k]) - nxt - B
            src, dst = q[int(plan.seg_src[k]) + B:][:n], got[int(plan.seg_out[k]) + B:][:n]
            assert not bl[int(plan.seg_out[k]) + B:][:n].any()
            assert np.array_equal(_bytes(dst[:, 2]), _bytes(src[:, 2])) and np.array_equal(_bytes(dst[:, 7:]), _bytes(src[:, 7:])), k   # z and hinges: copies
            if n > 1:                                                                       # a rigid map keeps the step lengths
                d0, d1 = np.linalg.norm(np.diff(src[:, :2], axis=0), axis=1), np.linalg.norm(np.diff(dst[:, :2], axis=0), axis=1)
                assert np.abs(d1 - d0).max() <= 8 * EPS * (1 + L), k
    assert np.abs(T[:, 0] ** 2 + T[:, 1] ** 2 - 1.0).max() <= 4 * EPS
    for k in range(plan.n_seg):                                                            # (hw, hz) is +- the half angle of (c, s), whose hw >= 0
        hw, hz = CR.half_angle(T[k, 0], T[k, 1])
        assert hw >= 0.0 and (T[k, 4:].tolist() == [hw, hz] or T[k, 4:].tolist() == [-hw, -hz]), k


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_a_clip_cut_into_overlapping_pieces_of_itself_composes_to_the_clip(robot):
    """Within four times the deviation the restatement shows on this input (compose_inputs.PIECES_D, measured on the CPU)."""
    got, T, plan, q = check(robot, "pieces")
    clip = q[int(ci.OFFS[ci.C130]):int(ci.OFFS[ci.C130 + 1])]
    d = float(np.abs(got - clip).max())
    print(f"{robot}: |composed - clip| {d:.3e}, the restatement's {ci.PIECES_D[robot]:.1e}")
    assert d <= 4.0 * ci.PIECES_D[robot]
    assert np.abs(T[:, 0] - 1.0).max() <= 4 * EPS and np.abs(T[:, 2:4]).max() <= 8 * EPS * (1 + np.abs(clip[:, :2]).max())


def test_the_result_does_not_depend_on_the_wavefronts_per_segment():
    robot = "unitree_g1"
    old = os.environ.get("GMR_AMD_COMPOSE_WAVES")
    try:
        for name in ("blend8", "overlap"):
            for waves in ("1", "2", "7"):
                os.environ["GMR_AMD_COMPOSE_WAVES"] = waves
                got = run(robot, *ci.case(robot, name))
                assert np.array_equal(_bytes(got[0]), _bytes(gpu(robot, name)[0])) and np.array_equal(_bytes(got[1]), _bytes(gpu(robot, name)[1])), (name, waves)
    finally:
        os.environ.pop("GMR_AMD_COMPOSE_WAVES", None)
        if old is not None:
            os.environ["GMR_AMD_COMPOSE_WAVES"] = old


def test_rows_no_segment_writes_keep_the_sentinel():
    """A plan whose tables leave a gap and point past the arrays: rows outside every segment keep their bytes, source rows are
    clamped, output rows outside the array are dropped."""
    robot = "booster_k1"
    q, plan = ci.case(robot, "blend8")
    eng = engine(robot)

    class Shifted:   # the same tables moved: 5 output rows down (a gap in front, the tail dropped), the last segment's source past the end
        n_seg, n_out, n_frames, n_out_frames = plan.n_seg, plan.n_out, plan.n_frames, plan.n_out_frames
        seg_src, seg_len, seg_blend, clip_segs = plan.seg_src.copy(), plan.seg_len, plan.seg_blend, plan.clip_segs
        seg_out = plan.seg_out + 5
        tables = ComposePlan.tables
        blended_rows = ComposePlan.blended_rows
    bad = Shifted()
    bad.seg_src[-1] = ci.N + 40
    out, tr = sentinel((plan.n_out_frames, eng.nq)), sentinel((plan.n_seg, 6))
    eng.motion_compose(_dev(q), bad, out=out, transform_out=tr)
    got = out.cpu().numpy()
    ref = CR.compose(bad, np.array(q), fill=np.frombuffer(bytes([ci.FILL]) * 8, dtype=np.float64)[0])[0]
    assert np.all(_bytes(got[:5]) == ci.FILL)
    bl = bad.blended_rows()[:got.shape[0]]
    exact = np.ones(got.shape, bool)
    exact[bl, 3:7] = False
    assert np.array_equal(_bytes(np.where(exact, got, 0.0)), _bytes(np.where(exact, ref, 0.0)))
    assert np.array_equal(_bytes(got[-17:, 7:]), _bytes(np.tile(q[-1, 7:], (17, 1))))        # the clamped source: the last row, over and over


# ------------------------------------------------------------------ h: no work, the refusals
def _struct(robot, q, plan, out, tr):
    from gmr_amd import _native
    eng = engine(robot)
    tab = eng.compose_device(plan)
    st = _native.ComposeInput()
    st.qpos, st.n_frames = q.data_ptr(), int(q.shape[0])
    for k, t in tab.items():
        setattr(st, k, t.data_ptr())
    st.n_seg, st.n_out, st.n_out_frames = plan.n_seg, plan.n_out, plan.n_out_frames
    st.qpos_out, st.seg_transform = out.data_ptr(), tr.data_ptr()
    st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    return eng, st


def test_h_no_work_returns_without_a_launch_and_every_refusal_returns_its_code():
    robot = "booster_k1"
    qh, plan = ci.case(robot, "blend8")
    q, out, tr = _dev(qh), sentinel((plan.n_out_frames, engine(robot).nq)), sentinel((plan.n_seg, 6))
    call = lambda eng, st: eng._lib.gmr_motion_compose(eng._h, C.byref(st))   # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -3
    eng, st = _struct(robot, q, plan, out, tr)
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    out.view(U8).fill_(ci.FILL)
    tr.view(U8).fill_(ci.FILL)
    null = lambda name: (lambda s: setattr(s, name, None))                     # noqa: E731
    neg = lambda name: (lambda s: setattr(s, name, -1))                        # noqa: E731
    for edit, code, text in [(null(k), EINVAL, "null") for k in ("qpos", "qpos_out", "seg_transform", "seg_src", "seg_len", "seg_blend", "seg_out", "clip_segs")] \
            + [(neg(k), EINVAL, "negative") for k in ("n_frames", "n_seg", "n_out", "n_out_frames")] \
            + [(lambda s: setattr(s, "n_frames", 0), EINVAL, "without frames"), (lambda s: setattr(s, "qpos_out", s.qpos), EINVAL, "must not be qpos")]:
        eng, st = _struct(robot, q, plan, out, tr)
        edit(st)
        assert call(eng, st) == code and text in eng._lib.gmr_last_error(eng._h).decode(), text
    # no work: GMR_OK without a launch, NULL arrays and all
    for field in ("n_seg", "n_out", "n_out_frames"):
        eng, st = _struct(robot, q, plan, out, tr)
        setattr(st, field, 0)
        st.qpos = st.qpos_out = st.seg_transform = st.seg_src = st.clip_segs = None
        assert call(eng, st) == 0
    empty = ComposePlan(ci.OFFS, [[], []], 8)                                               # and through the Python layer
    a, b = eng.motion_compose(q, empty)
    assert tuple(a.shape) == (0, eng.nq) and tuple(b.shape) == (0, 6)
    torch.cuda.synchronize()
    assert bool((out.view(U8) == ci.FILL).all()) and bool((tr.view(U8) == ci.FILL).all())   # none of them wrote a byte
    assert bool(torch.equal(q.cpu(), torch.from_numpy(np.array(qh))))
    # the Python layer refuses the same before the library is called
    from gmr_amd.engine import EngineError
    with pytest.raises(EngineError, match="source rows"):
        eng.motion_compose(q[:-1], plan)
    with pytest.raises(EngineError, match="transform_out"):
        eng.motion_compose(q, plan, transform_out=torch.empty((plan.n_seg, 5), dtype=F64, device=DEV()))
    same = ComposePlan(ci.OFFS, [[Segment(s, 0, n)] for s, n in enumerate(ci.LENS) if n])
    with pytest.raises(EngineError, match="must not be qpos"):
        eng.motion_compose(q, same, out=q)
    # a planar base: GMR_EUNSUPPORTED from the library, NotImplementedError from the engine
    from gmr_amd.engine import Engine
    planar = Engine(compiled("smplx", "galaxea_r1pro"), device=0)
    assert planar.cm.robot.planar_base
    qp = torch.zeros((ci.N, planar.nq), dtype=F64, device=DEV())
    _, st = _struct(robot, qp, plan, torch.empty((plan.n_out_frames, planar.nq), dtype=F64, device=DEV()), tr)
    assert planar._lib.gmr_motion_compose(planar._h, C.byref(st)) == EUNSUPPORTED
    assert "planar base" in planar._lib.gmr_last_error(planar._h).decode()
    with pytest.raises(NotImplementedError):
        planar.motion_compose(qp, plan)


def test_the_plans_tables_are_uploaded_once_and_a_side_stream_gives_the_same_bytes():
    robot = "unitree_g1"
    q, plan = ci.case(robot, "blend8")
    eng = engine(robot)
    tab = eng.compose_device(plan)
    assert tab is eng.compose_device(plan) and sorted(tab) == ["clip_segs", "seg_blend", "seg_len", "seg_out", "seg_src"]
    assert tab["seg_len"].dtype == tab["seg_blend"].dtype == torch.int32 and tab["seg_src"].dtype == tab["seg_out"].dtype == tab["clip_segs"].dtype == torch.int64
    side = torch.cuda.Stream(DEV())
    qd = _dev(q)
    torch.cuda.synchronize()
    out, tr = eng.motion_compose(qd, plan, stream=side)
    side.synchronize()
    assert np.array_equal(_bytes(out.cpu().numpy()), _bytes(gpu(robot, "blend8")[0])) and np.array_equal(_bytes(tr.cpu().numpy()), _bytes(gpu(robot, "blend8")[1]))
