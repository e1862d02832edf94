"""gmr_motion_mirror on the GPU against the numpy definition (tests/mirror_reference.py; inputs: tests/mirror_inputs.py).

GMR_MIRROR_WORLD and the hinge columns of GMR_MIRROR_CLIP_START are copies and sign flips: bit for bit.  The root columns of
GMR_MIRROR_CLIP_START are allowed mirror_reference.bound: ten times the numpy reference's own worst distance to its 50-digit
evaluator on the same rows (FLOAT_WORST; tests/test_symmetry_host.py re-measures it), absolute, with no other factor.  Nothing in the
bound was measured on a kernel."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import mirror_inputs as mi  # noqa: E402
from tests import mirror_reference as MR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.util import compiled  # noqa: E402

F64, U8 = torch.float64, torch.uint8
SENTINEL = np.frombuffer(bytes([mi.FILL]) * 8, dtype=np.float64)[0]


def sentinel(shape):
    t = torch.empty(shape, dtype=F64, device=DEV())
    if t.numel():
        t.view(U8).fill_(mi.FILL)
    return t


def run(robot, q, offs, about, plan=None):
    """One call into a pre-filled caller-owned output, as a host array."""
    out = sentinel(q.shape)
    res = engine(robot).motion_mirror(_dev(q), offs, plan=mi.plan(robot) if plan is None else plan, about=about, out=out)
    assert res is out
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def gpu(robot, about):
    """The GPU's answer on the shared inputs: computed once, shared, read-only."""
    a = run(robot, mi.qpos(robot), mi.OFFS, about)
    a.setflags(write=False)
    return a


def root_errors(got, ref):
    with np.errstate(all="ignore"):
        return float(np.abs(got[:, :3] - ref[:, :3]).max()), float(np.abs(got[:, 3:7] - ref[:, 3:7]).max())


# ------------------------------------------------------------------ 1: the two modes against the definition
@pytest.mark.parametrize("robot", mi.ROBOTS)
def test_world_mode_equals_the_definition_bit_for_bit_and_is_an_involution(robot):
    got, ref = gpu(robot, "world"), mi.reference(robot, "world")
    assert engine(robot).nq == {"unitree_g1": 36, "booster_k1": 29, "unitree_g1_with_hands": 50}[robot]
    assert np.array_equal(_bytes(got), _bytes(ref))
    assert not np.array_equal(got[:, 7:], mi.qpos(robot)[:, 7:])                           # (it is not the identity)
    back = run(robot, got, mi.OFFS, "world")
    assert np.array_equal(_bytes(back), _bytes(mi.qpos(robot)))                            # mirror(mirror(q)): the input bytes
    assert np.array_equal(_bytes(run(robot, mi.qpos(robot), mi.OFFS, "world")), _bytes(got))   # two calls: identical bytes


@pytest.mark.parametrize("robot", mi.ROBOTS)
def test_clip_start_mode_hinges_bit_for_bit_and_the_root_within_the_bound(robot):
    got, ref, q = gpu(robot, "start"), mi.reference(robot, "start"), mi.qpos(robot)
    assert np.array_equal(_bytes(got[:, 7:]), _bytes(ref[:, 7:]))
    assert np.array_equal(_bytes(got[:, 7:]), _bytes(gpu(robot, "world")[:, 7:]))
    assert np.array_equal(_bytes(got[:, 2]), _bytes(q[:, 2]))                              # z is a copy
    e_pos, e_quat = root_errors(got, ref)
    print(f"{robot}: worst |GPU - numpy| on the root: position {e_pos:.2e} m ({e_pos / MR.bound(robot, 'pos'):.2f} of its bound), "
          f"quaternion {e_quat:.2e} ({e_quat / MR.bound(robot, 'quat'):.2f} of its bound)")
    assert e_pos <= MR.bound(robot, "pos") and e_quat <= MR.bound(robot, "quat")
    assert np.abs(got[:, :2] - gpu(robot, "world")[:, :2]).max() > 0.1                     # (the two modes differ where they should)
    assert np.array_equal(_bytes(run(robot, q, mi.OFFS, "start")), _bytes(got))            # two calls: identical bytes
    n0, n1 = np.sqrt(np.sum(q[:, 3:7] ** 2, axis=1)), np.sqrt(np.sum(got[:, 3:7] ** 2, axis=1))
    assert np.abs(n1 - n0).max() <= 1e-15                           # the norm carries over; nothing is normalised


@pytest.mark.parametrize("robot", mi.ROBOTS)
def test_a_mirrored_clip_starts_where_the_original_does_facing_the_same_way(robot):
    got, q = gpu(robot, "start"), mi.qpos(robot)
    first = [int(mi.OFFS[s]) for s, T in enumerate(mi.LENS) if T]
    assert len(first) == 8
    assert np.abs(got[first, :3] - q[first, :3]).max() <= MR.bound(robot, "pos")
    h0, h1 = MR.heading(q[first, 3:7]), MR.heading(got[first, 3:7])                        # (cos psi, sin psi, ...) of the two first rows
    assert max(np.abs(h0[0] - h1[0]).max(), np.abs(h0[1] - h1[1]).max()) <= MR.bound(robot, "quat")


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_k1"])
def test_clip_start_then_world_is_one_rigid_motion_per_clip(robot):
    """W(S(q)): the hinges come back bit for bit, and the root is the input's moved by the rotation about z by -2 psi that takes p0
    to its mirror image (x, -y): p'' = D p0 + R_z(-2 psi) (p - p0), r'' = r_z(-2 psi) (x) r, with psi from the reference."""
    q = mi.qpos(robot)
    got = run(robot, np.array(gpu(robot, "start")), mi.OFFS, "world")
    assert np.array_equal(_bytes(got[:, 7:]), _bytes(q[:, 7:]))
    want = q.copy()
    for s, T in enumerate(mi.LENS):
        if not T:
            continue
        a, b = int(mi.OFFS[s]), int(mi.OFFS[s + 1])
        cp, sp, c2, s2 = (float(v) for v in MR.heading(q[a, 3:7]))
        dx, dy = q[a:b, 0] - q[a, 0], q[a:b, 1] - q[a, 1]
        want[a:b, 0] = q[a, 0] + (c2 * dx + s2 * dy)
        want[a:b, 1] = -q[a, 1] + (-s2 * dx + c2 * dy)
        w, x, y, z = (q[a:b, 3 + i] for i in range(4))
        want[a:b, 3:7] = np.stack([cp * w + sp * z, cp * x + sp * y, cp * y - sp * x, cp * z - sp * w], 1)   # (cp, 0, 0, -sp) (x) r
    e_pos, e_quat = root_errors(got, want)
    print(f"{robot}: worst distance to the rigid motion: position {e_pos:.2e} m, quaternion {e_quat:.2e}")
    assert e_pos <= MR.bound(robot, "pos") and e_quat <= MR.bound(robot, "quat")
    assert np.array_equal(_bytes(got), _bytes(MR.world_clips(mi.plan(robot), np.array(gpu(robot, "start")), mi.OFFS)))   # the second step is exact


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_k1"])
def test_a_vertical_first_row_takes_the_psi_zero_branch(robot):
    q, offs = mi.vertical(robot)
    got, ref = run(robot, q, offs, "start"), MR.clip_start(mi.plan(robot), q, offs)
    e_pos, e_quat = root_errors(got, ref)
    assert e_pos <= MR.bound(robot, "pos") and e_quat <= MR.bound(robot, "quat")
    # psi = 0: the reflection in the plane y = p0_y, and the quaternion map is the world mirror's exactly (1 * v + 0 * other)
    assert np.array_equal(got[:, 3:7], q[:, 3:7] * np.array([1.0, -1.0, 1.0, -1.0]))
    for a in (0, 5):
        assert np.abs(got[a:a + 5, 0] - q[a:a + 5, 0]).max() <= MR.bound(robot, "pos")
        assert np.abs(got[a:a + 5, 1] - (2.0 * q[a, 1] - q[a:a + 5, 1])).max() <= MR.bound(robot, "pos")
    assert np.array_equal(_bytes(got[:, 7:]), _bytes(ref[:, 7:]))


# ------------------------------------------------------------------ 2: what is written
@pytest.mark.parametrize("about", mi.MODES)
def test_rows_outside_every_clip_keep_the_sentinel_also_with_gaps_and_clamped_offsets(about):
    robot = "booster_k1"
    q, plan = mi.qpos(robot), mi.plan(robot)
    ref_of = MR.world_clips if about == "world" else MR.clip_start
    for offs in ([2, 5, 5, 40], [7, 70, 200, 200, 329], [-5, 3, mi.N + 7], [0, 0], [mi.N, mi.N]):
        offs = np.array(offs, np.int64)
        got, ref = run(robot, q, offs, about), ref_of(plan, q, offs, fill=SENTINEL)
        written = ~np.all(_bytes(ref).reshape(mi.N, -1) == mi.FILL, axis=1)
        assert np.array_equal(_bytes(got[~written]), _bytes(ref[~written])), offs            # the sentinel, byte for byte
        assert np.array_equal(_bytes(got[written][:, 7:]), _bytes(ref[written][:, 7:])), offs
        e_pos, e_quat = root_errors(got[written], ref[written]) if written.any() else (0.0, 0.0)
        assert e_pos <= MR.bound(robot, "pos") and e_quat <= MR.bound(robot, "quat"), offs
        if about == "world":
            assert np.array_equal(_bytes(got), _bytes(ref)), offs
    # without `out` the rows outside every clip hold a copy of the input
    res = engine(robot).motion_mirror(_dev(q), np.array([2, 5], np.int64), plan=plan, about=about).cpu().numpy()
    assert np.array_equal(_bytes(res[:2]), _bytes(q[:2])) and np.array_equal(_bytes(res[5:]), _bytes(q[5:])) and not np.array_equal(res[2:5], q[2:5])


@pytest.mark.parametrize("about", mi.MODES)
def test_the_result_does_not_depend_on_the_wavefronts_per_clip(about):
    robot = "unitree_g1"
    old = os.environ.get("GMR_AMD_MIRROR_WAVES")
    try:
        for waves in ("1", "2", "7"):
            os.environ["GMR_AMD_MIRROR_WAVES"] = waves
            assert np.array_equal(_bytes(run(robot, mi.qpos(robot), mi.OFFS, about)), _bytes(gpu(robot, about))), waves
    finally:
        os.environ.pop("GMR_AMD_MIRROR_WAVES", None)
        if old is not None:
            os.environ["GMR_AMD_MIRROR_WAVES"] = old


# ------------------------------------------------------------------ 3: the refusals
def _struct(robot, q, out, offs, mode=0):
    from gmr_amd import _native
    eng = engine(robot)
    tab = eng.symmetry_device(mi.plan(robot))
    st = _native.MirrorInput()
    st.qpos, st.n_frames, st.seq_offsets, st.n_seq = q.data_ptr(), int(q.shape[0]), offs.data_ptr(), int(offs.shape[0]) - 1
    st.mode, st.col_src, st.col_sign, st.qpos_out = mode, tab["col_src"].data_ptr(), tab["col_sign"].data_ptr(), out.data_ptr()
    st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    return eng, st


def test_every_refusal_returns_its_code_and_writes_nothing():
    robot = "booster_k1"
    q, offs, out = _dev(mi.qpos(robot)), _dev(mi.OFFS), sentinel((mi.N, engine(robot).nq))
    call = lambda eng, st: eng._lib.gmr_motion_mirror(eng._h, C.byref(st))   # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -3
    eng, st = _struct(robot, q, out, offs)
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    out.view(U8).fill_(mi.FILL)
    for edit, code, text in [(lambda s: setattr(s, "qpos", None), EINVAL, "null"), (lambda s: setattr(s, "qpos_out", None), EINVAL, "null"),
                             (lambda s: setattr(s, "seq_offsets", None), EINVAL, "null"), (lambda s: setattr(s, "col_src", None), EINVAL, "null"),
                             (lambda s: setattr(s, "col_sign", None), EINVAL, "null"), (lambda s: setattr(s, "n_frames", -1), EINVAL, "negative"),
                             (lambda s: setattr(s, "n_seq", -1), EINVAL, "negative"), (lambda s: setattr(s, "mode", 2), EINVAL, "unknown mode"),
                             (lambda s: setattr(s, "mode", -1), EINVAL, "unknown mode"),
                             (lambda s: setattr(s, "qpos_out", s.qpos), EINVAL, "must not be qpos")]:
        eng, st = _struct(robot, q, out, offs)
        edit(st)
        assert call(eng, st) == code and text in eng._lib.gmr_last_error(eng._h).decode(), text
    # no work: GMR_OK without a launch, NULL arrays and all
    for n_frames, n_seq in ((0, mi.S), (mi.N, 0)):
        eng, st = _struct(robot, q, out, offs)
        st.n_frames, st.n_seq, st.qpos, st.qpos_out, st.seq_offsets = n_frames, n_seq, None, None, None
        assert call(eng, st) == 0
    torch.cuda.synchronize()
    assert bool((out.view(U8) == mi.FILL).all())                                          # none of them wrote a byte
    assert bool(torch.equal(q.cpu(), torch.from_numpy(np.array(mi.qpos(robot)))))
    # the Python layer refuses the same, and a plan of another robot, before the library is called
    from gmr_amd.engine import EngineError
    from gmr_amd.symmetry import SymmetryError
    with pytest.raises(EngineError, match="must not be qpos"):
        eng.motion_mirror(q, offs, plan=mi.plan(robot), out=q)
    with pytest.raises(ValueError, match="about"):
        eng.motion_mirror(q, offs, plan=mi.plan(robot), about="sideways")
    with pytest.raises(SymmetryError):
        eng.motion_mirror(q, offs, plan=mi.plan("unitree_g1"))
    # a planar base: GMR_EUNSUPPORTED from the library, NotImplementedError from the plan
    from gmr_amd.engine import Engine
    planar = Engine(compiled("smplx", "galaxea_r1pro"), device=0)
    assert planar.cm.robot.planar_base
    qp = torch.zeros((4, planar.nq), dtype=F64, device=DEV())
    eng, st = _struct(robot, qp, torch.empty_like(qp), _dev(np.array([0, 4], np.int64)))
    assert planar._lib.gmr_motion_mirror(planar._h, C.byref(st)) == EUNSUPPORTED
    assert "planar base" in planar._lib.gmr_last_error(planar._h).decode()
    with pytest.raises(NotImplementedError):
        planar.motion_mirror(qp, [0, 4])


def test_the_default_plan_is_the_robots_own_and_is_cached():
    eng = engine("booster_k1")
    assert eng.symmetry_plan() is eng.symmetry_plan() and eng.symmetry_plan() == mi.plan("booster_k1")
    tab = eng.symmetry_device(eng.symmetry_plan())
    assert tab is eng.symmetry_device(eng.symmetry_plan()) and tab["col_src"].dtype == torch.int32 and tab["col_sign"].dtype == F64
    q = mi.qpos("booster_k1")
    got = eng.motion_mirror(_dev(q), mi.OFFS).cpu().numpy()                               # plan=None, about="world"
    assert np.array_equal(_bytes(got), _bytes(gpu("booster_k1", "world")))


# ------------------------------------------------------------------ 4: the FK identity on the device
def _qmul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


@pytest.mark.parametrize("robot", mi.ROBOTS)
def test_fk_of_the_mirrored_qpos_is_the_reflected_partner_permuted_fk(robot):
    """gmr_evaluate's poses of the mirrored qpos against the reflected poses of the original, body b against its partner.  The bound
    is plan.fk_bound + 2e-9 m: two evaluations at the 1e-9 the foot-lock test allows gmr_evaluate's xpos against numpy.  Orientations
    are compared as displacements from the rest pose, Q (x) Q0^-1, which do not depend on how a body's frame is drawn, sign-free."""
    eng, plan = engine(robot), mi.plan(robot)
    q = mi.qpos(robot)
    rest = np.zeros((1, eng.nq))
    rest[0, 3] = 1.0
    both = np.concatenate([q, gpu(robot, "world"), rest])
    _, xp, xq = eng.evaluate(_dev(both), want_errors=False, want_poses=True)
    xp, xq = xp.cpu().numpy(), xq.cpu().numpy()
    X, X2, Q, Q2, Q0 = xp[:mi.N], xp[mi.N:2 * mi.N], xq[:mi.N], xq[mi.N:2 * mi.N], xq[-1]
    ok = np.flatnonzero(plan.body_partner >= 0)
    part = plan.body_partner[ok]
    err = float(np.abs(X[:, ok] * np.array([1.0, -1.0, 1.0]) - X2[:, part]).max())
    bound = plan.fk_bound + 2e-9
    print(f"{robot}: worst |M X[b] - X'[partner b]| {err:.3e} m, bound {bound:.3e} m (fk_bound {plan.fk_bound:.3e})")
    assert err <= bound
    if robot == "booster_k1":
        assert plan.fk_bound <= 2e-12
    else:
        assert 1e-6 < err                                                                  # G1: the shoulders' 1e-5 m shows
    inv0 = Q0 * np.array([1.0, -1.0, -1.0, -1.0])
    D, D2 = _qmul(Q, inv0[None]), _qmul(Q2, inv0[None])
    want = D[:, ok] * np.array([1.0, -1.0, 1.0, -1.0])
    got = D2[:, part]
    sgn = np.sign(np.sum(want * got, axis=-1, keepdims=True))
    e_q = float(np.abs(sgn * got - want).max())
    print(f"{robot}: worst displacement-quaternion mismatch {e_q:.3e}")
    assert e_q <= eng.nbody * plan.residual_axis + 2e-9
