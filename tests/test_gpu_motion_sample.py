"""The motion library's random access (gmr_motion_sample, Engine.motion_sample, dataset.MotionLibrary) on the GPU, against the
contract in include/gmr_amd.h as tests/motion_sample_reference.py restates it.

One library per robot: clips of 1, 2, 3, 7, 0, 64 and 65 frames at 30, 120, 50, 30, 30, 32 and 128 fps, smooth random qpos, the
7-frame clip with its root quaternion negated from frame 4 on.  The query list holds, for every clip with frames, the times
before, at and beyond both ends, interior times and exact frame times, then random (id, time) pairs, shuffled: unsorted ids with
repeats.  Its first 1, 63, 64, 65 and 200 entries are the query sets (one lane, the edges of the 64-query wavefront, four
wavefronts)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import motion_sample_reference as ref  # noqa: E402
from tests.test_gpu_motion_track import _smooth_qpos  # noqa: E402
from tests.util import compiled  # noqa: E402

ROBOTS = ["unitree_g1", "stanford_toddy"]
LENS, FPS = [1, 2, 3, 7, 0, 64, 65], [30.0, 120.0, 50.0, 30.0, 30.0, 32.0, 128.0]
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
SIZES = [1, 63, 64, 65, 200]
GEN = ("root_pos", "root_rot", "joint_pos", "root_lin_vel", "root_ang_vel", "joint_vel")
BODY = ("body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")
_GMR, _CASES = {}, {}


def _gmr(robot):
    from gmr_amd import GeneralMotionRetargeting
    if robot not in _GMR:
        _GMR[robot] = GeneralMotionRetargeting("smplx", robot, device=0)
    return _GMR[robot]


def _queries(seed):
    rng = np.random.default_rng(seed)
    ids, ts = [], []
    for s, (T, f) in enumerate(zip(LENS, FPS)):
        if T == 0:
            continue
        last = (T - 1) / f
        edge = [-1.0, -1e-300, 0.0, last, np.nextafter(last, np.inf), last + 1.0, 0.25 / f, (T - 1 - 0.25) / f, (T // 2) / f]
        edge += list(rng.uniform(0.0, max(last, 1e-3), size=4))
        ids += [s] * len(edge)
        ts += edge
    n = 200 - len(ids)
    rid = rng.choice([s for s, T in enumerate(LENS) if T > 0], size=n)
    ids += list(rid)
    ts += [rng.uniform(-0.05, (LENS[s] - 1) / FPS[s] + 0.05) for s in rid]
    order = rng.permutation(len(ids))
    return np.asarray(ids, dtype=np.int64)[order], np.asarray(ts, dtype=np.float64)[order]


def _library_qpos(robot, seed):
    q = _smooth_qpos(robot, OFFS, seed=seed)
    a = int(OFFS[3])
    q[a + 4:a + 7, 3:7] *= -1.0  # the same rotations, the other sign: the slerp and both stencils cross the flip
    return q


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _case(robot):
    """Per robot, once: the library, the 200 queries, the float64 call on them, and the two restatements."""
    if robot not in _CASES:
        from gmr_amd.dataset import MotionLibrary
        g = _gmr(robot)
        q = _library_qpos(robot, 70 + ROBOTS.index(robot) if robot in ROBOTS else 79)
        lib = MotionLibrary(g, q, OFFS, FPS)
        ids, ts = _queries(7)
        got = _host(g._engine.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(ts)))
        tree = ref.Tree(compiled("smplx", robot).robot)
        want, plan = ref.sample(tree, q, OFFS, FPS, ids, ts)
        w32 = ref.chain(tree, want, np.float32)
        _CASES[robot] = dict(gmr=g, lib=lib, q=q, ids=ids, ts=ts, got=got, want=want, w32=w32, plan=plan, tree=tree)
    return _CASES[robot]


def _same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype for k in (keys or a.keys()))


# ------------------------------------------------------------------ 1: the definition
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_generalized_arrays_match_the_definition(robot, E):
    from scipy.spatial.transform import Rotation as R, Slerp
    c = _case(robot)
    eng, lib = c["gmr"]._engine, c["lib"]
    ids, ts = c["ids"][:E], c["ts"][:E]
    got = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(ts)))
    assert _same(got, {k: v[:E] for k, v in c["got"].items()})  # a query does not depend on the size of its call
    want = {k: v[:E] for k, v in c["want"].items()}
    assert all(got[k].dtype == np.float64 and got[k].shape == want[k].shape for k in GEN)
    assert all(got[k].dtype == np.float32 for k in BODY)
    for k in ("root_pos", "joint_pos", "root_lin_vel", "joint_vel"):
        assert np.array_equal(got[k], want[k]), k
    e_rot = np.abs(got["root_rot"] - want["root_rot"]).max()
    fq = np.asarray(FPS)[ids]
    e_w = np.abs(got["root_ang_vel"] - want["root_ang_vel"])
    frac = (e_w / (1e-12 * np.abs(want["root_ang_vel"]) + 1e-12 * fq[:, None])).max()
    ang = 0.0
    for j in range(E):
        s = int(ids[j])
        T, src = LENS[s], c["q"][OFFS[s]:OFFS[s + 1]][:, [4, 5, 6, 3]]
        u = min(max(ts[j] * FPS[s], 0.0), T - 1.0)
        w = R.from_quat(src[0]) if T == 1 else Slerp(np.arange(T, dtype=np.float64), R.from_quat(src))(u)
        ang = max(ang, float((R.from_quat(got["root_rot"][j]) * w.inv()).magnitude()))
    print(f"[motion_sample] {robot} E={E}: root_rot {e_rot:.3e}, vs scipy {ang:.3e} rad, root_ang_vel {frac:.3e} of the bound")
    assert e_rot <= 1e-12 and ang <= 1e-12 and frac <= 1.0
    # float32 outputs: the single rounding of the float64 result
    g32 = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(ts), dtype=torch.float32))
    for k in GEN:
        assert g32[k].dtype == np.float32 and np.array_equal(g32[k], got[k].astype(np.float32)), k
    assert _same(g32, got, BODY)
    # float32 times are promoted first
    t32 = ts.astype(np.float32)
    a = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(t32), fields=GEN))
    b = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(t32.astype(np.float64)), fields=GEN))
    assert set(a) == set(GEN) and _same(a, b)


# ------------------------------------------------------------------ 2: body poses
@pytest.mark.parametrize("robot", ROBOTS)
def test_body_poses_are_engine_fk_of_the_calls_own_outputs(robot):
    c = _case(robot)
    g = c["got"]
    bp, br = c["gmr"]._engine.fk(_dev(g["root_pos"].astype(np.float32)), _dev(g["root_rot"].astype(np.float32)),
                                 _dev(g["joint_pos"].astype(np.float32)), want_rot=True)
    assert np.array_equal(g["body_pos_w"], bp.cpu().numpy()) and np.array_equal(g["body_quat_w"], br.cpu().numpy())


# ------------------------------------------------------------------ 3: body velocities
@pytest.mark.parametrize("robot", ROBOTS)
def test_body_velocities_within_four_times_the_float32_restatements_error(robot):
    """d32: the largest deviation of the float32 restatement from the float64 one over the 200 queries, per array.  The kernel may
    deviate from the float64 restatement by 4 d32 (its sin / cos and operand order beyond one rounding step)."""
    c = _case(robot)
    for k in ("body_lin_vel_w", "body_ang_vel_w"):
        w64 = c["want"][k]
        d32 = np.abs(c["w32"][k].astype(np.float64) - w64).max()
        dk = np.abs(c["got"][k].astype(np.float64) - w64).max()
        k32 = np.abs(c["got"][k].astype(np.float64) - c["w32"][k].astype(np.float64)).max()
        print(f"[motion_sample] {robot} {k}: d32 {d32:.3e}, kernel {dk:.3e} ({dk / d32:.2f} d32), max |value| {np.abs(w64).max():.2f}, "
              f"kernel vs float32 restatement {k32:.3e}")
        assert d32 > 0 and dk <= 4.0 * d32, k


# ------------------------------------------------------------------ 4: cross-check against the tracking export
@pytest.mark.parametrize("s", [5, 6])
@pytest.mark.parametrize("robot", ROBOTS)
def test_frame_times_reproduce_motion_track_at_equal_rates(robot, s):
    c = _case(robot)
    eng, lib, T, f = c["gmr"]._engine, c["lib"], LENS[s], FPS[s]
    tr = _host(eng.motion_track(lib.qpos[OFFS[s]:OFFS[s + 1]].contiguous(), np.array([0, T], dtype=np.int64), f, f))
    ts = np.arange(T, dtype=np.float64) / f
    got = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(np.full(T, s, dtype=np.int64)), _dev(ts)))
    for k in GEN + ("body_pos_w", "body_quat_w"):
        assert np.array_equal(got[k], tr[k]) and got[k].dtype == tr[k].dtype, k


# ------------------------------------------------------------------ 5: k_per_id and future
def test_k_per_id_and_future():
    c = _case("unitree_g1")
    eng, lib = c["gmr"]._engine, c["lib"]
    E, K = 65, 3
    ids, t0 = c["ids"][:E], c["ts"][:E]
    fut = np.array([0.0, 0.02, 0.3])
    t2 = t0[:, None] + fut[None, :]
    two = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(t2)))
    flat = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(np.repeat(ids, K)), _dev(t2.reshape(-1))))
    assert two["root_pos"].shape == (E, K, 3) and two["body_quat_w"].shape == (E, K, eng.nbody, 4)
    assert all(np.array_equal(two[k].reshape(flat[k].shape), flat[k]) for k in GEN + BODY)
    viak = _host(eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(ids), _dev(t2.reshape(-1)), k_per_id=K))
    assert _same(viak, flat)
    a = _host(lib.query(_dev(ids), _dev(t0), future=_dev(fut), dtype=torch.float64))
    assert _same(a, two)
    b = _host(lib.query(_dev(np.repeat(ids, K)), _dev(t2.reshape(-1))))  # (float32 by default)
    a32 = _host(lib.query(_dev(ids), _dev(t0), future=_dev(fut)))
    assert a32["joint_vel"].dtype == np.float32 and all(np.array_equal(a32[k].reshape(b[k].shape), b[k]) for k in GEN + BODY)


# ------------------------------------------------------------------ 6: body subset
def test_body_subset_and_no_bodies():
    c = _case("unitree_g1")
    lib, names = c["lib"], list(c["gmr"].model.body_names)
    pick = [names[17], names[3], names[len(names) - 1], names[0]]
    ids, ts = _dev(c["ids"]), _dev(c["ts"])
    sub = _host(lib.query(ids, ts, bodies=pick, dtype=torch.float64))
    cols = [names.index(b) for b in pick]
    for k in BODY:
        assert sub[k].shape[1] == 4 and np.array_equal(sub[k], c["got"][k][:, cols]), k
    assert _same(sub, c["got"], GEN)
    assert lib.body_ids(pick) is lib.body_ids(tuple(pick))  # resolved once per tuple of names
    rep = _host(lib.query(ids, ts, bodies=[names[5]] * 3 + [names[6]], fields=("body_pos_w",), dtype=torch.float64))
    assert set(rep) == {"body_pos_w"} and np.array_equal(rep["body_pos_w"], c["got"]["body_pos_w"][:, [5, 5, 5, 6]])
    lean = _host(lib.query(ids, ts, fields=GEN, dtype=torch.float64))
    assert set(lean) == set(GEN) and _same(lean, c["got"], GEN)
    with pytest.raises(KeyError):
        lib.query(ids, ts, bodies=["no_such_body"])


# ------------------------------------------------------------------ 7: invalid queries and non-finite rows
@pytest.mark.parametrize("robot", ROBOTS)
def test_invalid_queries_are_nan_and_touch_nothing_else(robot):
    c = _case(robot)
    lib = c["lib"]
    E = 130
    ids, ts = c["ids"][:E].copy(), c["ts"][:E].copy()
    bad = {3: (-1, 0.1), 64: (len(LENS), 0.1), 65: (2 ** 40, 0.1), 70: (4, 0.0), 100: (5, np.nan), 129: (6, np.inf), 0: (-2 ** 62, 0.0), 63: (5, -np.inf)}
    for j, (s, t) in bad.items():
        ids[j], ts[j] = s, t
    got = _host(lib.query(_dev(ids), _dev(ts), dtype=torch.float64, check=False))
    good = np.array([j not in bad for j in range(E)])
    for k in GEN + BODY:
        assert np.isnan(got[k][~good]).all(), k
        assert np.array_equal(got[k][good], c["got"][k][:E][good]), k
    with pytest.raises(ValueError):
        lib.query(_dev(ids), _dev(ts))
    ok_ids = np.where((ids >= 0) & (ids < len(LENS)), ids, 0)
    lib.query(_dev(ok_ids), _dev(ts))  # the empty clip and the non-finite times pass the id check; their rows are NaN


@pytest.mark.parametrize("robot", ROBOTS)
def test_one_nan_coordinate_poisons_only_the_queries_that_read_it(robot):
    from gmr_amd.dataset import MotionLibrary
    c = _case(robot)
    s, r, col = 5, 20, 7 + 4  # a hinge angle of frame 20 of the 64-frame clip
    q = c["q"].copy()
    q[OFFS[s] + r, col] = np.nan
    lib = MotionLibrary(c["gmr"], q, OFFS, FPS)
    f = FPS[s]
    ts = np.concatenate([np.arange(14, 27) / f, (np.arange(14, 27) + 0.5) / f, c["ts"][:40]])
    ids = np.concatenate([np.full(26, s, dtype=np.int64), c["ids"][:40]])
    got = _host(lib.query(_dev(ids), _dev(ts), dtype=torch.float64))
    clean = _host(c["lib"].query(_dev(ids), _dev(ts), dtype=torch.float64))
    want, (valid, rows, a, h0, h1) = ref.sample(c["tree"], q, OFFS, FPS, ids, ts)
    touched = (rows[:, :4] == OFFS[s] + r).any(axis=1)
    assert 8 <= touched.sum() < len(ids)
    for k in GEN + BODY:
        assert np.array_equal(got[k][~touched], clean[k][~touched]), k            # no other query is affected
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k              # exactly the outputs the formulas poison
        fin = ~np.isnan(want[k])
        if k in ("root_pos", "joint_pos", "root_lin_vel", "joint_vel"):
            assert np.array_equal(got[k][fin], want[k][fin]), k
    assert np.isnan(got["joint_pos"][touched]).any() and not np.isnan(got["root_pos"]).any()


# ------------------------------------------------------------------ 8: refusals and trivia
def test_refusals_and_trivia():
    from gmr_amd import GeneralMotionRetargeting, _native
    from gmr_amd.dataset import MotionLibrary
    from gmr_amd.engine import EngineError
    c = _case("unitree_g1")
    eng, lib = c["gmr"]._engine, c["lib"]
    # no queries: empty tensors, no launch
    none = eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, _dev(np.zeros(0, dtype=np.int64)), _dev(np.zeros(0)))
    assert none["root_pos"].shape == (0, 3) and none["body_quat_w"].shape == (0, eng.nbody, 4)
    none = lib.query(_dev(np.zeros(0, dtype=np.int64)), _dev(np.zeros(0)), future=_dev(np.zeros(3)))
    assert none["joint_pos"].shape == (0, 3, eng.nq - 7)
    torch.cuda.synchronize()
    # a planar base
    planar = GeneralMotionRetargeting("smplx", "galaxea_r1pro", device=0)
    qp = torch.zeros((10, planar._engine.nq), dtype=torch.float64, device="cuda")
    qp[:, 3] = 1.0
    with pytest.raises(EngineError, match="not supported"):
        planar._engine.motion_sample(qp, _dev(np.array([0, 10])), _dev(np.array([30.0])), _dev(np.zeros(4, dtype=np.int64)), _dev(np.zeros(4)))
    with pytest.raises(NotImplementedError):
        MotionLibrary(planar, qp, [0, 10], 30.0)
    # the library's own argument checks
    ids, ts = _dev(c["ids"][:6]), _dev(c["ts"][:6])
    si = _native.SampleInput()
    si.qpos, si.n_frames, si.seq_offsets, si.fps, si.n_seq = lib.qpos.data_ptr(), lib.num_frames, lib._offs_dev.data_ptr(), lib._fps_dev.data_ptr(), lib.num_clips
    si.ids, si.times, si.time_dtype, si.out_dtype, si.n_queries, si.k_per_id = ids.data_ptr(), ts.data_ptr(), 1, 1, 6, 1
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: eng._lib.gmr_motion_sample(eng._h, C.byref(si), stream)
    assert call() == 0  # (no outputs: nothing to write)
    for field, value, back in (("k_per_id", 0, 1), ("k_per_id", 4, 1), ("n_queries", -1, 6), ("n_sel", -1, 0), ("n_sel", 2, 0), ("n_seq", -1, lib.num_clips),
                               ("time_dtype", 7, 1)):
        setattr(si, field, value)
        assert call() == -1, (field, value)
        setattr(si, field, back)
    si.n_queries = 0
    assert call() == 0
    with pytest.raises(EngineError):
        eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, ids, ts.to(torch.float16))
    with pytest.raises(EngineError):
        eng.motion_sample(lib.qpos, lib._offs_dev, lib._fps_dev, ids[:5], ts)
    # a non-default stream
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        other = lib.query(_dev(c["ids"]), _dev(c["ts"]), dtype=torch.float64, check=False)
    st.synchronize()
    assert _same(_host(other), c["got"])


def test_hands_model_fits_in_lds():
    """52 bodies, 43 hinges: the largest tile.  Generalized arrays against the definition, body poses against Engine.fk."""
    c = _case("unitree_g1_with_hands")
    got, want = c["got"], c["want"]
    assert got["body_pos_w"].shape == (200, 52, 3)
    assert all(np.array_equal(got[k], want[k]) for k in ("root_pos", "joint_pos", "root_lin_vel", "joint_vel"))
    bp, br = c["gmr"]._engine.fk(_dev(got["root_pos"].astype(np.float32)), _dev(got["root_rot"].astype(np.float32)),
                                 _dev(got["joint_pos"].astype(np.float32)), want_rot=True)
    assert np.array_equal(got["body_pos_w"], bp.cpu().numpy()) and np.array_equal(got["body_quat_w"], br.cpu().numpy())
    for k in ("body_lin_vel_w", "body_ang_vel_w"):
        d32 = np.abs(c["w32"][k].astype(np.float64) - want[k]).max()
        assert np.abs(got[k].astype(np.float64) - want[k]).max() <= 4.0 * d32, k


# ------------------------------------------------------------------ 9: MotionLibrary
def test_motion_library_from_motions_and_sampling():
    import gmr_amd
    from gmr_amd import dataset, synth
    from gmr_amd.schedule import clip_durations
    assert gmr_amd.MotionLibrary is dataset.MotionLibrary
    g = _gmr("unitree_g1")
    dev = torch.device("cuda", 0)
    lens = np.array([40, 25, 33])
    pos, quat, names, offs = synth.synth_clips_torch(compiled("smplx", "unitree_g1"), lens, seed=11, device=dev, yaw0=0.3, dtype=torch.float64)
    motions = dataset.retarget_clips(g, pos, quat, names, offs, fps=32)  # (k / 32) * 32 == k: frame times are exact
    lib = dataset.MotionLibrary.from_motions(g, motions)
    assert lib.num_clips == 3 and lib.num_frames == int(lens.sum())
    assert np.array_equal(lib.durations.cpu().numpy(), clip_durations(lib.seq_offsets, 32.0))
    for s, m in enumerate(motions):
        T = int(lens[s])
        got = _host(lib.query(_dev(np.full(T, s, dtype=np.int64)), _dev(np.arange(T) / 32.0), fields=("root_pos", "root_rot", "joint_pos"),
                              dtype=torch.float64))
        assert np.array_equal(got["root_pos"], m["root_pos"]) and np.array_equal(got["root_rot"], m["root_rot"])
        assert np.array_equal(got["joint_pos"], m["dof_pos"])
    # sampling: the empty clip is never drawn, a seeded generator reproduces, times lie inside the clips
    c = _case("unitree_g1")
    big = c["lib"]
    assert np.array_equal(big.durations.cpu().numpy(), clip_durations(OFFS, FPS)) and big.durations.dtype == torch.float64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    ids = big.sample_ids(4096, generator=gen)
    ts = big.sample_times(ids, generator=gen)
    gen.manual_seed(3)
    ids2 = big.sample_ids(4096, generator=gen)
    assert torch.equal(ids, ids2) and torch.equal(ts, big.sample_times(ids2, generator=gen))
    drawn = set(ids.cpu().numpy().tolist())
    assert drawn <= {1, 2, 3, 5, 6} and {5, 6} <= drawn  # clips 0 (one frame: duration 0) and 4 (no frames) have no weight
    assert bool((ts >= 0).all()) and bool((ts <= big.durations[ids]).all()) and ts.dtype == torch.float64
    still = dataset.MotionLibrary(g, c["q"][:3], [0, 1, 1, 2, 3], 30.0)  # every duration 0: uniform over the clips with a frame
    assert set(still.sample_ids(512, generator=gen).cpu().numpy().tolist()) == {0, 2, 3}
    # caller-owned outputs are written in place
    out = {k: torch.zeros_like(v) for k, v in big.query(_dev(c["ids"]), _dev(c["ts"]), check=False).items()}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    res = big.query(_dev(c["ids"]), _dev(c["ts"]), out=out, check=False)
    assert all(res[k] is out[k] and out[k].data_ptr() == ptrs[k] for k in out) and set(res) == set(GEN + BODY)
    ref32 = _host(big.query(_dev(c["ids"]), _dev(c["ts"])))
    assert _same(_host(out), ref32)
    part = big.query(_dev(c["ids"]), _dev(c["ts"]), out={"joint_vel": out["joint_vel"]}, check=False)
    assert set(part) == {"joint_vel"}
