"""The kernels' large-launch paths, at the sizes production batches reach: grid-stride loops that go round several times
(dof_to_rot_kernel, rot_to_dof_kernel), wavefronts that take several batches (local_to_global_kernel), per-wavefront chunks past
8 frames whose double-buffered refill really loads data (bvh_fk_kernel, smplx_keypoints_kernel), and the group epilogue with
members that differ in clips, flags and work.  Every test first asserts that its size reaches the path it is about, naming the
launch constant it depends on, so a later change of a grid cap makes the test say so instead of quietly testing the small path.

Large inputs are drawn on the device with a seeded torch.Generator; only what a reference needs travels to the host."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from tests.test_gpu_adapters import _bvh_restatement, _random_tree, _smplx_restatement  # noqa: E402
from tests.test_gpu_motion_epilogue import KEYS, _gmr, _random_qpos  # noqa: E402
from tests.util import compiled  # noqa: E402

vp = C.c_void_p
NAN = float("nan")

# launch constants of api.hip the sizes below are chosen against
KIN_THREADS = 256                         # kKinThreads
KIN_STRIDE = 256 * 32 * KIN_THREADS       # kin_grid: at most 256 x 32 workgroups of 256 threads, one item per thread and stride
KIN_WAVES = 256 * 64                      # gmr_local_rot_to_global: at most 256 x 64 one-wavefront workgroups
KIN_PASSES = 8                            # GMR_KIN_CHAIN_PASSES: a batch of local_to_global_kernel is 64 x 8 quaternions
ADAPTER_WAVES = 16384                     # adapter_chunk: ceil(T / 16384) frames per wavefront, clamped to [8, 64]
SLICE = 8 * ADAPTER_WAVES                 # the most frames one adapter launch takes with 8-frame chunks


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _bits_equal(a, b):
    """Bit for bit (NaN payloads and signed zeros included), on the device."""
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


def _groups(J):  # tree_chain.hip.h chain_geom: frames a wavefront runs side by side
    return 1 if J > 32 else 64 // (1 << (J - 1).bit_length())


def _adapter_chunk(T, groups):  # api.hip adapter_chunk
    c = min(max(-(-T // ADAPTER_WAVES), 8), 64)
    return -(-c // groups) * groups


def _bvh_batch(per_frame, groups):  # bvh_kernel.hip.h bvh_batch: frames per stage buffer
    n = min(2304 // 8 // per_frame, 8)
    if n < groups:
        n = min(groups, 8)
    n = max(n, 1)
    return n // groups * groups if n >= groups else n


# ---------------------------------------------------------------------------------------------------------------- kin ops
@pytest.mark.parametrize("robot", ["unitree_g1", "unitree_g1_with_hands"])
def test_kin_ops_several_strides_and_batches_per_wavefront(robot, dev):
    """Every frame of local_rot_to_global (bit for bit), dof_to_rot and rot_to_dof against the oracle, at sizes where every
    wavefront of local_to_global_kernel runs 3 or more batches (and, at a second size, only some run a second one) and every
    thread of the two grid-stride kernels runs 3 or more strides.  Outputs start as NaN, so a frame the kernel skips fails."""
    from gmr_amd.engine import Engine
    cm = compiled("smplx", robot)
    eng, orc = Engine(cm, 0), Oracle(cm.blob)
    nb, nd = cm.robot.nbody, cm.robot.nq - 7
    F = 64 * KIN_PASSES // nb  # frames per batch
    g = _gen(dev, nb)
    T_many = 3 * KIN_WAVES * F + 5
    T_over = (KIN_WAVES + 1001) * F + F // 2 + 1
    for T in (T_many, T_over):
        n_batches = -(-T // F)
        assert T % F != 0  # a ragged last batch
        if T == T_many:
            assert n_batches > 3 * KIN_WAVES  # every wavefront runs at least 3 batches
        else:
            assert KIN_WAVES < n_batches < 2 * KIN_WAVES  # only some wavefronts go round twice
        q = torch.randn((T, nb, 4), generator=g, device=dev)
        q /= torch.linalg.vector_norm(q, dim=-1, keepdim=True)
        q_h = q.cpu().numpy()
        out = torch.full_like(q, NAN)
        eng.local_rot_to_global(q, out=out)
        assert np.array_equal(out.cpu().numpy(), orc.local_rot_to_global(q_h)), (robot, T)
        del out
        if T != T_many:
            continue
        # each thread runs >= 3 strides; a stride that is not a multiple of the row length moves the (frame, joint) pair by
        # a remainder and wraps
        assert T * (nb - 1) > 3 * KIN_STRIDE and KIN_STRIDE % (nb - 1) != 0
        assert T * nd > 3 * KIN_STRIDE and KIN_STRIDE % nd != 0
        dof = torch.rand((T, nd), generator=g, device=dev) * 6.4 - 3.2
        jr = torch.full((T, nb - 1, 4), NAN, device=dev)
        eng.dof_to_rot(dof, out=jr)
        err = np.abs(jr.cpu().numpy() - orc.dof_to_rot(dof.cpu().numpy())).max()
        assert err < 2e-7, (robot, err)
        del jr, dof
        r = q[:, 1:].contiguous()
        dd = torch.full((T, nd), NAN, device=dev)
        eng.rot_to_dof(r, out=dd)
        err = np.abs(dd.cpu().numpy() - orc.rot_to_dof(np.ascontiguousarray(q_h[:, 1:]))).max()
        assert err < 2e-6, (robot, err)
        del r, dd
    eng.close()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- BVH adapter
def _bvh_into(lib, parents, order, extra_pos, extra_rot, layout, d_off, d_rows, scale, out_cols, pos, quat):
    """gmr_bvh_fk_rows on device rows into caller-owned (possibly sliced) outputs."""
    J, E = len(parents), len(extra_pos)
    par, od = np.ascontiguousarray(parents, np.int32), np.asarray(order, np.int32)
    ep, er = np.asarray(extra_pos, np.int32), np.asarray(extra_rot, np.int32)
    oc = None if out_cols is None else np.asarray(out_cols, np.int32)
    B = pos.shape[1]
    return lib.gmr_bvh_fk_rows(par.ctypes.data_as(vp), J, od.ctypes.data_as(vp), ep.ctypes.data_as(vp) if E else None,
                               er.ctypes.data_as(vp) if E else None, E, layout, vp(d_off.data_ptr()), vp(d_rows.data_ptr()),
                               d_rows.shape[1], d_rows.shape[0], scale, oc.ctypes.data_as(vp) if oc is not None else None, B,
                               vp(pos.data_ptr()), vp(quat.data_ptr()), None)


def _bvh_decode(layout, rows, offsets):
    """The local positions and Euler degrees the kernel reads from rows (rows-9: offset + position * scale, numpy's two roundings)."""
    n, J = rows.shape[0], offsets.shape[0]
    lpos = np.repeat(offsets[None], n, axis=0)
    eul = np.zeros((n, J, 3))
    lpos[:, 0] = rows[:, :3]
    if layout == 3:
        eul[:] = rows[:, 3:].reshape(n, J, 3)
    else:
        blk = rows[:, 3:].reshape(n, J - 1, 9)
        lpos[:, 1:] = offsets[None, 1:] + blk[:, :, 0:3] * blk[:, :, 6:9]
        eul[:, 1:] = blk[:, :, 3:6]  # the root keeps a zero rotation
    return lpos, eul


@pytest.mark.parametrize("J,T,layout", [
    (22, 300_007, 3),     # the LAFAN1 shape: 4 frames per batch, a chunk of 20
    (5, 1_040_003, 3),    # 8 frames per batch, the largest chunk (64): 8 batches per wavefront
    (12, 200_003, 9),     # 9-channel rows, two extra entries, a column selection
])
def test_bvh_fk_rows_chunks_over_8_frames(J, T, layout, dev):
    """One large gmr_bvh_fk_rows launch (chunks past 8 frames, refills that load) equals, bit for bit on every frame, the same
    rows in launches of at most 131 072 frames (8-frame chunks); windows around chunk and batch edges, on the last wavefront and
    on the final frame, equal the numpy restatement."""
    lib = _native.load()
    rng = np.random.default_rng(J)
    parents = _random_tree(rng, J, 0.6)
    order = tuple(int(x) for x in rng.permutation(3))
    offsets = rng.normal(0, 20.0, (J, 3))
    extra_pos = [int(x) for x in rng.integers(0, J, 2)]
    extra_rot = [int(x) for x in rng.integers(0, J, 2)]
    B = J + 2
    out_cols = [int(x) for x in rng.permutation(J)[:7]] + [J + 1, J] if layout == 9 else None  # 7 joints and both extras
    NO = B if out_cols is None else len(out_cols)
    g = _gen(dev, J)
    root = torch.randn((T, 3), generator=g, device=dev, dtype=torch.float64) * 50.0 + torch.tensor([0.0, 90.0, 0.0], device=dev, dtype=torch.float64)
    if layout == 3:
        rows = torch.cat([root, torch.rand((T, 3 * J), generator=g, device=dev, dtype=torch.float64) * 360.0 - 180.0], dim=1)
    else:
        blk = torch.cat([torch.randn((T, J - 1, 3), generator=g, device=dev, dtype=torch.float64) * 5.0,
                         torch.rand((T, J - 1, 3), generator=g, device=dev, dtype=torch.float64) * 360.0 - 180.0,
                         torch.rand((T, J - 1, 3), generator=g, device=dev, dtype=torch.float64) * 1.5 + 0.5], dim=2)
        rows = torch.cat([root, blk.reshape(T, -1)], dim=1)
        del blk
    del root
    G = _groups(J)
    chunk, nbatch = _adapter_chunk(T, G), _bvh_batch(rows.shape[1], G)
    assert T > SLICE and chunk > 8               # adapter_chunk: more than 16384 x 8 frames
    assert chunk >= 3 * nbatch                   # the refill of the batch after next loads rows (bvh_batch: <= 8 frames per batch)
    if J == 5:
        assert chunk == 64 and chunk // nbatch == 8  # T > 63 x 16384
    assert _adapter_chunk(SLICE, G) == 8
    d_off = torch.from_numpy(offsets).to(dev)
    pos = torch.full((T, NO, 3), NAN, dtype=torch.float64, device=dev)
    quat = torch.full((T, NO, 4), NAN, dtype=torch.float64, device=dev)
    assert _bvh_into(lib, parents, order, extra_pos, extra_rot, layout, d_off, rows, 0.01, out_cols, pos, quat) == 0
    pos_s, quat_s = torch.full_like(pos, NAN), torch.full_like(quat, NAN)
    for a in range(0, T, SLICE):
        b = min(a + SLICE, T)
        assert _bvh_into(lib, parents, order, extra_pos, extra_rot, layout, d_off, rows[a:b], 0.01, out_cols, pos_s[a:b], quat_s[a:b]) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(pos).any() and not torch.isnan(quat).any()
    assert _bits_equal(pos, pos_s) and _bits_equal(quat, quat_s)
    del pos_s, quat_s
    # restatement windows: whole chunks of a few wavefronts with two frames on either side (every batch edge in them)
    nblk = -(-T // chunk)
    frames = set()
    for w in (0, 1, nblk // 2, nblk - 2, nblk - 1):
        frames.update(range(max(w * chunk - 2, 0), min((w + 1) * chunk + 2, T)))
    idx = np.array(sorted(frames))
    assert idx[-1] == T - 1
    sel = torch.from_numpy(idx).to(dev)
    lpos, eul = _bvh_decode(layout, rows[sel].cpu().numpy(), offsets)
    p_ref, q_ref = _bvh_restatement(parents, order, lpos, np.radians(eul), extra_pos, extra_rot, 0.01)
    if out_cols is not None:
        p_ref, q_ref = p_ref[:, out_cols], q_ref[:, out_cols]
    got_p, got_q = pos[sel].cpu().numpy(), quat[sel].cpu().numpy()
    scale_p = max(1.0, np.abs(p_ref).max())
    assert np.abs(got_p - p_ref).max() < 1e-11 * scale_p * max(1, J // 8)
    assert np.abs(got_q - q_ref).max() < 1e-12 * max(1, J // 4)
    del pos, quat, rows
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- SMPL-X adapter
def _smplx_into(lib, parents, J, S, go, fp, jt, T_out, resample, pos, quat):
    """gmr_smplx_keypoints_in on device arrays (float32 or float64) into caller-owned outputs."""
    par = np.ascontiguousarray(parents, np.int32)
    dt = _native.GMR_DTYPE_F32 if go.dtype == torch.float32 else _native.GMR_DTYPE_F64
    return lib.gmr_smplx_keypoints_in(par.ctypes.data_as(vp), J, S, vp(go.data_ptr()), vp(fp.data_ptr()), vp(jt.data_ptr()), dt,
                                      go.shape[0], T_out, int(resample), None, J, vp(pos.data_ptr()), vp(quat.data_ptr()), None)


def _smplx_inputs(g, dev, T, J, S, dtype, spread):
    go = torch.randn((T, 3), generator=g, device=dev, dtype=dtype) * 0.5
    fp = torch.randn((1, J, 3), generator=g, device=dev, dtype=dtype) * 0.5 + torch.randn((T, J, 3), generator=g, device=dev, dtype=dtype) * spread
    jt = torch.randn((1, S, 3), generator=g, device=dev, dtype=dtype) * 0.5 + torch.randn((T, S, 3), generator=g, device=dev, dtype=dtype) * 0.01
    return go, fp, jt


def _smplx_close(pos, quat, p_ref, q_ref):
    assert np.abs(pos - p_ref).max() < 1e-12
    d = np.minimum(np.abs(quat - q_ref).max(-1), np.abs(quat + q_ref).max(-1))
    assert d.max() < 1e-10, d.max()


def test_smplx_keypoints_1to1_chunk_64(dev):
    """resample = 0, 24 joints, T > 1 032 192: one launch (64-frame chunks, 32 iterations of the next-rows prefetch per wavefront)
    equals launches of at most 131 072 frames bit for bit; the first and last wavefronts' frames equal the restatement."""
    lib = _native.load()
    rng = np.random.default_rng(24)
    J, S, T = 24, 29, 1_040_003
    parents = _random_tree(rng, J, 0.6)
    assert T > 63 * ADAPTER_WAVES and _adapter_chunk(T, _groups(J)) == 64 and _adapter_chunk(SLICE, _groups(J)) == 8
    go, fp, jt = _smplx_inputs(_gen(dev, 24), dev, T, J, S, torch.float64, 0.3)
    pos = torch.full((T, J, 3), NAN, dtype=torch.float64, device=dev)
    quat = torch.full((T, J, 4), NAN, dtype=torch.float64, device=dev)
    assert _smplx_into(lib, parents, J, S, go, fp, jt, T, 0, pos, quat) == 0
    pos_s, quat_s = torch.full_like(pos, NAN), torch.full_like(quat, NAN)
    for a in range(0, T, SLICE):
        b = min(a + SLICE, T)
        assert _smplx_into(lib, parents, J, S, go[a:b], fp[a:b], jt[a:b], b - a, 0, pos_s[a:b], quat_s[a:b]) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(pos).any() and not torch.isnan(quat).any()
    assert _bits_equal(pos, pos_s) and _bits_equal(quat, quat_s)
    del pos_s, quat_s
    for a, b in ((0, 130), (T - 64 - 3, T)):  # frames are independent at resample = 0: a window is a clip of its own
        p_ref, q_ref = _smplx_restatement(go[a:b].cpu().numpy(), fp[a:b].cpu().numpy(), jt[a:b].cpu().numpy(), parents, b - a, False)
        _smplx_close(pos[a:b].cpu().numpy(), quat[a:b].cpu().numpy(), p_ref, q_ref)
    del pos, quat, go, fp, jt
    torch.cuda.empty_cache()


def test_smplx_keypoints_resampled_long_clip(dev):
    """SMPL-X's 55 joints at 120 -> 30 fps over a long clip (T_out > 131 072: chunks past 8 frames): sampled output frames on both
    sides of several chunk edges, on the last wavefront and the linspace endpoint k = T_out - 1 equal the restatement; float32
    input through gmr_smplx_keypoints_in equals, bit for bit, the float64 call on the promoted arrays."""
    from gmr_amd.smplx_adapter import SMPLX_PARENTS
    lib = _native.load()
    parents = np.asarray(SMPLX_PARENTS, np.int32)
    J, S, T = 55, 60, 600_003
    T_out = T // 4  # frame_skip = 120 / 30 (smplx_adapter.get_smplx_data_offline_fast)
    chunk = _adapter_chunk(T_out, _groups(J))
    assert len(parents) == J and T_out > SLICE and chunk > 8  # adapter_chunk: more than 16384 x 8 output frames
    go32, fp32, jt32 = _smplx_inputs(_gen(dev, 55), dev, T, J, S, torch.float32, 0.05)  # neighbours 0.1 rad apart: both slerp arms
    go, fp, jt = go32.double(), fp32.double(), jt32.double()
    pos = torch.full((T_out, J, 3), NAN, dtype=torch.float64, device=dev)
    quat = torch.full((T_out, J, 4), NAN, dtype=torch.float64, device=dev)
    assert _smplx_into(lib, parents, J, S, go, fp, jt, T_out, 1, pos, quat) == 0
    pos32, quat32 = torch.full_like(pos, NAN), torch.full_like(quat, NAN)
    assert _smplx_into(lib, parents, J, S, go32, fp32, jt32, T_out, 1, pos32, quat32) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(pos).any() and not torch.isnan(quat).any()
    assert _bits_equal(pos, pos32) and _bits_equal(quat, quat32)
    del pos32, quat32, go32, fp32, jt32
    nblk = -(-T_out // chunk)
    ks = {0, 1, T_out - 2, T_out - 1}
    for w in (1, 2, 3, nblk // 3, nblk // 2, nblk - 2, nblk - 1):
        ks.update((w * chunk - 2, w * chunk - 1, w * chunk, w * chunk + 1))
    ks = sorted(k for k in ks if 0 <= k < T_out)
    # only the input rows the samples read go to the host (np.zeros pages the rest in on touch only)
    tt = np.linspace(0, T - 1, T_out)[ks]
    need = np.unique(np.concatenate([np.floor(tt), np.minimum(np.floor(tt) + 1, T - 1)]).astype(np.int64))
    d_need = torch.from_numpy(need).to(dev)
    go_h, fp_h, jt_h = np.zeros((T, 3)), np.zeros((T, J, 3)), np.zeros((T, S, 3))
    go_h[need], fp_h[need], jt_h[need] = go[d_need].cpu().numpy(), fp[d_need].cpu().numpy(), jt[d_need].cpu().numpy()
    p_ref, q_ref = _smplx_restatement(go_h, fp_h, jt_h, parents, T_out, True, ks=ks)
    d_ks = torch.tensor(ks, device=dev)
    _smplx_close(pos[d_ks].cpu().numpy(), quat[d_ks].cpu().numpy(), p_ref, q_ref)
    del pos, quat, go, fp, jt
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- group epilogue
GROUP = ["unitree_g1", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01"]
CLIPS = {
    "a": [0, 0, 1, 1, 65, 66, 300],      # an empty first clip, clips of one frame, one across several tiles
    "b": [0, 1000, 1000, 1001, 4097],    # long clips around an empty and a one-frame clip
    "c": [0, 7, 7],                      # one short clip, then an empty one
    "big": [0, 1, 640_001, 640_005],     # more than 10 000 tiles of 64 frames
    "zero": [0, 0],                      # a member with no frames
}
# (clip table per member, None = no batch at all; members that also ask for min_z)
ARRANGEMENTS = [
    (["none", "a", "zero", "b", "c"], {1, 2, 4}),   # no work first and in the middle
    (["zero", "b", "none", "c", "a"], {0, 3}),
    (["c", "big", "a", "zero", "none"], {1, 3}),    # no work last
]
_QPOS = {}


@pytest.fixture(scope="module")
def group():
    from gmr_amd import MultiRobotRetargeting
    mr = MultiRobotRetargeting("smplx", GROUP, device=0)
    yield mr
    mr.close()
    _QPOS.clear()


def _member_qpos(robot, name, seed):
    key = (robot, name)
    if key not in _QPOS:
        offs = np.asarray(CLIPS[name], np.int64)
        _QPOS[key] = _random_qpos(robot, offs, seed) if offs[-1] else torch.zeros((0, compiled("smplx", robot).robot.nq), dtype=torch.float64, device="cuda")
    return _QPOS[key]


@pytest.mark.parametrize("height,origin", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("arr", range(len(ARRANGEMENTS)))
def test_group_epilogue_members_differ(group, arr, height, origin):
    """gmr_group_motion_epilogue with members that have no batch or no frames (first, in the middle, last), their own clip
    tables (empty clips, one-frame clips, clips over many tiles, a member of more than 10 000 tiles) and min_z on some members
    only (so the pass-2 work differs per member): each member's four arrays and min_z equal, bit for bit, Engine.motion_epilogue
    for that member alone, dataset.motions_from_qpos and fk_min_height."""
    from gmr_amd import dataset
    names, want_min = ARRANGEMENTS[arr]
    assert any(np.diff(CLIPS[n]).sum() == 0 for n in names if n != "none") and "none" in names
    if "big" in names:
        assert (CLIPS["big"][-1] + 63) // 64 > 10_000  # kFkWave = 64 frames per tile
    ground = 0.03
    batches, mins = [], []
    for i, (r, n) in enumerate(zip(GROUP, names)):
        if n == "none":
            batches.append(None)
            mins.append(None)
            continue
        batches.append((_member_qpos(r, n, 100 + 7 * i), np.asarray(CLIPS[n], np.int64)))
        mins.append(torch.full((len(CLIPS[n]) - 1,), NAN, dtype=torch.float32, device="cuda") if i in want_min else None)
    got = group.group.motion_epilogue(batches, height_adjust=height, root_origin_offset=origin, ground_offset=ground, min_z=mins)
    for i, (r, n) in enumerate(zip(GROUP, names)):
        if n == "none":
            assert got[i] is None
            continue
        q, offs = batches[i]
        eng = _gmr(r)._engine
        N = int(offs[-1])
        assert tuple(got[i][3].shape) == (N, eng.nbody, 3)
        mz = torch.full_like(mins[i], NAN) if mins[i] is not None else None
        alone = eng.motion_epilogue(q, offs, height_adjust=height, root_origin_offset=origin, ground_offset=ground, min_z=mz)
        for k, a, b in zip(KEYS, got[i], alone):
            assert _bits_equal(a, b), (r, n, k)
        if mins[i] is not None:
            assert _bits_equal(mins[i], mz), (r, n)
            if N:
                q32 = q.to(torch.float32)
                want = eng.fk_min_height(q32[:, :3].contiguous(), q[:, [4, 5, 6, 3]].to(torch.float32), q32[:, 7:].contiguous(), offs)
                assert _bits_equal(mins[i], want), (r, n)
            else:
                assert torch.isinf(mins[i]).all() and (mins[i] > 0).all()  # fk_min_height's value for a clip without frames
        if N == 0:
            continue
        ref = dataset.motions_from_qpos(_gmr(r), q, offs, 30, height_adjust=height, root_origin_offset=origin, ground_offset=ground)
        host = [t.cpu().numpy() for t in got[i]]
        for s in range(len(offs) - 1):
            a, b = offs[s], offs[s + 1]
            for k, arr_ in zip(KEYS, host):
                assert np.array_equal(arr_[a:b], ref[s][k]) and arr_.dtype == ref[s][k].dtype, (r, n, s, k)
        del ref, host


def _at_byte_offset(shape, dtype, shift):
    """A contiguous tensor of `shape` that starts `shift` elements into a NaN-filled buffer."""
    buf = torch.full((int(np.prod(shape)) + shift,), NAN, dtype=dtype, device="cuda")
    return buf[shift:].view(shape)


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_t1"])
def test_engine_epilogue_unaligned_out(robot):
    """Caller out= tensors at a byte offset that is not a multiple of 16 take the epilogue's scalar store fallback for the tile
    image of local_body_pos; the results equal an aligned call bit for bit."""
    offs = np.array([0, 37, 37, 101, 330, 331, 500], dtype=np.int64)
    eng = _gmr(robot)._engine
    q = _random_qpos(robot, offs, seed=77)
    N = int(offs[-1])
    for height in (True, False):
        ref = eng.motion_epilogue(q, offs, height_adjust=height, ground_offset=0.02)
        out = (_at_byte_offset((N, 3), torch.float64, 1), _at_byte_offset((N, 4), torch.float64, 1),
               _at_byte_offset((N, eng.nq - 7), torch.float64, 1), _at_byte_offset((N, eng.nbody, 3), torch.float32, 1))
        assert all(t.is_contiguous() and t.data_ptr() % 16 != 0 for t in out)  # the `(dst & 15) == 0` test of motion_kernel fails
        got = eng.motion_epilogue(q, offs, height_adjust=height, ground_offset=0.02, out=out)
        assert all(g is o for g, o in zip(got, out))
        for k, a, b in zip(KEYS, got, ref):
            assert _bits_equal(a, b), (robot, height, k)
