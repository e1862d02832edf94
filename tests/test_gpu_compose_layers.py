"""The layers on top of Engine.motion_compose: dataset.compose_clips and dataset.repeat_clip, and the result as ordinary
(qpos, seq_offsets) through tracking_from_qpos and MotionLibrary."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd.compose import ComposeError, ComposePlan, Segment  # noqa: E402
from tests import compose_inputs as ci  # noqa: E402
from tests import compose_reference as CR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev  # noqa: E402
from tests.test_gpu_compose import gpu  # noqa: E402

K1 = "booster_k1"
CHAINS = [[Segment(ci.C63, 0, 63), Segment(ci.C64, 0, 64), Segment(ci.C65, 0, 65), Segment(ci.C130, 0, 130), Segment(ci.C63, 10, 40)],
          [Segment(ci.C130, 20, 60), Segment(ci.C65, 0, 30)]]                               # case c's


@functools.lru_cache(maxsize=None)
def retargeter(robot):
    from gmr_amd import GeneralMotionRetargeting
    return GeneralMotionRetargeting("smplx", robot, device=0, verbose=False)


def test_compose_clips_and_repeat_clip_equal_the_engine_on_the_same_plan():
    import gmr_amd
    from gmr_amd import dataset
    g = retargeter(K1)
    q = _dev(ci.qpos(K1))
    out, offs, T = dataset.compose_clips(g, q, ci.OFFS, CHAINS, blend=8)
    plan = ci.case(K1, "blend8")[1]
    assert offs.dtype == np.int64 and np.array_equal(offs, plan.out_offsets) and tuple(out.shape) == (plan.n_out_frames, g._engine.nq)
    assert np.array_equal(_bytes(out.cpu().numpy()), _bytes(gpu(K1, "blend8")[0])) and np.array_equal(_bytes(T.cpu().numpy()), _bytes(gpu(K1, "blend8")[1]))
    assert dataset.compose_clips.__defaults__ == (8,) and gmr_amd.compose_clips is dataset.compose_clips and gmr_amd.repeat_clip is dataset.repeat_clip
    # a cycle: the 65-frame clip three times over
    rep, roffs, rT = dataset.repeat_clip(g, q, ci.OFFS, ci.C65, 3, 5)
    cyc = ComposePlan(ci.OFFS, [[Segment(ci.C65, 0, 65)] * 3], 5)
    want, wantT = g._engine.motion_compose(q, cyc)
    assert roffs.tolist() == [0, 3 * 65 - 2 * 5] and np.array_equal(_bytes(rep.cpu().numpy()), _bytes(want.cpu().numpy()))
    assert np.array_equal(_bytes(rT.cpu().numpy()), _bytes(wantT.cpu().numpy()))
    ref, refT = CR.compose(cyc, np.array(ci.qpos(K1)))
    assert np.array_equal(_bytes(rT.cpu().numpy()), _bytes(refT)) and np.array_equal(_bytes(rep.cpu().numpy()[:, 7:]), _bytes(ref[:, 7:]))
    # each pass starts where the last one ended: the placed anchor rows of a transition coincide in xy and heading
    qh, got = ci.qpos(K1), rep.cpu().numpy()
    a = int(ci.OFFS[ci.C65])
    for k in (1, 2):
        pa, pb = CR.place(refT[k - 1], qh[a + 62:a + 63], k == 1), CR.place(refT[k], qh[a + 2:a + 3], False)
        L = float(np.abs(got[:, :2]).max())
        assert np.abs(pa[0, :2] - pb[0, :2]).max() <= CR.mp_bound(3, L)
        ha, hb = CR.heading(pa[0, 3:7]), CR.heading(pb[0, 3:7])
        assert abs(float(ha[0]) - float(hb[0])) <= CR.mp_bound(3, 1.0) and abs(float(ha[1]) - float(hb[1])) <= CR.mp_bound(3, 1.0)
    with pytest.raises(ComposeError, match="segment 1"):
        dataset.compose_clips(g, q, ci.OFFS, [[Segment(ci.C63, 0, 10), Segment(ci.C64, 0, 10)]], blend=11)


def test_the_result_is_ordinary_qpos_for_the_tracking_export_and_the_motion_library():
    from gmr_amd import dataset
    g = retargeter(K1)
    q = _dev(ci.qpos(K1))
    out, offs, _ = dataset.compose_clips(g, q, ci.OFFS, CHAINS, blend=8)
    tracks = dataset.tracking_from_qpos(g, out, offs, 30.0, 30.0)
    assert len(tracks) == 2
    host = out.cpu().numpy()
    for s, tr in enumerate(tracks):
        a, b = int(offs[s]), int(offs[s + 1])
        assert np.asarray(tr["root_pos"]).shape == (b - a, 3) and np.all(np.isfinite(np.asarray(tr["joint_vel"])))
        assert np.abs(np.asarray(tr["root_pos"], np.float64) - host[a:b, :3]).max() <= 1e-12   # the same rate: the rows themselves
        assert np.abs(np.asarray(tr["joint_pos"], np.float64) - host[a:b, 7:]).max() <= 1e-12
    lib = dataset.MotionLibrary(g, out, offs, fps=30.0)
    assert lib.num_clips == 2 and lib.num_frames == int(offs[-1])
    ids = torch.tensor([0, 1], dtype=torch.int64, device=DEV())
    frames = torch.tensor([100, 45], dtype=torch.float64, device=DEV())                     # whole frames: the rows themselves
    ref = lib.query(ids, frames / 30.0, dtype=torch.float64)
    rows = host[[100, int(offs[1]) + 45]]
    assert np.abs(ref["root_pos"].cpu().numpy().reshape(2, 3) - rows[:, :3]).max() <= 1e-12
    assert np.abs(ref["joint_pos"].cpu().numpy().reshape(2, -1) - rows[:, 7:]).max() <= 1e-12
