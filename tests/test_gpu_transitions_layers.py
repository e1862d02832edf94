"""The layers on top of gmr_motion_transitions: Engine.motion_transitions (allocation, a side stream, body subsets),
dataset.find_transitions (names, defaults) and the way on to compose_clips through transitions.transition_walks."""
import functools
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import transitions as tr  # noqa: E402
from gmr_amd.compose import ComposePlan  # noqa: E402
from tests import transitions_inputs as ti  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_transitions import main_case  # noqa: E402

K1 = "booster_k1"
L = 8


@functools.lru_cache(maxsize=None)
def retargeter(robot):
    from gmr_amd import GeneralMotionRetargeting
    return GeneralMotionRetargeting("smplx", robot, device=0, verbose=False)


def test_the_engine_allocates_runs_on_a_side_stream_and_takes_device_offsets():
    q, offs = ti.library(K1, L)
    ids, w = ti.all_bodies(K1)
    eng, base = engine(K1), main_case(K1, L)[0]
    qd = _dev(q)
    mt = eng.motion_transitions(qd, offs, ids, 3.0 * w, L, min_gap=L)                        # weights are normalised: a common factor drops out
    assert sorted(mt) == ["best_cost", "best_frame", "moments", "points"] and mt.window == L and mt.stride == 1 and mt.min_gap == L
    assert np.array_equal(_bytes(mt["best_cost"].cpu().numpy()), _bytes(base["best_cost"])) and np.array_equal(mt["best_frame"].cpu().numpy(), base["best_frame"])
    assert mt["best_frame"].dtype == torch.int32 and bool(torch.isnan(mt["moments"][1, 3:]).all())   # (a one-frame clip starts no window: not written)
    side = torch.cuda.Stream(DEV())
    torch.cuda.synchronize()
    ms = eng.motion_transitions(qd, torch.from_numpy(offs).to(DEV()), ids, w, L, min_gap=L, dense=True, stream=side)
    side.synchronize()
    for k in ("points", "best_cost", "best_frame", "cost_out"):
        assert np.array_equal(_bytes(ms[k].cpu().numpy()), _bytes(base[k])), k


def test_find_transitions_names_defaults_and_the_way_on_to_compose_clips():
    import gmr_amd
    from gmr_amd import dataset
    g = retargeter(K1)
    q, offs = ti.library(K1, L)
    qd = _dev(q)
    sig = inspect.signature(dataset.find_transitions)
    assert sig.parameters["window"].default == 8 == tr.DEFAULT_WINDOW and gmr_amd.find_transitions is dataset.find_transitions
    assert all(sig.parameters[k].default is None for k in ("bodies", "weights", "src_clips", "dst_clips", "min_gap", "threshold", "radius"))
    # the defaults are all bodies, equal weights, min_gap = window: the main comparison's search
    trans, bc, bf = dataset.find_transitions(g, qd, offs, threshold=np.inf)
    base = main_case(K1, L)[0]
    assert np.array_equal(_bytes(bc), _bytes(base["best_cost"])) and np.array_equal(bf, base["best_frame"])
    src, so, dst, do = ti.tables(offs, L)
    assert trans == tr.select_transitions(bc, bf, src, so, 1, dst, np.inf, L) and len(trans) > 20
    assert all(bc[int(so[t.src_clip]) + t.src_frame, t.dst_clip] == t.cost and bf[int(so[t.src_clip]) + t.src_frame, t.dst_clip] == t.dst_frame for t in trans)
    assert dataset.find_transitions(g, qd, offs)[0] == tr.select_transitions(bc, bf, src, so, 1, dst, tr.DEFAULT_THRESHOLD, L)
    # bodies by name or index, with weights
    names = list(g._engine.cm.robot.body_names)
    by_name = dataset.find_transitions(g, qd, offs, bodies=[names[0], names[5], names[12]], weights=[1.0, 2.0, 1.0], stride=3, threshold=np.inf)
    by_id = dataset.find_transitions(g, qd, offs, bodies=[0, 5, 12], weights=[0.25, 0.5, 0.25], stride=3, threshold=np.inf)
    assert np.array_equal(_bytes(by_name[1]), _bytes(by_id[1])) and by_name[0] == by_id[0] and all(t.src_frame % 3 == 0 for t in by_id[0])
    # random walks along the transitions compose without an error, and the result is ordinary qpos
    seqs = tr.transition_walks(trans, offs, 4, 3, L, 12, rng=1)
    out, out_offs, T = dataset.compose_clips(g, qd, offs, seqs, blend=L)
    plan = ComposePlan(offs, seqs, L)
    assert out_offs.tolist() == plan.out_offsets.tolist() and tuple(out.shape) == (plan.n_out_frames, g._engine.nq)
    assert bool(torch.isfinite(out).all()) and tuple(T.shape) == (12, 6)
