"""The shaped IK kernel instance against the generic one: the same arithmetic with the model's counts compiled in,
so every result is required to be bit-identical, and every launch a shape does not cover must take the generic instance.

Which instance a launch took is read from the ``GMR_DEBUG_PLAN`` line the library writes to stderr per IK launch;
``GMR_AMD_GENERIC_SHAPE`` is read at model creation, hence a fresh Engine per setting.
"""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd._native import INIT_ROOT_TARGET  # noqa: E402
from gmr_amd.engine import Engine, IKParams  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from tests.util import compiled  # noqa: E402

SHAPED = "IkShapeG1Smplx"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture
def run(monkeypatch, capfd, dev):
    """run(cm, generic_shape, fn) -> (fn(engine)'s result, [(kind, instance) of every IK launch it made])."""
    monkeypatch.setenv("GMR_DEBUG_PLAN", "1")

    def go(cm, generic_shape, fn):
        monkeypatch.setenv("GMR_AMD_GENERIC_SHAPE", "1" if generic_shape else "0")
        eng = Engine(cm, 0)
        capfd.readouterr()
        res = fn(eng)
        torch.cuda.synchronize()
        launches = re.findall(r"gmr: ik launch: (\w+) instance (\w+)", capfd.readouterr().err)
        eng.close()
        return res, launches
    return go


def _clips(cm, dev, n_each, T, dtype=np.float32, tile=1):
    """n_each easy and n_each hard synthetic clips of T frames (the existing tests' generator), the set repeated `tile` times."""
    pe, qe, names, _, _ = synth.synth_clips(cm, n_each, T, seed=21, hard=False, dtype=dtype)
    ph, qh, names_h, _, _ = synth.synth_clips(cm, n_each, T, seed=22, hard=True, dtype=dtype)
    assert names == names_h
    pos, quat = np.tile(np.concatenate([pe, ph]), (tile, 1, 1)), np.tile(np.concatenate([qe, qh]), (tile, 1, 1))
    offs = np.arange(2 * n_each * tile + 1, dtype=np.int64) * T
    return torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev), cm.slot_columns(names), offs


def _same(a, b):
    (qa, ia, _), (qb, ib, _) = a, b
    assert not torch.isnan(qa).any()
    assert torch.equal(qa, qb) and torch.equal(ia, ib)


def test_plain_call_is_bit_identical(run, dev):
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = _clips(cm, dev, 3, 40)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, make_items(offs), launch_order=None)  # noqa: E731
    shaped, how_s = run(cm, False, solve)
    generic, how_g = run(cm, True, solve)
    assert how_s == [("solve", SHAPED)] and how_g == [("solve", "generic")]
    _same(shaped, generic)
    assert int((shaped[1] & 0x3fffffff).max()) > 2  # the hard clips iterate: not a trivial comparison


def test_more_items_than_wavefront_slots_and_auto_order_are_bit_identical(run, dev):
    """2080 items (> 2048 slots: LDS, registers and plans of a slot are reused by a second item), in array order and with
    launch_order="auto" (probe + device sort + ordered launch).  The order the shaped probe plans must be the one its costs imply:
    an item's probe cost is the number of solves of its first frames, which the solve itself reports (and which is compared bit
    for bit above), so the buckets of plan_order_kernel can be recomputed here."""
    cm = compiled("smplx", "unitree_g1")
    T = 64
    pos, quat, sc, offs = _clips(cm, dev, 8, T, tile=130)
    items = make_items(offs)
    assert len(items) == 2080
    plain = lambda eng: eng.ik_solve(pos, quat, sc, items, launch_order=None)  # noqa: E731

    def auto(eng):
        pf = eng._probe_frames(items)
        assert pf > 0  # "auto" does probe this batch
        return eng.ik_solve(pos, quat, sc, items, launch_order="auto") + (eng.plan_order(pos, quat, sc, items, probe_frames=pf), pf)

    s_plain, how = run(cm, False, plain)
    assert how == [("solve", SHAPED)]
    g_plain, how = run(cm, True, plain)
    assert how == [("solve", "generic")]
    _same(s_plain, g_plain)
    for generic_shape in (False, True):
        (q, it, qf, order, pf), how = run(cm, generic_shape, auto)
        name = "generic" if generic_shape else SHAPED
        assert how == [("probe", name), ("solve", name), ("probe", name)]
        _same((q, it, qf), g_plain)
        order = order.cpu().numpy()
        assert np.array_equal(np.sort(order), np.arange(len(items)))
        cost = (it.cpu().numpy() & 0x3fffffff).reshape(len(items), T)[:, :pf].sum(1)
        key = cost.astype(np.float32) * np.float32(T) / np.float32(pf)
        scale = np.float32(4095.0) / key.max()
        bucket = 4095 - np.minimum(4095, (key * scale).astype(np.int32))
        assert np.all(np.diff(bucket[order]) >= 0)  # most expensive first, by the probe's own buckets


def _generic_only(how):
    assert len(how) > 0 and all(inst == "generic" for _, inst in how), how


def test_float64_keypoints_fall_through(run, dev):
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = _clips(cm, dev, 2, 30, dtype=np.float64)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, make_items(offs), launch_order=None)  # noqa: E731
    a, how = run(cm, False, solve)
    _generic_only(how)
    _same(a, run(cm, True, solve)[0])


def test_offset_to_ground_falls_through(run, dev):
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = _clips(cm, dev, 2, 30)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, make_items(offs), params=IKParams(offset_to_ground=1), launch_order=None)  # noqa: E731
    a, how = run(cm, False, solve)
    _generic_only(how)
    _same(a, run(cm, True, solve)[0])


def test_chunked_call_falls_through(run, dev):
    """ik_solve_chunked: speculative chunk starts in the first launch, verification walks in the second."""
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = _clips(cm, dev, 2, 96)
    solve = lambda eng: eng.ik_solve_chunked(pos, quat, sc, offs, chunk=32, burn_in=8)  # noqa: E731
    (q, it, info), how = run(cm, False, solve)
    assert len(how) == 2
    _generic_only(how)
    (q2, it2, _), _ = run(cm, True, solve)
    assert torch.equal(q, q2) and torch.equal(it, it2)


def test_root_target_clip_start_falls_through(run, dev):
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = _clips(cm, dev, 2, 30)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, make_items(offs, clip_init=INIT_ROOT_TARGET), launch_order=None)  # noqa: E731
    a, how = run(cm, False, solve)
    _generic_only(how)
    _same(a, run(cm, True, solve)[0])


def test_a_robot_with_another_shape_falls_through(run, dev):
    cm = compiled("smplx", "booster_t1")
    pos, quat, sc, offs = _clips(cm, dev, 2, 30)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, make_items(offs), launch_order=None)  # noqa: E731
    a, how = run(cm, False, solve)
    _generic_only(how)
    _same(a, run(cm, True, solve)[0])


def test_generic_qp_falls_through(run, dev, monkeypatch):
    monkeypatch.setenv("GMR_AMD_GENERIC_QP", "1")
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = _clips(cm, dev, 2, 30)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, make_items(offs), launch_order=None)  # noqa: E731

    def checked(eng):
        assert eng.info.reserved[0] == 0  # the dense generic QP
        return solve(eng)
    a, how = run(cm, False, checked)
    _generic_only(how)
