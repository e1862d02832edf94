"""The sliced IK launch (DESIGN 4.2 "Slices", ``ik_kernel_sliced``) against the whole-clip launch of the same call: a clip cut into
slices, the solver state handed from one wavefront to the next, must produce what one wavefront running the clip from start to end
produces -- every comparison here is bitwise (``torch.equal``) on qpos, the solve words, ``frames_done`` and ``qpos_final``.

``GMR_AMD_BALANCE`` / ``GMR_AMD_BALANCE_SLICE`` are read per call, so one Engine serves both sides; which kernel a call took is read
from the ``GMR_DEBUG_PLAN`` line the library writes per IK launch.  Half of the clips are ``hard=True``: their QPs end with active
bounds, so the hand-over of the working set is exercised at the boundaries.
"""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native, synth  # noqa: E402
from gmr_amd.engine import Engine  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from tests.util import compiled  # noqa: E402

SHAPED = "IkShapeG1Smplx"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


_cache = {}


def _setup(dev, robot, lengths, dtype, monkeypatch=None, generic_qp=False):
    """Engine, clips (half easy, half hard, cut to `lengths`; 0 = an empty item) and the whole-clip result of the call, made once per
    configuration and left unchanged.  generic_qp: an Engine built under GMR_AMD_GENERIC_QP=1 (read at model creation)."""
    key = (robot, tuple(lengths), np.dtype(dtype).name, generic_qp)
    if key not in _cache:
        if generic_qp:
            monkeypatch.setenv("GMR_AMD_GENERIC_QP", "1")
        cm = compiled("smplx", robot)
        n, T = len(lengths), max(lengths)
        pe, qe, names, _, _ = synth.synth_clips(cm, n - n // 2, T, seed=31, hard=False, dtype=dtype)
        ph, qh, names_h, _, _ = synth.synth_clips(cm, n // 2, T, seed=32, hard=True, dtype=dtype)
        assert names == names_h
        pos, quat = np.concatenate([pe, ph]), np.concatenate([qe, qh])
        keep = np.concatenate([np.arange(c * T, c * T + ln) for c, ln in enumerate(lengths)])  # clip c: its first lengths[c] frames
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        items = np.zeros(n, dtype=_native.WORK_ITEM_DTYPE)  # (by hand: make_items leaves empty clips out)
        items["frame_begin"], items["n_out"], items["init_row"], items["burn_row"], items["height_scale"] = offs[:-1], lengths, -1, -1, 1.0
        items["final_row"] = np.arange(n)
        assert np.array_equal(items[np.asarray(lengths) > 0], _with_final(make_items(offs), np.flatnonzero(np.asarray(lengths) > 0)))
        _cache[key] = dict(cm=cm, eng=Engine(cm, 0), pos=torch.from_numpy(pos[keep]).to(dev), quat=torch.from_numpy(quat[keep]).to(dev),
                           sc=cm.slot_columns(names), items=items, ref={})
    return _cache[key]


def _with_final(items, rows):
    items["final_row"] = rows
    return items


def _solve(s, monkeypatch, capfd, balance, slice_len=None, qpos_init=None):
    """(qpos, iters, qpos_final, frames_done), [(kind, instance) of every IK launch]"""
    monkeypatch.setenv("GMR_DEBUG_PLAN", "1")
    monkeypatch.setenv("GMR_AMD_BALANCE", balance)
    if slice_len is None:
        monkeypatch.delenv("GMR_AMD_BALANCE_SLICE", raising=False)
    else:
        monkeypatch.setenv("GMR_AMD_BALANCE_SLICE", str(slice_len))
    n = len(s["items"])
    fd = torch.full((n,), -1, dtype=torch.int32, device=s["pos"].device)
    capfd.readouterr()
    q, it, qf = s["eng"].ik_solve(s["pos"], s["quat"], s["sc"], s["items"], qpos_init=qpos_init, n_final=n, frames_done=fd, launch_order=None)
    torch.cuda.synchronize()
    how = re.findall(r"gmr: ik launch: (\w+) instance (\w+)", capfd.readouterr().err)
    assert s["eng"].sliced_timeouts == 0
    return (q, it, qf, fd), how


def _whole(s, monkeypatch, capfd, name, qpos_init=None, tag="plain"):
    if tag not in s["ref"]:
        res, how = _solve(s, monkeypatch, capfd, "0", qpos_init=qpos_init)
        assert how == [("solve", name)]
        q, it, qf, fd = res
        assert not torch.isnan(q).any() and not torch.isnan(qf).any()
        assert np.array_equal(fd.cpu().numpy(), s["items"]["n_out"])
        assert int((it & 0x3fffffff).max()) > 2  # the hard clips iterate: not a trivial comparison
        s["ref"][tag] = res
    return s["ref"][tag]


def _check(s, monkeypatch, capfd, name, slice_len, qpos_init=None, tag="plain"):
    ref = _whole(s, monkeypatch, capfd, name, qpos_init, tag)
    res, how = _solve(s, monkeypatch, capfd, "1", slice_len, qpos_init)
    assert how == [("sliced", name)]
    for a, b, what in zip(res, ref, ("qpos", "iters", "qpos_final", "frames_done")):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("slice_len", [1, 7, 64])
def test_hand_over_at_every_boundary(dev, monkeypatch, capfd, slice_len):
    """12 clips x 45 frames.  Slice 1: every frame is a hand-over; 7: a ragged 3-frame last slice; 64: one slice per clip."""
    s = _setup(dev, "unitree_g1", [45] * 12, np.float32)
    _check(s, monkeypatch, capfd, SHAPED, slice_len)


def test_wait_path_with_fewer_clips_than_wavefronts(dev, monkeypatch, capfd):
    """2 clips x 20 frames, slice 4: all ten tickets are drawn at once, so slice r waits while slice r - 1 of its clip still runs
    -- the one shape in which a wrong flag or fence order shows.  (A broken wait ends at the poll cap and fails the comparison.)"""
    s = _setup(dev, "unitree_g1", [20, 20], np.float32)
    _check(s, monkeypatch, capfd, SHAPED, 4)


def test_ragged_lengths_inside_the_band(dev, monkeypatch, capfd):
    """Lengths 40 .. 44, slice 7: the longest clip sets the rounds (7), tickets past a shorter clip's end (40, 41, 42: six slices) are
    no-ops, and the last slices are 5, 6, 7, 1 and 2 frames long."""
    lengths = [40, 41, 42, 43, 44, 44, 43, 42, 41, 40]
    s = _setup(dev, "unitree_g1", lengths, np.float32)
    ln = np.asarray(lengths, dtype=np.float64)
    assert ln.std() <= Engine.PROBE_MAX_LENGTH_SPREAD * ln.mean()
    _check(s, monkeypatch, capfd, SHAPED, 7)


def test_empty_items_report_as_in_the_whole_clip_launch(dev, monkeypatch, capfd):
    """Items of no frames among the clips: slice 0 of an empty item still writes frames_done = 0 and its start state to qpos_final,
    as the whole-clip kernel does (the reference asserts both in _whole)."""
    s = _setup(dev, "unitree_g1", [30, 0, 30, 29, 0, 31], np.float32)
    _check(s, monkeypatch, capfd, SHAPED, 7)


def test_dense_qp_instance(dev, monkeypatch, capfd):
    """GMR_AMD_GENERIC_QP=1: ik_kernel_sliced<NVP, false>, whose hand-over carries the dense QP's `status` instead of `sq_status`."""
    s = _setup(dev, "unitree_g1", [33] * 6, np.float32, monkeypatch, generic_qp=True)
    assert s["eng"].info.reserved[0] == 0  # the dense generic QP
    _check(s, monkeypatch, capfd, "generic", 5)


def test_generic_instance(dev, monkeypatch, capfd):
    """Another registry robot, float64 key-points: ik_kernel_sliced's generic instance."""
    s = _setup(dev, "booster_t1", [33] * 6, np.float64)
    _check(s, monkeypatch, capfd, "generic", 5)


def test_caller_supplied_start(dev, monkeypatch, capfd):
    """qpos_init for slice 0: every clip starts from its own row (a perturbed qpos0), later slices from the records."""
    s = _setup(dev, "unitree_g1", [45] * 12, np.float32)
    rng = np.random.default_rng(5)
    q0 = np.tile(np.asarray(s["cm"].robot.qpos0, dtype=np.float64), (12, 1))
    q0[:, 7:] += rng.uniform(-0.05, 0.05, size=q0[:, 7:].shape)
    q0[:, :2] += rng.uniform(-0.2, 0.2, size=(12, 2))
    items = s["items"].copy()
    items["init_row"] = np.arange(12)
    s2 = dict(s, items=items, ref=s["ref"])
    qi = torch.from_numpy(q0).to(dev)
    _check(s2, monkeypatch, capfd, SHAPED, 7, qpos_init=qi, tag="init")
    assert not torch.equal(s["ref"]["init"][0], _whole(s, monkeypatch, capfd, SHAPED)[0])  # the start rows were used
