"""The tapered schedule of the sliced IK launch (gmr_amd/csrc/slice_plan.h, DESIGN 4.2 "Slices") against the whole-clip launch of
the same call, in the pattern of tests/test_gpu_ik_sliced.py, whose clips and whole-clip references these tests share: every
comparison is bitwise (``torch.equal``) on qpos, the solve words, ``qpos_final`` and ``frames_done``, and no wavefront may have hit
its poll cap.  ``GMR_AMD_BALANCE_TAPER`` is read per call like the other two variables; the schedule a call ran is read from the
``GMR_DEBUG_PLAN`` line (ticket count, taper slice lengths) and set against what slice_plan.h gives on the host.
"""
import re
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_gpu_ik_sliced import SHAPED, _setup, _whole  # noqa: E402
from tests.test_ik_slice_plan_host import build_slice_plan_host, slice_lengths  # noqa: E402

L = 16
_host = {}


def host_schedule(T, slice_len, floor):
    """The slice lengths slice_plan.h gives on the host (tests/slice_plan_host.cpp, built once, without sanitizers)."""
    if "exe" not in _host:
        _host["dir"] = tempfile.TemporaryDirectory()
        _host["exe"] = build_slice_plan_host(_host["dir"].name, sanitize=False)
    if _host["exe"] is None:
        pytest.fail("the host schedule needs a C++ compiler")
    return slice_lengths(_host["exe"], T, slice_len, floor)


LINE = re.compile(r"gmr: ik launch: sliced instance (\w+), slice (\d+) frames, (\d+) tickets for (\d+) items(?:, taper((?: \d+)+)|, no taper)\n")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


def _solve(s, monkeypatch, capfd, floor):
    """(qpos, iters, qpos_final, frames_done), (instance, tickets, [taper slice lengths]) of the one sliced launch"""
    monkeypatch.setenv("GMR_DEBUG_PLAN", "1")
    monkeypatch.setenv("GMR_AMD_BALANCE", "1")
    monkeypatch.setenv("GMR_AMD_BALANCE_SLICE", str(L))
    if floor is None:
        monkeypatch.delenv("GMR_AMD_BALANCE_TAPER", raising=False)
    else:
        monkeypatch.setenv("GMR_AMD_BALANCE_TAPER", str(floor))
    n = len(s["items"])
    fd = torch.full((n,), -1, dtype=torch.int32, device=s["pos"].device)
    capfd.readouterr()
    q, it, qf = s["eng"].ik_solve(s["pos"], s["quat"], s["sc"], s["items"], n_final=n, frames_done=fd, launch_order=None)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert s["eng"].sliced_timeouts == 0
    lines = LINE.findall(err)
    assert len(lines) == 1 and "gmr: ik launch: solve" not in err, err
    name, slice_len, tickets, items, taper = lines[0]
    assert int(slice_len) == L and int(items) == n
    return (q, it, qf, fd), (name, int(tickets), [int(v) for v in taper.split()])


def _check(s, monkeypatch, capfd, name, floor, slices):
    """One tapered call: the result of the whole-clip launch, and the schedule `slices` (None: whatever slice_plan.h makes)."""
    ref = _whole(s, monkeypatch, capfd, name)
    res, (how, tickets, taper) = _solve(s, monkeypatch, capfd, floor)
    assert how == name
    for a, b, what in zip(res, ref, ("qpos", "iters", "qpos_final", "frames_done")):
        assert torch.equal(a, b), what
    n, T = len(s["items"]), int(s["items"]["n_out"].max())
    host = host_schedule(T, L, floor)
    assert slices is None or host == slices
    assert tickets == n * len(host)
    n_taper = len(taper)
    assert n_taper >= 2 and taper == host[-n_taper:] and sum(taper) == L  # a tapered call: the last L frames, as the host cuts them


@pytest.mark.parametrize("floor,slices", [(1, [16, 13, 8, 4, 2, 1, 1]), (4, [16, 13, 8, 4, 4])])
def test_hand_over_through_the_taper(dev, monkeypatch, capfd, floor, slices):
    """12 clips x 45 frames, half of them hard.  Floor 1: hand-overs after slices of 2 and 1 frames, shorter than a target block."""
    s = _setup(dev, "unitree_g1", [45] * 12, np.float32)
    _check(s, monkeypatch, capfd, SHAPED, floor, slices)


def test_ragged_lengths_end_in_different_taper_rounds(dev, monkeypatch, capfd):
    """Lengths 40 .. 44, slices 16 12 8 4 2 2: the clips end in the 4-frame slice (40), the first 2-frame slice (41, 42) and the last
    (43, 44); the later tickets of the shorter clips leave at once."""
    lengths = [40, 41, 42, 43, 44, 44, 43, 42, 41, 40]
    s = _setup(dev, "unitree_g1", lengths, np.float32)
    _check(s, monkeypatch, capfd, SHAPED, 2, [16, 12, 8, 4, 2, 2])


def test_wait_path_through_the_taper_rounds(dev, monkeypatch, capfd):
    """2 clips x 40 frames, slices 16 8 8 4 2 2: all twelve tickets are resident at once, so every taper slice waits for the one
    before it while that one still runs.  (A broken wait ends at the poll cap and fails the call.)"""
    s = _setup(dev, "unitree_g1", [40, 40], np.float32)
    _check(s, monkeypatch, capfd, SHAPED, 2, [16, 8, 8, 4, 2, 2])


def test_empty_items(dev, monkeypatch, capfd):
    s = _setup(dev, "unitree_g1", [30, 0, 30, 29, 0, 31], np.float32)
    _check(s, monkeypatch, capfd, SHAPED, 2, [15, 8, 4, 2, 2])


def test_generic_instance(dev, monkeypatch, capfd):
    """booster_t1, float64 key-points: the generic instance.  6 x 33 frames: slices 16 1 8 4 2 2."""
    s = _setup(dev, "booster_t1", [33] * 6, np.float64)
    _check(s, monkeypatch, capfd, "generic", 2, [16, 1, 8, 4, 2, 2])


def test_dense_qp_instance(dev, monkeypatch, capfd):
    """GMR_AMD_GENERIC_QP=1: the hand-over carries the dense QP's `status`."""
    s = _setup(dev, "unitree_g1", [33] * 6, np.float32, monkeypatch, generic_qp=True)
    assert s["eng"].info.reserved[0] == 0
    _check(s, monkeypatch, capfd, "generic", 2, [16, 1, 8, 4, 2, 2])


@pytest.mark.parametrize("floor", [0, 9, 16, 40])
def test_taper_off_is_the_fixed_length_grid(dev, monkeypatch, capfd, floor):
    """GMR_AMD_BALANCE_TAPER=0, a floor above ceil(L / 2) and floors >= L: n_items x ceil(T / L) tickets, no taper, same result."""
    s = _setup(dev, "unitree_g1", [45] * 12, np.float32)
    ref = _whole(s, monkeypatch, capfd, SHAPED)
    res, (how, tickets, taper) = _solve(s, monkeypatch, capfd, floor)
    assert how == SHAPED and taper == [] and tickets == 12 * 3
    assert host_schedule(45, L, floor) == [16, 16, 13]
    for a, b, what in zip(res, ref, ("qpos", "iters", "qpos_final", "frames_done")):
        assert torch.equal(a, b), what
