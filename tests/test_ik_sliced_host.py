"""``gmr_ik_balance_plan`` (include/gmr_amd.h): the pure host choice between the whole-clip and the sliced IK launch, and
``Engine._probe_frames`` following it.  No device is touched."""
import ctypes as C
import types

import numpy as np
import pytest

from gmr_amd import _native
from gmr_amd.build import build_lib
from gmr_amd.schedule import make_items

SLOTS = 2048  # an MI355X: 256 compute units x 8


@pytest.fixture
def plan(monkeypatch):
    build_lib()
    lib = _native.load()
    monkeypatch.delenv("GMR_AMD_BALANCE", raising=False)
    monkeypatch.delenv("GMR_AMD_BALANCE_SLICE", raising=False)

    def go(items, slots=SLOTS):
        items = np.ascontiguousarray(items, dtype=_native.WORK_ITEM_DTYPE)
        return int(lib.gmr_ik_balance_plan(items.ctypes.data_as(C.c_void_p), len(items), slots))
    return go


def _equal(n, T):
    return make_items(np.arange(n + 1, dtype=np.int64) * T)


def test_forced_plan_and_overrides(plan, monkeypatch):
    items = _equal(8192, 3000)
    monkeypatch.setenv("GMR_AMD_BALANCE", "1")
    default = plan(items)
    assert default >= 32  # (tests/test_gpu_ik_shapes.py relies on 2080 x 64 frames staying a whole-clip launch: 64 < 4 slices)
    assert plan(_equal(3, 10)) == default  # forced: any plain batch
    monkeypatch.setenv("GMR_AMD_BALANCE_SLICE", "48")
    assert plan(items) == 48 and plan(_equal(3, 10)) == 48
    monkeypatch.setenv("GMR_AMD_BALANCE", "0")
    assert plan(items) == 0
    monkeypatch.delenv("GMR_AMD_BALANCE")
    assert plan(items) in (0, 48)  # the default follows the measured gain; the override sets the length only


def test_not_plain_is_never_sliced(plan, monkeypatch):
    monkeypatch.setenv("GMR_AMD_BALANCE", "1")
    items = _equal(8192, 3000)
    assert plan(items) > 0
    walk = items.copy()
    walk["check_stride"][5], walk["burn_row"][5], walk["final_row"][5] = 100, 0, 1
    assert plan(walk) == 0
    burn = items.copy()
    burn["n_burn"][7], burn["n_out"][7] = 16, 2984
    assert plan(burn) == 0
    chunk_start = items.copy()
    chunk_start["init_row"][9] = _native.INIT_ROOT_TARGET
    assert plan(chunk_start) == 0
    assert plan(items[:0]) == 0


def test_where_slicing_pays(plan, monkeypatch):
    """The automatic rule, with the slice length pinned so that the answers do not depend on the shipped default."""
    monkeypatch.setenv("GMR_AMD_BALANCE", "1")
    monkeypatch.setenv("GMR_AMD_BALANCE_SLICE", "64")
    assert plan(_equal(SLOTS, 3000)) == 64  # forced ignores the rule ...
    monkeypatch.setenv("GMR_AMD_BALANCE", "2")      # ... this is the rule, whether or not it is the build's default
    assert plan(_equal(8192, 3000)) == 64
    assert plan(_equal(SLOTS, 3000)) == 0          # too few items: one per wavefront slot
    assert plan(_equal(SLOTS + 1, 3000)) == 64
    assert plan(_equal(8192, 255)) == 0            # mean length under four slices
    assert plan(_equal(8192, 256)) == 64
    rng = np.random.default_rng(0)
    wide = make_items(np.concatenate([[0], np.cumsum(rng.integers(1000, 5001, size=8192))]).astype(np.int64))
    assert plan(wide) == 0                         # lengths U(T/3, 5T/3): far over the band
    ln = np.full(8192, 3000)
    ln[::2] += 500                                 # std 250 = 7.7 % of the mean: inside
    assert plan(make_items(np.concatenate([[0], np.cumsum(ln)]).astype(np.int64))) == 64
    ln[::2] += 300                                 # std 400 = 11.8 %: outside
    assert plan(make_items(np.concatenate([[0], np.cumsum(ln)]).astype(np.int64))) == 0


def test_probe_frames_follows_the_plan(plan, monkeypatch):
    torch = pytest.importorskip("torch")
    from gmr_amd.engine import Engine
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=SLOTS // 8))
    eng = Engine.__new__(Engine)
    eng._h, eng._lib, eng.device = None, _native.load(), "cuda:0"
    items, short = _equal(8192, 3000), _equal(8192, 100)
    monkeypatch.setenv("GMR_AMD_BALANCE", "0")
    assert eng.balance_plan(items, SLOTS) == 0
    assert eng._probe_frames(items) == Engine.PROBE_FRAMES and eng._order_pays(items)
    assert eng._probe_frames(short) == Engine.PROBE_FRAMES_SHORT
    monkeypatch.setenv("GMR_AMD_BALANCE", "1")
    monkeypatch.setenv("GMR_AMD_BALANCE_SLICE", "64")
    assert eng.balance_plan(items, SLOTS) == 64
    assert eng._probe_frames(items) == 0 and not eng._order_pays(items)  # sliced: nothing to probe
    assert eng._probe_frames(short) == 0
    walk = items.copy()
    walk["check_stride"][:], walk["burn_row"][:], walk["final_row"][:] = 100, 0, 1
    assert eng._probe_frames(walk) == 0  # (walks are never probed either)
    assert Engine.PROBE_MAX_LENGTH_SPREAD == 0.10  # the band gmr_ik_balance_plan uses for "equal lengths"


def test_group_launches_keep_their_probe(plan, monkeypatch):
    """A group launch never slices (gmr_group_ik_solve runs whole clips), so its "auto" order must not follow the balance plan: the
    members' items together are probed as before, whatever the plan says about them."""
    torch = pytest.importorskip("torch")
    from gmr_amd import engine
    from gmr_amd.engine import Engine
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=SLOTS // 8))
    eng = Engine.__new__(Engine)
    eng._h, eng._lib, eng.device = None, _native.load(), "cuda:0"
    monkeypatch.setenv("GMR_AMD_BALANCE", "1")
    members = [_equal(4096, 3000), _equal(4096, 3000)]
    both = np.concatenate(members)
    assert eng.balance_plan(both, SLOTS) > 0
    assert eng._probe_frames(both, sliced=False) == Engine.PROBE_FRAMES and eng._probe_frames(both) == 0
    asked = []
    plan_order = lambda pf: asked.append(pf)  # noqa: E731  (returns None: no order tensor to check without a device)
    assert engine._launch_order(eng, "auto", members, plan_order) is None and asked == [Engine.PROBE_FRAMES]  # what EngineGroup.ik_solve calls
    asked.clear()
    assert engine._launch_order(eng, "auto", [both], plan_order, sliced=True) is None and asked == []  # what Engine.ik_solve calls
