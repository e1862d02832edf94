"""gmr_motion_compose behind a late producer on a busy stream (tests/stream_order.py has the harness): the entry is outside the 27
stream-taking prototypes -- its stream travels in the struct -- so its case lives here.  One call enqueues two kernels; the second
reads what the first wrote (seg_transform), on the same stream.

Everything the call reads comes in two valid versions behind the same counts: another motion, and another plan of the same
segment lengths and blends whose segments begin elsewhere (seg_src differs; seg_len, seg_blend, seg_out and clip_segs are equal, so
n_seg, n_out and n_out_frames are)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd.compose import ComposePlan, Segment  # noqa: E402
from tests import compose_inputs as ci  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_compose import gpu  # noqa: E402

ROBOT = "unitree_g1"
NAME = "blend8"


def decoy_plan():
    return ComposePlan(ci.OFFS, [[Segment(ci.C64, 1, 63), Segment(ci.C65, 1, 64), Segment(ci.C130, 3, 65), Segment(ci.C130, 0, 130), Segment(ci.C64, 7, 40)],
                                 [Segment(ci.C130, 50, 60), Segment(ci.C63, 4, 30)]], 8)


class ComposeCase(so.Case):
    """The launches of tests/test_gpu_compose.py's case c."""
    entry, launches, h2d = "gmr_motion_compose", 2, 0

    def __init__(self, robot=ROBOT):
        super().__init__()
        self.robot = robot
        eng = engine(robot)
        q, self.plan = ci.case(robot, NAME)
        other = decoy_plan()
        for k in ("seg_len", "seg_blend", "seg_out", "clip_segs"):
            assert np.array_equal(getattr(other, k), getattr(self.plan, k)), k
        assert not np.array_equal(other.seg_src, self.plan.seg_src)
        self.dev_in = {"qpos": (_dev(q), _dev(ci.qpos(robot, 20)))}
        self.dev_in.update({k: (_dev(v), _dev(other.tables()[k])) for k, v in self.plan.tables().items()})
        self.out_spec = {"qpos_out": ((self.plan.n_out_frames, eng.nq), torch.float64), "seg_transform": ((self.plan.n_seg, 6), torch.float64)}

    def new_struct(self):
        from gmr_amd import _native
        return _native.ComposeInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.n_frames, st.n_seg, st.n_out, st.n_out_frames = ci.N, self.plan.n_seg, self.plan.n_out, self.plan.n_out_frames

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_compose(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = ComposeCase()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    assert not so.same(ser["dev_decoy"], ser["true"]), "the decoy answer equals the true one: the case could not tell an ordering error"
    assert so.differing(ser["dev_decoy"], ser["true"]) == ["qpos_out", "seg_transform"]
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


def test_stream_order_behind_a_late_producer():
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the call
    computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case()
    assert case.launches == 2
    assert np.array_equal(ser["true"]["qpos_out"], _bytes(gpu(ROBOT, NAME)[0]).reshape(-1))   # the serial answer is the tests' answer
    assert np.array_equal(ser["true"]["seg_transform"], _bytes(gpu(ROBOT, NAME)[1]).reshape(-1))
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_compose: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
          f"returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not so.same(r["answer"], ser["dev_decoy"])
    assert r["returned_before_producer"]


def test_the_control_on_an_unordered_stream_sees_the_decoy():
    """The same call on a stream that does not wait for the producer reads the decoy inputs: the harness can fail."""
    case, ser, cycles, _ = _stream_case()
    r = so.run_late(case, DEV(), cycles, control=True)
    assert not r["vacuous"]
    if r["overtook_producer"]:
        assert not so.same(r["answer"], ser["true"])
