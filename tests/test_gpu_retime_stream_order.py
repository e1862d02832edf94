"""gmr_motion_retime_plan and gmr_motion_retime_apply behind a late producer on a busy stream (tests/stream_order.py has the
harness): the entries are outside the 27 stream-taking prototypes -- their stream travels in the struct -- so their cases live here.
The plan enqueues three kernels, each reading what the one before wrote (need, ticks), on the same stream; the apply one.

Everything a call reads comes in two valid versions behind the same counts.  Plan: another motion and other limits.  Apply: another
motion and another plan of the same clips -- every clip's ticks in reverse order, so that every total, every out_len and with them
out_offsets are the same."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import retime_inputs as ri  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_retime import PLAN_KEYS, gpu  # noqa: E402

ROBOT = "unitree_g1"
NAME = "wide"          # the widest window: the ticks kernel reads 64 intervals beyond its tile on either side, clamped at the clips' ends
F64, I64 = torch.float64, torch.int64


def reversed_plan(ticks, offs):
    """(ticks, cum) with every clip's intervals in reverse order: the same totals."""
    t2, c2 = ticks.copy(), np.zeros_like(ticks)
    for a, b in zip(offs[:-1], offs[1:]):
        if b - a > 1:
            t2[a:b - 1] = ticks[a:b - 1][::-1]
        if b > a:
            c2[a:b] = np.concatenate([[0], np.cumsum(t2[a:b - 1])])
    return t2, c2


class RetimePlanCase(so.Case):
    entry, launches, h2d = "gmr_motion_retime_plan", 3, 0

    def __init__(self, robot=ROBOT):
        super().__init__()
        self.robot = robot
        self.c = c = ri.case(robot, NAME)
        other = ri.case(robot, "columns").vmax
        n, s = c.q.shape[0], len(c.offs) - 1
        self.dev_in = {"qpos": (_dev(c.q), _dev(ri.qpos(robot, 20))), "seq_offsets": (_dev(c.offs), _dev(c.offs)), "vmax": (_dev(c.vmax), _dev(other))}
        self.out_spec = {"need": ((n,), F64), "ticks": ((n,), I64), "cum": ((n,), I64), "out_len": ((s,), I64), "clip_stats": ((s, 4), I64),
                         "need_max": ((s,), F64)}

    def new_struct(self):
        from gmr_amd import _native
        return _native.RetimePlanInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        c = self.c
        st.n_frames, st.n_seq, st.window, st.fps, st.max_stretch = c.q.shape[0], len(c.offs) - 1, c.window, c.fps, c.max_stretch

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_retime_plan(eng._h, C.byref(st))


class RetimeApplyCase(so.Case):
    entry, launches, h2d = "gmr_motion_retime_apply", 1, 0

    def __init__(self, robot=ROBOT):
        super().__init__()
        self.robot = robot
        self.c = c = ri.case(robot, NAME)
        p, _, _, oo = gpu(robot, NAME)
        t2, c2 = reversed_plan(p["ticks"], c.offs)
        assert all(c2[b - 1] == p["cum"][b - 1] for a, b in zip(c.offs[:-1], c.offs[1:]) if b > a)    # the same totals: the same out_offsets
        self.decoy_plan_differs = not np.array_equal(t2, p["ticks"])
        self.oo = oo
        self.dev_in = {"qpos": (_dev(c.q), _dev(ri.qpos(robot, 20))), "seq_offsets": (_dev(c.offs), _dev(c.offs)),
                       "ticks": (_dev(p["ticks"]), _dev(t2)), "cum": (_dev(p["cum"]), _dev(c2)), "out_offsets": (_dev(oo), _dev(oo))}
        self.out_spec = {"qpos_out": ((int(oo[-1]), c.q.shape[1]), F64), "src_time": ((int(oo[-1]),), F64)}

    def new_struct(self):
        from gmr_amd import _native
        return _native.RetimeApplyInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.n_frames, st.n_seq, st.n_out_frames = self.c.q.shape[0], len(self.c.offs) - 1, int(self.oo[-1])

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_retime_apply(eng._h, C.byref(st))


CASES = {"plan": RetimePlanCase, "apply": RetimeApplyCase}


@functools.lru_cache(maxsize=None)
def _stream_case(which):
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = CASES[which]()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    assert not so.same(ser["dev_decoy"], ser["true"]), "the decoy answer equals the true one: the case could not tell an ordering error"
    want = ["need", "ticks", "cum", "out_len", "clip_stats", "need_max"] if which == "plan" else ["qpos_out", "src_time"]
    assert which == "plan" or case.decoy_plan_differs
    assert so.differing(ser["dev_decoy"], ser["true"]) == want
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


@pytest.mark.parametrize("which", sorted(CASES))
def test_stream_order_behind_a_late_producer(which):
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the call
    computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case(which)
    base = gpu(ROBOT, NAME)
    if which == "plan":                                                                     # the serial answer is the tests' answer
        assert all(np.array_equal(ser["true"][k], _bytes(base[0][k]).reshape(-1)) for k in PLAN_KEYS)
    else:
        assert np.array_equal(ser["true"]["qpos_out"], _bytes(base[1]).reshape(-1)) and np.array_equal(ser["true"]["src_time"], _bytes(base[2]).reshape(-1))
    r = so.run_late(case, DEV(), cycles)
    print(f"{case.entry}: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
          f"returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not so.same(r["answer"], ser["dev_decoy"])
    assert r["returned_before_producer"]


@pytest.mark.parametrize("which", sorted(CASES))
def test_the_control_on_an_unordered_stream_sees_the_decoy(which):
    """The same call on a stream that does not wait for the producer reads the decoy inputs: the harness can fail."""
    case, ser, cycles, _ = _stream_case(which)
    r = so.run_late(case, DEV(), cycles, control=True)
    assert not r["vacuous"]
    if r["overtook_producer"]:
        assert not so.same(r["answer"], ser["true"])
