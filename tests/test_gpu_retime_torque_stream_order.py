"""gmr_motion_retime_plan_torque and gmr_motion_retime_apply with interp = 1 behind a late producer on a busy stream
(tests/stream_order.py has the harness): like the velocity pair's, the stream travels in the struct, so the cases live here.  The plan
enqueues four kernels, each reading what the one before wrote (need, ticks, cum and the clip totals), on the same stream; the apply
one.

Everything a call reads comes in two valid versions behind the same counts.  Plan: other torques, other limits and another floor.
Apply: another motion and another plan of the same clips -- every clip's ticks in reverse order, so that every total and with them
out_offsets are the same."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import retime_inputs as ri  # noqa: E402
from tests import retime_torque_inputs as ti  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_retime_stream_order import NAME, reversed_plan  # noqa: E402
from tests.test_gpu_retime_torque import KEYS, gpu_plan  # noqa: E402

ROBOT = "unitree_g1"
F64, I64, I32 = torch.float64, torch.int64, torch.int32


class RetimeTorqueCase(so.Case):
    entry, launches, h2d = "gmr_motion_retime_plan_torque", 4, 0

    def __init__(self, robot=ROBOT, layout="lens"):
        super().__init__()
        self.robot, self.layout = robot, layout
        self.c = c = ti.case(robot, layout, True, True)
        n, s = c.tau.shape[0], len(c.offs) - 1
        rng = np.random.default_rng(11)
        tau2, g2 = np.ascontiguousarray(c.tau[::-1]), np.ascontiguousarray(c.tau_static[::-1])   # the same torques in other rows
        lim2 = np.where(np.isfinite(c.limit), 0.8 * c.limit, np.inf)
        self.dev_in = {"tau": (_dev(c.tau), _dev(tau2)), "tau_static": (_dev(c.tau_static), _dev(g2)), "seq_offsets": (_dev(c.offs), _dev(c.offs)),
                       "torque_limit": (_dev(c.limit), _dev(lim2)), "need_floor": (_dev(c.floor), _dev(rng.uniform(0.0, 2.5, n)))}
        self.out_spec = {"need": ((n,), F64), "ticks": ((n,), I64), "cum": ((n,), I64), "out_len": ((s,), I64), "clip_stats": ((s, 4), I64),
                         "need_max": ((s,), F64), "static_over": ((n,), I32)}

    def new_struct(self):
        from gmr_amd import _native
        return _native.RetimeTorqueInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        c = self.c
        st.n_frames, st.n_seq, st.window, st.limit_scale, st.max_stretch, st.align_end = c.tau.shape[0], len(c.offs) - 1, c.window, c.scale, c.max_stretch, 1

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_retime_plan_torque(eng._h, C.byref(st))


class RetimeCubicCase(so.Case):
    entry, launches, h2d = "gmr_motion_retime_apply", 1, 0

    def __init__(self, robot=ROBOT):
        super().__init__()
        self.robot = robot
        self.c = c = ri.case(robot, NAME)
        p, _, _, oo, _ = ri.reference(robot, NAME)
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
        st.n_frames, st.n_seq, st.n_out_frames, st.interp = self.c.q.shape[0], len(self.c.offs) - 1, int(self.oo[-1]), 1

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_retime_apply(eng._h, C.byref(st))


CASES = {"plan_torque": RetimeTorqueCase, "apply_cubic": RetimeCubicCase}


@functools.lru_cache(maxsize=None)
def _stream_case(which):
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = CASES[which]()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    assert not so.same(ser["dev_decoy"], ser["true"]), "the decoy answer equals the true one: the case could not tell an ordering error"
    want = list(KEYS) if which == "plan_torque" else ["qpos_out", "src_time"]
    assert which == "plan_torque" or case.decoy_plan_differs
    assert so.differing(ser["dev_decoy"], ser["true"]) == want
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


@pytest.mark.parametrize("which", sorted(CASES))
def test_stream_order_behind_a_late_producer(which):
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the call
    computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case(which)
    if which == "plan_torque":                                                              # the serial answer is the tests' answer
        base = gpu_plan(ROBOT, "lens", True, True)
        assert all(np.array_equal(ser["true"][k], _bytes(base[k]).reshape(-1)) for k in KEYS)
    r = so.run_late(case, DEV(), cycles)
    print(f"{case.entry} ({which}): serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
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
