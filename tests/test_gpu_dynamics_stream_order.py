"""gmr_motion_dynamics behind a late producer on a busy stream (tests/stream_order.py has the harness): the entry is outside the
27 stream-taking prototypes -- its stream travels in the struct -- so its case lives here.

Everything the call reads comes in two valid versions: another motion behind the same offsets, another inertial table (every mass
doubled, every limit halved), and in the struct another frame rate, gravity and ground height."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dynamics_inputs as di  # noqa: E402
from tests import dynamics_reference as R  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine, gpu, shapes  # noqa: E402

ROBOT = "unitree_g1"


class DynamicsCase(so.Case):
    """The differenced launch of tests/test_gpu_dynamics.py (``outputs``: the names to pass, None for all fifteen)."""
    entry, launches, h2d = "gmr_motion_dynamics", 2, 0
    struct_values = True

    def __init__(self, outputs=None, robot=ROBOT):
        super().__init__()
        from gmr_amd import _native
        self.robot = robot
        eng = engine(robot)
        tab = eng.inertial_device(R.model(robot)[1])
        finite = torch.where(torch.isfinite(tab["torque_limit"]), tab["torque_limit"], torch.full_like(tab["torque_limit"], 50.0))
        decoy = {"body_parent": tab["body_parent"], "body_mass": 2.0 * tab["body_mass"], "body_com": -tab["body_com"],
                 "body_inertia": 2.0 * tab["body_inertia"], "armature": tab["armature"] + 0.01, "torque_limit": 0.5 * finite}
        self.dev_in = {"qpos": (_dev(di.quantised(robot)), _dev(di.quantised(robot, 20))), "seq_offsets": (_dev(di.OFFS), _dev(di.OFFS))}
        self.dev_in.update({k: (tab[k], decoy[k]) for k in _native.DYNAMICS_TABLE})
        self.out_spec = {k + "_out": v for k, v in shapes(robot).items() if outputs is None or k in outputs}

    def new_struct(self):
        from gmr_amd import _native
        return _native.DynamicsInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.n_frames, st.n_seq, st.nbody = di.N, di.S, engine(self.robot).nbody
        st.fps, st.gravity_x, st.gravity_y, st.gravity_z = (30.0, 0.5, 0.0, -3.7) if decoy else (di.FPS, 0.0, 0.0, -9.81)
        st.ground_z, st.fz_min = (0.25, 0.2) if decoy else (0.0, R.FZ_MIN)

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_dynamics(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = DynamicsCase()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    for k in ("dev_decoy", "host_decoy"):
        assert not so.same(ser[k], ser["true"]), f"the {k} answer equals the true one: the case could not tell an ordering error"
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


def test_stream_order_behind_a_late_producer():
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the call
    computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case()
    want = gpu(ROBOT, "diff")
    assert all(np.array_equal(ser["true"][k + "_out"], _bytes(v).reshape(-1)) for k, v in want.items())   # the serial answer is the tests' answer
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_dynamics: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
          f"returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not so.same(r["answer"], ser["dev_decoy"]) and not so.same(r["answer"], ser["host_decoy"])
    assert r["returned_before_producer"]


def test_the_control_on_an_unordered_stream_sees_the_decoy():
    """The same call on a stream that does not wait for the producer reads the decoy inputs: the harness can fail."""
    case, ser, cycles, _ = _stream_case()
    r = so.run_late(case, DEV(), cycles, control=True)
    assert not r["vacuous"]
    if r["overtook_producer"]:
        assert not so.same(r["answer"], ser["true"])
