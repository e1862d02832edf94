"""gmr_motion_self_collision behind a late producer on a busy stream (tests/stream_order.py has the harness): the entry is outside
the 27 stream-taking prototypes -- its stream travels in the struct -- so its case lives here.  One call enqueues two kernels.

Everything the call reads comes in two valid versions: another motion behind the same offsets, other proxies (fatter, shorter
capsules; the pair table reversed), and in the struct another margin."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dynamics_inputs as di  # noqa: E402
from tests import self_collision_inputs as ci  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_self_collision import gpu, shapes  # noqa: E402

ROBOT = "unitree_g1"


class SelfCollisionCase(so.Case):
    """The launch of tests/test_gpu_self_collision.py (``outputs``: the names to pass, None for all ten)."""
    entry, launches, h2d = "gmr_motion_self_collision", 2, 0
    struct_values = True

    def __init__(self, outputs=None, robot=ROBOT):
        super().__init__()
        from gmr_amd import _native
        self.robot = robot
        caps, pairs = ci.tables(robot)
        tab = engine(robot).collision_device(caps, pairs)
        decoy = {"cap_body": tab["cap_body"], "cap_p0": tab["cap_p0"] + 0.01, "cap_p1": 0.9 * tab["cap_p1"], "cap_radius": 1.5 * tab["cap_radius"],
                 "pairs": torch.flip(tab["pairs"], dims=(0,)).contiguous()}
        self.dev_in = {"qpos": (_dev(ci.qpos(robot)), _dev(di.explicit(robot, 20)[0])), "seq_offsets": (_dev(ci.OFFS), _dev(ci.OFFS))}
        self.dev_in.update({k: (tab[k], decoy[k]) for k in _native.SELF_COLLISION_TABLE})
        self.out_spec = {k + "_out": v for k, v in shapes().items() if outputs is None or k in outputs}

    def new_struct(self):
        from gmr_amd import _native
        return _native.SelfCollisionInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        caps, pairs = ci.tables(self.robot)
        st.n_frames, st.n_seq, st.n_caps, st.n_pairs = ci.N, ci.S, len(caps), len(pairs)
        st.margin = 0.05 if decoy else ci.MARGIN

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_self_collision(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = SelfCollisionCase()
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
    want = gpu(ROBOT)
    assert all(np.array_equal(ser["true"][k + "_out"], _bytes(v).reshape(-1)) for k, v in want.items())   # the serial answer is the tests' answer
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_self_collision: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
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
