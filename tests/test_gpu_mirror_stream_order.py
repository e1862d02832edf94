"""gmr_motion_mirror behind a late producer on a busy stream (tests/stream_order.py has the harness): the entry is outside the 27
stream-taking prototypes -- its stream travels in the struct -- so its case lives here.  One call enqueues one kernel.

Everything the call reads comes in two valid versions: another motion behind the same offsets, another table (the identity
permutation with every sign negative, an involution too), and in the struct the other mode."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import mirror_inputs as mi  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_mirror import gpu  # noqa: E402

ROBOT = "unitree_g1"
MODE = {"world": 0, "start": 1}


class MirrorCase(so.Case):
    """The launch of tests/test_gpu_mirror.py in one mode (the decoy struct asks for the other one)."""
    entry, launches, h2d = "gmr_motion_mirror", 1, 0
    struct_values = True

    def __init__(self, about="world", robot=ROBOT):
        super().__init__()
        self.robot, self.about = robot, about
        eng = engine(robot)
        tab = eng.symmetry_device(mi.plan(robot))
        decoy = {"col_src": torch.arange(eng.nq, dtype=torch.int32, device=DEV()),
                 "col_sign": torch.cat([torch.ones(7, dtype=torch.float64, device=DEV()), -torch.ones(eng.nq - 7, dtype=torch.float64, device=DEV())])}
        self.dev_in = {"qpos": (_dev(mi.qpos(robot)), _dev(mi.qpos(robot, 20))), "seq_offsets": (_dev(mi.OFFS), _dev(mi.OFFS)),
                       "col_src": (tab["col_src"], decoy["col_src"]), "col_sign": (tab["col_sign"], decoy["col_sign"])}
        self.out_spec = {"qpos_out": ((mi.N, eng.nq), torch.float64)}

    def new_struct(self):
        from gmr_amd import _native
        return _native.MirrorInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.n_frames, st.n_seq = mi.N, mi.S
        st.mode = MODE[self.about] ^ 1 if decoy else MODE[self.about]

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_mirror(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case(about):
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = MirrorCase(about)
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    for k in ("dev_decoy", "host_decoy"):
        assert not so.same(ser[k], ser["true"]), f"the {k} answer equals the true one: the case could not tell an ordering error"
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


@pytest.mark.parametrize("about", mi.MODES)
def test_stream_order_behind_a_late_producer(about):
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the call
    computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case(about)
    assert np.array_equal(ser["true"]["qpos_out"], _bytes(gpu(ROBOT, about)).reshape(-1))   # the serial answer is the tests' answer
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_mirror ({about}): serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
          f"returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not so.same(r["answer"], ser["dev_decoy"]) and not so.same(r["answer"], ser["host_decoy"])
    assert r["returned_before_producer"]


def test_the_control_on_an_unordered_stream_sees_the_decoy():
    """The same call on a stream that does not wait for the producer reads the decoy inputs: the harness can fail."""
    case, ser, cycles, _ = _stream_case("start")
    r = so.run_late(case, DEV(), cycles, control=True)
    assert not r["vacuous"]
    if r["overtook_producer"]:
        assert not so.same(r["answer"], ser["true"])
