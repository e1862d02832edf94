"""gmr_motion_self_collision_repair behind a late producer on a busy stream (tests/stream_order.py has the harness): the entry is
outside the 27 stream-taking prototypes -- its stream travels in the struct -- so its case lives here.  One call enqueues two kernels.

Everything the call reads comes in two valid versions: another motion behind the same offsets, other proxies (fatter, shorter
capsules; the pair table reversed), and in the struct another margin, pass count, damping, step cap and hinge mask."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dynamics_inputs as di  # noqa: E402
from tests import self_collision_inputs as ci  # noqa: E402
from tests import self_collision_repair_inputs as ri  # noqa: E402
from tests import self_collision_repair_reference as RR  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_self_collision_repair import gpu, shapes  # noqa: E402

CASE = "k1_margin"     # (146 of its 332 frames are repaired)


class SelfCollisionRepairCase(so.Case):
    """The launch of tests/test_gpu_self_collision_repair.py (``outputs``: the names to pass, None for all nine)."""
    entry, launches, h2d = "gmr_motion_self_collision_repair", 2, 0
    struct_values = True

    def __init__(self, outputs=None, case=CASE):
        super().__init__()
        from gmr_amd import _native
        self.case, self.robot = case, ri.robot_of(case)
        caps, pairs = ri.tables(case)
        tab = engine(self.robot).collision_device(caps, pairs)
        decoy = {"cap_body": tab["cap_body"], "cap_p0": tab["cap_p0"] + 0.01, "cap_p1": 0.9 * tab["cap_p1"], "cap_radius": 1.5 * tab["cap_radius"],
                 "pairs": torch.flip(tab["pairs"], dims=(0,)).contiguous()}
        q, offs = ri.rows(case)
        self.dev_in = {"qpos": (_dev(q), _dev(di.explicit(self.robot, 20)[0])), "seq_offsets": (_dev(offs), _dev(offs))}
        self.dev_in.update({k: (tab[k], decoy[k]) for k in _native.SELF_COLLISION_TABLE})
        self.out_spec = {k + "_out": v for k, v in shapes(robot=self.robot).items() if outputs is None or k in outputs}

    def new_struct(self):
        from gmr_amd import _native
        return _native.SelfCollisionRepairInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        caps, pairs = ri.tables(self.case)
        st.n_frames, st.n_seq, st.n_caps, st.n_pairs = ri.N, ri.S, len(caps), len(pairs)
        st.margin = 0.05 if decoy else ri.margin(self.case)
        st.iterations, st.damping, st.step_cap = (3, 1e-3, 0.05) if decoy else (RR.ITERATIONS, RR.DAMPING, RR.STEP_CAP)
        st.resolve_tol, st.hinge_mask = RR.RESOLVE_TOL, (0x5555 if decoy else ri.hinge_mask(self.case))

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_self_collision_repair(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = SelfCollisionRepairCase()
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
    want = gpu(CASE)
    assert all(np.array_equal(ser["true"][k + "_out"], _bytes(v).reshape(-1)) for k, v in want.items())   # the serial answer is the tests' answer
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_self_collision_repair: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
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
