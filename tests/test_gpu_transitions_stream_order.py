"""gmr_motion_transitions behind a late producer on a busy stream (tests/stream_order.py has the harness): the entry is outside the
stream-taking prototypes -- its stream travels in the struct -- so its case lives here.  One call enqueues three kernels; the second
reads what the first wrote (moments), the third what both wrote (points, moments), on the same stream.

Everything the call reads that can have one comes in two valid versions behind the same counts: another motion, other bodies and
other weights.  The clip tables exist in one version (another would change the counts)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import stream_order as so  # noqa: E402
from tests import transitions_inputs as ti  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.test_gpu_transitions import main_case  # noqa: E402

ROBOT = "unitree_g1"
L = 8


class TransitionsCase(so.Case):
    """The launches of tests/test_gpu_transitions.py's main comparison at L = 8."""
    entry, launches, h2d = "gmr_motion_transitions", 3, 0

    def __init__(self, robot=ROBOT):
        super().__init__()
        self.robot = robot
        q, self.offs = ti.library(robot, L)
        ids, w = ti.all_bodies(robot)
        self.P, self.N = len(ids), q.shape[0]
        src, so_, dst, do = ti.tables(self.offs, L)
        self.E, self.D, self.NT = int(so_[-1]), len(dst), int(do[-1])
        w = w / w.sum()
        w2 = np.linspace(1.0, 2.0, self.P)
        same = lambda a: (_dev(a), _dev(a))   # noqa: E731
        self.dev_in = {"qpos": (_dev(q), _dev(ti.rows(robot)[-self.N:])), "seq_offsets": same(self.offs),
                       "body_ids": (_dev(ids), _dev(ids[::-1].copy())), "weights": (_dev(w), _dev(w2 / w2.sum())),
                       "src_clips": same(src), "src_offsets": same(so_), "dst_clips": same(dst), "dst_offsets": same(do)}
        f64 = torch.float64
        self.out_spec = {"points": ((self.N, self.P, 3), f64), "moments": ((self.N, 6), f64), "best_cost": ((self.E, self.D), f64),
                         "best_frame": ((self.E, self.D), torch.int32), "cost_out": ((self.E, self.NT), f64)}

    def written(self, b, name):
        """What the call writes of each output: all of it, but of `moments` the windowed half only for rows that start a window."""
        return ti.written_moments(self.offs, self.N, L) if name == "moments" else None

    def new_struct(self):
        from gmr_amd import _native
        return _native.TransitionsInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.n_frames, st.n_seq, st.n_bodies, st.window, st.src_stride, st.min_gap = self.N, len(self.offs) - 1, self.P, L, 1, L
        st.n_src_clips, st.n_dst_clips, st.n_sources, st.n_targets = self.D, self.D, self.E, self.NT

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = engine(self.robot)
        return eng._lib.gmr_motion_transitions(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = TransitionsCase()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    assert not so.same(ser["dev_decoy"], ser["true"]), "the decoy answer equals the true one: the case could not tell an ordering error"
    assert so.differing(ser["dev_decoy"], ser["true"]) == ["points", "moments", "best_cost", "best_frame", "cost_out"]
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


def test_stream_order_behind_a_late_producer():
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the call
    computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case()
    assert case.launches == 3
    for k in ("points", "best_cost", "best_frame", "cost_out"):                             # the serial answer is the tests' answer
        assert np.array_equal(ser["true"][k], _bytes(main_case(ROBOT, L)[0][k]).reshape(-1)), k
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_transitions: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
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
