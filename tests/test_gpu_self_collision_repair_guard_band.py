"""gmr_motion_self_collision_repair stays inside the arrays it was given (tests/guard_band.py has the harness; include/gmr_amd.h,
"Extent and alignment", the contract): every input and every output alone in a guarded arena under the fills 0x00, 0xFF and 0x41.
The case is the one of tests/test_gpu_self_collision_repair_stream_order.py -- clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames --
on booster_k1 with a margin (146 frames repaired), on G1 (45 capsules, 869 pairs: 37 lanes idle in the last pass over the pairs)
and with outputs left out."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV  # noqa: E402
from tests.test_gpu_self_collision_repair_stream_order import SelfCollisionRepairCase  # noqa: E402

CASES = {"k1": lambda: SelfCollisionRepairCase(), "g1": lambda: SelfCollisionRepairCase(case="g1"),
         "qpos_only": lambda: SelfCollisionRepairCase(outputs=("qpos",)),
         "frames_only": lambda: SelfCollisionRepairCase(outputs=("qpos", "clearance_after"), case="g1"),
         "statistics_only": lambda: SelfCollisionRepairCase(outputs=("qpos", "clearance_before", "clearance_after", "move", "unresolved_frames", "move_max"))}


@functools.lru_cache(maxsize=None)
def _case(name):
    case = CASES[name]()
    ser = so.serial_answers(case, DEV())
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    return case, ser["true"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stays_inside_its_arrays(name):
    """Every output array is written inside its declared extent and completely; an output that is left out (a NULL pointer) is not
    touched: there is no array of it, and no guard of any other array changes."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, 0, 0)


@pytest.mark.parametrize("shift_in,shift_out", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("name", ["g1", "k1"])
def test_element_aligned_pointers(name, shift_in, shift_out):
    """Arrays that have the alignment of their element type only: the kernels load and store one element at a time."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, shift_in, shift_out)
