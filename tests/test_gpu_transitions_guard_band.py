"""gmr_motion_transitions stays inside the arrays it was given (tests/guard_band.py has the harness; include/gmr_amd.h, "Extent and
alignment", the contract): every input, every table and all five outputs -- `points` and `moments`, the scratch that is also a result,
included -- alone in a guarded arena under the fills 0x00, 0xFF and 0x41.  The case is the one of
tests/test_gpu_transitions_stream_order.py: clips of 0, 1, 7, 8, 9, 63, 64, 65 and 130 frames against themselves at L = 8, so every
diagonal pass stages target rows clamped at both ends of a clip, on G1 (38 points) and on booster_k1 (23 points: 41 lanes idle in the
points kernel, a row of 69 doubles in the ring)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV  # noqa: E402
from tests.test_gpu_transitions_stream_order import TransitionsCase  # noqa: E402

CASES = {"g1": lambda: TransitionsCase(), "k1": lambda: TransitionsCase(robot="booster_k1")}


@functools.lru_cache(maxsize=None)
def _case(name):
    case = CASES[name]()
    ser = so.serial_answers(case, DEV())
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    return case, ser["true"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stays_inside_its_arrays(name):
    """The outputs are written inside their declared extents and completely (of `moments`: what the contract says is written), no
    input changes, and no guard of any array changes."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, 0, 0)


@pytest.mark.parametrize("shift_in,shift_out", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_element_aligned_pointers(name, shift_in, shift_out):
    """Arrays that have the alignment of their element type only: the kernels load and store one element at a time."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, shift_in, shift_out)
