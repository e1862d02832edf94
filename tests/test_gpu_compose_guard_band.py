"""gmr_motion_compose stays inside the arrays it was given (tests/guard_band.py has the harness; include/gmr_amd.h, "Extent and
alignment", the contract): every input, every table and both outputs alone in a guarded arena under the fills 0x00, 0xFF and 0x41.  The
case is the one of tests/test_gpu_compose_stream_order.py -- blends of 8 frames across segments of 63, 64, 65, 130, 40, 60 and 30
frames, so the last batch of most segments repeats its last row in idle loads -- on G1 (28 lanes idle) and on booster_k1 (35 lanes
idle)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV  # noqa: E402
from tests.test_gpu_compose_stream_order import ComposeCase  # noqa: E402

CASES = {"g1": lambda: ComposeCase(), "k1": lambda: ComposeCase(robot="booster_k1")}


@functools.lru_cache(maxsize=None)
def _case(name):
    case = CASES[name]()
    ser = so.serial_answers(case, DEV())
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    return case, ser["true"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stays_inside_its_arrays(name):
    """The outputs are written inside their declared extents and completely, no input changes, and no guard of any array changes."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, 0, 0)


@pytest.mark.parametrize("shift_in,shift_out", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_element_aligned_pointers(name, shift_in, shift_out):
    """Arrays that have the alignment of their element type only: the kernels load and store one element at a time."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, shift_in, shift_out)
