"""gmr_motion_retime_plan and gmr_motion_retime_apply stay inside the arrays they were given (tests/guard_band.py has the harness;
include/gmr_amd.h, "Extent and alignment", the contract): every input and every output of both entries alone in a guarded arena under
the fills 0x00, 0xFF and 0x41.  The cases are those of tests/test_gpu_retime_stream_order.py -- clips of 0 to 130 frames and the
widest window, so that the need kernel's batches repeat the clips' last rows in idle loads, the ticks kernel's halo of 64 intervals
reaches past both ends of every clip, and the apply kernel's last tiles are partial -- on G1 (28 lanes idle) and on booster_k1 (35
lanes idle)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV  # noqa: E402
from tests.test_gpu_retime_stream_order import RetimeApplyCase, RetimePlanCase  # noqa: E402

ROBOTS = {"g1": "unitree_g1", "k1": "booster_k1"}
CASES = {f"{which}-{r}": (cls, robot) for which, cls in (("plan", RetimePlanCase), ("apply", RetimeApplyCase)) for r, robot in ROBOTS.items()}


@functools.lru_cache(maxsize=None)
def _case(name):
    cls, robot = CASES[name]
    case = cls(robot)
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
