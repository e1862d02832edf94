"""gmr_motion_retime_plan_torque and the cubic gmr_motion_retime_apply stay inside the arrays they were given (tests/guard_band.py has
the harness; include/gmr_amd.h, "Extent and alignment", the contract): every input and every output alone in a guarded arena under
the fills 0x00, 0xFF and 0x41.  The cases are those of tests/test_gpu_retime_torque_stream_order.py -- clips of 0 to 130 rows, so that
the need kernel reads one row past its tile only where the clip has one, the alignment reaches back over 64 intervals or the whole
clip, and the cubic's stencil is reflected at both ends of every clip -- on G1 (29 hinge columns), on G1 with hands (43) and on
tree/chain/2 (one hinge column: 63 idle lanes)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_dynamics import DEV  # noqa: E402
from tests.test_gpu_retime_torque_stream_order import RetimeCubicCase, RetimeTorqueCase  # noqa: E402

CASES = {"plan-g1": lambda: RetimeTorqueCase("unitree_g1", "lens"), "plan-g1-ragged": lambda: RetimeTorqueCase("unitree_g1", "ragged"),
         "plan-hands": lambda: RetimeTorqueCase("unitree_g1_with_hands", "lens"), "plan-chain2": lambda: RetimeTorqueCase("tree/chain/2", "lens"),
         "cubic-g1": lambda: RetimeCubicCase("unitree_g1"), "cubic-k1": lambda: RetimeCubicCase("booster_k1")}


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
@pytest.mark.parametrize("name", ["plan-g1", "plan-chain2", "cubic-k1"])
def test_element_aligned_pointers(name, shift_in, shift_out):
    """Arrays that have the alignment of their element type only: the kernels load and store one element at a time."""
    case, plain = _case(name)
    gb.check(case, DEV(), plain, shift_in, shift_out)
