"""The HIP IK kernels under the certificate of tests/ik_certificate.py: does the qpos the GPU returns put the robot on the
prepared targets, and is it a constrained minimiser of the stage cost?  No oracle here -- the judge reads the Python-side robot
and config only, so a mistake made while compiling the blob, or one the kernel and the oracle share, does not cancel.  The cases
and the thresholds (10 x what the CPU oracle reaches, tests/test_ik_certificate_host.py) are the host tests'.
"""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd.engine import Engine, IKParams  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from tests import ik_certificate as ikc  # noqa: E402
from tests import ik_certificate_cases as cases  # noqa: E402

SHAPED = "IkShapeG1Smplx"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture
def solve(monkeypatch, capfd, dev):
    """solve(case, qp, generic_shape) -> (final qpos of every clip, kernel instances of the launches); both switches are read at
    model creation."""
    monkeypatch.setenv("GMR_DEBUG_PLAN", "1")

    def go(case, qp, generic_shape=False):
        monkeypatch.setenv("GMR_AMD_GENERIC_QP", "1" if qp == "generic" else "0")
        monkeypatch.setenv("GMR_AMD_GENERIC_SHAPE", "1" if generic_shape else "0")
        eng = Engine(case.cm, 0)
        assert qp != "generic" or eng.info.reserved[0] == 0  # core size of the structured layout, 0 = dense generic QP
        pos, quat, offs = case.held_input()
        capfd.readouterr()
        q, it, _ = eng.ik_solve(torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev), case.cm.slot_columns(case.names),
                                make_items(offs), params=IKParams(**case.solver), launch_order=None)
        q, it = q.cpu().numpy(), it.cpu().numpy()
        how = re.findall(r"gmr: ik launch: solve instance (\w+)", capfd.readouterr().err)
        eng.close()
        assert not np.isnan(q).any() and (it >> 30).max() == 0, "a QP hit its iteration cap"
        return q[case.final_rows()], how
    return go


def _assert_passes(case, q_final, family):
    got = cases.certify(case, q_final)
    print(f"[certificate] gpu {case.name}: {got}")
    for key, bound in ikc.thresholds(family, case.tables).items():
        assert got[key] <= bound, (case.name, key, got[key], bound)
    return got


@pytest.mark.parametrize("qp", ["structured", "generic"])
@pytest.mark.parametrize("robot_name", cases.REACHABLE_ROBOTS)
def test_reachable_targets(robot_name, qp, solve):
    """(a): the robot is on its targets (cost ratio) and stationary for every table that is switched on."""
    case = cases.reachable_case(robot_name)
    q_final, how = solve(case, qp)
    if robot_name == "unitree_g1":
        assert how == [SHAPED if qp == "structured" else "generic"]
    _assert_passes(case, q_final, "reachable")


def test_reachable_targets_generic_kernel_instance(solve):
    """unitree_g1 again on the kernel instance without the model's shape compiled in."""
    case = cases.reachable_case("unitree_g1")
    q_final, how = solve(case, "structured", generic_shape=True)
    assert how == ["generic"]
    _assert_passes(case, q_final, "reachable")


def test_reachable_targets_through_the_group_kernel(dev):
    """Two robots in one launch (MultiRobotRetargeting.retarget_batch -> EngineGroup), the class's own constants."""
    from gmr_amd.multi_robot import MultiRobotRetargeting
    by_robot = {r: cases.pair_case(r) for r in cases.PAIR_ROBOTS}
    first = by_robot[cases.PAIR_ROBOTS[0]]
    pos, quat, offs = first.held_input()
    mr = MultiRobotRetargeting("smplx", list(cases.PAIR_ROBOTS), device=0)
    assert dict(max_iter=mr.max_iter, tol=IKParams().tol) == first.solver
    qpos = mr.retarget_batch(pos, quat, first.names, seq_offsets=offs)
    mr.close()
    for r, case in by_robot.items():
        _assert_passes(case, qpos[r][case.final_rows()], "reachable_default")


@pytest.mark.parametrize("qp", ["structured", "generic"])
def test_held_reference_frame(qp, solve, golden_dir):
    """(b) 1: unreachable targets, joint limits active; the last stage's table is stationary under the limits."""
    case = cases.held_reference_frame_case(golden_dir)
    q_final, _ = solve(case, qp)
    assert _assert_passes(case, q_final, "limits")["active"] >= 1


@pytest.mark.parametrize("qp", ["structured", "generic"])
def test_synthetic_robot_at_its_limits(qp, solve, tmp_path):
    """(b) 2: two identical tables, a narrow joint range."""
    case = cases.synthetic_limits_case(tmp_path)
    q_final, _ = solve(case, qp)
    assert _assert_passes(case, q_final, "limits")["active"] >= 1
