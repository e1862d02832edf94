"""Multi-robot batch retargeting, the parts that need no GPU: the two group-order exports, the public class's refusals, the
group item planning (global item bases, the combined auto_chunk input)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmr_group_plan_order", "gmr_group_ik_solve_ordered")


def test_group_order_exports_are_declared_and_bound():
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(gmr_group \*g, const gmr_group_input \*inputs, const gmr_ik_params \*params", src), name
        assert name in _native.EXPORTS
    lib = _native.load()
    assert lib.gmr_abi_version() == 5
    # a null group is refused before anything else (no device needed)
    prm = _native.IKParams()
    assert lib.gmr_group_plan_order(None, None, ctypes.byref(prm), 32, None, None) == -1
    assert lib.gmr_group_ik_solve_ordered(None, None, ctypes.byref(prm), None, None) == -1


@pytest.fixture
def no_device_work(monkeypatch):
    """Any attempt to build the group (the first device work) fails the test."""
    from gmr_amd import engine

    def boom(*a, **k):
        raise AssertionError("device work started before the robot list was checked")
    monkeypatch.setattr(engine, "EngineGroup", boom)


@pytest.mark.parametrize("robots,exc", [
    (["unitree_g1", "no_such_robot"], KeyError),
    ([], ValueError),
    (["unitree_g1", "booster_t1", "unitree_g1"], ValueError),
    (["unitree_g1"] * 65, ValueError),
])
def test_multi_robot_refuses_bad_robot_lists(no_device_work, robots, exc):
    from gmr_amd import MultiRobotRetargeting
    with pytest.raises(exc):
        MultiRobotRetargeting("smplx", robots)


def test_multi_robot_refuses_a_robot_without_a_config_for_the_source(no_device_work):
    from gmr_amd import IK_CONFIG_DICT, MultiRobotRetargeting
    assert "galaxea_r1pro" in IK_CONFIG_DICT["smplx"] and "galaxea_r1pro" not in IK_CONFIG_DICT["bvh"]
    with pytest.raises(KeyError):
        MultiRobotRetargeting("bvh", ["unitree_g1", "galaxea_r1pro"])
    with pytest.raises(KeyError):
        MultiRobotRetargeting("no_such_source", ["unitree_g1"])


def test_the_reference_names_are_unchanged():
    import gmr_amd
    assert "MultiRobotRetargeting" not in gmr_amd.__all__
    assert gmr_amd.__all__ == ["GeneralMotionRetargeting", "KinematicsModel", "load_robot_motion", "ROBOT_XML_DICT", "IK_CONFIG_DICT",
                               "ROBOT_BASE_DICT", "IK_CONFIG_ROOT", "ASSET_ROOT", "VIEWER_CAM_DISTANCE_DICT"]
    from gmr_amd.multi_robot import MultiRobotRetargeting
    assert gmr_amd.MultiRobotRetargeting is MultiRobotRetargeting


def test_group_item_bases():
    from gmr_amd.schedule import group_item_bases, make_items
    n = [len(make_items([0, 10, 30])), 0, len(make_items([0, 5, 5, 9, 20])), len(make_items([0, 7]))]
    assert n == [2, 0, 3, 1]
    b = group_item_bases(n)
    assert b.tolist() == [0, 2, 2, 5, 6]  # a member without work adds nothing; b[-1] = the total
    assert group_item_bases([]).tolist() == [0]
    with pytest.raises(ValueError):
        group_item_bases([1, -1])


def test_group_auto_chunk_sees_every_members_clips():
    from gmr_amd.schedule import auto_chunk, group_chunk_offsets
    a = np.array([0, 100, 400], dtype=np.int64)
    b = np.array([0, 50], dtype=np.int64)
    offs = group_chunk_offsets([a, None, b])
    assert offs.tolist() == [0, 100, 400, 450]
    assert group_chunk_offsets([None]).tolist() == [0]
    # config 4 as stated: 5 robots x 64 clips x 1000 frames on 2048 slots -> chunked (one robot alone would chunk too, but by the
    # frame total of all five)
    one = np.arange(65, dtype=np.int64) * 1000
    five = group_chunk_offsets([one] * 5)
    assert len(five) == 321 and five[-1] == 320000
    c, bi = auto_chunk(five, 2048)
    assert c > 0 and bi == 24
    assert (c, bi) == (80, 24)
    # many clips across robots: more than one per four slots in total -> whole clips, even if each robot alone would chunk
    small = np.arange(129, dtype=np.int64) * 300
    assert auto_chunk(small, 2048)[0] > 0
    assert auto_chunk(group_chunk_offsets([small] * 5), 2048) == (0, 0)
