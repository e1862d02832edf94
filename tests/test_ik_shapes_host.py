"""Host-only checks of the shaped IK kernel dispatch: which kernel instance the library picks for a model and a launch.

``gmr_debug_ik_shape`` (api.hip; a test hook outside include/gmr_amd.h) builds a blob's model as ``gmr_model_create`` does up to the
first device call and runs the same match (``ik_shape_of`` / ``ik_launch_shape``) a launch runs, so none of this needs a GPU.
"""
import ctypes as C
import os

import pytest

from gmr_amd import params
from tests.util import compiled

# GMR_IK_SHAPE_FIELDS, in order (ik_kernel.hip.h)
FIELDS = ["nlimb", "ntask0", "ntask1", "use0", "use1", "same_tasks", "ncpass0", "ncpass1", "npairp", "nbody", "fkrounds", "n_act", "nslot", "nq",
          "root_slot"]
G1_SHAPE = dict(nlimb=7, ntask0=14, ntask1=14, use0=1, use1=1, same_tasks=1, ncpass0=3, ncpass1=3, npairp=384, nbody=32, fkrounds=4, n_act=35,
                nslot=14, nq=36, root_slot=0)


@pytest.fixture(scope="module")
def shape_of():
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    lib = _native.load()
    f = lib.gmr_debug_ik_shape
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_size_t] + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]

    def call(cm, force_generic_qp=0, alter=-1, delta=0, in_f64=0, offset_to_ground=0, plain=1):
        fields, name = (C.c_int * 16)(), C.create_string_buffer(64)
        rc = f(cm.blob, len(cm.blob), force_generic_qp, alter, delta, in_f64, offset_to_ground, plain, fields, name, len(name))
        assert rc >= -1, rc
        return rc, name.value.decode(), dict(zip(FIELDS, fields))
    return call


def test_g1_smplx_plain_call_takes_the_shaped_instance(shape_of):
    rc, name, fields = shape_of(compiled("smplx", "unitree_g1"))
    assert rc == 0 and name == "IkShapeG1Smplx"
    assert fields == G1_SHAPE  # the values compiled into the instance are the packed model's


def test_every_registry_robot_gets_its_instance(shape_of):
    """The only shaped instance is unitree_g1 / smplx's; every other registry model (other counts in at least one field) is generic."""
    seen = 0
    for src, robots in params.IK_CONFIG_DICT.items():
        for robot in robots:
            if not os.path.exists(params.IK_CONFIG_DICT[src][robot]):
                continue  # (the registry names more configs than have been packed)
            rc, name, fields = shape_of(compiled(src, robot))
            want = fields == G1_SHAPE
            assert (rc == 0 and name == "IkShapeG1Smplx") if want else (rc == -1 and name == "generic"), (src, robot, fields)
            seen += 1
    assert seen >= 12
    assert shape_of(compiled("smplx", "booster_t1"))[0] == -1
    assert shape_of(compiled("smplx", "unitree_g1_with_hands"))[0] == -1  # same tree counts, 14 more coordinates


@pytest.mark.parametrize("field", range(len(FIELDS)))
@pytest.mark.parametrize("delta", [1, -1])
def test_a_model_altered_in_one_field_does_not_match(shape_of, field, delta):
    rc, name, fields = shape_of(compiled("smplx", "unitree_g1"), alter=field, delta=delta)
    assert fields[FIELDS[field]] == G1_SHAPE[FIELDS[field]] + delta
    assert rc == -1 and name == "generic"


@pytest.mark.parametrize("launch", [dict(in_f64=1), dict(offset_to_ground=1), dict(plain=0), dict(force_generic_qp=1)])
def test_a_launch_that_is_not_plain_takes_the_generic_instance(shape_of, launch):
    assert shape_of(compiled("smplx", "unitree_g1"), **launch)[:2] == (-1, "generic")
