"""Host-only checks of the shared-stage-tables property of a shaped IK instance ("Shared stage tables").

``IkShapeG1Smplx::stage_shared = 1`` lets the instance read a stage's tables once per work item: it is only sound for a model whose two
task tables differ in their weights alone (``stage_tables_shared``, model_plan.h), so ``ik_shape_matches`` requires that of the model
beside the 15 shape fields.  ``gmr_debug_ik_shape`` (api.hip) runs the same match without a device; its ``alter_field`` indices 15 .. 18,
behind the fields, each break one of the equalities in table 1 of the host model.
"""
import ctypes as C
import os

import pytest

from gmr_amd import params
from tests.util import compiled

N_FIELDS = 15  # GMR_IK_SHAPE_FIELDS (dev_model.h); tests/test_ik_shapes_host.py names them
G1_FIELDS = [7, 14, 14, 1, 1, 1, 3, 3, 384, 32, 4, 35, 14, 36, 0]  # IkShapeG1Smplx, in that order
BROKEN = {15: "tbody", 16: "tslot", 17: "acomp", 18: "comp_plan"}  # table 1's first entry of each


@pytest.fixture(scope="module")
def shape_of():
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    f = _native.load().gmr_debug_ik_shape
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_size_t] + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]

    def call(cm, alter=-1, delta=0):
        fields, name = (C.c_int * 16)(*([-7] * 16)), C.create_string_buffer(64)
        rc = f(cm.blob, len(cm.blob), 0, alter, delta, 0, 0, 1, fields, name, len(name))
        assert rc >= -1, rc
        assert fields[N_FIELDS] == -7  # 15 ints written, as before
        return rc, name.value.decode(), list(fields)[:N_FIELDS]
    return call


def test_g1_smplx_still_takes_the_shaped_instance(shape_of):
    assert shape_of(compiled("smplx", "unitree_g1")) == (0, "IkShapeG1Smplx", G1_FIELDS)


@pytest.mark.parametrize("alter", sorted(BROKEN), ids=[BROKEN[k] for k in sorted(BROKEN)])
@pytest.mark.parametrize("delta", [1, -1])
def test_one_broken_equality_sends_it_to_the_generic_instance(shape_of, alter, delta):
    """The 15 fields still carry the shape's values: only the property fails."""
    assert shape_of(compiled("smplx", "unitree_g1"), alter=alter, delta=delta) == (-1, "generic", G1_FIELDS)


def test_an_index_behind_the_last_alters_nothing(shape_of):
    assert shape_of(compiled("smplx", "unitree_g1"), alter=19, delta=1) == (0, "IkShapeG1Smplx", G1_FIELDS)


def test_every_registry_config_gets_the_instance_its_fields_imply(shape_of):
    """As tests/test_ik_shapes_host.py expects: a packed config whose fields are the shape's is shaped (so its tables are shared),
    every other one is generic."""
    seen = shaped = 0
    for src, robots in params.IK_CONFIG_DICT.items():
        for robot in robots:
            if not os.path.exists(params.IK_CONFIG_DICT[src][robot]):
                continue
            rc, name, fields = shape_of(compiled(src, robot))
            want = fields == G1_FIELDS
            assert (rc == 0 and name == "IkShapeG1Smplx") if want else (rc == -1 and name == "generic"), (src, robot, fields)
            seen += 1
            shaped += want
    assert seen >= 12 and shaped >= 1
