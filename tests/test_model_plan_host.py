"""gmr_amd/csrc/model_plan.h without a GPU: a stand-alone C++ program (tests/model_plan_host.cpp: its own main, built with the host
compiler under AddressSanitizer and UBSan, never loaded into Python) plans blobs that Python writes to temporary files.

- Every packed registry config x force_generic x min_nvp: the dump of the plan (both DevModels, both LdsLayouts, the scalars, every
  table of the model image with its offset) hashes to the digest recorded from the commit before model_plan.h existed
  (tests/golden/model_plan_digests.json, tools/record_model_plan.py).  No tolerance: nothing in a plan is floating-point arithmetic.
- The plan the host compiler makes is the one hipcc builds into the library: gmr_debug_ik_shape agrees field by field.
- On every blob that plans, the program checks what the kernels assume of the tables (check_plan in the program).
- Small synthetic blobs reach the branches the registry does not, and the refusals keep their code and exact message.

"More than kMaxCompPass passes" has no blob: GMR_MAX_TASKS = 32 tasks per table give at most 29 dependent passes (a chain of composites
that each add one task to the one below; an entry of more own tasks takes fewer passes per task).  The stage is called with a hand-made
chain of composites instead (--too-many-passes).
"""
import ctypes as C
import json
import struct

import numpy as np
import pytest

from gmr_amd import model as gm
from tests import model_plan_cases as mp
from tests.util import compiled

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
NONE, HINGE, FREE = 0, 1, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx, rocm = mp.toolchain()
    if cxx is None:
        pytest.skip("no C++ compiler")
    if not rocm:
        pytest.skip("no ROCm headers")
    return mp.build_program(cxx, tmp_path_factory.mktemp("model_plan") / "model_plan_host", mp.SANITIZE)


@pytest.fixture(scope="module")
def registry(program, tmp_path_factory):
    return mp.run_cases(program, mp.registry_cases(), tmp_path_factory.mktemp("registry"))


def test_registry_plans_are_the_parents(registry):
    with open(mp.GOLDEN) as f:
        golden = json.load(f)["digests"]
    assert len(mp.registry_configs()) >= 12
    assert sorted(golden) == sorted(registry)  # every config x force_generic {0, 1} x min_nvp {0, 64}
    for key, r in registry.items():
        assert r["code"] == OK and r["message"] == "", (key, r)
    wrong = [key for key, r in registry.items() if r["digest"] != golden[key]]
    assert not wrong, wrong


def test_the_library_plans_what_the_host_compiler_plans(registry):
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    f = _native.load().gmr_debug_ik_shape
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_size_t] + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    shaped = 0
    for src, robot in mp.registry_configs():
        blob = compiled(src, robot).blob
        for fg in (0, 1):
            fields, name = (C.c_int * 16)(), C.create_string_buffer(64)
            rc = f(blob, len(blob), fg, -1, 0, 0, 0, 1, fields, name, len(name))
            r = registry[f"{src}/{robot}/generic{fg}/min_nvp0"]
            assert (rc, name.value.decode(), list(fields)[:15]) == (r["shape"], r["name"], r["fields"]), (src, robot, fg)
            shaped += rc >= 0
    assert shaped >= 1  # unitree_g1 / smplx


# ---------------------------------------------------------------------------------------------------------------- synthetic blobs
def synth_blob(parent, hinge=(), tasks=((), ()), nslot=1, root_mask=0, edit=None):
    """A blob by hand (gmr_blob.h): bodies by `parent`, hinges (about z) on the bodies in `hinge`, tasks[k] = [(body, slot), ...].
    edit(header fields, arrays, offsets) may break it before it is packed."""
    nb = len(parent)
    jtype = np.array([FREE] + [HINGE if b in hinge else NONE for b in range(1, nb)], "<i4")
    qadr, dadr = np.full(nb, -1, "<i4"), np.full(nb, -1, "<i4")
    qadr[0] = dadr[0] = 0
    nq, nv = 7, 6
    for b in range(1, nb):
        if jtype[b] == HINGE:
            qadr[b], dadr[b] = nq, nv
            nq, nv = nq + 1, nv + 1
    axis = np.zeros((nb, 3))
    axis[jtype == HINGE, 2] = 1.0
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (nb, 1))
    rng = np.random.default_rng(nb)
    qpos0 = np.zeros(nq)
    qpos0[3] = 1.0
    arrays = dict(
        parent=np.asarray(parent, "<i4"), jnt_type=jtype, qpos_adr=qadr, dof_adr=dadr, jnt_limited=(jtype == HINGE).astype("<i4"),
        body_pos=rng.uniform(-0.2, 0.2, (nb, 3)), body_quat=quat, body_quat_raw=quat, jnt_axis=axis, jnt_range=np.tile([-1.5, 1.5], (nb, 1)),
        qpos0=qpos0, slot_scale=np.ones(nslot), slot_pos_off=np.zeros((nslot, 3)), slot_rot_off=np.tile([1.0, 0.0, 0.0, 0.0], (nslot, 1)),
        slot_is_foot=np.zeros(nslot, "<i4"),
        task_body0=np.array([t[0] for t in tasks[0]], "<i4"), task_body1=np.array([t[0] for t in tasks[1]], "<i4"),
        task_slot0=np.array([t[1] for t in tasks[0]], "<i4"), task_slot1=np.array([t[1] for t in tasks[1]], "<i4"),
        task_wp0=np.full(len(tasks[0]), 100.0), task_wp1=np.full(len(tasks[1]), 100.0),
        task_wr0=np.full(len(tasks[0]), 10.0), task_wr1=np.full(len(tasks[1]), 10.0))
    hdr = dict(nbody=nb, nq=nq, nv=nv, nslot=nslot, ntask0=len(tasks[0]), ntask1=len(tasks[1]), use0=1, use1=1, root_slot=0, root_mask=root_mask,
               total=None)
    offs, body, cur = {}, bytearray(), (gm.HEADER_BYTES + 7) & ~7
    for name, a in arrays.items():
        raw = np.ascontiguousarray(a, dtype=a.dtype if a.dtype.kind == "i" else "<f8").tobytes()
        raw += b"\0" * (-len(raw) % 8)
        offs[name] = cur
        body += raw
        cur += len(raw)
    if edit:
        edit(hdr, offs)
    header = struct.pack(gm._HEADER_FMT, gm.BLOB_MAGIC, gm.BLOB_VERSION, cur if hdr["total"] is None else hdr["total"], 0,
                         hdr["nbody"], hdr["nq"], hdr["nv"], hdr["nslot"], hdr["ntask0"], hdr["ntask1"], hdr["use0"], hdr["use1"], hdr["root_slot"],
                         hdr["root_mask"], 0, 0,
                         *[offs[n] for n in ("parent", "jnt_type", "qpos_adr", "dof_adr", "jnt_limited", "body_pos", "body_quat", "body_quat_raw",
                                             "jnt_axis", "jnt_range", "qpos0", "slot_scale", "slot_pos_off", "slot_rot_off", "slot_is_foot",
                                             "task_body0", "task_body1", "task_slot0", "task_slot1", "task_wp0", "task_wp1", "task_wr0", "task_wr1")],
                         0, 0, 0)
    blob = header + b"\0" * (((gm.HEADER_BYTES + 7) & ~7) - gm.HEADER_BYTES) + bytes(body)
    assert len(blob) == cur
    return blob


def set_axis_on_root(blob):
    """The same blob with a hinge axis written on body 0."""
    off = struct.unpack_from("<I", blob, 16 + 12 * 4 + 8 * 4)[0]  # off_jnt_axis: the ninth offset behind 4 + 12 header words
    return blob[:off] + struct.pack("<d", 1.0) + blob[off + 8:]


CHAIN64 = list(range(-1, 63))
# a trunk (1, 2) with two arms of three hinges and a leg of two
SMALL = [-1, 0, 1, 2, 3, 4, 2, 6, 7, 0, 9]
SMALL_HINGES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
SMALL_TASKS = [(5, 0), (8, 1), (10, 2), (0, 3)]


def bushy(n):
    """A spine 0 .. n whose bodies each have a leaf that comes after the whole subtree below them: n poses are parked at once (the
    last spine body's leaf is its next body, which needs no slot)."""
    return list(range(-1, n)) + list(range(n, -1, -1))


PLANS = {
    "chain of 64 bodies": dict(parent=CHAIN64, hinge=tuple(range(1, 64, 7)), tasks=([(63, 0), (30, 1)], [(63, 0)]), nslot=2),
    "planar base": dict(parent=SMALL, hinge=SMALL_HINGES, tasks=(SMALL_TASKS, SMALL_TASKS), nslot=4, root_mask=0x23),
    "free base": dict(parent=SMALL, hinge=SMALL_HINGES, tasks=(SMALL_TASKS, SMALL_TASKS[:2]), nslot=4),
    "second table empty": dict(parent=SMALL, hinge=SMALL_HINGES, tasks=(SMALL_TASKS, ()), nslot=4),
    "both tables empty": dict(parent=SMALL, hinge=SMALL_HINGES, tasks=((), ()), nslot=0),
    "twelve branch slots": dict(parent=bushy(12), tasks=([(12, 0)], ())),
    "one body": dict(parent=[-1], tasks=([(0, 0)], [(0, 0)])),
    "64 active dofs": dict(parent=list(range(-1, 58)), hinge=tuple(range(1, 59)), tasks=([(58, 0)], ())),
}


def test_small_blobs_plan(program, tmp_path):
    # structured and generic QP of each; a wider kernel variant (min_nvp) where the tree is not trivial
    cases = [(f"{name} {fg} {nvp}", synth_blob(**kw), nvp, fg) for name, kw in PLANS.items() for fg in (0, 1)
             for nvp in ((0, 64) if name in ("chain of 64 bodies", "planar base") else (0,))]
    res = mp.run_cases(program, cases, tmp_path)  # (the program checks the invariants of every plan)
    for key, r in res.items():
        assert r["code"] == OK and r["message"] == "" and r["digest"], (key, r)
    f = dict(zip(["nlimb", "ntask0", "ntask1", "use0", "use1", "same_tasks", "ncpass0", "ncpass1", "npairp", "nbody", "fkrounds", "n_act", "nslot",
                  "nq", "root_slot"], res["chain of 64 bodies 0 0"]["fields"]))
    assert (f["nbody"], f["fkrounds"], f["n_act"], f["nq"]) == (64, 6, 15, 16)
    f = res["planar base 0 0"]["fields"]
    assert f[11] == 16 and f[8] == 128 and f[5] == 1  # n_act: the three null dofs stay rows; same_tasks
    assert res["second table empty 0 0"]["fields"][4] == 0  # use1
    assert res["64 active dofs 0 0"]["fields"][11] == 64
    assert res["both tables empty 0 0"]["fields"][9] == 1  # nothing but the root is needed


def breaks(**changes):
    def edit(hdr, offs):
        for k, v in changes.items():
            (hdr if k in hdr else offs)[k] = v
    return edit


# (blob, code, message): the messages as the commit before model_plan.h spelt them (api.hip, build_device_model / model_create_impl)
def refusals():
    small = dict(parent=SMALL, hinge=SMALL_HINGES, tasks=(SMALL_TASKS, SMALL_TASKS), nslot=4)
    good = synth_blob(**small)
    hdr_end = gm.HEADER_BYTES
    return {
        "bodies out of depth-first order": (synth_blob(**dict(small, parent=[-1, 0, 3, 2, 3, 4, 2, 6, 7, 0, 9])), EINVAL,
                                            "bodies are not in depth-first order"),
        "a body that is its own parent": (synth_blob(**dict(small, parent=[-1, 0, 1, 3, 3, 4, 2, 6, 7, 0, 9])), EINVAL,
                                          "bodies are not in depth-first order"),
        "nq / nv mismatch": (synth_blob(**small, edit=breaks(nq=19, nv=18)), EINVAL, "nq/nv do not match the joint list"),
        "nq is not nv + 1": (synth_blob(**small, edit=breaks(nq=19)), EINVAL, "bad nq/nv"),
        "task body out of range": (synth_blob(**dict(small, tasks=(SMALL_TASKS, [(5, 0), (11, 1)]))), EINVAL, "task 1 of table 2 out of range"),
        "task slot out of range": (synth_blob(**dict(small, tasks=([(5, 4)], ()))), EINVAL, "task 0 of table 1 out of range"),
        "root mask": (synth_blob(**small, root_mask=0x3b), EUNSUPPORTED,
                      "root_dof_mask 0x3b: only a free joint (0x3f) or a planar base (0x23) is supported"),
        "hinge axis on the root": (set_axis_on_root(good), EINVAL, "the root body must not carry a hinge axis"),
        "65 active dofs": (synth_blob(parent=list(range(-1, 59)), hinge=tuple(range(1, 60)), tasks=([(59, 0)], ())), EUNSUPPORTED,
                           "65 active dofs exceed the kernel limit of 64"),
        "thirteen branch slots": (synth_blob(parent=bushy(13), tasks=([(13, 0)], ())), EUNSUPPORTED,
                                  "tree too bushy for the FK kernel (13 branch slots)"),
        "two roots": (synth_blob(parent=[-1, -1], tasks=((), ())), EINVAL, "bodies are not in depth-first order"),
        "body 0 with a parent": (synth_blob(parent=[0, 0], tasks=((), ())), EINVAL, "body 0 must be the free-joint root"),
        # truncated or mis-offset: refused before anything is read through the offsets
        "empty file": (b"", EINVAL, "blob too small"),
        "header cut short": (good[:hdr_end - 4], EINVAL, "blob too small"),
        "truncated": (good[:-8], EINVAL, "blob size mismatch"),
        "truncated, size patched": (good[:8] + struct.pack("<I", len(good) - 8) + good[12:-8], EINVAL, "blob array offsets out of range"),
        "bad magic": (b"XXXX" + good[4:], EINVAL, "bad blob magic/version"),
        "offset behind the end": (synth_blob(**small, edit=breaks(task_wr1=1 << 20)), EINVAL, "blob array offsets out of range"),
        "offset wraps with the length": (synth_blob(**small, edit=breaks(body_pos=0xfffffff8)), EINVAL, "blob array offsets out of range"),
        "offset inside the header": (synth_blob(**small, edit=breaks(parent=8)), EINVAL, "blob array offsets out of range"),
        "offset not a multiple of 8": (synth_blob(**small, edit=lambda h, o: o.update(jnt_range=o["jnt_range"] + 4)), EINVAL,
                                       "blob array offsets out of range"),
        "nbody of 65": (synth_blob(**small, edit=breaks(nbody=65)), EINVAL, "nbody outside [1, 64]"),
        "33 tasks": (synth_blob(**small, edit=breaks(ntask0=33)), EINVAL, "slot/task counts out of range"),
        "root slot": (synth_blob(**small, edit=breaks(root_slot=4)), EINVAL, "root_slot out of range"),
        "more bodies than the arrays hold": (synth_blob(**small, edit=breaks(nbody=64)), EINVAL, "blob array offsets out of range"),
    }


def test_refusals_keep_code_and_message(program, tmp_path):
    want = refusals()
    res = mp.run_cases(program, [(name, blob, 0, 0) for name, (blob, _, _) in want.items()], tmp_path)
    for name, (_, code, message) in want.items():
        assert (res[name]["code"], res[name]["message"]) == (code, message), name
        assert res[name]["digest"] is None


def test_the_library_refuses_a_blob_with_offsets_out_of_range():
    """gmr_debug_ik_shape used to read such a blob out of bounds; it answers -2 like any blob whose header is wrong."""
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    f = _native.load().gmr_debug_ik_shape
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_size_t] + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    small = dict(parent=SMALL, hinge=SMALL_HINGES, tasks=(SMALL_TASKS, SMALL_TASKS), nslot=4)
    for blob, rc in [(synth_blob(**small), -1), (synth_blob(**small, edit=breaks(task_wr1=1 << 20)), -2),
                     (synth_blob(**small, root_mask=0x3b), -3)]:
        assert f(blob, len(blob), 0, -1, 0, 0, 0, 1, None, None, 0) == rc


def test_composite_plan_of_too_many_passes(program):
    import subprocess
    r = subprocess.run([program, "--too-many-passes"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert r.stdout.strip() == f"{EUNSUPPORTED}|composite plan of table 1 needs more than 32 passes"


def test_headers_compile_without_the_hip_runtime():
    """model_plan.h and dev_model.h include no HIP runtime header (only the vector types), as the stand-alone build needs."""
    import os
    for name in ("model_plan.h", "dev_model.h"):
        text = open(os.path.join(mp.CSRC, name)).read()
        includes = [ln for ln in text.split("\n") if ln.lstrip().startswith("#include")]
        assert not [ln for ln in includes if "hip" in ln and "hip_vector_types.h" not in ln], name
