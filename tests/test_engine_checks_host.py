"""The argument checks the clip-wise calls of gmr_amd/engine.py share -- ``_qpos_rows``, ``_clip_offsets``, ``_named_outputs`` --
on CPU tensors, without a GPU: the accepting case and every refusing branch of each, with the exception class and the full message
as the calls raised them before the helpers existed.  The second half calls the ``_*_input`` front ends of contacts, foot
locking, inverse dynamics, self-collision and the tracking export with a stand-in engine on the CPU: the helpers are wired to the
right names and shapes, every pointer is bound, and a call with two faults raises the one it raised before.  A tensor on the
"meta" device stands for one on another device."""
import types

import numpy as np
import pytest
import torch

from gmr_amd import _native
from gmr_amd import engine as E
from gmr_amd.engine import EngineError

CPU = torch.device("cpu")
NQ = 10


def raises(cls, message, f, *a, **k):
    with pytest.raises(cls) as e:
        f(*a, **k)
    assert type(e.value) is cls and str(e.value) == message


# ---------------------------------------------------------------------------------------------------------------- _qpos_rows
QPOS_MSG = f"qpos must be a contiguous float64 [N, {NQ}] tensor on the engine's device"
QPOS_MSG_LOOSE = f"qpos must be a float64 [N, {NQ}] tensor on the engine's device"

BAD_QPOS = {
    "type": lambda: np.zeros((5, NQ)),
    "device": lambda: torch.zeros((5, NQ), dtype=torch.float64, device="meta"),
    "dtype": lambda: torch.zeros((5, NQ), dtype=torch.float32),
    "rank": lambda: torch.zeros((5 * NQ,), dtype=torch.float64),
    "rank3": lambda: torch.zeros((5, NQ, 1), dtype=torch.float64),
    "width": lambda: torch.zeros((5, NQ + 1), dtype=torch.float64),
}


def test_qpos_rows_accepts():
    assert E._qpos_rows(torch.zeros((5, NQ), dtype=torch.float64), NQ, CPU) == 5
    assert E._qpos_rows(torch.zeros((0, NQ), dtype=torch.float64), NQ, CPU) == 0
    n = E._qpos_rows(torch.zeros((5, NQ), dtype=torch.float64, device="meta"), NQ, torch.device("meta"))
    assert n == 5 and type(n) is int


@pytest.mark.parametrize("fault", sorted(BAD_QPOS))
def test_qpos_rows_refuses(fault):
    raises(EngineError, QPOS_MSG, E._qpos_rows, BAD_QPOS[fault](), NQ, CPU)
    raises(EngineError, "robot 1: " + QPOS_MSG_LOOSE, E._qpos_rows, BAD_QPOS[fault](), NQ, CPU, "robot 1: ", contiguous=False)


def test_qpos_rows_contiguity():
    q = torch.zeros((5, 2 * NQ), dtype=torch.float64)[:, ::2]
    assert tuple(q.shape) == (5, NQ) and not q.is_contiguous()
    raises(EngineError, QPOS_MSG, E._qpos_rows, q, NQ, CPU)
    assert E._qpos_rows(q, NQ, CPU, contiguous=False) == 5   # the epilogue, the tracking export and the clip report copy it themselves


# ---------------------------------------------------------------------------------------------------------------- _clip_offsets
def offsets_messages(name):
    return f"{name} must be a contiguous 1-D int64 tensor (or a host sequence)", f"{name} must hold n_seq + 1 entries"


def test_clip_offsets_accepts():
    t = torch.tensor([0, 3, 5], dtype=torch.int64)
    assert E._clip_offsets(t, CPU) is t                      # a device tensor is taken as it is: no copy
    for host in ([0, 3, 5], (0, 3, 5), np.array([0, 3, 5], dtype=np.int32), [0]):
        got = E._clip_offsets(host, CPU)
        assert got.dtype == torch.int64 and got.device == CPU and got.tolist() == list(host)
    assert E._clip_offsets(torch.tensor([0], dtype=torch.int64), CPU, "out_offsets").tolist() == [0]


@pytest.mark.parametrize("name", ["seq_offsets", "out_offsets"])
def test_clip_offsets_refuses(name):
    tensor_msg, host_msg = offsets_messages(name)
    args = (CPU,) if name == "seq_offsets" else (CPU, name)
    bad_tensors = {
        "device": torch.zeros(3, dtype=torch.int64, device="meta"),
        "dtype": torch.zeros(3, dtype=torch.int32),
        "rank": torch.zeros((3, 1), dtype=torch.int64),
        "empty": torch.zeros(0, dtype=torch.int64),
        "non-contiguous": torch.zeros(6, dtype=torch.int64)[::2],
    }
    for t in bad_tensors.values():
        raises(EngineError, tensor_msg, E._clip_offsets, t, *args)
    for host in ([], (), [[0, 3], [3, 5]], np.zeros((0,), dtype=np.int64)):
        raises(ValueError, host_msg, E._clip_offsets, host, *args)


# ---------------------------------------------------------------------------------------------------------------- _named_outputs
FIELDS = ("contact", "frames", "base")     # three of gmr_contact_input's outputs: the binding is checked on the real structure
SHAPES = {"contact": ((6, 2), torch.uint8), "frames": ((3, 2), torch.int32), "base": ((3,), torch.float64)}
OUT_MSG = "out must map names of X_FIELDS to contiguous tensors of the call's shapes on the engine's device"


def zeros(k, sh, dt):
    return torch.zeros(sh, dtype=dt)


def good_out():
    return {k: torch.zeros(sh, dtype=dt) for k, (sh, dt) in SHAPES.items()}


def bound(inp, name):
    return getattr(inp, name + "_out") or 0


def test_named_outputs_allocates_and_binds():
    ci = _native.ContactInput()
    res = E._named_outputs(ci, None, FIELDS, SHAPES, CPU, "X_FIELDS", zeros)
    assert list(res) == list(FIELDS)
    for k, (sh, dt) in SHAPES.items():
        assert tuple(res[k].shape) == sh and res[k].dtype == dt and bound(ci, k) == res[k].data_ptr() != 0
    assert bound(ci, "touchdowns") == 0
    # alloc may leave a name out
    ci = _native.ContactInput()
    res = E._named_outputs(ci, None, FIELDS, SHAPES, CPU, "X_FIELDS", lambda k, sh, dt: None if k == "frames" else zeros(k, sh, dt))
    assert list(res) == ["contact", "base"] and bound(ci, "frames") == 0 and bound(ci, "base") == res["base"].data_ptr()


def test_named_outputs_takes_the_callers():
    out = good_out()
    ci = _native.ContactInput()
    res = E._named_outputs(ci, dict(reversed(list(out.items()))), FIELDS, SHAPES, CPU, "X_FIELDS", None)
    assert list(res) == list(FIELDS) and all(res[k] is out[k] and bound(ci, k) == out[k].data_ptr() for k in FIELDS)
    ci = _native.ContactInput()
    res = E._named_outputs(ci, {"base": out["base"]}, FIELDS, SHAPES, CPU, "X_FIELDS", None)   # a name left out is not computed
    assert list(res) == ["base"] and bound(ci, "contact") == 0 and bound(ci, "base") == out["base"].data_ptr()
    assert E._named_outputs(_native.ContactInput(), {}, FIELDS, SHAPES, CPU, "X_FIELDS", None) == {}


BAD_OUT = {
    "unknown name": lambda o: o.update(touchdowns=torch.zeros((3, 2), dtype=torch.int32)),
    "type": lambda o: o.update(base=np.zeros(3)),
    "shape": lambda o: o.update(frames=torch.zeros((3, 3), dtype=torch.int32)),
    "rank": lambda o: o.update(base=torch.zeros((3, 1), dtype=torch.float64)),
    "dtype": lambda o: o.update(base=torch.zeros(3, dtype=torch.float32)),
    "device": lambda o: o.update(base=torch.zeros(3, dtype=torch.float64, device="meta")),
    "non-contiguous": lambda o: o.update(frames=torch.zeros((3, 4), dtype=torch.int32)[:, ::2]),
}


@pytest.mark.parametrize("fault", sorted(BAD_OUT))
def test_named_outputs_refuses(fault):
    out = good_out()
    BAD_OUT[fault](out)
    raises(EngineError, OUT_MSG, E._named_outputs, _native.ContactInput(), out, FIELDS, SHAPES, CPU, "X_FIELDS", None)
    raises(EngineError, "robot 1: " + OUT_MSG.replace("the call's", "the plan's"), E._named_outputs, _native.ContactInput(), out, FIELDS, SHAPES,
           CPU, "X_FIELDS", None, whose="the plan's", what="robot 1: ")


# ---------------------------------------------------------------------------------------------------------------- the front ends
NB, S, N = 4, 2, 6
OFFS = [0, 4, 6]


def fake_engine():
    f64 = torch.float64
    inertial = {"body_parent": torch.zeros(NB, dtype=torch.int32), "body_mass": torch.ones(NB, dtype=f64), "body_com": torch.zeros((NB, 3), dtype=f64),
                "body_inertia": torch.ones((NB, 6), dtype=f64), "armature": torch.zeros(NQ - 7, dtype=f64), "torque_limit": torch.ones(NQ - 7, dtype=f64)}
    proxies = {"cap_body": torch.zeros(3, dtype=torch.int32), "cap_p0": torch.zeros((3, 3), dtype=f64), "cap_p1": torch.zeros((3, 3), dtype=f64),
               "cap_radius": torch.ones(3, dtype=f64), "pairs": torch.zeros((2, 2), dtype=torch.int32)}
    return types.SimpleNamespace(device=CPU, nq=NQ, nbody=NB, inertial_device=lambda table: inertial, collision_device=lambda c, p: proxies)


def qpos(n=N):
    return torch.zeros((n, NQ), dtype=torch.float64)


def contacts(out=None, offsets=OFFS, pos=None):
    pos = torch.zeros((N, NB, 3), dtype=torch.float32) if pos is None else pos
    return E._contact_input(fake_engine(), (pos, torch.zeros((N, NB, 3), dtype=torch.float32)), offsets, [1, 3], None, "clip_min", 0.03, 0.05, 0.3, 0.6, out)


def footlock(q=None, offsets=OFFS, out=None):
    return E._footlock_input(fake_engine(), qpos() if q is None else q, offsets, torch.zeros((N, 2), dtype=torch.uint8), [1, 3], 5, 2, 8, 1e-6, 0.2, out)


def dynamics(q=None, offsets=OFFS, out=None, qvel=None):
    return E._dynamics_input(fake_engine(), qpos() if q is None else q, offsets, 30.0, qvel, None, (0.0, 0.0, -9.81), 0.0, 0.05, None, out)


def self_collision(q=None, offsets=OFFS, out=None, stats=True, margin=0.0):
    return E._self_collision_input(fake_engine(), qpos() if q is None else q, offsets, None, None, margin, out, stats)


def track(q=None, out=None, bodies=True, what=""):
    return E._track_input(fake_engine(), qpos() if q is None else q, OFFS, 30.0, 30.0, out, bodies, what=what)


CALLS = {"contacts": (contacts, E.CONTACT_FIELDS, "CONTACT_FIELDS"), "footlock": (footlock, E.FOOTLOCK_FIELDS, "FOOTLOCK_FIELDS"),
         "dynamics": (dynamics, E.DYNAMICS_FIELDS, "DYNAMICS_FIELDS"), "self_collision": (self_collision, E.SELF_COLLISION_FIELDS, "SELF_COLLISION_FIELDS"),
         "track": (track, E.TRACK_FIELDS, "TRACK_FIELDS")}


@pytest.mark.parametrize("call", sorted(CALLS))
def test_front_end_allocates_every_field_and_binds_it(call):
    f, fields, _ = CALLS[call]
    inp, res, _ = f()
    assert list(res) == list(fields)
    assert all(bound(inp, k) == res[k].data_ptr() != 0 for k in fields)
    # the caller's own tensors, in any order, come back in the fields' order; one left out stays NULL
    out = dict(reversed(list(res.items())))
    if call == "footlock":
        out["qpos"] = torch.ones_like(out["qpos"])
    last = fields[-1]
    del out[last]
    inp2, res2, _ = f(out=out)
    assert list(res2) == list(fields[:-1]) and all(res2[k] is out[k] and bound(inp2, k) == out[k].data_ptr() for k in res2)
    assert bound(inp2, last) == 0


@pytest.mark.parametrize("call", sorted(CALLS))
def test_front_end_refuses_outputs_with_its_own_message(call):
    f, fields, name = CALLS[call]
    whose = "the plan's" if call == "track" else "the call's"
    msg = f"out must map names of {name} to contiguous tensors of {whose} shapes on the engine's device"
    _, res, _ = f()
    raises(EngineError, msg, f, out={**res, "nonsense": res[fields[0]]})
    raises(EngineError, msg, f, out={fields[0]: res[fields[0]].to(torch.float16)})
    raises(EngineError, msg, f, out={fields[0]: res[fields[0]][:-1]})


def test_front_end_shapes_and_fills():
    _, res, _ = contacts()
    assert {k: (tuple(t.shape), t.dtype) for k, t in res.items()} == {
        "contact": ((N, 2), torch.uint8), "frames": ((S, 2), torch.int32), "touchdowns": ((S, 2), torch.int32), "slide_sum": ((S, 2), torch.float64),
        "slide_step_max": ((S, 2), torch.float64), "depth_max": ((S, 2), torch.float64), "airborne_frames": ((S,), torch.int32), "base": ((S,), torch.float64)}
    # a call without rows: base is what an empty clip reports
    _, res, _ = E._contact_input(fake_engine(), (torch.zeros((0, NB, 3), dtype=torch.float32),) * 2, [0, 0, 0], [1], None, "clip_min", 0.03, 0.05, 0.3, 0.6, None)
    assert torch.isnan(res["base"]).all()
    q = torch.arange(N * NQ, dtype=torch.float64).reshape(N, NQ)
    _, res, _ = footlock(q)
    assert torch.equal(res["qpos"], q) and res["qpos"].data_ptr() != q.data_ptr() and not res["shift"].any()
    _, res, _ = self_collision(stats=False)
    assert list(res) == list(_native.SELF_COLLISION_FRAME_OUTPUTS)
    _, res, _ = self_collision()
    assert torch.isnan(res["clearance"]).all() and (res["pair"] == -1).all() and torch.isinf(res["clearance_min"]).all() and not res["hits"].any()
    _, res, _ = track(bodies=False)
    assert list(res) == [k for k in E.TRACK_FIELDS if not k.startswith("body_")]
    _, res, _ = track()
    assert res["body_pos_w"].dtype == torch.float32 and tuple(res["body_quat_w"].shape) == (N, NB, 4) and res["joint_pos"].dtype == torch.float64


def test_front_end_rules_behind_the_shared_check():
    _, res, _ = footlock()
    raises(EngineError, "out must hold qpos, pos and shift: the three are required", footlock, out={"qpos": res["qpos"], "pos": res["pos"]})
    q = qpos()
    raises(EngineError, "out['qpos'] must not alias qpos", footlock, q, out={"qpos": q, "pos": res["pos"], "shift": res["shift"]})
    _, res, _ = dynamics()
    raises(EngineError, "out must hold tau and root_wrench when it holds a statistic: the statistics are reduced from them", dynamics,
           out={"tau": res["tau"], "tau_rms": res["tau_rms"]})
    _, res, _ = self_collision()
    raises(EngineError, "out must hold clearance, pair and hits when it holds a statistic: the statistics are reduced from them", self_collision,
           out={"clearance": res["clearance"], "hits_sum": res["hits_sum"]})


def test_front_end_order_of_checks():
    """A call with two faults raises the one that came first before the helpers existed."""
    bad_q, bad_offs, bad_out = qpos().to(torch.float32), torch.zeros(3, dtype=torch.int32), {"nonsense": qpos()}
    seq_tensor, seq_host = offsets_messages("seq_offsets")
    for f in (footlock, dynamics, self_collision):
        raises(EngineError, QPOS_MSG, f, bad_q, bad_offs, bad_out)           # qpos before the offsets
        raises(EngineError, seq_tensor, f, None, bad_offs, bad_out)          # the offsets before the outputs
        raises(ValueError, seq_host, f, None, [], bad_out)
    # inverse dynamics: qvel between qpos and the offsets; its parameters before the outputs
    raises(EngineError, f"qvel must be a contiguous float64 [{N}, {NQ - 1}] tensor on the engine's device (or None)", dynamics, None, bad_offs, bad_out,
           qvel=torch.zeros((N, NQ), dtype=torch.float64))
    raises(ValueError, "margin must be finite", self_collision, None, OFFS, bad_out, margin=float("nan"))
    # contacts: the arrays before the offsets, which take the argument's name
    out_tensor, out_host = offsets_messages("out_offsets")
    raises(EngineError, f"body_pos_w and body_lin_vel_w must be contiguous float32 [M, {NB}, 3] tensors on the engine's device", contacts, bad_out,
           bad_offs, torch.zeros((N, NB, 3), dtype=torch.float64))
    raises(EngineError, out_tensor, contacts, bad_out, bad_offs)
    raises(ValueError, out_host, contacts, bad_out, [])
    # the tracking export: qpos with the member's prefix and without "contiguous" -- it copies a strided qpos itself
    raises(EngineError, "robot 2: " + QPOS_MSG_LOOSE, track, bad_q, bad_out, what="robot 2: ")
    raises(EngineError, "robot 2: out must map names of TRACK_FIELDS to contiguous tensors of the plan's shapes on the engine's device", track, None,
           bad_out, what="robot 2: ")
    strided = torch.zeros((N, 2 * NQ), dtype=torch.float64)[:, ::2]
    inp, _, keep = track(strided)
    assert keep[0].is_contiguous() and inp.qpos == keep[0].data_ptr()
