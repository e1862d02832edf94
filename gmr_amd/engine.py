"""Torch-facing wrapper of one native model handle.

PyTorch is plumbing here: device buffers, the current HIP stream, and (elsewhere)
``torch.distributed``.  All arithmetic happens in libgmr_amd.so's kernels.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional

import numpy as np
import torch

from . import _native
from ._native import IKParams, IKStats, ModelInfo
from .model import CompiledModel

_ERR = {-1: "invalid argument", -2: "HIP runtime error", -3: "model not supported by the kernels", -4: "model has no IK config"}


class EngineError(RuntimeError):
    pass


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _qpos_rows(qpos, nq: int, device, what: str = "", contiguous: bool = True) -> int:
    """Check a call's qpos -- a float64 ``[N, nq]`` tensor on ``device``, contiguous unless the caller makes it so -- and return N.
    ``what`` prefixes the message (a group member)."""
    if not isinstance(qpos, torch.Tensor) or qpos.device != device or qpos.dtype != torch.float64 or qpos.dim() != 2 \
            or qpos.shape[1] != nq or (contiguous and not qpos.is_contiguous()):
        raise EngineError(what + f"qpos must be a {'contiguous ' if contiguous else ''}float64 [N, {nq}] tensor on the engine's device")
    return int(qpos.shape[0])


def _clip_offsets(offsets, device, name: str = "seq_offsets") -> torch.Tensor:
    """The clips' row offsets ``[S + 1]`` on ``device``: a device int64 tensor as it is, or a host sequence uploaded once.  The
    messages carry the argument's ``name``: "seq_offsets must be a contiguous 1-D int64 tensor (or a host sequence)"."""
    if isinstance(offsets, torch.Tensor):
        if offsets.device != device or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1 or not offsets.is_contiguous():
            raise EngineError(f"{name} must be a contiguous 1-D int64 tensor (or a host sequence)")
        return offsets
    o = np.ascontiguousarray(offsets, dtype=np.int64)
    if o.ndim != 1 or o.size < 1:
        raise ValueError(f"{name} must hold n_seq + 1 entries")
    return torch.from_numpy(o).to(device)  # the one upload of the call


def _named_outputs(inp, out, fields, shapes, device, fields_name: str, alloc, whose: str = "the call's", what: str = "") -> dict:
    """The result tensors of a call by name, in the order of ``fields``, each bound to ``inp``'s pointer ``name + "_out"``.
    ``shapes``: ``{name: (shape, dtype)}``.  With ``out`` -- a mapping of caller-owned tensors; a name left out is not computed -- the
    tensors are checked against it; without, ``alloc(name, shape, dtype)`` makes each (``None``: the name is left out)."""
    if out is None:
        made = ((k, alloc(k, *shapes[k])) for k in fields)
        res = {k: t for k, t in made if t is not None}
    else:
        res = {k: out[k] for k in fields if k in out}
        if set(out) - set(fields) or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[k][0] or t.dtype != shapes[k][1]
                                         or t.device != device or not t.is_contiguous() for k, t in res.items()):
            raise EngineError(what + f"out must map names of {fields_name} to contiguous tensors of {whose} shapes on the engine's device")
    for k, t in res.items():
        setattr(inp, k + "_out", t.data_ptr())
    return res


def _state_arrays(nq: int, device, items: np.ndarray, qpos_init: Optional[torch.Tensor], qpos_final: Optional[torch.Tensor], n_final: int,
                  frames_done: Optional[torch.Tensor], what: str = ""):
    """Host-side checks of a batch's state arrays against its work items -- the C side cannot check row counts, and on the device a
    wrong row is an out-of-bounds write.  Returns (qpos_init, qpos_final): qpos_init made contiguous, qpos_final allocated with
    ``n_final`` rows (zeros) when the caller gives none.  ``what`` prefixes the error messages (a group member)."""
    if qpos_final is not None:
        if qpos_final.dtype != torch.float64 or qpos_final.dim() != 2 or qpos_final.shape[1] != nq or not qpos_final.is_contiguous() \
                or qpos_final.device != device:
            raise EngineError(what + "qpos_final must be a contiguous float64 [R, nq] tensor on the engine's device")
        qfin, n_final = qpos_final, int(qpos_final.shape[0])
    else:
        qfin = torch.zeros((n_final, nq), dtype=torch.float64, device=device) if n_final > 0 else None
    if qpos_init is not None:
        if qpos_init.dtype != torch.float64 or qpos_init.dim() != 2 or qpos_init.shape[1] != nq or qpos_init.device != device:
            raise EngineError(what + "qpos_init must be float64 [R, nq] on the engine's device")
        if not qpos_init.is_contiguous():
            qpos_init = qpos_init.contiguous()
        if len(items) and int(items["init_row"].max()) >= qpos_init.shape[0]:
            raise EngineError(what + "init_row outside qpos_init")
    if len(items):
        reach = np.where(items["check_stride"] > 0, (np.maximum(items["n_out"], 1) - 1) // np.maximum(items["check_stride"], 1), 0)
        if int(max((items["final_row"] + reach).max(), (items["burn_row"] + reach).max())) >= n_final:
            raise EngineError(what + "final_row outside qpos_final")
    if frames_done is not None and (frames_done.dtype != torch.int32 or frames_done.device != device or not frames_done.is_contiguous()
                                    or frames_done.numel() < len(items)):
        raise EngineError(what + "frames_done must be a contiguous int32 [n_items] tensor on the engine's device")
    return qpos_init, qfin


def _ik_batch(eng: "Engine", pos: torch.Tensor, quat: torch.Tensor, slot_col, items, *, out=None, iters=None, want_iters: bool = True,
              qpos_init=None, qpos_final=None, n_final: int = 0, frames_done=None, host_out: bool = False, with_outputs: bool = True,
              what: str = ""):
    """Check one model's key-point batch and give it the form the library takes: contiguous tensors, ``slot_col`` int32, ``items`` as
    work-item records, ``out`` (NaN) / ``iters`` / ``qpos_final`` allocated where the caller gives none.  ``host_out``: ``out`` may be
    pinned host memory; ``with_outputs=False`` (a probe) leaves ``out`` / ``iters`` alone.  ``what`` prefixes the error messages (a group
    member).  Returns (pos, quat, slot_col, items, out, iters, qpos_init, qpos_final)."""
    if pos.device != eng.device or quat.device != eng.device:
        raise EngineError(what + "inputs must live on the engine's device")
    if pos.dtype != quat.dtype or pos.dtype not in (torch.float32, torch.float64):
        raise EngineError(what + "pos/quat must both be float32 or both float64")
    if pos.dim() != 3 or quat.dim() != 3 or pos.shape[2] != 3 or quat.shape[2] != 4 or pos.shape[:2] != quat.shape[:2]:
        raise EngineError(what + f"bad input shapes {tuple(pos.shape)} / {tuple(quat.shape)}")
    pos, quat = pos.contiguous(), quat.contiguous()
    N = int(pos.shape[0])
    items = np.ascontiguousarray(items, dtype=_native.WORK_ITEM_DTYPE)
    slot_col = np.ascontiguousarray(slot_col, dtype=np.int32)
    if slot_col.shape != (eng.info.nslot,):
        raise EngineError(what + "slot_col has the wrong length")
    if with_outputs:
        if out is None:
            out = torch.full((N, eng.nq), float("nan"), dtype=torch.float64, device=eng.device)
        elif out.shape != (N, eng.nq) or out.dtype != torch.float64 or not out.is_contiguous() or \
                (out.device != eng.device and not (host_out and out.is_pinned())):
            raise EngineError(what + "out must be a contiguous float64 [N, nq] tensor on the engine's device")
        if iters is None:
            iters = torch.zeros(N, dtype=torch.int32, device=eng.device) if want_iters else None
        elif iters.shape != (N,) or iters.dtype != torch.int32 or not iters.is_contiguous() or iters.device != eng.device:
            raise EngineError(what + "iters must be a contiguous int32 [N] tensor on the engine's device")
    qpos_init, qfin = _state_arrays(eng.nq, eng.device, items, qpos_init, qpos_final, n_final, frames_done, what)
    return pos, quat, slot_col, items, out, iters, qpos_init, qfin


def _launch_order(eng: "Engine", launch_order, item_arrays, plan, sliced: bool = False):
    """What an ``ik_solve`` launches by: ``None`` or a checked order tensor.  ``item_arrays``: the work items of the launch (one array per
    model); ``"auto"`` asks ``eng``'s probe policy about all of them together and has ``plan(probe_frames)`` make the order.  ``sliced``:
    the launch is a model's own ``gmr_ik_solve``, which may cut the batch into slices instead (a group launch never does)."""
    total = sum(len(it) for it in item_arrays)
    if isinstance(launch_order, str):
        if launch_order != "auto":
            raise EngineError("launch_order must be a tensor, None or 'auto'")
        pf = eng._probe_frames(np.concatenate(item_arrays), sliced=sliced)
        launch_order = plan(pf) if pf else None
    if launch_order is not None and (not isinstance(launch_order, torch.Tensor) or launch_order.dtype != torch.int32
                                     or launch_order.device != eng.device or not launch_order.is_contiguous() or launch_order.numel() != total):
        raise EngineError(f"launch_order must be a contiguous int32 [{total}] tensor on the engine's device (one entry per work item)")
    return launch_order


def _chunk_params(params: Optional[IKParams], eps: float) -> IKParams:
    """``params`` with the verification walks' tolerance ``eps``."""
    prm = params or IKParams()
    return IKParams(prm.damping, prm.tol, prm.limit_gain, prm.lm_damping, prm.max_iter, prm.offset_to_ground, eps)


def _chunk_batch(pos, quat, slot_col, offs, chunk: int, burn_in: int, height_scales, chunk_init: int, clip_init: int) -> dict:
    """Launch 1 of a chunked solve as an ``ik_solve`` batch: the tracked chunk items of the clips ``offs`` and room for their states."""
    from .schedule import make_items
    items = make_items(offs, chunk=chunk, burn_in=burn_in, track=True, height_scales=height_scales, chunk_init=chunk_init, clip_init=clip_init)
    return {"pos": pos, "quat": quat, "slot_col": slot_col, "items": items, "n_final": 2 * len(items)}


def _walk_batch(first: dict, res, offs, chunk: int):
    """Launch 2 from launch 1's batch and its results (qpos, iters, qpos_final): the verification walks writing into the same arrays, or
    ``None`` where there is nothing to walk.  Returns (batch, info); ``info()`` -- to be called after launch 2 -- is the chunked solve's
    info dict."""
    from .schedule import plan_walks
    items = first["items"]
    walks = plan_walks(items, offs, chunk) if len(items) else items
    if len(walks) == 0:
        return None, lambda: {"chunks": len(items), "passes": 0, "resolved_frames": 0}
    done = torch.zeros(len(walks), dtype=torch.int32, device=res[0].device)
    batch = {"pos": first["pos"], "quat": first["quat"], "slot_col": first["slot_col"], "items": walks, "qpos_init": res[2], "qpos_final": res[2],
             "out": res[0], "iters": res[1], "frames_done": done}
    return batch, lambda: {"chunks": len(items), "passes": 1, "resolved_frames": int(done.sum().item())}


def _motion_input(eng: "Engine", qpos: torch.Tensor, seq_offsets, height_adjust: bool, root_origin_offset: bool, ground_offset: float,
                  out, min_z: Optional[torch.Tensor], what: str = ""):
    """Check one model's epilogue arguments and fill its ``MotionInput``.  Returns (input, (root_pos, root_rot, dof_pos,
    local_body_pos), keep-alive)."""
    N = _qpos_rows(qpos, eng.nq, eng.device, what, contiguous=False)
    qpos = qpos.contiguous()
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if offs.ndim != 1 or len(offs) < 2 or offs[0] != 0 or offs[-1] != N:
        raise ValueError(what + "seq_offsets must span [0, N]")
    if (np.diff(offs) < 0).any():
        raise ValueError(what + "seq_offsets must not decrease")
    shapes = ((N, 3, torch.float64), (N, 4, torch.float64), (N, eng.nq - 7, torch.float64), (N, eng.nbody, 3, torch.float32))
    if out is None:
        res = tuple(torch.empty(sh[:-1], dtype=sh[-1], device=eng.device) for sh in shapes)
    else:
        res = tuple(out)
        if len(res) != 4 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != sh[:-1] or t.dtype != sh[-1] or t.device != eng.device
                                or not t.is_contiguous() for t, sh in zip(res, shapes)):
            raise EngineError(what + "out must be contiguous (root_pos f64 [N, 3], root_rot f64 [N, 4], dof_pos f64 [N, nq-7], "
                                     "local_body_pos f32 [N, nbody, 3]) on the engine's device")
    if min_z is not None and (min_z.device != eng.device or min_z.dtype != torch.float32 or tuple(min_z.shape) != (len(offs) - 1,)
                              or not min_z.is_contiguous()):
        raise EngineError(what + "min_z must be a contiguous float32 [n_seq] tensor on the engine's device")
    mi = _native.MotionInput()
    mi.qpos, mi.n_frames = qpos.data_ptr(), N
    mi.seq_offsets, mi.n_seq = offs.ctypes.data, len(offs) - 1
    mi.flags = (_native.MOTION_HEIGHT_ADJUST if height_adjust else 0) | (_native.MOTION_ROOT_ORIGIN if root_origin_offset else 0)
    mi.ground_offset = float(ground_offset)
    mi.root_pos_out, mi.root_rot_out, mi.dof_pos_out = (t.data_ptr() for t in res[:3])
    mi.local_body_pos_out = res[3].data_ptr()
    mi.min_z_out = None if min_z is None else min_z.data_ptr()
    return mi, res, (qpos, offs)


TRACK_FIELDS = _native.TRACK_OUTPUTS   # the arrays of a tracking export, in gmr_track_input's order
_TRACK_BODY_FIELDS = ("body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")


class MotionTrack(dict):
    """Result of ``motion_track``: the device tensors by name (``TRACK_FIELDS``; the four body arrays only with ``bodies``), plus
    ``out_offsets`` (int64 numpy ``[S + 1]``: clip s owns the rows ``out_offsets[s]:out_offsets[s + 1]``) and ``fps`` as attributes."""

    def __init__(self, tensors, out_offsets, fps):
        super().__init__(tensors)
        self.out_offsets = out_offsets
        self.fps = fps


def _track_input(eng: "Engine", qpos: torch.Tensor, seq_offsets, fps_in, fps_out, out, bodies: bool, what: str = "",
                 lowpass_hz=0.0):
    """Check one model's tracking arguments, plan the resampling and fill its ``TrackInput``.  Returns (input, MotionTrack,
    keep-alive)."""
    from .schedule import lowpass_check, track_plan
    N = _qpos_rows(qpos, eng.nq, eng.device, what, contiguous=False)
    qpos = qpos.contiguous()
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if offs.ndim != 1 or len(offs) < 2 or offs[0] != 0 or offs[-1] != N:
        raise ValueError(what + "seq_offsets must span [0, N]")
    try:
        out_offs, ratio = track_plan(offs, fps_in, fps_out)
        lowpass_hz = lowpass_check(offs, fps_in, fps_out, lowpass_hz, ratio=ratio)
    except ValueError as e:
        raise EngineError(what + f"gmr_motion_track: {_ERR[-1]}: {e}") from None
    M = int(out_offs[-1])
    nd, nb = eng.nq - 7, eng.nbody
    f64, f32 = torch.float64, torch.float32
    shapes = {"root_pos": ((M, 3), f64), "root_rot": ((M, 4), f64), "joint_pos": ((M, nd), f64), "root_lin_vel": ((M, 3), f64),
              "root_ang_vel": ((M, 3), f64), "joint_vel": ((M, nd), f64), "body_pos_w": ((M, nb, 3), f32), "body_quat_w": ((M, nb, 4), f32),
              "body_lin_vel_w": ((M, nb, 3), f32), "body_ang_vel_w": ((M, nb, 3), f32)}
    fields = [k for k in TRACK_FIELDS if bodies or k not in _TRACK_BODY_FIELDS]
    ti = _native.TrackInput()
    res = _named_outputs(ti, out, fields, shapes, eng.device, "TRACK_FIELDS", lambda k, sh, dt: torch.empty(sh, dtype=dt, device=eng.device),
                         whose="the plan's", what=what)
    ti.qpos, ti.n_frames = qpos.data_ptr(), N
    ti.seq_offsets, ti.out_offsets, ti.ratio, ti.n_seq = offs.ctypes.data, out_offs.ctypes.data, ratio.ctypes.data, len(offs) - 1
    ti.fps_out = float(fps_out)
    ti.lowpass_hz = lowpass_hz
    return ti, MotionTrack(res, out_offs, fps_out), (qpos, offs, out_offs, ratio)


class MotionSample(dict):
    """Result of ``motion_sample``: the device tensors by name (``TRACK_FIELDS``), ``[E, K, ...]`` for 2-D times, else ``[Q, ...]``."""


def _sample_input(eng: "Engine", qpos, seq_offsets_dev, fps_dev, ids, times, k_per_id, bodies, fields, out, dtype):
    """Check the arguments of one query call and fill its ``SampleInput``.  Returns (input, MotionSample, keep-alive).  Nothing
    here touches the device: shapes and dtypes only."""
    dev = eng.device
    N = _qpos_rows(qpos, eng.nq, dev)
    for t, dt, what in ((seq_offsets_dev, torch.int64, "seq_offsets_dev"), (fps_dev, torch.float64, "fps_dev"), (ids, torch.int64, "ids")):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
            raise EngineError(f"{what} must be a contiguous 1-D {dt} tensor on the engine's device")
    n_seq = int(fps_dev.shape[0])
    if int(seq_offsets_dev.shape[0]) != n_seq + 1:
        raise EngineError("seq_offsets_dev must hold one entry more than fps_dev")
    if not isinstance(times, torch.Tensor) or times.device != dev or times.dtype not in (torch.float32, torch.float64) \
            or times.dim() not in (1, 2) or not times.is_contiguous():
        raise EngineError("times must be a contiguous float32 / float64 [Q] or [E, K] tensor on the engine's device")
    if dtype not in (torch.float32, torch.float64):
        raise EngineError("dtype must be torch.float32 or torch.float64")
    k_per_id = int(k_per_id)
    if times.dim() == 2:
        if k_per_id not in (1, int(times.shape[1])):
            raise EngineError("k_per_id must equal the second dimension of 2-D times")
        k_per_id = int(times.shape[1])
    lead = tuple(times.shape)
    Q = int(times.numel())
    if k_per_id < 1 or int(ids.shape[0]) * k_per_id != Q:
        raise EngineError("ids must hold one entry per k_per_id times")
    if bodies is not None:
        if not isinstance(bodies, torch.Tensor) or bodies.device != dev or bodies.dtype != torch.int32 or bodies.dim() != 1 or not bodies.is_contiguous():
            raise EngineError("bodies must be a contiguous 1-D int32 tensor of body indices on the engine's device")
    nd, nc = eng.nq - 7, eng.nbody if bodies is None else int(bodies.shape[0])
    tail = {"root_pos": (3,), "root_rot": (4,), "joint_pos": (nd,), "root_lin_vel": (3,), "root_ang_vel": (3,), "joint_vel": (nd,),
            "body_pos_w": (nc, 3), "body_quat_w": (nc, 4), "body_lin_vel_w": (nc, 3), "body_ang_vel_w": (nc, 3)}
    want = list(TRACK_FIELDS) if fields is None else list(fields)
    if set(want) - set(TRACK_FIELDS):
        raise EngineError("fields must name arrays of TRACK_FIELDS")
    dt_of = lambda k: torch.float32 if k in _TRACK_BODY_FIELDS else dtype
    if out is None:
        res = {k: torch.empty(lead + tail[k], dtype=dt_of(k), device=dev) for k in TRACK_FIELDS if k in want}
    else:
        res = {k: out[k] for k in TRACK_FIELDS if k in out and k in want}
        if set(out) - set(TRACK_FIELDS) or (fields is not None and set(want) - set(out)) \
                or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != lead + tail[k] or t.dtype != dt_of(k) or t.device != dev
                       or not t.is_contiguous() for k, t in res.items()):
            raise EngineError("out must map names of TRACK_FIELDS to contiguous tensors of the query's shapes on the engine's device")
    si = _native.SampleInput()
    si.qpos, si.n_frames = qpos.data_ptr(), N
    si.seq_offsets, si.fps, si.n_seq, si.k_per_id = seq_offsets_dev.data_ptr(), fps_dev.data_ptr(), n_seq, k_per_id
    si.ids, si.times, si.n_queries = ids.data_ptr(), times.data_ptr(), Q
    si.time_dtype = _native.GMR_DTYPE_F64 if times.dtype == torch.float64 else _native.GMR_DTYPE_F32
    si.out_dtype = _native.GMR_DTYPE_F64 if dtype == torch.float64 else _native.GMR_DTYPE_F32
    if bodies is not None:
        si.body_ids, si.n_sel = bodies.data_ptr(), nc
    for k, t in res.items():
        setattr(si, k + "_out", t.data_ptr())
    return si, MotionSample(res), (qpos, seq_offsets_dev, fps_dev, ids, times, bodies)


CONTACT_FIELDS = _native.CONTACT_OUTPUTS   # the arrays of the contact labels, in gmr_contact_input's order
# Thresholds of the contact labels when none are given: conventions from common practice (enter at 3 cm and 0.3 m/s, leave at
# 5 cm and 0.6 m/s), not measured on any robot here.
CONTACT_DEFAULTS = {"height_on": 0.03, "height_off": 0.05, "speed_on": 0.3, "speed_off": 0.6}


class MotionContacts(dict):
    """Result of ``motion_contacts``: the device tensors by name (``CONTACT_FIELDS``): ``contact`` uint8 ``[M, C]``, ``frames`` and
    ``touchdowns`` int32 ``[S, C]``, ``slide_sum`` (m), ``slide_step_max`` (m) and ``depth_max`` (m) float64 ``[S, C]``,
    ``airborne_frames`` int32 ``[S]``, ``base`` float64 ``[S]`` (the ground height the clip was measured against)."""


def _contact_input(eng: "Engine", track_or_arrays, out_offsets, body_ids, height_offset, ground, height_on, height_off,
                   speed_on, speed_off, out):
    """Check the arguments of one contacts call and fill its ``ContactInput`` (all but the stream).  Returns (input,
    MotionContacts, keep-alive)."""
    dev = eng.device
    if isinstance(track_or_arrays, dict):
        pos, vel = track_or_arrays.get("body_pos_w"), track_or_arrays.get("body_lin_vel_w")
        if out_offsets is None:
            out_offsets = getattr(track_or_arrays, "out_offsets", None)
    else:
        pos, vel = track_or_arrays
    for t in (pos, vel):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or t.dim() != 3 \
                or tuple(t.shape[1:]) != (eng.nbody, 3) or not t.is_contiguous():
            raise EngineError(f"body_pos_w and body_lin_vel_w must be contiguous float32 [M, {eng.nbody}, 3] tensors on the engine's device")
    M = int(pos.shape[0])
    if int(vel.shape[0]) != M:
        raise EngineError("body_pos_w and body_lin_vel_w must hold the same rows")
    if out_offsets is None:
        raise EngineError("out_offsets is needed with plain arrays")
    offs = _clip_offsets(out_offsets, dev, "out_offsets")
    S = int(offs.shape[0]) - 1
    if isinstance(body_ids, torch.Tensor):
        ids = body_ids
        if ids.device != dev or ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
            raise EngineError("body_ids must be a contiguous 1-D int32 tensor of body indices on the engine's device (or a host sequence)")
    else:
        b = np.ascontiguousarray(body_ids, dtype=np.int32)
        if b.ndim != 1 or (b.size and (b.min() < 0 or b.max() >= eng.nbody)):
            raise ValueError(f"body_ids must be body indices in [0, {eng.nbody})")
        ids = torch.from_numpy(b).to(dev)
    Cn = int(ids.shape[0])
    keep = [pos, vel, offs, ids]
    ci = _native.ContactInput()
    if height_offset is not None:
        ho = height_offset if isinstance(height_offset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(height_offset, dtype=np.float64))
        ho = ho.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(ho.shape) != (Cn,):
            raise EngineError("height_offset must hold one height per contact body")
        ci.height_offset = ho.data_ptr()
        keep.append(ho)
    if isinstance(ground, str):
        if ground != "clip_min":
            raise ValueError("ground must be 'clip_min' or the ground height")
        ci.ground_mode, ci.ground_z = _native.CONTACT_GROUND_CLIP_MIN, 0.0
    else:
        ci.ground_mode, ci.ground_z = _native.CONTACT_GROUND_FIXED, float(ground)
    f64, i32 = torch.float64, torch.int32
    shapes = {"contact": ((M, Cn), torch.uint8), "frames": ((S, Cn), i32), "touchdowns": ((S, Cn), i32), "slide_sum": ((S, Cn), f64),
              "slide_step_max": ((S, Cn), f64), "depth_max": ((S, Cn), f64), "airborne_frames": ((S,), i32), "base": ((S,), f64)}
    # zeros: rows outside every clip are not written, and a call without rows launches nothing (every clip is empty then)
    res = _named_outputs(ci, out, CONTACT_FIELDS, shapes, dev, "CONTACT_FIELDS", lambda k, sh, dt: torch.zeros(sh, dtype=dt, device=dev))
    if out is None and M == 0 and S > 0:
        res["base"].fill_(float("nan") if isinstance(ground, str) else float(ground))
    ci.body_pos_w, ci.body_lin_vel_w, ci.n_rows = pos.data_ptr(), vel.data_ptr(), M
    ci.out_offsets, ci.body_ids, ci.n_seq, ci.n_contact = offs.data_ptr(), ids.data_ptr(), S, Cn
    ci.height_on, ci.height_off, ci.speed_on, ci.speed_off = float(height_on), float(height_off), float(speed_on), float(speed_off)
    return ci, MotionContacts(res), keep


FOOTLOCK_FIELDS = _native.FOOTLOCK_OUTPUTS   # the arrays of the foot locking, in gmr_footlock_input's order
# Parameters of the foot locking when none are given: conventions (a five-frame ramp, runs of two frames, eight damped iterations
# with lambda^2 = 1e-6 m^2 and steps of at most 0.2 rad), not measured on any robot here.
FOOTLOCK_DEFAULTS = {"blend_frames": 5, "min_run": 2, "iterations": 8, "damping": 1e-6, "step_cap": 0.2}


class MotionFootlock(dict):
    """Result of ``motion_footlock``: the device tensors by name (``FOOTLOCK_FIELDS``): ``qpos`` float64 ``[N, nq]`` (the cleaned
    rows), ``pos`` and ``shift`` float64 ``[N, C, 3]`` (the contact bodies' origins before, and how far each is moved), ``runs``,
    ``locked_frames`` and ``limit_frames`` int32 ``[S, C]``, ``shift_max`` and ``residual_max`` (m) float64 ``[S, C]``."""


def _footlock_input(eng: "Engine", qpos, seq_offsets, contact, body_ids, blend_frames, min_run, iterations, damping, step_cap, out):
    """Check the arguments of one foot-locking call and fill its ``FootlockInput`` (all but the stream).  Returns (input,
    MotionFootlock, keep-alive)."""
    dev = eng.device
    N = _qpos_rows(qpos, eng.nq, dev)
    offs = _clip_offsets(seq_offsets, dev)
    S = int(offs.shape[0]) - 1
    ids = np.ascontiguousarray(body_ids, dtype=np.int32)   # a host array: the library reads it before it returns
    if ids.ndim != 1 or not 1 <= ids.size <= _native.FOOTLOCK_MAX_BODIES:
        raise ValueError(f"body_ids must name 1 .. {_native.FOOTLOCK_MAX_BODIES} contact bodies")
    if ids.min() < 0 or ids.max() >= eng.nbody or len(set(ids.tolist())) != ids.size:
        raise ValueError(f"body_ids must be distinct body indices in [0, {eng.nbody})")
    Cn = int(ids.size)
    if not isinstance(contact, torch.Tensor) or contact.device != dev or contact.dtype != torch.uint8 or tuple(contact.shape) != (N, Cn) \
            or not contact.is_contiguous():
        raise EngineError(f"contact must be a contiguous uint8 [{N}, {Cn}] tensor on the engine's device")
    if int(blend_frames) < 0 or int(min_run) < 1 or not 1 <= int(iterations) <= _native.FOOTLOCK_MAX_ITERATIONS:
        raise ValueError(f"blend_frames >= 0, min_run >= 1 and 1 <= iterations <= {_native.FOOTLOCK_MAX_ITERATIONS} are required")
    if not (np.isfinite(damping) and damping > 0.0 and np.isfinite(step_cap) and step_cap > 0.0):
        raise ValueError("damping and step_cap must be finite and > 0")
    f64, i32 = torch.float64, torch.int32
    shapes = {"qpos": ((N, eng.nq), f64), "pos": ((N, Cn, 3), f64), "shift": ((N, Cn, 3), f64), "runs": ((S, Cn), i32),
              "locked_frames": ((S, Cn), i32), "shift_max": ((S, Cn), f64), "residual_max": ((S, Cn), f64), "limit_frames": ((S, Cn), i32)}
    fi = _native.FootlockInput()
    # rows outside every clip are not written, and a call without rows launches nothing: zeros, and qpos starts as a copy
    res = _named_outputs(fi, out, FOOTLOCK_FIELDS, shapes, dev, "FOOTLOCK_FIELDS",
                         lambda k, sh, dt: qpos.clone() if k == "qpos" else torch.zeros(sh, dtype=dt, device=dev))
    if not {"qpos", "pos", "shift"} <= set(res):
        raise EngineError("out must hold qpos, pos and shift: the three are required")
    if res["qpos"].data_ptr() == qpos.data_ptr() and N > 0:
        raise EngineError("out['qpos'] must not alias qpos")
    fi.qpos, fi.n_frames, fi.seq_offsets, fi.contact = qpos.data_ptr(), N, offs.data_ptr(), contact.data_ptr()
    fi.body_ids, fi.n_seq, fi.n_contact = ids.ctypes.data, S, Cn
    fi.blend_frames, fi.min_run, fi.iterations = int(blend_frames), int(min_run), int(iterations)
    fi.damping, fi.step_cap = float(damping), float(step_cap)
    return fi, MotionFootlock(res), [qpos, offs, contact, ids]


DYNAMICS_FIELDS = _native.DYNAMICS_OUTPUTS   # the arrays of the inverse dynamics, in gmr_dynamics_input's order
DYNAMICS_STATS = _native.DYNAMICS_STATS     # of them the per-clip statistics
# Parameters of the inverse dynamics when none are given.  fz_min -- a frame whose ground reaction is below 5 % of the robot's weight
# counts as unloaded and gets no ZMP -- is a convention, not measured on any robot.
DYNAMICS_DEFAULTS = {"gravity": (0.0, 0.0, -9.81), "ground_z": 0.0, "fz_min": 0.05}


class MotionDynamics(dict):
    """Result of ``motion_dynamics``: the device tensors by name (``DYNAMICS_FIELDS``).  Per frame, float64: ``tau`` ``[N, nq - 7]``
    (N m, hinges in qpos order), ``root_wrench`` ``[N, 6]`` (the force and the moment about the root's position the contacts must
    supply, world frame), ``com`` ``[N, 3]``, ``zmp`` ``[N, 2]`` (NaN in an unloaded frame), ``qvel`` / ``qacc`` ``[N, nv]`` (what was
    used; the root's angular part in the world frame).  Per clip (``DYNAMICS_STATS``): ``tau_abs_max``, ``tau_rms``,
    ``tau_ratio_max`` float64 and ``frames_over_limit`` int32 ``[S, nq - 7]``; ``frames_any_over_limit``, ``unloaded_frames``,
    ``nonfinite_frames`` int32 and ``fz_ratio_max``, ``fz_ratio_min`` float64 ``[S]``."""

    @property
    def stats(self):
        return {k: self[k] for k in DYNAMICS_STATS if k in self}


def _dynamics_input(eng: "Engine", qpos, seq_offsets, fps, qvel, qacc, gravity, ground_z, fz_min, table, out):
    """Check the arguments of one inverse-dynamics call and fill its ``DynamicsInput`` (all but the stream).  Returns (input,
    MotionDynamics, keep-alive)."""
    dev = eng.device
    N, nv, nh = _qpos_rows(qpos, eng.nq, dev), eng.nq - 1, eng.nq - 7
    for name, t in (("qvel", qvel), ("qacc", qacc)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float64 or tuple(t.shape) != (N, nv)
                              or not t.is_contiguous()):
            raise EngineError(f"{name} must be a contiguous float64 [{N}, {nv}] tensor on the engine's device (or None)")
    offs = _clip_offsets(seq_offsets, dev)
    S = int(offs.shape[0]) - 1
    g = np.asarray(gravity, dtype=np.float64)
    if g.shape != (3,) or not np.all(np.isfinite(g)) or not np.any(g != 0.0):
        raise ValueError("gravity must hold three finite numbers, not all zero")
    if not (np.isfinite(fps) and fps > 0.0 and np.isfinite(ground_z) and np.isfinite(fz_min) and fz_min >= 0.0):
        raise ValueError("fps > 0, a finite ground_z and fz_min >= 0 are required")
    dev_table = eng.inertial_device(table)
    f64, i32 = torch.float64, torch.int32
    shapes = {"tau": ((N, nh), f64), "root_wrench": ((N, 6), f64), "com": ((N, 3), f64), "zmp": ((N, 2), f64), "qvel": ((N, nv), f64),
              "qacc": ((N, nv), f64), "tau_abs_max": ((S, nh), f64), "tau_rms": ((S, nh), f64), "tau_ratio_max": ((S, nh), f64),
              "frames_over_limit": ((S, nh), i32), "frames_any_over_limit": ((S,), i32), "fz_ratio_max": ((S,), f64),
              "fz_ratio_min": ((S,), f64), "unloaded_frames": ((S,), i32), "nonfinite_frames": ((S,), i32)}
    di = _native.DynamicsInput()
    # rows outside every clip are not written, and a call without rows launches nothing: zeros
    res = _named_outputs(di, out, DYNAMICS_FIELDS, shapes, dev, "DYNAMICS_FIELDS", lambda k, sh, dt: torch.zeros(sh, dtype=dt, device=dev))
    if set(res) & set(DYNAMICS_STATS) and not {"tau", "root_wrench"} <= set(res):
        raise EngineError("out must hold tau and root_wrench when it holds a statistic: the statistics are reduced from them")
    di.qpos, di.n_frames, di.seq_offsets, di.n_seq = qpos.data_ptr(), N, offs.data_ptr(), S
    di.qvel = qvel.data_ptr() if qvel is not None else None
    di.qacc = qacc.data_ptr() if qacc is not None else None
    di.nbody, di.fps = int(dev_table["body_mass"].shape[0]), float(fps)
    di.gravity_x, di.gravity_y, di.gravity_z = float(g[0]), float(g[1]), float(g[2])
    di.ground_z, di.fz_min = float(ground_z), float(fz_min)
    for k in _native.DYNAMICS_TABLE:
        setattr(di, k, dev_table[k].data_ptr())
    return di, MotionDynamics(res), [qpos, offs, qvel, qacc, dev_table]


SELF_COLLISION_FIELDS = _native.SELF_COLLISION_OUTPUTS   # the arrays of the self-collision report, in gmr_self_collision_input's order
SELF_COLLISION_STATS = _native.SELF_COLLISION_STATS      # of them the per-clip statistics


class MotionSelfCollision(dict):
    """Result of ``motion_self_collision``: the device tensors by name (``SELF_COLLISION_FIELDS``).  Per frame ``[N]``:
    ``clearance`` float64 (metres, negative = penetration; NaN for a non-finite frame), ``pair`` int32 (row of the pair table, -1
    in a NaN frame), ``hits`` int32.  Per clip ``[S]`` (``SELF_COLLISION_STATS``): ``clearance_min`` float64, ``worst_frame``,
    ``worst_pair``, ``colliding_frames``, ``longest_run``, ``nonfinite_frames`` int32 and ``hits_sum`` int64."""

    @property
    def stats(self):
        return {k: self[k] for k in SELF_COLLISION_STATS if k in self}


def _self_collision_input(eng: "Engine", qpos, seq_offsets, capsules, pairs, margin, out, stats):
    """Check the arguments of one self-collision call and fill its ``SelfCollisionInput`` (all but the stream).  Returns (input,
    MotionSelfCollision, keep-alive)."""
    dev = eng.device
    N = _qpos_rows(qpos, eng.nq, dev)
    offs = _clip_offsets(seq_offsets, dev)
    S = int(offs.shape[0]) - 1
    if not np.isfinite(margin):
        raise ValueError("margin must be finite")
    dev_table = eng.collision_device(capsules, pairs)
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    shapes = {"clearance": ((N,), f64), "pair": ((N,), i32), "hits": ((N,), i32), "clearance_min": ((S,), f64), "worst_frame": ((S,), i32),
              "worst_pair": ((S,), i32), "colliding_frames": ((S,), i32), "longest_run": ((S,), i32), "hits_sum": ((S,), i64),
              "nonfinite_frames": ((S,), i32)}
    # rows outside every clip are not written, and a call without rows launches nothing: what an empty clip reports
    fill = {"clearance": float("nan"), "pair": -1, "clearance_min": float("inf"), "worst_frame": -1, "worst_pair": -1}
    ci = _native.SelfCollisionInput()
    res = _named_outputs(ci, out, SELF_COLLISION_FIELDS, shapes, dev, "SELF_COLLISION_FIELDS",
                         lambda k, sh, dt: torch.full(sh, fill.get(k, 0), dtype=dt, device=dev)
                         if stats or k in _native.SELF_COLLISION_FRAME_OUTPUTS else None)
    if set(res) & set(SELF_COLLISION_STATS) and not set(_native.SELF_COLLISION_FRAME_OUTPUTS) <= set(res):
        raise EngineError("out must hold clearance, pair and hits when it holds a statistic: the statistics are reduced from them")
    ci.qpos, ci.n_frames, ci.seq_offsets, ci.n_seq = qpos.data_ptr(), N, offs.data_ptr(), S
    ci.n_caps, ci.n_pairs, ci.margin = int(dev_table["cap_body"].shape[0]), int(dev_table["pairs"].shape[0]), float(margin)
    for k in _native.SELF_COLLISION_TABLE:
        setattr(ci, k, dev_table[k].data_ptr())
    return ci, MotionSelfCollision(res), [qpos, offs, dev_table]


SELF_COLLISION_REPAIR_FIELDS = _native.SELF_COLLISION_REPAIR_OUTPUTS   # the arrays of the repair, in gmr_self_collision_repair_input's order
SELF_COLLISION_REPAIR_STATS = _native.SELF_COLLISION_REPAIR_STATS      # of them the per-clip statistics
# 16 passes, lambda^2 = 1e-6 m^2, steps of at most 0.2 rad, 0.1 mm left over counts as resolved: conventions, not measured on a robot
SELF_COLLISION_REPAIR_DEFAULTS = {"iterations": 16, "damping": 1e-6, "step_cap": 0.2, "resolve_tol": 1e-4}


class MotionSelfCollisionRepair(dict):
    """Result of ``motion_self_collision_repair``: the device tensors by name (``SELF_COLLISION_REPAIR_FIELDS``).  ``qpos`` ``[N, nq]``
    float64, the repaired rows.  Per frame ``[N]`` float64: ``clearance_before``, ``clearance_after`` (NaN in a frame that is not
    evaluated), ``move`` (the largest change of a hinge, rad).  Per clip ``[S]`` (``SELF_COLLISION_REPAIR_STATS``):
    ``repaired_frames``, ``unresolved_frames``, ``nonfinite_frames`` int32, ``move_max``, ``clearance_min_after`` float64."""

    def statistics(self) -> dict:
        return {k: self[k] for k in SELF_COLLISION_REPAIR_STATS if k in self}


def _self_collision_repair_input(eng: "Engine", qpos, seq_offsets, capsules, pairs, margin, iterations, damping, step_cap, resolve_tol,
                                 movable, out, stats):
    """Check the arguments of one repair call and fill its ``SelfCollisionRepairInput`` (all but the stream).  Returns (input,
    MotionSelfCollisionRepair, keep-alive)."""
    dev = eng.device
    if eng.cm.robot.planar_base:
        raise NotImplementedError("the self-collision repair assumes a free-joint root; a planar-base robot is not supported")
    N = _qpos_rows(qpos, eng.nq, dev)
    offs = _clip_offsets(seq_offsets, dev)
    S = int(offs.shape[0]) - 1
    if not np.isfinite(margin):
        raise ValueError("margin must be finite")
    if not 1 <= int(iterations) <= _native.SELF_COLLISION_REPAIR_MAX_ITERATIONS:
        raise ValueError(f"iterations must be 1 .. {_native.SELF_COLLISION_REPAIR_MAX_ITERATIONS}")
    if not (np.isfinite(damping) and damping > 0.0 and np.isfinite(step_cap) and step_cap > 0.0):
        raise ValueError("damping and step_cap must be finite and > 0")
    if not (np.isfinite(resolve_tol) and resolve_tol >= 0.0):
        raise ValueError("resolve_tol must be finite and >= 0")
    nh = eng.nq - 7
    mask = (1 << 64) - 1 if movable is None else int(movable)
    if mask < 0 or mask >> 64:
        raise ValueError("movable is a 64-bit mask, bit i for hinge i in qpos order (gmr_amd.collision.movable_mask)")
    dev_table = eng.collision_device(capsules, pairs)
    f64, i32 = torch.float64, torch.int32
    shapes = {"qpos": ((N, eng.nq), f64), "clearance_before": ((N,), f64), "clearance_after": ((N,), f64), "move": ((N,), f64),
              "repaired_frames": ((S,), i32), "unresolved_frames": ((S,), i32), "move_max": ((S,), f64),
              "clearance_min_after": ((S,), f64), "nonfinite_frames": ((S,), i32)}
    # rows outside every clip are not written, and a call without rows launches nothing: what an empty clip reports
    fill = {"clearance_before": float("nan"), "clearance_after": float("nan"), "clearance_min_after": float("inf")}

    def alloc(k, sh, dt):
        if k == "qpos":
            return qpos.clone()
        return torch.full(sh, fill.get(k, 0), dtype=dt, device=dev) if stats or k in _native.SELF_COLLISION_REPAIR_FRAME_OUTPUTS else None

    ri = _native.SelfCollisionRepairInput()
    res = _named_outputs(ri, out, SELF_COLLISION_REPAIR_FIELDS, shapes, dev, "SELF_COLLISION_REPAIR_FIELDS", alloc)
    if "qpos" not in res:
        raise EngineError("out must hold qpos: the repaired rows are the call's result")
    if res["qpos"].numel() and res["qpos"].data_ptr() == qpos.data_ptr():
        raise EngineError("out['qpos'] must not be qpos: the call does not work in place")
    if set(res) & set(SELF_COLLISION_REPAIR_STATS) and not set(_native.SELF_COLLISION_REPAIR_FRAME_OUTPUTS) <= set(res):
        raise EngineError("out must hold clearance_before, clearance_after and move when it holds a statistic: the statistics are reduced from them")
    ri.qpos, ri.n_frames, ri.seq_offsets, ri.n_seq = qpos.data_ptr(), N, offs.data_ptr(), S
    ri.n_caps, ri.n_pairs, ri.margin = int(dev_table["cap_body"].shape[0]), int(dev_table["pairs"].shape[0]), float(margin)
    ri.iterations, ri.damping, ri.step_cap, ri.resolve_tol = int(iterations), float(damping), float(step_cap), float(resolve_tol)
    ri.hinge_mask = mask & ((1 << nh) - 1 if nh < 64 else (1 << 64) - 1)
    for k in _native.SELF_COLLISION_TABLE:
        setattr(ri, k, dev_table[k].data_ptr())
    return ri, MotionSelfCollisionRepair(res), [qpos, offs, dev_table]


class MotionTransitions(dict):
    """Result of ``motion_transitions``: the device tensors by name -- ``points`` ``[N, P, 3]`` and ``moments`` ``[N, 6]`` float64,
    ``best_cost`` ``[E, D]`` float64 (``inf`` where a source has no target frame), ``best_frame`` ``[E, D]`` int32 (``-1`` there) and,
    when asked for, ``cost_out`` ``[E, n_targets]`` -- and as attributes the host tables of the call (``src_clips``, ``src_offsets``,
    ``dst_clips``, ``dst_offsets``: ``gmr_amd.transitions.search_tables``), ``window``, ``stride``, ``min_gap`` and the normalised
    ``weights``.  Source ``src_offsets[a] + u`` is frame ``u * stride`` of clip ``src_clips[a]``."""


RETIME_FIELDS = _native.RETIME_PLAN_OUTPUTS   # the arrays of a retiming plan, in gmr_retime_plan_input's order
RETIME_STATS = _native.RETIME_STATS           # the columns of its clip_stats


class MotionRetimePlan(dict):
    """Result of ``motion_retime_plan``: the device tensors by name -- ``need`` ``[N]`` float64, ``ticks`` and ``cum`` ``[N]`` int64
    (1024 ticks per source frame; an interval's values at its first row), ``out_len`` ``[S]`` int64, ``clip_stats`` ``[S, 4]`` int64
    (``RETIME_STATS``) and ``need_max`` ``[S]`` float64 -- and as attributes ``seq_offsets`` (the device tensor the call read),
    ``fps``, ``window`` and ``max_stretch``.  What ``motion_retime_apply`` takes."""


CLIP_REPORT_SEGMENT = _native.CLIP_REPORT_SEGMENT      # frames per wavefront of the clip report (GMR_CLIP_REPORT_SEGMENT)
CLIP_REPORT_LIMIT_EPS = _native.CLIP_REPORT_LIMIT_EPS  # rad: a hinge this close to a limit counts as "near" it

_REPORT_FIELDS = ("err_max", "err_sum", "task_pos_max", "task_pos_sum", "task_rot_max", "task_rot_sum", "near_lo", "near_hi",
                  "dof_step_max", "root_step_max", "root_turn_max", "solves_max", "solves_sum", "nonfinite_frames")
_REPORT_SUMS = ("err_sum", "task_pos_sum", "task_rot_sum", "solves_sum")


class ClipReport:
    """Per-clip quality statistics of a retargeted batch (``gmr_clip_report``, include/gmr_amd.h): one row per clip.

    ``err_max`` / ``err_sum`` [S, 2] (stage errors, ``error1()`` / ``error2()``), ``task_pos_max`` / ``task_pos_sum`` [S, nt] (m),
    ``task_rot_max`` / ``task_rot_sum`` [S, nt] (rad), ``near_lo`` / ``near_hi`` [S, nh] int32, ``dof_step_max`` [S, nh] (rad),
    ``root_step_max`` (m) / ``root_turn_max`` (rad) [S], ``solves_max`` int32 / ``solves_sum`` int64 [S] (``None`` without
    ``iters``), ``nonfinite_frames`` [S] int32.  A field that was not computed (no key-points, no ``iters``) is ``None``.
    ``frames`` [S] holds the clip lengths; ``err_mean``, ``task_pos_mean``, ``task_rot_mean`` and ``solves_mean`` are sum / length,
    NaN for a clip without frames.  ``task_names`` (``"<table>:<robot body>"``) and ``hinge_names`` label the columns."""

    def __init__(self, frames, task_names, hinge_names, tables_used, **fields):
        self.frames = np.asarray(frames, dtype=np.int64)
        self.task_names, self.hinge_names, self.tables_used = list(task_names), list(hinge_names), tuple(tables_used)
        for k in _REPORT_FIELDS:
            setattr(self, k, fields.get(k))

    def __len__(self):
        return int(self.frames.shape[0])

    def _mean(self, total):
        if total is None:
            return None
        n = torch.as_tensor(self.frames, dtype=torch.float64, device=total.device) if isinstance(total, torch.Tensor) \
            else self.frames.astype(np.float64)
        n = n.reshape((-1,) + (1,) * (total.dim() - 1 if isinstance(total, torch.Tensor) else total.ndim - 1))
        if isinstance(total, torch.Tensor):
            return torch.where(n > 0, total.to(torch.float64) / n.clamp(min=1), torch.full_like(n, float("nan")))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, total.astype(np.float64) / np.maximum(n, 1), np.nan)

    err_mean = property(lambda self: self._mean(self.err_sum))
    task_pos_mean = property(lambda self: self._mean(self.task_pos_sum))
    task_rot_mean = property(lambda self: self._mean(self.task_rot_sum))
    solves_mean = property(lambda self: self._mean(self.solves_sum))

    @property
    def last_table(self) -> int:
        """Index (0 / 1) of the last table the config uses: its ``err_max`` is a clip's difficulty."""
        return 1 if self.tables_used[1] else 0

    def numpy(self) -> "ClipReport":
        """The same report with host arrays (one synchronisation)."""
        f = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in ((k, getattr(self, k)) for k in _REPORT_FIELDS)}
        return ClipReport(self.frames, self.task_names, self.hinge_names, self.tables_used, **f)


def _report_names(cm: CompiledModel):
    """(task names in the row order of ``task_err_out``, hinge names in qpos order, tables in use) of a compiled model."""
    robot = cm.robot
    tasks = [f"{k + 1}:{t.frame}" for k, tab in enumerate(cm.tasks or [[], []]) for t in tab]
    order = sorted((int(robot.qpos_adr[b]), b) for b in range(robot.nbody) if int(robot.jnt_type[b]) == 1)
    jn = getattr(robot, "jnt_names", None)
    hinges = [str(jn[b]) if jn is not None and jn[b] else str(robot.body_names[b]) for _, b in order]
    cfg = cm.config
    used = (bool(cfg and cfg.use_ik_match_table1 and cm.tasks[0]), bool(cfg and cfg.use_ik_match_table2 and cm.tasks[1]))
    return tasks, hinges, used


def _report_input(eng: "Engine", qpos, pos, quat, slot_col, seq_offsets, height_scale, iters, what: str = ""):
    """Check one model's clip-report arguments, allocate its outputs and fill its ``ClipReportInput``.  Returns (input, report, keep-alive)."""
    N = _qpos_rows(qpos, eng.nq, eng.device, what, contiguous=False)
    qpos = qpos.contiguous()
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if offs.ndim != 1 or len(offs) < 2 or offs[0] != 0 or offs[-1] != N:
        raise ValueError(what + "seq_offsets must span [0, N]")
    if (np.diff(offs) < 0).any():
        raise ValueError(what + "seq_offsets must not decrease")
    S = len(offs) - 1
    ri = _native.ClipReportInput()
    ri.qpos, ri.n_frames, ri.seq_offsets, ri.n_seq = qpos.data_ptr(), N, offs.ctypes.data, S
    keep = [qpos, offs]
    have_kp = pos is not None or quat is not None
    if have_kp:
        if pos is None or quat is None or slot_col is None:
            raise EngineError(what + "the error fields need pos, quat and slot_col")
        if pos.device != eng.device or quat.device != eng.device or pos.dtype != quat.dtype or pos.dtype not in (torch.float32, torch.float64) \
                or pos.dim() != 3 or quat.dim() != 3 or pos.shape[0] != N or pos.shape[:2] != quat.shape[:2] or pos.shape[2] != 3 or quat.shape[2] != 4:
            raise EngineError(what + "bad key-point tensors")
        pos, quat = pos.contiguous(), quat.contiguous()
        slot_col = np.ascontiguousarray(slot_col, dtype=np.int32)
        if slot_col.shape != (eng.info.nslot,):
            raise EngineError(what + "slot_col has the wrong length")
        ri.human_pos, ri.human_quat, ri.slot_col = pos.data_ptr(), quat.data_ptr(), slot_col.ctypes.data
        ri.in_dtype = _native.GMR_DTYPE_F64 if pos.dtype == torch.float64 else _native.GMR_DTYPE_F32
        ri.n_cols = int(pos.shape[1])
        keep += [pos, quat, slot_col]
    if height_scale is not None:
        height_scale = torch.as_tensor(np.asarray(height_scale, dtype=np.float64) if not isinstance(height_scale, torch.Tensor) else height_scale,
                                       dtype=torch.float64).to(eng.device).contiguous()
        if tuple(height_scale.shape) != (S,):
            raise EngineError(what + "height_scale must hold one factor per clip")
        ri.height_scale = height_scale.data_ptr()
        keep.append(height_scale)
    if iters is not None:
        if not isinstance(iters, torch.Tensor) or iters.device != eng.device or iters.dtype != torch.int32 or tuple(iters.shape) != (N,):
            raise EngineError(what + "iters must be an int32 [N] tensor on the engine's device")
        iters = iters.contiguous()
        ri.iters = iters.data_ptr()
        keep.append(iters)
    nt, nh, dev = eng.info.ntask[0] + eng.info.ntask[1], eng.nq - 7, eng.device
    f64, i32 = torch.float64, torch.int32
    shapes = {"err_max": ((S, 2), f64), "err_sum": ((S, 2), f64), "task_pos_max": ((S, nt), f64), "task_pos_sum": ((S, nt), f64),
              "task_rot_max": ((S, nt), f64), "task_rot_sum": ((S, nt), f64), "near_lo": ((S, nh), i32), "near_hi": ((S, nh), i32),
              "dof_step_max": ((S, nh), f64), "root_step_max": ((S,), f64), "root_turn_max": ((S,), f64),
              "solves_max": ((S,), i32), "solves_sum": ((S,), torch.int64), "nonfinite_frames": ((S,), i32)}
    skip = set() if have_kp else {"err_max", "err_sum", "task_pos_max", "task_pos_sum", "task_rot_max", "task_rot_sum"}
    if iters is None:
        skip |= {"solves_max", "solves_sum"}
    fields = {}
    for k, (sh, dt) in shapes.items():
        if k in skip:
            continue
        fields[k] = torch.zeros(sh, dtype=dt, device=dev)
        setattr(ri, k + "_out", fields[k].data_ptr())
    tasks, hinges, used = _report_names(eng.cm)
    return ri, ClipReport(np.diff(offs), tasks, hinges, used, **fields), keep


class Engine:
    def __init__(self, cm: CompiledModel, device: int = 0, _borrowed_handle=None):
        if not torch.cuda.is_available():
            raise EngineError("no HIP device visible to torch: the gmr_amd engine has no CPU path")
        self._lib = _native.load()
        self.cm = cm
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self._owns = _borrowed_handle is None
        if _borrowed_handle is not None:  # a member of an EngineGroup: the group owns the handle
            self._h = _borrowed_handle
        else:
            err = C.create_string_buffer(512)
            self._h = self._lib.gmr_model_create(cm.blob, len(cm.blob), self.device_index, err, len(err))
            if not self._h:
                raise EngineError(f"gmr_model_create: {err.value.decode()}")
        info = ModelInfo()
        self._lib.gmr_model_info_get(self._h, C.byref(info))
        self.info = info
        self.nq, self.nv, self.nbody = info.nq, info.nv, info.nbody
        self._inertial_dev = {}   # inertial tables on the device (inertial_device): None -> the robot's own, id(table) -> an explicit one
        self._collision_dev = {}      # collision proxies on the device (collision_device): (id(capsules), id(pairs)) -> the upload
        self._collision_default = {}  # the skeleton's proxies by radius (default_proxies), default pairs of explicit capsules
        self._symmetry_default = None  # plan_symmetry(robot) at the default tolerances (symmetry_plan), made once
        self._symmetry_dev = {}        # symmetry plans on the device (symmetry_device): id(plan) -> the upload
        self._compose_dev = {}         # composition plans on the device (compose_device): id(plan) -> the upload
        if getattr(cm, "step_cap", None) is not None:  # the model's velocity limit (model.step_cap): part of the handle from here on
            self.set_step_cap(cm.step_cap)

    def set_step_cap(self, cap) -> None:
        """``gmr_model_set_step_cap``: ``cap [nv]`` (dof order, each > 0 or ``inf``) bounds ``|dq|`` of every QP solve of every
        later launch of this engine -- batch, ordered, chunked, group member; ``None`` switches it off.  Sessions keep the cap they
        were created under.  Not while launches of this engine are in flight: synchronise first."""
        if cap is None:
            self._check(self._lib.gmr_model_set_step_cap(self._h, None), "gmr_model_set_step_cap")
            return
        a = np.ascontiguousarray(cap, dtype=np.float64)
        if a.shape != (self.nv,):
            raise ValueError(f"step cap must hold nv = {self.nv} entries, got shape {a.shape}")
        self._check(self._lib.gmr_model_set_step_cap(self._h, a.ctypes.data), "gmr_model_set_step_cap")

    @property
    def step_cap(self) -> np.ndarray:
        """``gmr_model_get_step_cap``: the handle's cap ``[nv]``, all ``inf`` when the limit is off."""
        out = np.empty(self.nv, dtype=np.float64)
        self._check(self._lib.gmr_model_get_step_cap(self._h, out.ctypes.data), "gmr_model_get_step_cap")
        return out

    def close(self):
        if getattr(self, "_h", None):
            if self._owns:
                self._lib.gmr_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.gmr_last_error(self._h)
            raise EngineError(f"{what}: {_ERR.get(rc, rc)}: {msg.decode() if msg else ''}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def session(self, slot_col: np.ndarray, n_cols: int, params: Optional[IKParams] = None, dtype=np.float64) -> "Session":
        return Session(self, slot_col, n_cols, params, dtype)

    # ------------------------------------------------------------------
    def ik_solve(self, pos: torch.Tensor, quat: torch.Tensor, slot_col: np.ndarray, items: np.ndarray,
                 params: Optional[IKParams] = None, qpos_init: Optional[torch.Tensor] = None, n_final: int = 0,
                 want_iters: bool = True, out: Optional[torch.Tensor] = None, qpos_final: Optional[torch.Tensor] = None,
                 iters: Optional[torch.Tensor] = None, frames_done: Optional[torch.Tensor] = None, launch_order="auto",
                 _host_out: bool = False):
        """pos [N,B,3], quat [N,B,4] (float32 or float64 CUDA tensors) -> qpos [N,nq] float64.

        Frames not covered by any item's output range are left as NaN.  Returns (qpos, iters or None, qpos_final or None).
        ``frames_done`` (int32 [n_items] on the device) receives the output frames each item solved (repair runs, gmr_blob.h).
        ``launch_order``: an int32 device tensor from :meth:`plan_order`, ``None`` (array order, longer items first) or ``"auto"``
        -- plan an order when that pays: more plain items than wavefront slots, long enough for the probe to be a small fraction of
        the work (``PROBE_*`` below).  The order only moves work in time; results are identical.
        A plain batch of equal-length clips may run as slices instead (``gmr_ik_balance_plan``; same results).  A slice that gives up
        waiting -- a guard that a correct run never reaches -- leaves the rest of its clip unwritten (NaN rows in a fresh ``out``) and
        sets a word that this method checks, without synchronising, at the START of the next call: it raises for an earlier launch that
        has already finished that way.  To check one call, synchronise and read :attr:`sliced_timeouts` (1 = it happened; reading clears).
        """
        pos, quat, slot_col, items, out, iters, qpos_init, qfin = _ik_batch(
            self, pos, quat, slot_col, items, out=out, iters=iters, want_iters=want_iters, qpos_init=qpos_init, qpos_final=qpos_final,
            n_final=n_final, frames_done=frames_done, host_out=_host_out)
        N, B = int(pos.shape[0]), int(pos.shape[1])
        prm = params or IKParams()
        stats = IKStats()
        self.last_stats = stats
        if N == 0 or len(items) == 0:  # nothing to launch (empty tensors have no device pointer)
            return out, iters, qfin
        if self.sliced_timeouts:  # (a word in host memory: no device call)
            raise EngineError("an earlier sliced ik_solve launch of this engine gave up waiting for a slice: the rest of that clip was not written")
        launch_order = _launch_order(self, launch_order, [items],
                                     lambda pf: self.plan_order(pos, quat, slot_col, items, prm, qpos_init, probe_frames=pf), sliced=True)
        args = (self._h, _ptr(pos), _ptr(quat), _native.GMR_DTYPE_F64 if pos.dtype == torch.float64 else _native.GMR_DTYPE_F32, B,
                slot_col.ctypes.data_as(C.c_void_p), N, items.ctypes.data_as(C.c_void_p), len(items), C.byref(prm), _ptr(qpos_init), _ptr(qfin),
                _ptr(out), _ptr(iters), _ptr(frames_done), C.byref(stats))
        if launch_order is None:
            self._check(self._lib.gmr_ik_solve(*args, self._stream()), "gmr_ik_solve")
        else:
            self._check(self._lib.gmr_ik_solve_ordered(*args, _ptr(launch_order), self._stream()), "gmr_ik_solve_ordered")
        return out, iters, qfin

    # Launch order by predicted cost (gmr_ik_plan_order: solves of an item's first frames x its length): when it is worth a probe, and of
    # how many frames.  Measured on 8192 distinct clips per launch, any heading, probe and device sort included
    # (tools/experiments/short_clip_probe.py, unshaped_probe_order.py; profiles/r03_unshaped_breakdown.md):
    #   equal lengths (nothing else tells the clips apart): 100 / 150 / 200 frames 32.4 -> 30.2, 47.9 -> 45.0, 65.3 -> 57.6 ms with a 4-frame probe;
    #     300 / 600 / 1000 / 3000 frames 94.8 -> 81.5, 183.7 -> 150.3, 306.5 -> 240.9, 608 -> 549 ms with 32 frames;
    #   lengths U(T/3, 5T/3) (the length order gmr_ik_solve applies by itself is most of the cost order): 300 / 600 frames: any probe loses
    #     (74.9 -> 78.6+, 147.3 -> 150.0+); 1000 / 1500 / 2000 / 3000 frames: 245.5 -> 243.0, 365.6 -> 351.1, 493.7 -> 470.8, 728.7 -> 691.8 ms with 32
    #     frames, shorter probes lose -- a few per cent of the clips need ~12 solves per frame against a median of 6.6 (twice the cost of their length,
    #     DESIGN 6) and have to start first, but it takes 32 frames to tell them from the start-up every clip goes through.
    PROBE_FRAMES = 32
    PROBE_FRAMES_SHORT = 4           # equal-length items of fewer than PROBE_SHORT_BELOW frames
    PROBE_SHORT_BELOW = 256
    PROBE_MIN_ITEMS_PER_SLOT = 1.0   # at most one item per wavefront slot: everything starts at once, order is irrelevant
    PROBE_MAX_LENGTH_SPREAD = 0.10   # coefficient of variation of the item lengths below which lengths carry no cost information
    PROBE_MIN_LENGTH_EQUAL = 64      # mean item length from which a probe pays: equal lengths ...
    PROBE_MIN_LENGTH = 1000          # ... and lengths that differ

    def _probe_frames(self, items: np.ndarray, sliced: bool = True) -> int:
        """Frames of every item to probe before an ``launch_order="auto"`` launch; 0 = launch in length order without a probe.
        ``sliced``: the launch is this engine's own ``gmr_ik_solve`` (``ik_solve``, ``bench.py``), which slices the batches
        ``gmr_ik_balance_plan`` names and needs no order for them; group launches run whole clips and pass ``False``."""
        if len(items) == 0 or np.any(items["check_stride"] != 0) or np.any(items["n_burn"] > 0):
            return 0  # walks cannot be probed; speculative chunks (burn-in) are short and alike within a clip: 1.84e7 -> 1.69e7 frames/s with a probe
        slots = 8 * torch.cuda.get_device_properties(self.device).multi_processor_count  # two wavefronts per SIMD
        if sliced and self.balance_plan(items, slots) > 0:
            return 0  # gmr_ik_solve cuts this batch into slices drawn by ticket: no order to plan, no probe
        if len(items) <= self.PROBE_MIN_ITEMS_PER_SLOT * slots:
            return 0
        ln = (items["n_burn"] + items["n_out"]).astype(np.float64)
        mean = float(ln.mean())
        if ln.std() <= self.PROBE_MAX_LENGTH_SPREAD * mean:
            if mean < self.PROBE_MIN_LENGTH_EQUAL:
                return 0
            return self.PROBE_FRAMES if mean >= self.PROBE_SHORT_BELOW else self.PROBE_FRAMES_SHORT
        return self.PROBE_FRAMES if mean >= self.PROBE_MIN_LENGTH else 0

    def balance_plan(self, items: np.ndarray, slots: int) -> int:
        """``gmr_ik_balance_plan``: the slice length ``gmr_ik_solve`` would run ``items`` with on ``slots`` wavefront slots, 0 = whole clips."""
        items = np.ascontiguousarray(items, dtype=_native.WORK_ITEM_DTYPE)
        return int(self._lib.gmr_ik_balance_plan(items.ctypes.data_as(C.c_void_p), len(items), int(slots)))

    @property
    def sliced_timeouts(self) -> int:
        """``gmr_ik_sliced_timeouts``: 1 if a sliced launch of this engine gave up waiting since the last look (synchronise first), else 0;
        reading clears it.  ``ik_solve`` looks at every call and raises for an earlier launch that did."""
        return int(self._lib.gmr_ik_sliced_timeouts(self._h))

    def _order_pays(self, items: np.ndarray) -> bool:
        return self._probe_frames(items) > 0

    def plan_order(self, pos: torch.Tensor, quat: torch.Tensor, slot_col: np.ndarray, items: np.ndarray, params: Optional[IKParams] = None,
                   qpos_init: Optional[torch.Tensor] = None, probe_frames: Optional[int] = None) -> torch.Tensor:
        """Items by predicted cost, most expensive first: int32 ``[n_items]`` on the device, for ``ik_solve(launch_order=...)``.
        Solves the first ``probe_frames`` frames of every item for their cost alone; asynchronous on the current stream."""
        items = np.ascontiguousarray(items, dtype=_native.WORK_ITEM_DTYPE)
        slot_col = np.ascontiguousarray(slot_col, dtype=np.int32)
        order = torch.empty(len(items), dtype=torch.int32, device=self.device)
        if len(items) == 0:
            return order
        prm = params or IKParams()
        rc = self._lib.gmr_ik_plan_order(
            self._h, _ptr(pos), _ptr(quat), _native.GMR_DTYPE_F64 if pos.dtype == torch.float64 else _native.GMR_DTYPE_F32, int(pos.shape[1]),
            slot_col.ctypes.data_as(C.c_void_p), int(pos.shape[0]), items.ctypes.data_as(C.c_void_p), len(items), C.byref(prm), _ptr(qpos_init),
            int(probe_frames or self.PROBE_FRAMES), _ptr(order), self._stream())
        self._check(rc, "gmr_ik_plan_order")
        return order

    def ik_solve_host(self, pos: np.ndarray, quat: np.ndarray, slot_col: np.ndarray, seq_offsets, params: Optional[IKParams] = None,
                      height_scales=None, first_batch_clips: Optional[int] = None, max_batch_frames: Optional[int] = None, want_iters: bool = True,
                      check: bool = True, out: Optional[np.ndarray] = None):
        """Whole clips from HOST arrays to a HOST result, pipelined: what the dataset scripts hand over
        (scripts/smplx_to_robot_dataset.py:84-89 builds host key-points per file) without a serial copy-in / solve / copy-out.

        * in: the caller's pageable arrays are read in place by the copy engine (all their columns; ``slot_col`` picks the ones the
          config consumes on the device), batch by batch, into two alternating device buffers on two HIP streams, so that batch
          k+1 crosses PCIe while batch k's kernel runs.  The first batch is small -- ``first_batch_clips``, by default one clip per
          wavefront slot -- because its copy is the only one nothing hides; the rest goes in batches of up to ``max_batch_frames``
          frames (default: what fits 16 GiB of staged key-points per buffer), big enough for the engine's cost-ordered launch.
        * out: there is no copy-out.  The kernel writes every frame's qpos straight into the pinned host result (288 B per frame
          of posted PCIe writes against the ~46 us a wavefront spends on a frame); a fresh pageable result array would cost more in
          page faults than the kernel takes, a device buffer + copy engine leaves the last batch's copy exposed.
        Results are bitwise those of ``ik_solve`` on resident tensors (same kernel, same per-clip work items).  With ``check``
        every batch's solve counts are inspected on the device: bit 31 (a non-finite qpos) -> FloatingPointError, bit 30 (a
        capped QP) -> RuntimeError.  Returns (qpos [N, nq] float64, iters [N] int32 or None) as numpy arrays backed by pinned
        memory.  ``out``: the qpos array of an earlier call of the same size, to be overwritten -- page-locking a fresh multi-GB
        result costs more than the solve (7 GB: 0.7 s), so loops over many batches should hand the previous result back (or
        simply drop it before the next call: the allocator then reuses its pinned block).  Measured rates: DESIGN.md.
        """
        from .schedule import make_items
        if pos.dtype != quat.dtype or pos.dtype not in (np.float32, np.float64):
            raise EngineError("pos/quat must both be float32 or both float64")
        if pos.ndim != 3 or quat.ndim != 3 or pos.shape[2] != 3 or quat.shape[2] != 4 or pos.shape[:2] != quat.shape[:2]:
            raise EngineError(f"bad input shapes {pos.shape} / {quat.shape}")
        offs = np.asarray(seq_offsets, dtype=np.int64)
        N, B = int(pos.shape[0]), int(pos.shape[1])
        if offs[0] != 0 or offs[-1] != N:
            raise EngineError("seq_offsets must span [0, N]")
        slot_col = np.ascontiguousarray(slot_col, dtype=np.int32)
        tdt = torch.float32 if pos.dtype == np.float32 else torch.float64
        hs = None if height_scales is None else np.asarray(height_scales, dtype=np.float64)
        if out is not None:
            if not isinstance(out, np.ndarray) or out.shape != (N, self.nq) or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise EngineError("out must be a C-contiguous float64 [N, nq] array (the result of an earlier call)")
            out = torch.from_numpy(out)
            if not out.is_pinned():
                raise EngineError("out must be pinned host memory: pass the result of an earlier ik_solve_host call")
        else:
            out = torch.empty((N, self.nq), dtype=torch.float64, pin_memory=True)
        iters = torch.empty(N, dtype=torch.int32, pin_memory=True) if want_iters else None
        if N == 0:
            return out.numpy(), (iters.numpy() if want_iters else None)
        n_clips = len(offs) - 1
        # batch bounds (clip indices): a first batch of one clip per wavefront slot, then batches of up to max_batch_frames frames
        slots = 8 * torch.cuda.get_device_properties(self.device).multi_processor_count
        per = max(1, int(max_batch_frames)) if max_batch_frames else max(1, (16 << 30) // (B * 7 * pos.dtype.itemsize))
        bounds = [0, min(n_clips, max(1, int(first_batch_clips) if first_batch_clips else slots))]
        while bounds[-1] < n_clips:
            nxt = int(np.searchsorted(offs, offs[bounds[-1]] + per, side="right")) - 1
            bounds.append(min(n_clips, max(nxt, bounds[-1] + 1)))
        cap = max(int(offs[bounds[k + 1]] - offs[bounds[k]]) for k in range(len(bounds) - 1))
        tpos, tquat = torch.from_numpy(np.ascontiguousarray(pos)), torch.from_numpy(np.ascontiguousarray(quat))
        nbuf = min(2, len(bounds) - 1)
        st = [torch.cuda.Stream(self.device) for _ in range(nbuf)]
        dp = [torch.empty((cap, B, 3), dtype=tdt, device=self.device) for _ in range(nbuf)]
        dq = [torch.empty((cap, B, 4), dtype=tdt, device=self.device) for _ in range(nbuf)]
        want_i = want_iters or check
        di = [torch.empty(cap, dtype=torch.int32, device=self.device) for _ in range(nbuf)] if want_i else None
        flags = torch.zeros((nbuf, 2), dtype=torch.int32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        for s_ in st:
            s_.wait_stream(cur)
        for k in range(len(bounds) - 1):
            b = k % nbuf
            c0, c1 = bounds[k], bounds[k + 1]
            f0, f1 = int(offs[c0]), int(offs[c1])
            n = f1 - f0
            if n == 0:
                continue
            items = make_items(offs[c0:c1 + 1] - f0, height_scales=None if hs is None else hs[c0:c1])
            with torch.cuda.stream(st[b]):
                # pageable -> device: the runtime stages the copy and returns when the host data has been consumed; the other
                # stream's kernel keeps running meanwhile
                dp[b][:n].copy_(tpos[f0:f1], non_blocking=True)
                dq[b][:n].copy_(tquat[f0:f1], non_blocking=True)
                self.ik_solve(dp[b][:n], dq[b][:n], slot_col, items, params=params, out=out[f0:f1], iters=di[b][:n] if want_i else None,
                              want_iters=want_i, _host_out=True)
                if check:
                    flags[b, 0] |= (di[b][:n] >> 31).ne(0).any().to(torch.int32)
                    flags[b, 1] |= ((di[b][:n] >> 30) & 1).ne(0).any().to(torch.int32)
                if want_iters:
                    iters[f0:f1].copy_(di[b][:n], non_blocking=True)
        for s_ in st:
            s_.synchronize()
            cur.wait_stream(s_)
        if check:
            bad = flags.sum(0).cpu().numpy()
            if bad[0]:
                raise FloatingPointError("non-finite qpos")
            if bad[1]:
                raise RuntimeError("a box QP hit its iteration cap (the reference would assert on a failed QP)")
        return out.numpy(), (iters.numpy() if want_iters else None)

    def ik_solve_chunked(self, pos: torch.Tensor, quat: torch.Tensor, slot_col: np.ndarray, seq_offsets, chunk: int, burn_in: int,
                         params: Optional[IKParams] = None, eps: float = 1e-7, height_scales=None,
                         chunk_init: int = _native.INIT_ROOT_TARGET, clip_init: int = _native.INIT_QPOS0):
        """Parallel-in-time solve of long clips with *verified* chunk boundaries, in two launches.

        Launch 1 solves every chunk of ``chunk`` frames concurrently, each (but a clip's first) warmed up over
        ``burn_in`` earlier frames from a speculative state (``chunk_init``: qpos0 with the floating base on the root task's
        target, gmr_blob.h), and records per chunk the state B its first output frame started from and its final state F.
        Launch 2 is one *verification walk* per clip (``schedule.plan_walks``): starting from the exact first chunk it
        compares, boundary by boundary, the true state with the next chunk's B; if they agree to ``eps`` the chunk's stored
        frames are what the sequential run produces and the walk jumps to its F, otherwise it solves that chunk itself from
        the true state.  The result therefore follows the reference's sequential warm-start semantics to ``eps`` however
        good the speculative start was; its quality only decides how much of a clip the walk has to re-solve.
        Returns (qpos [N,nq], iters [N], info dict).
        """
        offs = np.asarray(seq_offsets, dtype=np.int64)
        prm = _chunk_params(params, eps)
        first = _chunk_batch(pos, quat, slot_col, offs, chunk, burn_in, height_scales, chunk_init, clip_init)
        res = self.ik_solve(params=prm, **first)
        walk, info = _walk_batch(first, res, offs, chunk)
        if walk is not None:
            self.ik_solve(params=prm, **walk)
        return res[0], res[1], info()

    def ik_solve_chunked_sharded(self, pos: torch.Tensor, quat: torch.Tensor, slot_col: np.ndarray, seq_offsets, chunk: int, burn_in: int,
                                 params: Optional[IKParams] = None, eps: float = 1e-7, height_scales=None):
        """``ik_solve_chunked`` with the chunks of every clip spread over all ranks of the default process group
        (``distributed.solve_chunked_sharded``: BASELINE config 3, few long clips on several GPUs).  Every rank passes the
        same full inputs and receives the full result."""
        from .distributed import solve_chunked_sharded
        prm = _chunk_params(params, eps)

        def solve(items, qinit, qfinal, out, iters, done):
            self.ik_solve(pos, quat, slot_col, items, params=prm, qpos_init=qinit, qpos_final=qfinal, out=out, iters=iters, frames_done=done)

        return solve_chunked_sharded(solve, int(pos.shape[0]), self.nq, seq_offsets, chunk, burn_in, self.device, height_scales=height_scales)

    def evaluate(self, qpos: torch.Tensor, pos: Optional[torch.Tensor] = None, quat: Optional[torch.Tensor] = None,
                 slot_col: Optional[np.ndarray] = None, offset_to_ground: bool = False, want_errors: bool = True, want_poses: bool = False,
                 height_scale: Optional[torch.Tensor] = None, want_task_errors: bool = False):
        """Stage errors [N,2] and/or MuJoCo-convention body poses (xpos [N,nb,3], xquat [N,nb,4] wxyz) at ``qpos`` [N,nq].
        With ``want_task_errors`` a fourth value is returned: the per-task 6-vectors [N, ntask1+ntask2, 6]."""
        if qpos.device != self.device or qpos.dtype != torch.float64 or qpos.dim() != 2 or qpos.shape[1] != self.nq:
            raise EngineError("qpos must be float64 [N, nq] on the engine's device")
        qpos = qpos.contiguous()
        N = int(qpos.shape[0])
        err = xp = xq = None
        B, dt = 0, 0
        if want_errors:
            if pos is None or quat is None or slot_col is None:
                raise EngineError("errors need the human key-points and slot_col")
            if pos.device != self.device or quat.device != self.device or pos.dtype != quat.dtype or pos.dtype not in (torch.float32, torch.float64) \
                    or pos.shape[0] != N or pos.shape[:2] != quat.shape[:2] or pos.shape[2] != 3 or quat.shape[2] != 4:
                raise EngineError("bad key-point tensors")
            pos, quat = pos.contiguous(), quat.contiguous()
            slot_col = np.ascontiguousarray(slot_col, dtype=np.int32)
            if slot_col.shape != (self.info.nslot,):
                raise EngineError("slot_col has the wrong length")
            B, dt = int(pos.shape[1]), _native.GMR_DTYPE_F64 if pos.dtype == torch.float64 else _native.GMR_DTYPE_F32
            err = torch.empty((N, 2), dtype=torch.float64, device=self.device)
        terr = None
        if want_task_errors:
            if not want_errors:
                raise EngineError("task errors need want_errors")
            terr = torch.zeros((N, self.info.ntask[0] + self.info.ntask[1], 6), dtype=torch.float64, device=self.device)
        if want_poses:
            xp = torch.empty((N, self.nbody, 3), dtype=torch.float64, device=self.device)
            xq = torch.empty((N, self.nbody, 4), dtype=torch.float64, device=self.device)
        if N == 0:
            return (err, xp, xq, terr) if want_task_errors else (err, xp, xq)
        if height_scale is not None and (height_scale.dtype != torch.float64 or height_scale.device != self.device or height_scale.shape != (N,)
                                         or not height_scale.is_contiguous()):
            raise EngineError("height_scale must be a contiguous float64 [N] tensor on the engine's device")
        rc = self._lib.gmr_evaluate(self._h, _ptr(qpos), N, _ptr(pos) if want_errors else None, _ptr(quat) if want_errors else None, dt, B,
                                    slot_col.ctypes.data_as(C.c_void_p) if want_errors else None, int(bool(offset_to_ground)), _ptr(height_scale),
                                    _ptr(err), _ptr(terr), _ptr(xp), _ptr(xq), self._stream())
        self._check(rc, "gmr_evaluate")
        return (err, xp, xq, terr) if want_task_errors else (err, xp, xq)

    def fk(self, root_pos: torch.Tensor, root_rot_xyzw: torch.Tensor, dof: torch.Tensor, want_rot: bool = True,
           out_pos: Optional[torch.Tensor] = None, out_rot: Optional[torch.Tensor] = None, fitted_shape: Optional[torch.Tensor] = None):
        """``KinematicsModel.forward_kinematics``: body_pos [T,nbody,3] (and body_rot [T,nbody,4] xyzw), float32.  ``out_pos`` /
        ``out_rot``: caller-owned result tensors (a fresh multi-GB allocation costs more than the kernel).  ``fitted_shape``: float32
        [nbody] or [nbody, 3] on the device, the per-body scale of the local translations (kinematics_model.py:225)."""
        for t in (root_pos, root_rot_xyzw, dof):
            if t.device != self.device or t.dtype != torch.float32:
                raise EngineError("fk inputs must be float32 tensors on the engine's device")
        T = int(root_pos.shape[0])
        if root_pos.shape != (T, 3) or root_rot_xyzw.shape != (T, 4) or dof.shape != (T, self.nq - 7):
            raise EngineError("bad fk input shapes")
        root_pos, root_rot_xyzw, dof = root_pos.contiguous(), root_rot_xyzw.contiguous(), dof.contiguous()
        def _out(t, k):
            if t is None:
                return torch.empty((T, self.nbody, k), dtype=torch.float32, device=self.device)
            if t.shape != (T, self.nbody, k) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise EngineError("fk output tensors must be contiguous float32 [T, nbody, 3 / 4] on the engine's device")
            return t
        bp = _out(out_pos, 3)
        br = _out(out_rot, 4) if want_rot else None
        if fitted_shape is None:
            rc = self._lib.gmr_fk(self._h, _ptr(root_pos), _ptr(root_rot_xyzw), _ptr(dof), T, _ptr(bp), _ptr(br), self._stream())
        else:
            sh = fitted_shape
            if sh.device != self.device or sh.dtype != torch.float32 or tuple(sh.shape) not in ((self.nbody,), (self.nbody, 1), (self.nbody, 3)):
                raise EngineError("fitted_shape must be a float32 [nbody] or [nbody, 3] tensor on the engine's device")
            sh = sh.contiguous()
            rc = self._lib.gmr_fk_shape(self._h, _ptr(root_pos), _ptr(root_rot_xyzw), _ptr(dof), _ptr(sh), 3 if sh.dim() == 2 and sh.shape[1] == 3 else 1,
                                        T, _ptr(bp), _ptr(br), self._stream())
        self._check(rc, "gmr_fk")
        return bp, br

    def _kin_op(self, name: str, x: torch.Tensor, in_shape, out_shape, out: Optional[torch.Tensor]):
        if x.device != self.device or x.dtype != torch.float32 or tuple(x.shape[1:]) != tuple(in_shape):
            raise EngineError(f"{name}: input must be a float32 [T, {', '.join(map(str, in_shape))}] tensor on the engine's device")
        T = int(x.shape[0])
        x = x.contiguous()
        if out is None:
            out = torch.empty((T,) + tuple(out_shape), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (T,) + tuple(out_shape) or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise EngineError(f"{name}: the output tensor must be contiguous float32 [T, {', '.join(map(str, out_shape))}] on the engine's device")
        rc = getattr(self._lib, name)(self._h, _ptr(x), T, _ptr(out), self._stream())
        self._check(rc, name)
        return out

    def dof_to_rot(self, dof: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``KinematicsModel.dof_to_rot`` (kinematics_model.py:172-182): [T, ndof] -> [T, nbody-1, 4] xyzw."""
        return self._kin_op("gmr_dof_to_rot", dof, (self.nq - 7,), (self.nbody - 1, 4), out)

    def rot_to_dof(self, joint_rot: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``KinematicsModel.rot_to_dof`` (kinematics_model.py:184-197): [T, nbody-1, 4] -> [T, ndof], clamped to the joint limits."""
        return self._kin_op("gmr_rot_to_dof", joint_rot, (self.nbody - 1, 4), (self.nq - 7,), out)

    def local_rot_to_global(self, local_rot: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``KinematicsModel.convert_local_rot_to_global`` (kinematics_model.py:199-211): [T, nbody, 4] -> [T, nbody, 4]."""
        return self._kin_op("gmr_local_rot_to_global", local_rot, (self.nbody, 4), (self.nbody, 4), out)

    def fk_min_height(self, root_pos: torch.Tensor, root_rot_xyzw: torch.Tensor, dof: torch.Tensor, seq_offsets) -> torch.Tensor:
        for t in (root_pos, root_rot_xyzw, dof):
            if t.device != self.device or t.dtype != torch.float32:
                raise EngineError("fk inputs must be float32 tensors on the engine's device")
        offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
        T = int(root_pos.shape[0])
        if offs[-1] != T or root_pos.shape != (T, 3) or root_rot_xyzw.shape != (T, 4) or dof.shape != (T, self.nq - 7):
            raise EngineError("bad fk_min_height shapes")
        out = torch.empty(len(offs) - 1, dtype=torch.float32, device=self.device)
        rc = self._lib.gmr_fk_min_height(self._h, _ptr(root_pos.contiguous()), _ptr(root_rot_xyzw.contiguous()), _ptr(dof.contiguous()),
                                         offs.ctypes.data_as(C.c_void_p), len(offs) - 1, _ptr(out), self._stream())
        self._check(rc, "gmr_fk_min_height")
        return out


    def motion_epilogue(self, qpos: torch.Tensor, seq_offsets, height_adjust: bool = True, root_origin_offset: bool = True,
                        ground_offset: float = 0.0, out=None, min_z: Optional[torch.Tensor] = None):
        """The dataset post-processing of ``dataset.motions_from_qpos`` in one native call (``gmr_motion_epilogue``): qpos
        ``[N, nq]`` float64 (free-joint layout, concatenated clips) -> device tensors (root_pos f64 [N, 3], root_rot f64 [N, 4]
        xyzw, dof_pos f64 [N, nq-7], local_body_pos f32 [N, nbody, 3]), bit for bit what the two FK launches and the torch ops
        give.  ``out``: caller-owned result tensors in that order; ``min_z``: a float32 [n_seq] tensor that also receives the
        per-clip minimum body height (``fk_min_height``; +inf for a clip without frames, also when N = 0).  Asynchronous on the current stream."""
        mi, res, keep = _motion_input(self, qpos, seq_offsets, height_adjust, root_origin_offset, ground_offset, out, min_z)
        self._check(self._lib.gmr_motion_epilogue(self._h, C.byref(mi), self._stream()), "gmr_motion_epilogue")
        return res

    def motion_track(self, qpos: torch.Tensor, seq_offsets, fps_in, fps_out, out=None, bodies: bool = True,
                     lowpass_hz: float = 0.0) -> MotionTrack:
        """The tracking export in one native call (``gmr_motion_track``; the definition is the contract in include/gmr_amd.h):
        qpos ``[N, nq]`` float64 (free-joint layout, concatenated clips at ``fps_in``: one rate or one per clip) resampled to
        ``fps_out`` -> a :class:`MotionTrack` of device tensors with ``M = out_offsets[-1]`` rows: root_pos, root_rot (xyzw),
        joint_pos and their velocities root_lin_vel, root_ang_vel (world frame), joint_vel in float64; with ``bodies`` the world
        poses body_pos_w, body_quat_w (xyzw) -- bit for bit ``fk`` of the float32 casts of the resampled root and joints -- and
        their velocities body_lin_vel_w, body_ang_vel_w in float32.  ``out``: caller-owned result tensors by name (a name left
        out is not computed).  ``lowpass_hz`` > 0: qpos is first filtered per clip with a zero-phase 2nd-order Butterworth
        low-pass at that cutoff, on the device (one more kernel; root quaternion sign-continuous and normalised), and every
        output is what the unfiltered call gives on the filtered qpos; the cutoff must lie below half of every clip's rate.
        Asynchronous on the current stream."""
        ti, res, keep = _track_input(self, qpos, seq_offsets, fps_in, fps_out, out, bodies, lowpass_hz=lowpass_hz)
        self._check(self._lib.gmr_motion_track(self._h, C.byref(ti), self._stream()), "gmr_motion_track")
        return res

    def motion_sample(self, qpos: torch.Tensor, seq_offsets_dev: torch.Tensor, fps_dev: torch.Tensor, ids: torch.Tensor,
                      times: torch.Tensor, k_per_id: int = 1, bodies: Optional[torch.Tensor] = None, fields=None, out=None,
                      dtype=torch.float64) -> MotionSample:
        """Random access into a library of clips kept as qpos, in one kernel and nothing else (``gmr_motion_sample``; the
        definition is the contract in include/gmr_amd.h).  qpos ``[N, nq]`` float64 (concatenated clips), the clip table
        ``seq_offsets_dev`` int64 ``[S + 1]`` and ``fps_dev`` float64 ``[S]`` ON THE DEVICE, ``ids`` int64 and ``times`` (seconds,
        float32 or float64) ``[Q]``, or ``[E]`` and ``[E, K]`` (``k_per_id = K``: K times per id).  Returns a
        :class:`MotionSample` named as ``TRACK_FIELDS``, shaped ``[E, K, ...]`` for 2-D times and ``[Q, ...]`` otherwise: the six
        generalized arrays in ``dtype``, the four body arrays in float32 with one column per entry of ``bodies`` (an int32
        device tensor of body indices, trusted; ``None``: every body in model order).  ``fields``: the names to compute;
        ``out``: caller-owned result tensors by name (a name left out is not computed).  A query with an id outside the table,
        an empty clip or a non-finite time yields NaN in every array.  Asynchronous on the current stream; no allocation
        with ``out``, no copy, no synchronisation."""
        si, res, keep = _sample_input(self, qpos, seq_offsets_dev, fps_dev, ids, times, k_per_id, bodies, fields, out, dtype)
        self._check(self._lib.gmr_motion_sample(self._h, C.byref(si), self._stream()), "gmr_motion_sample")
        return res

    def motion_contacts(self, track_or_arrays, out_offsets=None, body_ids=(), height_offset=None, ground="clip_min",
                        height_on: float = CONTACT_DEFAULTS["height_on"], height_off: float = CONTACT_DEFAULTS["height_off"],
                        speed_on: float = CONTACT_DEFAULTS["speed_on"], speed_off: float = CONTACT_DEFAULTS["speed_off"],
                        out=None) -> MotionContacts:
        """Foot-contact labels and slide statistics of a tracking export in one kernel (``gmr_motion_contacts``; the definition
        is the contract in include/gmr_amd.h).  ``track_or_arrays``: a :class:`MotionTrack` (or any dict with ``body_pos_w`` and
        ``body_lin_vel_w``), or the pair ``(body_pos_w, body_lin_vel_w)`` of float32 ``[M, nbody, 3]`` device tensors.
        ``out_offsets`` ``[S + 1]``: the clips' rows, a host sequence (uploaded once) or a device int64 tensor; ``None`` takes a
        MotionTrack's own.  ``body_ids``: the C <= 64 contact bodies, a host sequence of body indices (range-checked here) or a
        device int32 tensor (trusted).  ``height_offset`` ``[C]``: height of each body origin above its own sole (``None``:
        zeros).  ``ground``: ``"clip_min"`` measures every clip against the lowest contact-body height it reaches, a number is
        the ground height.  A body is in contact from a frame at or below ``height_on`` and ``speed_on`` until one above
        ``height_off`` or ``speed_off``; the defaults (3 cm and 0.3 m/s, 5 cm and 0.6 m/s) are conventions from common practice,
        not measured on any robot.  Returns a :class:`MotionContacts` of device tensors; ``out``: caller-owned result tensors by
        name (a name left out is not computed).  Asynchronous on the current stream."""
        ci, res, keep = _contact_input(self, track_or_arrays, out_offsets, body_ids, height_offset, ground, height_on, height_off,
                                       speed_on, speed_off, out)
        ci.stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.gmr_motion_contacts(self._h, C.byref(ci)), "gmr_motion_contacts")
        return res

    def motion_footlock(self, qpos: torch.Tensor, seq_offsets, contact: torch.Tensor, body_ids,
                        blend_frames: int = FOOTLOCK_DEFAULTS["blend_frames"], min_run: int = FOOTLOCK_DEFAULTS["min_run"],
                        iterations: int = FOOTLOCK_DEFAULTS["iterations"], damping: float = FOOTLOCK_DEFAULTS["damping"],
                        step_cap: float = FOOTLOCK_DEFAULTS["step_cap"], out=None) -> MotionFootlock:
        """Remove the horizontal slide of planted feet from qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in three
        kernels (``gmr_motion_footlock``; the definition is the contract in include/gmr_amd.h).  ``seq_offsets`` ``[S + 1]``: the
        clips' rows, a host sequence (uploaded once) or a device int64 tensor.  ``contact`` uint8 ``[N, C]``: non-zero = planted,
        labels at qpos's own frames.  ``body_ids``: the 1 <= C <= 8 contact bodies, a host sequence of distinct body indices.  Over
        every run of at least ``min_run`` planted frames a body is pinned to the mean of its own xy; the shift fades over
        ``blend_frames`` frames on both sides; ``iterations`` damped least-squares steps (``damping`` = lambda^2 in m^2, steps of at
        most ``step_cap`` rad) over the hinges only that body hangs on move it there.  The defaults are conventions, not measured
        on any robot.  Returns a :class:`MotionFootlock` of device tensors; ``out``: caller-owned result tensors by name (``qpos``,
        ``pos`` and ``shift`` are required, a statistic left out is not computed).  Asynchronous on the current stream."""
        fi, res, keep = _footlock_input(self, qpos, seq_offsets, contact, body_ids, blend_frames, min_run, iterations, damping, step_cap, out)
        fi.stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.gmr_motion_footlock(self._h, C.byref(fi)), "gmr_motion_footlock")
        return res

    def inertial_device(self, table=None):
        """The inertial table on the engine's device, by the field names of ``gmr_dynamics_input``: uploaded once per engine (or
        once per explicit ``table``, a :class:`gmr_amd.inertial.InertialTable`) and cached.  ``table=None`` reads the robot's own
        MJCF file (``gmr_amd.inertial.inertial_table``)."""
        cache = self._inertial_dev
        key = id(table) if table is not None else None
        if key not in cache:
            from .inertial import inertial_table
            t = table if table is not None else inertial_table(self.cm.robot)
            nh = self.nq - 7
            if t.nbody != self.nbody or t.armature.shape != (nh,) or t.torque_limit.shape != (nh,):
                raise EngineError(f"the inertial table holds {t.nbody} bodies and {t.armature.shape[0]} hinges, the model {self.nbody} and {nh}")
            I = t.inertia
            host = {"body_parent": np.ascontiguousarray(t.parent, dtype=np.int32), "body_mass": np.ascontiguousarray(t.mass, dtype=np.float64),
                    "body_com": np.ascontiguousarray(t.com, dtype=np.float64),
                    "body_inertia": np.ascontiguousarray(np.stack([I[:, 0, 0], I[:, 1, 1], I[:, 2, 2], I[:, 0, 1], I[:, 0, 2], I[:, 1, 2]], -1)),
                    "armature": np.ascontiguousarray(t.armature, dtype=np.float64), "torque_limit": np.ascontiguousarray(t.torque_limit, dtype=np.float64)}
            cache[key] = ({k: torch.from_numpy(v).to(self.device) for k, v in host.items()},)
            if table is not None:   # an explicit table's upload lives as long as the table does: its id is the key
                weakref.finalize(table, cache.pop, key, None)
        return cache[key][0]

    def motion_dynamics(self, qpos: torch.Tensor, seq_offsets, fps: float, qvel: Optional[torch.Tensor] = None,
                        qacc: Optional[torch.Tensor] = None, gravity=DYNAMICS_DEFAULTS["gravity"], ground_z: float = DYNAMICS_DEFAULTS["ground_z"],
                        fz_min: float = DYNAMICS_DEFAULTS["fz_min"], out=None, table=None) -> MotionDynamics:
        """Floating-base inverse dynamics of qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in two kernels
        (``gmr_motion_dynamics``; the definition is the contract in include/gmr_amd.h): joint torques, the wrench the contacts must
        supply on the root, centre of mass and ZMP per frame, torque-limit and ground-reaction statistics per clip.
        ``seq_offsets`` ``[S + 1]``: the clips' rows, a host sequence (uploaded once) or a device int64 tensor.  ``fps``: the one
        frame rate of the call.  ``qvel`` / ``qacc`` ``[N, nv]``: generalized velocity and acceleration with the root's angular
        part in the WORLD frame (what ``motion_track`` writes as ``root_ang_vel``, not MuJoCo's local-frame convention); ``None``:
        the tracking export's central differences, and second differences, of qpos.  ``fz_min`` (a fraction of the robot's
        weight below which a frame is unloaded and has no ZMP) is a convention, not measured on any robot.  ``table``: an
        :class:`gmr_amd.inertial.InertialTable` instead of the one read from the robot's MJCF file.  Returns a
        :class:`MotionDynamics` of device tensors; ``out``: caller-owned result tensors by name (a name left out is not computed;
        a statistic needs ``tau`` and ``root_wrench``).  A planar base is refused (``GMR_EUNSUPPORTED``).  Asynchronous on the current
        stream; with ``out`` and a device ``seq_offsets`` no allocation, no copy, no synchronisation."""
        di, res, keep = _dynamics_input(self, qpos, seq_offsets, fps, qvel, qacc, gravity, ground_z, fz_min, table, out)
        di.stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.gmr_motion_dynamics(self._h, C.byref(di)), "gmr_motion_dynamics")
        return res

    def default_proxies(self, radius=None):
        """``(CapsuleTable, PairTable)`` of the robot's skeleton at ``radius`` (``gmr_amd.collision.skeleton_capsules`` and
        ``default_pairs``; ``None``: 0.03 m, a convention, not measured on any robot), built once per engine and radius."""
        from . import collision
        r = collision.DEFAULT_RADIUS if radius is None else radius
        key = tuple(sorted(r.items())) if isinstance(r, dict) else float(r)
        if key not in self._collision_default:
            self._collision_default[key] = collision.proxies(self.cm.robot, radius=r)
        return self._collision_default[key]

    def resolve_proxies(self, capsules=None, pairs=None, radius=None):
        """``(capsules, pairs)`` with the defaults filled in, each default built once: without ``capsules`` the skeleton's at
        ``radius`` (:meth:`default_proxies`), without ``pairs`` the ``default_pairs`` of ``capsules``."""
        if capsules is None:
            capsules, default = self.default_proxies(radius)
            return capsules, (default if pairs is None else pairs)
        if pairs is None:
            key = ("pairs", id(capsules))
            if key not in self._collision_default:
                from . import collision
                self._collision_default[key] = collision.default_pairs(self.cm.robot, capsules)[0]
                weakref.finalize(capsules, self._collision_default.pop, key, None)
            pairs = self._collision_default[key]
        return capsules, pairs

    def collision_device(self, capsules, pairs):
        """The proxy tables on the engine's device, by the field names of ``gmr_self_collision_input``: uploaded once per
        ``(capsules, pairs)`` (a :class:`gmr_amd.collision.CapsuleTable` and a :class:`gmr_amd.collision.PairTable`; their
        identity is the key, so a table changed in place needs a new object) and cached as long as both live."""
        cache = self._collision_dev
        key = (id(capsules), id(pairs))
        if key not in cache:
            from . import collision
            collision.check_tables(self.nbody, capsules, pairs)
            host = {"cap_body": capsules.body, "cap_p0": capsules.p0, "cap_p1": capsules.p1, "cap_radius": capsules.radius, "pairs": pairs.pairs}
            cache[key] = ({k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in host.items()},)
            for t in (capsules, pairs):
                weakref.finalize(t, cache.pop, key, None)
        return cache[key][0]

    def motion_self_collision(self, qpos: torch.Tensor, seq_offsets, capsules=None, pairs=None, margin: float = 0.0, out=None,
                              stats: bool = True) -> MotionSelfCollision:
        """Capsule clearance of qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in two kernels
        (``gmr_motion_self_collision``; the definition is the contract in include/gmr_amd.h): per frame the smallest clearance over
        the pair table, the pair that attains it and the number of pairs below ``margin``; per clip the deepest frame, its pair,
        the colliding frames and their longest run.  ``seq_offsets`` ``[S + 1]``: the clips' rows, a host sequence (uploaded once)
        or a device int64 tensor.  ``capsules`` / ``pairs``: a :class:`gmr_amd.collision.CapsuleTable` and
        :class:`gmr_amd.collision.PairTable`; ``None``: the skeleton's (:meth:`default_proxies` -- capsules of 0.03 m along the
        links, a convention, not the robot's collision geometry), and ``pairs=None`` alone: ``default_pairs`` of ``capsules``.
        ``stats=False`` leaves the per-clip statistics out (one kernel).  Returns a :class:`MotionSelfCollision` of device tensors;
        ``out``: caller-owned result tensors by name (a name left out is not computed; a statistic needs ``clearance``, ``pair``
        and ``hits``).  Asynchronous on the current stream; with ``out``, cached tables and a device ``seq_offsets`` no allocation,
        no copy, no synchronisation."""
        capsules, pairs = self.resolve_proxies(capsules, pairs)
        ci, res, keep = _self_collision_input(self, qpos, seq_offsets, capsules, pairs, margin, out, stats)
        ci.stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.gmr_motion_self_collision(self._h, C.byref(ci)), "gmr_motion_self_collision")
        return res

    def motion_self_collision_repair(self, qpos: torch.Tensor, seq_offsets, capsules=None, pairs=None, margin: float = 0.0,
                                     iterations: int = SELF_COLLISION_REPAIR_DEFAULTS["iterations"],
                                     damping: float = SELF_COLLISION_REPAIR_DEFAULTS["damping"],
                                     step_cap: float = SELF_COLLISION_REPAIR_DEFAULTS["step_cap"],
                                     resolve_tol: float = SELF_COLLISION_REPAIR_DEFAULTS["resolve_tol"], movable=None, out=None,
                                     stats: bool = True, stream=None) -> MotionSelfCollisionRepair:
        """Push the colliding capsule pairs of qpos ``[N, nq]`` float64 (engine layout, concatenated clips) apart in two kernels
        (``gmr_motion_self_collision_repair``; the definition is the contract in include/gmr_amd.h): in every frame in which a
        pair of the table is closer than ``margin``, ``iterations`` damped projection passes (``damping`` = lambda^2 in m^2, steps
        of at most ``step_cap`` rad) over the hinges between the pair's two bodies move it back to the margin; a frame below
        ``margin - resolve_tol`` afterwards counts as unresolved.  The defaults (16 passes, 1e-6 m^2, 0.2 rad, 1e-4 m) are
        conventions, not measured on a robot.  ``seq_offsets``, ``capsules`` and ``pairs`` as in :meth:`motion_self_collision`.
        ``movable``: a 64-bit mask, bit ``i`` for hinge ``i`` in qpos order (``gmr_amd.collision.movable_mask``; ``None``: every
        hinge).  The root never moves.  ``stats=False`` leaves the per-clip statistics out (one kernel).  Returns a
        :class:`MotionSelfCollisionRepair` of device tensors; ``out``: caller-owned result tensors by name (``qpos`` is required
        and must not be the input; a name left out is not computed; a statistic needs the three per-frame arrays).  ``stream``: a
        ``torch.cuda.Stream`` (``None``: the current one).  Asynchronous; with ``out``, cached tables and a device ``seq_offsets``
        no allocation, no copy, no synchronisation.  A planar base is refused."""
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        with torch.cuda.stream(st):
            capsules, pairs = self.resolve_proxies(capsules, pairs)
            ri, res, keep = _self_collision_repair_input(self, qpos, seq_offsets, capsules, pairs, margin, iterations, damping, step_cap,
                                                         resolve_tol, movable, out, stats)
        ri.stream = st.cuda_stream
        self._check(self._lib.gmr_motion_self_collision_repair(self._h, C.byref(ri)), "gmr_motion_self_collision_repair")
        return res

    def symmetry_plan(self):
        """``gmr_amd.symmetry.plan_symmetry`` of the robot at the default tolerances, made once per engine.  Raises
        ``gmr_amd.symmetry.SymmetryError`` for a robot that is not left-right symmetric within them."""
        if self._symmetry_default is None:
            from .symmetry import plan_symmetry
            self._symmetry_default = plan_symmetry(self.cm.robot)
        return self._symmetry_default

    def symmetry_device(self, plan):
        """``col_src`` (int32) and ``col_sign`` (float64) of a :class:`gmr_amd.symmetry.SymmetryPlan` on the engine's device, checked
        (the involution and ``7 <= col_src[c] < nq``: what ``gmr_motion_mirror`` trusts) and uploaded once per plan; its identity is
        the key, so a plan changed in place needs a new object."""
        cache = self._symmetry_dev
        key = id(plan)
        if key not in cache:
            plan.check()
            plan.check_robot(self.cm.robot)
            cache[key] = ({"col_src": torch.from_numpy(np.ascontiguousarray(plan.col_src, dtype=np.int32)).to(self.device),
                           "col_sign": torch.from_numpy(np.ascontiguousarray(plan.col_sign, dtype=np.float64)).to(self.device)},)
            weakref.finalize(plan, cache.pop, key, None)
        return cache[key][0]

    def motion_mirror(self, qpos: torch.Tensor, seq_offsets, plan=None, about: str = "world", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The left-right mirrored copy of qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in one kernel
        (``gmr_motion_mirror``; the definition is the contract in include/gmr_amd.h): the hinge columns permuted with signs by
        ``plan`` (a :class:`gmr_amd.symmetry.SymmetryPlan`; ``None``: :meth:`symmetry_plan`, which refuses an asymmetric robot), the
        root reflected in the world plane y = 0 (``about="world"``) or, per clip, in the vertical plane through the clip's first
        root position along its heading (``about="start"``: the mirrored clip starts where the original does, facing the same way).
        ``seq_offsets`` ``[S + 1]``: a host sequence (uploaded once) or a device int64 tensor.  Rows outside every clip are not
        written: without ``out`` they hold a copy of the input.  ``out``: a caller-owned ``[N, nq]`` tensor, not ``qpos``.
        Asynchronous on the current stream; with ``out``, a cached plan and a device ``seq_offsets`` no allocation, no copy, no
        synchronisation."""
        dev = self.device
        if about not in _native.MIRROR_MODES:
            raise ValueError(f"about must be one of {sorted(_native.MIRROR_MODES)}")
        N = _qpos_rows(qpos, self.nq, dev)
        offs = _clip_offsets(seq_offsets, dev)
        tab = self.symmetry_device(self.symmetry_plan() if plan is None else plan)
        if out is None:
            out = qpos.clone()  # rows outside every clip are not written
        elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float64 or tuple(out.shape) != tuple(qpos.shape) \
                or not out.is_contiguous():
            raise EngineError("out must be a contiguous float64 tensor of qpos's shape on the engine's device")
        elif out.numel() and out.data_ptr() == qpos.data_ptr():
            raise EngineError("out must not be qpos: a row is permuted, so the call cannot work in place")
        mi = _native.MirrorInput()
        mi.qpos, mi.n_frames, mi.seq_offsets, mi.n_seq = qpos.data_ptr(), N, offs.data_ptr(), int(offs.shape[0]) - 1
        mi.mode, mi.col_src, mi.col_sign, mi.qpos_out = _native.MIRROR_MODES[about], tab["col_src"].data_ptr(), tab["col_sign"].data_ptr(), out.data_ptr()
        mi.stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.gmr_motion_mirror(self._h, C.byref(mi)), "gmr_motion_mirror")
        return out

    def compose_device(self, plan):
        """The five tables of a :class:`gmr_amd.compose.ComposePlan` on the engine's device, uploaded once per plan (the plan
        checked its invariants when it was made: what ``gmr_motion_compose`` trusts); its identity is the key."""
        cache = self._compose_dev
        key = id(plan)
        if key not in cache:
            cache[key] = ({k: torch.from_numpy(np.array(v)).to(self.device) for k, v in plan.tables().items()},)  # (a copy: the plan's are read-only)
            weakref.finalize(plan, cache.pop, key, None)
        return cache[key][0]

    def motion_compose(self, qpos: torch.Tensor, plan, stream=None, out: Optional[torch.Tensor] = None,
                       transform_out: Optional[torch.Tensor] = None):
        """Composed clips from qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in two kernels
        (``gmr_motion_compose``; the definition is the contract in include/gmr_amd.h): every segment of ``plan`` (a
        :class:`gmr_amd.compose.ComposePlan` made for these ``N`` rows) moved in the plane onto the end of the segment before it
        and cross-faded into it over their overlap.  Returns ``(qpos_out [plan.n_out_frames, nq], seg_transform [plan.n_seg, 6])``:
        the clips of ``plan.out_offsets``, and ``(c, s, tx, ty, hw, hz)`` of every segment's placement.  ``stream``: a
        ``torch.cuda.Stream`` (``None``: the current one).  ``out`` / ``transform_out``: caller-owned tensors of those shapes.
        The plan's tables are uploaded once per plan.  Asynchronous; with ``out``, ``transform_out`` and a cached plan no
        allocation, no copy, no synchronisation."""
        dev = self.device
        if self.cm.robot.planar_base:
            raise NotImplementedError("composing assumes a free-joint root; a planar-base robot is not supported")
        N = _qpos_rows(qpos, self.nq, dev)
        if N != plan.n_frames:
            raise EngineError(f"the plan was made for {plan.n_frames} source rows, qpos has {N}")
        st = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(st):
            tab = self.compose_device(plan)
            shapes = {"out": (plan.n_out_frames, self.nq), "transform_out": (plan.n_seg, 6)}
            res = {}
            for name, t in (("out", out), ("transform_out", transform_out)):
                if t is None:
                    t = torch.empty(shapes[name], dtype=torch.float64, device=dev)
                elif not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float64 or tuple(t.shape) != shapes[name] \
                        or not t.is_contiguous():
                    raise EngineError(f"{name} must be a contiguous float64 {list(shapes[name])} tensor on the engine's device")
                res[name] = t
        if res["out"].numel() and res["out"].data_ptr() == qpos.data_ptr():
            raise EngineError("out must not be qpos: an output row reads other rows")
        ci = _native.ComposeInput()
        ci.qpos, ci.n_frames = qpos.data_ptr(), N
        for k, t in tab.items():
            setattr(ci, k, t.data_ptr())
        ci.n_seg, ci.n_out, ci.n_out_frames = plan.n_seg, plan.n_out, plan.n_out_frames
        ci.qpos_out, ci.seg_transform, ci.stream = res["out"].data_ptr(), res["transform_out"].data_ptr(), st.cuda_stream
        self._check(self._lib.gmr_motion_compose(self._h, C.byref(ci)), "gmr_motion_compose")
        return res["out"], res["transform_out"]

    def motion_transitions(self, qpos: torch.Tensor, seq_offsets, body_ids, weights, window: int, src_clips=None, dst_clips=None,
                           stride: int = 1, min_gap: int = 0, dense: bool = False, stream=None, out=None) -> "MotionTransitions":
        """The transition search over qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in three kernels
        (``gmr_motion_transitions``; the definition is the contract in include/gmr_amd.h): for every ``stride``-th frame of the
        clips ``src_clips`` the motion-graph cost of its window of ``window`` frames against every window of every clip of
        ``dst_clips`` (``None``: all clips), reduced to the best target frame per (source, target clip).  ``seq_offsets`` ``[S + 1]``
        is a host sequence: the source and target tables are made from it (``gmr_amd.transitions.search_tables``).  ``body_ids``
        ``[P]``: the bodies whose positions are the points; ``weights`` ``[P]`` >= 0, normalised here to sum 1.  Same clip on both
        sides: pairs with ``|j - i| < min_gap`` are excluded.  Returns a :class:`MotionTransitions` of device tensors ``points``
        ``[N, P, 3]``, ``moments`` ``[N, 6]``, ``best_cost`` ``[E, D]`` float64, ``best_frame`` ``[E, D]`` int32 and, with
        ``dense=True``, ``cost_out`` ``[E, n_targets]``, with the host tables as attributes.  ``stream``: a ``torch.cuda.Stream``
        (``None``: the current one).  ``out``: caller-owned tensors by those names.  Asynchronous; the tables (a few integers per
        clip) are uploaded in every call."""
        from .transitions import search_tables
        dev = self.device
        N = _qpos_rows(qpos, self.nq, dev)
        offs = np.ascontiguousarray(seq_offsets.cpu().numpy() if isinstance(seq_offsets, torch.Tensor) else seq_offsets, dtype=np.int64)
        src, src_offs, dst, dst_offs = search_tables(offs, src_clips, dst_clips, window, stride)
        if int(offs[-1]) > N:
            raise EngineError(f"seq_offsets ends at row {int(offs[-1])}, qpos has {N}")
        ids = np.ascontiguousarray(body_ids, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if ids.size < 1 or ids.size != w.size or ids.size > _native.TRANSITIONS_MAX_BODIES:
            raise ValueError(f"body_ids and weights must hold the same 1 .. {_native.TRANSITIONS_MAX_BODIES} entries")
        if ids.min() < 0 or ids.max() >= self.nbody:
            raise ValueError(f"body_ids must lie in [0, {self.nbody})")
        if not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.sum() > 0.0:
            raise ValueError("weights must be finite, not negative, and not all zero")
        if int(min_gap) < 0:
            raise ValueError("min_gap must not be negative")
        w = w / w.sum()
        E, D, NT, P = int(src_offs[-1]), int(dst.size), int(dst_offs[-1]), int(ids.size)
        f64, i32 = torch.float64, torch.int32
        shapes = {"points": ((N, P, 3), f64), "moments": ((N, _native.TRANSITIONS_MOMENTS), f64), "best_cost": ((E, D), f64),
                  "best_frame": ((E, D), i32)}
        if dense:
            shapes["cost_out"] = ((E, NT), f64)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(st):
            tabs = {k: torch.from_numpy(v).to(dev) for k, v in (("seq_offsets", offs), ("body_ids", ids), ("weights", w), ("src_clips", src),
                                                                ("src_offsets", src_offs), ("dst_clips", dst), ("dst_offsets", dst_offs))}
            if out is None:
                # a call without work launches nothing, and rows outside every clip are not written
                fill = {"points": float("nan"), "moments": float("nan"), "best_cost": float("inf"), "best_frame": -1, "cost_out": float("inf")}
                res = {k: torch.full(sh, fill[k], dtype=dt, device=dev) for k, (sh, dt) in shapes.items()}
            else:
                if set(out) != set(shapes) or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[k][0] or t.dtype != shapes[k][1]
                                                  or t.device != dev or not t.is_contiguous() for k, t in out.items()):
                    raise EngineError(f"out must map {sorted(shapes)} to contiguous tensors of the call's shapes on the engine's device")
                res = {k: out[k] for k in shapes}
        ti = _native.TransitionsInput()
        ti.qpos, ti.n_frames, ti.seq_offsets, ti.n_seq, ti.n_bodies = qpos.data_ptr(), N, tabs["seq_offsets"].data_ptr(), int(offs.size) - 1, P
        ti.window, ti.src_stride, ti.min_gap, ti.n_src_clips, ti.n_dst_clips = int(window), int(stride), int(min_gap), int(src.size), D
        for k in ("body_ids", "weights", "src_clips", "src_offsets", "dst_clips", "dst_offsets"):
            setattr(ti, k, tabs[k].data_ptr())
        ti.n_sources, ti.n_targets, ti.stream = E, NT, st.cuda_stream
        for k, t in res.items():
            setattr(ti, k, t.data_ptr())
        self._check(self._lib.gmr_motion_transitions(self._h, C.byref(ti)), "gmr_motion_transitions")
        for t in tabs.values():
            t.record_stream(st)
        mt = MotionTransitions(res)
        mt.src_clips, mt.src_offsets, mt.dst_clips, mt.dst_offsets = src, src_offs, dst, dst_offs
        mt.window, mt.stride, mt.min_gap, mt.weights = int(window), int(stride), int(min_gap), w
        return mt

    def motion_retime_plan(self, qpos: torch.Tensor, seq_offsets, fps: float, vmax, window: int, max_stretch: float, out=None) -> MotionRetimePlan:
        """The time warp that plays qpos ``[N, nq]`` float64 (engine layout, concatenated clips at the one rate ``fps``) slower exactly
        where a hinge turns faster than ``vmax`` ``[nq - 7]`` rad/s (qpos order, every entry > 0, ``inf``: no limit), in three kernels
        (``gmr_motion_retime_plan``; the definition is the contract in include/gmr_amd.h): per interval the need, the stretch
        capped at ``max_stretch`` (1 .. 64), widened and averaged over ``window`` (0 .. 32) intervals on either side, as integer ticks
        of 1/1024 frame; per clip their prefix sum, the output length and the statistics.  ``seq_offsets`` ``[S + 1]``: a host
        sequence (uploaded once) or a device int64 tensor.  ``vmax``: a host sequence (checked, uploaded) or a device float64
        tensor (trusted).  Returns a :class:`MotionRetimePlan` of device tensors; ``out``: caller-owned tensors by all its names.
        Asynchronous on the current stream; with ``out``, a device ``seq_offsets`` and a device ``vmax`` no allocation, no copy, no
        synchronisation."""
        dev = self.device
        if self.cm.robot.planar_base:
            raise NotImplementedError("retiming assumes a free-joint root; a planar-base robot is not supported")
        N = _qpos_rows(qpos, self.nq, dev)
        offs = _clip_offsets(seq_offsets, dev)
        S, nh = int(offs.shape[0]) - 1, self.nq - 7
        fps, window, max_stretch = float(fps), int(window), float(max_stretch)
        if not np.isfinite(fps) or not fps > 0.0:
            raise ValueError("fps must be finite and > 0")
        if not 0 <= window <= _native.RETIME_MAX_WINDOW:
            raise ValueError(f"window must lie in [0, {_native.RETIME_MAX_WINDOW}]")
        if not 1.0 <= max_stretch <= _native.RETIME_MAX_STRETCH:
            raise ValueError(f"max_stretch must lie in [1, {_native.RETIME_MAX_STRETCH:g}]")
        if isinstance(vmax, torch.Tensor):
            if vmax.device != dev or vmax.dtype != torch.float64 or tuple(vmax.shape) != (nh,) or not vmax.is_contiguous():
                raise EngineError(f"vmax must be a contiguous float64 [{nh}] tensor on the engine's device (or a host sequence)")
        else:
            v = np.ascontiguousarray(vmax, dtype=np.float64)
            if v.shape != (nh,) or not np.all(v > 0.0):
                raise ValueError(f"vmax must hold {nh} limits, every one > 0 (inf: no limit)")
            vmax = torch.from_numpy(v).to(dev)
        f64, i64 = torch.float64, torch.int64
        shapes = {"need": ((N,), f64), "ticks": ((N,), i64), "cum": ((N,), i64), "out_len": ((S,), i64), "clip_stats": ((S, 4), i64),
                  "need_max": ((S,), f64)}
        if out is None:
            res = {k: torch.zeros(sh, dtype=dt, device=dev) for k, (sh, dt) in shapes.items()}  # rows outside every clip are not written
        else:
            if set(out) != set(shapes) or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[k][0] or t.dtype != shapes[k][1]
                                              or t.device != dev or not t.is_contiguous() for k, t in out.items()):
                raise EngineError(f"out must map {sorted(shapes)} to contiguous tensors of the call's shapes on the engine's device")
            res = {k: out[k] for k in shapes}
        pi = _native.RetimePlanInput()
        pi.qpos, pi.n_frames, pi.seq_offsets, pi.n_seq, pi.window = qpos.data_ptr(), N, offs.data_ptr(), S, window
        pi.fps, pi.vmax, pi.max_stretch = fps, vmax.data_ptr(), max_stretch
        for k, t in res.items():
            setattr(pi, k, t.data_ptr())
        pi.stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.gmr_motion_retime_plan(self._h, C.byref(pi)), "gmr_motion_retime_plan")
        plan = MotionRetimePlan(res)
        plan.seq_offsets, plan.fps, plan.window, plan.max_stretch = offs, fps, window, max_stretch
        return plan

    def motion_retime_plan_torque(self, tau: torch.Tensor, tau_static: torch.Tensor, seq_offsets, torque_limit, limit_scale: float,
                                  window: int, max_stretch: float, need_floor=None, align_end: bool = True, out=None) -> MotionRetimePlan:
        """The time warp that plays clips slower exactly where a hinge needs more torque than ``limit_scale * torque_limit``
        (``gmr_motion_retime_plan_torque``; the definition is the contract above ``gmr_retime_torque_input`` in include/gmr_amd.h).
        ``tau`` and ``tau_static`` ``[N, nq - 7]`` float64: ``motion_dynamics``' ``tau`` of the clips, differenced and with zero
        ``qvel`` / ``qacc``.  ``seq_offsets`` ``[S + 1]``: a host sequence (uploaded once) or a device int64 tensor.  ``torque_limit``
        ``[nq - 7]`` N m (every entry > 0, ``inf``: no limit): a host sequence (checked, uploaded) or a device float64 tensor
        (trusted).  ``limit_scale`` in (0, 1]; ``window`` 0 .. 32; ``max_stretch`` 1 .. 64.  ``need_floor`` ``[N]`` float64 on the
        device or ``None``: the ``need`` of a ``motion_retime_plan`` of the same clips, so that one warp meets both limits.
        ``align_end``: pad every clip's total to whole frames over its last intervals, so that the last output row is the final pose
        at its planned time.  Returns a :class:`MotionRetimePlan` for ``motion_retime_apply`` (``fps`` is ``None``) that also holds
        ``static_over`` ``[N]`` int32: per row the hinges whose gravity torque alone is at or over the scaled limit.  ``out``:
        caller-owned tensors by all its names.  Asynchronous on the current stream; with ``out`` and device arrays no allocation,
        no copy, no synchronisation."""
        dev = self.device
        if self.cm.robot.planar_base:
            raise NotImplementedError("retiming assumes a free-joint root; a planar-base robot is not supported")
        nh = self.nq - 7
        for name, t in (("tau", tau), ("tau_static", tau_static)):
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != nh \
                    or t.shape[0] != tau.shape[0] or not t.is_contiguous():
                raise EngineError(f"{name} must be a contiguous float64 [N, {nh}] tensor on the engine's device")
        N = int(tau.shape[0])
        offs = _clip_offsets(seq_offsets, dev)
        S = int(offs.shape[0]) - 1
        limit_scale, window, max_stretch = float(limit_scale), int(window), float(max_stretch)
        if not 0.0 < limit_scale <= 1.0:
            raise ValueError("limit_scale must lie in (0, 1]")
        if not 0 <= window <= _native.RETIME_MAX_WINDOW:
            raise ValueError(f"window must lie in [0, {_native.RETIME_MAX_WINDOW}]")
        if not 1.0 <= max_stretch <= _native.RETIME_MAX_STRETCH:
            raise ValueError(f"max_stretch must lie in [1, {_native.RETIME_MAX_STRETCH:g}]")
        if isinstance(torque_limit, torch.Tensor):
            if torque_limit.device != dev or torque_limit.dtype != torch.float64 or tuple(torque_limit.shape) != (nh,) or not torque_limit.is_contiguous():
                raise EngineError(f"torque_limit must be a contiguous float64 [{nh}] tensor on the engine's device (or a host sequence)")
        else:
            v = np.array(torque_limit, dtype=np.float64)  # (a copy: the caller's may be read-only)
            if v.shape != (nh,) or not np.all(v > 0.0):
                raise ValueError(f"torque_limit must hold {nh} limits, every one > 0 (inf: no limit)")
            torque_limit = torch.from_numpy(v).to(dev)
        if need_floor is not None and (not isinstance(need_floor, torch.Tensor) or need_floor.device != dev or need_floor.dtype != torch.float64
                                       or tuple(need_floor.shape) != (N,) or not need_floor.is_contiguous()):
            raise EngineError(f"need_floor must be a contiguous float64 [{N}] tensor on the engine's device (or None)")
        f64, i64 = torch.float64, torch.int64
        shapes = {"need": ((N,), f64), "ticks": ((N,), i64), "cum": ((N,), i64), "out_len": ((S,), i64), "clip_stats": ((S, 4), i64),
                  "need_max": ((S,), f64), "static_over": ((N,), torch.int32)}
        if out is None:
            res = {k: torch.zeros(sh, dtype=dt, device=dev) for k, (sh, dt) in shapes.items()}  # rows outside every clip are not written
        else:
            if set(out) != set(shapes) or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[k][0] or t.dtype != shapes[k][1]
                                              or t.device != dev or not t.is_contiguous() for k, t in out.items()):
                raise EngineError(f"out must map {sorted(shapes)} to contiguous tensors of the call's shapes on the engine's device")
            res = {k: out[k] for k in shapes}
        ti = _native.RetimeTorqueInput()
        ti.tau, ti.tau_static, ti.n_frames, ti.seq_offsets, ti.n_seq, ti.window = tau.data_ptr(), tau_static.data_ptr(), N, offs.data_ptr(), S, window
        ti.torque_limit, ti.limit_scale, ti.max_stretch = torque_limit.data_ptr(), limit_scale, max_stretch
        ti.need_floor, ti.align_end = (need_floor.data_ptr() if need_floor is not None else None), int(bool(align_end))
        for k, t in res.items():
            setattr(ti, k, t.data_ptr())
        ti.stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.gmr_motion_retime_plan_torque(self._h, C.byref(ti)), "gmr_motion_retime_plan_torque")
        plan = MotionRetimePlan(res)
        plan.seq_offsets, plan.fps, plan.window, plan.max_stretch = offs, None, window, max_stretch
        plan.limit_scale, plan.align_end = limit_scale, bool(align_end)
        return plan

    def motion_retime_apply(self, qpos: torch.Tensor, seq_offsets, plan, out_offsets=None, out=None, interp: str = "linear"):
        """qpos ``[N, nq]`` float64 resampled along ``plan`` (a :class:`MotionRetimePlan` of these clips, or a mapping with its
        ``ticks`` and ``cum``) in one kernel (``gmr_motion_retime_apply``; the definition is the contract in include/gmr_amd.h).
        ``interp``: ``"linear"`` (the lerp and slerp between the two source rows) or ``"cubic"`` (Catmull-Rom over four rows: C1,
        what a plan from torques needs; it may overshoot a joint range and, by a little, a velocity limit).
        ``out_offsets`` ``[S + 1]``: the output clips' rows, a host sequence or a device int64 tensor; ``None``: the prefix sum of
        ``plan["out_len"]``, which is READ BACK from the device -- a host synchronisation.  Returns ``(qpos_out [M, nq], src_time [M],
        out_offsets)``: the retimed clips, per output row the source time in frames of its clip, and the offsets (a host int64 array,
        or the device tensor that was given).  ``out``: caller-owned ``{"qpos": [M, nq], "src_time": [M]}`` float64 tensors, required
        with a device ``out_offsets``; with ``out`` M is its number of rows (the offsets are clamped into them), without it the last
        offset; ``out["qpos"]`` must not be ``qpos``.  Asynchronous on the current
        stream; with ``out`` and device offsets no allocation, no copy, no synchronisation."""
        dev = self.device
        if self.cm.robot.planar_base:
            raise NotImplementedError("retiming assumes a free-joint root; a planar-base robot is not supported")
        if interp not in _native.RETIME_INTERP:
            raise ValueError(f"interp must be one of {sorted(_native.RETIME_INTERP)}")
        N = _qpos_rows(qpos, self.nq, dev)
        offs = _clip_offsets(seq_offsets, dev)
        S = int(offs.shape[0]) - 1
        for k in ("ticks", "cum"):
            t = plan[k]
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int64 or tuple(t.shape) != (N,) or not t.is_contiguous():
                raise EngineError(f"plan[{k!r}] must be a contiguous int64 [{N}] tensor on the engine's device")
        if out_offsets is None:
            oo = np.concatenate([[0], np.cumsum(plan["out_len"].cpu().numpy())]).astype(np.int64)  # the pair's one host synchronisation
            if oo.size != S + 1:
                raise EngineError(f"the plan was made for {oo.size - 1} clips, seq_offsets has {S}")
            ret_offs, M = oo, int(oo[-1])
            oo = torch.from_numpy(oo).to(dev)
        elif isinstance(out_offsets, torch.Tensor):
            oo = ret_offs = _clip_offsets(out_offsets, dev, "out_offsets")
            if out is None:
                raise EngineError("a device out_offsets needs out: its tensors say how many output rows there are")
            M = -1
        else:
            ret_offs = np.array(out_offsets, dtype=np.int64)  # (a copy: the caller's may be read-only)
            oo = _clip_offsets(ret_offs, dev, "out_offsets")
            M = int(ret_offs[-1])
        if out is not None and isinstance(out.get("qpos"), torch.Tensor) and out["qpos"].dim() == 2:
            M = int(out["qpos"].shape[0])  # (the offsets are clamped into the rows there are, as seq_offsets is)
        if int(oo.shape[0]) != S + 1:
            raise EngineError(f"out_offsets must hold {S + 1} entries")
        shapes = {"qpos": ((M, self.nq), torch.float64), "src_time": ((M,), torch.float64)}
        if out is None:
            res = {k: torch.zeros(sh, dtype=dt, device=dev) for k, (sh, dt) in shapes.items()}  # rows outside every clip are not written
        else:
            if set(out) != set(shapes) or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[k][0] or t.dtype != shapes[k][1]
                                              or t.device != dev or not t.is_contiguous() for k, t in out.items()):
                raise EngineError(f"out must map {sorted(shapes)} to contiguous float64 tensors of {M} rows on the engine's device")
            res = {k: out[k] for k in shapes}
        if res["qpos"].numel() and res["qpos"].data_ptr() == qpos.data_ptr():
            raise EngineError("out must not be qpos: an output row reads other rows")
        ai = _native.RetimeApplyInput()
        ai.qpos, ai.n_frames, ai.seq_offsets, ai.n_seq = qpos.data_ptr(), N, offs.data_ptr(), S
        ai.ticks, ai.cum, ai.out_offsets, ai.n_out_frames = plan["ticks"].data_ptr(), plan["cum"].data_ptr(), oo.data_ptr(), M
        ai.qpos_out, ai.src_time, ai.interp = res["qpos"].data_ptr(), res["src_time"].data_ptr(), _native.RETIME_INTERP[interp]
        ai.stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.gmr_motion_retime_apply(self._h, C.byref(ai)), "gmr_motion_retime_apply")
        return res["qpos"], res["src_time"], ret_offs

    def clip_report(self, qpos: torch.Tensor, seq_offsets, pos: Optional[torch.Tensor] = None, quat: Optional[torch.Tensor] = None,
                    slot_col: Optional[np.ndarray] = None, height_scale=None, iters: Optional[torch.Tensor] = None,
                    offset_to_ground: bool = False, limit_eps: float = CLIP_REPORT_LIMIT_EPS, segment_frames: int = 0) -> ClipReport:
        """Per-clip quality statistics of qpos ``[N, nq]`` float64 (engine layout, concatenated clips) in one fused pass
        (``gmr_clip_report``): see :class:`ClipReport`.  ``pos`` / ``quat`` / ``slot_col`` as in :meth:`evaluate` (without them the
        error fields are ``None``); ``height_scale [S]``: per-clip factor on the human scale table; ``iters [N]`` int32: the solve
        counts of ``ik_solve``; ``segment_frames``: frames per wavefront, 0 = ``CLIP_REPORT_SEGMENT`` (maxima and counts do not
        depend on it, sums to rounding).  Asynchronous on the current stream."""
        ri, rep, keep = _report_input(self, qpos, pos, quat, slot_col, seq_offsets, height_scale, iters)
        prm = _native.ClipReportParams(limit_eps, segment_frames, int(bool(offset_to_ground)))
        self._check(self._lib.gmr_clip_report(self._h, C.byref(ri), C.byref(prm), self._stream()), "gmr_clip_report")
        return rep


class EngineGroup:
    """Several robots' batches in ONE launch (``gmr_group_*``; BASELINE config 4, "heterogeneous trees in one launch").

    The members are built for one common kernel variant; ``ik_solve`` takes one batch per member and runs all their work items
    in a single grid.  ``engines[i]`` is member i as an ordinary ``Engine`` (FK, evaluate, sessions, its own launches).
    """

    def __init__(self, cms, device: int = 0):
        if not torch.cuda.is_available():
            raise EngineError("no HIP device visible to torch: the gmr_amd engine has no CPU path")
        self._lib = _native.load()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        n = len(cms)
        blobs = (C.c_char_p * n)(*[cm.blob for cm in cms])
        sizes = (C.c_size_t * n)(*[len(cm.blob) for cm in cms])
        err = C.create_string_buffer(512)
        self._g = self._lib.gmr_group_create(blobs, sizes, n, self.device_index, err, len(err))
        if not self._g:
            raise EngineError(f"gmr_group_create: {err.value.decode()}")
        self.engines = [Engine(cm, device, _borrowed_handle=self._lib.gmr_group_model(self._g, i)) for i, cm in enumerate(cms)]

    def close(self):
        if getattr(self, "_g", None):
            for e in self.engines:
                e.close()
            self._lib.gmr_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    STATE_KEYS = ("qpos_init", "qpos_final", "n_final", "frames_done", "out", "iters")

    def _inputs(self, batches, with_outputs: bool = True):
        """Validate every member's batch and fill the C input array.  Returns (inputs, per-member results, per-member items, keep-alive)."""
        if len(batches) != len(self.engines):
            raise EngineError("one batch (or None) per group member")
        inputs = (_native.GroupInput * len(batches))()
        keep, outs, all_items = [], [], []
        for i, (eng, b) in enumerate(zip(self.engines, batches)):
            all_items.append(np.zeros(0, dtype=_native.WORK_ITEM_DTYPE))
            if b is None:
                outs.append((None, None))
                continue
            what = f"member {i}: "
            state = isinstance(b, dict)
            kw = {}
            if state:
                unknown = set(b) - {"pos", "quat", "slot_col", "items"} - set(self.STATE_KEYS)
                if unknown:
                    raise EngineError(what + f"unknown batch keys {sorted(unknown)}")
                pos, quat, slot_col, items = b["pos"], b["quat"], b["slot_col"], b["items"]
                kw = {k: b[k] for k in self.STATE_KEYS if b.get(k) is not None}
                kw["n_final"] = int(kw.get("n_final", 0))
            else:
                pos, quat, slot_col, items = b
                items = np.ascontiguousarray(items, dtype=_native.WORK_ITEM_DTYPE)
                if len(items) and (int(items["init_row"].max()) >= 0 or int(items["final_row"].max()) >= 0 or int(items["burn_row"].max()) >= 0):
                    raise EngineError("group launches take plain per-clip items (no state rows) unless the batch supplies the state arrays")
            pos, quat, slot_col, items, out, iters, qinit, qfin = _ik_batch(eng, pos, quat, slot_col, items, with_outputs=with_outputs,
                                                                            what=what, **kw)
            done = kw.get("frames_done")
            if len(items) and qinit is None and int(items["init_row"].max()) >= 0:
                raise EngineError(what + "init_row outside qpos_init")
            N, B = int(pos.shape[0]), int(pos.shape[1])
            outs.append((out, iters, qfin) if state else (out, iters))
            keep += [pos, quat, items, slot_col, qinit]
            if N == 0 or len(items) == 0:
                continue
            all_items[i] = items
            inputs[i].human_pos, inputs[i].human_quat = pos.data_ptr(), quat.data_ptr()
            inputs[i].in_dtype = _native.GMR_DTYPE_F64 if pos.dtype == torch.float64 else _native.GMR_DTYPE_F32
            inputs[i].n_cols, inputs[i].slot_col, inputs[i].n_frames = B, slot_col.ctypes.data, N
            inputs[i].items, inputs[i].n_items = items.ctypes.data, len(items)
            inputs[i].qpos_init = None if qinit is None else qinit.data_ptr()
            inputs[i].qpos_final = None if qfin is None else qfin.data_ptr()
            inputs[i].frames_done = None if done is None else done.data_ptr()
            if with_outputs:
                inputs[i].qpos_out, inputs[i].iters_out = out.data_ptr(), iters.data_ptr()
        return inputs, outs, all_items, keep

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.gmr_group_last_error(self._g)
            raise EngineError(f"{what}: {_ERR.get(rc, rc)}: {msg.decode() if msg else ''}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def ik_solve(self, batches, params: Optional[IKParams] = None, launch_order=None):
        """``batches[i]`` for member i: ``(pos, quat, slot_col, items)``, or ``None`` (no work), or a dict with the keys ``pos``, ``quat``,
        ``slot_col``, ``items`` and any of ``qpos_init``, ``qpos_final`` (or ``n_final``), ``frames_done``, ``out``, ``iters`` -- the
        state arrays and outputs of ``Engine.ik_solve``, validated the same way; only such a batch may carry items with state rows
        (chunks, verification walks).  Returns per member (qpos, iters) for a tuple batch, (qpos, iters, qpos_final) for a dict.

        ``launch_order``: ``None`` (default: one grid, the member with the longest item first, each member's items longest first),
        an int32 device tensor from :meth:`plan_order` over all members' items (item k of member i has the global index
        base_i + k, base_i = the items of the members before it), or ``"auto"`` -- plan an order when ``Engine``'s probe policy
        says it pays for all members' items together (they share the wavefront slots).  The order only moves work in time."""
        prm = params or IKParams()
        inputs, outs, all_items, keep = self._inputs(batches)
        launch_order = _launch_order(self.engines[0], launch_order, all_items, lambda pf: self.plan_order(batches, prm, probe_frames=pf))
        if launch_order is None:
            self._check(self._lib.gmr_group_ik_solve(self._g, inputs, C.byref(prm), self._stream()), "gmr_group_ik_solve")
        else:
            self._check(self._lib.gmr_group_ik_solve_ordered(self._g, inputs, C.byref(prm), _ptr(launch_order), self._stream()),
                        "gmr_group_ik_solve_ordered")
        return outs

    def plan_order(self, batches, params: Optional[IKParams] = None, probe_frames: Optional[int] = None) -> torch.Tensor:
        """All members' items by predicted cost, most expensive first, across robots: int32 ``[sum of n_items]`` on the device (global
        item indices, see :meth:`ik_solve`).  Probes the first ``probe_frames`` frames of every item in one grid; asynchronous."""
        prm = params or IKParams()
        from .schedule import group_item_bases
        inputs, _, _, keep = self._inputs(batches, with_outputs=False)
        total = int(group_item_bases([inputs[i].n_items for i in range(len(batches))])[-1])
        order = torch.empty(total, dtype=torch.int32, device=self.device)
        if total == 0:
            return order
        self._check(self._lib.gmr_group_plan_order(self._g, inputs, C.byref(prm), int(probe_frames or Engine.PROBE_FRAMES), _ptr(order),
                                                   self._stream()), "gmr_group_plan_order")
        return order

    def motion_epilogue(self, batches, height_adjust: bool = True, root_origin_offset: bool = True, ground_offset: float = 0.0, min_z=None):
        """:meth:`Engine.motion_epilogue` for every member in shared launches (``gmr_group_motion_epilogue``).  ``batches[i]``:
        ``(qpos, seq_offsets)`` of member i, or ``None`` (no work); ``min_z``: ``None`` or one float32 [n_seq] tensor (or ``None``)
        per member.  Returns per member the four device tensors, or ``None``."""
        if len(batches) != len(self.engines):
            raise EngineError("one batch (or None) per group member")
        mz = [None] * len(batches) if min_z is None else list(min_z)
        if len(mz) != len(batches):
            raise EngineError("min_z: one tensor (or None) per group member")
        inputs = (_native.MotionInput * len(batches))()
        outs, keep = [], []
        for i, (eng, b) in enumerate(zip(self.engines, batches)):
            if b is None:
                outs.append(None)
                continue
            qpos, offs = b
            mi, res, k = _motion_input(eng, qpos, offs, height_adjust, root_origin_offset, ground_offset, None, mz[i], f"member {i}: ")
            inputs[i] = mi
            outs.append(res)
            keep.append(k)
        self._check(self._lib.gmr_group_motion_epilogue(self._g, inputs, self._stream()), "gmr_group_motion_epilogue")
        return outs

    def motion_track(self, batches, fps_out, bodies: bool = True, lowpass_hz=0.0):
        """:meth:`Engine.motion_track` for every member, all members' tiles in one grid (``gmr_group_motion_track``).
        ``batches[i]``: ``(qpos, seq_offsets, fps_in)`` of member i, or ``None`` (no work).  ``lowpass_hz``: one cutoff, or one
        per member (0: that member is not filtered); the filtered members share one filter launch.  Returns one
        :class:`MotionTrack` (or ``None``) per member, bit for bit the single calls'."""
        if len(batches) != len(self.engines):
            raise EngineError("one batch (or None) per group member")
        cut = [lowpass_hz] * len(batches) if lowpass_hz is None or np.ndim(lowpass_hz) == 0 else list(lowpass_hz)
        if len(cut) != len(batches):
            raise EngineError("lowpass_hz: one cutoff, or one per group member")
        inputs = (_native.TrackInput * len(batches))()
        outs, keep = [], []
        for i, (eng, b) in enumerate(zip(self.engines, batches)):
            if b is None:
                outs.append(None)
                continue
            qpos, offs, fps_in = b
            ti, res, k = _track_input(eng, qpos, offs, fps_in, fps_out, None, bodies, f"member {i}: ", lowpass_hz=cut[i])
            inputs[i] = ti
            outs.append(res)
            keep.append(k)
        self._check(self._lib.gmr_group_motion_track(self._g, inputs, self._stream()), "gmr_group_motion_track")
        return outs

    def clip_report(self, batches, offset_to_ground: bool = False, limit_eps: float = CLIP_REPORT_LIMIT_EPS, segment_frames: int = 0):
        """:meth:`Engine.clip_report` for every member, all members' segments in one grid (``gmr_group_clip_report``).
        ``batches[i]``: ``None`` (no work) or a dict with ``qpos``, ``seq_offsets`` and optionally ``pos``, ``quat``, ``slot_col``,
        ``height_scale``, ``iters``.  Returns one :class:`ClipReport` (or ``None``) per member, bit for bit the single calls'."""
        if len(batches) != len(self.engines):
            raise EngineError("one batch (or None) per group member")
        inputs = (_native.ClipReportInput * len(batches))()
        outs, keep = [], []
        for i, (eng, b) in enumerate(zip(self.engines, batches)):
            if b is None:
                outs.append(None)
                continue
            unknown = set(b) - {"qpos", "seq_offsets", "pos", "quat", "slot_col", "height_scale", "iters"}
            if unknown:
                raise EngineError(f"member {i}: unknown batch keys {sorted(unknown)}")
            ri, rep, k = _report_input(eng, b["qpos"], b.get("pos"), b.get("quat"), b.get("slot_col"), b["seq_offsets"],
                                       b.get("height_scale"), b.get("iters"), f"member {i}: ")
            inputs[i] = ri
            outs.append(rep)
            keep.append(k)
        prm = _native.ClipReportParams(limit_eps, segment_frames, int(bool(offset_to_ground)))
        self._check(self._lib.gmr_group_clip_report(self._g, inputs, C.byref(prm), self._stream()), "gmr_group_clip_report")
        return outs

    def ik_solve_chunked(self, batches, chunk, burn_in: int, params: Optional[IKParams] = None, eps: float = 1e-7, height_scales=None,
                         chunk_init: int = _native.INIT_ROOT_TARGET, clip_init: int = _native.INIT_QPOS0):
        """``Engine.ik_solve_chunked`` for every member at once: ``batches[i] = (pos, quat, slot_col, seq_offsets)`` or ``None``;
        ``height_scales``: ``None`` or one entry (per-clip factors or ``None``) per member.  Launch 1 runs every member's tracked
        chunk items in one grid, launch 2 every member's verification walks in another.  Returns per member (qpos, iters, info) --
        info as the single-model call's -- or ``(None, None, None)``.

        ``chunk="auto"``: ``schedule.auto_chunk`` over the clips of ALL members (they share the wavefront slots); ``(0, 0)`` means
        whole clips, through :meth:`ik_solve` with ``launch_order="auto"``.  The choice is kept in ``last_chunk``."""
        from .schedule import auto_chunk, group_chunk_offsets, make_items
        if len(batches) != len(self.engines):
            raise EngineError("one batch (or None) per group member")
        if height_scales is not None and len(height_scales) != len(batches):
            raise EngineError("height_scales: one entry (or None) per group member")
        hs = [None] * len(batches) if height_scales is None else list(height_scales)
        offs = [None if b is None else np.asarray(b[3], dtype=np.int64) for b in batches]
        if isinstance(chunk, str):
            if chunk != "auto":
                raise EngineError("chunk must be an integer or 'auto'")
            chunk, burn_in = auto_chunk(group_chunk_offsets(offs), 8 * torch.cuda.get_device_properties(self.device).multi_processor_count)
        self.last_chunk = (int(chunk), int(burn_in))
        prm = _chunk_params(params, eps)
        if chunk <= 0:
            items = [None if b is None else make_items(o, height_scales=h, clip_init=clip_init) for b, o, h in zip(batches, offs, hs)]
            res = self.ik_solve([None if b is None else (b[0], b[1], b[2], it) for b, it in zip(batches, items)], prm, launch_order="auto")
            return [(None, None, None) if b is None else (r[0], r[1], {"chunks": len(it), "passes": 0, "resolved_frames": 0})
                    for b, r, it in zip(batches, res, items)]
        first = [None if b is None else _chunk_batch(b[0], b[1], b[2], o, chunk, burn_in, h, chunk_init, clip_init)
                 for b, o, h in zip(batches, offs, hs)]
        res = self.ik_solve(first, prm)
        second = [(None, None) if f is None else _walk_batch(f, r, o, chunk) for f, r, o in zip(first, res, offs)]
        if any(w is not None for w, _ in second):
            self.ik_solve([w for w, _ in second], prm)
        return [(None, None, None) if f is None else (r[0], r[1], info()) for f, r, (_, info) in zip(first, res, second)]


class Session:
    """One live sequence (``gmr_session_*``): a frame in, a qpos out, warm start kept on the device.

    The latency path behind ``GeneralMotionRetargeting.retarget`` -- what scripts/optitrack_to_robot.py:37-46 and the
    interactive viewers drive once per captured frame.  Host numpy in, host numpy out; no torch tensors on the path.
    """

    def __init__(self, engine: Engine, slot_col: np.ndarray, n_cols: int, params: Optional[IKParams] = None, dtype=np.float64):
        self._e = engine  # keeps the model alive for as long as the session
        self._lib = engine._lib
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("session inputs must be float32 or float64")
        self.n_cols = int(n_cols)
        sc = np.ascontiguousarray(slot_col, dtype=np.int32)
        prm = params or IKParams()
        self._h = self._lib.gmr_session_create(engine._h, int(self.dtype == np.float64), self.n_cols, sc.ctypes.data, C.byref(prm))
        if not self._h:
            msg = self._lib.gmr_last_error(engine._h)
            raise EngineError(f"gmr_session_create: {msg.decode() if msg else ''}")
        self._q = np.empty(engine.nq, dtype=np.float64)
        self._solves = C.c_int32(0)

    def step(self, pos: np.ndarray, quat: np.ndarray, offset_to_ground: bool = False):
        """pos ``[n_cols, 3]``, quat ``[n_cols, 4]`` wxyz -> (qpos ``[nq]`` float64 (fresh copy), solves spent)."""
        p = np.ascontiguousarray(pos, dtype=self.dtype)
        q = np.ascontiguousarray(quat, dtype=self.dtype)
        if p.shape != (self.n_cols, 3) or q.shape != (self.n_cols, 4):
            raise ValueError(f"expected pos [{self.n_cols},3] and quat [{self.n_cols},4], got {p.shape} and {q.shape}")
        rc = self._lib.gmr_session_step(self._h, p.ctypes.data, q.ctypes.data, int(bool(offset_to_ground)), self._q.ctypes.data,
                                        C.addressof(self._solves))
        self._e._check(rc, "gmr_session_step")
        return self._q.copy(), int(self._solves.value)

    def set_persistent(self, idle_ms: int = 200):
        """Serve the following steps from one resident wavefront fed through a pinned mailbox (``gmr_session_set_persistent``):
        lower latency per frame, identical results.  ``idle_ms = 0`` switches back to one launch per frame."""
        self._e._check(self._lib.gmr_session_set_persistent(self._h, int(idle_ms)), "gmr_session_set_persistent")

    def reset(self, qpos: Optional[np.ndarray] = None):
        q = None if qpos is None else np.ascontiguousarray(qpos, dtype=np.float64).reshape(self._e.nq)
        self._e._check(self._lib.gmr_session_reset(self._h, None if q is None else q.ctypes.data), "gmr_session_reset")

    def state(self) -> np.ndarray:
        out = np.empty(self._e.nq, dtype=np.float64)
        self._e._check(self._lib.gmr_session_state(self._h, out.ctypes.data), "gmr_session_state")
        return out

    def close(self):
        if getattr(self, "_h", None) and getattr(self._e, "_h", None):
            self._lib.gmr_session_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
