"""Dataset path: clips in -> the reference's motion dicts / pickles out, post-processing on the GPU.

Reproduces what ``process_file`` does after the retarget loop (reference
scripts/smplx_to_robot_dataset.py:93-146; the BVH variant scripts/bvh_to_robot_dataset.py:106-151 is the same
with both adjustments off):

* ``root_rot`` wxyz -> xyzw (:101-102), ``dof_pos = qpos[:, 7:]`` (:103)
* ``local_body_pos``: FK with zero root position and identity root rotation, float32 (:106-112)
* HEIGHT_ADJUST: FK with the real root, clip-global ``min z`` over all bodies, ``root_pos.z -= min`` (:118-126)
* ROOT_ORIGIN_OFFSET: subtract the first frame's root xy (:128-131)
* schema ``{fps, root_pos, root_rot, dof_pos, local_body_pos, link_body_list}`` (:134-141), read back by
  general_motion_retargeting/data_loader.py:4-18 and validated by scripts/smoke_test.py:19-72.

All clips of a batch go through two FK launches (``gmr_fk``, ``gmr_fk_min_height``); nothing is looped per clip
on the device.
"""
from __future__ import annotations

import os
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .motion_retarget import GeneralMotionRetargeting


def motions_from_qpos(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps,
                      height_adjust: bool = True, root_origin_offset: bool = True, ground_offset: float = 0.0) -> List[Dict]:
    """qpos ``[N, nq]`` float64 on the GPU (concatenated clips) -> one motion dict per clip.

    The arrays of the returned dicts are row slices of four batch-sized PAGE-LOCKED host arrays (no per-clip copy): any surviving
    motion dict keeps its whole batch pinned -- gigabytes for a dataset-sized batch.  Write the clips (``MotionWriter``) and drop
    them, or ``copy()`` the arrays of a clip that has to outlive its batch."""
    if gmr.model.planar_base:
        # the dataset scripts read a free-joint root out of qpos (root_pos = qpos[:3], root_rot = qpos[3:7],
        # scripts/smplx_to_robot_dataset.py:97-103); the reference has no such path for galaxea_r1pro either
        raise NotImplementedError("the dataset post-processing assumes a free-joint root; use retarget_batch for a planar-base robot")
    eng = gmr._engine
    offs = np.asarray(seq_offsets, dtype=np.int64)
    N = int(qpos.shape[0])
    if offs[0] != 0 or offs[-1] != N:
        raise ValueError("seq_offsets must span [0, N]")
    fps_list = list(fps) if isinstance(fps, (list, tuple, np.ndarray)) else [fps] * (len(offs) - 1)
    root_pos = qpos[:, 0:3].clone()
    root_rot = qpos[:, [4, 5, 6, 3]].contiguous()          # wxyz -> xyzw
    dof_pos = qpos[:, 7:].contiguous()
    dof32 = dof_pos.to(torch.float32)
    zeros = torch.zeros((N, 3), dtype=torch.float32, device=qpos.device)
    ident = torch.zeros((N, 4), dtype=torch.float32, device=qpos.device)
    ident[:, 3] = 1.0
    local_body_pos, _ = eng.fk(zeros, ident, dof32, want_rot=False)
    if height_adjust and N > 0:
        lowest = eng.fk_min_height(root_pos.to(torch.float32), root_rot.to(torch.float32), dof32, offs).to(torch.float64)
        lens = torch.from_numpy(np.diff(offs)).to(qpos.device)
        root_pos[:, 2] = root_pos[:, 2] - torch.repeat_interleave(lowest, lens) + ground_offset
    if root_origin_offset and N > 0:
        nonempty = np.diff(offs) > 0
        first = torch.zeros((len(offs) - 1, 2), dtype=torch.float64, device=qpos.device)
        first[torch.from_numpy(nonempty).to(qpos.device)] = root_pos[torch.from_numpy(offs[:-1][nonempty]).to(qpos.device), :2]
        lens = torch.from_numpy(np.diff(offs)).to(qpos.device)
        root_pos[:, :2] = root_pos[:, :2] - torch.repeat_interleave(first, lens, dim=0)
    # to the host through pinned arrays, all four copies in flight together: a fresh pageable array costs more in first-touch
    # page faults than the copy itself, and torch's host allocator hands the pinned blocks back to the next batch once these
    # arrays are dropped (pickled and released)
    host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (root_pos, root_rot, dof_pos, local_body_pos)]
    for h, t in zip(host, (root_pos, root_rot, dof_pos, local_body_pos)):
        h.copy_(t, non_blocking=True)
    torch.cuda.current_stream(qpos.device).synchronize()
    rp, rr, dp, lb = (h.numpy() for h in host)
    names = list(gmr.model.body_names)
    out = []
    for s in range(len(offs) - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        # row slices of the batch arrays (C-contiguous views): no second host copy; pickling a slice stores only the slice
        out.append({"fps": fps_list[s], "root_pos": rp[a:b], "root_rot": rr[a:b], "dof_pos": dp[a:b],
                    "local_body_pos": lb[a:b], "link_body_list": names})
    return out


def retarget_clips(gmr: GeneralMotionRetargeting, pos, quat, body_names: Sequence[str], seq_offsets: Sequence[int], fps=30,
                   height_adjust: bool = True, root_origin_offset: bool = True, chunk: int = 0, burn_in: int = 0,
                   human_heights: Optional[Sequence[float]] = None, clip_start: str = "qpos0", report: bool = False,
                   track_fps: Optional[float] = None, lowpass_hz: Optional[float] = None,
                   contact_bodies: Optional[Sequence[str]] = None, contact=None, lock_feet=False, dynamics: bool = False,
                   collision=None, mirror=False, retime=None, retime_torque=None, resolve_collisions=False):
    """The whole ``process_file`` compute path for a batch of clips: batched IK, FK, post-processing.  ``human_heights``:
    one ``actual_human_height`` per clip (the per-file ``GMR(..., actual_human_height=...)`` of
    scripts/smplx_to_robot_dataset.py:79-83).  ``clip_start``: ``retarget_batch``'s (``"root_target"`` is the opt-in departure
    from the reference that spares wound-up clips their slow start).  With ``report`` a second value is returned: the
    ``engine.ClipReport`` of the solved qpos (``GeneralMotionRetargeting.clip_report``, solve counts included), host arrays.
    With ``track_fps`` a last value is added: the clips' tracking dicts at that rate (``tracking_from_qpos`` on the same qpos).
    With ``lowpass_hz`` the solved qpos is smoothed once (``smooth_qpos`` at ``fps``), and the motions, the report and the tracks
    are all made from the smoothed qpos.  ``contact_bodies`` / ``contact`` (with ``track_fps``): ``tracking_from_qpos``'s contact
    labels on the tracking dicts; ``lock_feet``: ``tracking_from_qpos``'s foot locking of those bodies (the tracking dicts only: the
    motions and the report are made from the qpos as solved).  With ``dynamics`` the ``dynamics_report`` of the same qpos follows
    the clip report (or the motions, without ``report``) and precedes the tracks.  With ``collision`` (``True``, or a dict of
    ``self_collision_report``'s keywords: ``radius``, ``capsules``, ``pairs``, ``margin``) the ``self_collision_report`` of the same
    qpos follows the dynamics report (or what precedes it) and precedes the tracks.  With ``mirror`` (``True``, or a dict of
    ``augment_mirror``'s keywords ``about`` and ``plan``) the motions and the tracks are made from ``augment_mirror`` of the (smoothed)
    qpos: twice the clips, clip ``S + i`` the mirror image of clip ``i``; the reports stay those of the ``S`` solved clips (a
    mirrored clip has no human targets to be compared with).  A robot that is not symmetric raises ``SymmetryError`` before the solve.
    With ``retime`` (``True``, one rate in rad/s, or ``{joint: rad/s}``: ``retime_to_limits``' ``velocity_limits``, ``True`` standing for
    ``None``) the (smoothed) qpos is retimed to those limits before anything but the clip report is made from it: the motions, the
    dynamics and self-collision reports, the mirror images and the tracks are those of the retimed clips, which are longer where a
    hinge was too fast; the clip report stays that of the solved clips (a retimed frame has no human targets to be compared with).
    With ``retime_torque`` (``True``, or ``retime_to_torque_limits``' ``limit_scale``) the (smoothed, velocity-retimed) qpos is then
    retimed to the robot's torque limits, in the same place.  Torques are second differences of qpos and those of unfiltered IK
    output are noise (``dynamics_from_qpos``): give ``lowpass_hz`` with it.  With ``resolve_collisions`` (``True``, or a dict of
    ``resolve_self_collisions``' keywords) the (smoothed, retimed) qpos then goes through ``resolve_self_collisions``, before the
    mirror images, the motions, the dynamics and self-collision reports, the foot locking and the tracks are made from it; the clip
    report stays that of the solved clips."""
    mirror_kw = dict(mirror) if isinstance(mirror, dict) else {}
    if mirror and mirror_kw.get("plan") is None:
        gmr.symmetry_plan()  # (SymmetryError here, before any solve)
    if contact_bodies is not None and track_fps is None:
        raise ValueError("contact_bodies needs track_fps: the labels are made on the tracking export")
    if lock_feet and contact_bodies is None:
        raise ValueError("lock_feet needs contact_bodies: the bodies to lock")
    tpos = torch.from_numpy(np.ascontiguousarray(pos)) if isinstance(pos, np.ndarray) else pos
    tquat = torch.from_numpy(np.ascontiguousarray(quat)) if isinstance(quat, np.ndarray) else quat
    tpos, tquat = tpos.to(gmr.device), tquat.to(gmr.device)
    if not report:
        qpos = gmr.retarget_batch(tpos, tquat, body_names, seq_offsets=seq_offsets, chunk=chunk, burn_in=burn_in,
                                  human_heights=human_heights, clip_start=clip_start)  # (raises on non-finite qpos / a capped QP)
        if lowpass_hz:
            qpos = smooth_qpos(gmr, qpos, seq_offsets, fps, lowpass_hz)
        rep = None
    else:
        qpos, iters = gmr.retarget_batch(tpos, tquat, body_names, seq_offsets=seq_offsets, chunk=chunk, burn_in=burn_in,
                                         human_heights=human_heights, clip_start=clip_start, return_iters=True)
        if lowpass_hz:
            qpos = smooth_qpos(gmr, qpos, seq_offsets, fps, lowpass_hz)
        rep = gmr.clip_report(qpos, tpos, tquat, body_names, seq_offsets, human_heights=human_heights, iters=iters)
    if retime is not None and retime is not False:
        qpos, seq_offsets, _ = retime_to_limits(gmr, qpos, seq_offsets, fps, None if retime is True else retime)
    if retime_torque is not None and retime_torque is not False:
        scale = {} if retime_torque is True else {"limit_scale": float(retime_torque)}
        qpos, seq_offsets, _ = retime_to_torque_limits(gmr, qpos, seq_offsets, fps, **scale)
    if resolve_collisions:
        qpos, _ = resolve_self_collisions(gmr, qpos, seq_offsets, **(resolve_collisions if isinstance(resolve_collisions, dict) else {}))
    q_all, offs_all, fps_all = augment_mirror(gmr, qpos, seq_offsets, fps, **mirror_kw) if mirror else (qpos, seq_offsets, fps)
    res = (motions_from_qpos(gmr, q_all, offs_all, fps_all, height_adjust=height_adjust, root_origin_offset=root_origin_offset),)
    if rep is not None:
        res += (rep.numpy(),)
    if dynamics:
        res += (dynamics_report(gmr, qpos, seq_offsets, fps),)
    if collision:
        res += (self_collision_report(gmr, qpos, seq_offsets, **(collision if isinstance(collision, dict) else {})),)
    if track_fps is not None:
        lock_kw = {"lock_feet": lock_feet} if lock_feet else {}  # (absent without the flag: nothing changes then)
        res += (tracking_from_qpos(gmr, q_all, offs_all, fps_all, track_fps, contact_bodies=contact_bodies, contact=contact, **lock_kw),)
    return res[0] if len(res) == 1 else res


# ------------------------------------------------------------------ the tracking export
TRACK_ARRAYS = ("joint_pos", "joint_vel", "root_pos", "root_rot", "root_lin_vel", "root_ang_vel",
                "body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")


CONTACT_STATS = ("frames", "touchdowns", "slide_sum", "slide_step_max", "depth_max", "base")  # the keys of a clip's contact_stats


class ContactParams:
    """The parameters of the contact labels of ``tracking_from_qpos`` (``Engine.motion_contacts``): a body is in contact from a
    frame at or below ``height_on`` (m above the ground) and ``speed_on`` (m/s) until one above ``height_off`` or ``speed_off``.
    ``ground``: ``"clip_min"`` (every clip is measured against the lowest contact-body height it reaches) or the ground height;
    ``height_offset``: one height per contact body of its origin above its own sole (``None``: zeros).  The default thresholds
    -- enter at 0.03 m and 0.3 m/s, leave at 0.05 m and 0.6 m/s -- are conventions from common practice, not measured on any
    robot here."""

    def __init__(self, height_on: Optional[float] = None, height_off: Optional[float] = None, speed_on: Optional[float] = None,
                 speed_off: Optional[float] = None, ground="clip_min", height_offset=None):
        from .engine import CONTACT_DEFAULTS as d   # (None: the engine's default)
        given = {"height_on": height_on, "height_off": height_off, "speed_on": speed_on, "speed_off": speed_off}
        self.height_on, self.height_off, self.speed_on, self.speed_off = (float(d[k] if v is None else v) for k, v in given.items())
        self.ground, self.height_offset = ground, height_offset

    def kwargs(self) -> Dict:
        return {"height_on": self.height_on, "height_off": self.height_off, "speed_on": self.speed_on, "speed_off": self.speed_off,
                "ground": self.ground, "height_offset": self.height_offset}


def contact_body_ids(model_body_names, contact_bodies: Sequence[str]) -> List[int]:
    """The body indices of a list of body names; an unknown name raises ``KeyError`` listing the model's names."""
    names = list(model_body_names)
    missing = [b for b in contact_bodies if b not in names]
    if missing:
        raise KeyError(f"unknown contact bodies {missing}; the model's bodies are {names}")
    return [names.index(b) for b in contact_bodies]


def _track_contacts(eng, track, model_body_names, contact_bodies, contact: Optional[ContactParams]):
    """One contacts launch on a ``MotionTrack``: (``engine.MotionContacts``, the names)."""
    ids = contact_body_ids(model_body_names, contact_bodies)
    prm = contact if contact is not None else ContactParams()
    return eng.motion_contacts(track, track.out_offsets, ids, **prm.kwargs()), list(contact_bodies)


FOOTLOCK_STATS = ("runs", "locked_frames", "shift_max", "residual_max", "limit_frames")  # the keys of a clip's footlock_stats


def lock_feet(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, contact_bodies: Sequence[str],
              contact: Optional[ContactParams] = None, **footlock_kwargs):
    """qpos ``[N, nq]`` float64 on the GPU (concatenated clips at ``fps``: one rate or one per clip) with the foot slide of the
    planted ``contact_bodies`` removed (``Engine.motion_footlock``; the definition is the contract above ``gmr_footlock_input`` in
    include/gmr_amd.h) -> ``(qpos_locked, stats)``: the cleaned qpos ``[N, nq]`` on the device and ``stats``, the device tensors
    ``runs``, ``locked_frames``, ``limit_frames`` (int32 ``[S, C]``), ``shift_max`` and ``residual_max`` (float64 ``[S, C]``,
    metres).  The labels are the tracking export's own: ``Engine.motion_track`` at ``fps_out = fps`` (every output frame is one
    qpos row), then ``Engine.motion_contacts`` with ``contact`` (a :class:`ContactParams`); with per-clip rates that is one pass
    per distinct rate.  ``footlock_kwargs``: ``blend_frames``, ``min_run``, ``iterations``, ``damping``, ``step_cap`` of
    ``Engine.motion_footlock``; its defaults are conventions, not measured on any robot.  Only the hinges between a contact body
    and the first joint it shares with another one move; everything else is copied bit for bit."""
    if gmr.model.planar_base:
        raise NotImplementedError("foot locking assumes a free-joint root; a planar-base robot is not supported")
    return _lock_feet(gmr._engine, gmr.model.body_names, qpos, seq_offsets, fps, contact_bodies, contact, footlock_kwargs)


def _lock_feet(eng, model_body_names, qpos, seq_offsets, fps, contact_bodies, contact, footlock_kwargs):
    """``lock_feet`` on an ``Engine`` (a free-joint model)."""
    ids = contact_body_ids(model_body_names, contact_bodies)
    prm = contact if contact is not None else ContactParams()
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    S, Cn = offs.size - 1, len(ids)
    f = np.asarray(fps.detach().cpu().numpy() if isinstance(fps, torch.Tensor) else fps, dtype=np.float64)
    f = np.full(S, float(f)) if f.ndim == 0 else f
    if f.shape != (S,):
        raise ValueError("fps must be one rate or one rate per clip")
    lens = np.diff(offs)
    res = qpos.clone()
    stats = {k: torch.zeros((S, Cn), dtype=torch.int32 if k in ("runs", "locked_frames", "limit_frames") else torch.float64,
                            device=qpos.device) for k in FOOTLOCK_STATS}
    for rate in np.unique(f[lens > 0]):
        sel = np.flatnonzero((f == rate) & (lens > 0))
        whole = sel.size == np.count_nonzero(lens > 0)  # one rate: the batch as it is
        if whole:
            rows, q, o = None, qpos.contiguous(), offs
        else:
            rows = torch.from_numpy(np.concatenate([np.arange(offs[s], offs[s + 1]) for s in sel])).to(qpos.device)
            q, o = qpos.index_select(0, rows), np.concatenate([[0], np.cumsum(lens[sel])]).astype(np.int64)
        track = eng.motion_track(q, o, float(rate), float(rate))
        assert np.array_equal(track.out_offsets, o)   # fps_out = fps: one output frame per row
        labels = eng.motion_contacts(track, track.out_offsets, ids, out={"contact": torch.zeros((int(q.shape[0]), Cn), dtype=torch.uint8,
                                                                                                 device=q.device)}, **prm.kwargs())
        got = eng.motion_footlock(q, o, labels["contact"], ids, **footlock_kwargs)
        if whole:
            res = got["qpos"]
            stats = {k: got[k] for k in FOOTLOCK_STATS}
        else:
            res.index_copy_(0, rows, got["qpos"])
            clips = torch.from_numpy(sel).to(qpos.device)
            for k in FOOTLOCK_STATS:
                stats[k].index_copy_(0, clips, got[k])
    return res, stats


def tracks_to_host(tracks, fps_out, body_names, joint_names, contacts=None, locks=None) -> List[List[Dict]]:
    """Several ``engine.MotionTrack`` results (one per robot) to the host with every copy in flight before the one
    synchronisation; per result the list of per-clip dicts of ``tracking_from_qpos``.  ``contacts``: per result ``None`` or
    (``engine.MotionContacts``, contact body names) -- its copies ride in the same synchronisation and every clip's dict also
    gets ``contact``, ``contact_body_names``, ``contact_stats`` and ``airborne_frames``.  ``locks``: per result ``None`` or the
    ``stats`` of ``lock_feet``; every clip's dict then also gets ``footlock_stats``."""
    hosts, chosts = [], []
    dev = None
    contacts = [None] * len(tracks) if contacts is None else list(contacts)
    locks = [None] * len(tracks) if locks is None else list(locks)
    lhosts = []
    for lk in locks:
        if lk is None:
            lhosts.append(None)
            continue
        lhost = {k: torch.empty(lk[k].shape, dtype=lk[k].dtype, pin_memory=True) for k in FOOTLOCK_STATS}
        for k, h in lhost.items():
            h.copy_(lk[k], non_blocking=True)
        lhosts.append({k: h.numpy() for k, h in lhost.items()})
    for tr, ct in zip(tracks, contacts):
        host = {k: torch.empty(tr[k].shape, dtype=tr[k].dtype, pin_memory=True) for k in TRACK_ARRAYS}
        for k, h in host.items():
            h.copy_(tr[k], non_blocking=True)
            dev = tr[k].device
        hosts.append({k: h.numpy() for k, h in host.items()})
        if ct is None:
            chosts.append(None)
            continue
        chost = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in ct[0].items()}
        for k, h in chost.items():
            h.copy_(ct[0][k], non_blocking=True)
        chosts.append({k: h.numpy() for k, h in chost.items()})
    if dev is not None:
        torch.cuda.current_stream(dev).synchronize()
    out = []
    for tr, host, bn, jn, ct, chost, lhost in zip(tracks, hosts, body_names, joint_names, contacts, chosts, lhosts):
        offs, bn, jn = tr.out_offsets, list(bn), list(jn)
        clips = []
        for s in range(len(offs) - 1):
            a, b = int(offs[s]), int(offs[s + 1])
            d = {"fps": fps_out}
            d.update((k, host[k][a:b]) for k in TRACK_ARRAYS)
            d.update(body_names=bn, joint_names=jn, quat_order="xyzw")
            if ct is not None:
                stats = {k: chost[k][s] for k in CONTACT_STATS}
                d.update(contact=chost["contact"][a:b], contact_body_names=list(ct[1]), contact_stats=stats,
                         airborne_frames=int(chost["airborne_frames"][s]))
            if lhost is not None:
                d["footlock_stats"] = {k: lhost[k][s] for k in FOOTLOCK_STATS}
            clips.append(d)
        out.append(clips)
    return out


def tracking_from_qpos(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, fps_out,
                       lowpass_hz: Optional[float] = None, contact_bodies: Optional[Sequence[str]] = None,
                       contact: Optional[ContactParams] = None, lock_feet=False) -> List[Dict]:
    """qpos ``[N, nq]`` float64 on the GPU (concatenated clips at ``fps``: one rate or one per clip) -> one tracking dict per clip
    at ``fps_out`` (``Engine.motion_track``, one launch): ``fps``, ``joint_pos``, ``joint_vel``, ``root_pos``, ``root_rot`` (xyzw),
    ``root_lin_vel``, ``root_ang_vel`` (world frame) in float64, ``body_pos_w``, ``body_quat_w`` (xyzw), ``body_lin_vel_w``,
    ``body_ang_vel_w`` in float32, ``body_names``, ``joint_names`` (the hinges in qpos order) and ``quat_order = "xyzw"``.
    The arrays are row slices of batch-sized page-locked host arrays, as ``motions_from_qpos`` hands them out.  ``lowpass_hz``:
    the cutoff of the zero-phase low-pass applied to qpos first, in the same call (``None``: off).
    ``contact_bodies``: body names (the feet) whose contact with the ground is labelled on the export, one more kernel
    (``Engine.motion_contacts``); every clip's dict then also holds ``contact`` (uint8 ``[M_s, C]``, 1 = on the ground),
    ``contact_body_names``, ``contact_stats`` -- ``frames``, ``touchdowns`` (int32 ``[C]``), ``slide_sum``, ``slide_step_max``,
    ``depth_max`` (float64 ``[C]``, metres: how far a planted body slides in all and in one frame, how deep it goes below the
    ground) and ``base`` (float64: the ground height the clip was measured against) -- and ``airborne_frames`` (frames with no
    body in contact).  ``contact``: a :class:`ContactParams` (thresholds, ground, height offsets); the defaults are conventions
    from common practice, not measured on any robot.  An unknown body name raises ``KeyError`` listing the model's names.
    ``lock_feet`` (only with ``contact_bodies``): the foot slide of the contact bodies is removed from qpos (:func:`lock_feet`, behind
    the low-pass) before the export, and every clip's dict also holds ``footlock_stats`` -- ``runs``, ``locked_frames``,
    ``limit_frames`` (int32 ``[C]``), ``shift_max``, ``residual_max`` (float64 ``[C]``, metres); ``True`` or a dict of
    ``Engine.motion_footlock``'s parameters."""
    if gmr.model.planar_base:
        raise NotImplementedError("the tracking export assumes a free-joint root; use retarget_batch for a planar-base robot")
    from .engine import _report_names
    if lock_feet and contact_bodies is None:
        raise ValueError("lock_feet needs contact_bodies: the bodies to lock")
    if contact_bodies is not None:
        contact_body_ids(gmr.model.body_names, contact_bodies)  # (an unknown name: before any launch)
    locks = None
    if lock_feet:
        qpos, stats, lowpass_hz = _smooth_and_lock(gmr._engine, gmr.model.body_names, qpos, seq_offsets, fps, lowpass_hz, contact_bodies,
                                                   contact, lock_feet)
        locks = [stats]
    track = gmr._engine.motion_track(qpos, seq_offsets, fps, fps_out, lowpass_hz=0.0 if lowpass_hz is None else lowpass_hz)
    contacts = None if contact_bodies is None else [_track_contacts(gmr._engine, track, gmr.model.body_names, contact_bodies, contact)]
    return tracks_to_host([track], fps_out, [gmr.model.body_names], [_report_names(gmr._cm)[1]], contacts=contacts, locks=locks)[0]


def _smooth_and_lock(eng, model_body_names, qpos, seq_offsets, fps, lowpass_hz, contact_bodies, contact, lock_feet):
    """The front of ``tracking_from_qpos(lock_feet=...)`` on an ``Engine``: the low-pass, then the foot locking.  Returns (qpos,
    stats, the low-pass left for the export: none)."""
    if lowpass_hz:
        qpos = _smooth_qpos(eng, qpos, seq_offsets, fps, lowpass_hz)
    kw = dict(lock_feet) if isinstance(lock_feet, dict) else {}
    qpos, stats = _lock_feet(eng, model_body_names, qpos, seq_offsets, fps, contact_bodies, contact, kw)
    return qpos, stats, None


def smooth_qpos(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, lowpass_hz) -> torch.Tensor:
    """qpos ``[N, nq]`` float64 on the GPU (concatenated clips at ``fps``: one rate or one per clip) through the zero-phase
    2nd-order Butterworth low-pass of the tracking export (the contract above ``gmr_track_input`` in include/gmr_amd.h) ->
    the filtered qpos ``[N, nq]`` float64 on the device, root quaternion wxyz, sign-continuous and of unit norm.  It runs the
    export at ``fps_out = fps`` without body outputs, where every output frame is a copy of one filtered row; with per-clip
    rates that is one call per distinct rate.  ``lowpass_hz`` ``None`` or 0: a copy.  No clamp to the joint ranges: the clip
    report of the result shows any overshoot."""
    if gmr.model.planar_base:
        raise NotImplementedError("the low-pass assumes a free-joint root; a planar-base robot is not supported")
    return _smooth_qpos(gmr._engine, qpos, seq_offsets, fps, lowpass_hz)


def _smooth_qpos(eng, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, lowpass_hz) -> torch.Tensor:
    """``smooth_qpos`` on an ``Engine`` (a free-joint model)."""
    from .schedule import lowpass_check
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    S = offs.size - 1
    f = np.asarray(fps.detach().cpu().numpy() if isinstance(fps, torch.Tensor) else fps, dtype=np.float64)
    f = np.full(S, float(f)) if f.ndim == 0 else f
    if f.shape != (S,):
        raise ValueError("fps must be one rate or one rate per clip")
    if lowpass_check(offs, f, 1.0, lowpass_hz, ratio=f) == 0.0:  # (ratio 1 in the calls below: fs is the clip's own rate)
        return qpos.clone()
    lens = np.diff(offs)
    res = torch.empty_like(qpos)
    fields = ("root_pos", "root_rot", "joint_pos")
    for rate in np.unique(f[lens > 0]):
        sel = np.flatnonzero((f == rate) & (lens > 0))
        if sel.size == np.count_nonzero(lens > 0):  # one rate: the batch as it is
            rows, q, o = None, qpos, offs
        else:
            rows = torch.from_numpy(np.concatenate([np.arange(offs[s], offs[s + 1]) for s in sel])).to(qpos.device)
            q, o = qpos.index_select(0, rows), np.concatenate([[0], np.cumsum(lens[sel])]).astype(np.int64)
        n = int(q.shape[0])
        out = {"root_pos": torch.empty((n, 3), dtype=torch.float64, device=q.device),
               "root_rot": torch.empty((n, 4), dtype=torch.float64, device=q.device),
               "joint_pos": torch.empty((n, eng.nq - 7), dtype=torch.float64, device=q.device)}
        tr = eng.motion_track(q, o, float(rate), float(rate), out=out, bodies=False, lowpass_hz=lowpass_hz)
        assert int(tr.out_offsets[-1]) == n
        sm = torch.cat([tr["root_pos"], tr["root_rot"][:, [3, 0, 1, 2]], tr["joint_pos"]], dim=1)
        if rows is None:
            res = sm
        else:
            res.index_copy_(0, rows, sm)
    return res


# ------------------------------------------------------------------ inverse dynamics
DYNAMICS_CSV_FIELDS = ("frames_any_over_limit", "fz_ratio_max", "fz_ratio_min", "unloaded_frames", "nonfinite_frames")


def dynamics_from_qpos(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, lowpass_hz: float = 0.0,
                       table=None, **dynamics_kwargs) -> List[Dict]:
    """Inverse dynamics of qpos ``[N, nq]`` float64 on the GPU (concatenated clips at the one rate ``fps``) -> one dict of host
    arrays per clip: ``tau`` ``[T, nh]``, ``root_wrench`` ``[T, 6]``, ``com`` ``[T, 3]``, ``zmp`` ``[T, 2]``, ``qvel`` / ``qacc``
    ``[T, nv]``, the clip's row of every statistic of ``Engine.motion_dynamics``, and ``joint_names``, ``torque_limit``, ``fps``
    (the definition is the contract above ``gmr_dynamics_input`` in include/gmr_amd.h).  Velocities and accelerations are central
    and second differences of qpos.  Second differences of unfiltered IK output are noisy -- the torques of a raw clip are
    dominated by frame-to-frame jitter of the solve -- so ``lowpass_hz > 0`` routes qpos through ``smooth_qpos`` first; the default
    0 leaves qpos as it is and the choice to the caller.  ``dynamics_kwargs``: ``gravity``, ``ground_z``, ``fz_min`` (a
    convention, not measured on any robot)."""
    if gmr.model.planar_base:
        raise NotImplementedError("inverse dynamics assumes a free-joint root; a planar-base robot is not supported")
    eng = gmr._engine
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if lowpass_hz:
        qpos = _smooth_qpos(eng, qpos, offs, fps, lowpass_hz)
    got = eng.motion_dynamics(qpos, offs, float(fps), table=table, **dynamics_kwargs)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    names = [gmr.model.jnt_names[b] for b in gmr.model.hinge_bodies()]
    limit = eng.inertial_device(table)["torque_limit"].cpu().numpy()
    out = []
    for s in range(offs.size - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        d = {k: host[k][a:b] for k in ("tau", "root_wrench", "com", "zmp", "qvel", "qacc")}
        d.update((k, host[k][s]) for k in got.stats)
        d.update(joint_names=names, torque_limit=limit, fps=float(fps))
        out.append(d)
    return out


def dynamics_report(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, lowpass_hz: float = 0.0,
                    table=None, **dynamics_kwargs) -> Dict:
    """The per-clip statistics of ``dynamics_from_qpos`` alone, as host arrays with one row per clip, plus ``joint_names`` and
    ``torque_limit``: ``tau_abs_max``, ``tau_rms``, ``tau_ratio_max``, ``frames_over_limit`` ``[S, nh]``; ``frames_any_over_limit``,
    ``fz_ratio_max``, ``fz_ratio_min``, ``unloaded_frames``, ``nonfinite_frames`` ``[S]``."""
    if gmr.model.planar_base:
        raise NotImplementedError("inverse dynamics assumes a free-joint root; a planar-base robot is not supported")
    return _dynamics_report(gmr._engine, qpos, seq_offsets, fps, lowpass_hz, table, dynamics_kwargs)


def _dynamics_report(eng, qpos, seq_offsets, fps, lowpass_hz=0.0, table=None, dynamics_kwargs=None) -> Dict:
    """``dynamics_report`` on an ``Engine`` (a free-joint model)."""
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if lowpass_hz:
        qpos = _smooth_qpos(eng, qpos, offs, fps, lowpass_hz)
    got = eng.motion_dynamics(qpos, offs, float(fps), table=table, **(dynamics_kwargs or {}))
    rep = {k: v.cpu().numpy() for k, v in got.stats.items()}
    model = eng.cm.robot
    rep["joint_names"] = [model.jnt_names[b] for b in model.hinge_bodies()]
    rep["torque_limit"] = eng.inertial_device(table)["torque_limit"].cpu().numpy()
    return rep


def write_dynamics_csv(path: str, names: Sequence[str], report: Dict, append: bool = False) -> None:
    """One row per clip of a ``dynamics_report``: the per-clip fields, then the worst joint -- the hinge with the largest
    ``tau_ratio_max``, or with the largest ``tau_abs_max`` where no hinge has a limit -- its name, its ratio and its peak torque."""
    import csv
    ratio, peak = np.asarray(report["tau_ratio_max"]), np.asarray(report["tau_abs_max"])
    if len(names) != ratio.shape[0]:
        raise ValueError("one name per clip is required")
    with open(path, "a" if append else "w", newline="") as f:
        w = csv.writer(f)
        if not append:
            w.writerow(("clip",) + DYNAMICS_CSV_FIELDS + ("worst_joint", "worst_ratio", "worst_tau_abs_max"))
        for s, n in enumerate(names):
            j = int(np.argmax(ratio[s])) if ratio.shape[1] and ratio[s].max() > 0.0 else (int(np.argmax(peak[s])) if peak.shape[1] else -1)
            w.writerow([n] + [repr(report[k][s].item()) for k in DYNAMICS_CSV_FIELDS]
                       + ([report["joint_names"][j], repr(float(ratio[s, j])), repr(float(peak[s, j]))] if j >= 0 else ["", "0.0", "0.0"]))


def dynamics_hard_mask(report: Dict, max_torque_ratio: float) -> np.ndarray:
    """Clips in which some hinge needs more than ``max_torque_ratio`` times its torque limit."""
    r = np.asarray(report["tau_ratio_max"])
    return (r.max(axis=1) > float(max_torque_ratio)) if r.shape[1] else np.zeros(r.shape[0], dtype=bool)


# ------------------------------------------------------------------ self-collision
COLLISION_CSV_FIELDS = ("clearance_min", "penetration_max", "worst_frame", "colliding_frames", "longest_run", "hits_sum", "nonfinite_frames")


def self_collision_from_qpos(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], capsules=None, pairs=None,
                             margin: float = 0.0, radius: float = 0.03) -> List[Dict]:
    """Capsule clearance of qpos ``[N, nq]`` float64 on the GPU (concatenated clips) -> one dict of host arrays per clip:
    ``clearance`` ``[T]`` (metres, negative = penetration), ``pair`` ``[T]`` (row of the pair table), ``hits`` ``[T]``, the clip's
    row of every statistic of ``Engine.motion_self_collision``, and ``pair_names`` (the two capsule names of every pair of the
    table).  The definition is the contract above ``gmr_self_collision_input`` in include/gmr_amd.h.  ``capsules`` / ``pairs``:
    ``gmr_amd.collision`` tables; ``None``: the skeleton's capsules of ``radius`` along the links and their default pairs -- the
    radius is a convention, not measured on any robot, and the skeleton is not the robot's collision geometry."""
    from .collision import pair_names
    eng = gmr._engine
    capsules, pairs = eng.resolve_proxies(capsules, pairs, radius)
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    got = eng.motion_self_collision(qpos, offs, capsules, pairs, margin=margin)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    names = pair_names(capsules, pairs)
    out = []
    for s in range(offs.size - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        d = {k: host[k][a:b] for k in ("clearance", "pair", "hits")}
        d.update((k, host[k][s]) for k in got.stats)
        d["pair_names"] = names
        out.append(d)
    return out


def self_collision_report(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], capsules=None, pairs=None,
                          margin: float = 0.0, radius: float = 0.03) -> Dict:
    """The per-clip statistics of ``self_collision_from_qpos`` alone, as host arrays with one row per clip: ``clearance_min``,
    ``worst_frame``, ``worst_pair``, ``colliding_frames``, ``longest_run``, ``hits_sum``, ``nonfinite_frames``; plus
    ``worst_pair_names`` (the two capsule names of ``worst_pair``, ``("", "")`` where there is none) and ``penetration_max =
    max(0, -clearance_min)``."""
    return _self_collision_report(gmr._engine, qpos, seq_offsets, capsules, pairs, margin, radius)


def _self_collision_report(eng, qpos, seq_offsets, capsules=None, pairs=None, margin=0.0, radius=0.03) -> Dict:
    """``self_collision_report`` on an ``Engine``."""
    capsules, pairs = eng.resolve_proxies(capsules, pairs, radius)
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    got = eng.motion_self_collision(qpos, offs, capsules, pairs, margin=margin)
    rep = {k: v.cpu().numpy() for k, v in got.stats.items()}
    rep["worst_pair_names"] = [(capsules.names[int(pairs.pairs[p, 0])], capsules.names[int(pairs.pairs[p, 1])]) if p >= 0 else ("", "")
                               for p in rep["worst_pair"]]
    rep["penetration_max"] = np.maximum(0.0, -rep["clearance_min"])
    return rep


def resolve_self_collisions(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], radius: float = 0.03,
                            capsules=None, pairs=None, margin: float = 0.0, freeze_joints: Sequence[str] = (),
                            freeze_bodies: Sequence[str] = (), **repair_kwargs):
    """Push the colliding capsule pairs of qpos ``[N, nq]`` float64 on the GPU (concatenated clips) apart
    (``Engine.motion_self_collision_repair``; the definition is the contract above ``gmr_self_collision_repair_input`` in
    include/gmr_amd.h) -> ``(qpos_out, info)``: the repaired rows, a device tensor, and host arrays with one row per clip --
    ``repaired_frames``, ``unresolved_frames``, ``move_max`` (rad), ``clearance_min_after`` (m), ``nonfinite_frames`` -- plus
    ``clearance_before`` / ``clearance_after`` / ``move`` ``[N]``.  ``capsules`` / ``pairs``: ``gmr_amd.collision`` tables; ``None``: the
    skeleton's capsules of ``radius`` and ``default_pairs(robot, capsules, rest_margin=margin)``, so that a pair which rests
    below the margin, and which no hinge changes, does not stay unresolved forever.  ``freeze_joints`` / ``freeze_bodies``:
    ``gmr_amd.collision.movable_mask`` -- freezing the ankle links keeps a locked foot where ``lock_feet`` put it.
    ``repair_kwargs``: ``iterations``, ``damping``, ``step_cap``, ``resolve_tol``; their defaults (16 passes, 1e-6 m^2, 0.2 rad,
    1e-4 m) and the radius are conventions, not measured on a robot.  The velocity of the result has a kink where a pair enters
    the margin: ``smooth_qpos`` afterwards is the user's tool."""
    return _resolve_self_collisions(gmr._engine, qpos, seq_offsets, radius, capsules, pairs, margin, freeze_joints, freeze_bodies,
                                    repair_kwargs)


def _resolve_self_collisions(eng, qpos, seq_offsets, radius=0.03, capsules=None, pairs=None, margin=0.0, freeze_joints=(),
                             freeze_bodies=(), repair_kwargs=None):
    """``resolve_self_collisions`` on an ``Engine``."""
    from . import collision
    if capsules is None:
        capsules, default = eng.default_proxies(radius)
        if pairs is None and float(margin) == 0.0:
            pairs = default
    if pairs is None:
        if float(margin) == 0.0:
            pairs = eng.resolve_proxies(capsules, None)[1]
        else:   # (built once per capsule table and margin, as the engine's own defaults are)
            key = ("pairs", id(capsules), float(margin))
            if key not in eng._collision_default:
                import weakref
                eng._collision_default[key] = collision.default_pairs(eng.cm.robot, capsules, rest_margin=float(margin))[0]
                weakref.finalize(capsules, eng._collision_default.pop, key, None)
            pairs = eng._collision_default[key]
    mask = collision.movable_mask(eng.cm.robot, freeze_joints, freeze_bodies)
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    got = eng.motion_self_collision_repair(qpos, offs, capsules, pairs, margin=margin, movable=mask, **(repair_kwargs or {}))
    info = {k: v.cpu().numpy() for k, v in got.items() if k != "qpos"}
    return got["qpos"], info


def write_collision_csv(path: str, names: Sequence[str], report: Dict, append: bool = False) -> None:
    """One row per clip of a ``self_collision_report``: the per-clip fields, then the two capsule names of the worst pair."""
    import csv
    if len(names) != len(report["clearance_min"]):
        raise ValueError("one name per clip is required")
    with open(path, "a" if append else "w", newline="") as f:
        w = csv.writer(f)
        if not append:
            w.writerow(("clip",) + COLLISION_CSV_FIELDS + ("worst_capsule_a", "worst_capsule_b"))
        for s, n in enumerate(names):
            w.writerow([n] + [repr(report[k][s].item()) for k in COLLISION_CSV_FIELDS] + list(report["worst_pair_names"][s]))


def collision_hard_mask(report: Dict, max_penetration: float) -> np.ndarray:
    """Clips whose deepest penetration exceeds ``max_penetration`` metres."""
    return np.asarray(report["penetration_max"]) > float(max_penetration)


# ------------------------------------------------------------------ mirror augmentation
def mirror_qpos(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], about: str = "world", plan=None) -> torch.Tensor:
    """The left-right mirrored copy of qpos ``[N, nq]`` float64 on the GPU (concatenated clips), one kernel
    (``Engine.motion_mirror``; the definition is the contract above ``gmr_mirror_input`` in include/gmr_amd.h).  ``about="world"``:
    the reflection in the world plane y = 0; ``"start"``: per clip in the vertical plane through its first root position along its
    heading.  ``plan``: a ``gmr_amd.symmetry.SymmetryPlan``; ``None``: the robot's own at the default tolerances, which raises
    ``SymmetryError`` for a robot that is not symmetric (pass looser tolerances to ``gmr.symmetry_plan`` or a plan of your own).
    No clamp to the joint ranges: a symmetric robot's ranges mirror onto each other."""
    if gmr.model.planar_base:
        raise NotImplementedError("mirroring assumes a free-joint root; a planar-base robot is not supported")
    return gmr._engine.motion_mirror(qpos, np.ascontiguousarray(seq_offsets, dtype=np.int64), plan=plan, about=about)


def augment_mirror(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, about: str = "start", plan=None):
    """A batch of clips and its mirror images: ``(qpos2 [2N, nq], seq_offsets2 [2S + 1], fps2)``, the originals first, then the
    mirrors in the same order, so clip ``S + i`` is the mirror of clip ``i``.  ``fps``: one rate (returned as it is) or one per clip
    (returned twice over).  The result feeds ``tracking_from_qpos``, ``lock_feet``, ``dynamics_report`` and ``MotionLibrary``
    unchanged; body names that go with a mirrored clip (``contact_bodies``) are ``plan.mirror_names(names)``."""
    return _augment_mirror(gmr._engine, qpos, seq_offsets, fps, about, plan, planar=gmr.model.planar_base)


def _augment_mirror(eng, qpos, seq_offsets, fps, about="start", plan=None, planar=False):
    """``augment_mirror`` on an ``Engine``."""
    if planar:
        raise NotImplementedError("mirroring assumes a free-joint root; a planar-base robot is not supported")
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1 or offs[0] != 0 or offs[-1] != qpos.shape[0] or np.any(np.diff(offs) < 0):
        raise ValueError("seq_offsets must span [0, N] without going back")
    N = int(qpos.shape[0])
    both = torch.empty((2 * N, int(qpos.shape[1])), dtype=qpos.dtype, device=qpos.device)
    both[:N].copy_(qpos)
    eng.motion_mirror(qpos, offs, plan=plan, about=about, out=both[N:])
    if isinstance(fps, torch.Tensor):
        f2 = torch.cat([fps, fps]) if fps.dim() else fps
    elif np.ndim(fps) == 0:
        f2 = fps
    else:  # (a list stays a list of the same objects: what motions_from_qpos writes into the clips' dicts)
        f2 = np.concatenate([fps, fps]) if isinstance(fps, np.ndarray) else list(fps) * 2
    return both, np.concatenate([offs, offs[1:] + N]).astype(np.int64), f2


# ------------------------------------------------------------------ composed clips
def compose_clips(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], sequences, blend=8):
    """Long reference motions from segments of the clips, on the GPU (``Engine.motion_compose``; the definition is the contract
    above ``gmr_compose_input`` in include/gmr_amd.h): ``sequences`` is a list of output clips, each a list of
    ``gmr_amd.compose.Segment(clip, begin, length)``; every segment but the first of its output clip is turned and shifted in the
    plane onto the end of the one before it and cross-faded into it over ``blend`` frames (one int, or one per transition).
    Returns ``(qpos_out, seq_offsets_out, seg_transform)``: ordinary qpos and offsets for ``lock_feet`` (which removes the slide a
    cross-fade puts into planted feet), ``tracking_from_qpos``, ``dynamics_report`` and ``MotionLibrary``, and every segment's
    placement ``(c, s, tx, ty, hw, hz)``.  A plan that breaks an invariant raises ``gmr_amd.compose.ComposeError``."""
    from .compose import ComposePlan
    plan = ComposePlan(seq_offsets, sequences, blend)
    qpos_out, seg_transform = gmr._engine.motion_compose(qpos, plan)
    return qpos_out, np.array(plan.out_offsets), seg_transform  # (a copy: the plan's arrays are read-only)


def repeat_clip(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], clip: int, times: int, blend=8):
    """One output clip: clip ``clip`` ``times`` times over, each pass starting where the last one ended (``compose_clips``)."""
    frames = int(seq_offsets[clip + 1]) - int(seq_offsets[clip])
    return compose_clips(gmr, qpos, seq_offsets, [[(clip, 0, frames)] * int(times)], blend)


# ------------------------------------------------------------------ retiming to velocity limits
# Conventions, not measured on a robot: four intervals on either side spread a stretch over about a tenth of a second at 30 - 60 Hz,
# and a clip that needs more than eight times its duration somewhere is better looked at than played.
RETIME_WINDOW = 4
RETIME_MAX_STRETCH = 8.0


def retime_vmax(robot, velocity_limits=None, retargeter_limits=None) -> np.ndarray:
    """``[nq - 7]`` rad/s per hinge in qpos order for ``retime_to_limits``: ``velocity_limits`` in the forms
    ``GeneralMotionRetargeting`` takes (one number, or ``{joint: rad/s}``; ``resolve_velocity_limits``); ``None``: the retargeter's own
    table ``retargeter_limits`` where it has one, else every limited hinge at ``DEFAULT_VELOCITY_LIMIT``.  A hinge the table does not
    name is ``inf``.  No device is needed."""
    from .model import resolve_velocity_limits
    if velocity_limits is not None:
        table = resolve_velocity_limits(robot, False, velocity_limits)
    elif retargeter_limits is not None:
        table = dict(retargeter_limits)
    else:
        table = resolve_velocity_limits(robot, True, None)
    bodies = sorted((int(b) for b in robot.hinge_bodies()), key=lambda b: int(robot.qpos_adr[b]))
    vmax = np.array([float(table.get(robot.jnt_names[b], np.inf)) for b in bodies], dtype=np.float64)
    if not np.all(vmax > 0.0):
        raise ValueError("every velocity limit must be > 0 (inf: no limit)")
    return vmax


def retime_to_limits(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, velocity_limits=None,
                     window: int = RETIME_WINDOW, max_stretch: float = RETIME_MAX_STRETCH, interp: str = "linear"):
    """qpos ``[N, nq]`` float64 on the GPU (concatenated clips at ``fps``: one rate or one per clip) played slower exactly where a
    hinge turns faster than its velocity limit, on the GPU (``Engine.motion_retime_plan`` / ``motion_retime_apply``; the definition
    is the contract above ``gmr_retime_plan_input`` in include/gmr_amd.h): a monotone time warp and a resampling at the clip's own
    rate.  The joint-space path is kept, unlike ``use_velocity_limit=True`` in the solve, and no clip is dropped.
    ``velocity_limits``: see ``retime_vmax`` (``None``: ``gmr.velocity_limits``, else ``DEFAULT_VELOCITY_LIMIT`` on every limited
    hinge).  ``window``: the intervals on either side over which a stretch is widened and averaged; ``max_stretch``: the largest
    local slow-down, beyond which an interval is counted as capped and still exceeds its limit (``RETIME_WINDOW`` and
    ``RETIME_MAX_STRETCH`` are conventions, not measured on a robot).  ``interp``: ``Engine.motion_retime_apply``'s -- ``"cubic"`` gives
    a C1 path that may overshoot a joint range and, by a little, the limit the plan was made for.
    Returns ``(qpos_out, seq_offsets_out, info)``: ordinary qpos and offsets at the same ``fps`` for ``lock_feet``,
    ``tracking_from_qpos``, ``dynamics_report``, ``MotionLibrary`` and ``compose_clips``; ``info`` holds per clip ``stretch`` (output
    over input duration; 1 for a clip of fewer than two frames), ``stretched_intervals``, ``capped_intervals``,
    ``nonfinite_intervals`` and ``need_max`` (host arrays ``[S]``), and per frame ``need`` (device ``[N]``: the interval's largest
    speed over its limit, at its first row) and ``src_time`` (device ``[M]``: the source time of every output row in frames of its
    clip, for warping per-frame labels such as contacts).
    The output lengths depend on the data: between the two calls ``out_len`` is read back from the device -- the one host
    synchronisation, once per distinct rate."""
    if gmr.model.planar_base:
        raise NotImplementedError("retiming assumes a free-joint root; a planar-base robot is not supported")
    eng = gmr._engine
    vmax = retime_vmax(gmr.model, velocity_limits, getattr(gmr, "velocity_limits", None))
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    S, N = offs.size - 1, int(qpos.shape[0])
    if offs.ndim != 1 or S < 0 or offs[0] != 0 or offs[-1] != N or np.any(np.diff(offs) < 0):
        raise ValueError("seq_offsets must span [0, N] and not go back")
    f = np.asarray(fps.detach().cpu().numpy() if isinstance(fps, torch.Tensor) else fps, dtype=np.float64)
    f = np.full(S, float(f)) if f.ndim == 0 else f
    if f.shape != (S,):
        raise ValueError("fps must be one rate or one rate per clip")
    lens = np.diff(offs)
    out_len = np.zeros(S, dtype=np.int64)
    stats = np.zeros((S, 4), dtype=np.int64)
    need_max = np.zeros(S)
    need = torch.zeros(N, dtype=torch.float64, device=qpos.device)
    vdev = torch.from_numpy(vmax).to(qpos.device)
    parts = []   # (clips, their plan, their qpos and offsets) per distinct rate
    for rate in np.unique(f[lens > 0]):
        sel = np.flatnonzero((f == rate) & (lens > 0))
        if sel.size == np.count_nonzero(lens > 0):  # one rate: the batch as it is
            sel, rows, q, o = np.arange(S), None, qpos, offs
        else:
            rows = torch.from_numpy(np.concatenate([np.arange(offs[s], offs[s + 1]) for s in sel])).to(qpos.device)
            q, o = qpos.index_select(0, rows), np.concatenate([[0], np.cumsum(lens[sel])]).astype(np.int64)
        plan = eng.motion_retime_plan(q, o, float(rate), vdev, window, max_stretch)
        out_len[sel] = plan["out_len"].cpu().numpy()   # the host synchronisation
        stats[sel], need_max[sel] = plan["clip_stats"].cpu().numpy(), plan["need_max"].cpu().numpy()
        if rows is None:
            need = plan["need"]
        else:
            need.index_copy_(0, rows, plan["need"])
        parts.append((sel, plan, q, o))
    offs_out = np.concatenate([[0], np.cumsum(out_len)]).astype(np.int64)
    M = int(offs_out[-1])
    qpos_out = torch.empty((M, eng.nq), dtype=torch.float64, device=qpos.device)
    src_time = torch.empty(M, dtype=torch.float64, device=qpos.device)
    for sel, plan, q, o in parts:
        oo = np.concatenate([[0], np.cumsum(out_len[sel])]).astype(np.int64)
        if len(parts) == 1:
            eng.motion_retime_apply(q, o, plan, oo, out={"qpos": qpos_out, "src_time": src_time}, interp=interp)
        else:
            part, st, _ = eng.motion_retime_apply(q, o, plan, oo, interp=interp)
            rows = torch.from_numpy(np.concatenate([np.arange(offs_out[s], offs_out[s + 1]) for s in sel])).to(qpos.device)
            qpos_out.index_copy_(0, rows, part)
            src_time.index_copy_(0, rows, st)
    with np.errstate(invalid="ignore", divide="ignore"):
        stretch = np.where(lens > 1, (out_len - 1) / np.maximum(lens - 1, 1), 1.0)
    info = {"stretch": stretch, "stretched_intervals": stats[:, 0], "capped_intervals": stats[:, 1], "nonfinite_intervals": stats[:, 2],
            "need_max": need_max, "need": need, "src_time": src_time}
    return qpos_out, offs_out, info


# ------------------------------------------------------------------ retiming to torque limits
# Conventions from CPU runs on synthetic G1 trajectories, not measured on a robot: planning against 0.95 of the limit
# leaves room for the term of a changing stretch that the plan does not model, twelve intervals on either side keep that term small,
# and four passes were one or two more than those runs needed.
RETIME_TORQUE_SCALE = 0.95
RETIME_TORQUE_WINDOW = 12
RETIME_TORQUE_PASSES = 4


def _compose_src_time(prev: torch.Tensor, prev_offs: np.ndarray, st: torch.Tensor, out_len: np.ndarray) -> torch.Tensor:
    """The source time of the rows of a pass: ``prev`` (the source time of the pass's input rows, clips at ``prev_offs``) read at the
    pass's own ``st`` (in frames of its input clip), piecewise linearly.  Plumbing: torch indexing."""
    dev = st.device
    lens = torch.from_numpy(np.diff(prev_offs)).to(dev)
    reps = torch.from_numpy(np.ascontiguousarray(out_len)).to(dev)
    base = torch.repeat_interleave(torch.from_numpy(np.ascontiguousarray(prev_offs[:-1])).to(dev), reps)
    last = torch.repeat_interleave(lens, reps) - 1
    i = torch.minimum(st.floor().to(torch.int64), last)
    u = st - i.to(st.dtype)
    a, b = prev[base + i], prev[base + torch.minimum(i + 1, last)]
    return torch.where(u == 0.0, a, a + u * (b - a))


def retime_to_torque_limits(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], fps, table=None,
                            limit_scale: float = RETIME_TORQUE_SCALE, velocity_limits=False, window: int = RETIME_TORQUE_WINDOW,
                            max_stretch: float = RETIME_MAX_STRETCH, passes: int = RETIME_TORQUE_PASSES, interp: str = "cubic"):
    """qpos ``[N, nq]`` float64 on the GPU (concatenated clips at the one rate ``fps``) played slower exactly where a hinge needs more
    torque than its actuator has, on the GPU (the definition is the contract above ``gmr_retime_torque_input`` in
    include/gmr_amd.h).  Played slower by ``s``, a hinge's torque is ``g + (tau - g) / s^2``, ``g`` the gravity torque of the pose,
    so per pass ``Engine.motion_dynamics`` runs twice on the current clips -- once differenced, once with zero ``qvel`` / ``qacc`` --
    then ``Engine.motion_retime_plan_torque`` (against ``limit_scale`` of ``table``'s torque limits; ``None``: the robot's MJCF
    file's), the one read-back of the pass (``out_len`` and ``clip_stats`` together) and ``Engine.motion_retime_apply`` with
    ``interp``.  A slower clip has other torques where the stretch changes along it, which the plan does not model: the passes meet
    that by iteration.  The loop stops when no interval of any clip has need > 1, or after ``passes``; a clip with nothing to
    stretch gets 1024 ticks per interval, so the later passes copy it bit for bit.  ``velocity_limits``: ``False``: torques alone;
    ``True``: ``retime_vmax``'s default table, else its ``velocity_limits`` -- each pass then also runs ``Engine.motion_retime_plan``,
    whose ``need`` becomes the floor of the torque plan, so that one warp meets both limits.
    Torques are made from second differences of qpos: those of unfiltered IK output are dominated by the frame-to-frame jitter of
    the solve (``dynamics_from_qpos``), and a warp planned from noise is noise.  Smooth first (``smooth_qpos``).
    ``limit_scale``, ``window`` and ``passes`` default to ``RETIME_TORQUE_SCALE`` (0.95), ``RETIME_TORQUE_WINDOW`` (12) and
    ``RETIME_TORQUE_PASSES`` (4): conventions from CPU runs on synthetic trajectories, not measured on a robot.
    Returns ``(qpos_out, seq_offsets_out, info)``: ordinary qpos and offsets at the same ``fps``.  ``info`` holds per clip (host
    arrays ``[S]``) ``passes`` (the passes that stretched the clip), ``tau_ratio_before`` and ``tau_ratio_after`` (the largest
    ``tau_ratio_max`` of the dynamics statistics over the hinges, against the unscaled limits), ``converged`` (``tau_ratio_after <=
    1``), ``static_over_frames`` (source frames in which gravity alone puts a hinge at or over the scaled limit: no retiming
    mends those) and ``stretch``; per pass and clip (``[P, S]``) ``stretched_intervals``, ``capped_intervals`` and
    ``nonfinite_intervals``; and per output row ``src_time`` (device ``[M]``): the source time in frames of its clip, composed over
    the passes."""
    if gmr.model.planar_base:
        raise NotImplementedError("retiming assumes a free-joint root; a planar-base robot is not supported")
    eng = gmr._engine
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    S, N = offs.size - 1, int(qpos.shape[0])
    if offs.ndim != 1 or S < 0 or offs[0] != 0 or offs[-1] != N or np.any(np.diff(offs) < 0):
        raise ValueError("seq_offsets must span [0, N] and not go back")
    f = np.asarray(fps.detach().cpu().numpy() if isinstance(fps, torch.Tensor) else fps, dtype=np.float64)
    if f.ndim != 0 and np.unique(f).size > 1:
        raise ValueError("retiming to torque limits takes one rate per call: the inverse dynamics does")
    rate = float(f) if f.ndim == 0 else (float(f.flat[0]) if f.size else 30.0)
    if int(passes) < 1:
        raise ValueError("passes must be at least 1")
    dev = qpos.device
    limit = eng.inertial_device(table)["torque_limit"]
    vdev = None
    if velocity_limits is not False:
        vmax = retime_vmax(gmr.model, None if velocity_limits is True else velocity_limits, getattr(gmr, "velocity_limits", None))
        vdev = torch.from_numpy(vmax).to(dev)
    lens0 = np.diff(offs)
    q, o = qpos, offs
    src = torch.cat([torch.arange(int(n), dtype=torch.float64, device=dev) for n in lens0]) if N else torch.zeros(0, dtype=torch.float64, device=dev)
    ratios, per_pass, static_frames = [], [], None
    used = np.zeros(S, dtype=np.int64)
    for p in range(int(passes) + 1):
        n = int(q.shape[0])
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)   # noqa: E731  (the outputs the loop needs, no others)
        dyn = eng.motion_dynamics(q, o, rate, table=table, out={"tau": z(n, eng.nq - 7), "root_wrench": z(n, 6), "tau_ratio_max": z(S, eng.nq - 7)})
        ratios.append(dyn["tau_ratio_max"].max(dim=1).values if eng.nq > 7 else torch.zeros(S, dtype=torch.float64, device=dev))
        if p == int(passes):
            break
        zero = z(n, eng.nq - 1)
        rest = eng.motion_dynamics(q, o, rate, qvel=zero, qacc=zero, table=table, out={"tau": z(n, eng.nq - 7)})
        floor = eng.motion_retime_plan(q, o, rate, vdev, window, max_stretch)["need"] if vdev is not None else None
        plan = eng.motion_retime_plan_torque(dyn["tau"], rest["tau"], o, limit, limit_scale, window, max_stretch, floor, True)
        if static_frames is None:
            cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((plan["static_over"] > 0).to(torch.int64), 0)])
            od = plan.seq_offsets
            static_frames = cs[od[1:]] - cs[od[:-1]]
        back = torch.cat([plan["out_len"][:, None], plan["clip_stats"]], dim=1).cpu().numpy()   # the pass's one read-back
        out_len, stats = back[:, 0], back[:, 1:]
        per_pass.append(stats[:, :3].copy())
        if not stats[:, 0].any():
            break
        used += stats[:, 0] > 0
        oo = np.concatenate([[0], np.cumsum(out_len)]).astype(np.int64)
        q_new, st, _ = eng.motion_retime_apply(q, o, plan, oo, interp=interp)
        src = _compose_src_time(src, o, st, out_len)
        q, o = q_new, oo
    before, after = ratios[0].cpu().numpy(), ratios[-1].cpu().numpy()
    pp = np.stack(per_pass) if per_pass else np.zeros((0, S, 3), dtype=np.int64)
    lens = np.diff(o)
    with np.errstate(invalid="ignore", divide="ignore"):
        stretch = np.where(lens0 > 1, (lens - 1) / np.maximum(lens0 - 1, 1), 1.0)
    info = {"passes": used, "tau_ratio_before": before, "tau_ratio_after": after, "converged": after <= 1.0,
            "static_over_frames": static_frames.cpu().numpy() if static_frames is not None else np.zeros(S, dtype=np.int64),
            "stretch": stretch, "stretched_intervals": pp[:, :, 0], "capped_intervals": pp[:, :, 1], "nonfinite_intervals": pp[:, :, 2],
            "src_time": src}
    return q, o, info


# ------------------------------------------------------------------ transitions between clips
def find_transitions(gmr: GeneralMotionRetargeting, qpos: torch.Tensor, seq_offsets: Sequence[int], bodies=None, weights=None,
                     window: int = 8, stride: int = 1, src_clips=None, dst_clips=None, min_gap=None, threshold=None, radius=None):
    """Where a segment of one clip may follow a segment of another, on the GPU (``Engine.motion_transitions``; the definition is the
    contract above ``gmr_transitions_input`` in include/gmr_amd.h): the motion-graph distance of every ``stride``-th window of
    ``window`` frames of the clips ``src_clips`` to every window of the clips ``dst_clips`` (``None``: all clips), and of those the
    transitions worth taking (``gmr_amd.transitions.select_transitions``).  ``bodies``: body names or indices (``None``: all bodies);
    ``weights``: one per body (``None``: equal).  ``min_gap=None`` means ``window``: inside one clip a window is not matched with
    itself or an overlapping neighbour.  ``threshold=None`` and ``radius=None`` mean ``gmr_amd.transitions.DEFAULT_THRESHOLD``
    (m^2) and ``window``: conventions, not measured on a robot.  The default ``window`` is ``compose_clips``' default ``blend``.
    Returns ``(transitions, best_cost [E, D], best_frame [E, D])``: a list of ``gmr_amd.transitions.Transition`` and the host
    arrays it was chosen from, source ``e`` as in ``gmr_amd.transitions.search_tables``.  ``gmr_amd.transitions.transition_walks``
    turns the list into ``sequences`` for ``compose_clips(..., blend=window)``."""
    from .transitions import DEFAULT_THRESHOLD, select_transitions
    eng = gmr._engine
    names = list(eng.cm.robot.body_names)
    if bodies is None:
        ids = np.arange(eng.nbody, dtype=np.int32)
    else:
        ids = np.asarray([names.index(b) if isinstance(b, str) else int(b) for b in bodies], dtype=np.int32)
    w = np.ones(ids.size) if weights is None else np.asarray(weights, dtype=np.float64)
    got = eng.motion_transitions(qpos, seq_offsets, ids, w, int(window), src_clips, dst_clips, int(stride),
                                 int(window) if min_gap is None else int(min_gap))
    best_cost, best_frame = got["best_cost"].cpu().numpy(), got["best_frame"].cpu().numpy()
    trans = select_transitions(best_cost, best_frame, got.src_clips, got.src_offsets, got.stride, got.dst_clips,
                               DEFAULT_THRESHOLD if threshold is None else float(threshold), int(window) if radius is None else int(radius))
    return trans, best_cost, best_frame


# ------------------------------------------------------------------ the motion library
class MotionLibrary:
    """A set of retargeted clips of one robot kept on the GPU as qpos (288 B per G1 frame) and sampled at arbitrary times: what a
    tracking / AMP trainer asks at every simulation step, one kernel per call (``Engine.motion_sample``; the definition is the
    contract of ``gmr_motion_sample`` in include/gmr_amd.h).

    ``qpos`` ``[N, nq]`` float64 (free-joint layout ``[x y z qw qx qy qz hinges]``, concatenated clips) and ``seq_offsets``
    ``[S + 1]`` as numpy arrays or device tensors; ``fps``: one rate, or one per clip.  Attributes: ``num_clips``, ``num_frames``,
    ``durations`` (device float64 ``[S]``: ``(T - 1) / fps``, 0 for a clip of one frame or none).  ``lowpass_hz``: the clips are
    filtered once at construction (``smooth_qpos``); ``None``: kept as they are.  ``mirror=True``: the library stores
    ``augment_mirror``'s result -- the (filtered) clips and then their mirror images about ``mirror_about`` -- so ``num_clips``
    doubles and clip ``S + i`` is the mirror of clip ``i``; the sampling kernel knows nothing of it."""

    def __init__(self, gmr: GeneralMotionRetargeting, qpos, seq_offsets, fps, lowpass_hz: Optional[float] = None, mirror: bool = False,
                 mirror_about: str = "start", mirror_plan=None):
        if gmr.model.planar_base:
            raise NotImplementedError("the motion library assumes a free-joint root; a planar-base robot is not supported")
        from .schedule import clip_durations
        self.gmr = gmr
        self._eng = eng = gmr._engine
        dev = eng.device
        offs = seq_offsets.detach().cpu().numpy() if isinstance(seq_offsets, torch.Tensor) else seq_offsets
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        q = torch.from_numpy(np.ascontiguousarray(qpos, dtype=np.float64)) if not isinstance(qpos, torch.Tensor) else qpos
        if q.dim() != 2 or q.shape[1] != eng.nq or q.dtype != torch.float64:
            raise ValueError(f"qpos must be a float64 [N, {eng.nq}] array")
        if offs.ndim != 1 or offs.size < 1 or offs[0] != 0 or offs[-1] != q.shape[0]:
            raise ValueError("seq_offsets must span [0, N]")
        f = fps.detach().cpu().numpy() if isinstance(fps, torch.Tensor) else fps
        dur = clip_durations(offs, f)  # (checks the offsets and the rates)
        S = offs.size - 1
        f = np.array(np.broadcast_to(np.asarray(f, dtype=np.float64), (S,)))  # (a writable copy)
        self.qpos = q.to(dev).contiguous()
        if lowpass_hz:  # filtered once, here: the queries read the smoothed clips
            self.qpos = smooth_qpos(gmr, self.qpos, offs, f, lowpass_hz)
        if mirror:
            self.qpos, offs, f = augment_mirror(gmr, self.qpos, offs, f, about=mirror_about, plan=mirror_plan)
            dur, S = np.concatenate([dur, dur]), 2 * S
        self.seq_offsets = offs
        self.fps = f
        self.num_clips, self.num_frames = S, int(offs[-1])
        self._offs_dev = torch.from_numpy(offs).to(dev)
        self._fps_dev = torch.from_numpy(f).to(dev)
        self.durations = torch.from_numpy(dur).to(dev)
        lens = np.diff(offs)
        w = dur if dur.sum() > 0 else (lens > 0).astype(np.float64)  # all durations 0: uniform over the clips that have a frame
        self._weights = torch.from_numpy(np.ascontiguousarray(w)).to(dev) if w.sum() > 0 else None
        self._bodies = {}

    @classmethod
    def from_motions(cls, gmr: GeneralMotionRetargeting, motions: Sequence[Dict], lowpass_hz: Optional[float] = None, **mirror_kw) -> "MotionLibrary":
        """From motion dicts (``retarget_clips`` / the dict of ``load_robot_motion``): ``root_pos``, xyzw ``root_rot``, ``dof_pos``
        and ``fps`` of every clip, checked with ``validate_motion``."""
        nq = gmr._engine.nq
        rows, lens, fps = [], [], []
        for m in motions:
            validate_motion(m, nq)
            rr = np.asarray(m["root_rot"], dtype=np.float64)
            rows.append(np.concatenate([np.asarray(m["root_pos"], dtype=np.float64), rr[:, [3, 0, 1, 2]],
                                        np.asarray(m["dof_pos"], dtype=np.float64)], axis=1))
            lens.append(rows[-1].shape[0])
            fps.append(float(m["fps"]))
        qpos = np.concatenate(rows) if rows else np.zeros((0, nq))
        return cls(gmr, qpos, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(fps, dtype=np.float64),
                   lowpass_hz=lowpass_hz, **mirror_kw)

    def sample_ids(self, n: int, generator=None) -> torch.Tensor:
        """``n`` clip ids (device int64) drawn in proportion to the durations; a clip without frames is never drawn."""
        if self._weights is None:
            raise ValueError("the library holds no frames")
        return torch.multinomial(self._weights, int(n), replacement=True, generator=generator)

    def sample_times(self, ids: torch.Tensor, generator=None) -> torch.Tensor:
        """One time per id (device float64), uniform in ``[0, duration]``."""
        d = self.durations[ids]
        return torch.rand(d.shape, dtype=torch.float64, device=d.device, generator=generator) * d

    def body_ids(self, bodies: Sequence[str]) -> torch.Tensor:
        """The device int32 index tensor of a list of body names, resolved once per tuple of names."""
        key = tuple(bodies)
        if key not in self._bodies:
            names = list(self.gmr.model.body_names)
            missing = [b for b in key if b not in names]
            if missing:
                raise KeyError(f"unknown bodies {missing}")
            self._bodies[key] = torch.tensor([names.index(b) for b in key], dtype=torch.int32, device=self._eng.device)
        return self._bodies[key]

    def query(self, ids: torch.Tensor, times: torch.Tensor, future: Optional[torch.Tensor] = None, bodies: Optional[Sequence[str]] = None,
              fields=None, out=None, dtype=torch.float32, check: bool = True):
        """The reference state of clip ``ids[e]`` at ``times[e]`` seconds (device tensors ``[E]``; or flat ``[Q]`` pairs), as an
        ``engine.MotionSample`` named as ``TRACK_ARRAYS``.  ``future``: a 1-D device tensor of K offsets in seconds -- every id is
        then answered at ``times[e] + future[k]``, shapes ``[E, K, ...]``.  ``bodies``: the body names of the four body arrays, in
        this order (default: all, in model order).  ``fields`` / ``out`` / ``dtype``: as ``Engine.motion_sample``.  Times outside
        ``[0, duration]`` clamp to the clip's ends.  ``check=True`` validates the id range on the device (one synchronisation)
        and raises ``ValueError``; ``check=False`` is for training loops: a bad id, an empty clip or a non-finite time gives NaN
        rows and nothing is read out of range."""
        if check and ids.numel() > 0 and bool(((ids < 0) | (ids >= self.num_clips)).any()):
            raise ValueError(f"clip ids must lie in [0, {self.num_clips})")
        if future is not None:
            if future.dim() != 1 or times.dim() != 1:
                raise ValueError("future must be 1-D offsets for 1-D times")
            times = times[:, None] + future
        return self._eng.motion_sample(self.qpos, self._offs_dev, self._fps_dev, ids, times,
                                       k_per_id=int(times.shape[1]) if times.dim() == 2 else 1,
                                       bodies=None if bodies is None else self.body_ids(bodies), fields=fields, out=out, dtype=dtype)


def save_tracking(path: str, track: Dict, override: bool = False) -> bool:
    """One tracking dict as an uncompressed ``.npz`` (``np.savez``); like ``save_motion``, an existing file is skipped unless
    ``override``.  Names and ``quat_order`` are stored as unicode arrays, ``fps`` as a float64 scalar.  A dict with contact
    labels (``tracking_from_qpos(..., contact_bodies=...)``) also stores ``contact``, ``contact_body_names``, one array
    ``contact_stats_<key>`` per statistic and ``airborne_frames``, behind the other arrays; without them the file is what it
    always was."""
    if os.path.exists(path) and not override:
        return False
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    extra = {}
    if "contact" in track:
        extra = {"contact": track["contact"], "contact_body_names": np.asarray(list(track["contact_body_names"]), dtype=np.str_),
                 "airborne_frames": np.int32(track["airborne_frames"])}
        extra.update(("contact_stats_" + k, np.asarray(track["contact_stats"][k])) for k in CONTACT_STATS)
    if "footlock_stats" in track:  # (tracking_from_qpos(..., lock_feet=...): one array footlock_stats_<key> per statistic)
        extra.update(("footlock_stats_" + k, np.asarray(track["footlock_stats"][k])) for k in FOOTLOCK_STATS)
    with open(path, "wb") as f:  # (a file object: np.savez appends nothing to the name)
        np.savez(f, fps=np.float64(track["fps"]), body_names=np.asarray(list(track["body_names"]), dtype=np.str_),
                 joint_names=np.asarray(list(track["joint_names"]), dtype=np.str_), quat_order=np.asarray(track["quat_order"]),
                 **{k: track[k] for k in TRACK_ARRAYS}, **extra)
    return True


def load_tracking(path: str) -> Dict:
    """Read a ``save_tracking`` file back: the same keys, arrays as written, names as lists, ``fps`` a float; the contact keys
    when the file holds them (``airborne_frames`` an int, ``base`` of ``contact_stats`` a float64 scalar)."""
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in TRACK_ARRAYS}
        d.update(fps=float(z["fps"]), body_names=[str(n) for n in z["body_names"]], joint_names=[str(n) for n in z["joint_names"]],
                 quat_order=str(z["quat_order"]))
        if "contact" in z.files:
            stats = {k: z["contact_stats_" + k] for k in CONTACT_STATS}
            stats["base"] = np.float64(stats["base"])
            d.update(contact=z["contact"], contact_body_names=[str(n) for n in z["contact_body_names"]], contact_stats=stats,
                     airborne_frames=int(z["airborne_frames"]))
        if "footlock_stats_runs" in z.files:
            d["footlock_stats"] = {k: z["footlock_stats_" + k] for k in FOOTLOCK_STATS}
    return d


# ------------------------------------------------------------------ the clip report on disk
def _report_host(report):
    """The report with host arrays: a ``ClipReport`` holding any device tensor is copied (``ClipReport.numpy``)."""
    if hasattr(report, "numpy") and any(isinstance(v, torch.Tensor) for v in vars(report).values()):
        return report.numpy()
    return report


def write_report_csv(path: str, names: Sequence[str], report, append: bool = False) -> None:
    """One row per clip of an ``engine.ClipReport``: clip name, frames, the scalar fields (both stage errors' max and mean, root
    step / turn, solves, non-finite frames), then per task ``<task>:pos_max`` / ``<task>:rot_max`` and per hinge
    ``<hinge>:step_max`` / ``<hinge>:near_lo`` / ``<hinge>:near_hi``.  A field the report does not hold is left out.  ``append``:
    add the rows to an existing file of the same columns, without a second header (a run's batches, one after the other)."""
    import csv
    r = _report_host(report)
    if len(names) != len(r):
        raise ValueError("one name per clip")
    cols = [("clip", list(names)), ("frames", r.frames.tolist())]
    if r.err_max is not None:
        mean = r.err_mean
        for k in (0, 1):
            cols += [(f"err{k + 1}_max", r.err_max[:, k].tolist()), (f"err{k + 1}_mean", mean[:, k].tolist())]
    for key in ("root_step_max", "root_turn_max", "solves_max", "solves_sum", "nonfinite_frames"):
        v = getattr(r, key)
        if v is not None:
            cols.append((key, v.tolist()))
    for field, tag in (("task_pos_max", "pos_max"), ("task_rot_max", "rot_max")):
        v = getattr(r, field)
        if v is not None:
            cols += [(f"{n}:{tag}", v[:, i].tolist()) for i, n in enumerate(r.task_names)]
    for field, tag in (("dof_step_max", "step_max"), ("near_lo", "near_lo"), ("near_hi", "near_hi")):
        v = getattr(r, field)
        if v is not None:
            cols += [(f"{n}:{tag}", v[:, i].tolist()) for i, n in enumerate(r.hinge_names)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a" if append else "w", newline="") as f:
        w = csv.writer(f)
        if not append:
            w.writerow([c for c, _ in cols])
        for i in range(len(r)):
            w.writerow([repr(v[i]) if isinstance(v[i], float) else v[i] for _, v in cols])


def report_difficulty(report) -> np.ndarray:
    """[S]: ``err_max`` of the last table the config uses -- the difficulty ``write_hard_list`` records."""
    r = _report_host(report)
    if r.err_max is None:
        raise ValueError("the report holds no stage errors (it was made without key-points)")
    return np.asarray(r.err_max)[:, r.last_table]


def report_hard_mask(report, max_pos_err: Optional[float] = None, max_dof_step: Optional[float] = None) -> np.ndarray:
    """[S] bool: clips whose largest task position error exceeds ``max_pos_err`` (m) or whose largest joint step between
    consecutive frames exceeds ``max_dof_step`` (rad); ``None`` switches a test off."""
    r = _report_host(report)
    mask = np.zeros(len(r), dtype=bool)
    if max_pos_err is not None:
        if r.task_pos_max is None:
            raise ValueError("the report holds no task errors (it was made without key-points)")
        mask |= np.asarray(r.task_pos_max).max(axis=1, initial=0.0) > max_pos_err
    if max_dof_step is not None:
        mask |= np.asarray(r.dof_step_max).max(axis=1, initial=0.0) > max_dof_step
    return mask


def write_hard_list(path: str, names: Sequence[str], report, mask, append: bool = False) -> int:
    """The clips of ``mask`` in the reference's hard-motion list format (assets/hard_motions/*.txt, read back by the dataset
    scripts' ``--hard_motions``): ``Motion: <name>.pkl, Difficulty: <%.2f>`` per line, difficulty = ``report_difficulty``.
    Returns the number of lines written."""
    mask = np.asarray(mask, dtype=bool)
    if len(names) != len(mask):
        raise ValueError("one name per clip")
    diff = report_difficulty(report)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    n = 0
    with open(path, "a" if append else "w") as f:
        for name, hard, d in zip(names, mask, diff):
            if hard:
                f.write(f"Motion: {name}.pkl, Difficulty: {d:.2f}\n")
                n += 1
    return n


# ------------------------------------------------------------------ writing motion files (row f-3)
class _RawBytes:
    """The data of a C-contiguous array standing in for the ``bytes`` object numpy's reduce would copy it into."""
    __slots__ = ("view",)

    def __init__(self, arr: np.ndarray):
        self.view = memoryview(arr).cast("B")

    def __len__(self):
        return self.view.nbytes


class _MotionPickler(pickle._Pickler):
    """``pickle.dump(motion, f)`` byte for byte (protocol 4, the default the reference's ``pickle.dump`` uses,
    scripts/smplx_to_robot_dataset.py:143-146), without the two things that make it slow for motion dicts: ``ndarray.__reduce__``
    first copies every array into a ``bytes`` object (under the GIL), and only then is that copy written.  Here an array's reduce
    tuple is rebuilt around a view of its own memory and the payload goes from that memory straight into ``file.write`` (which
    releases the GIL), so a pool of threads writes clips in parallel.  ``fast_pickle_ok()`` checks the byte identity once per
    process against the stock pickler; where it does not hold the stock pickler is used."""

    def reducer_override(self, obj):
        if type(obj) is np.ndarray and obj.flags.c_contiguous and obj.dtype.kind in "fiub" and obj.nbytes >= 1 << 16:
            fn, args, state = np.empty((0,) * obj.ndim, dtype=obj.dtype).__reduce__()
            return fn, args, (state[0], obj.shape, obj.dtype, False, _RawBytes(obj))
        return NotImplemented

    def _save_raw(self, obj):  # pickle._Pickler.save_bytes for a payload that is a view, not a bytes object
        n = len(obj)
        if n > 0xFFFFFFFF:
            self._write_large_bytes(pickle.BINBYTES8 + n.to_bytes(8, "little"), obj.view)
        else:
            self._write_large_bytes(pickle.BINBYTES + n.to_bytes(4, "little"), obj.view)
        self.memoize(obj)

    dispatch = dict(pickle._Pickler.dispatch)
    dispatch[_RawBytes] = _save_raw


_FAST_PICKLE_OK: Optional[bool] = None


def fast_pickle_ok() -> bool:
    """True when ``_MotionPickler`` reproduces the stock ``pickle.dump`` byte for byte on a motion-shaped dict here (checked once:
    it rests on numpy's reduce format and the pickler's framing rules, both of which a new version could change)."""
    global _FAST_PICKLE_OK
    if _FAST_PICKLE_OK is None:
        import io
        rng = np.random.default_rng(0)
        probe = {"fps": 30, "root_pos": rng.random((4000, 3)), "root_rot": rng.random((4000, 4)), "dof_pos": rng.random((4000, 29)),
                 "local_body_pos": rng.random((4000, 38, 3)).astype(np.float32), "link_body_list": ["a", "b"], "small": rng.random((5, 3))}
        f = io.BytesIO()
        try:
            _MotionPickler(f, pickle.DEFAULT_PROTOCOL).dump(probe)
            _FAST_PICKLE_OK = pickle.DEFAULT_PROTOCOL >= 4 and f.getvalue() == pickle.dumps(probe)
        except Exception:
            _FAST_PICKLE_OK = False
    return _FAST_PICKLE_OK


def save_motion(path: str, motion: Dict, override: bool = False) -> bool:
    """Pickle one motion dict; like the scripts, skip files that already exist unless ``override`` (:219).  The file is
    what ``pickle.dump(motion, f)`` writes, byte for byte (see ``_MotionPickler``).  A ``.npz`` path takes a tracking dict
    (``save_tracking``), so ``MotionWriter`` writes both kinds."""
    if str(path).endswith(".npz"):  # a tracking dict (tracking_from_qpos)
        return save_tracking(path, motion, override)
    if os.path.exists(path) and not override:
        return False
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if str(path).endswith(".pt"):  # the torch twin of the schema (scripts/convert_motion_pkl_to_pt.py:40-48): arrays as tensors
        torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v for k, v in motion.items()}, path)
        return True
    if fast_pickle_ok():
        _write_all(path, motion_stream(motion))
    else:
        with open(path, "wb") as f:
            pickle.dump(motion, f)
    return True


class _Pieces:
    """File object of ``_MotionPickler`` that keeps what it is given: small pieces as bytes, array payloads as views."""

    def __init__(self):
        self.pieces = []

    def write(self, b):
        self.pieces.append(b if isinstance(b, memoryview) and b.nbytes >= 1 << 16 else bytes(b))
        return len(b)


_STREAM_TEMPLATES: Dict = {}
_SMALL_MIN = 256  # arrays below this many bytes are part of a layout's key, like the scalars


class _Template:
    """The pickle of one motion layout with its numbers taken out: ``pieces`` are the stream's buffers in order -- bytes (opcodes,
    frame headers, strings, ...), or the KEY of a large array whose memory goes there as it is; ``patches`` say where, inside the
    bytes pieces, the raw data of the layout's small arrays lie (piece, offset, size, key).  Built from the first clip of a layout,
    compared once against the full pickler run of the second clip (``verified``), used from the third on."""
    __slots__ = ("pieces", "patches", "verified")

    def __init__(self, pieces, patches):
        self.pieces, self.patches, self.verified = pieces, patches, False

    def fill(self, motion: Dict) -> list:
        out = list(self.pieces)
        touched = {}
        for pi, off, n, k in self.patches:
            b = touched.get(pi)
            if b is None:
                b = touched[pi] = bytearray(out[pi])
                out[pi] = b
            b[off:off + n] = memoryview(motion[k]).cast("B")
        return [memoryview(motion[t]).cast("B") if isinstance(t, str) else t for t in out]


def _is_plain(v) -> bool:
    return type(v) is np.ndarray and v.flags.c_contiguous and v.dtype.kind in "fiub"


def _full_stream(motion: Dict):
    out = _Pieces()
    _MotionPickler(out, pickle.DEFAULT_PROTOCOL).dump(motion)
    return out.pieces


def _build_template(motion: Dict, big, small) -> Optional[_Template]:
    """Pickle a SHADOW of the clip -- same layout, the small arrays filled with random bytes -- and find those bytes in the stream: a
    clip's own numbers can be degenerate (a block of zeros also matches the zero bytes of the length field in front of it)."""
    rng = np.random.default_rng(0x5EED)
    shadow = dict(motion)
    marks = []
    for k, v in small:
        m = np.frombuffer(rng.bytes(v.nbytes), dtype=v.dtype).reshape(v.shape).copy()
        shadow[k] = m
        marks.append((k, m))
    pieces = _full_stream(shadow)
    small = marks
    order = {id(v): k for k, v in big}
    tp = []
    for p in pieces:
        if isinstance(p, memoryview) and id(p.obj) in order:
            tp.append(order[id(p.obj)])
        else:
            tp.append(bytes(p))
    if sum(isinstance(t, str) for t in tp) != len(big):
        return None
    patches, pi, pos = [], 0, 0
    for k, v in small:  # in dict order = stream order: search on from where the previous one ended
        raw = memoryview(v).cast("B").tobytes()
        while pi < len(tp):
            at = tp[pi].find(raw, pos) if isinstance(tp[pi], bytes) else -1
            if at >= 0:
                patches.append((pi, at, len(raw), k))
                pos = at + len(raw)
                break
            pi, pos = pi + 1, 0
        else:
            return None
    return _Template(tp, patches)


def motion_stream(motion: Dict) -> list:
    """The pickle of a motion dict as a list of buffers (headers as bytes, array payloads as views of the arrays' own memory).
    Clips of one batch differ in their numbers only, so the stream is kept per LAYOUT -- keys, array shapes and dtypes, and the pickle
    of everything that is not an array -- with the numbers taken out (``_Template``): a clip of a known layout costs a dict lookup and
    a copy of its small arrays (those below the pickler's 64 KB frame size, which travel inside frames), not a run of the pure-Python
    pickler (~0.5 ms under the GIL: every clip shorter than 2 731 frames has such arrays).  A layout's template is checked against the
    full pickler on the second clip that uses it before it is trusted."""
    big = [(k, v) for k, v in motion.items() if _is_plain(v) and v.nbytes >= 1 << 16]
    small = [(k, v) for k, v in motion.items() if _is_plain(v) and _SMALL_MIN <= v.nbytes < 1 << 16]
    if sum(v.nbytes for _, v in big) + sum(v.nbytes for _, v in small) < 1 << 15 or any(_is_plain(v) and v.nbytes < _SMALL_MIN for v in motion.values()):
        return [pickle.dumps(motion, pickle.DEFAULT_PROTOCOL)]  # a handful of frames: the stock pickler's copy costs nothing
    arrays = {k for k, _ in big} | {k for k, _ in small}
    try:
        rest = pickle.dumps([v for k, v in motion.items() if k not in arrays], pickle.DEFAULT_PROTOCOL)
    except Exception:
        return _full_stream(motion)
    key = (tuple(motion.keys()), tuple((k, v.shape, v.dtype.str) for k, v in big), tuple((k, v.shape, v.dtype.str) for k, v in small), rest)
    tmpl = _STREAM_TEMPLATES.get(key)
    if tmpl is False:  # a layout the template cannot express
        return _full_stream(motion)
    if tmpl is not None and tmpl.verified:
        return tmpl.fill(motion)
    pieces = _full_stream(motion)
    if tmpl is None:
        if len(_STREAM_TEMPLATES) >= 256:
            _STREAM_TEMPLATES.clear()
        _STREAM_TEMPLATES[key] = _build_template(motion, big, small) or False
    else:  # second clip of the layout: the template must reproduce the pickler's stream exactly
        a = b"".join(bytes(memoryview(x).cast("B")) for x in tmpl.fill(motion))
        b = b"".join(bytes(memoryview(x).cast("B")) for x in pieces)
        if a == b:
            tmpl.verified = True
        else:
            _STREAM_TEMPLATES[key] = False
    return pieces


def _write_all(path: str, pieces: list) -> None:
    """One gather-write of the whole file: a single system call, which is also the single stretch a writer thread spends without
    the GIL (threads that re-take the GIL between several writes of one file queue up behind each other's Python code)."""
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
    try:
        views = [memoryview(p).cast("B") for p in pieces]
        while views:
            n = os.writev(fd, views[:1024])
            while n > 0 and views:  # (a short write: drop what went out, go on with the rest)
                if n >= views[0].nbytes:
                    n -= views[0].nbytes
                    views.pop(0)
                else:
                    views[0] = views[0][n:]
                    n = 0
            while views and views[0].nbytes == 0:
                views.pop(0)
    finally:
        os.close(fd)


class MotionWriter:
    """Writes motion files on a pool of threads while the caller goes on to the next batch (the reference writes each clip from
    the process that solved it, scripts/smplx_to_robot_dataset.py:134-146, 241-242: one pickle per clip, skipped when it exists).

        with MotionWriter(workers=8) as w:
            for batch in batches:                        # batch k + 1 is solved while batch k is being written
                motions = retarget_clips(gmr, ...)
                w.submit(motions, paths)
        w.written, w.skipped

    ``submit`` returns at once while at most ``max_pending`` earlier batches are unwritten, else it waits for the oldest of them:
    the motion dicts (row slices of the batch's pinned result arrays, ``motions_from_qpos``) stay alive until their files are closed,
    so a disk slower than the GPU must hold the producer back instead of piling up page-locked batches.  An error in a worker is
    raised by the next ``submit`` / ``close``."""

    def __init__(self, workers: int = 8, override: bool = False, max_pending: int = 3):
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))
        self._override = override
        self._max_pending = max(1, int(max_pending))
        self._batches = []  # one list of futures per submitted batch, oldest first
        self._futures = []
        self.written = 0
        self.skipped = 0
        fast_pickle_ok()  # (decide once, before the threads start)

    def _reap(self, wait: bool):
        keep = []
        for f in self._futures:
            if wait or f.done():
                if f.result():
                    self.written += 1
                else:
                    self.skipped += 1
            else:
                keep.append(f)
        self._futures = keep

    def submit(self, motions: Sequence[Dict], paths: Sequence[str]) -> None:
        if len(motions) != len(paths):
            raise ValueError("one path per motion")
        self._reap(False)
        self._batches = [b for b in self._batches if not all(f.done() for f in b)]
        while len(self._batches) >= self._max_pending:   # back-pressure: wait for the oldest unwritten batch
            for f in self._batches.pop(0):
                f.exception()  # (waits; the error itself is raised by _reap below)
            self._reap(False)
        fs = [self._pool.submit(save_motion, p, m, self._override) for m, p in zip(motions, paths)]
        self._futures += fs
        self._batches.append(fs)

    def close(self) -> None:
        try:
            self._reap(True)
        finally:
            self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def save_motions(motions: Sequence[Dict], paths: Sequence[str], workers: int = 8, override: bool = False) -> int:
    """Write a batch of motion files (``.pkl`` or ``.pt`` by extension) on ``workers`` threads; returns how many were written
    (existing files are skipped unless ``override``).  Files are byte-identical to those of a serial ``save_motion`` loop."""
    with MotionWriter(workers, override) as w:
        w.submit(motions, paths)
    return w.written


def load_robot_motion(motion_file: str):
    """Reader with the contract of general_motion_retargeting/data_loader.py:4-18 (root_rot returned as wxyz)."""
    if str(motion_file).endswith(".pt"):  # (:50-58 of the converter: tensors back to arrays; files this package wrote)
        d = {k: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in torch.load(motion_file, map_location="cpu", weights_only=True).items()}
    else:
        with open(motion_file, "rb") as f:
            d = pickle.load(f)
    root_rot = d["root_rot"][:, [3, 0, 1, 2]]
    return d, d["fps"], d["root_pos"], root_rot, d["dof_pos"], d["local_body_pos"], d["link_body_list"]


def validate_motion(motion: Dict, nq: Optional[int] = None) -> None:
    """The structural checks of scripts/smoke_test.py:19-72."""
    for k in ("fps", "root_pos", "root_rot", "dof_pos"):
        if k not in motion:
            raise KeyError(k)
    T = motion["root_pos"].shape[0]
    if motion["root_pos"].shape != (T, 3) or motion["root_rot"].shape != (T, 4) or motion["dof_pos"].shape[0] != T:
        raise ValueError("bad motion shapes")
    if nq is not None and motion["dof_pos"].shape[1] != nq - 7:
        raise ValueError("dof count does not match the model")
    n = np.linalg.norm(motion["root_rot"], axis=1)
    if T and (n.min() < 0.5 or n.max() > 1.5):
        raise ValueError("root_rot is not a quaternion track")
