"""``MultiRobotRetargeting`` -- one human motion set retargeted to several robots in shared launches.

The reference retargets to one robot per process (scripts/smplx_to_robot_dataset.py:79-83: one ``GeneralMotionRetargeting`` per
file and robot).  Here the robots form one ``EngineGroup`` (a common kernel variant, ``gmr_group_*``): every robot's clips -- or
their parallel-in-time chunks and verification walks -- run in ONE grid, reading the same human key-points through each robot's
own slot columns.  Every argument of :meth:`MultiRobotRetargeting.retarget_batch` means what it means in
``GeneralMotionRetargeting.retarget_batch``, and each robot's result is what that call gives for the robot alone.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ._native import IKParams
from .params import IK_CONFIG_DICT, ROBOT_XML_DICT

MAX_ROBOTS = 64  # gmr_group_create's limit


class MultiRobotRetargeting:
    """Several robots retargeted from one human source in shared launches.

    ``mr.robots``: the robot names, in the order given; ``mr.engines``: the group's per-robot ``Engine`` (FK, evaluation, the dataset
    post-processing); ``mr.ik_columns``: the union of the robots' ``ik_columns`` (what a narrowed input needs);
    ``mr.last_chunk_info``: per robot, ``GeneralMotionRetargeting.last_chunk_info`` of the last batch.
    """

    def __init__(self, src_human: str, tgt_robots: Sequence[str], actual_human_height: float = None, damping: float = 5e-1,
                 device: int = 0, verbose: bool = False, use_velocity_limit: bool = False, velocity_limits=None) -> None:
        robots = list(tgt_robots)
        # every refusal before any device work
        if not robots:
            raise ValueError("no robots given")
        if len(robots) > MAX_ROBOTS:
            raise ValueError(f"{len(robots)} robots: a group holds at most {MAX_ROBOTS}")
        if len(set(robots)) != len(robots):
            raise ValueError(f"duplicate robots in {robots}")
        cfgs = IK_CONFIG_DICT[src_human]  # KeyError where the reference raises (motion_retarget.py:24-33)
        for r in robots:
            _ = ROBOT_XML_DICT[r], cfgs[r]
        from .engine import EngineGroup
        from .ik_config import load_ik_config
        from .mjcf import load_robot
        from .model import compile_model, resolve_velocity_limits
        self.src_human = src_human
        self.robots = robots
        self.damping = damping
        self.max_iter = 10
        self.models, self._cms = [], []
        # use_velocity_limit / velocity_limits as GeneralMotionRetargeting takes them, for every robot; velocity_limits may also be
        # {robot: number or {joint: rad/s}} -- a robot it does not name then has the switch alone
        per_robot = isinstance(velocity_limits, dict) and len(velocity_limits) > 0 and all(k in robots for k in velocity_limits)
        self.velocity_limits: Dict[str, Optional[dict]] = {}
        for r in robots:
            if verbose:
                print("Use robot model: ", ROBOT_XML_DICT[r], " IK config: ", cfgs[r])
            model = load_robot(str(ROBOT_XML_DICT[r]), name=r)
            self.models.append(model)
            self.velocity_limits[r] = resolve_velocity_limits(model, use_velocity_limit, velocity_limits.get(r) if per_robot else velocity_limits)
            self._cms.append(compile_model(model, load_ik_config(cfgs[r]), actual_human_height, velocity_limits=self.velocity_limits[r]))
        self.group = EngineGroup(self._cms, device)
        self.engines = self.group.engines
        self.device = self.group.device
        self.last_chunk_info: Dict[str, dict] = {}

    def close(self):
        self.group.close()

    @property
    def ik_columns(self) -> List[str]:
        """The human bodies any of the robots consumes, in first-appearance order over the robots."""
        out: List[str] = []
        for cm in self._cms:
            out += [n for n in cm.slot_names if n not in out]
        return out

    def _params(self, offset_to_ground: bool) -> IKParams:
        return IKParams(damping=self.damping, max_iter=self.max_iter, offset_to_ground=int(bool(offset_to_ground)))

    def retarget_batch(self, pos, quat, body_names: Sequence[str], seq_offsets=None, chunk=0, burn_in: int = 0,
                       offset_to_ground: bool = False, return_iters: bool = False, verify: bool = True,
                       human_heights: Optional[Sequence[float]] = None, check: bool = True, clip_start: str = "qpos0"):
        """``GeneralMotionRetargeting.retarget_batch`` for every robot at once: pos ``[N, B, 3]``, quat ``[N, B, 4]`` (wxyz),
        float32/float64, numpy or CUDA torch, one input for all robots.  Returns ``{robot: qpos [N, nq]}`` (numpy for numpy input,
        planar bases in the XML's layout) and, with ``return_iters``, ``{robot: solves per frame}`` as a second value.

        ``chunk > 0`` with ``verify``: every robot's chunks in one launch, every robot's verification walks in a second
        (``EngineGroup.ik_solve_chunked``).  ``chunk="auto"`` chooses chunk and burn-in (``schedule.auto_chunk``) from all robots'
        clips together, since they share the wavefront slots; ``(0, 0)`` means whole clips.  Whole clips go in one launch,
        cost-ordered across robots when the probe pays (``EngineGroup.ik_solve(launch_order="auto")``).  ``human_heights[s]`` applies to clip s of every robot,
        through each robot's own ``human_height_assumption`` and scale ratio.  ``check`` inspects every robot's solve-count flags.
        Numpy inputs with more columns than ``ik_columns`` are narrowed on the host first; there is no overlapped host pipeline
        (``Engine.ik_solve_host``) for several robots: large numpy batches are copied to the device in one piece.
        """
        from .motion_retarget import caller_layout_batch
        is_np = isinstance(pos, np.ndarray)
        outs, offs = self._solve(pos, quat, body_names, seq_offsets, chunk, burn_in, offset_to_ground, verify, human_heights, check, clip_start)
        qpos, iters = {}, {}
        for r, model, (q, it) in zip(self.robots, self.models, outs):
            q = caller_layout_batch(model, q, offs)
            qpos[r], iters[r] = (q.cpu().numpy(), it.cpu().numpy()) if is_np else (q, it)
        return (qpos, iters) if return_iters else qpos

    def clip_report(self, qpos: Dict[str, torch.Tensor], pos, quat, body_names: Sequence[str], seq_offsets=None,
                    human_heights: Optional[Sequence[float]] = None, iters: Optional[Dict] = None, offset_to_ground: bool = False,
                    limit_eps: Optional[float] = None, segment_frames: int = 0):
        """``GeneralMotionRetargeting.clip_report`` for every robot, all robots' segments in one grid
        (``EngineGroup.clip_report``): ``qpos[robot]`` / ``iters[robot]`` as :meth:`retarget_batch` returned them for these
        key-points.  Returns ``{robot: engine.ClipReport}``, bit for bit the single-robot reports."""
        from .engine import CLIP_REPORT_LIMIT_EPS
        names = list(body_names)
        as_t = lambda x: torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        tpos, tquat = as_t(pos).to(self.device).contiguous(), as_t(quat).to(self.device).contiguous()
        N = int(tpos.shape[0])
        offs = np.asarray([0, N] if seq_offsets is None else seq_offsets, dtype=np.int64)
        hh = None
        if human_heights is not None:
            hh = np.asarray(human_heights, dtype=np.float64)
            if hh.shape != (len(offs) - 1,):
                raise ValueError("human_heights must hold one height per clip")
        batches = []
        for r, model, cm in zip(self.robots, self.models, self._cms):
            q = as_t(qpos[r]).to(self.device)
            if model.planar_base and q.shape[1] == model.mj_nq:  # the XML's [x, y, yaw, hinges] -> the engine's layout
                q = torch.from_numpy(np.ascontiguousarray(model.from_mj_qpos(q.cpu().numpy()))).to(self.device)
            it = None if iters is None or iters.get(r) is None else as_t(iters[r]).to(self.device).to(torch.int32)
            batches.append({"qpos": q.to(torch.float64).contiguous(), "seq_offsets": offs, "pos": tpos, "quat": tquat,
                            "slot_col": cm.slot_columns(names), "iters": it,
                            "height_scale": None if hh is None else hh / cm.config.human_height_assumption / cm.ratio})
        reps = self.group.clip_report(batches, offset_to_ground=offset_to_ground, segment_frames=segment_frames,
                                      limit_eps=CLIP_REPORT_LIMIT_EPS if limit_eps is None else limit_eps)
        return dict(zip(self.robots, reps))

    def _refuse_planar(self):
        planar = [r for r, m in zip(self.robots, self.models) if m.planar_base]
        if planar:
            # dataset.motions_from_qpos's refusal: the motion schema reads a free-joint root out of qpos
            raise NotImplementedError(f"{planar}: the dataset post-processing assumes a free-joint root; use retarget_batch for a planar-base robot")

    def motions_from_qpos(self, qpos: Dict[str, torch.Tensor], seq_offsets: Sequence[int], fps, height_adjust: bool = True,
                          root_origin_offset: bool = True, ground_offset: float = 0.0) -> Dict[str, List[Dict]]:
        """``dataset.motions_from_qpos`` for every robot, post-processed in shared launches (``EngineGroup.motion_epilogue``):
        ``qpos[robot]`` ``[N, nq]`` float64 on the group's device, the same clips for every robot -> ``{robot: [motion dict per
        clip]}``, the same keys, dtypes and arrays as the single-robot call.  The arrays are row slices of per-robot page-locked
        host arrays; every copy is in flight before the one synchronisation."""
        self._refuse_planar()
        offs = np.asarray(seq_offsets, dtype=np.int64)
        missing = [r for r in self.robots if r not in qpos]
        if missing:
            raise KeyError(f"no qpos for {missing}")
        batches = []
        for r in self.robots:
            q = qpos[r]
            q = torch.from_numpy(np.ascontiguousarray(q)).to(self.device) if isinstance(q, np.ndarray) else q
            if offs.ndim != 1 or len(offs) < 2 or offs[0] != 0 or offs[-1] != int(q.shape[0]):
                raise ValueError("seq_offsets must span [0, N]")
            batches.append((q, offs))
        fps_list = list(fps) if isinstance(fps, (list, tuple, np.ndarray)) else [fps] * (len(offs) - 1)
        res = self.group.motion_epilogue(batches, height_adjust=height_adjust, root_origin_offset=root_origin_offset, ground_offset=ground_offset)
        hosts = []
        for arrays in res:
            host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in arrays]
            for h, t in zip(host, arrays):
                h.copy_(t, non_blocking=True)
            hosts.append(host)
        torch.cuda.current_stream(self.device).synchronize()
        out: Dict[str, List[Dict]] = {}
        for r, model, host in zip(self.robots, self.models, hosts):
            rp, rr, dp, lb = (h.numpy() for h in host)
            names = list(model.body_names)
            clips = []
            for s in range(len(offs) - 1):
                a, b = int(offs[s]), int(offs[s + 1])
                clips.append({"fps": fps_list[s], "root_pos": rp[a:b], "root_rot": rr[a:b], "dof_pos": dp[a:b],
                              "local_body_pos": lb[a:b], "link_body_list": names})
            out[r] = clips
        return out

    def tracking_from_qpos(self, qpos: Dict[str, torch.Tensor], seq_offsets: Sequence[int], fps, fps_out,
                           lowpass_hz=None, contact_bodies: Optional[Dict[str, Sequence[str]]] = None,
                           contact=None, lock_feet=False) -> Dict[str, List[Dict]]:
        """``dataset.tracking_from_qpos`` for every robot in one launch (``EngineGroup.motion_track``): ``qpos[robot]`` ``[N, nq]``
        float64 on the group's device, the same clips (at ``fps``: one rate or one per clip) for every robot -> ``{robot:
        [tracking dict per clip]}`` at ``fps_out``, the same keys, dtypes and arrays as the single-robot call.  ``lowpass_hz``:
        the cutoff of the zero-phase low-pass applied to qpos first (``None``: off); one value, or one per robot.
        ``contact_bodies``: ``{robot: [body names]}`` -- the contact labels of ``dataset.tracking_from_qpos`` for the robots it
        names, one ``Engine.motion_contacts`` launch per robot behind the shared export (there is no group entry); ``contact``:
        one ``dataset.ContactParams`` for all, or ``{robot: ContactParams}``.  ``lock_feet`` (only with ``contact_bodies``): the
        foot locking of ``dataset.tracking_from_qpos`` for the robots ``contact_bodies`` names, robot after robot in front of the
        shared export (there is no group entry); the low-pass of those robots then runs in front of it, per robot too."""
        from . import dataset
        from .engine import _report_names
        self._refuse_planar()
        offs = np.asarray(seq_offsets, dtype=np.int64)
        missing = [r for r in self.robots if r not in qpos]
        if missing:
            raise KeyError(f"no qpos for {missing}")
        contacts = locks = None
        if lock_feet and contact_bodies is None:
            raise ValueError("lock_feet needs contact_bodies: the bodies to lock")
        if contact_bodies is not None:
            unknown = [r for r in contact_bodies if r not in self.robots]
            if unknown:
                raise KeyError(f"contact_bodies names robots that are not solved here: {unknown}")
            for r, m in zip(self.robots, self.models):
                if r in contact_bodies:
                    dataset.contact_body_ids(m.body_names, contact_bodies[r])  # (an unknown name: before any launch)
        batches = []
        for r in self.robots:
            q = qpos[r]
            q = torch.from_numpy(np.ascontiguousarray(q)).to(self.device) if isinstance(q, np.ndarray) else q
            batches.append((q, offs, fps))
        if lock_feet:
            hz = list(lowpass_hz) if isinstance(lowpass_hz, (list, tuple, np.ndarray)) else [lowpass_hz] * len(self.robots)
            locks, left = [], []
            for i, (r, eng, m) in enumerate(zip(self.robots, self.group.engines, self.models)):
                if r not in contact_bodies:
                    locks.append(None)
                    left.append(0.0 if hz[i] is None else hz[i])
                    continue
                q, st, _ = dataset._smooth_and_lock(eng, m.body_names, batches[i][0], offs, fps, hz[i], contact_bodies[r],
                                                    contact.get(r) if isinstance(contact, dict) else contact, lock_feet)
                batches[i] = (q, offs, fps)
                locks.append(st)
                left.append(0.0)   # (filtered already)
            lowpass_hz = left
        res = self.group.motion_track(batches, fps_out, lowpass_hz=0.0 if lowpass_hz is None else lowpass_hz)
        if contact_bodies is not None:
            contacts = [dataset._track_contacts(eng, tr, m.body_names, contact_bodies[r], contact.get(r) if isinstance(contact, dict) else contact)
                        if r in contact_bodies else None for r, eng, m, tr in zip(self.robots, self.group.engines, self.models, res)]
        clips = dataset.tracks_to_host(res, fps_out, [m.body_names for m in self.models], [_report_names(cm)[1] for cm in self._cms],
                                       contacts=contacts, locks=locks)
        return dict(zip(self.robots, clips))

    def retarget_clips(self, pos, quat, body_names: Sequence[str], seq_offsets: Sequence[int], fps=30, height_adjust: bool = True,
                       root_origin_offset: bool = True, chunk=0, burn_in: int = 0, human_heights: Optional[Sequence[float]] = None,
                       clip_start: str = "qpos0", report: bool = False, track_fps: Optional[float] = None,
                       lowpass_hz: Optional[float] = None, contact_bodies: Optional[Dict[str, Sequence[str]]] = None, contact=None,
                       lock_feet=False, dynamics: bool = False, collision=None, mirror=False):
        """``dataset.retarget_clips`` for every robot: one solve (:meth:`retarget_batch`'s), then :meth:`motions_from_qpos` on the
        solved qpos, which stays on the device.  Returns ``{robot: [motion dict per clip]}``; each robot's clips feed
        ``dataset.MotionWriter.submit`` as they are.  With ``report`` a second value is returned: ``{robot: engine.ClipReport}``
        of the solved qpos (:meth:`clip_report`, solve counts included), host arrays.  With ``track_fps`` a last value is added:
        ``{robot: [tracking dict per clip]}`` at that rate (:meth:`tracking_from_qpos` on the same qpos).  With ``lowpass_hz``
        every robot's solved qpos is smoothed once (``dataset.smooth_qpos`` at ``fps``) and everything is made from that.
        ``contact_bodies`` / ``contact`` (with ``track_fps``): :meth:`tracking_from_qpos`'s contact labels; ``lock_feet``: its foot
        locking (the tracking dicts only).  With ``dynamics`` :meth:`dynamics_report` of the same qpos follows the clip reports (or
        the motions) and precedes the tracks.  With ``collision`` (``True`` or a dict of :meth:`self_collision_report`'s keywords)
        that report follows the dynamics reports (or what precedes them) and precedes the tracks.  With ``mirror`` (``True``, or a
        dict: ``about``, and ``plan`` as ``{robot: SymmetryPlan}``) the motions and the tracks are made from
        ``dataset.augment_mirror`` of every robot's qpos, one ``Engine.motion_mirror`` call per robot (the robots share no grid):
        twice the clips per robot, clip ``S + i`` the mirror image of clip ``i``; the reports stay those of the solved clips.  A
        robot whose symmetry plan is refused raises ``SymmetryError`` before any solve."""
        self._refuse_planar()
        mirror_kw = dict(mirror) if isinstance(mirror, dict) else {}
        plans = mirror_kw.pop("plan", None) or {}
        if mirror:
            plans = {r: plans[r] if plans.get(r) is not None else eng.symmetry_plan() for r, eng in zip(self.robots, self.group.engines)}
        if contact_bodies is not None and track_fps is None:
            raise ValueError("contact_bodies needs track_fps: the labels are made on the tracking export")
        if lock_feet and contact_bodies is None:
            raise ValueError("lock_feet needs contact_bodies: the bodies to lock")
        tpos = torch.from_numpy(np.ascontiguousarray(pos)) if isinstance(pos, np.ndarray) else pos
        tquat = torch.from_numpy(np.ascontiguousarray(quat)) if isinstance(quat, np.ndarray) else quat
        tpos, tquat = tpos.to(self.device), tquat.to(self.device)
        outs, offs = self._solve(tpos, tquat, body_names, seq_offsets, chunk, burn_in, False, True, human_heights, True, clip_start)
        if lowpass_hz:
            from .dataset import _smooth_qpos
            outs = [(_smooth_qpos(eng, q, offs, fps, lowpass_hz), it) for eng, (q, it) in zip(self.group.engines, outs)]
        reps = None
        if report:
            reps = self.clip_report({r: q for r, (q, _) in zip(self.robots, outs)}, tpos, tquat, body_names, offs, human_heights,
                                    iters={r: it for r, (_, it) in zip(self.robots, outs)})
        q_all, offs_all, fps_all = {r: q for r, (q, _) in zip(self.robots, outs)}, offs, fps
        if mirror:
            from .dataset import _augment_mirror
            for r, eng in zip(self.robots, self.group.engines):
                q_all[r], offs_all, fps_all = _augment_mirror(eng, q_all[r], offs, fps, plan=plans[r], **mirror_kw)
        motions = self.motions_from_qpos(q_all, offs_all, fps_all, height_adjust=height_adjust, root_origin_offset=root_origin_offset)
        res = (motions, {r: rep.numpy() for r, rep in reps.items()}) if report else (motions,)
        if dynamics:
            res += (self.dynamics_report({r: q for r, (q, _) in zip(self.robots, outs)}, offs, fps),)
        if collision:
            res += (self.self_collision_report({r: q for r, (q, _) in zip(self.robots, outs)}, offs,
                                               **(collision if isinstance(collision, dict) else {})),)
        if track_fps is not None:
            res += (self.tracking_from_qpos(q_all, offs_all, fps_all, track_fps,
                                            contact_bodies=contact_bodies, contact=contact, **({"lock_feet": lock_feet} if lock_feet else {})),)
        return res[0] if len(res) == 1 else res

    def dynamics_report(self, qpos: Dict[str, torch.Tensor], seq_offsets: Sequence[int], fps, lowpass_hz: float = 0.0, tables=None,
                        **dynamics_kwargs) -> Dict[str, Dict]:
        """``dataset.dynamics_report`` per robot: ``{robot: statistics}`` of ``{robot: qpos [N, nq]}`` on the device, one
        ``Engine.motion_dynamics`` call per member (the members share no grid).  ``tables``: ``{robot: InertialTable}`` instead of
        the ones read from the robots' MJCF files."""
        from .dataset import _dynamics_report
        self._refuse_planar()
        return {r: _dynamics_report(eng, qpos[r], seq_offsets, fps, lowpass_hz, (tables or {}).get(r), dynamics_kwargs)
                for r, eng in zip(self.robots, self.group.engines) if r in qpos}

    def self_collision_report(self, qpos: Dict[str, torch.Tensor], seq_offsets: Sequence[int], capsules=None, pairs=None,
                              margin: float = 0.0, radius: float = 0.03) -> Dict[str, Dict]:
        """``dataset.self_collision_report`` per robot: ``{robot: statistics}`` of ``{robot: qpos [N, nq]}`` on the device, one
        ``Engine.motion_self_collision`` call per member (the members share no grid).  ``capsules`` / ``pairs``: ``{robot: table}``
        instead of the skeletons' at ``radius`` (a convention, not measured on any robot)."""
        from .dataset import _self_collision_report
        return {r: _self_collision_report(eng, qpos[r], seq_offsets, (capsules or {}).get(r), (pairs or {}).get(r), margin, radius)
                for r, eng in zip(self.robots, self.group.engines) if r in qpos}

    def _solve(self, pos, quat, body_names, seq_offsets, chunk, burn_in, offset_to_ground, verify, human_heights, check, clip_start):
        """The solve of :meth:`retarget_batch`: per robot (qpos [N, nq] in the engine's layout, solves per frame) on the device, and
        the clip offsets."""
        from ._native import INIT_QPOS0, INIT_ROOT_TARGET
        from .schedule import make_items
        if clip_start not in ("qpos0", "root_target"):
            raise ValueError("clip_start must be 'qpos0' (the reference) or 'root_target'")
        clip_init = INIT_ROOT_TARGET if clip_start == "root_target" else INIT_QPOS0
        names = list(body_names)
        cols = [cm.slot_columns(names) for cm in self._cms]  # KeyError where the reference raises
        is_np = isinstance(pos, np.ndarray)
        if is_np and isinstance(quat, np.ndarray) and pos.ndim == 3:
            used = np.unique(np.concatenate(cols))
            if pos.shape[1] > len(used):
                # host arrays with more bodies than the robots consume: gather the used columns on the host first
                pos, quat = pos[:, used], quat[:, used]
                cols = [np.searchsorted(used, c).astype(np.int32) for c in cols]
        tpos = torch.from_numpy(np.ascontiguousarray(pos)) if is_np else pos
        tquat = torch.from_numpy(np.ascontiguousarray(quat)) if isinstance(quat, np.ndarray) else quat
        tpos, tquat = tpos.to(self.device).contiguous(), tquat.to(self.device).contiguous()
        N = int(tpos.shape[0])
        offs = np.asarray([0, N] if seq_offsets is None else seq_offsets, dtype=np.int64)
        if offs[0] != 0 or offs[-1] != N:
            raise ValueError("seq_offsets must span [0, N]")
        hs = [None] * len(self.robots)
        if human_heights is not None:
            hh = np.asarray(human_heights, dtype=np.float64)
            if hh.shape != (len(offs) - 1,):
                raise ValueError("human_heights must hold one height per clip")
            hs = [hh / cm.config.human_height_assumption / cm.ratio for cm in self._cms]
        if isinstance(chunk, str):
            if chunk != "auto":
                raise ValueError("chunk must be an integer or 'auto'")
            from .schedule import auto_chunk, group_chunk_offsets
            slots = 8 * torch.cuda.get_device_properties(self.device).multi_processor_count
            chunk, burn_in = auto_chunk(group_chunk_offsets([offs] * len(self.robots)), slots)
        prm = self._params(offset_to_ground)
        if chunk > 0 and verify:
            res = self.group.ik_solve_chunked([(tpos, tquat, c, offs) for c in cols], chunk, burn_in, params=prm, height_scales=hs,
                                              clip_init=clip_init)
            outs = [(q, it) for q, it, _ in res]
            infos = [info for _, _, info in res]
        else:
            items = [make_items(offs, chunk=chunk, burn_in=burn_in, height_scales=h, clip_init=clip_init) for h in hs]
            outs = self.group.ik_solve([(tpos, tquat, c, it) for c, it in zip(cols, items)], params=prm, launch_order="auto")
            infos = [{"chunks": len(it), "passes": 0, "resolved_frames": 0} for it in items]
        self.last_chunk_info = dict(zip(self.robots, infos))
        if check and N > 0:
            flags = torch.stack([torch.stack([(it >> 31).ne(0).any(), ((it >> 30) & 1).ne(0).any()]) for _, it in outs]).cpu().numpy()
            for r, bad in zip(self.robots, flags):
                if bad[0]:
                    raise FloatingPointError(f"{r}: retarget_batch produced non-finite qpos")
                if bad[1]:
                    raise RuntimeError(f"{r}: a box QP hit its iteration cap (the reference would assert on a failed QP)")
        return outs, offs
