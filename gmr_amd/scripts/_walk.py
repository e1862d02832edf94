"""What both dataset scripts share: their common flags, which files to convert and where each result goes, and the batch -> pickles loop."""
from __future__ import annotations

import os
import re
from typing import Callable, List, Sequence, Tuple

import numpy as np


def natural_key(name: str):
    """natsort's default order for plain file names (scripts/smplx_to_robot_dataset.py:207 sorts with natsorted): digit runs compare as numbers."""
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def plan_files(src_folder: str, tgt_folder: str, want: Callable[[str], bool], src_ext: str, override: bool, natural: bool = False) -> Tuple[List[str], List[str], int]:
    """(sources, targets, skipped): every file below ``src_folder`` that ``want`` accepts, folder by folder in ``os.walk`` order with the
    names sorted (bvh_to_robot_dataset.py:59-60: ``sorted``; smplx_to_robot_dataset.py:206-207: ``natsorted``), its target
    ``path.replace(src_folder, tgt_folder).replace(src_ext, ".pkl")`` (:67, :212), left out when the target exists unless ``override`` (:69-71, :213)."""
    srcs, tgts, skipped = [], [], 0
    for dirpath, _, filenames in os.walk(src_folder):
        for filename in sorted(filenames, key=natural_key if natural else None):
            if not want(filename):
                continue
            s = os.path.join(dirpath, filename)
            t = s.replace(src_folder, tgt_folder).replace(src_ext, ".pkl")
            if os.path.exists(t) and not override:
                skipped += 1
                continue
            srcs.append(s)
            tgts.append(t)
    return srcs, tgts, skipped


def plan_robot_targets(srcs: Sequence[str], src_folder: str, tgt_folder: str, robots: Sequence[str], src_ext: str,
                       override: bool) -> Tuple[List[str], List[Tuple[str, ...]], int]:
    """``--robots``: robot r's target of a source is ``<tgt_folder>/<r>/<relative path>.pkl`` (``plan_files``'s rule with
    ``tgt_folder/r`` as the target folder).  A source is converted when any robot lacks its target, or with ``override``.
    Returns (sources, per-source tuples of targets in robot order, skipped)."""
    out_s, out_t, skipped = [], [], 0
    for s in srcs:
        ts = tuple(s.replace(src_folder, os.path.join(tgt_folder, r)).replace(src_ext, ".pkl") for r in robots)
        if not override and all(os.path.exists(t) for t in ts):
            skipped += 1
            continue
        out_s.append(s)
        out_t.append(ts)
    return out_s, out_t, skipped


def resolve_robots(ap, args, default: str = "unitree_g1") -> None:
    """``--robot`` xor ``--robots``: sets ``args.robot_list`` (the ``--robots`` names, or ``None``) and ``args.robot`` (its default
    when neither is given)."""
    if args.robots is not None and args.robot is not None:
        ap.error("--robot and --robots exclude each other")
    args.robot_list = None
    if args.robots is not None:
        names = [r.strip() for r in args.robots.split(",") if r.strip()]
        if not names:
            ap.error("--robots needs at least one robot name")
        if len(set(names)) != len(names):
            ap.error(f"--robots names a robot twice: {args.robots}")
        args.robot_list = names
    elif args.robot is None:
        args.robot = default


def plan(args, src_ext: str, want: Callable[[str], bool], natural: bool = False) -> Tuple[List[str], list, int]:
    """The sources to convert and their targets: one path each (``--robot``), or a tuple per source in ``--robots`` order."""
    if args.robot_list is None:
        return plan_files(args.src_folder, args.tgt_folder, want, src_ext, args.override, natural=natural)
    srcs, _, _ = plan_files(args.src_folder, args.tgt_folder, want, src_ext, True, natural=natural)
    return plan_robot_targets(srcs, args.src_folder, args.tgt_folder, args.robot_list, src_ext, args.override)


def hard_motion_names(paths: Sequence[str]) -> List[str]:
    """Motion names listed in the reference's ``assets/hard_motions/*.txt`` (``Motion: <path>, ...`` lines; smplx_to_robot_dataset.py:193-203)."""
    out = []
    for p in paths:
        if not os.path.exists(p):
            continue
        with open(p, "r") as f:
            for line in f:
                if "Motion:" not in line:
                    continue
                out.append(line.split(":")[1].strip().split(",")[0].strip().split(".")[0])
    return out


def add_common_flags(ap) -> None:
    ap.add_argument("--override", default=False, action="store_true")
    ap.add_argument("--device", default=None, type=int, help="GPU to use (default: LOCAL_RANK under torch.distributed.run, else 0)")
    ap.add_argument("--clip_start", default="qpos0", choices=["qpos0", "root_target"],
                    help="qpos0: the reference (every clip starts from the model's rest pose); root_target: start with the floating base on the first root target (not the reference's numbers for the first frames; spares clips that face away from qpos0 their slow start)")
    ap.add_argument("--use_velocity_limit", default=False, action="store_true", help="cap every limited hinge at 3 pi rad/s in each IK solve (the reference's use_velocity_limit: |dq| <= model timestep x limit per solve)")
    ap.add_argument("--velocity_limit", default=None, type=float, metavar="RAD_PER_S", help="cap every hinge at this rate instead (implies --use_velocity_limit)")
    ap.add_argument("--robots", default=None, type=str,
                    help="comma-separated robots solved together from each batch (MultiRobotRetargeting); robot r's files go to <tgt_folder>/<r>/...")
    ap.add_argument("--report_csv", default=None, type=str, help="write the per-clip quality report (stage and task errors, joint-limit and step statistics; one row per clip) to this CSV; with --robots one file per robot, <stem>.<robot><ext>; under --shard_by_rank one per rank, <stem>[.<robot>].rank<k><ext>")
    ap.add_argument("--hard_out", default=None, type=str, help="write the clips that exceed --max_pos_err / --max_dof_step as a hard-motion list (the format --hard_motions reads); with --robots one file per robot, under --shard_by_rank one per rank (named like --report_csv)")
    ap.add_argument("--max_pos_err", default=None, type=float, help="metres: a clip whose largest task position error exceeds this is not written and is listed in --hard_out")
    ap.add_argument("--dynamics_csv", default=None, type=str, help="write the per-clip inverse-dynamics statistics (frames over a torque limit, ground-reaction ratios, unloaded and non-finite frames, the worst joint and its torque ratio; one row per clip) to this CSV, named like --report_csv; needs the robot's MJCF file (GMR_ROOT) for masses and torque limits")
    ap.add_argument("--max_torque_ratio", default=None, type=float, help="a clip in which some joint needs more than this many times its torque limit is not written and is listed in --hard_out (with the clip report's difficulty: this flag computes the clip report too; --dynamics_csv alone does not)")
    ap.add_argument("--collision_csv", default=None, type=str, help="write the per-clip self-collision statistics (smallest clearance and deepest penetration of the capsule proxies, its frame and pair, colliding frames and their longest run; one row per clip) to this CSV, named like --report_csv")
    ap.add_argument("--max_penetration", default=None, type=float, metavar="M", help="metres: a clip whose capsule proxies penetrate each other deeper than this is not written and is listed in --hard_out (with the clip report's difficulty: this flag computes the clip report too; --collision_csv alone does not)")
    ap.add_argument("--collision_radius", default=None, type=float, metavar="R", help="radius of the default proxies, capsules along the skeleton's links (default 0.03 m, a convention, not measured on any robot; the skeleton is not the robot's collision geometry)")
    ap.add_argument("--collision_proxies", default=None, type=str, metavar="FILE.json", help="capsules (and optionally pairs) from this file instead of the skeleton's (gmr_amd.collision.save_proxies writes one); with --robots: robot:file;robot2:file2")
    ap.add_argument("--max_dof_step", default=None, type=float, help="radians: a clip whose largest joint step between consecutive frames exceeds this is not written and is listed in --hard_out")
    ap.add_argument("--track_fps", default=None, type=float, help="with --track_folder: also write every clip's tracking export (resampled root, joints and world body poses with their velocities, dataset.tracking_from_qpos) at this rate")
    ap.add_argument("--track_folder", default=None, type=str, help="with --track_fps: where the tracking exports go, <track_folder>/<relative path>.npz (with --robots <track_folder>/<robot>/...); the pickles are unchanged")
    ap.add_argument("--lowpass_hz", default=None, type=float, metavar="HZ", help="smooth the solved qpos once with a zero-phase 2nd-order Butterworth low-pass at this cutoff (dataset.smooth_qpos, on the GPU) before the report, the pickles and the tracking exports are made; default: off")
    ap.add_argument("--contact_bodies", default=None, type=str, metavar="A,B", help="with --track_fps: label these bodies' contact with the ground on every tracking export (contact, contact_stats, airborne_frames in the .npz; dataset.tracking_from_qpos); with --robots: robot:a,b;robot2:c,d")
    ap.add_argument("--contact_height_on", default=None, type=float, metavar="M", help="a body enters contact at or below this height above the clip's lowest contact height (default 0.03, a convention, not measured on any robot)")
    ap.add_argument("--contact_height_off", default=None, type=float, metavar="M", help="... and leaves it above this height (default 0.05)")
    ap.add_argument("--contact_speed_on", default=None, type=float, metavar="M_PER_S", help="a body enters contact at or below this speed (default 0.3)")
    ap.add_argument("--contact_speed_off", default=None, type=float, metavar="M_PER_S", help="... and leaves it above this speed (default 0.6)")
    ap.add_argument("--lock_feet", default=False, action="store_true", help="with --contact_bodies: remove the foot slide of those bodies from qpos before the tracking exports are made (dataset.lock_feet, on the GPU; the .npz gain footlock_stats_*); the pickles are unchanged; default: off")
    ap.add_argument("--mirror", default=False, action="store_true", help="also write the left-right mirrored copy of every clip, X_mirror.pkl beside X.pkl (and X_mirror.npz beside a tracking export), made on the GPU from the solved qpos (dataset.augment_mirror) with the same post-processing; a robot that is not symmetric within 1e-3 (gmr_amd.symmetry.plan_symmetry) ends the run before any file is read; the reports stay those of the solved clips; default: off")
    ap.add_argument("--mirror_about", default="start", choices=["world", "start"], help="with --mirror: reflect in the world plane y = 0 (world), or each clip in the vertical plane through its first root position along its heading, so that the mirrored clip starts where the original does (start, the default)")
    ap.add_argument("--mirror_plan", default=None, type=str, metavar="FILE.json", help="with --mirror: the symmetry plan from this file (gmr_amd.symmetry.save_plan writes one) instead of the robot's own; with --robots: robot:file;robot2:file2")
    ap.add_argument("--retime_to_limits", nargs="?", const=True, default=None, type=float, metavar="RAD_PER_S", help="play every solved clip slower exactly where a hinge turns faster than its velocity limit (dataset.retime_to_limits, on the GPU: a monotone time warp, resampled at the clip's rate) before the pickles, the dynamics and collision reports and the tracking exports are made; the clip report stays that of the solved clips; with a number: that limit on every hinge; without: the retargeter's limits (--use_velocity_limit / --velocity_limit), else 3 pi rad/s on every limited hinge; not with --robots; default: off")
    ap.add_argument("--retime_to_torque", nargs="?", const=True, default=None, type=float, metavar="SCALE", help="play every solved clip slower exactly where a hinge needs more torque than its actuator has (dataset.retime_to_torque_limits, on the GPU: inverse dynamics, a time warp and a cubic resampling, up to four passes), after --lowpass_hz and --retime_to_limits and before the pickles, the dynamics and collision reports and the tracking exports are made; with a number: the share of the MJCF torque limits the warp is planned against (default 0.95, a convention, not measured on a robot); torques of unfiltered qpos are noise: give --lowpass_hz; not with --robots; default: off")
    ap.add_argument("--resolve_collisions", default=False, action="store_true", help="push the colliding capsule proxies of every solved clip apart (dataset.resolve_self_collisions, on the GPU: 16 damped passes per frame over the hinges between the two capsules, steps of at most 0.2 rad -- conventions, not measured on a robot) after --lowpass_hz and the retiming and before the pickles, the dynamics and collision reports, the foot locking and the tracking exports are made; the clip report stays that of the solved clips; takes --collision_radius and --collision_proxies as --collision_csv does; not with --robots; default: off")
    ap.add_argument("--shard_by_rank", default=False, action="store_true", help="under torch.distributed.run: convert files[RANK::WORLD_SIZE] only (no exchange between ranks)")


def resolve_track(ap, args) -> None:
    """``--track_fps`` and ``--track_folder`` come together, and the rate is positive."""
    if (args.track_fps is None) != (args.track_folder is None):
        ap.error("--track_fps and --track_folder go together")
    if args.track_fps is not None and not args.track_fps > 0:
        ap.error("--track_fps must be positive")
    if getattr(args, "lowpass_hz", None) is not None and not args.lowpass_hz > 0:
        ap.error("--lowpass_hz must be positive")
    retime = getattr(args, "retime_to_limits", None)
    if retime is not None and retime is not True and not retime > 0:
        ap.error("--retime_to_limits must be positive")
    if retime is not None and getattr(args, "robots", None):
        ap.error("--retime_to_limits is not available with --robots")
    torque = getattr(args, "retime_to_torque", None)
    if torque is not None and torque is not True and not 0.0 < torque <= 1.0:
        ap.error("--retime_to_torque must lie in (0, 1]")
    if torque is not None and getattr(args, "robots", None):
        ap.error("--retime_to_torque is not available with --robots")
    if getattr(args, "resolve_collisions", False) and getattr(args, "robots", None):
        ap.error("--resolve_collisions is not available with --robots")
    resolve_contact(ap, args)
    resolve_mirror(ap, args)


def mirror_path(target: str) -> str:
    """Where the mirrored copy of a clip goes: ``X_mirror.pkl`` beside ``X.pkl``."""
    root, ext = os.path.splitext(target)
    return root + "_mirror" + ext


def resolve_mirror(ap, args) -> None:
    """``--mirror``: plans every robot's symmetry on the host, before a file is read or a GPU is touched, and ends the run with the
    ``SymmetryError`` text for a robot that is refused.  Sets ``args.mirror_kw``: the ``mirror`` argument of ``retarget_clips``
    (empty without the flag: nothing changes then)."""
    args.mirror_kw = {}
    spec = getattr(args, "mirror_plan", None)
    if not getattr(args, "mirror", False):
        if spec is not None:
            ap.error("--mirror_plan needs --mirror")
        return
    from .. import params
    from ..mjcf import load_robot
    from ..symmetry import SymmetryError, load_plan, plan_symmetry
    robots = getattr(args, "robot_list", None)
    files = {}
    if spec is not None and robots is None:
        files[args.robot] = spec
    elif spec is not None:
        for part in (p for p in spec.split(";") if p.strip()):
            r, sep, path = part.partition(":")
            if not sep or r.strip() not in robots or r.strip() in files:
                ap.error("--mirror_plan with --robots takes robot:file;robot2:file2, each robot one of --robots and named once")
            files[r.strip()] = path.strip()
    plans = {}
    for r in (robots if robots is not None else [args.robot]):
        if r not in params.ROBOT_XML_DICT:
            ap.error(f"--mirror: unknown robot {r!r}")
        try:
            model = load_robot(params.ROBOT_XML_DICT[r], name=r)
            plans[r] = load_plan(files[r]) if r in files else plan_symmetry(model)
            plans[r].check_robot(model)
        except (SymmetryError, NotImplementedError) as e:
            ap.error(f"--mirror: {e}")
    args.mirror_kw = {"mirror": {"about": args.mirror_about, "plan": plans if robots is not None else plans[args.robot]}}


_CONTACT_THRESHOLDS = ("height_on", "height_off", "speed_on", "speed_off")


def resolve_contact(ap, args) -> None:
    """``--contact_bodies`` needs ``--track_fps``; sets ``args.contact_kw``: the ``contact_bodies`` / ``contact`` arguments of
    ``retarget_clips`` (empty without the flag: nothing changes then).  One robot: ``a,b``; ``--robots``: ``robot:a,b;robot2:c,d``."""
    args.contact_kw = {}
    given = [k for k in _CONTACT_THRESHOLDS if getattr(args, "contact_" + k, None) is not None]
    spec = getattr(args, "contact_bodies", None)
    if spec is None:
        if given:
            ap.error("--contact_" + given[0] + " needs --contact_bodies")
        if getattr(args, "lock_feet", False):
            ap.error("--lock_feet needs --contact_bodies")
        return
    if args.track_fps is None:
        ap.error("--contact_bodies is only valid with --track_fps")
    names = lambda text: [n.strip() for n in text.split(",") if n.strip()]
    robots = getattr(args, "robot_list", None)
    if robots is None:
        if ":" in spec or ";" in spec:
            ap.error("--contact_bodies takes a,b for one robot (robot:a,b;robot2:c,d goes with --robots)")
        bodies = names(spec)
        if not bodies:
            ap.error("--contact_bodies needs at least one body name")
    else:
        bodies = {}
        for part in (p for p in spec.split(";") if p.strip()):
            robot, sep, rest = part.partition(":")
            robot = robot.strip()
            if not sep or robot not in robots or robot in bodies or not names(rest):
                ap.error("--contact_bodies with --robots takes robot:a,b;robot2:c,d, each robot one of --robots and named once")
            bodies[robot] = names(rest)
        if not bodies:
            ap.error("--contact_bodies needs at least one robot:a,b group")
    from ..dataset import ContactParams
    prm = ContactParams(**{k: getattr(args, "contact_" + k) for k in given})
    if not (prm.height_on <= prm.height_off and 0 <= prm.speed_on <= prm.speed_off):
        ap.error("--contact_height_on <= --contact_height_off and 0 <= --contact_speed_on <= --contact_speed_off are required")
    args.contact_kw = {"contact_bodies": bodies, "contact": prm}
    if getattr(args, "lock_feet", False):  # (absent without the flag: nothing changes then)
        args.contact_kw["lock_feet"] = True


def track_path(args, target: str) -> str:
    """The tracking export beside a clip's pickle: the pickle's path below ``--tgt_folder``, moved below ``--track_folder``, as ``.npz``."""
    return os.path.join(args.track_folder, os.path.splitext(os.path.relpath(target, args.tgt_folder))[0] + ".npz")


def wants_report(args) -> bool:
    """Whether the clip report is needed: one of its own flags is given, or ``--max_torque_ratio`` / ``--max_penetration``, whose
    clips go to the hard list with the clip report's difficulty.  ``--dynamics_csv`` or ``--collision_csv`` alone does not compute it."""
    return any(getattr(args, k, None) is not None for k in ("report_csv", "hard_out", "max_pos_err", "max_dof_step", "max_torque_ratio", "max_penetration"))


def wants_dynamics(args) -> bool:
    """Whether the inverse-dynamics statistics are asked for."""
    return any(getattr(args, k, None) is not None for k in ("dynamics_csv", "max_torque_ratio"))


def wants_collision(args) -> bool:
    """Whether the self-collision statistics are asked for."""
    return any(getattr(args, k, None) is not None for k in ("collision_csv", "max_penetration"))


def collision_kw(args, model=None) -> dict:
    """The ``collision`` argument of ``retarget_clips`` from the flags ({} without them: nothing changes then).  ``model``: the
    ``RobotModel`` (a proxies file may name bodies), or with ``--robots`` ``{robot: RobotModel}``: the tables are then
    ``{robot: table}`` and ``--collision_proxies`` reads ``robot:file;robot2:file2``."""
    if not wants_collision(args):
        return {}
    from ..collision import load_proxies
    kw = {}
    if getattr(args, "collision_radius", None) is not None:
        kw["radius"] = args.collision_radius
    spec = getattr(args, "collision_proxies", None)
    if spec is not None:
        if isinstance(model, dict):   # --robots
            caps, prs = {}, {}
            for part in (p for p in spec.split(";") if p.strip()):
                r, sep, path = part.partition(":")
                if not sep or r.strip() not in model:
                    raise ValueError("--collision_proxies with --robots takes robot:file;robot2:file2, each robot one of --robots")
                caps[r.strip()], pr = load_proxies(path.strip(), model[r.strip()])
                if pr is not None:
                    prs[r.strip()] = pr
            kw.update(capsules=caps, pairs=prs)
        else:
            caps, pr = load_proxies(spec, model)
            kw.update(capsules=caps, pairs=pr)
    return {"collision": kw or True}


def resolve_collisions_kw(args, model=None) -> dict:
    """The ``resolve_collisions`` argument of ``retarget_clips`` from the flags ({} without ``--resolve_collisions``: nothing changes
    then): ``--collision_radius`` and ``--collision_proxies`` as ``collision_kw`` reads them."""
    if not getattr(args, "resolve_collisions", False):
        return {}
    from ..collision import load_proxies
    kw = {}
    if getattr(args, "collision_radius", None) is not None:
        kw["radius"] = args.collision_radius
    if getattr(args, "collision_proxies", None) is not None:
        caps, pr = load_proxies(args.collision_proxies, model)
        kw.update(capsules=caps, pairs=pr)
    return {"resolve_collisions": kw or True}


def wants_sink(args) -> bool:
    return wants_report(args) or wants_dynamics(args) or wants_collision(args)


def report_path(path: str, robot=None, rank=None) -> str:
    """Where one writer's share of ``--report_csv`` / ``--hard_out`` goes: ``<stem>[.<robot>][.rank<k>]<ext>``.  Every robot of
    ``--robots`` and, under ``--shard_by_rank``, every rank writes files of its own, so none overwrites another's."""
    stem, ext = os.path.splitext(path)
    return stem + (f".{robot}" if robot is not None else "") + (f".rank{rank}" if rank is not None else "") + ext


class ReportSink:
    """One robot's clip reports of a run, batch by batch: the CSV rows and the hard list are on disk as soon as their batch is
    solved (a run that dies leaves what it had), the withheld clips are counted."""

    def __init__(self, args, robot=None, rank=None):
        self.args = args
        self.csv = report_path(args.report_csv, robot, rank) if args.report_csv else None
        self.hard = report_path(args.hard_out, robot, rank) if args.hard_out else None
        self.dyn_csv = report_path(args.dynamics_csv, robot, rank) if getattr(args, "dynamics_csv", None) else None
        self.col_csv = report_path(args.collision_csv, robot, rank) if getattr(args, "collision_csv", None) else None
        self.withheld, self._started = 0, False

    def take(self, dataset, targets: Sequence[str], motions: list, report, dynamics=None, collision=None):
        """One batch: returns the (motions, targets) that are to be written.  ``dynamics``: the batch's ``dynamics_report``;
        ``collision``: its ``self_collision_report``."""
        names = [os.path.splitext(os.path.basename(t))[0] for t in targets]
        mask = dataset.report_hard_mask(report, self.args.max_pos_err, self.args.max_dof_step) if report is not None else np.zeros(len(names), dtype=bool)
        if dynamics is not None:
            if getattr(self.args, "max_torque_ratio", None) is not None:
                mask |= dataset.dynamics_hard_mask(dynamics, self.args.max_torque_ratio)
            if self.dyn_csv:
                dataset.write_dynamics_csv(self.dyn_csv, names, dynamics, append=self._started)
        if collision is not None:
            if getattr(self.args, "max_penetration", None) is not None:
                mask |= dataset.collision_hard_mask(collision, self.args.max_penetration)
            if self.col_csv:
                dataset.write_collision_csv(self.col_csv, names, collision, append=self._started)
        if self.csv and report is not None:
            dataset.write_report_csv(self.csv, names, report, append=self._started)
        if self.hard and report is not None:
            dataset.write_hard_list(self.hard, names, report, mask, append=self._started)
        self._started = True
        self.withheld += int(mask.sum())
        return [m for m, h in zip(motions, mask) if not h], [t for t, h in zip(targets, mask) if not h]

    def close(self):
        if self.withheld:
            print(f"{self.withheld} clips withheld (--max_pos_err / --max_dof_step / --max_torque_ratio / --max_penetration)" + (f", listed in {self.hard}" if self.hard else ""))


def convert(args, pairs: List[Tuple[str, str]], src_human: str, batches: Callable, retarget_kw: Callable, workers: int, done: str) -> int:
    """This rank's share of the (source, target) pairs -> pickles: ``batches(sources, columns)`` yields the loader's batches, each one
    goes through ``dataset.retarget_clips(..., **retarget_kw(batch))`` and to the writer pool; files that could not be loaded are
    reported and counted like the reference's ``except: print; continue``."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if args.device is None:
        args.device = int(os.environ.get("LOCAL_RANK", "0"))
    args.report_rank = None
    if args.shard_by_rank and world > 1:
        pairs = pairs[rank::world]
        args.report_rank = rank  # every rank writes report files of its own (report_path)
        print(f"rank {rank} of {world}: {len(pairs)} of them")
    if pairs and getattr(args, "robot_list", None):
        return _convert_robots(args, pairs, src_human, batches, retarget_kw, workers, done)
    if pairs:
        from .. import GeneralMotionRetargeting as GMR, dataset
        g = GMR(src_human=src_human, tgt_robot=args.robot, device=args.device, use_velocity_limit=args.use_velocity_limit, velocity_limits=args.velocity_limit)
        target_of, failed = dict(pairs), 0
        sink = ReportSink(args, rank=args.report_rank) if wants_sink(args) else None
        rep_on = wants_report(args)
        track_fps = getattr(args, "track_fps", None)
        track_kw = {}if track_fps is None else {"track_fps": track_fps}  # (absent without the flags: nothing changes then)
        if getattr(args, "lowpass_hz", None) is not None:
            track_kw["lowpass_hz"] = args.lowpass_hz
        track_kw.update(getattr(args, "contact_kw", {}))
        dyn_kw = {"dynamics": True} if wants_dynamics(args) else {}  # (absent without the flags: nothing changes then)
        col_kw = collision_kw(args, model=g.model) if wants_collision(args) else {}  # (ditto)
        mir_kw = getattr(args, "mirror_kw", {})  # (ditto)
        ret_kw = {} if getattr(args, "retime_to_limits", None) is None else {"retime": args.retime_to_limits}  # (ditto)
        if getattr(args, "retime_to_torque", None) is not None:
            ret_kw["retime_torque"] = args.retime_to_torque
        if getattr(args, "resolve_collisions", False):
            ret_kw.update(resolve_collisions_kw(args, model=g.model))
        with dataset.MotionWriter(workers=max(1, workers), override=True) as writer:
            for batch in batches([s for s, _ in pairs], g.ik_columns):
                for f, why in batch.skipped:
                    print(f"Error loading {f}: {why}")
                    failed += 1
                if not len(batch):
                    continue
                targets = [target_of[f] for f in batch.files]
                res = dataset.retarget_clips(g, batch.pos, batch.quat, batch.body_names, batch.seq_offsets, human_heights=batch.human_heights,
                                             clip_start=args.clip_start, report=rep_on, **retarget_kw(batch), **track_kw, **dyn_kw, **col_kw, **mir_kw, **ret_kw)
                res = res if isinstance(res, tuple) else (res,)
                S = len(targets)
                motions, mirror_of = res[0][:S], dict(zip(targets, res[0][S:]))  # (with --mirror clip S + i is the mirror of clip i)
                track_of = dict(zip(targets, res[-1][:S])) if track_fps is not None else None
                track_mirror_of = dict(zip(targets, res[-1][S:])) if track_fps is not None else {}
                if sink is not None:
                    motions, targets = sink.take(dataset, targets, motions, res[1] if rep_on else None, res[1 + rep_on] if dyn_kw else None,
                                                 res[1 + rep_on + bool(dyn_kw)] if col_kw else None)
                writer.submit(motions, targets)
                if track_of is not None:  # (a withheld clip has no tracking export either)
                    writer.submit([track_of[t] for t in targets], [track_path(args, t) for t in targets])
                if mirror_of:  # (nor a mirrored copy)
                    writer.submit([mirror_of[t] for t in targets], [mirror_path(t) for t in targets])
                if track_mirror_of:
                    writer.submit([track_mirror_of[t] for t in targets], [mirror_path(track_path(args, t)) for t in targets])
        if sink is not None:
            sink.close()
        print(f"{writer.written} files written, {failed} could not be loaded")
    print(done, args.tgt_folder)
    return 0


def _convert_robots(args, pairs, src_human: str, batches: Callable, retarget_kw: Callable, workers: int, done: str) -> int:
    """``convert`` for ``--robots``: each batch is loaded once and solved for every robot (``MultiRobotRetargeting.retarget_clips``);
    a target that exists already is skipped by the writer unless ``--override``."""
    from .. import MultiRobotRetargeting, dataset
    mr = MultiRobotRetargeting(src_human, args.robot_list, device=args.device, use_velocity_limit=args.use_velocity_limit, velocity_limits=args.velocity_limit)
    target_of, failed = dict(pairs), 0
    sinks = {r: ReportSink(args, r, getattr(args, "report_rank", None)) for r in mr.robots} if wants_sink(args) else None
    rep_on = wants_report(args)
    track_fps = getattr(args, "track_fps", None)
    track_kw = {} if track_fps is None else {"track_fps": track_fps}  # (absent without the flags: nothing changes then)
    if getattr(args, "lowpass_hz", None) is not None:
        track_kw["lowpass_hz"] = args.lowpass_hz
    track_kw.update(getattr(args, "contact_kw", {}))
    dyn_kw = {"dynamics": True} if wants_dynamics(args) else {}
    col_kw = collision_kw(args, model=dict(zip(mr.robots, mr.models))) if wants_collision(args) else {}
    mir_kw = getattr(args, "mirror_kw", {})
    with dataset.MotionWriter(workers=max(1, workers), override=args.override) as writer:
        for batch in batches([s for s, _ in pairs], mr.ik_columns):
            for f, why in batch.skipped:
                print(f"Error loading {f}: {why}")
                failed += 1
            if not len(batch):
                continue
            res = mr.retarget_clips(batch.pos, batch.quat, batch.body_names, batch.seq_offsets, human_heights=batch.human_heights,
                                    clip_start=args.clip_start, report=rep_on, **retarget_kw(batch), **track_kw, **dyn_kw, **col_kw, **mir_kw)
            res = res if isinstance(res, tuple) else (res,)
            motions, reps = res[0], res[1] if rep_on else None
            dyns = res[1 + rep_on] if dyn_kw else None
            cols = res[1 + rep_on + bool(dyn_kw)] if col_kw else None
            for i, r in enumerate(mr.robots):
                ts = [target_of[f][i] for f in batch.files]
                S = len(ts)
                ms, mirror_of = motions[r][:S], dict(zip(ts, motions[r][S:]))  # (with --mirror clip S + i is the mirror of clip i)
                track_of = dict(zip(ts, res[-1][r][:S])) if track_fps is not None else None
                track_mirror_of = dict(zip(ts, res[-1][r][S:])) if track_fps is not None else {}
                if sinks is not None:
                    ms, ts = sinks[r].take(dataset, ts, ms, reps[r] if reps is not None else None, dyns[r] if dyns is not None else None,
                                             cols[r] if cols is not None else None)
                writer.submit(ms, ts)
                if track_of is not None:
                    writer.submit([track_of[t] for t in ts], [track_path(args, t) for t in ts])
                if mirror_of:
                    writer.submit([mirror_of[t] for t in ts], [mirror_path(t) for t in ts])
                if track_mirror_of:
                    writer.submit([track_mirror_of[t] for t in ts], [mirror_path(track_path(args, t)) for t in ts])
    if sinks is not None:
        for sink in sinks.values():
            sink.close()
    print(f"{writer.written} files written, {failed} could not be loaded")
    print(done, args.tgt_folder)
    return 0
