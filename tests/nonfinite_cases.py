"""Non-finite qpos rows through the post-solve kernels: poison table, clip layout, dependency sets and an independent predictor.

gmr_ik_solve may hand on a qpos whose rows hold non-finite coordinates (bit 31 of iters_out, include/gmr_amd.h).  This module says,
for every kernel that takes such a qpos next, which output elements may change when ONE coordinate of ONE frame is replaced by
+NaN, -NaN, +inf or -inf -- twice, by two routes that share nothing:

  dep_*   the structural set, written from the contract text of include/gmr_amd.h and the joint tree alone: the outputs that are
          arithmetic functions of the poisoned coordinate.  Everything outside it must stay byte for byte what the clean input gives.
  pred_*  the same operation evaluated on the host with what the project already has (the C oracle's fk_kin / kin ops / fk_mj /
          stage_error, tests/rotation_edges.track_reference over numpy, plain numpy statements of the contract) on the poisoned
          input; ~isfinite of the result is the predicted mask.

Masks only are ever compared: never NaN against inf, never a NaN's payload or sign.

Where the two differ, the difference has a name (EXCEPTIONS) and a reason; tests/test_nonfinite_host.py asserts that they differ
nowhere else, tests/test_gpu_nonfinite_rows.py asserts the kernels against both.  No GPU and no torch device is needed here.
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

from gmr_amd.schedule import track_plan
from oracle.oracle import Oracle
from tests import rotation_edges as E
from tests.util import compiled

# ------------------------------------------------------------------ the poison values
BITS64 = {"+nan": 0x7FF8000000000000, "-nan": 0xFFF8000000000000, "+inf": 0x7FF0000000000000, "-inf": 0xFFF0000000000000}
BITS32 = {"+nan": 0x7FC00000, "-nan": 0xFFC00000, "+inf": 0x7F800000, "-inf": 0xFF800000}
VALUES = list(BITS64)


def value64(name):
    return np.array([BITS64[name]], dtype=np.uint64).view(np.float64)[0]


def value32(name):
    return np.array([BITS32[name]], dtype=np.uint32).view(np.float32)[0]


def f32(a):
    """THE dtype conversion of these tests: float64 host arrays are rounded by numpy and uploaded as they are."""
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------ the clip layout
TILE = 64         # frames per wavefront of fk_pos_kernel / motion_epilogue_kernel (kFkWave); fk_kernel takes two such wavefronts
TRACK_TILE = 62   # output frames per wavefront of motion_track_kernel (kTrackTile): 62 central lanes and a halo lane on each side
# a 37-frame clip, an empty one, a one-frame one, a 63-frame one whose first frame is in tile 0 and whose last in tile 1, and one
# of 209 frames that starts inside tile 1, holds tiles 2 and 3 whole and ends in the partial tile 4
OFFS = np.array([0, 37, 37, 38, 101, 310], dtype=np.int64)
N = int(OFFS[-1])
S = len(OFFS) - 1
FRAMES = {
    "first_of_all": 0,        # first frame of the first clip
    "one_frame_clip": 37,     # the clip [37, 38): its first, last and only frame
    "clip_first": 38,         # the GMR_MOTION_ROOT_ORIGIN frame of a clip that continues into the next tile
    "before_boundary": 100,   # a clip's last frame; the boundary 101 falls inside tile 1
    "after_boundary": 101,    # the next clip's first frame, same tile
    "middle": 150,
    "lane63": 191,            # last lane of tile 2 ...
    "lane0": 192,             # ... first lane of tile 3; both tiles lie inside the last clip
    "last_of_all": 309,       # last frame of the last clip, in a partial tile: the tile's dead lanes repeat it
}
TRACK_RATES = {"30to50": (30.0, 50.0), "120to30": (120.0, 30.0)}   # (fps_in, fps_out) of the existing tracking tests


def clip_of(frame):
    """The clip that holds global source frame `frame` (empty clips hold none)."""
    return int(np.searchsorted(OFFS, frame, side="right") - 1)


class Case(NamedTuple):
    value: str   # a key of BITS64
    coord: str   # a key of robot_tree(robot).cols
    frame: int   # global source frame


COORDS = ["root_x", "root_z", "root_qw", "first_hinge", "leaf_hinge"]


def _cases(frames):
    """One poisoned coordinate per case.  Every value x every coordinate at the middle frame; the root height -- the coordinate the
    per-clip minimum hangs on -- as +NaN and -NaN at every frame position; and at every other position one more coordinate as a
    +- pair (NaN and inf alternate), chosen so that root x sits on the clips' first frames."""
    mid = FRAMES["middle"]
    out = [Case(v, c, mid) for c in COORDS for v in VALUES]
    out += [Case(v, "root_z", f) for f in frames.values() if f != mid for v in ("+nan", "-nan")]
    extra = {"first_of_all": ("leaf_hinge", "nan"), "one_frame_clip": ("root_x", "inf"), "clip_first": ("root_x", "nan"),
             "before_boundary": ("first_hinge", "inf"), "after_boundary": ("root_qw", "nan"), "lane63": ("first_hinge", "nan"),
             "lane0": ("root_qw", "inf"), "last_of_all": ("leaf_hinge", "inf")}
    rot = [("root_x", "nan"), ("first_hinge", "inf"), ("root_qw", "nan"), ("root_z", "inf")]
    for i, (name, f) in enumerate(frames.items()):
        if f == mid:
            continue
        c, kind = extra.get(name, rot[i % len(rot)])
        out += [Case(s + kind, c, f) for s in "+-"]
    return list(dict.fromkeys(out))


TABLE = _cases(FRAMES)


# ------------------------------------------------------------------ the robots' trees
@functools.lru_cache(maxsize=None)
def robot_tree(robot):
    """What the dependency sets need of a robot: parents, the body of every hinge in qpos order, `below[j]` = the bodies strictly
    below body j, and the qpos columns of the poisoned coordinates: the first hinge of the tree and the hinge nearest a leaf --
    the last hinge with no hinge below it (in these robots every tip is a fixed body: a toe, a rubber hand, a finger tip)."""
    r = compiled("smplx", robot).robot
    nb = int(r.nbody)
    parent = np.asarray(r.parent, dtype=np.int64)
    dof_body = sorted((int(b) for b in r.hinge_bodies()), key=lambda b: int(r.qpos_adr[b]))
    below = np.zeros((nb, nb), dtype=bool)
    for j in range(1, nb):
        p = parent[j]
        while p >= 0:
            below[p, j] = True
            p = parent[p]
    leaves = [d for d, b in enumerate(dof_body) if not below[b][dof_body].any()]
    fixed = [j for j in range(1, nb) if j not in dof_body]
    cols = {"root_x": 0, "root_z": 2, "root_qw": 3, "first_hinge": 7, "leaf_hinge": 7 + leaves[-1]}
    return SimpleNamespace(name=robot, nb=nb, nq=int(r.nq), ndof=int(r.nq) - 7, parent=parent, dof_body=dof_body, below=below, cols=cols, fixed=fixed,
                           range=np.asarray(r.jnt_range, dtype=np.float64)[dof_body])


def oracle(robot):
    return _oracle(robot)


@functools.lru_cache(maxsize=None)
def _oracle(robot):
    return Oracle(compiled("smplx", robot).blob)


@functools.lru_cache(maxsize=None)
def _clean_qpos(robot):
    t = robot_tree(robot)
    rng = np.random.default_rng(20 + len(robot))
    lo = np.where(t.range[:, 0] < t.range[:, 1], t.range[:, 0], -1.0)
    hi = np.where(t.range[:, 0] < t.range[:, 1], t.range[:, 1], 1.0)
    q = np.empty((N, t.nq))
    q[:, :3] = rng.normal(size=(N, 3)) * [2.0, 2.0, 0.2] + [0.0, 0.0, 0.8]
    w = rng.normal(size=(N, 4))
    q[:, 3:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
    q[:, 7:] = rng.uniform(lo, hi, size=(N, t.ndof))
    q.setflags(write=False)
    return q


def clean_qpos(robot):
    """[N, nq] float64, read-only: hinges uniform within the joint ranges, unit root quaternions (wxyz), roots around a standing
    height -- every coordinate finite and away from zero, every frame different from its neighbours."""
    return _clean_qpos(robot)


def poisoned_qpos(robot, case):
    q = clean_qpos(robot).copy()
    q[case.frame, robot_tree(robot).cols[case.coord]] = value64(case.value)
    return q


def fk_inputs(q):
    """(root_pos, root_rot xyzw, dof) float32 of a qpos: what gmr_fk / gmr_fk_min_height take."""
    return f32(q[:, :3]), f32(q[:, [4, 5, 6, 3]]), f32(q[:, 7:])


@functools.lru_cache(maxsize=None)
def fitted_shape(robot):
    a = np.random.default_rng(5).uniform(0.8, 1.2, size=robot_tree(robot).nb).astype(np.float32)
    a.setflags(write=False)
    return a


def nonfinite(a):
    return ~np.isfinite(a)


# ------------------------------------------------------------------ exceptions: where a dependency set and the predictor may differ
EXCEPTIONS = {
    "inf_in_minimum": "low_s takes +-inf as values (include/gmr_amd.h): an infinite height changes the minimum only when it wins it, "
                      "so min_z_out and, with GMR_MOTION_HEIGHT_ADJUST, the other frames' z may stay finite",
    "unit_of_inf": "the slerp's r / |r| of an r with one infinite component is 0 in the three others (the contract's arithmetic): "
                   "only the poisoned component of a resampled root_rot row is non-finite",
    "rot_to_dof_select": "Joint.rot_to_dof's selects (torch_utils.quat_to_axis_angle: angle 0 where |xyz| > 1e-5 is false, the clamp "
                         "to the joint's range) give a finite angle for a NaN in xyz and for an infinite component; the reference's own",
    "rsqrt_of_inf": "gmr_evaluate normalises the root quaternion by a refined reciprocal square root of |q|^2, which is NaN at an infinite "
                    "norm (0 x inf): all four components of the root's xquat row are NaN where the oracle's q / |q| gives 0 in the "
                    "three finite ones (include/gmr_amd.h says so); every pose below and every error is NaN either way",
    "evaluate_rows": "gmr_evaluate's set is the frame's own rows; which poses and task errors of the frame depend on a coordinate "
                     "is the tree's and the task table's business, taken from the oracle",
}


def exception_for(call, case, output):
    """The name of the exception that lets `output` of `call` have a predicted mask smaller than its dependency set, or None."""
    inf = case.value.endswith("inf")
    if call in ("min_height", "epilogue") and inf and output in ("min_z", "root_pos"):
        return "inf_in_minimum"
    if call == "track" and inf and case.coord == "root_qw" and output in ("root_rot", "body_quat_w"):
        return "unit_of_inf"
    if call == "evaluate":
        return "evaluate_rows"
    if call == "rot_to_dof":
        return "rot_to_dof_select"
    return None


def listed_mask(call, case, output, predicted):
    """The mask a kernel must show for `output`: the predictor's, except where a listed exception says how the kernel differs from it
    (rsqrt_of_inf: the whole root row of xquat)."""
    if call == "evaluate" and output == "xquat" and case.coord == "root_qw" and case.value.endswith("inf"):
        m = predicted.copy()
        m[case.frame, 0] = True
        return m
    return predicted


# ------------------------------------------------------------------ FK (gmr_fk, gmr_fk_shape) and the per-clip minimum
def _fk_frame_dep(t, coord):
    """(pos [nb, 3], rot [nb, 4] xyzw) of one frame: the poses that are functions of `coord` of that frame."""
    pos, rot = np.zeros((t.nb, 3), dtype=bool), np.zeros((t.nb, 4), dtype=bool)
    if coord in ("root_x", "root_z"):
        pos[:, {"root_x": 0, "root_z": 2}[coord]] = True   # p_body = p_root + (a function of the rotations)
    elif coord == "root_qw":
        pos[1:] = True
        rot[0, 3] = True   # the root's row is a copy
        rot[1:] = True
    else:
        j = t.dof_body[t.cols[coord] - 7]
        pos[t.below[j]] = True   # p_j = p_parent + R_parent l_j: the hinge of j turns j, and moves only what hangs on it
        rot[j] = True
        rot[t.below[j]] = True
    return pos, rot


def dep_fk(robot, case):
    t = robot_tree(robot)
    pos, rot = np.zeros((N, t.nb, 3), dtype=bool), np.zeros((N, t.nb, 4), dtype=bool)
    pos[case.frame], rot[case.frame] = _fk_frame_dep(t, case.coord)
    return {"pos": pos, "rot": rot}


def pred_fk(robot, q, shape=None):
    bp, br = oracle(robot).fk_kin(*fk_inputs(q), want_rot=True, fitted_shape=shape)
    return {"pos": bp, "rot": br}


def dep_min_height(robot, case):
    t = robot_tree(robot)
    m = np.zeros(S, dtype=bool)
    m[clip_of(case.frame)] = _fk_frame_dep(t, case.coord)[0][:, 2].any()   # some body height of the clip is a function of it
    return {"min_z": m}


def clip_min(z):
    """torch.min's rule per clip over [N, nb] heights: NaN if any is NaN, +-inf as values; +inf for a clip without frames."""
    with np.errstate(invalid="ignore"):
        return np.array([np.min(z[a:b]) if b > a else np.inf for a, b in zip(OFFS[:-1], OFFS[1:])], dtype=np.float32)


def pred_min_height(robot, q):
    return {"min_z": clip_min(pred_fk(robot, q)["pos"][..., 2])}


# ------------------------------------------------------------------ the dataset epilogue
EPILOGUE_FLAGS = [(True, True), (True, False), (False, True), (False, False)]   # (height_adjust, root_origin_offset)
EPILOGUE_KEYS = ("root_pos", "root_rot", "dof_pos", "local_body_pos", "min_z")
GROUND = 0.05


def dep_epilogue(robot, case, height, origin):
    t = robot_tree(robot)
    f, c, s = case.frame, t.cols[case.coord], clip_of(case.frame)
    a, b = int(OFFS[s]), int(OFFS[s + 1])
    d = {"root_pos": np.zeros((N, 3), dtype=bool), "root_rot": np.zeros((N, 4), dtype=bool), "dof_pos": np.zeros((N, t.ndof), dtype=bool),
         "local_body_pos": np.zeros((N, t.nb, 3), dtype=bool)}
    if c < 3:
        d["root_pos"][f, c] = True
        if origin and f == a and c < 2:
            d["root_pos"][a:b, c] = True   # every frame of the clip loses the first frame's xy
    elif c < 7:
        d["root_rot"][f, (c - 3 + 3) & 3] = True   # wxyz column c - 3 -> xyzw
    else:
        d["dof_pos"][f, c - 7] = True
        d["local_body_pos"][f] = _fk_frame_dep(t, case.coord)[0]   # identity root: only the hinges reach it
    d.update(dep_min_height(robot, case))
    if height and d["min_z"][s]:
        d["root_pos"][a:b, 2] = True   # every frame of the clip is lowered by low_s
    return d


def pred_epilogue(robot, q, height, origin, ground=GROUND):
    """The epilogue's arrays as include/gmr_amd.h states them, in plain numpy over the oracle's FK."""
    orc = oracle(robot)
    rp32, rr32, dof32 = fk_inputs(q)
    ident = np.tile(np.array([[0, 0, 0, 1]], np.float32), (N, 1))
    local, _ = orc.fk_kin(np.zeros((N, 3), np.float32), ident, dof32, want_rot=False)
    body, _ = orc.fk_kin(rp32, rr32, dof32, want_rot=False)
    low = clip_min(body[..., 2])
    root_pos = q[:, :3].copy()
    with np.errstate(invalid="ignore"):
        for s in range(S):
            a, b = int(OFFS[s]), int(OFFS[s + 1])
            if b == a:
                continue
            if height:
                root_pos[a:b, 2] = (root_pos[a:b, 2] - np.float64(low[s])) + ground
            if origin:
                root_pos[a:b, :2] = root_pos[a:b, :2] - root_pos[a, :2].copy()
    return {"root_pos": root_pos, "root_rot": q[:, [4, 5, 6, 3]], "dof_pos": q[:, 7:], "local_body_pos": local, "min_z": low}


# ------------------------------------------------------------------ the tracking export
TRACK_KEYS = ("root_pos", "root_rot", "joint_pos", "root_lin_vel", "root_ang_vel", "joint_vel", "body_pos_w", "body_quat_w",
              "body_lin_vel_w", "body_ang_vel_w")


@functools.lru_cache(maxsize=None)
def plan(rate):
    """The resampling plan of OFFS at TRACK_RATES[rate], per global output frame: source rows src0 / src1 (global), weight a,
    in-clip neighbours km / kp (global) and step h, from the contract's formulas over schedule.track_plan's offsets."""
    fps_in, fps_out = TRACK_RATES[rate]
    out_offs, ratio = track_plan(OFFS, fps_in, fps_out)
    M = int(out_offs[-1])
    src0, src1, km, kp = (np.zeros(M, dtype=np.int64) for _ in range(4))
    a, h = np.zeros(M), np.zeros(M)
    for s in range(S):
        T, Ms = int(OFFS[s + 1] - OFFS[s]), int(out_offs[s + 1] - out_offs[s])
        for k in range(Ms):
            u = float(k) * float(ratio[s])
            i0 = min(int(np.floor(u)), T - 1)
            i1 = min(i0 + 1, T - 1)
            g = int(out_offs[s]) + k
            src0[g], src1[g], a[g] = OFFS[s] + i0, OFFS[s] + i1, (u - i0 if i1 > i0 else 0.0)
            km[g], kp[g] = out_offs[s] + max(k - 1, 0), out_offs[s] + min(k + 1, Ms - 1)
            h[g] = (kp[g] - km[g]) / fps_out
    return SimpleNamespace(fps_in=fps_in, fps_out=fps_out, out_offs=out_offs, ratio=ratio, M=M, src0=src0, src1=src1, a=a, km=km, kp=kp, h=h)


def track_reads(rate, frame):
    """Global output frames whose resampled rows read source frame `frame`: as i0, or as i1 with a weight above 0."""
    p = plan(rate)
    return (p.src0 == frame) | ((p.src1 == frame) & (p.a > 0))


def track_edges(rate):
    """The first two output-tile edges that lie inside a clip: global output frames g with g % TRACK_TILE == TRACK_TILE - 1 whose
    successor g + 1 -- the first central lane of the next tile -- belongs to the same clip."""
    p = plan(rate)
    clip = np.searchsorted(p.out_offs, np.arange(p.M), side="right") - 1
    return [g for g in range(TRACK_TILE - 1, p.M - 1, TRACK_TILE) if clip[g] == clip[g + 1]][:2]


@functools.lru_cache(maxsize=None)
def track_frames(rate):
    """FRAMES plus, for the tracking kernel's own tiling, the source frames read by the last central lane of an output tile and by
    the first central lane of the next (each is the other tile's halo lane), at the tile edges of track_edges."""
    p = plan(rate)
    fr = dict(FRAMES)
    for n, g in enumerate(track_edges(rate)):
        fr[f"edge{n}_last"], fr[f"edge{n}_first"] = int(p.src0[g]), int(p.src0[g + 1])
    return fr


@functools.lru_cache(maxsize=None)
def track_table(rate):
    return _cases(track_frames(rate))


def dep_track(robot, case, rate):
    t, p = robot_tree(robot), plan(rate)
    c = t.cols[case.coord]
    row = track_reads(rate, case.frame)                      # the resampled rows that are functions of the frame
    vel = (row[p.km] | row[p.kp]) & (p.h != 0)               # central differences: the rows k-1 and k+1 inside the clip
    copy = row & ((p.a == 0) | (p.src0 == p.src1))           # a = 0: the row is a copy of frame i0
    M = p.M
    d = {"root_pos": np.zeros((M, 3), bool), "root_rot": np.zeros((M, 4), bool), "joint_pos": np.zeros((M, t.ndof), bool),
         "root_lin_vel": np.zeros((M, 3), bool), "root_ang_vel": np.zeros((M, 3), bool), "joint_vel": np.zeros((M, t.ndof), bool),
         "body_pos_w": np.zeros((M, t.nb, 3), bool), "body_quat_w": np.zeros((M, t.nb, 4), bool),
         "body_lin_vel_w": np.zeros((M, t.nb, 3), bool), "body_ang_vel_w": np.zeros((M, t.nb, 3), bool)}
    pos, rot = _fk_frame_dep(t, case.coord)
    if c < 3:
        d["root_pos"][row, c] = True
        d["root_lin_vel"][vel, c] = True
    elif c < 7:
        d["root_rot"][row] = True                            # the slerp mixes the four components ...
        d["root_rot"][copy] = False
        d["root_rot"][copy, 3] = True                        # ... a copy does not
        d["root_ang_vel"][vel] = True
    else:
        d["joint_pos"][row, c - 7] = True
        d["joint_vel"][vel, c - 7] = True
    d["body_pos_w"][row] = pos
    d["body_quat_w"][row] = rot
    if c == 3:
        d["body_quat_w"][row & ~copy, 0] = True              # the root's row is the float32 cast of root_rot's
    d["body_lin_vel_w"][vel] = pos
    d["body_ang_vel_w"][vel] = rot.any(axis=1)[:, None]      # rotvec(q[kp] (x) conj(q[km])) mixes the components
    return d


def _ang_vel(pq, qq, h):
    """rotvec(p (x) conj(q)) / h for xyzw rows [..., 4] in float64, as include/gmr_amd.h writes it; 0 where h = 0."""
    with np.errstate(all="ignore"):
        pv, pw, qv, qw = pq[..., :3], pq[..., 3:], qq[..., :3], qq[..., 3:]
        w = pw * qw + (pv * qv).sum(-1, keepdims=True)
        v = qw * pv - pw * qv - np.cross(pv, qv)
        neg = w < 0
        w, v = np.where(neg, -w, w), np.where(neg, -v, v)
        n = np.sqrt((v * v).sum(-1, keepdims=True))
        f = np.where(n > 1e-12, 2.0 * np.arctan2(n, w) / n, 2.0)
        hh = np.reshape(h, h.shape + (1,) * (v.ndim - 1))
        return np.where(hh != 0, v * f / np.where(hh != 0, hh, 1.0), 0.0)


def pred_track(robot, q, rate):
    """The ten arrays by the contract: lerps and differences in numpy, the root's slerp and angular velocity by
    rotation_edges.track_reference over numpy float64, the body poses by the oracle's FK of the float32 casts."""
    p = plan(rate)
    with np.errstate(all="ignore"):
        x0, x1, a = q[p.src0], q[p.src1], p.a[:, None]
        lerp = np.where(a == 0, x0, x0 + a * (x1 - x0))
        root_rot, root_ang = E.track_reference(E.F64, q, OFFS, p.out_offs, p.ratio, p.fps_out)
        h = p.h[:, None]
        diff = lambda x: np.where(h != 0, (x[p.kp] - x[p.km]) / np.where(h != 0, h, 1.0), 0.0)   # noqa: E731
        root_pos, joint_pos = lerp[:, :3], lerp[:, 7:]
        bp, br = oracle(robot).fk_kin(f32(root_pos), f32(root_rot), f32(joint_pos), want_rot=True)
        bp64, br64 = bp.astype(np.float64), br.astype(np.float64)
        h3 = p.h[:, None, None]
        blin = np.where(h3 != 0, (bp64[p.kp] - bp64[p.km]) / np.where(h3 != 0, h3, 1.0), 0.0).astype(np.float32)
        bang = _ang_vel(br64[p.kp], br64[p.km], p.h).astype(np.float32)
        lin, jvel = diff(root_pos), diff(joint_pos)
    return {"root_pos": root_pos, "root_rot": root_rot, "joint_pos": joint_pos, "root_lin_vel": lin, "root_ang_vel": root_ang,
            "joint_vel": jvel, "body_pos_w": bp, "body_quat_w": br, "body_lin_vel_w": blin, "body_ang_vel_w": bang}


# ------------------------------------------------------------------ gmr_evaluate
EVAL_KEYS = ("err", "task_err", "xpos", "xquat")


@functools.lru_cache(maxsize=None)
def keypoints(robot):
    """Finite key-points for every frame of the layout: (pos [N, B, 3], quat [N, B, 4] float64, slot columns)."""
    from gmr_amd import synth
    cm = compiled("smplx", robot)
    pos, quat, names, _, _ = synth.synth_clips(cm, 1, N, seed=17, hard=True, dtype=np.float64)
    return pos, quat, cm.slot_columns(names)


def dep_evaluate(robot, case):
    t, cm = robot_tree(robot), compiled("smplx", robot)
    nt = len(cm.tasks[0]) + len(cm.tasks[1])
    d = {"err": np.zeros((N, 2), bool), "task_err": np.zeros((N, nt, 6), bool), "xpos": np.zeros((N, t.nb, 3), bool),
         "xquat": np.zeros((N, t.nb, 4), bool)}
    for v in d.values():
        v[case.frame] = True
    return d


def _eval_frame(robot, qf, f):
    cm, orc = compiled("smplx", robot), oracle(robot)
    pos, quat, sc = keypoints(robot)
    tp, tq = orc.prepare_targets(pos[f][sc], quat[f][sc])
    xp, xq = orc.fk_mj(qf)
    err, rows = np.zeros(2), []
    for tab in range(2):
        n, e = orc.stage_error(tab, qf, tp, tq, len(cm.tasks[tab]))
        err[tab] = n
        rows.append(e)
    return err, np.concatenate(rows), xp, xq


@functools.lru_cache(maxsize=None)
def _eval_clean(robot):
    q = clean_qpos(robot)
    return tuple(np.stack(x) for x in zip(*(_eval_frame(robot, q[f], f) for f in range(N))))


def pred_evaluate(robot, q):
    """The oracle's fk_mj and stage_error, frame by frame (its API is per frame): the frames that differ from the clean qpos are
    evaluated again, the others are the clean result."""
    out = [x.copy() for x in _eval_clean(robot)]
    clean = clean_qpos(robot)
    for f in np.nonzero((q.view(np.uint64) != clean.view(np.uint64)).any(axis=1))[0]:
        for o, x in zip(out, _eval_frame(robot, q[f], int(f))):
            o[f] = x
    return dict(zip(EVAL_KEYS, out))


# ------------------------------------------------------------------ the other KinematicsModel operators, poisoned in their own inputs
class OwnCase(NamedTuple):
    value: str
    where: tuple   # index into the op's input array after the frame: (dof,) / (row, component)
    frame: int


def _own_cases(wheres):
    """Every value at the middle frame, +-NaN at every frame position, for the first place; one value per frame, rotating, for the rest."""
    out = [OwnCase(v, w, FRAMES["middle"]) for w in wheres for v in VALUES]
    out += [OwnCase(v, wheres[0], f) for f in FRAMES.values() for v in ("+nan", "-nan")]
    for i, f in enumerate(FRAMES.values()):
        for k, w in enumerate(wheres[1:]):
            out.append(OwnCase(VALUES[(i + k) % 4], w, f))
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def kin_setup(robot, op):
    """(clean input float32 (read-only), cases) of one operator.  dof_to_rot reads the clean qpos' hinges, the other two the
    quaternions the oracle derives from them, so that every row is a proper, distinct rotation."""
    t, orc = robot_tree(robot), oracle(robot)
    dof = f32(clean_qpos(robot)[:, 7:])
    d0, d1 = 0, t.cols["leaf_hinge"] - 7
    if op == "dof_to_rot":
        x, wheres = dof, [(d0,), (d1,)]
    elif op == "rot_to_dof":
        x = orc.dof_to_rot(dof)
        wheres = [(t.dof_body[d0] - 1, 0), (t.dof_body[d0] - 1, 3), (t.dof_body[d1] - 1, 1), (t.fixed[-1] - 1, 0)]   # xyz, w, the last
        # hinge's, and the row of a body without a hinge, which no output reads
    else:
        x = np.concatenate([f32(clean_qpos(robot)[:, None, [4, 5, 6, 3]]), orc.dof_to_rot(dof)], axis=1)
        wheres = [(t.dof_body[d0], 0), (0, 3), (t.dof_body[d1], 2)]   # the first hinge's body, the root's row, a leaf
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x, _own_cases(wheres)


def kin_poisoned(robot, op, case):
    x = kin_setup(robot, op)[0].copy()
    x[(case.frame,) + case.where] = value32(case.value)
    return x


def dep_kin(robot, op, case):
    t = robot_tree(robot)
    f = case.frame
    if op == "dof_to_rot":
        d = np.zeros((N, t.nb - 1, 4), bool)
        d[f, t.dof_body[case.where[0]] - 1] = True   # axis sin, cos, renormalised: the whole quaternion of that hinge
    elif op == "rot_to_dof":
        d = np.zeros((N, t.ndof), bool)
        if case.where[0] + 1 in t.dof_body:
            d[f, t.dof_body.index(case.where[0] + 1)] = True
    else:
        j, comp = case.where
        d = np.zeros((N, t.nb, 4), bool)
        d[f, t.below[j]] = True
        if j == 0:
            d[f, 0, comp] = True   # row 0 is copied
        else:
            d[f, j] = True
    return {"out": d}


def pred_kin(robot, op, x):
    return {"out": getattr(oracle(robot), op)(x)}
