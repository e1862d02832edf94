"""The left-right symmetry plan of a robot for mirror augmentation (``Engine.motion_mirror``, ``gmr_motion_mirror``): which body
is the mirror image of which, and from it the permutation and signs of the hinge columns of qpos.  Host only, numpy only.

"Symmetric" is a property of the kinematic tree in its rest pose (root at the origin with identity rotation, every hinge at 0),
under the reflection ``M = diag(1, -1, 1)`` in the root's own xz-plane: body ``c`` with world position ``X0[c]`` and world hinge
axis ``W[c]`` is the image of ``d`` when ``M X0[c] = X0[d]`` and ``W[d] = -+ M W[c]``.  A reflection turns a rotation about ``w`` by
``theta`` into one about ``-M w`` by ``theta``, so ``W[d] = -M W[c]`` copies the angle (``sign = +1``) and ``W[d] = M W[c]`` negates
it.  Real robots meet this only up to the digits of their model files, and some not at all: ``plan_symmetry`` pairs within
tolerances -- conventions, 1e-3 in metres, in axis components and in radians -- and refuses a robot (``SymmetryError``) rather
than produce a plausible but wrong motion.  Masses, geometry and actuators are not looked at.  Nothing is ever clamped to a range.

A plan travels as a plain JSON dict (``SymmetryPlan.to_json`` / ``from_json``, ``save_plan`` / ``load_plan``): a user whose robot
is refused passes looser tolerances or a plan of their own.
"""
import dataclasses
import json
from typing import Dict, List, Sequence, Union

import numpy as np

from .mjcf import JNT_HINGE

DEFAULT_TOL = 1e-3          # tol_pos (m), tol_axis (axis components), tol_range (rad).  Conventions.
FK_ROUNDING = 1e-12         # metres: the rounding allowance inside fk_bound


class SymmetryError(ValueError):
    """The robot is not left-right symmetric within the tolerances, or a plan is not a valid mirror map."""


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rot(q, v):
    t = 2.0 * np.cross(q[1:], v)
    return v + q[0] * t + np.cross(q[1:], t)


def rest_pose(robot):
    """``(X0 [nb, 3], W [nb, 3])``: world positions and world hinge axes (0 for a body without a hinge) with the root at the origin,
    identity rotation, every hinge at 0."""
    nb = robot.nbody
    X, Q, W = np.zeros((nb, 3)), np.zeros((nb, 4)), np.zeros((nb, 3))
    Q[0, 0] = 1.0
    for b in range(1, nb):
        p = int(robot.parent[b])
        X[b] = X[p] + _rot(Q[p], np.asarray(robot.body_pos[b], dtype=np.float64))
        Q[b] = _qmul(Q[p], np.asarray(robot.body_quat[b], dtype=np.float64))
        if robot.jnt_type[b] == JNT_HINGE:
            W[b] = _rot(Q[b], np.asarray(robot.jnt_axis[b], dtype=np.float64))
    return X, W


def _children(robot):
    ch = [[] for _ in range(robot.nbody)]
    for c in range(1, robot.nbody):
        ch[int(robot.parent[c])].append(c)
    return ch


def _subtrees(robot):
    """Per body the bodies of its subtree, itself included."""
    sub = [[b] for b in range(robot.nbody)]
    for b in range(robot.nbody - 1, 0, -1):
        sub[int(robot.parent[b])] += sub[b]
    return sub


M = np.array([1.0, -1.0, 1.0])


@dataclasses.dataclass(eq=False)
class SymmetryPlan:
    """``body_partner`` int32 ``[nb]`` (-1: unpaired), ``col_src`` int32 ``[nq]`` and ``col_sign`` float64 ``[nq]``: the mirrored row
    is ``out[c] = col_sign[c] * q[col_src[c]]`` on the hinge columns ``c >= 7`` (the root columns hold the identity and are not read
    by the kernel), ``unpaired``: names of the hinge-free bodies without a partner.  ``residual_pos`` (m), ``residual_axis`` and
    ``range_mismatch`` (rad) are the largest mismatches the pairing accepted, ``fk_bound`` (m) bounds how far the FK of a mirrored
    pose is from the reflected FK of the pose."""
    robot: str
    body_names: List[str]
    body_partner: np.ndarray
    col_src: np.ndarray
    col_sign: np.ndarray
    unpaired: List[str]
    residual_pos: float
    residual_axis: float
    range_mismatch: float
    fk_bound: float
    tol: Dict[str, float]

    def __post_init__(self):
        self.body_partner = np.ascontiguousarray(self.body_partner, dtype=np.int32).reshape(-1)
        self.col_src = np.ascontiguousarray(self.col_src, dtype=np.int32).reshape(-1)
        self.col_sign = np.ascontiguousarray(self.col_sign, dtype=np.float64).reshape(-1)
        self.body_names = [str(n) for n in self.body_names]
        self.unpaired = [str(n) for n in self.unpaired]
        self.check()

    @property
    def nq(self) -> int:
        return int(self.col_src.shape[0])

    def check(self) -> None:
        """What the kernel trusts and what makes the map a mirror: every hinge column reads a hinge column with a sign of +-1, and
        bodies and columns are involutions with equal signs."""
        nb, nq = len(self.body_names), self.nq
        p, src, sg = self.body_partner, self.col_src, self.col_sign
        if p.shape != (nb,) or sg.shape != (nq,) or nq < 7:
            raise SymmetryError("body_partner must hold one entry per body, col_src and col_sign one per qpos column (at least 7)")
        if np.any(p < -1) or np.any(p >= nb) or p[0] != 0:
            raise SymmetryError("body_partner must hold -1 or a body index, and the root is its own partner")
        for b in range(nb):
            if p[b] >= 0 and p[p[b]] != b:
                raise SymmetryError(f"not an involution: the partner of {self.body_names[b]!r} is {self.body_names[p[b]]!r}, whose partner is "
                                    f"{self.body_names[p[p[b]]] if p[p[b]] >= 0 else None!r}")
        if not (np.array_equal(src[:7], np.arange(7)) and np.all(sg[:7] == 1.0)):
            raise SymmetryError("the root columns 0..6 of col_src / col_sign must hold the identity")
        if np.any(src[7:] < 7) or np.any(src[7:] >= nq):
            raise SymmetryError(f"col_src must hold 7 <= col_src[c] < {nq} on the hinge columns")
        if not np.all(np.abs(sg) == 1.0):
            raise SymmetryError("col_sign must hold +1 or -1")
        for c in range(7, nq):
            if src[src[c]] != c or sg[src[c]] != sg[c]:
                raise SymmetryError(f"not an involution: column {c} reads column {src[c]} with sign {sg[c]:+.0f}, which reads column "
                                    f"{src[src[c]]} with sign {sg[src[c]]:+.0f}")

    def mirror_names(self, names: Sequence[str]) -> List[str]:
        """Every body name replaced by its partner's (for example ``contact_bodies`` of a mirrored clip)."""
        out = []
        for n in names:
            if n not in self.body_names:
                raise KeyError(n)
            p = int(self.body_partner[self.body_names.index(n)])
            if p < 0:
                raise SymmetryError(f"body {n!r} has no mirror partner")
            out.append(self.body_names[p])
        return out

    def to_json(self) -> Dict:
        """A plain JSON dict; floats are written with 17 digits, so the round trip is exact."""
        return {"format": "gmr_amd.symmetry.v1", "robot": self.robot, "body_names": list(self.body_names),
                "body_partner": [int(v) for v in self.body_partner], "col_src": [int(v) for v in self.col_src],
                "col_sign": [float(v) for v in self.col_sign], "unpaired": list(self.unpaired), "residual_pos": float(self.residual_pos),
                "residual_axis": float(self.residual_axis), "range_mismatch": float(self.range_mismatch), "fk_bound": float(self.fk_bound),
                "tol": {k: float(v) for k, v in self.tol.items()}}

    @classmethod
    def from_json(cls, d: Union[Dict, str]) -> "SymmetryPlan":
        """The inverse of ``to_json`` (a dict or its text).  The involution and the column bounds are checked again: a plan written
        by hand is trusted no more than one made here."""
        if isinstance(d, str):
            d = json.loads(d)
        if d.get("format") != "gmr_amd.symmetry.v1":
            raise SymmetryError("not a gmr_amd symmetry plan")
        return cls(robot=d["robot"], body_names=d["body_names"], body_partner=d["body_partner"], col_src=d["col_src"], col_sign=d["col_sign"],
                   unpaired=d.get("unpaired", []), residual_pos=float(d.get("residual_pos", float("nan"))),
                   residual_axis=float(d.get("residual_axis", float("nan"))), range_mismatch=float(d.get("range_mismatch", float("nan"))),
                   fk_bound=float(d.get("fk_bound", float("nan"))), tol=dict(d.get("tol", {})))

    def __eq__(self, other):
        return isinstance(other, SymmetryPlan) and json.dumps(self.to_json(), sort_keys=True) == json.dumps(other.to_json(), sort_keys=True)

    __hash__ = object.__hash__

    def check_robot(self, robot) -> None:
        """The plan belongs to this tree: the same bodies and the same number of columns."""
        if list(robot.body_names) != self.body_names or int(robot.nq) != self.nq:
            raise SymmetryError(f"the plan of {self.robot!r} ({len(self.body_names)} bodies, nq {self.nq}) does not describe {robot.name!r} "
                                f"({robot.nbody} bodies, nq {robot.nq})")


def save_plan(path: str, plan: SymmetryPlan) -> None:
    with open(path, "w") as f:
        json.dump(plan.to_json(), f, indent=1)


def load_plan(path: str) -> SymmetryPlan:
    with open(path) as f:
        return SymmetryPlan.from_json(json.load(f))


def plan_symmetry(robot, tol_pos: float = DEFAULT_TOL, tol_axis: float = DEFAULT_TOL, tol_range: float = DEFAULT_TOL) -> SymmetryPlan:
    """Pair the bodies of ``robot`` (a ``RobotModel``) from the root down.  ``partner[root] = root``; a child ``c`` of ``b`` pairs with
    a child ``d`` of ``partner[b]`` that is not yet taken, has the same joint type, ``max|M X0[c] - X0[d]| <= tol_pos`` and, for a
    hinge, ``max|W[d] + M W[c]| <= tol_axis`` (``sign = +1``) or ``max|W[d] - M W[c]| <= tol_axis`` (``sign = -1``); of several the
    nearest in position, then the lowest index.  A body without a candidate stays unpaired when its subtree holds no hinge (it
    carries no qpos column) and raises ``SymmetryError`` otherwise, as do a pairing that is not an involution and limited hinges
    whose ranges do not mirror within ``tol_range``.  A planar base is refused with ``NotImplementedError``."""
    if robot.planar_base:
        raise NotImplementedError(f"{robot.name}: a planar base is not mirrored (its qpos is not the free-joint layout outside the engine)")
    nb, nq = robot.nbody, int(robot.nq)
    X0, W = rest_pose(robot)
    children, subs = _children(robot), _subtrees(robot)
    hinge = np.asarray(robot.jnt_type) == JNT_HINGE
    names = list(robot.body_names)
    partner = np.full(nb, -1, np.int64)
    sign = np.ones(nb)
    pos_mis, axis_mis = np.zeros(nb), np.zeros(nb)
    partner[0] = 0
    taken = {0}
    unpaired: List[str] = []
    for b in range(nb):                      # a parent precedes its children, so partner[b] is known when b is reached
        if partner[b] < 0:
            continue
        for c in children[b]:
            best, near = None, None
            for d in children[int(partner[b])]:
                if d in taken or robot.jnt_type[d] != robot.jnt_type[c]:
                    continue
                dp = float(np.max(np.abs(M * X0[c] - X0[d])))
                da_plus, da_minus = float(np.max(np.abs(W[d] + M * W[c]))), float(np.max(np.abs(W[d] - M * W[c])))
                da, sg = (da_plus, 1.0) if da_plus <= da_minus else (da_minus, -1.0)
                if near is None or dp < near[0]:
                    near = (dp, d, da)
                if dp <= tol_pos and (not hinge[c] or da <= tol_axis) and (best is None or dp < best[0]):
                    best = (dp, d, da if hinge[c] else 0.0, sg)
            if best is not None:
                dp, d, da, sg = best
                partner[c], sign[c], pos_mis[c], axis_mis[c] = d, sg, dp, da
                taken.add(d)
            elif not any(hinge[s] for s in subs[c]):
                unpaired += [names[s] for s in sorted(subs[c])]
            else:
                where = (f"the nearest candidate is {names[near[1]]!r}: position mismatch {near[0]:.3e} m (tol_pos {tol_pos:g}), axis mismatch "
                         f"{near[2]:.3e} (tol_axis {tol_axis:g})") if near is not None else \
                    f"{names[int(partner[b])]!r} has no free child with the same joint type"
                raise SymmetryError(f"{robot.name}: body {names[c]!r} has no mirror partner under {names[int(partner[b])]!r}; {where}")
    for b in range(nb):
        p = int(partner[b])
        if p >= 0 and (partner[p] != b or sign[p] != sign[b]):
            raise SymmetryError(f"{robot.name}: the pairing is not an involution at {names[b]!r} -> {names[p]!r} -> "
                                f"{names[int(partner[p])] if partner[p] >= 0 else None!r} (signs {sign[b]:+.0f}, {sign[p]:+.0f})")
    range_mis = 0.0
    for b in np.nonzero(hinge)[0]:
        p = int(partner[b])
        if bool(robot.jnt_limited[b]) != bool(robot.jnt_limited[p]):
            raise SymmetryError(f"{robot.name}: hinge {names[b]!r} is {'limited' if robot.jnt_limited[b] else 'unlimited'} and its partner {names[p]!r} is not")
        if robot.jnt_limited[b]:
            mis = float(np.max(np.abs(np.sort(sign[b] * np.asarray(robot.jnt_range[b], dtype=np.float64)) - np.asarray(robot.jnt_range[p], dtype=np.float64))))
            if mis > tol_range:
                raise SymmetryError(f"{robot.name}: the range of {names[b]!r} {list(map(float, robot.jnt_range[b]))} does not mirror onto the range of "
                                    f"{names[p]!r} {list(map(float, robot.jnt_range[p]))}: mismatch {mis:.3e} rad (tol_range {tol_range:g})")
            range_mis = max(range_mis, mis)
    col_src, col_sign = np.arange(nq, dtype=np.int32), np.ones(nq)
    for b in np.nonzero(hinge)[0]:           # the mirrored pose gives partner[b] the angle sign * q[b]
        col_src[int(robot.qpos_adr[partner[b]])] = int(robot.qpos_adr[b])
        col_sign[int(robot.qpos_adr[partner[b]])] = sign[b]
    # fk_bound: per body the sum over its ancestors a (itself included) of
    #   position mismatch of a + axis mismatch of a x rest-pose reach of a's subtree,
    # the largest over the bodies, plus the rounding allowance.
    reach = np.array([max(float(np.sqrt(np.sum((X0[s] - X0[a]) ** 2))) for s in subs[a]) for a in range(nb)])
    term = np.where(partner >= 0, pos_mis + axis_mis * reach, 0.0)
    acc = np.zeros(nb)
    for b in range(1, nb):
        acc[b] = acc[int(robot.parent[b])] + term[b]
    paired = partner >= 0
    return SymmetryPlan(robot=robot.name, body_names=names, body_partner=partner.astype(np.int32), col_src=col_src, col_sign=col_sign,
                        unpaired=unpaired, residual_pos=float(pos_mis[paired].max()), residual_axis=float(axis_mis[paired].max()),
                        range_mismatch=range_mis, fk_bound=float(acc[paired].max()) + FK_ROUNDING,
                        tol={"tol_pos": float(tol_pos), "tol_axis": float(tol_axis), "tol_range": float(tol_range)})


def mirror_rows(plan: SymmetryPlan, qpos: np.ndarray) -> np.ndarray:
    """The world-plane mirror (y = 0) of qpos rows ``[..., nq]`` on the host, in numpy: the definition of ``GMR_MIRROR_WORLD``
    (include/gmr_amd.h), copies and sign flips only."""
    q = np.asarray(qpos, dtype=np.float64)
    out = plan.col_sign * q[..., plan.col_src]
    out[..., :7] = q[..., :7] * np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0])
    return out
