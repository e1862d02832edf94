"""Collision proxies of a robot for the self-collision report (``Engine.motion_self_collision``, ``gmr_motion_self_collision``):
capsules fixed to bodies and the list of capsule pairs that are tested.  Host only, numpy only.

A capsule is a segment ``p0 .. p1`` in its body's frame with a radius; ``p0 == p1`` is a sphere.  ``skeleton_capsules`` builds the
default table from the kinematic tree alone: one capsule along every link and a sphere at every leaf.  The MJCF ``<geom>``
primitives and meshes of a robot are NOT read (G1's collision geometry is meshes, K1 and T1 use boxes and cylinders):
the skeleton is thinner than the robot almost everywhere, so a reported penetration is one of the skeleton's capsules, and the
default radius of 0.03 m is a convention, not measured on any robot.  A table tuned by hand travels as a plain JSON dict
(``CapsuleTable.to_dict`` / ``from_dict``, ``PairTable.to_dict`` / ``from_dict``, ``save_proxies`` / ``load_proxies``).
"""
import dataclasses
import json
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

DEFAULT_RADIUS = 0.03        # metres.  A convention, not measured on any robot.
MAX_CAPSULES, MAX_PAIRS = 256, 32768   # what one gmr_motion_self_collision call accepts
SAME_BODY, ALWAYS_OVERLAP, REST_OVERLAP = "same_body", "always_overlap", "rest_overlap"   # why default_pairs drops a pair


@dataclasses.dataclass(eq=False)
class CapsuleTable:
    """``C`` capsules: ``body`` int32 ``[C]`` (index into the robot's bodies), ``p0`` / ``p1`` float64 ``[C, 3]`` in the body frame,
    ``radius`` float64 ``[C]``, ``names`` (one per capsule).  ``anchors``: per capsule the bodies whose origins lie on its segment
    (``skeleton_capsules`` fills it; ``None`` for a hand-made table, which ``default_pairs`` then treats as anchored on its body
    alone when an end lies at the body's origin, and on nothing otherwise)."""
    body: np.ndarray
    p0: np.ndarray
    p1: np.ndarray
    radius: np.ndarray
    names: List[str]
    anchors: Optional[List[Tuple[int, ...]]] = None

    def __post_init__(self):
        self.body = np.ascontiguousarray(self.body, dtype=np.int32).reshape(-1)
        C = self.body.shape[0]
        self.p0 = np.ascontiguousarray(self.p0, dtype=np.float64).reshape(C, 3)
        self.p1 = np.ascontiguousarray(self.p1, dtype=np.float64).reshape(C, 3)
        self.radius = np.ascontiguousarray(self.radius, dtype=np.float64).reshape(-1)
        self.names = [str(n) for n in self.names]
        if self.radius.shape != (C,) or len(self.names) != C:
            raise ValueError("body, p0, p1, radius and names must describe the same number of capsules")
        if not (np.all(np.isfinite(self.p0)) and np.all(np.isfinite(self.p1)) and np.all(np.isfinite(self.radius)) and np.all(self.radius >= 0.0)):
            raise ValueError("capsule ends and radii must be finite, radii >= 0")
        if self.anchors is not None:
            self.anchors = [tuple(int(b) for b in a) for a in self.anchors]
            if len(self.anchors) != C:
                raise ValueError("one anchor set per capsule")

    def __len__(self):
        return int(self.body.shape[0])

    def to_dict(self) -> Dict:
        """A plain JSON dict; floats are written by ``repr`` semantics of ``json`` (17 digits), so the round trip is exact."""
        d = {"capsules": [{"name": n, "body": int(b), "p0": [float(x) for x in a], "p1": [float(x) for x in e], "radius": float(r)}
                          for n, b, a, e, r in zip(self.names, self.body, self.p0, self.p1, self.radius)]}
        if self.anchors is not None:
            for c, a in zip(d["capsules"], self.anchors):
                c["anchors"] = list(a)
        return d

    @classmethod
    def from_dict(cls, d: Dict, robot=None) -> "CapsuleTable":
        """The inverse of ``to_dict``.  With ``robot`` (a ``RobotModel``) a ``body`` may be given by name."""
        caps = d["capsules"]

        def body(v):
            if isinstance(v, str):
                if robot is None:
                    raise ValueError(f"capsule body '{v}' is a name: a robot is needed to resolve it")
                return robot.body_names.index(v)
            return int(v)

        anchors = [tuple(body(b) for b in c["anchors"]) for c in caps] if caps and all("anchors" in c for c in caps) else None
        return cls(body=np.array([body(c["body"]) for c in caps], np.int32), p0=np.array([c["p0"] for c in caps], np.float64).reshape(len(caps), 3),
                   p1=np.array([c.get("p1", c["p0"]) for c in caps], np.float64).reshape(len(caps), 3),
                   radius=np.array([c["radius"] for c in caps], np.float64), names=[c.get("name", f"capsule{i}") for i, c in enumerate(caps)],
                   anchors=anchors)


@dataclasses.dataclass(eq=False)
class PairTable:
    """``P`` capsule pairs, int32 ``[P, 2]`` with ``a < b``."""
    pairs: np.ndarray

    def __post_init__(self):
        self.pairs = np.ascontiguousarray(self.pairs, dtype=np.int32).reshape(-1, 2)
        if self.pairs.size and not (np.all(self.pairs[:, 0] < self.pairs[:, 1]) and np.all(self.pairs >= 0)):
            raise ValueError("every pair must hold 0 <= a < b")

    def __len__(self):
        return int(self.pairs.shape[0])

    def to_dict(self) -> Dict:
        return {"pairs": [[int(a), int(b)] for a, b in self.pairs]}

    @classmethod
    def from_dict(cls, d: Dict) -> "PairTable":
        return cls(np.array(d["pairs"], np.int32).reshape(-1, 2))


def save_proxies(path: str, capsules: CapsuleTable, pairs: Optional[PairTable] = None) -> None:
    """One JSON file with the capsules and, if given, the pairs."""
    d = capsules.to_dict()
    if pairs is not None:
        d.update(pairs.to_dict())
    with open(path, "w") as f:
        json.dump(d, f, indent=1)


def load_proxies(path: str, robot=None) -> Tuple[CapsuleTable, Optional[PairTable]]:
    """``(capsules, pairs or None)`` of a file written by ``save_proxies`` or by hand."""
    with open(path) as f:
        d = json.load(f)
    return CapsuleTable.from_dict(d, robot), (PairTable.from_dict(d) if "pairs" in d else None)


def skeleton_capsules(robot, radius: Union[float, Dict[str, float]] = DEFAULT_RADIUS) -> CapsuleTable:
    """The default proxies of ``robot`` (a ``RobotModel``): every body ``b`` gets one capsule per child ``c``, from the origin of
    ``b`` to ``body_pos[c]`` in b's frame (named ``"b -> c"``, anchors ``{b, c}``), and every leaf body a sphere at its origin
    (named ``"b"``, anchors ``{b}``).  ``radius``: one number, or ``{body_name: r, "default": r}`` by the name of ``b``.  The
    default of 0.03 m is a convention, not measured on any robot, and the skeleton is not the robot's collision geometry."""
    if isinstance(radius, dict):
        default = float(radius.get("default", DEFAULT_RADIUS))
        unknown = set(radius) - set(robot.body_names) - {"default"}
        if unknown:
            raise ValueError(f"radius names bodies the robot does not have: {sorted(unknown)}")
        rad = [float(radius.get(n, default)) for n in robot.body_names]
    else:
        rad = [float(radius)] * robot.nbody
    children = [[] for _ in range(robot.nbody)]
    for c in range(1, robot.nbody):
        children[int(robot.parent[c])].append(c)
    body, p0, p1, r, names, anchors = [], [], [], [], [], []
    for b in range(robot.nbody):
        for c in children[b]:
            body.append(b); p0.append(np.zeros(3)); p1.append(np.asarray(robot.body_pos[c], dtype=np.float64)); r.append(rad[b])
            names.append(f"{robot.body_names[b]} -> {robot.body_names[c]}"); anchors.append((b, c))
        if not children[b]:
            body.append(b); p0.append(np.zeros(3)); p1.append(np.zeros(3)); r.append(rad[b])
            names.append(robot.body_names[b]); anchors.append((b,))
    return CapsuleTable(np.array(body, np.int32), np.array(p0), np.array(p1), np.array(r), names, anchors)


def _tree_distance(robot):
    """[nb, nb]: the sum of |body_pos| along the tree path between two bodies (an upper bound of the distance of their origins in
    every pose: each link of the chain is rigid)."""
    nb = robot.nbody
    link = np.sqrt(np.sum(np.asarray(robot.body_pos, dtype=np.float64) ** 2, axis=1))
    up = []   # per body {ancestor (itself included): chain length to it}
    for b in range(nb):
        d, j, s = {b: 0.0}, b, 0.0
        while int(robot.parent[j]) >= 0:
            s += float(link[j])
            j = int(robot.parent[j])
            d[j] = s
        up.append(d)
    D = np.zeros((nb, nb))
    for a in range(nb):
        for b in range(a + 1, nb):
            D[a, b] = D[b, a] = min(up[a][j] + up[b][j] for j in up[a] if j in up[b])
    return D


def _anchors(capsules: CapsuleTable):
    if capsules.anchors is not None:
        return capsules.anchors
    return [((int(b),) if (not a.any() or not e.any()) else ()) for b, a, e in zip(capsules.body, capsules.p0, capsules.p1)]


def segment_distance(p1, q1, p2, q2):
    """The distance of the segments ``p1 .. q1`` and ``p2 .. q2`` (arrays ``[..., 3]``, broadcast): the clamped closest-point
    formula of the contract above ``gmr_self_collision_input`` (include/gmr_amd.h), in its operation order."""
    p1, q1, p2, q2 = (np.asarray(t, dtype=np.float64) for t in (p1, q1, p2, q2))
    dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]   # noqa: E731
    with np.errstate(all="ignore"):
        c01 = lambda x: np.where(x > 0.0, np.where(x < 1.0, x, 1.0), 0.0)                          # noqa: E731  (0 for a NaN)
        d1, d2, r = q1 - p1, q2 - p2, p1 - p2
        a, e, f, c, b = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
        den = a * e - b * b
        s = np.where(den > 0.0, c01((b * f - c * e) / den), 0.0)
        t = np.where(e > 0.0, (b * s + f) / e, 0.0)
        lo, hi = ~(e > 0.0) | (t < 0.0), t > 1.0
        s = np.where(lo, np.where(a > 0.0, c01(-c / a), 0.0), np.where(hi, np.where(a > 0.0, c01((b - c) / a), 0.0), s))
        t = np.where(lo, 0.0, np.where(hi, 1.0, t))
        w = (p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)
        return np.sqrt(dot(w, w))


def rest_ends(robot, capsules: CapsuleTable):
    """World ends ``(P, Q)`` ``[C, 3]`` of the capsules in the rest pose: zero hinges, identity root at the origin."""
    nb = robot.nbody
    X, Q = np.zeros((nb, 3)), np.zeros((nb, 4))
    Q[0, 0] = 1.0
    for b in range(1, nb):
        p = int(robot.parent[b])
        X[b] = X[p] + _rot(Q[p], robot.body_pos[b])
        Q[b] = _qmul(Q[p], robot.body_quat[b])
    return X[capsules.body] + _rot(Q[capsules.body], capsules.p0), X[capsules.body] + _rot(Q[capsules.body], capsules.p1)


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rot(q, v):
    t = 2.0 * np.cross(q[..., 1:], v)
    return v + q[..., :1] * t + np.cross(q[..., 1:], t)


def default_pairs(robot, capsules: CapsuleTable, rest_margin: float = 0.0):
    """All unordered capsule pairs ``(a, b)``, ``a < b``, in lexicographic order, without three kinds:

    ``same_body``       both capsules sit on the same body;
    ``always_overlap``  some anchor of one and some anchor of the other are joined by a chain of links whose lengths (``|body_pos|``
                        along the tree path) add up to at most ``rA + rB``: both anchor origins lie on the segments, so the
                        capsules overlap in every pose;
    ``rest_overlap``    the clearance in the rest pose (zero hinges, identity root) is at most ``rest_margin``.

    Returns ``(PairTable, dropped)``, ``dropped`` a list of ``((a, b), reason)`` in lexicographic order."""
    C = len(capsules)
    D = _tree_distance(robot)
    anchors = _anchors(capsules)
    P, Q = rest_ends(robot, capsules)
    ia, ib = np.triu_indices(C, 1)
    rest = segment_distance(P[ia], Q[ia], P[ib], Q[ib]) - (capsules.radius[ia] + capsules.radius[ib])
    kept, dropped = [], []
    for k, (a, b) in enumerate(zip(ia.tolist(), ib.tolist())):
        rr = float(capsules.radius[a] + capsules.radius[b])
        if capsules.body[a] == capsules.body[b]:
            dropped.append(((a, b), SAME_BODY))
        elif any(D[i, j] <= rr for i in anchors[a] for j in anchors[b]):
            dropped.append(((a, b), ALWAYS_OVERLAP))
        elif rest[k] <= rest_margin:
            dropped.append(((a, b), REST_OVERLAP))
        else:
            kept.append((a, b))
    return PairTable(np.array(kept, np.int32).reshape(-1, 2)), dropped


def pair_names(capsules: CapsuleTable, pairs: PairTable) -> List[Tuple[str, str]]:
    """The two capsule names of every pair."""
    return [(capsules.names[int(a)], capsules.names[int(b)]) for a, b in pairs.pairs]


def proxies(robot, capsules: Optional[CapsuleTable] = None, pairs: Optional[PairTable] = None,
            radius=DEFAULT_RADIUS) -> Tuple[CapsuleTable, PairTable]:
    """``(capsules, pairs)`` with the defaults filled in: ``skeleton_capsules(robot, radius)`` and ``default_pairs`` of them."""
    caps = capsules if capsules is not None else skeleton_capsules(robot, radius)
    return caps, (pairs if pairs is not None else default_pairs(robot, caps)[0])


def movable_mask(robot, freeze_joints=(), freeze_bodies=()) -> int:
    """The ``hinge_mask`` of the self-collision repair (``Engine.motion_self_collision_repair``): bit ``i`` set means that hinge
    ``i``, in qpos order, may move.  ``freeze_joints``: joint names whose hinges stay.  ``freeze_bodies``: body names (or indices);
    a frozen body freezes every hinge on its path to the root, so the body stays where it is -- freezing the ankle links keeps a
    locked foot where ``lock_feet`` put it."""
    hb = sorted((b for b in robot.hinge_bodies()), key=lambda b: int(robot.qpos_adr[b]))
    bit = {b: i for i, b in enumerate(hb)}
    if len(hb) > 64:
        raise ValueError(f"a hinge mask holds 64 hinges, the robot has {len(hb)}")
    by_joint = {robot.jnt_names[b]: b for b in hb}
    frozen = set()
    for n in freeze_joints:
        if n not in by_joint:
            raise ValueError(f"'{n}' is not a hinge joint of {robot.name}")
        frozen.add(by_joint[n])
    for n in freeze_bodies:
        if isinstance(n, str) and n not in robot.body_names:
            raise ValueError(f"'{n}' is not a body of {robot.name}")
        j = robot.body_names.index(n) if isinstance(n, str) else int(n)
        if not 0 <= j < robot.nbody:
            raise ValueError(f"body {j} is outside the robot's {robot.nbody}")
        while j >= 0:
            if j in bit:
                frozen.add(j)
            j = int(robot.parent[j])
    return sum(1 << bit[b] for b in hb if b not in frozen)


def check_tables(nbody: int, capsules: CapsuleTable, pairs: PairTable) -> None:
    """What the kernel trusts: bodies and pair entries in range, counts within one call's limits."""
    C, P = len(capsules), len(pairs)
    if not 1 <= C <= MAX_CAPSULES:
        raise ValueError(f"1 .. {MAX_CAPSULES} capsules per call, got {C}")
    if not 1 <= P <= MAX_PAIRS:
        raise ValueError(f"1 .. {MAX_PAIRS} pairs per call, got {P}")
    if capsules.body.min() < 0 or capsules.body.max() >= nbody:
        raise ValueError(f"a capsule names a body outside the model's {nbody}")
    if pairs.pairs.max() >= C:
        raise ValueError(f"a pair names a capsule outside the table's {C}")
