"""The inertial table of an MJCF robot: what ``mjcf.load_mjcf`` leaves out and ``Engine.motion_dynamics`` needs.

Per body, in the body order of :class:`gmr_amd.mjcf.RobotModel` (depth first): ``mass``, the centre of mass in the body frame and
the symmetric 3 x 3 inertia about it in the body frame (``<inertial pos quat mass diaginertia|fullinertia>``).  Per hinge, in qpos
order: ``armature`` and a symmetric torque limit -- the joint's ``actuatorfrcrange`` where present (the larger magnitude of its two
ends), otherwise the ``<motor>`` / ``<position>`` actuator on that joint (``ctrlrange`` times ``gear[0]``, class defaults, default
gear 1; a ``<position>`` actuator's ``forcerange`` wins over its ``ctrlrange``, which is an angle), otherwise ``+inf``.
``<include>`` and default classes are honoured as ``mjcf.py`` does.  ``<compiler angle>`` changes nothing here: the only angles an
``<inertial>`` can carry are its ``euler`` / ``axisangle`` orientations, and those are refused (``quat`` only, as for bodies).
``actuatorfrcrange`` counts as a limit when ``actuatorfrclimited`` is ``true``, or is absent / ``auto`` with ``<compiler
autolimits>`` on (MuJoCo's default); ``actuatorfrclimited="false"`` switches it off, and the actuator is looked at next.  An
actuator's ``ctrlrange`` / ``forcerange`` is taken where it is written, whatever ``ctrllimited`` / ``forcelimited`` say.  Nothing is
inferred from geoms or meshes: a body without ``<inertial>`` has mass 0 and is listed in ``missing``; a model without any
``<inertial>`` is an error.
"""
from __future__ import annotations

import dataclasses
import os
import xml.etree.ElementTree as ET
from typing import Dict, List, Optional

import numpy as np

from .mjcf import JNT_HINGE, MjcfError, RobotModel, _Defaults, _expand_includes, _floats


@dataclasses.dataclass
class InertialTable:
    body_names: List[str]
    parent: np.ndarray         # int32 [nb], -1 for the root
    mass: np.ndarray           # [nb] kg
    com: np.ndarray            # [nb, 3] centre of mass in the body frame
    inertia: np.ndarray        # [nb, 3, 3] symmetric, about the centre of mass, body frame
    hinge_names: List[Optional[str]]
    armature: np.ndarray       # [nh] kg m^2, qpos order
    torque_limit: np.ndarray   # [nh] N m, > 0, +inf where the model gives none
    limit_source: List[str]    # [nh] "actuatorfrcrange" | "motor" | "position" | "none"
    missing: List[str]         # bodies without <inertial> (mass 0)

    @property
    def nbody(self) -> int:
        return len(self.body_names)

    @property
    def total_mass(self) -> float:
        s = 0.0
        for m in self.mass:     # in body order, as the kernel adds them
            s = s + float(m)
        return s


def quat_to_mat(q) -> np.ndarray:
    """Rotation matrix of a wxyz quaternion (normalised first)."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class _ClassDefaults:
    """Attribute defaults of one element tag by class, with ``_Defaults``' inheritance (a nested class starts from its parent's)."""

    def __init__(self, root: ET.Element, tags):
        self.tags = tuple(tags)
        self.by_class: Dict[str, Dict[str, str]] = {"main": {}}
        for top in root.findall("default"):
            self._walk(top, top.attrib.get("class", "main"), {})

    def _walk(self, node, cls, inherited):
        attrs = dict(inherited)
        for t in self.tags:
            for e in node.findall(t):
                attrs.update(e.attrib)
        merged = dict(self.by_class.get(cls, {}))
        merged.update(attrs)
        self.by_class[cls] = merged
        for sub in node.findall("default"):
            if sub.attrib.get("class") is None:
                raise MjcfError("nested <default> without class")
            self._walk(sub, sub.attrib["class"], attrs)

    def attrs(self, elem: ET.Element) -> Dict[str, str]:
        out = dict(self.by_class.get(elem.attrib.get("class", "main"), self.by_class["main"]))
        out.update(elem.attrib)
        return out


def _symmetric_limit(text: str, what: str) -> float:
    lo, hi = _floats(text, 2, what)
    return float(max(abs(lo), abs(hi)))


def load_inertial(path: str) -> InertialTable:
    """Read the inertial table of the MJCF file at ``path`` (module docstring)."""
    path = os.fspath(path)
    root = ET.parse(path).getroot()
    root_dir = os.path.dirname(os.path.abspath(path))
    _expand_includes(root, root_dir, root_dir)
    jdef = _Defaults(root)
    autolimits = True
    for c in root.findall("compiler"):
        autolimits = c.attrib.get("autolimits", "true" if autolimits else "false") == "true"
    roots = [b for wb in root.findall("worldbody") for b in wb.findall("body")]
    if len(roots) != 1:
        raise MjcfError(f"expected exactly one top-level <body>, found {len(roots)}")

    names, parent, mass, com, inertia, missing = [], [], [], [], [], []
    hinge_names, armature, limit, source = [], [], [], []

    def add_body(node, par, childclass):
        childclass = node.attrib.get("childclass", childclass)
        idx = len(names)
        names.append(node.attrib.get("name", f"body{idx}"))
        parent.append(par)
        inertials = node.findall("inertial")
        if len(inertials) > 1:
            raise MjcfError(f"body {names[-1]}: more than one <inertial>")
        if not inertials:
            missing.append(names[-1])
            mass.append(0.0); com.append(np.zeros(3)); inertia.append(np.zeros((3, 3)))
        else:
            a = inertials[0].attrib
            for k in ("euler", "axisangle", "xyaxes", "zaxis"):
                if k in a:
                    raise MjcfError(f"body {names[-1]}: inertial orientation attribute {k!r} not supported")
            if "mass" not in a:
                raise MjcfError(f"body {names[-1]}: <inertial> without mass")
            m = float(a["mass"])
            if not m >= 0.0:
                raise MjcfError(f"body {names[-1]}: negative mass")
            R = quat_to_mat(_floats(a.get("quat", "1 0 0 0"), 4, "inertial quat"))
            if "fullinertia" in a:
                xx, yy, zz, xy, xz, yz = _floats(a["fullinertia"], 6, "fullinertia")
                I0 = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
            elif "diaginertia" in a:
                I0 = np.diag(_floats(a["diaginertia"], 3, "diaginertia"))
            else:
                raise MjcfError(f"body {names[-1]}: <inertial> without diaginertia or fullinertia")
            I = R @ I0 @ R.T
            mass.append(m); com.append(_floats(a.get("pos", "0 0 0"), 3, "inertial pos")); inertia.append(0.5 * (I + I.T))
        joints = node.findall("joint")
        if par != -1 and len(joints) == 1:
            ja = jdef.joint_attrs(joints[0], childclass)
            if ja.get("type", "hinge") == "hinge":
                hinge_names.append(ja.get("name"))
                armature.append(float(ja.get("armature", 0.0)))
                frclimited = ja.get("actuatorfrclimited", "auto")
                if "actuatorfrcrange" in ja and (frclimited == "true" or (frclimited == "auto" and autolimits)):
                    limit.append(_symmetric_limit(ja["actuatorfrcrange"], "actuatorfrcrange")); source.append("actuatorfrcrange")
                else:
                    limit.append(np.inf); source.append("none")
        for child in node.findall("body"):
            add_body(child, idx, childclass)

    add_body(roots[0], -1, None)
    if len(missing) == len(names):
        raise MjcfError(f"{os.path.basename(path)}: no body carries an <inertial>")

    adef = _ClassDefaults(root, ("motor", "position", "general"))   # <general> defaults carry gear / ctrlrange for both short forms
    by_joint = {n: i for i, n in enumerate(hinge_names) if n is not None}
    for act in root.findall("actuator"):
        for e in act:
            if e.tag not in ("motor", "position"):
                continue
            a = adef.attrs(e)
            i = by_joint.get(a.get("joint"))
            if i is None or source[i] != "none":
                continue
            gear = abs(float(a.get("gear", "1").split()[0]))
            if e.tag == "position" and "forcerange" in a:
                limit[i] = _symmetric_limit(a["forcerange"], "forcerange") * gear
            elif "ctrlrange" in a:
                limit[i] = _symmetric_limit(a["ctrlrange"], "ctrlrange") * gear
            else:
                continue
            source[i] = e.tag
    lim = np.asarray(limit, dtype=np.float64).reshape(-1)
    lim[~(lim > 0.0)] = np.inf   # a zero or NaN range limits nothing
    return InertialTable(body_names=names, parent=np.asarray(parent, dtype=np.int32), mass=np.asarray(mass, dtype=np.float64),
                         com=np.asarray(com, dtype=np.float64).reshape(-1, 3), inertia=np.asarray(inertia, dtype=np.float64).reshape(-1, 3, 3),
                         hinge_names=hinge_names, armature=np.asarray(armature, dtype=np.float64).reshape(-1), torque_limit=lim,
                         limit_source=source, missing=missing)


def inertial_table(robot: RobotModel) -> InertialTable:
    """The table of a loaded robot, read from the MJCF file it was compiled from and checked against its tree."""
    path = getattr(robot, "xml_path", None)
    if not path:
        raise MjcfError(f"robot {robot.name!r} was not loaded from an MJCF file: no inertial data")
    t = load_inertial(path)
    hinges = [robot.jnt_names[b] for b in np.nonzero(robot.jnt_type == JNT_HINGE)[0]]
    if t.body_names != list(robot.body_names) or not np.array_equal(t.parent, robot.parent) or t.hinge_names != hinges:
        raise MjcfError(f"{path}: the inertial table does not match the robot's tree")
    return t
