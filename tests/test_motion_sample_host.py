"""The motion library without a GPU: the header and the binding of gmr_motion_sample, schedule.clip_durations, and the numpy
restatement of the contract (tests/motion_sample_reference.py) checked against itself -- its twists against central differences
of its own forward kinematics, and the edge cases of its plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import motion_sample_reference as ref
from tests.util import compiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS = ["unitree_g1", "stanford_toddy"]


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------ 1: header and binding
def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_sample\s*\(gmr_model \*m, const gmr_sample_input \*in, void \*stream\);", code)
    assert "gmr_motion_sample" in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5
    lib = _native.load()
    assert lib.gmr_abi_version() == 5
    assert lib.gmr_motion_sample.restype == C.c_int and lib.gmr_motion_sample.argtypes[1]._type_ is _native.SampleInput


def test_struct_layout_equals_the_listing_in_the_header():
    from gmr_amd import _native
    src = _header()
    m = re.search(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct gmr_sample_input \{(.*?)\} gmr_sample_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_sample_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []  # field names in declaration order
    for stmt in body.split(";"):
        names = re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
        declared += names
    fields = [k for k, _ in _native.SampleInput._fields_]
    assert declared == fields
    assert C.sizeof(_native.SampleInput) == int(m.group(1)) == 168
    assert listing == {k: getattr(_native.SampleInput, k).offset for k in fields}
    assert fields[-10:] == [k + "_out" for k in _native.TRACK_OUTPUTS]


# ------------------------------------------------------------------ 2: clip_durations
def test_clip_durations():
    from gmr_amd.schedule import clip_durations
    offs = np.cumsum([0, 0, 1, 2, 31])
    d = clip_durations(offs, 30.0)
    assert d.dtype == np.float64 and d.tolist() == [0.0, 0.0, 1.0 / 30.0, 1.0]
    d = clip_durations(offs, [30.0, 60.0, 50.0, 120.0])
    assert d.tolist() == [0.0, 0.0, 1.0 / 50.0, 30.0 / 120.0]
    assert clip_durations([0], 30.0).shape == (0,)
    for bad_offs, bad_fps in (([0, 3, 2], 30.0), ([[0, 1]], 30.0), ([0, 1, 2], [30.0]), ([0, 1], 0.0), ([0, 1], -1.0),
                              ([0, 1], float("nan")), ([0, 1, 2], [30.0, float("inf")])):
        with pytest.raises(ValueError):
            clip_durations(bad_offs, bad_fps)


# ------------------------------------------------------------------ 3: the twist formula against the restatement's own FK
def _exp_quat(w):
    """exp of a rotation vector as an xyzw quaternion."""
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    return np.concatenate([np.sin(th / 2) * w / np.where(th == 0, 1.0, th), np.cos(th / 2)], axis=-1)


def _qmul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - np.sum(av * bv, axis=-1, keepdims=True)], axis=-1)


def _rotvec(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    q = np.where(q[..., 3:] < 0, -q, q)
    n = np.linalg.norm(q[..., :3], axis=-1, keepdims=True)
    return q[..., :3] * (2.0 * np.arctan2(n, q[..., 3:]) / np.where(n == 0, 1.0, n))


def _twist_vs_difference(tree, seed, eps=1e-5, Q=64):
    """Largest deviation of the float64 twist from the central difference of the restatement's own FK along the generalized
    velocity, linear (m/s) and angular (rad/s), and the case."""
    rng = np.random.default_rng(seed)
    rr = rng.normal(size=(Q, 4))
    gen = {"root_pos": rng.normal(size=(Q, 3)), "root_rot": rr / np.linalg.norm(rr, axis=1, keepdims=True),
           "joint_pos": rng.uniform(-1.0, 1.0, size=(Q, tree.nd)),
           "root_lin_vel": rng.uniform(-5, 5, size=(Q, 3)) / np.sqrt(3.0), "root_ang_vel": rng.uniform(-5, 5, size=(Q, 3)) / np.sqrt(3.0),
           "joint_vel": rng.uniform(-5, 5, size=(Q, tree.nd))}
    tw = ref.chain(tree, gen, np.float64)

    def moved(sgn):
        g = dict(gen)
        g["root_pos"] = gen["root_pos"] + sgn * eps * gen["root_lin_vel"]
        g["root_rot"] = _qmul(_exp_quat(sgn * eps * gen["root_ang_vel"]), gen["root_rot"])
        g["joint_pos"] = gen["joint_pos"] + sgn * eps * gen["joint_vel"]
        return ref.chain(tree, g, np.float64)

    plus, minus = moved(+1.0), moved(-1.0)
    lin = (plus["body_pos_w"] - minus["body_pos_w"]) / (2 * eps)
    conj = minus["body_quat_w"] * np.array([-1.0, -1.0, -1.0, 1.0])
    ang = _rotvec(_qmul(plus["body_quat_w"], conj)) / (2 * eps)
    return np.abs(lin - tw["body_lin_vel_w"]).max(), np.abs(ang - tw["body_ang_vel_w"]).max(), gen


@pytest.mark.parametrize("robot", ROBOTS)
def test_twist_is_the_derivative_of_the_restatements_fk(robot):
    """(FK(q + eps v) - FK(q - eps v)) / 2 eps against the float64 twist, eps = 1e-5, speeds <= 5 m/s and 5 rad/s: truncation
    ~ eps^2 |v|^3 reach / 6 < 1e-7, round-off ~ 1e-16 / eps = 1e-11; the bound is 1e-6.

    That reasoning is a rigid chain's, and the check runs on one: the tree with its local rotations normalised (measured: G1
    1.7e-8 m/s and 3.9e-8 rad/s, Toddy 1.4e-8 and 4.2e-8).  gmr_fk uses the XML's local quaternions as they are, |q|^2 = 1 + delta
    with delta up to 7e-7, and its quat_rotate(q, v) is then s^2 R v + (s^2 - 1) v with s^2 the product of the |q|^2 above the
    body: the chain is not quite rigid, and the rigid-body formula of the contract (on the chain's own x and R) departs from the
    chain's derivative by the defect -- per hinge at most 2 D |thetadot| in the angular velocity, per link |w| |l| D plus the
    angular error times |x_j - x_p| in the linear one, D the largest |s^2 - 1| of the tree.  Measured on the raw trees: G1
    8.5e-6 m/s and 1.8e-5 rad/s at |v| <= 8.5 m/s and |w| <= 18 rad/s, Toddy 4.4e-6 and 3.8e-5 -- a relative 1e-6, below the float32
    the body velocities are stored in.  The raw tree is held to that derived bound (second half of the test)."""
    rob = compiled("smplx", robot).robot
    e_lin, e_ang, _ = _twist_vs_difference(ref.Tree(rob, unit=True), ROBOTS.index(robot))
    print(f"[motion_sample] {robot} twist vs central difference, rigid tree: lin {e_lin:.3e} m/s, ang {e_ang:.3e} rad/s")
    assert e_lin <= 1e-6 and e_ang <= 1e-6
    tree = ref.Tree(rob)
    r_lin, r_ang, gen = _twist_vs_difference(tree, ROBOTS.index(robot))
    # the defect bound, from the tree and the case's inputs alone: along every root-to-body path
    n2 = np.sum(tree.lrot.astype(np.float64) ** 2, axis=1)
    s2, reach, rate = np.ones(tree.nb), np.zeros(tree.nb), np.zeros(tree.nb)
    jv = np.abs(gen["joint_vel"]).max(axis=0)
    for j in range(1, tree.nb):
        p = int(tree.parent[j])
        s2[j], reach[j] = s2[p] * n2[j], reach[p] + np.linalg.norm(tree.lpos[j].astype(np.float64))
        rate[j] = rate[p] + (jv[tree.dof[j]] if tree.dof[j] >= 0 else 0.0)
    D, S, L = np.abs(s2 - 1.0).max(), rate.max(), reach.max()
    b_ang = 1e-6 + 2.0 * D * S
    b_lin = 1e-6 + 1.01 * L * ((5.0 + S) * D + b_ang)
    print(f"[motion_sample] {robot} raw tree: lin {r_lin:.3e} (bound {b_lin:.3e}) m/s, ang {r_ang:.3e} (bound {b_ang:.3e}) rad/s, D = {D:.2e}")
    assert r_lin <= b_lin and r_ang <= b_ang


# ------------------------------------------------------------------ 4: plan edge cases of the restatement
LENS, FPS = [1, 2, 3, 7, 0, 64, 65], [30.0, 120.0, 50.0, 30.0, 30.0, 32.0, 128.0]
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)


def _plan1(s, t):
    valid, rows, a, h0, h1 = ref.plan(OFFS, FPS, [s], [t])
    return bool(valid[0]), (rows[0] - OFFS[s]).tolist(), float(a[0]), float(h0[0]), float(h1[0])


def test_plan_edges():
    for s, (T, f) in enumerate(zip(LENS, FPS)):
        if T == 0:
            assert not _plan1(s, 0.0)[0]
            continue
        last = (T - 1) / f
        for t in (-1.0, -1e-300, 0.0):  # before the clip and at its start: frame 0, a copy
            ok, (km0, i0, i1, kp1, km1), a, h0, h1 = _plan1(s, t)
            assert ok and i0 == 0 and km0 == 0 and a == 0.0 and i1 == min(1, T - 1)
        for t in (last, np.nextafter(last, np.inf), last + 1.0, 1e300):  # at the last frame and beyond: frame T-1, a copy
            ok, (km0, i0, i1, kp1, km1), a, h0, h1 = _plan1(s, t)
            assert ok and i0 == i1 == kp1 == T - 1 and a == 0.0 and km0 == max(T - 2, 0), (s, t)
        if T > 1:  # strictly inside the first interval
            ok, (km0, i0, i1, kp1, km1), a, h0, h1 = _plan1(s, 0.25 / f)
            assert ok and (km0, i0, i1, km1) == (0, 0, 1, 0) and kp1 == min(2, T - 1) and abs(a - 0.25) < 1e-15
            assert h0 == 1.0 * (1.0 / f) and h1 == float(kp1) * (1.0 / f)
    for t in (np.nan, np.inf, -np.inf):
        assert not _plan1(3, t)[0]
    for s in (-1, len(LENS), 2 ** 40):
        assert not ref.plan(OFFS, FPS, [s], [0.0])[0][0]


def test_single_frame_and_two_frame_clips():
    rng = np.random.default_rng(5)
    q = rng.normal(size=(int(OFFS[-1]), 10))
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    # T = 1: every velocity is 0 at any time, the pose is the frame
    gen, _ = ref.generalized(q, OFFS, FPS, [0, 0, 0], [-1.0, 0.0, 2.0])
    for k in ("root_lin_vel", "root_ang_vel", "joint_vel"):
        assert not gen[k].any()
    assert np.array_equal(gen["root_pos"], q[[0] * 3, :3]) and np.array_equal(gen["root_rot"], q[[0] * 3][:, [4, 5, 6, 3]])
    # T = 2: both stencils are the one-sided difference of the two frames, so the velocity is that constant
    a, b = q[1], q[2]
    gen, _ = ref.generalized(q, OFFS, FPS, [1, 1, 1], [0.0, 0.3 / 120.0, 1.0 / 120.0])
    want = (b[[0, 1, 2]] - a[[0, 1, 2]]) / (1.0 * (1.0 / 120.0))
    for r in range(3):
        assert np.array_equal(gen["root_lin_vel"][r], want)
        assert np.array_equal(gen["joint_vel"][r], (b[7:] - a[7:]) / (1.0 * (1.0 / 120.0)))
    assert np.array_equal(gen["root_pos"][0], a[:3]) and np.array_equal(gen["root_pos"][2], b[:3])


def test_frame_times_are_exact_for_the_cross_check_rates():
    """GPU test 4 queries every frame time k / fps of the fps-32 and fps-128 clips and expects the export's rows: (k / fps) * fps
    must be k exactly."""
    for T, f in ((64, 32.0), (65, 128.0)):
        k = np.arange(T, dtype=np.float64)
        assert np.array_equal((k / f) * f, k)
        for kk in range(T):
            ok, (km0, i0, i1, kp1, km1), a, h0, h1 = _plan1(LENS.index(T), kk / f)
            assert ok and i0 == kk and a == 0.0 and km0 == max(kk - 1, 0) and i1 == min(kk + 1, T - 1)
