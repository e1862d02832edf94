"""tests/rotation_edges.py on the CPU: the 50-digit reference is the operation scipy and the IK certificate compute (away from every
edge), every case of the tables sits on the side of its threshold that the table claims, FLOAT_WORST is what plain numpy really
does on the tables, and a restatement with one edge wrong misses the GPU bound by more than 100 x (the grid has teeth)."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R, Slerp

from tests import ik_certificate as ikc
from tests import rotation_edges as E
from tests.rotation_edges import mp, mpf

ANGLES = np.linspace(0.1, 3.0, 7)


def _f(t):
    return np.array([float(x) for x in t])


def test_reference_equals_scipy_away_from_edges():
    worst = 0.0
    for ax in E.AXES:
        for a in ANGLES:
            v = a * ax
            q = E.qexp(E.MP, E.MP.vec(v))
            worst = max(worst, np.abs(_f(q) - R.from_rotvec(v).as_quat(scalar_first=True)).max())
            worst = max(worst, np.abs(_f(E.qlog(E.MP, q)) - v).max())
            worst = max(worst, np.abs(_f(E.qlog(E.MP, E.qneg(q))) - v).max())
            # [V^-1 t, omega] against the certificate's se3_log
            t = np.array([0.1, -0.2, 0.3])
            mine = np.concatenate([_f(E.vinv_t(E.MP, E.MP.vec(v), E.MP.vec(t))), _f(E.qlog(E.MP, q))])
            worst = max(worst, np.abs(mine - ikc.se3_log(_f(q)[None], t[None])[0]).max())
            # slerp against scipy's, pair `a` apart about another axis
            q0 = R.from_rotvec(0.7 * E.OBLIQUE)
            q1 = q0 * R.from_rotvec(a * ax)
            for w in (0.25, 0.5, 0.75):
                want = Slerp([0.0, 1.0], R.concatenate([q0, q1]))(w).as_quat(scalar_first=True)
                got = _f(E.slerp(E.MP, E.MP.vec(q0.as_quat(scalar_first=True)), E.MP.vec(q1.as_quat(scalar_first=True)), E.MP.c(w)))
                worst = max(worst, min(np.abs(got - want).max(), np.abs(got + want).max()))
                got = _f(E.smplx_slerp(E.MP, E.MP.vec(q0.as_quat(scalar_first=True)), E.MP.vec(q1.as_quat(scalar_first=True)), E.MP.c(w)))
                worst = max(worst, min(np.abs(got - want).max(), np.abs(got + want).max()))
    for order in E.BVH_ORDERS:
        e = np.array([0.4, -1.1, 2.3])
        got = _f(E.euler_quat(E.MP, E.MP.vec(e), order))
        want = R.from_euler("".join("XYZ"[o] for o in order), e).as_quat(scalar_first=True)
        worst = max(worst, min(np.abs(got - want).max(), np.abs(got + want).max()))
    print(f"reference vs scipy / certificate: {worst:.2e}")
    assert worst < 1e-14


def test_tables_sit_on_the_branch_they_claim():
    # single rotations: the series arm (a <= 1e-3) and the short sincos kernel (a / 2 <= 1.6), decided on the exact input
    g = E.angle_grid()
    lo, mid, hi = (float(v) for v in E._nbrs(1e-3))
    assert [E.angle_branches(v)[0] for v in (lo, mid, hi)] == [True, True, False]
    lo, mid, hi = (float(v) for v in E._nbrs(3.2))
    assert [E.angle_branches(v)[1] for v in (lo, mid, hi)] == [True, True, False] and all(v in g for v in (lo, mid, hi))
    assert sum(E.angle_branches(v)[0] for v in g) == 12 and sum(not E.angle_branches(v)[1] for v in g) == 7
    lo, mid, hi = (float(v) for v in E._nbrs(183.3464944))
    print("bvh half-angles - 1.6:", [float(mpf(v) * mp.pi / 360 - mpf(1.6)) for v in (lo, mid, hi)])
    assert abs(float(mpf(mid) * mp.pi / 360 - mpf(1.6))) < 1e-9   # the file format has 7 decimals: the channel next to the threshold
    assert sum(bool(abs(mpf(v)) * mp.pi / 360 > mpf(1.6)) for v in E.BVH_DEGREES) >= 6
    # interpolation pairs: dot against 0.9995, never closer than 1e-12 (relative); the side is the one the table names
    for name, r0, r1, linear in E.rotvec_pairs():
        for dt in (np.float64, np.float32):
            q0, q1 = (E.qexp(E.MP, E.MP.vec(r.astype(dt))) for r in (r0, r1))
            d = abs(E.dot(q0, q1))
            rel = d / mpf(E.DOT_EDGE) - 1
            assert abs(rel) > mpf(1e-12), (name, dt)
            if dt is np.float64 or not name.startswith("dot"):   # (float32 rounding of the inputs moves the 1e-9 cases: either side, still > 1e-12)
                assert bool(d > mpf(E.DOT_EDGE)) == linear, (name, float(rel))
            if name.startswith("dot") and dt is np.float64:
                want = float(name[4:9].split("/")[0])
                assert abs(abs(float(rel)) / want - 1) < 1e-3, (name, float(rel))
            if name.split("/")[0] == "pi":   # cos(fl(pi) / 2): 6.1e-17 for the float64 value of pi, -4.4e-8 for the float32 one
                assert abs(E.dot(q0, q1)) < mpf(1e-15 if dt is np.float64 else 1e-7)
    # quaternion pairs of the tracking export: the angle om of the aligned pair against track_slerp's 1e-8
    for name, a, b in E.quat_pairs():
        ma, mb = E.MP.vec(a), E.MP.vec(b)   # (the angle between the rotations: a rounded unit quaternion has |q|^2 = 1 +- 2e-16)
        d = abs(E.dot(ma, mb)) / mp.sqrt(E.dot(ma, ma) * E.dot(mb, mb))
        om = mp.acos(min(d, mpf(1)))
        base = name.split("/")[0]
        if base.startswith("om="):   # the two float64 neighbours of the threshold, by the dot the kernel itself computes (exact here)
            df = float(np.dot(a, b))
            assert E.dot(ma, mb) == mpf(df) and df == (1.0 if base == "om=0" else float(np.nextafter(1.0, 0.0)))
            assert (mp.acos(mpf(df)) < mpf(1e-8)) == (base == "om=0") and mp.acos(mpf(float(np.nextafter(1.0, 0.0)))) > mpf(1.49e-8)
        elif base in ("same", "1e-9", "4e-12"):
            assert om < mpf(1e-8), name
        elif base == "2e-8":
            assert abs(float(om) / 1e-8 - 1) < 1e-6, (name, float(om))   # on the threshold as closely as a float64 quaternion can be
        else:
            assert om > mpf(1e-8), name
        if base == "pi":
            assert E.dot(E.MP.vec(a), E.MP.vec(b)) == 0
    # track_ang_vel: n against 1e-12 and w against 0, on the exact rows (q is the identity: w and v are p's components)
    sides = {}
    for name, p in E.ang_vel_cases():
        pm = E.MP.vec(p)
        r = E.qmul(pm, E.qconj(E.MP.vec([1.0, 0.0, 0.0, 0.0])))
        assert r == pm
        n = mp.sqrt(E.dot(r[1:], r[1:]))
        sides[name] = (int(mp.sign(n - mpf(1e-12))), int(mp.sign(r[0])))
    assert [sides[k][0] for k in ("n<1e-12", "n=1e-12", "n>1e-12", "n=0", "w=0", "w<0/n=1e-12")] == [-1, 0, 1, -1, 1, 0]
    assert abs(float(mp.sqrt(sum(mpf(float(v)) ** 2 for v in E.ang_vel_cases()[3][1][1:])) / mpf(1e-12) - 1)) < 1e-15
    assert [sides[k][1] for k in ("w=0", "w=+tiny", "w=-tiny", "w=-0.0", "w<0", "n=0/w<0")] == [0, 1, -1, 0, -1, -1]
    # the resampling weights of the tracking clips: 0, .25, .5, .75 and, on every pair, 2^-20 and 1 - 2^-20
    ti = E.family_inputs("track")[0]
    seen = set()
    for s_ in range(len(ti["offs"]) - 1):
        for k in range(int(ti["out_offs"][s_ + 1] - ti["out_offs"][s_])):
            u = k * float(ti["ratio"][s_])
            seen.add(u - np.floor(u))
    assert seen == set(E.WEIGHTS)
    # rot_to_dof: |xyz| of the float32 inputs against 1e-5 at +-1e-3, the clamp cases outside / inside the range
    axes, hb, nbody, lo32, hi32, limited, _ = E.g1_hinges()
    assert limited.all()   # unitree_g1 has no hinge without limits
    inp = E.family_inputs("rot_to_dof")[0]
    ref = E.reference("rot_to_dof")["dof"][0]
    for f, lab in enumerate(inp["labels"]):
        for d, b in enumerate(hb):
            x = E.MP.vec(inp["rot"][f, b - 1])
            n = mp.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
            if lab[0] == "len":
                assert bool(n > mpf(E.ROT_TO_DOF_EPS)) == (lab[1] > 1e-5), lab
                assert lab[1] in (0.0, 1e-7, 1e-3) or 5e-4 < abs(float(n / mpf(E.ROT_TO_DOF_EPS) - 1)) < 2e-3
            elif lab[0] == "clamp":
                outside = (lab[1] == 0) == (lab[2] < 0)
                lim = float((lo32, hi32)[lab[1]][d])
                assert (ref[f, d] == lim) == outside, (lab, d, ref[f, d], lim)
            elif lab == ("scaled", 0.5, "len"):
                assert n < mpf(E.ROT_TO_DOF_EPS) and ref[f, d] == min(max(0.0, lo32[d]), hi32[d])


@pytest.mark.parametrize("robot", ["unitree_g1", "galaxea_r1pro"])
def test_evaluate_turns_sit_on_the_branch_they_claim(robot):
    """gmr_evaluate's task errors: w of the relative quaternion against kLieEps (the sign rule) and th^2 against kLieEps (c2 = 1/12),
    computed at 50 digits from the key-points and the qpos the kernel receives; the reference equals the certificate."""
    s = E.evaluate_setup(robot)
    ref = E.reference("evaluate_" + robot)
    eps, pi = mpf(E.K_LIE_EPS), E.TURN_PI
    assert len(s["frames"]) >= 3 * len(E.TURN_ANGLES) * 3 and s["cert"].planar == (robot == "galaxea_r1pro")
    rows = {fr["row"] for fr in s["frames"]}
    assert len(rows) == sum(len(s["cert"].tables[k]) for k in s["cert"].used_tables())   # every task of every table in use, one at a time
    for f, fr in enumerate(s["frames"]):
        a, w, th2 = fr["angle"], ref["w"][f], ref["th2"][f]
        # th^2 against kLieEps: below for the tiny turns, 1e-9 either side of sqrt(kLieEps), on it to 1e-10 (relative) in between
        if a < 1e-6:
            assert th2 < eps, (fr, float(th2))
        elif a == E.SQRT_LIE * (1 - 1e-9):
            assert th2 < eps and abs(float(th2 / eps - 1) + 2e-9) < 1e-9, (fr, float(th2 / eps - 1))
        elif a == E.SQRT_LIE:
            assert abs(float(th2 / eps - 1)) < 1e-9, (fr, float(th2 / eps - 1))
        elif a == E.SQRT_LIE * (1 + 1e-9):
            assert th2 > eps and abs(float(th2 / eps - 1) - 2e-9) < 1e-9, (fr, float(th2 / eps - 1))
        else:
            assert th2 > eps
        # |w| against kLieEps, and the sign of w where it is a number
        if a == pi:
            assert abs(w) < mpf(1e-15)                      # zero to rounding: the sign is a convention
        elif abs(a - pi) == abs((pi - 2e-11) - pi) or abs(a - pi) < 3e-11:
            assert mpf(0.9e-11) < abs(w) < mpf(1.1e-11) and (w > 0) == (a < pi), (fr, float(w))
        elif a == pi - 2e-10 * (1 - 1e-3):
            assert 0 < w < eps and abs(float(w / eps - 1) + 1e-3) < 1e-4, (fr, float(w))
        elif a == pi - 2e-10 * (1 + 1e-3):
            assert w > eps and abs(float(w / eps - 1) - 1e-3) < 1e-4, (fr, float(w))
        else:
            assert abs(w) > eps and (w > 0) == (a < pi), (fr, float(w))
    # the same operation as the certificate's (numpy float64 with thresholds), on a sample of the frames away from pi's sign
    cert, nt0, worst = s["cert"], len(s["cm"].tasks[0]), 0.0
    for f in range(0, len(s["frames"]), 5):
        fr = s["frames"][f]
        if abs(fr["angle"] - pi) < 1e-10:
            continue
        k = 0 if fr["row"] < nt0 else 1
        e = cert.task_errors(k, s["qpos"], cert.prepare_targets(s["pos"][f], s["quat"][f], s["names"]))[fr["row"] - k * nt0]
        worst = max(worst, float(np.abs(e - ref["task_err"][0][f]).max()))
    xp, xq = cert.fk(s["hinge_qpos"])
    worst = max(worst, float(np.abs(xp - ref["xpos"][0]).max()), float(np.abs(xq - ref["xquat"][0]).max()))
    print(f"evaluate reference vs certificate ({robot}): {worst:.2e}")
    assert worst < 1e-14
    hv = s["hinge_values"]
    assert sum(abs(v) > 3.2 for v in hv) == 2 and 3.2 in hv and -3.2 in hv   # sincos_fk's ballot: half-angle 1.6 and one ulp beyond


def test_plain_float_worst():
    """FLOAT_WORST is what plain numpy does: every committed value is at least the measured one, and no more than 3 x it (one digit, rounded up, plus head-room)."""
    bad = []
    for fam in E.FAMILIES:
        ref, pf = E.reference(fam), E.plain_float(fam)
        for out in E.FLOAT_WORST[fam]:
            w = E.family_worst(fam, out, pf[out], ref)
            print(f"FLOAT_WORST {fam:24s} {out:14s} measured {w:.3e} committed {E.FLOAT_WORST[fam][out]:.3e}")
            if not w <= E.FLOAT_WORST[fam][out] <= max(3.0 * w, 1e-300):
                bad.append((fam, out, w))
    assert not bad, bad


def _miss(fam, out, variant, nan=np.inf):
    """How many times the bound a wrong restatement (plain float64) misses it by, at its worst element."""
    ref = E.reference(fam)[out]
    return max(float(np.nan_to_num(np.abs(v - r) / E.bound(fam, out, r), nan=nan).max()) for v, r in zip(variant, ref))   # (a NaN is a miss, unless told to look past it)


def test_controls_one_wrong_edge_fails_by_100x(monkeypatch):
    # the honest plain-float restatement passes its own bound everywhere
    for fam in ("smplx_chain3", "smplx_small_chain3", "smplx_resample_chain3", "track", "rot_to_dof"):
        pf = E.plain_float(fam)
        for out in pf:
            eps = E.EPS32 if fam == "rot_to_dof" else E.EPS64
            ref = E.reference(fam)[out]
            assert all((np.abs(v - r) <= E.bound(fam, out, r, eps)).all() for v, r in zip(pf[out], ref)), (fam, out)
    # (1) from_rotvec's series below 1e-3 with 1/24 in place of 1/48
    true_qexp = E.qexp

    def bad_series(B, v):
        a2 = E.dot(v, v)
        if B.sqrt(a2) <= B.c(1e-3):
            k = B.c(0.5) - a2 / B.c(24)
            return (B.cos(B.sqrt(a2) * B.c(0.5)), k * v[0], k * v[1], k * v[2])
        return true_qexp(B, v)
    monkeypatch.setattr(E, "qexp", bad_series)
    m1 = _miss("smplx_small_chain3", "quat", E.plain_float("smplx_small_chain3")["quat"])
    monkeypatch.setattr(E, "qexp", true_qexp)
    # (2) the dot < 0 flip dropped from the slerp
    true_slerp = E.slerp

    def no_flip(B, q0, q1, a):
        w0, w1 = E.slerp_weights(B, max(E.dot(q0, q1), -B.c(1)), a)   # d keeps its sign: the long arc, a finite wrong quaternion
        return E.qnormalise(B, tuple(w0 * x + w1 * y for x, y in zip(q0, q1)))
    monkeypatch.setattr(E, "slerp", no_flip)
    # (the long arc between q and -q has no midpoint: those rows are NaN and are looked past, the finite wrong rows are what counts)
    m2 = _miss("track", "root_rot", E.plain_float("track")["root_rot"], nan=0.0)
    monkeypatch.setattr(E, "slerp", true_slerp)
    # (3) atan2(n, w) without making w non-negative
    true_one = E.rot_to_dof_one

    def no_abs(B, q, axis, lo, hi):
        x, y, z, w = q
        n = B.sqrt(x * x + y * y + z * z)
        if not n > B.c(E.ROT_TO_DOF_EPS):
            return min(max(B.c(0), B.c(lo)), B.c(hi))
        ang = B.c(2) * B.atan2(n, w)
        if (x * axis[0] + y * axis[1] + z * axis[2]) / n < 0:
            ang = -ang
        return min(max(ang, B.c(lo)), B.c(hi))
    monkeypatch.setattr(E, "rot_to_dof_one", no_abs)
    ref = E.reference("rot_to_dof")["dof"][0]
    v = E.plain_float("rot_to_dof")["dof"][0]
    m3 = float((np.abs(v - ref) / E.bound("rot_to_dof", "dof", ref, E.EPS32)).max())   # (_miss is for float64 outputs)
    monkeypatch.setattr(E, "rot_to_dof_one", true_one)
    # (4) the linear blend of the SMPL-X slerp moved from 0.9995 to 0.999: the pair 1e-3 below the edge changes arm
    true_sm = E.smplx_slerp

    def moved_edge(B, q0, q1, a):
        d = E.dot(q0, q1)
        if abs(d) > B.c(0.999) and not abs(d) > B.c(0.9995):
            q1 = E.qneg(q1) if d < 0 else q1
            q = E.qnormalise(B, tuple(x + a * (y - x) for x, y in zip(q0, q1)))
            return E.qneg(q) if q[0] < 0 else q
        return true_sm(B, q0, q1, a)
    monkeypatch.setattr(E, "smplx_slerp", moved_edge)
    m4 = _miss("smplx_resample_chain3", "quat", E.plain_float("smplx_resample_chain3")["quat"])
    monkeypatch.setattr(E, "smplx_slerp", true_sm)
    print(f"controls miss the bound by: series 1/24 {m1:.3g} x, no flip {m2:.3g} x, w not made >= 0 {m3:.3g} x, blend edge moved {m4:.3g} x")
    assert min(m1, m2, m3, m4) >= 100.0
