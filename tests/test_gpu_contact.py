"""Foot-contact labels and slide statistics (gmr_motion_contacts, Engine.motion_contacts, dataset.tracking_from_qpos with
contact_bodies) on the GPU, against the contract in include/gmr_amd.h restated as a Python loop (tests/contact_reference.py).

The synthetic inputs are exactly representable -- z in multiples of 2^-10 (one hand-made value: one float32 ulp above a
threshold), thresholds 2^-5 and 2^-4, velocity components in multiples of 2^-4, speeds 0.25 and 0.5 -- so every comparison of the
definition is exact and labels, counts, depth_max and base must equal the reference exactly.  slide_step_max may differ by a 1-ulp
sqrt (2 * 2^-52 relative); slide_sum is a sum of at most M_s non-negative terms, each with one sqrt rounding, taken in another
order than the reference's: within (M_s + 2) * 2^-52 * sum of math.fsum of the reference's terms.

One launch holds clips of 0, 1, 2, 63, 64, 65, 129 and 200 frames (the edges of the 64-frame tile, one to four tiles) and three
contact bodies with non-adjacent, unsorted ids of the G1 model."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import contact_reference as ref  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.util import compiled  # noqa: E402

LENS = [0, 1, 2, 63, 64, 65, 129, 200]
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
M = int(OFFS[-1])
U = 2.0 ** -10                                   # the unit of every height and position
HON, HOFF, SON, SOFF = 2.0 ** -5, 2.0 ** -4, 0.25, 0.5    # 32 U and 64 U; sum of squared velocity units <= 16 and <= 64
GROUND_UNITS, GROUND_Z = 256, 0.25
HOFF_UNITS = [16, 0, 3]
HEIGHT_OFFSET = [u * U for u in HOFF_UNITS]
BODY_IDS = [14, 3, 29]
SLOW = [(0, 0, 0), (4, 0, 0), (2, 2, 2), (0, 3, 2), (-4, 0, 0), (1, -2, 3)]      # sum of squares <= 16
MID = [(4, 1, 0), (8, 0, 0), (4, 4, 4), (-6, 2, 1), (0, 0, -8)]                 # 17 .. 64
FAST = [(8, 1, 0), (9, 0, 0), (5, 5, 5), (0, -7, 5)]                            # >= 65
FILL = 0xA5
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
MODES = {"fixed": (ref.GROUND_FIXED, GROUND_Z), "clip_min": (ref.GROUND_CLIP_MIN, 0.0)}


def DEV():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _engine():
    from gmr_amd.engine import Engine
    return Engine(compiled("smplx", "unitree_g1"), device=0)


# ------------------------------------------------------------------ the inputs
def _frame(rng, kind):
    """(height above the ground in units, velocity in units) of an entering ('E'), undecided ('U') or leaving ('L') frame."""
    pick = lambda table: table[rng.integers(len(table))]  # noqa: E731
    if kind == "E":
        return int(rng.integers(-16, 33)), pick(SLOW)
    if kind == "U":
        if rng.random() < 0.5:
            return int(rng.integers(33, 65)), pick(SLOW + MID)
        return int(rng.integers(-16, 33)), pick(MID)
    if rng.random() < 0.5:
        return int(rng.integers(65, 300)), pick(SLOW + MID)
    return int(rng.integers(-16, 100)), pick(FAST)


@functools.lru_cache(maxsize=None)
def _patterns(seed, hand_made=True):
    """pos, vel float32 [M, nbody, 3]: every body random, the three contact columns random walks of entering, undecided and
    leaving frames (heights measured from GROUND_Z + HEIGHT_OFFSET), plus the hand-made cases."""
    nb = compiled("smplx", "unitree_g1").robot.nbody
    rng = np.random.default_rng(seed)
    pos = (rng.integers(-2000, 2000, (M, nb, 3)) * U).astype(np.float32)
    vel = (rng.integers(-12, 13, (M, nb, 3)) * 2.0 ** -4).astype(np.float32)

    def put(g, c, hk, v):
        pos[g, BODY_IDS[c], 2] = np.float32((GROUND_UNITS + HOFF_UNITS[c] + hk) * U)
        vel[g, BODY_IDS[c]] = np.asarray(v, np.float32) * np.float32(2.0 ** -4)

    for s, n in enumerate(LENS):
        a = int(OFFS[s])
        for c in range(3):
            kinds = rng.choice(["E", "U", "L"], size=n, p=[0.12, 0.76, 0.12])
            xy = rng.integers(-1000, 1000, 2) + np.cumsum(rng.integers(-6, 7, (n, 2)), axis=0)
            for k in range(n):
                put(a + k, c, *_frame(rng, kinds[k]))
                pos[a + k, BODY_IDS[c], :2] = (xy[k] * U).astype(np.float32)
    if hand_made:
        a = int(OFFS[7])   # the clip of 200 frames
        put(a + 0, 0, 32, (0, 0, 0))                                   # h == height_on exactly: enters; the clip starts in contact
        for k in range(1, 10):
            put(a + k, 0, 40, (0, 0, 0))                               # undecided
        put(a + 10, 0, 100, (0, 0, 0))                                 # leaves
        put(a + 11, 0, 32, (0, 0, 0))
        z = pos[a + 11, BODY_IDS[0], 2]
        pos[a + 11, BODY_IDS[0], 2] = np.nextafter(z, np.float32(np.inf))   # one float32 ulp above height_on: does not enter
        put(a + 12, 0, 32, (4, 0, 0))                                  # h == height_on and s2 == speed_on^2 exactly: enters
        put(a + 13, 0, 10, (4, 1, 0))                                  # one notch faster: undecided, stays on
        put(a + 14, 0, 100, (0, 0, 0))
        put(a + 59, 0, 100, (0, 0, 0))
        put(a + 60, 0, 0, (0, 0, 0))                                   # enter at 60, undecided 61 .. 70 (across the tile edge), leave at 71
        for k in range(61, 71):
            put(a + k, 0, 50, (0, 0, 0))
        put(a + 71, 0, 100, (0, 0, 0))
        put(a + 62, 1, 100, (0, 0, 0))
        put(a + 63, 1, 100, (0, 0, 0))
        put(a + 64, 1, 0, (0, 0, 0))                                   # a touchdown at frame 64: lane 0 of the second tile
        put(a + 62, 2, 0, (0, 0, 0))
        put(a + 63, 2, 0, (0, 0, 0))
        put(a + 64, 2, 0, (4, 1, 0))                                   # the contact pair (63, 64) slides 3 U and 4 U: 5 U
        put(a + 65, 2, 100, (0, 0, 0))
        pos[a + 63, BODY_IDS[2], :2] = np.float32(100 * U), np.float32(200 * U)
        pos[a + 64, BODY_IDS[2], :2] = np.float32(103 * U), np.float32(204 * U)
        b = int(OFFS[6])   # the clip of 129 frames: decided on lane 63, a whole undecided tile, decided again on lane 0 of the third
        put(b + 62, 0, 100, (0, 0, 0))
        put(b + 63, 0, 0, (0, 0, 0))
        for k in range(64, 128):
            put(b + k, 0, 50, (0, 0, 0))
        put(b + 128, 0, 100, (0, 0, 0))
        put(int(OFFS[1]), 0, 0, (0, 0, 0))                             # the clip of one frame: in contact
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))   # (a copy: the shared patterns are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV())


def _shapes(S=len(LENS), Cn=3, rows=M):
    return {"contact": ((rows, Cn), U8), "frames": ((S, Cn), I32), "touchdowns": ((S, Cn), I32), "slide_sum": ((S, Cn), F64),
            "slide_step_max": ((S, Cn), F64), "depth_max": ((S, Cn), F64), "airborne_frames": ((S,), I32), "base": ((S,), F64)}


def _sentinel_out(names=None):
    out = {}
    for k, (sh, dt) in _shapes().items():
        if names is None or k in names:
            out[k] = torch.empty(sh, dtype=dt, device=DEV())
            out[k].view(U8).fill_(FILL)
    return out


def _run(pos, vel, mode, with_offset, out=None):
    """Engine.motion_contacts on host arrays -> host arrays by name."""
    res = _engine().motion_contacts((_dev(pos), _dev(vel)), OFFS, BODY_IDS, HEIGHT_OFFSET if with_offset else None,
                                    ground="clip_min" if mode == "clip_min" else GROUND_Z, height_on=HON, height_off=HOFF,
                                    speed_on=SON, speed_off=SOFF, out=out)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _reference(pos, vel, mode, with_offset):
    gm, gz = MODES[mode]
    return ref.contacts(pos, vel, OFFS, BODY_IDS, HEIGHT_OFFSET if with_offset else None, gm, gz, HON, HOFF, SON, SOFF)


@functools.lru_cache(maxsize=None)
def _clean(mode, with_offset=True):
    """(reference, GPU answer) of the unpoisoned inputs: computed once, shared, never modified."""
    pos, vel = _patterns(1)
    return _reference(pos, vel, mode, with_offset), _run(pos, vel, mode, with_offset)


def _check(got, want, clips=range(len(LENS)), what=""):
    """The GPU answer against the reference on the given clips: exact, but for the two slide figures (module docstring)."""
    for s in clips:
        a, b = int(OFFS[s]), int(OFFS[s + 1])
        assert np.array_equal(got["contact"][a:b], want["contact"][a:b]), (what, s, "contact")
        for k in ("frames", "touchdowns", "airborne_frames"):
            assert np.array_equal(got[k][s], want[k][s]), (what, s, k, got[k][s], want[k][s])
        for k in ("depth_max", "base"):
            assert np.array_equal(got[k][s], want[k][s], equal_nan=True), (what, s, k, got[k][s], want[k][s])
        for c in range(3):
            g, w = float(got["slide_step_max"][s, c]), float(want["slide_step_max"][s, c])
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 2 * 2.0 ** -52 * w, (what, s, c, "slide_step_max", g, w)
            total = math.fsum(float(t) for t in want["slide_terms"][s][c])
            g = float(got["slide_sum"][s, c])
            assert (math.isnan(g) and math.isnan(total)) or abs(g - total) <= (b - a + 2) * 2.0 ** -52 * total, (what, s, c, "slide_sum", g, total)


def _bytes(d):
    return {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1) for k, v in d.items()}


# ------------------------------------------------------------------ 1: labels and statistics
@pytest.mark.parametrize("with_offset", [True, False], ids=["height_offset", "null_offset"])
@pytest.mark.parametrize("mode", ["fixed", "clip_min"])
def test_labels_and_statistics_equal_the_reference(mode, with_offset):
    pos, vel = _patterns(1)
    want = _reference(pos, vel, mode, with_offset)
    out = _sentinel_out()   # caller-owned, pre-filled: every element must be written
    got = _run(pos, vel, mode, with_offset, out=out)
    _check(got, want, what=(mode, with_offset))
    assert want["contact"].sum() > 100 and want["touchdowns"].sum() > 10 and (want["slide_sum"] > 0).sum() > 10   # the case says something
    assert got["base"][0] == GROUND_Z if mode == "fixed" else math.isnan(got["base"][0])   # the clip without frames
    for k in ("frames", "touchdowns", "slide_sum", "slide_step_max", "depth_max", "airborne_frames"):
        assert not np.any(got[k][0]), k
    again = _run(pos, vel, mode, with_offset, out=_sentinel_out())
    assert all(np.array_equal(a, b) for a, b in zip(_bytes(got).values(), _bytes(again).values()))   # two calls: identical bytes
    if mode == "fixed" and with_offset:   # the hand-made cases say what they were made to say
        a, b, c = int(OFFS[7]), int(OFFS[6]), got["contact"]
        assert c[a:a + 15, 0].tolist() == [1] * 10 + [0, 0, 1, 1, 0]
        assert c[a + 59, 0] == 0 and c[a + 60:a + 71, 0].tolist() == [1] * 11 and c[a + 71, 0] == 0
        assert c[a + 62:a + 65, 1].tolist() == [0, 0, 1]
        assert c[a + 62:a + 66, 2].tolist() == [1, 1, 1, 0] and np.float64(5 * U) in [np.float64(t) for t in want["slide_terms"][7][2]]
        assert c[b + 62, 0] == 0 and c[b + 63:b + 128, 0].tolist() == [1] * 65 and c[b + 128, 0] == 0
        assert c[int(OFFS[1]), 0] == 1 and got["touchdowns"][1, 0] == 1 and got["frames"][1, 0] == 1
        assert (got["depth_max"] > 0).any()


def test_outputs_left_out_are_not_computed_and_the_others_do_not_change():
    pos, vel = _patterns(1)
    _, full = _clean("clip_min")
    some = _sentinel_out(names=("contact", "slide_sum", "base"))
    untouched = _sentinel_out(names=("frames", "touchdowns", "slide_step_max", "depth_max", "airborne_frames"))
    got = _run(pos, vel, "clip_min", True, out=some)
    assert set(got) == {"contact", "slide_sum", "base"}
    for k in got:
        assert np.array_equal(_bytes(got)[k], _bytes(full)[k]), k
    for k, t in untouched.items():
        assert bool((t.view(U8) == FILL).all()), k


# ------------------------------------------------------------------ 2: non-finite elements
@functools.lru_cache(maxsize=None)
def _poison_frame():
    """A frame of the 65-frame clip whose column 1 is in contact with both neighbours in contact, in both modes: poisoning it shows."""
    a = int(OFFS[5])
    labels = [_clean(m)[0]["contact"][a:a + 65, 1] for m in MODES]
    ks = [k for k in range(1, 64) if all(l[k - 1] and l[k] and l[k + 1] for l in labels)]
    assert ks, "the random walk of clip 5, column 1 holds no run of three contact frames"
    return a + ks[0]


@pytest.mark.parametrize("mode", ["fixed", "clip_min"])
@pytest.mark.parametrize("field", ["z", "vx"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_non_finite_element_stays_in_its_clip_and_column(value, field, mode):
    want_clean, clean = _clean(mode)
    g = _poison_frame()
    pos, vel = (a.copy() for a in _patterns(1))
    (pos if field == "z" else vel)[g, BODY_IDS[1], 2 if field == "z" else 0] = value
    want = _reference(pos, vel, mode, True)
    got = _run(pos, vel, mode, True, out=_sentinel_out())
    _check(got, want, clips=[5], what=(value, field, mode))   # the poisoned clip: what the definition says
    a, b = int(OFFS[5]), int(OFFS[6])
    cb, gb = _bytes(clean), _bytes(got)
    for k, (sh, dt) in _shapes().items():   # every output of every other clip: byte for byte the clean run's
        row = int(np.prod(sh[1:])) * torch.empty((), dtype=dt).element_size()
        lo, hi = (a * row, b * row) if k == "contact" else (5 * row, 6 * row)
        assert np.array_equal(np.delete(gb[k], np.s_[lo:hi]), np.delete(cb[k], np.s_[lo:hi])), k
    assert got["contact"][g, 1] == 0 or (value == -np.inf and field == "z" and mode == "fixed")   # (-inf is below every threshold)
    assert not np.array_equal(got["contact"][a:b], clean["contact"][a:b]) or value == -np.inf
    if mode == "fixed":   # only its own column changes, plus airborne_frames
        for k in ("frames", "touchdowns", "slide_sum", "slide_step_max", "depth_max"):
            assert np.array_equal(got[k][5, [0, 2]].view(np.uint8), clean[k][5, [0, 2]].view(np.uint8)), k
        assert np.array_equal(got["contact"][a:b][:, [0, 2]], clean["contact"][a:b][:, [0, 2]])
        assert got["base"][5] == GROUND_Z
    if mode == "clip_min" and field == "z" and math.isnan(value):
        assert math.isnan(got["base"][5]) and not got["contact"][a:b].any() and got["airborne_frames"][5] == 65
        assert not got["frames"][5].any() and not got["depth_max"][5].any() and not got["slide_sum"][5].any()


# ------------------------------------------------------------------ 3: bad arguments
def test_bad_arguments_are_refused_with_a_message_and_launch_nothing():
    from gmr_amd import engine
    eng = _engine()
    pos, vel = _patterns(1)
    out = _sentinel_out()
    ci, _, keep = engine._contact_input(eng, (_dev(pos), _dev(vel)), OFFS, BODY_IDS, HEIGHT_OFFSET, "clip_min", HON, HOFF, SON, SOFF, out)
    ci.stream = torch.cuda.current_stream().cuda_stream
    fixed = {"ground_mode": 0}
    bad = [({"height_on": np.nan}, -1), ({"height_off": np.inf}, -1), ({"speed_on": np.nan}, -1), ({"speed_off": -np.inf}, -1),
           ({"height_on": HOFF + U}, -1), ({"speed_on": -0.125}, -1), ({"speed_on": SOFF + 0.125}, -1),
           ({"n_contact": 0}, -1), ({"n_contact": -3}, -1), ({"n_contact": 65}, -3), ({"ground_mode": 2}, -1), ({"ground_mode": -1}, -1),
           ({**fixed, "ground_z": np.nan}, -1), ({**fixed, "ground_z": np.inf}, -1),
           ({"body_pos_w": None}, -1), ({"body_lin_vel_w": None}, -1), ({"out_offsets": None}, -1), ({"body_ids": None}, -1),
           ({"n_rows": -1}, -1), ({"n_seq": -1}, -1)]
    for change, rc in bad:
        keep_vals = {k: getattr(ci, k) for k in change}
        for k, v in change.items():
            setattr(ci, k, v)
        got = eng._lib.gmr_motion_contacts(eng._h, C.byref(ci))
        msg = eng._lib.gmr_last_error(eng._h)
        for k, v in keep_vals.items():
            setattr(ci, k, v)
        assert got == rc and msg and len(msg) > 5, (change, got, msg)
    for change in ({"n_rows": 0}, {"n_seq": 0}):   # nothing to do: GMR_OK, and no launch either
        keep_vals = {k: getattr(ci, k) for k in change}
        for k, v in change.items():
            setattr(ci, k, v)
        assert eng._lib.gmr_motion_contacts(eng._h, C.byref(ci)) == 0
        for k, v in keep_vals.items():
            setattr(ci, k, v)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k
    assert eng._lib.gmr_motion_contacts(eng._h, C.byref(ci)) == 0   # the struct itself was good
    torch.cuda.synchronize()
    assert np.array_equal(out["contact"].cpu().numpy(), _clean("clip_min")[1]["contact"])
    with pytest.raises(engine.EngineError, match="height_on"):
        eng.motion_contacts((_dev(pos), _dev(vel)), OFFS, BODY_IDS, height_on=0.06, height_off=0.05)
    with pytest.raises(ValueError):
        eng.motion_contacts((_dev(pos), _dev(vel)), OFFS, [0, eng.nbody])   # a host list of ids is range-checked
    empty = eng.motion_contacts((_dev(pos[:0]), _dev(vel[:0])), [0, 0, 0], BODY_IDS)   # no rows: no launch, every clip empty
    assert empty["contact"].shape == (0, 3) and not empty["frames"].any() and bool(torch.isnan(empty["base"]).all())


# ------------------------------------------------------------------ 4: stream order (the entry is outside the 27 of the shared suite)
class ContactCase(so.Case):
    """The launch of the tests above with everything it reads in two versions: other patterns, other bodies, other height offsets
    behind the same offsets, and in the struct other thresholds and the other ground mode.  Both versions are in range."""
    entry, launches, h2d = "gmr_motion_contacts", 1, 0
    struct_values = True

    def __init__(self):
        super().__init__()
        (pos, vel), (dpos, dvel) = _patterns(1), _patterns(2, hand_made=False)
        self.dev_in = {"body_pos_w": (_dev(pos), _dev(dpos)), "body_lin_vel_w": (_dev(vel), _dev(dvel)),
                       "out_offsets": (_dev(OFFS), _dev(OFFS)), "body_ids": (_dev(BODY_IDS, I32), _dev([6, 31, 20], I32)),
                       "height_offset": (_dev(HEIGHT_OFFSET, F64), _dev([0.0, 5 * U, 9 * U], F64))}
        self.out_spec = {k + "_out": v for k, v in _shapes().items()}

    def new_struct(self):
        from gmr_amd import _native
        return _native.ContactInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.n_rows, st.n_seq, st.n_contact = M, len(LENS), 3
        st.ground_mode, st.ground_z = (ref.GROUND_FIXED, GROUND_Z + 8 * U) if decoy else (ref.GROUND_CLIP_MIN, 0.0)
        st.height_on, st.height_off = (HON / 2, HON) if decoy else (HON, HOFF)
        st.speed_on, st.speed_off = (0.125, 0.375) if decoy else (SON, SOFF)

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = _engine()
        return eng._lib.gmr_motion_contacts(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = ContactCase()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert spin_ms >= max(so.SPIN_MIN_MS, min(so.SPIN_MAX_MS, 10.0 * ser["ms"])) - 1e-9
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    for k in ("dev_decoy", "host_decoy"):
        assert not so.same(ser[k], ser["true"]), f"the {k} answer equals the true one: the case could not tell an ordering error"
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


def test_stream_order_behind_a_late_producer():
    """Issued behind a producer that is still running, with no host synchronisation and its struct overwritten on return, the
    call computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case()
    want = _clean("clip_min")[1]
    assert all(np.array_equal(ser["true"][k + "_out"], v) for k, v in _bytes(want).items())   # the serial answer is the tests' answer
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_contacts: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
          f"returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not so.same(r["answer"], ser["dev_decoy"]) and not so.same(r["answer"], ser["host_decoy"])
    assert r["returned_before_producer"]


def test_stream_order_control_sees_the_decoy():
    """The harness can fail: issued on a stream that does not wait for the producer, the call sees the decoy device inputs."""
    case, ser, cycles, _ = _stream_case()
    r = so.run_late(case, DEV(), cycles, control=True)
    assert not r["vacuous"] and r["overtook_producer"], "the producer had finished before the control call did: the run shows nothing"
    assert so.same(r["answer"], ser["dev_decoy"]), f"differs from the decoy answer in {so.differing(r['answer'], ser['dev_decoy'])}"


# ------------------------------------------------------------------ 5: end to end
FEET = {"unitree_g1": ["left_ankle_roll_link", "right_ankle_roll_link"], "booster_t1": ["left_foot_link", "right_foot_link"]}
E2E_OFFS = np.array([0, 80, 160], dtype=np.int64)


def _stand_and_lift(robot):
    """Two clips at 30 Hz: standing at the rest pose for 40 frames, the root raised over the next 20 (by 0.25 m and by 0.125 m)
    and lowered again over the last 20."""
    q0 = np.asarray(compiled("smplx", robot).robot.qpos0, dtype=np.float64)
    up = np.linspace(0.0, 1.0, 21)[1:]
    lift = np.concatenate([np.zeros(40), up, up[::-1] - up[0]])
    q = np.tile(q0, (160, 1))
    q[:80, 2] += 0.25 * lift
    q[80:, 2] += 0.125 * lift
    q[80:, 0] += 1.0
    return torch.from_numpy(q).to(DEV())


def _check_track_clip(d, names, model_names):
    from gmr_amd import dataset
    n = d["body_pos_w"].shape[0]
    ids = [list(model_names).index(b) for b in names]
    want = ref.contacts(d["body_pos_w"], d["body_lin_vel_w"], [0, n], ids, None, ref.GROUND_CLIP_MIN, 0.0, 0.03, 0.05, 0.3, 0.6)
    assert d["contact"].dtype == np.uint8 and d["contact"].shape == (n, 2) and d["contact_body_names"] == names
    assert np.array_equal(d["contact"], want["contact"])
    st = d["contact_stats"]
    assert set(st) == set(dataset.CONTACT_STATS)
    for k in ("frames", "touchdowns", "depth_max"):
        assert st[k].shape == (2,) and np.array_equal(st[k], want[k][0]), k
    assert st["base"] == want["base"][0] and d["airborne_frames"] == want["airborne_frames"][0]
    for c in range(2):
        w = float(want["slide_step_max"][0, c])
        assert abs(float(st["slide_step_max"][c]) - w) <= 2 * 2.0 ** -52 * w
        total = math.fsum(float(t) for t in want["slide_terms"][0][c])
        assert abs(float(st["slide_sum"][c]) - total) <= (n + 2) * 2.0 ** -52 * total
    apex = int(round(59 / 30.0 * 50.0))
    assert d["contact"][0].tolist() == [1, 1] and d["contact"][apex].tolist() == [0, 0]   # both feet down at the start, off at the apex
    assert d["airborne_frames"] > 0 and (st["touchdowns"] >= 1).all() and (st["frames"] >= 60).all()   # (1.3 s of standing at 50 Hz)


def test_tracking_from_qpos_labels_the_feet():
    from gmr_amd import GeneralMotionRetargeting, dataset
    g = GeneralMotionRetargeting("smplx", "unitree_g1", device=0)
    qpos = _stand_and_lift("unitree_g1")
    plain = dataset.tracking_from_qpos(g, qpos, E2E_OFFS, 30.0, 50.0)
    got = dataset.tracking_from_qpos(g, qpos, E2E_OFFS, 30.0, 50.0, contact_bodies=FEET["unitree_g1"])
    assert len(got) == len(plain) == 2
    for d, p in zip(got, plain):
        assert set(d) - set(p) == {"contact", "contact_body_names", "contact_stats", "airborne_frames"} and set(p) < set(d)
        for k in dataset.TRACK_ARRAYS:   # the ten arrays of the export: byte-identical with and without the labels
            assert d[k].dtype == p[k].dtype and np.array_equal(d[k].view(np.uint8), p[k].view(np.uint8)), k
        _check_track_clip(d, FEET["unitree_g1"], g.model.body_names)
    with pytest.raises(KeyError) as e:
        dataset.tracking_from_qpos(g, qpos, E2E_OFFS, 30.0, 50.0, contact_bodies=["left_ankle_roll_link", "left_toe"])
    assert "left_toe" in str(e.value) and "pelvis" in str(e.value)
    fixed = dataset.tracking_from_qpos(g, qpos, E2E_OFFS, 30.0, 50.0, contact_bodies=FEET["unitree_g1"],
                                       contact=dataset.ContactParams(ground=-1.0))   # a ground far below: nothing touches it
    assert not fixed[0]["contact"].any() and fixed[0]["contact_stats"]["base"] == -1.0 and fixed[0]["airborne_frames"] == fixed[0]["contact"].shape[0]


def test_multi_robot_tracking_from_qpos_labels_each_robots_feet():
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting, dataset
    robots = ["unitree_g1", "booster_t1"]
    mr = MultiRobotRetargeting("smplx", robots, device=0)
    qpos = {r: _stand_and_lift(r) for r in robots}
    got = mr.tracking_from_qpos(qpos, E2E_OFFS, 30.0, 50.0, contact_bodies=FEET)
    for r in robots:
        g = GeneralMotionRetargeting("smplx", r, device=0)
        one = dataset.tracking_from_qpos(g, qpos[r], E2E_OFFS, 30.0, 50.0, contact_bodies=FEET[r])
        for d, w in zip(got[r], one):
            assert d.keys() == w.keys()
            _check_track_clip(d, FEET[r], g.model.body_names)
            assert np.array_equal(d["contact"], w["contact"]) and d["airborne_frames"] == w["airborne_frames"]
            for k in dataset.CONTACT_STATS:   # the same kernel on the same arrays: the same bytes
                assert np.asarray(d["contact_stats"][k]).tobytes() == np.asarray(w["contact_stats"][k]).tobytes(), (r, k)
    only = mr.tracking_from_qpos(qpos, E2E_OFFS, 30.0, 50.0, contact_bodies={"booster_t1": FEET["booster_t1"]})
    assert "contact" not in only["unitree_g1"][0] and np.array_equal(only["booster_t1"][1]["contact"], got["booster_t1"][1]["contact"])
    with pytest.raises(KeyError):
        mr.tracking_from_qpos(qpos, E2E_OFFS, 30.0, 50.0, contact_bodies={"fourier_n1": ["a"]})
    mr.close()


# ------------------------------------------------------------------ 6: the dataset scripts
def test_dataset_script_contact_flags_end_to_end(tmp_path):
    """--contact_bodies beside --track_fps: the .npz files gain the contact keys, computed from their own arrays; the ten arrays
    and the pickles are those of a run without the flag; with --robots only the robots that are named get labels."""
    import os
    from gmr_amd import dataset, synth
    from gmr_amd.scripts import smplx_to_robot_dataset
    g1 = compiled("smplx", "unitree_g1")
    pos, quat, names, offs = synth.synth_clips_torch(g1, np.array([60, 45]), seed=9, device=DEV(), yaw0=0.5, dtype=torch.float64)
    src = str(tmp_path / "in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, pos, quat, names, offs, fps=30.0, heights=[1.7, 1.6])
    tree = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)  # noqa: E731
    base = ["--src_folder", src, "--num_cpus", "2", "--hard_motions", "--track_fps", "50"]
    plain, plain_trk, with_c, trk = (str(tmp_path / n) for n in ("plain", "plain_trk", "with", "trk"))
    assert smplx_to_robot_dataset.main(base + ["--robot", "unitree_g1", "--tgt_folder", plain, "--track_folder", plain_trk]) == 0
    assert smplx_to_robot_dataset.main(base + ["--robot", "unitree_g1", "--tgt_folder", with_c, "--track_folder", trk,
                                               "--contact_bodies", ",".join(FEET["unitree_g1"]), "--contact_height_off", "0.0625"]) == 0
    assert tree(plain) == tree(with_c) and tree(trk) == tree(plain_trk) and len(tree(trk)) == 2
    for f in tree(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(with_c, f), "rb").read(), f
    ids = [list(g1.robot.body_names).index(b) for b in FEET["unitree_g1"]]
    for f in tree(trk):
        got, was = dataset.load_tracking(os.path.join(trk, f)), dataset.load_tracking(os.path.join(plain_trk, f))
        assert set(got) - set(was) == {"contact", "contact_body_names", "contact_stats", "airborne_frames"}
        for k in dataset.TRACK_ARRAYS:
            assert got[k].dtype == was[k].dtype and np.array_equal(got[k], was[k]), (f, k)
        n = got["body_pos_w"].shape[0]
        want = ref.contacts(got["body_pos_w"], got["body_lin_vel_w"], [0, n], ids, None, ref.GROUND_CLIP_MIN, 0.0, 0.03, 0.0625, 0.3, 0.6)
        assert got["contact_body_names"] == FEET["unitree_g1"] and np.array_equal(got["contact"], want["contact"])
        assert got["airborne_frames"] == want["airborne_frames"][0] and got["contact_stats"]["base"] == want["base"][0]
        for k in ("frames", "touchdowns", "depth_max"):
            assert np.array_equal(got["contact_stats"][k], want[k][0]), (f, k)
    multi, mtrk = str(tmp_path / "multi"), str(tmp_path / "multi_trk")
    assert smplx_to_robot_dataset.main(base + ["--robots", "unitree_g1,booster_t1", "--tgt_folder", multi, "--track_folder", mtrk,
                                               "--contact_bodies", "booster_t1:" + ",".join(FEET["booster_t1"])]) == 0
    assert len(tree(mtrk)) == 4
    for f in tree(trk):
        a = dataset.load_tracking(os.path.join(mtrk, "unitree_g1", f))
        b = dataset.load_tracking(os.path.join(mtrk, "booster_t1", f))
        assert "contact" not in a and b["contact_body_names"] == FEET["booster_t1"] and b["contact"].shape == (b["body_pos_w"].shape[0], 2)
        assert all(np.array_equal(a[k], dataset.load_tracking(os.path.join(plain_trk, f))[k]) for k in dataset.TRACK_ARRAYS), f
