"""The transition search without a GPU: the numpy restatement against 50 digits and against brute force, the metric's properties,
the host layer (gmr_amd/transitions.py), the header, the export and the struct layout."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gmr_amd import transitions as tr
from gmr_amd.compose import ComposeError, ComposePlan
from tests import transitions_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = TR.EPS


def unit(P, L, radius):
    return EPS * P * L * (1.0 + radius * radius)


def cost_of(A, B, w):
    return float(TR.pair_costs(A, B, w, A.shape[0])[0, 0])


# ------------------------------------------------------------------ 1: the restatement against 50 digits and brute force
@pytest.mark.parametrize("P,L", TR.CASES)
def test_restatement_against_50_digits_and_the_brute_force_minimum(P, L):
    """The closed form in float64 is within c eps P L (1 + R^2) of its 50-digit evaluation (c: 4 x TR.C_MEASURED, and the measured
    ratio is not above the recorded one); the 50-digit closed form is the brute-force minimum over the angle; the best rotation
    is atan2(-C, D)."""
    A, B, w, radius = TR.case(P, L)
    got = cost_of(A, B, w)
    want, D, Cc = TR.mp_cost(A, B, w)
    ratio = abs(float(TR.mpf(got) - want)) / unit(P, L, radius)
    print(f"P {P} L {L} R {radius:.1f}: cost {got:.6e}, |numpy - 50 digits| {abs(float(TR.mpf(got) - want)):.2e} = {ratio:.4f} eps P L (1 + R^2)")
    assert ratio <= TR.C_MEASURED                         # the recorded figure covers what this machine measures
    assert abs(float(TR.mpf(got) - want)) <= TR.bound(P, L, radius)
    brute, theta = TR.mp_brute(A, B, w, normalise=True)           # (weights that sum to 1 in 50 digits: the closed form's premise)
    exact = TR.mp_cost(A, B, w, normalise=True)[0]
    assert abs(float(brute - exact)) <= 1e-30 * (1.0 + radius * radius), (float(brute), float(exact))
    _, _, Df, Cf, _ = TR.pair_terms(A, B, w, L)
    if float(TR.mp.sqrt(D * D + Cc * Cc)) > 1e-9 * (1.0 + radius * radius):       # (a single point has no angle)
        d = float(theta) - float(np.arctan2(-Cf[0, 0], Df[0, 0]))
        assert abs((d + np.pi) % (2.0 * np.pi) - np.pi) <= 1e-9                    # the sign and the angle
    else:
        assert P == 1 and L == 1


# ------------------------------------------------------------------ 2: properties of the metric
def _planar(X, th, t):
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * X[..., 0] - s * X[..., 1] + t[0], s * X[..., 0] + c * X[..., 1] + t[1], X[..., 2]], -1)


@pytest.mark.parametrize("P,L", TR.CASES)
def test_a_planar_rigid_motion_of_either_clip_leaves_the_cost(P, L):
    A, B, w, radius = TR.case(P, L, seed=1)
    base = cost_of(A, B, w)
    for th, t, which in ((1.0, (3.0, -2.0), 1), (-2.7, (-4.0, 0.5), 0), (np.pi, (0.0, 0.0), 1)):
        A2, B2 = (_planar(A, th, t), B) if which == 0 else (A, _planar(B, th, t))
        r2 = float(max(radius, np.hypot(A2[..., 0], A2[..., 1]).max(), np.hypot(B2[..., 0], B2[..., 1]).max()))
        assert abs(cost_of(A2, B2, w) - base) <= TR.bound(P, L, r2)                           # within that bound, once


@pytest.mark.parametrize("P,L", TR.CASES)
def test_the_cost_is_symmetric_and_zero_against_itself(P, L):
    A, B, w, radius = TR.case(P, L, seed=2)
    ab, ba = cost_of(A, B, w), cost_of(B, A, w)
    assert abs(ab - ba) <= TR.bound(P, L, radius)
    assert ab == ba                                       # (every product commutes and C only changes its sign: bit for bit, in fact)
    # a window against itself costs exactly 0: Gd(f, f) is q_f bit for bit, so D = V; C and Z are 0; and sqrt(V V) = V
    for X in (A, B):
        assert cost_of(X, X, w) == 0.0
    wide = np.concatenate([A, B])                         # windows inside longer clips: the diagonal of a clip against itself
    if L < wide.shape[0]:
        self_cost = TR.pair_costs(wide, wide, w, L)
        assert np.all(np.diag(self_cost) == 0.0) and np.all(self_cost >= 0.0)


def test_a_nan_row_reaches_only_the_windows_that_contain_it():
    A, B, w, _ = TR.case(3, 8)
    rng = np.random.default_rng(5)
    X, Y = rng.normal(size=(30, 3, 3)), rng.normal(size=(25, 3, 3))
    base = TR.pair_costs(X, Y, w, 4)
    X2 = X.copy()
    X2[11, 1, 2] = np.nan
    got = TR.pair_costs(X2, Y, w, 4)
    hit = np.zeros(base.shape, bool)
    hit[8:12] = True
    assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], base[~hit])
    m, j = TR.first_minimum(np.array([np.nan, 3.0, 1.0, 1.0, np.nan]), np.array([True, True, False, True, True]))
    assert (m, j) == (1.0, 3) and TR.first_minimum(np.array([np.nan]), np.array([True])) == (np.inf, -1)


# ------------------------------------------------------------------ 3: the host layer
def test_search_tables():
    offs = [0, 0, 1, 8, 17, 147]
    src, so, dst, do = tr.search_tables(offs, None, [4, 2], 8, 3)
    assert src.tolist() == [0, 1, 2, 3, 4] and src.dtype == dst.dtype == np.int32 and so.dtype == do.dtype == np.int64
    assert so.tolist() == [0, 0, 0, 0, 1, 1 + 41] and do.tolist() == [0, 123, 123]    # 0, 3, ... 120 <= 122; 0 .. 122; none
    assert tr.source_count(7, 8, 1) == 0 and tr.source_count(8, 8, 1) == 1 and tr.source_count(9, 8, 3) == 1 and tr.source_count(11, 8, 3) == 2
    with pytest.raises(ValueError):
        tr.search_tables(offs, [5], None, 8, 1)
    with pytest.raises(ValueError):
        tr.search_tables(offs, None, None, 0, 1)


def _select(cost, frame=None, stride=1, threshold=1.0, radius=0):
    cost = np.asarray(cost, float).reshape(-1, 1)
    frame = np.arange(cost.shape[0], dtype=np.int32).reshape(-1, 1) + 100 if frame is None else np.asarray(frame).reshape(-1, 1)
    return tr.select_transitions(cost, frame, [3], [0, cost.shape[0]], stride, [5], threshold, radius)


def test_select_transitions_plateaus_ties_radius_threshold_and_empty_input():
    inf, nan = np.inf, np.nan
    got = _select([0.5, 0.2, 0.2, 0.2, 0.9, 0.1, 0.8])
    assert [(t.src_frame, t.dst_frame, t.cost) for t in got] == [(1, 101, 0.2), (5, 105, 0.1)]      # a plateau: once, at its first frame
    assert all(t.src_clip == 3 and t.dst_clip == 5 for t in got)
    assert [t.src_frame for t in _select([0.3, 0.3, 0.3])] == [0]                                   # all equal: one candidate
    assert [t.src_frame for t in _select([0.1, 0.5, 0.2])] == [0, 2]                                # the ends count
    assert [t.src_frame for t in _select([0.5, 0.2, 0.2, 0.1, 0.7])] == [3]                         # a plateau on a slope is no minimum
    assert [t.src_frame for t in _select([0.1, 0.5, 0.2], threshold=0.15)] == [0]                   # the threshold, inclusive below
    assert [t.src_frame for t in _select([0.1, 0.5, 0.1], threshold=0.1)] == [0, 2]
    assert [t.src_frame for t in _select([0.1, 0.5, 0.2, 0.6, 0.05], radius=2)] == [0, 4]           # 2 loses to 4 (and to 0)
    assert [t.src_frame for t in _select([0.1, 0.5, 0.2, 0.6, 0.05], radius=1)] == [0, 2, 4]
    assert [t.src_frame for t in _select([0.1, 0.5, 0.1, 0.5, 0.1], radius=2)] == [0]               # a tie goes to the earlier frame: 2 loses to 0, 4 to 2
    assert [t.src_frame for t in _select([0.1, 0.5, 0.1], stride=3, radius=5)] == [0, 6]            # the radius is in frames: 6 > 5
    assert [t.src_frame for t in _select([0.1, 0.5, 0.1], stride=3, radius=6)] == [0]
    assert [t.src_frame for t in _select([nan, 0.4, nan, inf, 0.3], frame=[-1, 7, -1, -1, 9])] == [1, 4]   # NaN and no-target sources
    assert _select([inf, inf], frame=[-1, -1], threshold=inf) == []
    assert _select([]) == [] and tr.select_transitions(np.zeros((0, 0)), np.zeros((0, 0), np.int32), [], [0], 1, [], 1.0, 3) == []
    # two pairs of clips, sorted by (src_clip, src_frame, dst_clip); the radius does not reach across pairs
    cost = np.array([[0.1, 0.2], [0.5, 0.1], [0.3, 0.6], [0.2, 0.3]])
    frame = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], np.int32)
    got = tr.select_transitions(cost, frame, [9, 4], [0, 2, 4], 2, [0, 1], 1.0, 100)
    assert [tuple(t) for t in got] == [(4, 2, 0, 7, 0.2), (4, 2, 1, 8, 0.3), (9, 0, 0, 1, 0.1), (9, 2, 1, 4, 0.1)]
    with pytest.raises(ValueError):
        tr.select_transitions(cost, frame, [9, 4], [0, 2, 3], 2, [0, 1], 1.0, 1)


def test_transition_walks_build_compose_plans():
    offs = np.array([0, 100, 160, 165, 265], np.int64)
    L = 8
    T = tr.Transition
    trans = [T(0, 40, 1, 5, 0.0), T(0, 90, 3, 10, 0.0), T(1, 30, 0, 20, 0.0), T(1, 9, 3, 0, 0.0), T(3, 60, 0, 0, 0.0), T(3, 20, 1, 40, 0.0),
             T(1, 50, 1, 2, 0.0)]
    for n_segments, min_len in ((1, 30), (2, 1), (3, 16), (5, 20), (9, 1)):
        seqs = tr.transition_walks(trans, offs, 12, n_segments, L, min_len, rng=n_segments)
        assert len(seqs) == 12 and all(len(c) == n_segments for c in seqs)
        plan = ComposePlan(offs, seqs, blend=L)                       # every invariant of the contract, checked there
        assert plan.n_out == 12 and int(plan.seg_len.min()) >= max(min_len, L)
        for chain in seqs:                                            # and every joint is one of the transitions
            for s0, s1 in zip(chain[:-1], chain[1:]):
                assert any(t.src_clip == s0.clip and t.src_frame == s0.begin + s0.length - L and t.dst_clip == s1.clip and t.dst_frame == s1.begin
                           for t in trans)
    again = tr.transition_walks(trans, offs, 12, 5, L, 20, rng=5)
    assert again == tr.transition_walks(trans, offs, 12, 5, L, 20, rng=np.random.default_rng(5))
    # the exit must lie a window after the entry: 1 is entered at 5 and T(1, 9, ...) is too early; entered at 2 it is too
    two = tr.transition_walks([T(0, 40, 1, 5, 0.0), T(1, 9, 3, 0, 0.0), T(1, 13, 3, 0, 0.0)], offs, 6, 3, L, 1, rng=0)
    assert all(c[1] == (1, 5, 13 + L - 5) for c in two)
    with pytest.raises(ComposeError, match="no walk"):
        tr.transition_walks([T(0, 40, 1, 5, 0.0), T(1, 9, 3, 0, 0.0)], offs, 1, 3, L, 1, rng=0)
    with pytest.raises(ComposeError, match="no walk"):
        tr.transition_walks(trans, offs, 1, 2, L, 101, rng=0)                                       # no segment is that long
    with pytest.raises(ComposeError, match="no walk"):
        tr.transition_walks([], offs, 1, 2, L, 1, rng=0)
    with pytest.raises(ComposeError, match="no window"):
        tr.transition_walks([T(0, 95, 1, 5, 0.0)], offs, 1, 2, L, 1, rng=0)
    assert tr.DEFAULT_WINDOW == 8


# ------------------------------------------------------------------ 4: header, export, binding, layout
ENTRY = "gmr_motion_transitions"


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_transitions\s*\(gmr_model \*m, const gmr_transitions_input \*in\);", code)
    assert ENTRY in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert re.search(r"^ \*   gmr_motion_transitions\s+\(no counterpart in the reference\)", src, flags=re.M)
    assert (_native.TRANSITIONS_MAX_BODIES, _native.TRANSITIONS_MAX_WINDOW, _native.TRANSITIONS_MOMENTS) == (64, 32, 6)
    lib = _native.load()
    assert lib.gmr_motion_transitions.restype == C.c_int and len(lib.gmr_motion_transitions.argtypes) == 2
    assert lib.gmr_motion_transitions.argtypes[1]._type_ is _native.TransitionsInput
    assert lib.gmr_motion_transitions(None, C.byref(_native.TransitionsInput())) == -1   # a null handle is refused before anything else
    assert lib.gmr_abi_version() == 5
    import gmr_amd
    from gmr_amd import dataset
    assert gmr_amd.find_transitions is dataset.find_transitions


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.TransitionsInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_transitions_input")].rindex("Layout (LP64)"):]
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct gmr_transitions_input \{(.*?)\} gmr_transitions_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_transitions_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 168
    assert listing == {k: getattr(T, k).offset for k in fields}
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_transitions_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_transitions_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]
