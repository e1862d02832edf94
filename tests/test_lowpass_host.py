"""The low-pass of the tracking export, the parts that need no GPU: the library's coefficients against scipy's, the numpy
restatement of the contract (tests/lowpass_reference.py) against scipy.signal.filtfilt, the quaternion rule's properties, the
struct field and the host-side Nyquist check."""
import ctypes

import numpy as np
import pytest

from tests import lowpass_reference as ref

RATES = [(30.0, 6.0), (30.0, 3.0), (120.0, 6.0), (120.0, 3.0), (50.0, 10.0), (30.0, 14.0), (120.0, 1.0)]  # (fs, fc)
LENGTHS = [2, 3, 4, 9, 10, 11, 64, 65, 300, 3000]
COEF_BOUND = 4e-15      # absolute; the same formula with numpy's tan measures 4.4e-16 on RATES
FILTFILT_BOUND = 1e-11  # absolute, |x| <= 4


def _signal():
    return pytest.importorskip("scipy.signal")  # (only the comparisons with scipy need it)


def _lib():
    from gmr_amd import _native
    from gmr_amd.build import build_lib
    build_lib()
    return _native.load()


def _walks(T, n, seed):
    """n random walks of T samples, |x| <= 4."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(size=(T, n)) * 0.1, axis=0) + rng.uniform(-1, 1, size=n)
    return x * np.minimum(1.0, 4.0 / np.abs(x).max(axis=0))


def _unit_quats(T, seed):
    rng = np.random.default_rng(seed)
    q = np.cumsum(rng.normal(size=(T, 4)) * 0.05, axis=0) + rng.normal(size=4)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


@pytest.mark.parametrize("fs,fc", RATES)
def test_coefficients_match_scipy_butter(fs, fc):
    signal = _signal()
    _lib()
    c = ref.library_coefficients(fc, fs)
    b, a = signal.butter(2, 2 * fc / fs)
    assert a[0] == 1.0
    want = np.concatenate([b, a[1:]])
    err = np.abs(c - want).max()
    print(f"fs {fs} fc {fc}: library vs scipy {err:.3g}, numpy formula vs scipy {np.abs(ref.formula_coefficients(fc, fs) - want).max():.3g}")
    assert err <= COEF_BOUND
    assert c[1] == 2.0 * c[0] and c[2] == c[0]


def test_coefficients_refuse_what_the_header_says():
    lib = _lib()
    c = (ctypes.c_double * 5)()
    for fc, fs in ((15.0, 30.0), (0.0, 30.0), (-1.0, 30.0), (float("nan"), 30.0), (6.0, float("nan")), (6.0, float("inf")), (16.0, 30.0)):
        assert lib.gmr_lowpass_coefficients(fc, fs, c) == -1, (fc, fs)
    assert lib.gmr_lowpass_coefficients(6.0, 30.0, None) == -1
    assert lib.gmr_lowpass_coefficients(np.nextafter(15.0, 0.0), 30.0, c) == 0
    assert "gmr_lowpass_coefficients" in __import__("gmr_amd")._native.EXPORTS


@pytest.mark.parametrize("fs,fc", RATES)
def test_restatement_matches_filtfilt(fs, fc):
    signal = _signal()
    _lib()
    c = ref.library_coefficients(fc, fs)
    b, a = signal.butter(2, 2 * fc / fs)
    worst = 0.0
    for T in LENGTHS:
        x = _walks(T, 6, 1000 + T)
        assert np.abs(x).max() <= 4.0
        got = ref.filter_columns(c, x)
        want = signal.filtfilt(b, a, x, axis=0, padlen=min(9, T - 1))
        err = np.abs(got - want).max()
        worst = max(worst, err)
        print(f"fs {fs} fc {fc} T {T}: {err:.3g}")
        assert err <= FILTFILT_BOUND, (T, err)
    print(f"fs {fs} fc {fc}: worst {worst:.3g}")


def test_short_clips_are_copies():
    c = ref.formula_coefficients(6.0, 30.0)
    for T in (0, 1):
        x = _walks(max(T, 1), 5, 7)[:T]
        got = ref.filter_columns(c, x)
        assert got.shape == x.shape and np.array_equal(got, x) and got is not x


@pytest.mark.parametrize("T", [2, 11, 300])
def test_quaternion_rule(T):
    c = ref.formula_coefficients(6.0, 30.0)
    q = _unit_quats(T, 50 + T)
    out = ref.filter_quat(c, q)
    assert np.abs(np.linalg.norm(out, axis=1) - 1.0).max() <= 4.5e-16
    assert np.all(ref._dot4(out[:-1], out[1:]) > 0.0)  # sign-continuous
    rng = np.random.default_rng(T)
    flip = rng.random(T) < 0.3
    flip[0] = False
    if T == 2:
        flip[1] = True
    q2 = np.where(flip[:, None], -q, q)
    assert np.array_equal(ref.filter_quat(c, q2), out)          # negating rows other than row 0: no output bit changes
    q3 = q.copy()
    q3[0] = -q3[0]
    assert np.array_equal(ref.filter_quat(c, q3), -out)         # negating row 0 negates every output row
    full = np.concatenate([_walks(T, 3, 3), q, _walks(T, 5, 4)], axis=1)
    got = ref.filter_clip(c, full)
    assert np.array_equal(got[:, 3:7], out) and np.array_equal(got[:, :3], ref.filter_columns(c, full[:, :3]))


def test_track_input_carries_lowpass_hz():
    from gmr_amd import _native
    T = _native.TrackInput
    assert dict(T._fields_)["lowpass_hz"] is ctypes.c_float
    assert T.lowpass_hz.offset == 52 and T.lowpass_hz.size == 4 and ctypes.sizeof(T) == 136
    assert "reserved" not in dict(T._fields_)
    ti = T()
    assert ti.lowpass_hz == 0.0 and bytes(ti) == bytes(136)
    ti.lowpass_hz = 6.0
    assert bytes(ti)[52:56] == np.float32(6.0).tobytes()


def test_lowpass_check_names_the_clip_at_nyquist():
    from gmr_amd.schedule import lowpass_check
    offs = np.array([0, 10, 10, 40, 45], np.int64)
    fps = [120.0, 30.0, 30.0, 120.0]   # clip 1 (at 30) is empty: only clip 2 is at Nyquist for 15 Hz
    assert lowpass_check(offs, fps, 50.0, 6.0) == 6.0
    assert lowpass_check(offs, fps, 50.0, None) == 0.0 and lowpass_check(offs, fps, 50.0, 0.0) == 0.0 and lowpass_check(offs, fps, 50.0, -0.0) == 0.0
    assert lowpass_check(offs, 120.0, 50.0, 59.0) == 59.0
    with pytest.raises(ValueError, match="clip 2"):
        lowpass_check(offs, fps, 50.0, 15.0)
    with pytest.raises(ValueError, match="clip 2"):
        lowpass_check(offs, fps, 50.0, 20.0)
    with pytest.raises(ValueError, match="clip 0"):
        lowpass_check(offs, 30.0, 30.0, 15.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lowpass_check(offs, fps, 50.0, bad)
