"""The low-pass of the tracking export restated in numpy: the contract above ``gmr_track_input`` in include/gmr_amd.h, operation
by operation and in its order (float64; numpy's elementwise +, -, *, / and sqrt are correctly rounded and never fused, which is
what the kernel's arithmetic without contraction gives).  The coefficients are an argument: the library's come from
``gmr_lowpass_coefficients``, whose ``tan`` no restatement can reproduce bit for bit."""
import ctypes

import numpy as np

PAD = 9


def library_coefficients(fc, fs):
    """``gmr_lowpass_coefficients`` through ctypes: float64 [5] = b0 b1 b2 a1 a2; ``None`` where the library refuses."""
    from gmr_amd import _native
    c = (ctypes.c_double * 5)()
    rc = _native.load().gmr_lowpass_coefficients(float(fc), float(fs), c)
    return np.array(list(c)) if rc == 0 else None


def formula_coefficients(fc, fs):
    """The contract's formulas with numpy's tan."""
    K = np.tan(np.pi * fc / fs)
    r2 = np.sqrt(2.0)
    n = 1.0 / (1.0 + r2 * K + K * K)
    b0 = K * K * n
    return np.array([b0, 2.0 * b0, b0, 2.0 * (K * K - 1.0) * n, (1.0 - r2 * K + K * K) * n])


def _one_pass(c, x):
    """Transposed direct form II over axis 0 of x [L, ...], started at lfilter_zi times the first sample."""
    b0, b1, b2, a1, a2 = (np.float64(v) for v in c)
    u = x[0]
    z1 = (1.0 - b0) * u
    z2 = (b2 - a2) * u
    y = np.empty_like(x)
    for i in range(x.shape[0]):
        xi = x[i]
        yi = b0 * xi + z1
        z1 = (b1 * xi - a1 * yi) + z2
        z2 = b2 * xi - a2 * yi
        y[i] = yi
    return y


def filter_columns(c, x):
    """Columns of x [T, ...] (one clip) filtered forward and backward; T <= 1: a copy."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    if T <= 1:
        return x.copy()
    e = min(PAD, T - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        ext = np.concatenate([2.0 * x[0] - x[np.arange(e, 0, -1)], x, 2.0 * x[T - 1] - x[np.arange(T - 2, T - 2 - e, -1)]])
        fwd = _one_pass(c, ext)
        bwd = _one_pass(c, fwd[::-1])[::-1]
    return np.ascontiguousarray(bwd[e:e + T])


def _dot4(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def sign_continuous(q):
    """q [T, 4]: q'_0 = q_0, q'_i = -q_i when q'_{i-1} . q_i < 0."""
    q = np.array(q, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(1, q.shape[0]):
            if _dot4(q[i - 1], q[i]) < 0.0:
                q[i] = -q[i]
    return q


def filter_quat(c, q):
    """The root quaternion of one clip [T, 4] (any component order): sign-continuous, filtered, normalised."""
    r = filter_columns(c, sign_continuous(q))
    with np.errstate(invalid="ignore", divide="ignore"):
        return r / np.sqrt(_dot4(r, r))[:, None]


def filter_clip(c, qpos):
    """One clip of free-joint qpos [T, nq] (x y z qw qx qy qz hinges)."""
    qpos = np.asarray(qpos, dtype=np.float64)
    out = filter_columns(c, qpos)
    if qpos.shape[0]:
        out[:, 3:7] = filter_quat(c, qpos[:, 3:7])
    return out


def filter_qpos(qpos, seq_offsets, fs, fc, coefficients=library_coefficients):
    """Concatenated clips; ``fs``: one rate or one per clip.  Clips without frames need no coefficients."""
    qpos = np.asarray(qpos, dtype=np.float64)
    offs = np.asarray(seq_offsets, dtype=np.int64)
    fs = np.broadcast_to(np.asarray(fs, dtype=np.float64), (offs.size - 1,))
    out = np.empty_like(qpos)
    cache = {}
    for s in range(offs.size - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        if b > a:
            key = float(fs[s])
            if key not in cache:
                cache[key] = coefficients(fc, key)
            out[a:b] = filter_clip(cache[key], qpos[a:b])
    return out
