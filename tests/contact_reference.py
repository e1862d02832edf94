"""The contract of gmr_motion_contacts (include/gmr_amd.h) as a plain Python loop over frames, in numpy float64 scalars, and a
second, independent formulation of the label: the kind of the last decisive frame at or before k, found on Python-int bit masks in
tiles of 64 frames with a carry -- the identity the kernel relies on.  Nothing here imports gmr_amd."""
import math

import numpy as np

GROUND_FIXED, GROUND_CLIP_MIN = 0, 1
FIELDS = ("contact", "frames", "touchdowns", "slide_sum", "slide_step_max", "depth_max", "airborne_frames", "base")
TILE = 64


# ------------------------------------------------------------------ the label, twice
def labels_loop(enter, stay):
    """c_{-1} = 0; c_k = 1 when enter, 0 when not stay, c_{k-1} otherwise."""
    out, c = [], 0
    for e, s in zip(enter, stay):
        if e:
            c = 1
        elif not s:
            c = 0
        out.append(c)
    return out


def labels_tiled(enter, stay, tile=TILE):
    """The same labels without a loop over the frames of a tile: per tile the masks on (bit l: frame l enters) and off (bit l:
    frame l does not stay); frame l's label is the kind of the highest set bit of (on | off) at or below bit l, and the carry when
    there is none; the carry into the next tile is the kind of the tile's highest decisive bit, or the old carry."""
    n, out, carry = len(enter), [], 0
    for k0 in range(0, n, tile):
        m = min(tile, n - k0)
        on = sum(1 << l for l in range(m) if enter[k0 + l])
        off = sum(1 << l for l in range(m) if not stay[k0 + l] and not enter[k0 + l])
        dec = on | off
        for l in range(m):
            below = dec & ((2 << l) - 1)
            out.append(carry if below == 0 else (on >> (below.bit_length() - 1)) & 1)
        if dec:
            carry = (on >> (dec.bit_length() - 1)) & 1
    return out


# ------------------------------------------------------------------ the whole contract
def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def contacts(pos, vel, out_offsets, body_ids, height_offset, ground_mode, ground_z, height_on, height_off, speed_on, speed_off):
    """pos, vel float32 [M, nbody, 3]; returns the eight outputs by name (FIELDS) and ``slide_terms``: per clip and column the
    list of the d_k that slide_sum adds, in frame order."""
    pos, vel = np.asarray(pos), np.asarray(vel)
    assert pos.dtype == np.float32 and vel.dtype == np.float32
    M, S, C = pos.shape[0], len(out_offsets) - 1, len(body_ids)
    f64 = np.float64
    hoff = [f64(0.0)] * C if height_offset is None else [f64(v) for v in height_offset]
    hon, hof, son2, sof2 = f64(height_on), f64(height_off), f64(speed_on) * f64(speed_on), f64(speed_off) * f64(speed_off)
    res = {"contact": np.zeros((M, C), np.uint8), "frames": np.zeros((S, C), np.int32), "touchdowns": np.zeros((S, C), np.int32),
           "slide_sum": np.zeros((S, C)), "slide_step_max": np.zeros((S, C)), "depth_max": np.zeros((S, C)),
           "airborne_frames": np.zeros(S, np.int32), "base": np.zeros(S)}
    terms = [[[] for _ in range(C)] for _ in range(S)]
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            a = _clamp(int(out_offsets[s]), 0, M)
            b = _clamp(int(out_offsets[s + 1]), a, M)
            hc = [[f64(pos[g, body_ids[c], 2]) - hoff[c] for c in range(C)] for g in range(a, b)]
            if ground_mode == GROUND_FIXED:
                base = f64(ground_z)
            else:
                flat = [v for row in hc for v in row]
                if not flat or any(math.isnan(v) for v in flat):
                    base = f64(np.nan)
                else:
                    base = flat[0]
                    for v in flat[1:]:
                        base = v if v < base else base
            res["base"][s] = base
            label = [0] * C
            for k in range(b - a):
                g = a + k
                any_on = False
                for c in range(C):
                    j = body_ids[c]
                    h = hc[k][c] - base
                    vx, vy, vz = f64(vel[g, j, 0]), f64(vel[g, j, 1]), f64(vel[g, j, 2])
                    s2 = (vx * vx + vy * vy) + vz * vz
                    enter = bool(h <= hon) and bool(s2 <= son2)
                    stay = bool(h <= hof) and bool(s2 <= sof2)
                    prev = label[c]
                    cur = 1 if enter else (0 if not stay else prev)
                    label[c] = cur
                    res["contact"][g, c] = cur
                    res["frames"][s, c] += cur
                    res["touchdowns"][s, c] += int(cur == 1 and prev == 0)
                    if k >= 1 and cur == 1 and prev == 1:
                        dx = f64(pos[g, j, 0]) - f64(pos[g - 1, j, 0])
                        dy = f64(pos[g, j, 1]) - f64(pos[g - 1, j, 1])
                        d2 = dx * dx + dy * dy
                        terms[s][c].append(np.sqrt(d2))
                        res["slide_sum"][s, c] = res["slide_sum"][s, c] + terms[s][c][-1]
                        if d2 > res["slide_step_max"][s, c]:   # (holds the maximum of d2 until the clip is done)
                            res["slide_step_max"][s, c] = d2
                    dep = base - hc[k][c]
                    if dep > res["depth_max"][s, c]:
                        res["depth_max"][s, c] = dep
                    any_on = any_on or cur == 1
                res["airborne_frames"][s] += int(not any_on)
            res["slide_step_max"][s] = np.sqrt(res["slide_step_max"][s])
    res["slide_terms"] = terms
    return res
