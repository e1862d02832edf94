// mirror_kernel.hip.h -- the left-right mirrored copy of qpos (gmr_motion_mirror; the definition is the contract above
// gmr_mirror_input in include/gmr_amd.h).
//
// One launch, no scratch, no atomics, no LDS.  Lane = output column (nq <= 64; the lanes past nq repeat the last column and store
// nothing), one wavefront per workgroup.  Workgroup (s, y) of the grid (n_seq, waves per clip) takes the tiles y, y + gridDim.y, ...
// of kMirrorTile consecutive rows of clip s: the clip's rows come from seq_offsets on the device, so a clip longer than the
// host's estimate only makes its wavefronts walk further.  Lane c loads qpos[row nq + src[c]] and stores out[row nq + c]: both
// touch the one 8 nq-byte row, so the gather stays inside the lines the row brings in anyway, and the store is coalesced.
// kMirrorBatch rows are loaded before the first of them is stored, so that many rows are in flight per wavefront.  src and
// the sign of a column are read once per wavefront and kept in registers.
//
// GMR_MIRROR_WORLD is copies and sign flips (a negation flips the sign bit and nothing else; no arithmetic touches a value).
// GMR_MIRROR_CLIP_START reads the root of the clip's first row once per wavefront (seven doubles, out of the cache for all but
// the clip's first wavefront) and derives from it, wave-uniformly, cos psi, sin psi, cos 2 psi and sin 2 psi of the heading psi
// without a trigonometric function: with f = R(r0 / |r0|) e_x, cos psi = f_x / |f_xy| and so on.  Per row the two xy lanes and the
// four quaternion lanes then need one value of another lane each -- lane 0 <-> 1, lane 3 <-> 6, lane 4 <-> 5 -- which comes through
// v_readlane (lowpass_lane<L>); every lane takes part in every exchange (control flow is wave-uniform).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"       // kFkWave
#include "lowpass_kernel.hip.h"  // lowpass_lane<L>
#include "member_launch.hip.h"   // motion_const

namespace gmr {

constexpr int kMirrorMaxNq = kFkWave;
constexpr int kMirrorBatch = 16;          // rows in flight per wavefront
constexpr int kMirrorTile = 64;           // rows of one tile: four batches
constexpr int kMirrorTargetWaves = 16384; // wavefronts the host aims at in one launch: 256 CUs x 32 slots, twice over
constexpr int kMirrorWorld = 0, kMirrorClipStart = 1;   // GMR_MIRROR_WORLD, GMR_MIRROR_CLIP_START

struct MirrorArgs {
  const double *qpos;          // [n_frames][nq]
  double *out;                 // [n_frames][nq], not qpos
  const int64_t *seq_offsets;  // device, [n_seq + 1]
  const int32_t *col_src;      // device, [nq]; elements 7 .. nq-1 are read
  const double *col_sign;      // device, [nq]; elements 7 .. nq-1 are read
  int64_t n_frames;
  int n_seq, nq, mode;
};

// What lane `lane` does to a root column in CLIP_START mode: out = base + (a * (own - sub) + b * (other - osub)) on the xy lanes,
// out = a * own + b * other on the quaternion lanes, a copy on lane 2.
struct MirrorRoot {
  double a, b, sub, osub;
};

__global__ void __launch_bounds__(kFkWave) motion_mirror_kernel(MirrorArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kMirrorBatch;
  const int lane = threadIdx.x, nq = A.nq;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  const int64_t N = A.n_frames;
  int64_t o = motion_const(A.seq_offsets + s), e = motion_const(A.seq_offsets + s + 1);
  o = o < 0 ? 0 : (o > N ? N : o);
  e = e < o ? o : (e > N ? N : e);
  const int64_t T = e - o;
  if ((int64_t)blockIdx.y * kMirrorTile >= T) return;  // (a clip without frames, and the wavefronts past a short clip's last tile)
  const bool live = lane < nq;
  const int c = live ? lane : nq - 1;
  int src = c;
  bool neg = c == 1 || c == 4 || c == 6;  // the world mirror of the root: (x, -y, z), (w, -x, y, -z)
  if (c >= 7) {
    src = A.col_src[c];
    src = src < 7 ? 7 : (src > nq - 1 ? nq - 1 : src);  // trusted (the caller guarantees 7 <= col_src[c] < nq); only clamped
    neg = A.col_sign[c] < 0.0;
  }
  const bool clip_start = A.mode == kMirrorClipStart;   // (wave-uniform)
  const bool xy = lane < 2, quat = lane >= 3 && lane < 7;
  MirrorRoot r{};
  if (clip_start) {
    const double first = A.qpos[o * nq + (lane < 7 ? lane : 6)];
    const double p0x = lowpass_lane<0>(first), p0y = lowpass_lane<1>(first);
    const double w0 = lowpass_lane<3>(first), x0 = lowpass_lane<4>(first), y0 = lowpass_lane<5>(first), z0 = lowpass_lane<6>(first);
    const double n = sqrt(((w0 * w0 + x0 * x0) + y0 * y0) + z0 * z0);
    const double w = w0 / n, x = x0 / n, y = y0 / n, z = z0 / n;
    const double fx = 1.0 - 2.0 * (y * y + z * z), fy = 2.0 * (x * y + w * z);
    const double h2 = fx * fx + fy * fy;
    double cp = 1.0, sp = 0.0, c2 = 1.0, s2 = 0.0;  // psi = 0: the convention for a root pointing straight up
    if (!(h2 < 1e-12)) {                            // (a NaN takes this branch and stays a NaN)
      const double h = sqrt(h2);
      cp = fx / h;
      sp = fy / h;
      c2 = (fx * fx - fy * fy) / h2;
      s2 = (2.0 * fx * fy) / h2;
    }
    // x' = p0x + (c2 dx + s2 dy)      y' = p0y + (-c2 dy + s2 dx)
    // w' = cp w + sp z    x' = -cp x + -sp y    y' = cp y + -sp x    z' = -cp z + sp w
    r.a = lane == 0 ? c2 : lane == 1 ? -c2 : (lane == 3 || lane == 5) ? cp : -cp;
    r.b = xy ? s2 : (lane == 3 || lane == 6) ? sp : -sp;
    r.sub = lane == 0 ? p0x : p0y;
    r.osub = lane == 0 ? p0y : p0x;
  }
  const double *x = A.qpos + o * nq + src;
  double *w = A.out + o * nq + c;
  for (int64_t t0 = (int64_t)blockIdx.y * kMirrorTile; t0 < T; t0 += (int64_t)gridDim.y * kMirrorTile) {
    const int64_t t1 = t0 + kMirrorTile < T ? t0 + kMirrorTile : T;
    for (int64_t i0 = t0; i0 < t1; i0 += B) {
      double v[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {  // (rows past the tile's end repeat its last row and are not stored)
        const int64_t i = i0 + b;
        v[b] = x[(i < t1 ? i : t1 - 1) * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (i0 + b < t1) {  // (wave-uniform)
          double y = neg ? -v[b] : v[b];
          if (clip_start) {
            const double q0 = lowpass_lane<0>(v[b]), q1 = lowpass_lane<1>(v[b]);
            const double q3 = lowpass_lane<3>(v[b]), q4 = lowpass_lane<4>(v[b]), q5 = lowpass_lane<5>(v[b]), q6 = lowpass_lane<6>(v[b]);
            const double other = lane == 0 ? q1 : lane == 1 ? q0 : lane == 3 ? q6 : lane == 4 ? q5 : lane == 5 ? q4 : q3;
            if (xy) y = r.sub + (r.a * (v[b] - r.sub) + r.b * (other - r.osub));
            if (quat) y = r.a * v[b] + r.b * other;
          }
          if (live) w[(i0 + b) * nq] = y;
        }
      }
    }
  }
}

}  // namespace gmr
