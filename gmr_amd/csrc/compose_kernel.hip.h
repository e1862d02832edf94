// compose_kernel.hip.h -- long reference motions from aligned, blended segments of clips (gmr_motion_compose; the definition is the
// contract above gmr_compose_input in include/gmr_amd.h).
//
// Two launches, no scratch, no atomics, no LDS.
//
// motion_compose_plan_kernel: one wavefront per output clip.  Lane = segment for the loads: a batch of kFkWave segments reads
// its anchor pairs (the seven root doubles of two rows, 14 doubles per lane, all lanes' loads in flight together) and derives its
// relative map D_k = (cd, sd, tdx, tdy) in parallel.  The composition T_k = T_{k-1} o D_k, the half angle and the sign fix then
// run in segment order: step i reads lane i's twelve doubles through v_readlane (a wave-uniform lane index), every lane computes
// the same state, and lane i keeps it.  A chain longer than one batch carries the state into the next batch.  Each lane stores its
// segment's six doubles to seg_transform.
//
// motion_compose_kernel: motion_mirror_kernel's mapping.  Lane = column (nq <= 64; the lanes past nq repeat the last column and
// store nothing), one wavefront per workgroup.  Workgroup (k, y) of the grid (segments, waves per segment) takes the tiles y,
// y + gridDim.y, ... of kComposeTile consecutive output rows of segment k; the segment's rows come from the tables on the device,
// so a segment longer than the host's estimate only makes its wavefronts walk further.  Rows past the overlap are the segment's
// own: kComposeBatch of them are loaded before the first is stored, and the root lanes exchange through v_readlane
// (lowpass_lane<L>) as the mirror's do.  A row of the overlap loads both of its source rows, places each by its segment's map and
// blends them; the slerp's scalars are computed by every lane from the exchanged quaternions (the cost of one lane), so control
// flow stays wave-uniform.  The overlap's rows go one at a time -- two loads in flight -- in a loop that is not unrolled: track_slerp
// holds an acos and three sines, and sixteen copies of it would be most of the kernel's code for about one row in a hundred.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"       // kFkWave
#include "lowpass_kernel.hip.h"  // lowpass_lane<L>
#include "member_launch.hip.h"   // motion_const
#include "track_kernel.hip.h"    // track_slerp

namespace gmr {

constexpr int kComposeMaxNq = kFkWave;
constexpr int kComposeBatch = 16;          // rows in flight per wavefront
constexpr int kComposeTile = 64;           // rows of one tile: four batches
constexpr int kComposeTargetWaves = 16384; // wavefronts the host aims at in one launch (the mirror's figure)
constexpr double kComposeHeadingEps = 1e-12;

struct ComposeArgs {
  const double *qpos;          // [n_frames][nq]
  double *out;                 // [n_out_frames][nq], not qpos
  double *seg_transform;       // [n_seg][6]: c s tx ty hw hz; written by the plan kernel, read by the other
  const int64_t *seg_src;      // device, [n_seg]
  const int32_t *seg_len;      // device, [n_seg]
  const int32_t *seg_blend;    // device, [n_seg]
  const int64_t *seg_out;      // device, [n_seg]
  const int64_t *clip_segs;    // device, [n_out + 1]
  int64_t n_frames, n_out_frames;
  int n_seg, n_out, nq;
};

// lane `i`'s value in every lane; i is wave-uniform
__device__ __forceinline__ double compose_lane(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// (cos psi, sin psi) of the heading of a wxyz quaternion: the mirror contract's
__device__ __forceinline__ void compose_heading(double w0, double x0, double y0, double z0, double &cp, double &sp) {
#pragma clang fp contract(off)
  const double n = sqrt(((w0 * w0 + x0 * x0) + y0 * y0) + z0 * z0);
  const double w = w0 / n, x = x0 / n, y = y0 / n, z = z0 / n;
  const double fx = 1.0 - 2.0 * (y * y + z * z), fy = 2.0 * (x * y + w * z);
  const double h2 = fx * fx + fy * fy;
  cp = 1.0;
  sp = 0.0;  // psi = 0: the convention for a root pointing straight up
  if (!(h2 < kComposeHeadingEps)) {  // (a NaN takes this branch and stays a NaN)
    const double h = sqrt(h2);
    cp = fx / h;
    sp = fy / h;
  }
}

__device__ __forceinline__ int64_t compose_row(int64_t r, int64_t n) { return r < 0 ? 0 : (r > n - 1 ? n - 1 : r); }

__global__ void __launch_bounds__(kFkWave) motion_compose_plan_kernel(ComposeArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  const int lane = threadIdx.x;
  const int o = blockIdx.x;
  if (o >= A.n_out) return;
  const int64_t N = A.n_frames;
  int64_t k0 = motion_const(A.clip_segs + o), k1 = motion_const(A.clip_segs + o + 1);
  k0 = k0 < 0 ? 0 : (k0 > A.n_seg ? A.n_seg : k0);
  k1 = k1 < k0 ? k0 : (k1 > A.n_seg ? A.n_seg : k1);
  double c = 1.0, s = 0.0, tx = 0.0, ty = 0.0, hw = 1.0, hz = 0.0;  // T of the segment before: the carry
  for (int64_t kb = k0; kb < k1; kb += kFkWave) {
    const int64_t left = k1 - kb;
    const int nb = left < kFkWave ? (int)left : kFkWave;  // (wave-uniform)
    const int64_t k = kb + (lane < nb ? lane : nb - 1);
    // this lane's D_k and anchor quaternions; the chain's first segment has none
    double cd = 1.0, sd = 0.0, tdx = 0.0, tdy = 0.0, ra[4] = {1.0, 0.0, 0.0, 0.0}, rb[4] = {1.0, 0.0, 0.0, 0.0};
    if (k > k0) {
      const int64_t B = A.seg_blend[k], a = B / 2;
      const double *pa = A.qpos + compose_row(A.seg_src[k - 1] + A.seg_len[k - 1] - B + a, N) * A.nq;
      const double *pb = A.qpos + compose_row(A.seg_src[k] + a, N) * A.nq;
      double va[7], vb[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) { va[i] = pa[i]; vb[i] = pb[i]; }
      double ca, sa, cb, sb;
      compose_heading(va[3], va[4], va[5], va[6], ca, sa);
      compose_heading(vb[3], vb[4], vb[5], vb[6], cb, sb);
      cd = ca * cb + sa * sb;
      sd = sa * cb - ca * sb;
      tdx = va[0] - (cd * vb[0] - sd * vb[1]);
      tdy = va[1] - (sd * vb[0] + cd * vb[1]);
#pragma unroll
      for (int i = 0; i < 4; ++i) { ra[i] = va[3 + i]; rb[i] = vb[3 + i]; }
    }
    double mc = 1.0, ms = 0.0, mtx = 0.0, mty = 0.0, mhw = 1.0, mhz = 0.0;  // this lane's T_k
#pragma unroll 1
    for (int i = 0; i < nb; ++i) {
      if (kb + i > k0) {  // (wave-uniform)
        const double dcd = compose_lane(cd, i), dsd = compose_lane(sd, i), dtx = compose_lane(tdx, i), dty = compose_lane(tdy, i);
        const double aw = compose_lane(ra[0], i), ax = compose_lane(ra[1], i), ay = compose_lane(ra[2], i), az = compose_lane(ra[3], i);
        const double bw = compose_lane(rb[0], i), bx = compose_lane(rb[1], i), by = compose_lane(rb[2], i), bz = compose_lane(rb[3], i);
        // the previous segment's placed anchor quaternion, with its (sign-fixed) half angle
        const double paw = hw * aw - hz * az, pax = hw * ax - hz * ay, pay = hw * ay + hz * ax, paz = hw * az + hz * aw;
        const double nx = (c * dtx - s * dty) + tx, ny = (s * dtx + c * dty) + ty;
        const double c1 = c * dcd - s * dsd, s1 = s * dcd + c * dsd;
        const double n = sqrt(c1 * c1 + s1 * s1);
        c = c1 / n;
        s = s1 / n;
        tx = nx;
        ty = ny;
        if (c < 0.0) {  // a turn past a quarter: the sine's half first, so that a turn of pi is exact to rounding
          const double m = sqrt((1.0 - c) * 0.5);
          hw = fabs(s) / (2.0 * m);
          hz = s < 0.0 ? -m : m;
        } else {
          hw = sqrt((1.0 + c) * 0.5);
          hz = s / (2.0 * hw);
        }
        const double pbw = hw * bw - hz * bz, pbx = hw * bx - hz * by, pby = hw * by + hz * bx, pbz = hw * bz + hz * bw;
        const double dot = ((paw * pbw + pax * pbx) + pay * pby) + paz * pbz;
        if (dot < 0.0) {
          hw = -hw;
          hz = -hz;
        }
      } else {
        c = 1.0; s = 0.0; tx = 0.0; ty = 0.0; hw = 1.0; hz = 0.0;  // the chain's first segment: the identity
      }
      if (lane == i) { mc = c; ms = s; mtx = tx; mty = ty; mhw = hw; mhz = hz; }
    }
    if (lane < nb) {
      double *w = A.seg_transform + k * 6;
      w[0] = mc; w[1] = ms; w[2] = mtx; w[3] = mty; w[4] = mhw; w[5] = mhz;
    }
  }
}

// What lane `lane` does to a root column of a segment's row: out = (a * own + b * other) + t on the xy lanes, out = a * own +
// b * other on the quaternion lanes; every other lane, and every lane of a chain's first segment, copies.
struct ComposeMap {
  double a, b, t;
  bool copy;
};

__device__ __forceinline__ ComposeMap compose_map(const double *T, bool first, int lane) {
  ComposeMap m{1.0, 0.0, 0.0, true};
  if (!first) {
    // x' = (c x + (-s) y) + tx    y' = (c y + s x) + ty
    // w' = hw w + (-hz) z    x' = hw x + (-hz) y    y' = hw y + hz x    z' = hw z + hz w
    const double c = T[0], s = T[1], tx = T[2], ty = T[3], hw = T[4], hz = T[5];
    m.a = lane < 2 ? c : hw;
    m.b = lane == 0 ? -s : lane == 1 ? s : (lane == 3 || lane == 4) ? -hz : hz;
    m.t = lane == 0 ? tx : ty;
    m.copy = false;
  }
  return m;
}

// the row's value of this lane, placed; v is the loaded value, every lane takes part in the exchanges
__device__ __forceinline__ double compose_place(const ComposeMap &m, double v, int lane) {
#pragma clang fp contract(off)
  if (m.copy) return v;  // (wave-uniform)
  const double q0 = lowpass_lane<0>(v), q1 = lowpass_lane<1>(v);
  const double q3 = lowpass_lane<3>(v), q4 = lowpass_lane<4>(v), q5 = lowpass_lane<5>(v), q6 = lowpass_lane<6>(v);
  const double other = lane == 0 ? q1 : lane == 1 ? q0 : lane == 3 ? q6 : lane == 4 ? q5 : lane == 5 ? q4 : q3;
  double y = v;
  if (lane < 2) y = (m.a * v + m.b * other) + m.t;
  if (lane >= 3 && lane < 7) y = m.a * v + m.b * other;
  return y;
}

__global__ void __launch_bounds__(kFkWave) motion_compose_kernel(ComposeArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kComposeBatch;
  const int lane = threadIdx.x, nq = A.nq;
  const int k = blockIdx.x;
  if (k >= A.n_seg) return;
  const int64_t N = A.n_frames, M = A.n_out_frames;
  const int64_t len = motion_const(A.seg_len + k);
  int64_t bl = motion_const(A.seg_blend + k);
  int64_t nxt = k + 1 < A.n_seg ? (int64_t)motion_const(A.seg_blend + k + 1) : 0;  // 0: the next segment starts another chain
  bl = (bl < 0 || k == 0) ? 0 : bl;
  nxt = nxt < 0 ? 0 : nxt;
  const int64_t W = len - nxt;  // the rows this segment writes
  if ((int64_t)blockIdx.y * kComposeTile >= W) return;
  const int64_t src = motion_const(A.seg_src + k), dst = motion_const(A.seg_out + k);
  const bool live = lane < nq;
  const int c = live ? lane : nq - 1;
  const bool quat = lane >= 3 && lane < 7;
  const ComposeMap own = compose_map(A.seg_transform + (int64_t)k * 6, bl == 0, lane);
  const double *x = A.qpos + c;
  double *w = A.out + c;
  for (int64_t t0 = (int64_t)blockIdx.y * kComposeTile; t0 < W; t0 += (int64_t)gridDim.y * kComposeTile) {
    const int64_t t1 = t0 + kComposeTile < W ? t0 + kComposeTile : W;
    int64_t i0 = t0;
    if (i0 < bl) {  // the overlap with the segment before (wave-uniform)
      const int kp = k - 1;
      const int64_t psrc = motion_const(A.seg_src + kp) + (motion_const(A.seg_len + kp) - bl);
      const bool pfirst = motion_const(A.seg_blend + kp) <= 0 || kp == 0;
      const ComposeMap prev = compose_map(A.seg_transform + (int64_t)kp * 6, pfirst, lane);
      const int64_t e = bl < t1 ? bl : t1;
      const double den = (double)(bl + 1);
#pragma unroll 1
      for (; i0 < e; ++i0) {
        const double v0 = x[compose_row(psrc + i0, N) * nq], v1 = x[compose_row(src + i0, N) * nq];
        const double p0 = compose_place(prev, v0, lane), p1 = compose_place(own, v1, lane);
        const double u = (double)(i0 + 1) / den;
        const double wt = (u * u) * (3.0 - 2.0 * u);
        const double qa[4] = {lowpass_lane<4>(p0), lowpass_lane<5>(p0), lowpass_lane<6>(p0), lowpass_lane<3>(p0)};  // xyzw
        const double qb[4] = {lowpass_lane<4>(p1), lowpass_lane<5>(p1), lowpass_lane<6>(p1), lowpass_lane<3>(p1)};
        double qr[4];
        track_slerp(qa, qb, wt, qr);
        double y = p0 + wt * (p1 - p0);
        if (quat) y = lane == 3 ? qr[3] : lane == 4 ? qr[0] : lane == 5 ? qr[1] : qr[2];
        const int64_t r = dst + i0;
        if (live && r >= 0 && r < M) w[r * nq] = y;
      }
    }
    for (; i0 < t1; i0 += B) {  // the segment's own rows
      double v[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {  // (rows past the tile's end repeat its last row and are not stored)
        const int64_t i = i0 + b;
        v[b] = x[compose_row(src + (i < t1 ? i : t1 - 1), N) * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (i0 + b < t1) {  // (wave-uniform)
          const double y = compose_place(own, v[b], lane);
          const int64_t r = dst + i0 + b;
          if (live && r >= 0 && r < M) w[r * nq] = y;
        }
      }
    }
  }
}

}  // namespace gmr
