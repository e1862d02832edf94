// lowpass_kernel.hip.h -- the zero-phase 2nd-order Butterworth low-pass of qpos in front of the tracking export
// (gmr_track_input.lowpass_hz; the definition is the contract above gmr_track_input in include/gmr_amd.h).
//
// What a consumer does on the host with scipy.signal.filtfilt per clip and column, as one launch: the odd extension by
// e = min(9, T - 1) samples, a forward and a backward pass of the transposed direct form II section started in its steady
// state, the root quaternion made sign-continuous before and normalised after.
//
// One wavefront per clip of one member (a clip without frames returns at once), lane = qpos column (nq <= 64; the lanes past
// nq repeat the last column and store nothing), all filtered members in one grid.  Lane c reads qpos[(o + i) nq + c], so a row
// is one coalesced access.  The time loop is a dependent recurrence of four float64 operations per sample, so the rows are
// fetched kLowpassBatch = 16 ahead of it: while one batch of 16 rows is filtered the loads of the next are in flight.
//
//   A  rows 0 .. e (10 loads in flight), made sign-continuous; the left padding 2 x[0] - x[j] only advances the state
//   B  forward over the clip: sign, step, the result into the member's scratch image; the last 32 sign decisions are kept as bits
//   C  rows T-1-e .. T-1 again (out of the cache), signed from those bits; the e forward results of the right padding stay in
//      registers
//   D  backward: the right padding advances the state, then the lane's own scratch values from row T-1 down to row 0, each
//      overwritten in place by its result (the quaternion lanes divide by the norm first).  The left padding is skipped: nobody
//      reads its results.
//
// A lane only ever loads what it stored itself, in program order, so there is no traffic between lanes through memory and no
// fence.  The four quaternion lanes (3 .. 6) exchange through v_readlane: once per frame in B for the dot product that decides
// the sign, once per frame in D for the norm.  Every lane takes part in every exchange (control flow is wave-uniform).
// No LDS.  One long clip is one wavefront walking 2 (T + 2 e) dependent steps; a scan over time would shorten that chain and is
// not built.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"  // kFkWave
#include "member_launch.hip.h"

namespace gmr {

constexpr int kLowpassPad = 9;     // scipy's padlen for a 2nd-order filter: 3 * max(len(a), len(b))
constexpr int kLowpassBatch = 16;  // rows fetched ahead of the recurrence
constexpr int kLowpassMaxNq = kFkWave;

// One member's arguments of a launch, read by the kernel through the constant address space.
struct LowpassEntry {
  const double *src;           // qpos [n_frames][nq]
  double *dst;                 // the scratch image [n_frames][nq]: the filtered qpos
  const int64_t *seq_offsets;  // device copy, [n_seq + 1]
  const double *coef;          // device copy, [n_seq][5]: b0 b1 b2 a1 a2 of every clip
  int64_t clip_base;           // first workgroup of this member
  int n_seq, nq;               // n_seq = 0: this member is not filtered
};

// lane L's value in every lane
template <int L>
__device__ __forceinline__ double lowpass_lane(double v) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), L), hi = __builtin_amdgcn_readlane(__double2hiint(v), L);
  return __hiloint2double(hi, lo);
}

// ((p[3] + p[4]) + p[5]) + p[6] over the four quaternion lanes, in every lane
__device__ __forceinline__ double lowpass_quat_sum(double p) {
#pragma clang fp contract(off)
  return ((lowpass_lane<3>(p) + lowpass_lane<4>(p)) + lowpass_lane<5>(p)) + lowpass_lane<6>(p);
}

// One pass of the section, transposed direct form II.
struct LowpassSection {
  double b0, b1, b2, a1, a2, z1, z2;
  __device__ __forceinline__ void start(double u) {  // lfilter_zi times the first sample
#pragma clang fp contract(off)
    z1 = (1.0 - b0) * u;
    z2 = (b2 - a2) * u;
  }
  __device__ __forceinline__ double step(double x) {
#pragma clang fp contract(off)
    const double y = b0 * x + z1;
    z1 = (b1 * x - a1 * y) + z2;
    z2 = b2 * x - a2 * y;
    return y;
  }
};

__global__ void __launch_bounds__(kFkWave) lowpass_kernel(const LowpassEntry *entries, int n_entries) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kLowpassBatch, P = kLowpassPad;
  const int lane = threadIdx.x;
  const int ei = launch_member<LowpassEntry, &LowpassEntry::clip_base>(entries, n_entries, (int64_t)blockIdx.x);
  const LowpassEntry *ep = entries + ei;
  const int nq = motion_const(&ep->nq);
  const int s = (int)((int64_t)blockIdx.x - motion_const(&ep->clip_base));
  if (s >= motion_const(&ep->n_seq)) return;
  const int64_t *offs = motion_const(&ep->seq_offsets);
  const int64_t o = motion_const(offs + s), T = motion_const(offs + s + 1) - o;
  if (T <= 0) return;
  const bool live = lane < nq, quat = lane >= 3 && lane < 7;
  const int c = live ? lane : nq - 1;
  const double *x = motion_const(&ep->src) + o * nq + c;  // row i of this lane's column: x[i * nq]
  double *w = motion_const(&ep->dst) + o * nq + c;
  if (T == 1) {  // a copy; the quaternion is normalised like every other
    double v = x[0];
    const double n = sqrt(lowpass_quat_sum(v * v));
    if (quat) v = v / n;
    if (live) w[0] = v;
    return;
  }
  const double *cf = motion_const(&ep->coef) + (int64_t)5 * s;
  LowpassSection f;
  f.b0 = motion_const(cf); f.b1 = motion_const(cf + 1); f.b2 = motion_const(cf + 2); f.a1 = motion_const(cf + 3); f.a2 = motion_const(cf + 4);
  f.z1 = f.z2 = 0.0;
  LowpassSection g = f;
  const int e = T - 1 < P ? (int)(T - 1) : P;
  // ---- A: the head of the clip and the left padding
  double h[P + 1];
#pragma unroll
  for (int j = 0; j <= P; ++j) h[j] = x[(int64_t)(j < e ? j : e) * nq];
#pragma unroll
  for (int j = 1; j <= P; ++j) {  // (rows past e repeat row e and are not used)
    const double d = lowpass_quat_sum(h[j - 1] * h[j]);
    if (quat && d < 0.0) h[j] = -h[j];
  }
#pragma unroll
  for (int j = P; j >= 1; --j) {
    if (j <= e) {  // (wave-uniform)
      const double v = 2.0 * h[0] - h[j];
      if (j == e) f.start(v);
      f.step(v);
    }
  }
  // ---- B: forward over the clip.  prev starts as row 0 itself: its product with row 0 is a sum of squares, never < 0
  double prev = h[0];
  unsigned hist = 0;  // bit k: row (current - k) was negated
  {
    double cur[B], nxt[B];
#pragma unroll
    for (int b = 0; b < B; ++b) cur[b] = x[(b < T - 1 ? b : T - 1) * nq];
    for (int64_t i0 = 0; i0 < T; i0 += B) {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int64_t i = i0 + B + b;
        nxt[b] = x[(i < T - 1 ? i : T - 1) * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (i0 + b < T) {  // (wave-uniform)
          double v = cur[b];
          const bool neg = lowpass_quat_sum(prev * v) < 0.0;
          if (quat && neg) v = -v;
          prev = v;
          hist = (hist << 1) | (neg ? 1u : 0u);
          const double y = f.step(v);
          if (live) w[(i0 + b) * nq] = y;
        }
      }
#pragma unroll
      for (int b = 0; b < B; ++b) cur[b] = nxt[b];
    }
  }
  // ---- C: the right padding 2 x[T-1] - x[T-1-j], j = 1 .. e; its forward results stay in registers
  double r[P + 1];
  {
    double t[P + 1];
#pragma unroll
    for (int j = 1; j <= P; ++j) t[j] = x[(T - 1 - (j < e ? j : e)) * nq];
#pragma unroll
    for (int j = 1; j <= P; ++j) {
      r[j] = 0.0;
      if (j <= e) {
        double v = t[j];
        if (quat && ((hist >> j) & 1u)) v = -v;
        r[j] = f.step(2.0 * prev - v);
      }
    }
  }
  // ---- D: backward.  The forward result reversed: the right padding, then rows T-1 .. 0 of the scratch image, in place
#pragma unroll
  for (int j = P; j >= 1; --j) {
    if (j <= e) {
      if (j == e) g.start(r[j]);
      g.step(r[j]);
    }
  }
  {
    double cur[B], nxt[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int64_t i = T - 1 - b;
      cur[b] = w[(i > 0 ? i : 0) * nq];
    }
    for (int64_t i0 = T - 1; i0 >= 0; i0 -= B) {
#pragma unroll
      for (int b = 0; b < B; ++b) {  // rows below this batch: none of them is overwritten before its own batch
        const int64_t i = i0 - B - b;
        nxt[b] = w[(i > 0 ? i : 0) * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (i0 - b >= 0) {  // (wave-uniform)
          double y = g.step(cur[b]);
          const double n = sqrt(lowpass_quat_sum(y * y));
          if (quat) y = y / n;
          if (live) w[(i0 - b) * nq] = y;
        }
      }
#pragma unroll
      for (int b = 0; b < B; ++b) cur[b] = nxt[b];
    }
  }
}

}  // namespace gmr
