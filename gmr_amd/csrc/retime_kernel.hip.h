// retime_kernel.hip.h -- clips played slower exactly where a hinge turns faster than its limit (gmr_motion_retime_plan and
// gmr_motion_retime_apply; the definition is the contract above gmr_retime_plan_input in include/gmr_amd.h).
//
// Four kernels, one wavefront per workgroup, no atomics, no scratch: need, ticks and cum are the caller's arrays and the hand-over.
//
// motion_retime_need_kernel   grid (clips, wavefronts per clip), tiles of kRetimeTile rows.  Lane = column (nq <= 64; the lanes past
//                             nq repeat the last column), so a row is one coalesced load; kRetimeBatch + 1 rows are loaded before
//                             the first interval is reduced, and every row but a batch's last is loaded once.  A hinge lane divides
//                             its |step| fps by its vmax; the interval's maximum is a reduction in the VALU (wave_max: six DPP
//                             hops, no LDS round trip) and the non-finite test one ballot.  Lane r keeps row r's need, so that a tile
//                             stores its 64 values in one coalesced store.  This is the kernel that reads qpos: 8 nq bytes a frame.
// motion_retime_ticks_kernel  the same grid.  Lane = row.  A tile stages the stretches s of its rows and of 2 W intervals on either
//                             side in LDS (they cross the tile's edges; outside the clip they are 0, below every stretch), takes the
//                             windowed maximum d for its rows and W on either side into LDS, and then each lane sums its window of
//                             d in ascending order.  8 bytes read and written per frame (the halo comes out of the cache).
// motion_retime_scan_kernel   THE PER-CLIP KERNEL: one wavefront per clip walks the clip's tiles in order, kRetimeScanTiles of them
//                             loaded at a time, and carries the exact integer sum of ticks from tile to tile (an inclusive scan
//                             over the lanes, then lane 63's total).  It also counts the clip's statistics from need.  8 192 clips
//                             are 8 192 wavefronts; ONE clip of 10^6 frames is one wavefront that takes 15 625 tiles of 24 bytes a
//                             row one group after the other: latency-bound, milliseconds, while the other two kernels spread that
//                             clip over the chip.  No scratch means no tile sums to scan in parallel.
// motion_retime_apply_kernel  grid (clips, wavefronts per clip), tiles of kRetimeTile OUTPUT rows.  First lane = output row: each
//                             lane finds its interval by a binary search of cum (every interval has at least Q ticks, so row k
//                             lies in an interval <= k), computes u and src_time, stores src_time coalesced, and -- where u != 0 and
//                             the two root quaternions differ -- its row's slerp: 64 rows' acos and sines side by side instead of
//                             one after the other.  Then lane = column: the rows go in batches of kRetimeApplyBatch, the row's
//                             interval, u and quaternion come from its lane through v_readlane, both source rows are loaded
//                             coalesced (the second is the next row's first: it comes out of the cache) and the row is stored.
// motion_retime_apply_cubic_kernel, at the end of this file, is the apply with interp = 1: the same structure over a four-row stencil.
// The two kernels that gmr_motion_retime_plan_torque puts around the ticks and scan kernels are in retime_torque_kernel.hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"      // kFkWave
#include "ik_kernel.hip.h"      // wave_max, rdlane
#include "member_launch.hip.h"  // motion_const
#include "track_kernel.hip.h"   // track_lerp, track_slerp

namespace gmr {

constexpr int kRetimeMaxNq = kFkWave;
constexpr int kRetimeTile = 64;            // rows of one tile
constexpr int kRetimeBatch = 16;           // intervals reduced per batch of the need kernel: 17 rows in flight
constexpr int kRetimeApplyBatch = 8;       // output rows per batch of the apply kernel: 16 rows in flight
constexpr int kRetimeScanTiles = 4;        // tiles the scan kernel loads before it scans the first
constexpr int kRetimeTargetWaves = 16384;  // wavefronts the host aims at in one launch (the mirror's figure)
constexpr int kRetimeMaxWindow = 32;       // W: the ticks kernel's LDS holds a tile and 2 W intervals on either side
constexpr int64_t kRetimeQ = 1024;         // ticks per source frame

struct RetimePlanArgs {
  const double *qpos;          // [n_frames][nq]
  const int64_t *seq_offsets;  // device, [n_seq + 1]
  const double *vmax;          // device, [nq - 7]
  double *need;                // [n_frames]
  int64_t *ticks;              // [n_frames]
  int64_t *cum;                // [n_frames]
  int64_t *out_len;            // [n_seq]
  int64_t *clip_stats;         // [n_seq][4]
  double *need_max;            // [n_seq]
  double fps, max_stretch;
  int64_t n_frames;
  int n_seq, nq, window;
};

struct RetimeApplyArgs {
  const double *qpos;          // [n_frames][nq]
  const int64_t *seq_offsets;  // device, [n_seq + 1]
  const int64_t *out_offsets;  // device, [n_seq + 1]
  const int64_t *ticks;        // [n_frames]
  const int64_t *cum;          // [n_frames]
  double *out;                 // [n_out_frames][nq], not qpos
  double *src_time;            // [n_out_frames]
  int64_t n_frames, n_out_frames;
  int n_seq, nq;
};

// clip s of `offsets`, clamped into [0, N]: its first row and its rows
__device__ __forceinline__ int64_t retime_clip(const int64_t *offsets, int s, int64_t N, int64_t &rows) {
  int64_t o = motion_const(offsets + s), e = motion_const(offsets + s + 1);
  o = o < 0 ? 0 : (o > N ? N : o);
  e = e < o ? o : (e > N ? N : e);
  rows = e - o;
  return o;
}

// lane `r`'s value in every lane; r is wave-uniform
__device__ __forceinline__ int64_t retime_lane64(int64_t v, int r) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, r);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), r);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ void __launch_bounds__(kFkWave) motion_retime_need_kernel(RetimePlanArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kRetimeBatch;
  const int lane = threadIdx.x, nq = A.nq;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T);
  if ((int64_t)blockIdx.y * kRetimeTile >= T) return;  // (a clip without frames, and the wavefronts past a short clip's last tile)
  const int c = lane < nq ? lane : nq - 1;
  const bool hinge = lane >= 7 && lane < nq;
  const double vm = hinge ? A.vmax[lane - 7] : 1.0;
  const double fps = A.fps, inf = __builtin_huge_val(), nan = __longlong_as_double(0x7ff8000000000000LL);
  const double *x = A.qpos + o * nq + c;
  for (int64_t t0 = (int64_t)blockIdx.y * kRetimeTile; t0 < T; t0 += (int64_t)gridDim.y * kRetimeTile) {
    const int64_t t1 = t0 + kRetimeTile < T ? t0 + kRetimeTile : T;
    double mine = 0.0;  // the need of row t0 + lane
    for (int64_t i0 = t0; i0 < t1; i0 += B) {
      double v[B + 1];
#pragma unroll
      for (int b = 0; b <= B; ++b) {  // (rows past the clip's end repeat its last row: that row's interval is overwritten below)
        const int64_t i = i0 + b;
        v[b] = x[(i < T ? i : T - 1) * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int64_t i = i0 + b;
        if (i < t1) {  // (wave-uniform)
          double nd = 0.0;  // root columns and idle lanes do not enter
          if (hinge) nd = (fabs(v[b + 1] - v[b]) * fps) / vm;
          const bool bad = !(nd < inf);
          const bool any = __ballot(bad) != 0;
          const double mx = wave_max(bad ? 0.0 : nd);
          double need = any ? nan : mx;
          if (i == T - 1) need = 0.0;  // the clip's last row has no interval
          if (lane == (int)(i - t0)) mine = need;
        }
      }
    }
    if (t0 + lane < t1) A.need[o + t0 + lane] = mine;
  }
}

__global__ void __launch_bounds__(kFkWave) motion_retime_ticks_kernel(RetimePlanArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  __shared__ double ss[kRetimeTile + 4 * kRetimeMaxWindow];  // s of the intervals t0 - 2 W ... t0 + 63 + 2 W
  __shared__ double sd[kRetimeTile + 2 * kRetimeMaxWindow];  // d of the intervals t0 - W ... t0 + 63 + W
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T);
  if ((int64_t)blockIdx.y * kRetimeTile >= T) return;
  const int W = A.window < 0 ? 0 : (A.window > kRetimeMaxWindow ? kRetimeMaxWindow : A.window);
  const double cap = A.max_stretch, inf = __builtin_huge_val();
  const int64_t nI = T - 1;  // the clip's intervals
  for (int64_t t0 = (int64_t)blockIdx.y * kRetimeTile; t0 < T; t0 += (int64_t)gridDim.y * kRetimeTile) {
    for (int p = lane; p < kRetimeTile + 4 * W; p += kFkWave) {
      const int64_t k = t0 - 2 * W + p;
      double sv = 0.0;  // outside the clip: below every stretch
      if (k >= 0 && k < nI) {
        const double nd = A.need[o + k];
        sv = nd < inf ? fmin(fmax(1.0, nd), cap) : 1.0;  // (a non-finite interval stretches as 1)
      }
      ss[p] = sv;
    }
    __syncthreads();
    for (int p = lane; p < kRetimeTile + 2 * W; p += kFkWave) {  // interval k = t0 - W + p: s of k - W ... k + W is ss[p ... p + 2 W]
      double d = 0.0;
      for (int j = 0; j <= 2 * W; ++j) d = fmax(d, ss[p + j]);
      sd[p] = d;
    }
    __syncthreads();
    const int64_t i = t0 + lane;
    if (i < T) {
      int64_t tk = 0;  // the clip's last row
      if (i < nI) {
        const int lo = i - W < 0 ? (int)-i : -W, hi = i + W > nI - 1 ? (int)(nI - 1 - i) : W;  // the window, relative to i
        double sum = sd[lane + W + lo];
        for (int k = lo + 1; k <= hi; ++k) sum = sum + sd[lane + W + k];
        const double m = sum / (double)(hi - lo + 1);
        tk = (int64_t)ceil(m * 1024.0);
      }
      A.ticks[o + i] = tk;
    }
    __syncthreads();  // the next tile overwrites both arrays
  }
}

__global__ void __launch_bounds__(kFkWave) motion_retime_scan_kernel(RetimePlanArgs A) {
  constexpr int U = kRetimeScanTiles;
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T);
  const double cap = A.max_stretch, inf = __builtin_huge_val();
  int64_t carry = 0, stretched = 0, capped = 0, nonfinite = 0;  // (wave-uniform)
  double nmax = 0.0;                                           // this lane's rows
  for (int64_t t0 = 0; t0 < T; t0 += (int64_t)U * kRetimeTile) {
    long long tk[U];
    double nd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = t0 + u * kRetimeTile + lane;
      tk[u] = i < T ? (long long)A.ticks[o + i] : 0;
      nd[u] = i < T ? A.need[o + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t0 + u * kRetimeTile < T) {  // (wave-uniform)
        const int64_t i = t0 + u * kRetimeTile + lane;
        long long incl = tk[u];
#pragma unroll
        for (int d = 1; d < kFkWave; d <<= 1) {
          const long long up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        if (i < T) A.cum[o + i] = carry + (int64_t)(incl - tk[u]);  // the earlier intervals: the last row holds the total
        carry += (int64_t)__shfl(incl, kFkWave - 1);
        const bool interval = i < T - 1;
        stretched += __popcll(__ballot(interval && nd[u] > 1.0));
        capped += __popcll(__ballot(interval && nd[u] > cap));
        nonfinite += __popcll(__ballot(interval && !(nd[u] < inf)));
        if (interval && nd[u] < inf) nmax = fmax(nmax, nd[u]);
      }
    }
  }
  nmax = wave_max(nmax);
  if (lane == 0) {
    A.out_len[s] = T == 0 ? 0 : (carry + kRetimeQ - 1) / kRetimeQ + 1;
    int64_t *st = A.clip_stats + (int64_t)s * 4;
    st[0] = stretched; st[1] = capped; st[2] = nonfinite; st[3] = carry;
    A.need_max[s] = nmax;
  }
}

__global__ void __launch_bounds__(kFkWave) motion_retime_apply_kernel(RetimeApplyArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kRetimeApplyBatch;
  const int lane = threadIdx.x, nq = A.nq;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T, M;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T), oo = retime_clip(A.out_offsets, s, A.n_out_frames, M);
  if (T == 0 || (int64_t)blockIdx.y * kRetimeTile >= M) return;  // (a clip without frames writes nothing)
  const bool live = lane < nq, quat = lane >= 3 && lane < 7;
  const int c = live ? lane : nq - 1;
  const int64_t *cum = A.cum + o, *ticks = A.ticks + o;
  const int64_t total = cum[T - 1];
  const double *x = A.qpos + o * nq + c;
  double *w = A.out + oo * nq + c;
  for (int64_t t0 = (int64_t)blockIdx.y * kRetimeTile; t0 < M; t0 += (int64_t)gridDim.y * kRetimeTile) {
    const int64_t t1 = t0 + kRetimeTile < M ? t0 + kRetimeTile : M;
    // lane = output row (the lanes past the tile's end repeat its last row and store nothing)
    const int64_t k = t0 + lane < t1 ? t0 + lane : t1 - 1;
    const int64_t tau = k * kRetimeQ;
    const bool end = tau >= total || T < 2;
    int64_t i = T - 1;
    double u = 0.0;
    // the interval with cum[i] <= tau < cum[i + 1]: the last i in [0, min(k, T - 2)] with cum[i] <= tau.  Every index is inside the
    // clip whatever cum holds.
    const int64_t top = T - 2 < t1 - 1 ? T - 2 : t1 - 1;                                    // (wave-uniform)
    const int steps = top < 1 ? 0 : 64 - __builtin_clzll((unsigned long long)top);          // >= log2(top + 1)
    int64_t lo = 0, hi = k < T - 2 ? k : T - 2;
    for (int it = 0; it < steps; ++it) {
      if (!end && lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (cum[mid] <= tau) lo = mid; else hi = mid - 1;
      }
    }
    if (!end) {
      i = lo;
      u = (double)(tau - cum[i]) / (double)ticks[i];
    }
    if (t0 + lane < t1) A.src_time[oo + t0 + lane] = (double)i + u;
    // this row's root quaternion where it is neither a copy nor the same in both rows
    bool turn = !end && u != 0.0;
    double qr[4] = {0.0, 0.0, 0.0, 0.0};
    if (turn) {
      const double *p0 = A.qpos + (o + i) * nq + 3, *p1 = p0 + nq;  // (i <= T - 2)
      double q0[4], q1[4];
      bool same = true;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q0[j] = p0[j];
        q1[j] = p1[j];
        same = same && __double_as_longlong(q0[j]) == __double_as_longlong(q1[j]);
      }
      turn = !same;
      if (turn) track_slerp(q0, q1, u, qr);  // wxyz as stored
    }
    // lane = column
    for (int64_t i0 = t0; i0 < t1; i0 += B) {
      double v0[B], v1[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {  // (rows past the tile's end repeat its last row and are not stored)
        const int r = (int)((i0 + b < t1 ? i0 + b : t1 - 1) - t0);
        const int64_t ir = retime_lane64(i, r);
        const int64_t jr = rdlane(u, r) != 0.0 && ir + 1 < T ? ir + 1 : ir;
        v0[b] = x[ir * nq];
        v1[b] = x[jr * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (i0 + b < t1) {  // (wave-uniform)
          const int r = (int)(i0 + b - t0);
          double y = track_lerp(v0[b], v1[b], rdlane(u, r));
          if (__builtin_amdgcn_readlane((int)turn, r)) {  // (wave-uniform)
            const double qw = rdlane(qr[0], r), qx = rdlane(qr[1], r), qy = rdlane(qr[2], r), qz = rdlane(qr[3], r);
            if (quat) y = lane == 3 ? qw : lane == 4 ? qx : lane == 5 ? qy : qz;
          } else if (quat) {
            y = v0[b];  // u == 0, or the same quaternion in both rows: a copy
          }
          if (live) w[(i0 + b) * nq] = y;
        }
      }
    }
  }
}

// The sample point of output row k of a clip of T rows: the interval i and u of the contract, by the linear kernel's search (the
// last i in [0, min(k, T - 2)] with cum[i] <= tau; every index is inside the clip whatever cum holds).  `top` bounds the search's
// steps for the whole wavefront.  This is a second copy of the search written out inside motion_retime_apply_kernel, which keeps its
// own so that its code object stays what it was: the two must stay in step.
__device__ __forceinline__ void retime_sample_point(const int64_t *cum, const int64_t *ticks, int64_t T, int64_t total, int64_t k,
                                                    int64_t top, int64_t &i, double &u, bool &end) {
  const int64_t tau = k * kRetimeQ;
  end = tau >= total || T < 2;
  i = T - 1;
  u = 0.0;
  const int steps = top < 1 ? 0 : 64 - __builtin_clzll((unsigned long long)top);  // >= log2(top + 1)
  int64_t lo = 0, hi = k < T - 2 ? k : T - 2;
  for (int it = 0; it < steps; ++it) {
    if (!end && lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (cum[mid] <= tau) lo = mid; else hi = mid - 1;
    }
  }
  if (!end) {
    i = lo;
    u = (double)(tau - cum[i]) / (double)ticks[i];
  }
}

// y of the contract's cubic for one column: Catmull-Rom tangents from the four rows, Horner in u
__device__ __forceinline__ double retime_cubic(double p0, double p1, double p2, double p3, double u) {
#pragma clang fp contract(off)
  const double m1 = 0.5 * (p2 - p0), m2 = 0.5 * (p3 - p1), c = p2 - p1;
  return p1 + u * (m1 + u * (((3.0 * c - 2.0 * m1) - m2) + u * ((m1 + m2) - 2.0 * c)));
}

// motion_retime_apply_cubic_kernel  interp = 1 of gmr_motion_retime_apply: the linear kernel's structure with a four-row stencil.
//                             First lane = output row: the search, src_time and -- where u != 0 -- the row's root quaternion: the
//                             three neighbours flipped onto row i's hemisphere, the missing neighbour of an end interval reflected,
//                             the cubic per component, one norm.  Then lane = column: batches of kRetimeApplyBatch rows, four
//                             coalesced source rows each (three of them are the neighbouring output rows': they come out of the
//                             cache), and the row is stored.  A row with u == 0 or past the warp's end reads row i alone.
__global__ void __launch_bounds__(kFkWave) motion_retime_apply_cubic_kernel(RetimeApplyArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kRetimeApplyBatch;
  const int lane = threadIdx.x, nq = A.nq;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T, M;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T), oo = retime_clip(A.out_offsets, s, A.n_out_frames, M);
  if (T == 0 || (int64_t)blockIdx.y * kRetimeTile >= M) return;  // (a clip without frames writes nothing)
  const bool live = lane < nq, quat = lane >= 3 && lane < 7;
  const int c = live ? lane : nq - 1;
  const int64_t *cum = A.cum + o, *ticks = A.ticks + o;
  const int64_t total = cum[T - 1];
  const double *x = A.qpos + o * nq + c;
  double *w = A.out + oo * nq + c;
  for (int64_t t0 = (int64_t)blockIdx.y * kRetimeTile; t0 < M; t0 += (int64_t)gridDim.y * kRetimeTile) {
    const int64_t t1 = t0 + kRetimeTile < M ? t0 + kRetimeTile : M;
    // lane = output row (the lanes past the tile's end repeat its last row and store nothing)
    const int64_t k = t0 + lane < t1 ? t0 + lane : t1 - 1;
    int64_t i;
    double u;
    bool end;
    retime_sample_point(cum, ticks, T, total, k, T - 2 < t1 - 1 ? T - 2 : t1 - 1, i, u, end);
    if (t0 + lane < t1) A.src_time[oo + t0 + lane] = (double)i + u;
    const bool turn = !end && u != 0.0;  // (then i <= T - 2)
    double qr[4] = {0.0, 0.0, 0.0, 0.0};
    if (turn) {
      const double *r1 = A.qpos + (o + i) * nq + 3;
      const double *r0 = i > 0 ? r1 - nq : r1, *r2 = r1 + nq, *r3 = i + 2 < T ? r2 + nq : r2;
      double q0[4], q1[4], q2[4], q3[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { q0[j] = r0[j]; q1[j] = r1[j]; q2[j] = r2[j]; q3[j] = r3[j]; }
      const bool f0 = ((q0[0] * q1[0] + q0[1] * q1[1]) + q0[2] * q1[2]) + q0[3] * q1[3] < 0.0;
      const bool f2 = ((q2[0] * q1[0] + q2[1] * q1[1]) + q2[2] * q1[2]) + q2[3] * q1[3] < 0.0;
      const bool f3 = ((q3[0] * q1[0] + q3[1] * q1[1]) + q3[2] * q1[2]) + q3[3] * q1[3] < 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double b1 = q1[j], b2 = f2 ? -q2[j] : q2[j];
        const double b0 = i > 0 ? (f0 ? -q0[j] : q0[j]) : b1 + (b1 - b2);
        const double b3 = i + 2 < T ? (f3 ? -q3[j] : q3[j]) : b2 + (b2 - b1);
        qr[j] = retime_cubic(b0, b1, b2, b3, u);
      }
      const double nrm = sqrt(((qr[0] * qr[0] + qr[1] * qr[1]) + qr[2] * qr[2]) + qr[3] * qr[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) qr[j] = qr[j] / nrm;
    }
    // lane = column
    for (int64_t i0 = t0; i0 < t1; i0 += B) {
      double v0[B], v1[B], v2[B], v3[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {  // (rows past the tile's end repeat its last row and are not stored)
        const int r = (int)((i0 + b < t1 ? i0 + b : t1 - 1) - t0);
        const int64_t ir = retime_lane64(i, r);
        const bool tr = __builtin_amdgcn_readlane((int)turn, r) != 0;  // (wave-uniform)
        v1[b] = x[ir * nq];
        v0[b] = x[(tr && ir > 0 ? ir - 1 : ir) * nq];
        v2[b] = x[(tr ? ir + 1 : ir) * nq];
        v3[b] = x[(tr ? (ir + 2 < T ? ir + 2 : ir + 1) : ir) * nq];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (i0 + b < t1) {  // (wave-uniform)
          const int r = (int)(i0 + b - t0);
          double y = v1[b];  // u == 0, or past the warp's end: a copy
          if (__builtin_amdgcn_readlane((int)turn, r)) {  // (wave-uniform)
            const int64_t ir = retime_lane64(i, r);
            const double p0 = ir > 0 ? v0[b] : v1[b] + (v1[b] - v2[b]);
            const double p3 = ir + 2 < T ? v3[b] : v2[b] + (v2[b] - v1[b]);
            y = retime_cubic(p0, v1[b], v2[b], p3, rdlane(u, r));
            const double qw = rdlane(qr[0], r), qx = rdlane(qr[1], r), qy = rdlane(qr[2], r), qz = rdlane(qr[3], r);
            if (quat) y = lane == 3 ? qw : lane == 4 ? qx : lane == 5 ? qy : qz;
          }
          if (live) w[(i0 + b) * nq] = y;
        }
      }
    }
  }
}

}  // namespace gmr
