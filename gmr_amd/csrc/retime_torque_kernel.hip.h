// retime_torque_kernel.hip.h -- the two kernels gmr_motion_retime_plan_torque adds to the plan of retime_kernel.hip.h: the need from
// joint torques in front of motion_retime_ticks_kernel and motion_retime_scan_kernel, and the end alignment behind them (the
// definition is the contract above gmr_retime_torque_input in include/gmr_amd.h).  One wavefront per workgroup, vector stores only,
// no atomics, no scratch.
//
// motion_retime_torque_need_kernel  grid (clips, wavefronts per clip), tiles of kRetimeTile rows: the velocity need kernel's.  Lane =
//                             hinge column (nh <= 57; the lanes past nh repeat the last column and do not enter), so a row of tau
//                             and a row of tau_static are one coalesced load each; kRetimeTorqueBatch rows of both are loaded
//                             before the first is reduced (8: at the velocity kernel's 16 the unrolled batch's wave-uniform row
//                             state cost 124 spilled SGPRs and 118 VGPRs, at 8 it is 36 and 70).  A row's largest e is a reduction in the VALU (wave_max), its non-finite test and
//                             its static count are ballots, and lane r keeps row r's three values: a tile takes ONE square root for
//                             its 64 rows, gets the next row's values from the neighbouring lane (the tile's 65th row, which the
//                             next tile loads again, is the only row loaded twice) and stores need and static_over coalesced.
//                             16 nh bytes read per frame.
// motion_retime_align_kernel  one wavefront per clip, after the scan.  Lane = one of the clip's last k <= 64 intervals: its share of
//                             the ticks that round the clip's total up to whole frames, an inclusive scan of the shares over the
//                             lanes for cum, and lane 0 rewrites out_len and the total.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "retime_kernel.hip.h"  // retime_clip, kRetimeTile, kRetimeQ; wave_max through it

namespace gmr {

constexpr int kRetimeAlignSpan = 64;   // the intervals at a clip's end that share the alignment ticks: one per lane
constexpr int kRetimeTorqueBatch = 8;  // rows of tau and of tau_static in flight per batch of the torque need kernel: 16 loads

struct RetimeTorqueArgs {
  const double *tau;           // [n_frames][nh]
  const double *tau_static;    // [n_frames][nh]
  const int64_t *seq_offsets;  // device, [n_seq + 1]
  const double *torque_limit;  // device, [nh]
  const double *need_floor;    // [n_frames], or null
  double *need;                // [n_frames]
  int32_t *static_over;        // [n_frames], or null
  double limit_scale;
  int64_t n_frames;
  int n_seq, nh;
};

__global__ void __launch_bounds__(kFkWave) motion_retime_torque_need_kernel(RetimeTorqueArgs A) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  constexpr int B = kRetimeTorqueBatch;
  const int lane = threadIdx.x, nh = A.nh;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T);
  if ((int64_t)blockIdx.y * kRetimeTile >= T) return;  // (a clip without frames, and the wavefronts past a short clip's last tile)
  const bool hinge = lane < nh;
  const int c = hinge ? lane : (nh > 0 ? nh - 1 : 0);
  const double inf = __builtin_huge_val(), nan = __longlong_as_double(0x7ff8000000000000LL);
  const double lim = hinge ? A.torque_limit[lane] : inf;
  const bool limited = hinge && lim < inf;
  const double L = A.limit_scale * lim;
  const double *x = A.tau + o * nh + c, *g0 = A.tau_static + o * nh + c;
  for (int64_t t0 = (int64_t)blockIdx.y * kRetimeTile; t0 < T; t0 += (int64_t)gridDim.y * kRetimeTile) {
    const int64_t t1 = t0 + kRetimeTile < T ? t0 + kRetimeTile : T;  // the tile's rows are t0 .. t1 - 1; its intervals need row t1 too
    const int64_t tr = t1 < T ? t1 + 1 : T;                          // one past the last row this tile reduces
    double e_mine = 0.0, e_next = 0.0;   // the largest e of row t0 + lane, and of row t0 + 64 (wave-uniform)
    bool bad_mine = false, bad_next = false;
    int over_mine = 0;
    for (int64_t i0 = t0; i0 < tr; i0 += B) {
      double v[B], g[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {  // (wave-uniform: nothing is loaded past the last row, or for a model without hinges)
        const bool on = nh > 0 && i0 + b < tr;
        v[b] = on ? x[(i0 + b) * nh] : 0.0;
        g[b] = on ? g0[(i0 + b) * nh] : 0.0;
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int64_t i = i0 + b;
        if (i < tr) {  // (wave-uniform)
          const bool bad = __ballot(hinge && (!(fabs(v[b]) < inf) || !(fabs(g[b]) < inf))) != 0;
          const double d = v[b] - g[b];
          const double head = d >= 0.0 ? L - g[b] : L + g[b];
          const double e = limited && head > 0.0 ? fabs(d) / head : 0.0;
          const double mx = wave_max(bad ? 0.0 : e);
          const int over = bad ? 0 : __popcll(__ballot(limited && fabs(g[b]) >= L));
          const int r = (int)(i - t0);  // 0 .. 64
          if (lane == r) { e_mine = mx; bad_mine = bad; over_mine = over; }
          if (r == kRetimeTile) { e_next = mx; bad_next = bad; }
        }
      }
    }
    // lane = row: rho, the next row's from the neighbouring lane, the interval
    const double rho = sqrt(e_mine), rho_tile_next = sqrt(e_next);
    double rho_n = __shfl_down(rho, 1);
    bool bad_n = __shfl_down((int)bad_mine, 1) != 0;
    if (lane == kRetimeTile - 1) { rho_n = rho_tile_next; bad_n = bad_next; }
    const int64_t i = t0 + lane;
    if (i < t1) {
      double need = 0.0;  // the clip's last row has no interval
      if (i < T - 1) {
        need = fmax(rho, rho_n);
        bool nonfinite = bad_mine || bad_n;
        if (A.need_floor) {
          const double fl = A.need_floor[o + i];
          need = fmax(need, fl);
          nonfinite = nonfinite || !(fl < inf);
        }
        if (nonfinite) need = nan;
      }
      A.need[o + i] = need;
      if (A.static_over) A.static_over[o + i] = over_mine;
    }
  }
}

struct RetimeAlignArgs {
  const int64_t *seq_offsets;  // device, [n_seq + 1]
  int64_t *ticks;              // [n_frames]
  int64_t *cum;                // [n_frames]
  int64_t *out_len;            // [n_seq]
  int64_t *clip_stats;         // [n_seq][4]
  int64_t n_frames;
  int n_seq;
};

__global__ void __launch_bounds__(kFkWave) motion_retime_align_kernel(RetimeAlignArgs A) {
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (s >= A.n_seq) return;
  int64_t T;
  const int64_t o = retime_clip(A.seq_offsets, s, A.n_frames, T);
  if (T < 2) return;  // (nothing to align: the scan's results stand)
  const int64_t t = A.cum[o + T - 1];
  const int64_t r = (kRetimeQ - t % kRetimeQ) % kRetimeQ;
  if (r <= 0 || r >= kRetimeQ) return;  // (whole frames already; a total that is not the scan's leaves the clip alone)
  const int k = T - 1 < kRetimeAlignSpan ? (int)(T - 1) : kRetimeAlignSpan;
  const int64_t iv = T - 1 - k + lane;  // this lane's interval
  const bool mine = lane < k;
  long long incl = mine ? (long long)(r / k + (lane < r % k ? 1 : 0)) : 0;
  const long long add = incl;
#pragma unroll
  for (int d = 1; d < kFkWave; d <<= 1) {
    const long long up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (mine) {
    A.ticks[o + iv] = A.ticks[o + iv] + (int64_t)add;
    A.cum[o + iv + 1] = A.cum[o + iv + 1] + (int64_t)incl;  // the last row holds the total
  }
  if (lane == 0) {
    A.out_len[s] = (t + r) / kRetimeQ + 1;
    A.clip_stats[(int64_t)s * 4 + 3] = t + r;
  }
}

}  // namespace gmr
