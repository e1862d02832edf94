// transitions_kernel.hip.h -- the motion-graph metric between windows of retargeted clips in float64, three launches
// (gmr_motion_transitions; the definition is the contract above gmr_transitions_input in include/gmr_amd.h).
//
//   a  motion_transitions_points_kernel   grid (clip, wavefronts per clip), one wavefront per workgroup.  Phase 1 is the pose sweep of
//                                         self_collision_kernel.hip.h (LANE = BODY with tree_chain's geometry, level by level, 7
//                                         doubles per body left in LDS; the same statements, the same helpers).  Then per frame of the
//                                         pass LANE = POINT: the body's position minus the clip's first-row root (x, y) goes to
//                                         `points`, and lanes 0..2 sum m.x, m.y and q over the points in ascending order.
//   b  motion_transitions_window_kernel   grid (clip, wavefronts per clip), LANE = ROW: the windowed M.x, M.y and Q - |M|^2 of every row
//                                         that starts a full window, from the m, q of a.
//   c  motion_transitions_pair_kernel     the hot path.  A work item is (a run of `tile` sources, a target clip); a wavefront owns it
//                                         and walks the whole target clip itself, so a source's minimum and its tie rule belong to no
//                                         schedule.  A LANE owns one DIAGONAL d = j - i and walks along it: at source row f it computes
//                                         the per-row gram Gd, Gc, Gz of (f, f + d) (P terms), pushes it into a register ring of the
//                                         last LMAX values and re-sums the last L of them in order -- not a running add / subtract
//                                         sum, which would break the contract's order.  The source row is a broadcast read from LDS;
//                                         the 64 target rows the lanes need are a ring of 64 rows in LDS, stored [coordinate][row]
//                                         with a pitch of 65 doubles so that the store of a row and the lanes' reads of a coordinate
//                                         are both free of bank conflicts; one new row enters per step, fetched into registers before
//                                         the step's arithmetic and stored behind it.  At a step every lane holds the cost of
//                                         the SAME source against 64 neighbouring target frames: one wave_min of the cost and one of
//                                         the frame among the lanes at that minimum reduce them, and lane 0 keeps the source's running
//                                         (minimum, frame) in LDS with `<`, diagonals ascending, so the lowest frame of equals stays.
//                                         <LMAX> = 8 serves L <= 8, <32> the rest (96 ring doubles per lane: one wavefront per SIMD).
//
// No atomics, no scratch, no matrix instruction (its accumulation order is not the contract's), and no dense matrix unless cost_out is
// asked for.  Weaknesses, not engineered away: the LDS ring (65 x 3 P doubles: 59 KiB for the 38 bodies of unitree_g1) leaves room for
// two workgroups per CU when all bodies are points; L - 1 steps of every diagonal pass only fill the register ring; every pass refills
// the whole 64-row LDS ring although the next pass reads the same target rows shifted by 64, about half of them again; the corners of
// a pass where j leaves the target clip are computed and dropped; the pose sweep is the third copy of those statements.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "self_collision_kernel.hip.h"  // kColPose, col_clampi; dyn_clamp, dyn_qmul, dyn_rot; chain_geom, wave_lds_sync; wave_min

namespace gmr {

constexpr int kTrMaxBodies = kFkWave;   // points of one call: a lane each in kernel a
constexpr int kTrMaxWindow = 32;        // L of one call: the register ring of kernel c
constexpr int kTrTile = 64;             // sources of a work item of kernel c
constexpr int kTrMaxTile = 256;         // what GMR_AMD_TRANSITIONS_TILE may force
constexpr int kTrPitch = kFkWave + 1;   // doubles between two coordinates of the LDS ring
constexpr int kTrMoments = 6;           // doubles per row of `moments`: m.x m.y q, then M.x M.y Q - |M|^2
constexpr int kTrTargetWaves = 8192;    // wavefronts of one launch of kernels a and b that the host aims for
constexpr int kTrPairWaves = 16384;     // and of kernel c

struct TransitionsArgs {
  const DevModel *dm;            // the full body tree (gmr_evaluate's)
  const double *qpos;
  const int64_t *seq_offsets;
  int64_t n_frames;
  int n_seq, nbody, nq, P, L, stride, min_gap, n_src, n_dst, tile;
  const int32_t *body_ids;
  const double *weights;
  const int32_t *src_clips, *dst_clips;
  const int64_t *src_offsets, *dst_offsets;
  int64_t n_sources, n_targets;
  double *points, *moments, *best_cost;
  int32_t *best_frame;
  double *cost_out;
  uint8_t parent[kFkWave], depth[kFkWave];   // the tree, from the blob (parent of the root: 0xff)
};

// bytes of dynamic LDS of kernel c: the ring of target rows, the source row, the weights, the tile's running (minimum, frame)
__host__ __device__ inline int transitions_pair_lds_bytes(int P, int tile) { return (3 * P * kTrPitch + 3 * P + P + tile) * 8 + tile * 4; }

// ------------------------------------------------------------------ a: points and per-row moments
// grid (n_seq, wavefronts per clip)
__global__ void __launch_bounds__(kFkWave) motion_transitions_points_kernel(const TransitionsArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double pose[kColPose * kFkWave];   // [kColPose][64]
  __shared__ double pxy[2 * kFkWave], wts[kFkWave];
  const int lane = threadIdx.x;
  const int nb = a.nbody, nq = a.nq, P = a.P;
  const ChainGeom geom = chain_geom(nb);   // nb <= 64: jp <= 64
  const int jp = geom.jp, groups = geom.groups;
  const int grp = lane / jp, body = lane - grp * jp;
  const bool active = body < nb;
  const int bj = active ? body : 0;   // (idle lanes read body 0's constants and never write)
  const DevModel *dm = a.dm;

  // the lane's body, once per launch
  const int par = bj > 0 ? col_clampi((int)a.parent[bj], nb - 1) : 0;
  const int depth = a.depth[bj];
  int maxd = active ? depth : 0;
  for (int off = 32; off; off >>= 1) { const int o = __shfl_xor(maxd, off); maxd = o > maxd ? o : maxd; }
  const bool hinge = active && bj > 0 && dm->jtype[bj] == GMR_JNT_HINGE;
  const bool root = active && bj == 0;
  const int qadr = hinge ? dm->qadr[bj] : 7;
  const double bpos[3] = {dm->bpos[3 * bj], dm->bpos[3 * bj + 1], dm->bpos[3 * bj + 2]};
  const double bquat[4] = {dm->bquat[4 * bj], dm->bquat[4 * bj + 1], dm->bquat[4 * bj + 2], dm->bquat[4 * bj + 3]};
  const double axis[3] = {dm->axis[3 * bj], dm->axis[3 * bj + 1], dm->axis[3 * bj + 2]};

  // the lane's point, once per launch
  const bool point = lane < P;
  const int pb = point ? col_clampi(a.body_ids[lane], nb - 1) : 0;
  if (point) wts[lane] = a.weights[lane];
  wave_lds_sync();

  const int64_t r0 = dyn_clamp(a.seq_offsets[blockIdx.x], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[blockIdx.x + 1], r0, a.n_frames);
  const int64_t T = r1 - r0;
  if (T == 0) return;
  const double ox = a.qpos[r0 * nq], oy = a.qpos[r0 * nq + 1];   // the clip's origin: its first row's root (x, y)
  const int slot0 = grp * jp;   // the root's slot of this lane's frame

  for (int64_t k0 = (int64_t)blockIdx.y * groups; k0 < T; k0 += (int64_t)gridDim.y * groups) {
    // ---- 1: poses, LANE = BODY (the sweep of motion_self_collision_kernel)
    const int64_t k = k0 + grp;
    const bool live = active && k < T;
    const int64_t g = r0 + k;
    double th = 0.0, x[3] = {0.0, 0.0, 0.0}, r[4] = {1.0, 0.0, 0.0, 0.0};
    if (live && hinge) th = a.qpos[g * nq + qadr];
    if (live && root) {
      const double *row = a.qpos + g * nq;
      const double qn = sqrt(row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
      x[0] = row[0]; x[1] = row[1]; x[2] = row[2];
      r[0] = row[3] / qn; r[1] = row[4] / qn; r[2] = row[5] / qn; r[3] = row[6] / qn;
    }
    wave_lds_sync();   // (the previous pass no longer reads the buffers)
    for (int d = 0; d <= maxd; ++d) {
      if (live && depth == d) {
        if (d > 0) {
          const int ps = slot0 + par;
          const double xp[3] = {pose[0 * kFkWave + ps], pose[1 * kFkWave + ps], pose[2 * kFkWave + ps]};
          const double rp[4] = {pose[3 * kFkWave + ps], pose[4 * kFkWave + ps], pose[5 * kFkWave + ps], pose[6 * kFkWave + ps]};
          double dd[3], t[4];
          dyn_rot(rp, bpos, dd);
          x[0] = xp[0] + dd[0]; x[1] = xp[1] + dd[1]; x[2] = xp[2] + dd[2];
          dyn_qmul(rp, bquat, t);
          if (hinge) {
            const double hh = 0.5 * th;
            const double sn = sin(hh), cs = cos(hh);
            const double jq[4] = {cs, sn * axis[0], sn * axis[1], sn * axis[2]};
            dyn_qmul(t, jq, r);
          } else {
            r[0] = t[0]; r[1] = t[1]; r[2] = t[2]; r[3] = t[3];
          }
        }
        pose[0 * kFkWave + lane] = x[0]; pose[1 * kFkWave + lane] = x[1]; pose[2 * kFkWave + lane] = x[2];
        pose[3 * kFkWave + lane] = r[0]; pose[4 * kFkWave + lane] = r[1]; pose[5 * kFkWave + lane] = r[2]; pose[6 * kFkWave + lane] = r[3];
      }
      wave_lds_sync();
    }

    // ---- 2: points and moments, LANE = POINT
    for (int gi = 0; gi < groups; ++gi) {
      const int64_t kf = k0 + gi;
      if (kf >= T) break;   // (wave-uniform)
      const int64_t go = r0 + kf;
      if (point) {
        const int sl = gi * jp + pb;
        const double px = pose[0 * kFkWave + sl] - ox, py = pose[1 * kFkWave + sl] - oy, pz = pose[2 * kFkWave + sl];
        double *out = a.points + (go * P + lane) * 3;
        out[0] = px; out[1] = py; out[2] = pz;
        pxy[lane] = px; pxy[kFkWave + lane] = py;
      }
      wave_lds_sync();
      if (lane < 3) {   // m.x, m.y, q: sums over the points in ascending order, from 0
        double s = 0.0;
        for (int p = 0; p < P; ++p) {
          const double w = wts[p], vx = pxy[p], vy = pxy[kFkWave + p];
          const double term = lane == 0 ? w * vx : (lane == 1 ? w * vy : w * (vx * vx + vy * vy));
          s = s + term;
        }
        a.moments[go * kTrMoments + lane] = s;
      }
      wave_lds_sync();   // (the next frame's points overwrite these)
    }
  }
}

// ------------------------------------------------------------------ b: windowed moments
// grid (n_seq, wavefronts per clip); lane = row
__global__ void __launch_bounds__(kFkWave) motion_transitions_window_kernel(const TransitionsArgs a) {
#pragma clang fp contract(off)
  const int L = a.L;
  const int64_t r0 = dyn_clamp(a.seq_offsets[blockIdx.x], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[blockIdx.x + 1], r0, a.n_frames);
  const int64_t nwin = r1 - r0 - L + 1;   // rows that start a full window
  const double len = (double)L;
  for (int64_t i = (int64_t)blockIdx.y * kFkWave + threadIdx.x; i < nwin; i += (int64_t)gridDim.y * kFkWave) {
    double sx = 0.0, sy = 0.0, sq = 0.0;
    for (int k = 0; k < L; ++k) {
      const double *row = a.moments + (r0 + i + k) * kTrMoments;
      sx = sx + row[0]; sy = sy + row[1]; sq = sq + row[2];
    }
    const double mx = sx / len, my = sy / len, q = sq / len;
    double *out = a.moments + (r0 + i) * kTrMoments;
    out[3] = mx; out[4] = my; out[5] = q - (mx * mx + my * my);
  }
}

// ------------------------------------------------------------------ c: pairs
constexpr int kTrRowRegs = 3 * kTrMaxBodies / kFkWave;   // doubles of one row of points a lane moves: 3

// One row of `points`, by the whole wavefront, in two halves so that a step's arithmetic lies between them: row `g` of the clip at
// `base`, clamped into the clip's T rows, into registers; and from there into `dst` at `pitch` doubles per coordinate.
__device__ __forceinline__ void tr_fetch_row(double (&v)[kTrRowRegs], const double *points, int64_t base, int g, int T, int row_d, int lane) {
  const int gc = g < 0 ? 0 : (g > T - 1 ? T - 1 : g);
  const double *src = points + (base + gc) * row_d;
#pragma unroll
  for (int q = 0; q < kTrRowRegs; ++q) { const int c = lane + kFkWave * q; v[q] = c < row_d ? src[c] : 0.0; }
}
__device__ __forceinline__ void tr_commit_row(const double (&v)[kTrRowRegs], double *dst, int pitch, int row_d, int lane) {
#pragma unroll
  for (int q = 0; q < kTrRowRegs; ++q) { const int c = lane + kFkWave * q; if (c < row_d) dst[c * pitch] = v[q]; }
}
// The 64 rows g0 .. g0 + 63 into the ring, eight loads in flight per lane.
__device__ __forceinline__ void tr_fill_ring(double *ring, const double *points, int64_t base, int g0, int T, int row_d, int lane) {
  const int total = kFkWave * row_d;
  for (int at = 0; at < total; at += 8 * kFkWave) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = at + u * kFkWave + lane, r = idx / row_d, g = g0 + r;
      const int gc = g < 0 ? 0 : (g > T - 1 ? T - 1 : g);
      v[u] = idx < total ? points[(base + gc) * row_d + (idx - r * row_d)] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = at + u * kFkWave + lane, r = idx / row_d;
      if (idx < total) ring[(idx - r * row_d) * kTrPitch + ((g0 + r) & (kFkWave - 1))] = v[u];
    }
  }
}

// grid (wavefronts): each strides over the work items; dynamic LDS: transitions_pair_lds_bytes
template <int LMAX>
__global__ void __launch_bounds__(kFkWave) motion_transitions_pair_kernel(const TransitionsArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double tr_lds[];
  const int lane = threadIdx.x;
  const int P = a.P, L = a.L, s = a.stride, tile = a.tile, n_dst = a.n_dst, n_src = a.n_src, row_d = 3 * P;
  double *const ring = tr_lds;                       // [3 P][kTrPitch]
  double *const srow = ring + row_d * kTrPitch;      // [3 P]: the source row of the step
  double *const wts = srow + row_d;                  // [P]
  double *const bestc = wts + P;                     // [tile]
  int *const bestj = reinterpret_cast<int *>(bestc + tile);   // [tile]
  const double inf = __longlong_as_double(0x7ff0000000000000ll), len = (double)L;
  const int64_t E = a.n_sources, NT = a.n_targets;
  for (int p = lane; p < P; p += kFkWave) wts[p] = a.weights[p];
  wave_lds_sync();

  const int64_t n_items = ((E + tile - 1) / tile) * n_dst;
  for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int64_t chunk = item / n_dst;
    const int b = (int)(item - chunk * n_dst);   // (neighbouring wavefronts share their sources)
    const int64_t e0 = chunk * tile, e1 = e0 + tile < E ? e0 + tile : E;
    const int cb = col_clampi(a.dst_clips[b], a.n_seq - 1);
    const int64_t rb0 = dyn_clamp(a.seq_offsets[cb], 0, a.n_frames);
    const int TB = (int)(dyn_clamp(a.seq_offsets[cb + 1], rb0, a.n_frames) - rb0);
    const int nj = TB >= L ? TB - L + 1 : 0;   // the target frames of the clip
    const int64_t dcol = a.cost_out ? a.dst_offsets[b] : 0;
    for (int k = lane; k < (int)(e1 - e0); k += kFkWave) { bestc[k] = inf; bestj[k] = -1; }
    wave_lds_sync();

    // the source clip of e0 (src_offsets ascends from 0 to E: trusted, and a walk that leaves the table ends)
    int sa = 0;
    for (int lo = 0, hi = n_src - 1; lo <= hi;) { const int mid = (lo + hi) >> 1; if (a.src_offsets[mid] <= e0) { sa = mid; lo = mid + 1; } else hi = mid - 1; }
    for (int64_t e = e0; e < e1;) {
      while (sa < n_src - 1 && a.src_offsets[sa + 1] <= e) ++sa;
      const int64_t so0 = a.src_offsets[sa], so1 = a.src_offsets[sa + 1];
      if (e < so0 || e >= so1) break;
      const int64_t stop = so1 < e1 ? so1 : e1;
      const int ca = col_clampi(a.src_clips[sa], a.n_seq - 1);
      const int64_t ra0 = dyn_clamp(a.seq_offsets[ca], 0, a.n_frames);
      const int TA = (int)(dyn_clamp(a.seq_offsets[ca + 1], ra0, a.n_frames) - ra0);
      const int64_t nvalid = TA >= L ? (int64_t)(TA - L) / s + 1 : 0;   // the sources the clip has
      const int64_t u0 = e - so0, u1 = stop - so0 < nvalid ? stop - so0 : nvalid;
      if (u0 < u1 && nj > 0) {
        const int i_first = (int)(u0 * s), i_last = (int)((u1 - 1) * s);
        const bool same = ca == cb;
        const int64_t local0 = e - e0;   // the tile entry of source u0
        // diagonals d = j - i in passes of 64, ascending
        for (int64_t d0l = -(int64_t)i_last; d0l <= (int64_t)(nj - 1) - i_first; d0l += kFkWave) {
          const int d0 = (int)d0l, d = d0 + lane;
          const int ia = i_first > -(d0 + kFkWave - 1) ? i_first : -(d0 + kFkWave - 1);   // the windows in which some lane has a target frame
          const int ib = i_last < nj - 1 - d0 ? i_last : nj - 1 - d0;
          if (ia > ib) continue;
          // the ring holds the target rows f + d0 .. f + d0 + 63 of step f, srow the source row f; the rows of step f + 1 (one new
          // target row, the next source row) are fetched before the step's arithmetic and stored behind it
          double nt[kTrRowRegs], ns[kTrRowRegs];
          tr_fill_ring(ring, a.points, rb0, ia + d0, TB, row_d, lane);
          tr_fetch_row(ns, a.points, ra0, ia, TA, row_d, lane);
          tr_commit_row(ns, srow, 1, row_d, lane);
          wave_lds_sync();
          double rd[LMAX], rc[LMAX], rz[LMAX];
#pragma unroll
          for (int k = 0; k < LMAX; ++k) { rd[k] = 0.0; rc[k] = 0.0; rz[k] = 0.0; }
          for (int f = ia; f <= ib + L - 1; ++f) {
            tr_fetch_row(nt, a.points, rb0, f + d0 + kFkWave, TB, row_d, lane);
            tr_fetch_row(ns, a.points, ra0, f + 1, TA, row_d, lane);
            // the per-row gram of (f, f + d): sums over the points in ascending order, from 0
            const int slot = (f + d) & (kFkWave - 1);
            double gd = 0.0, gc = 0.0, gz = 0.0;
            for (int p = 0; p < P; ++p) {
              const double w = wts[p], xf = srow[3 * p], yf = srow[3 * p + 1], zf = srow[3 * p + 2];
              const double xg = ring[(3 * p) * kTrPitch + slot], yg = ring[(3 * p + 1) * kTrPitch + slot], zg = ring[(3 * p + 2) * kTrPitch + slot];
              const double dz = zf - zg;
              gd = gd + w * (xf * xg + yf * yg);
              gc = gc + w * (xf * yg - yf * xg);
              gz = gz + w * (dz * dz);
            }
#pragma unroll
            for (int k = 0; k < LMAX - 1; ++k) { rd[k] = rd[k + 1]; rc[k] = rc[k + 1]; rz[k] = rz[k + 1]; }
            rd[LMAX - 1] = gd; rc[LMAX - 1] = gc; rz[LMAX - 1] = gz;
            const int i = f - L + 1;   // the window that ends in row f
            if (i >= ia && (i - i_first) % s == 0) {   // (wave-uniform) a source
              double sd = 0.0, sc = 0.0, sz = 0.0;
#pragma unroll
              for (int k = 0; k < LMAX; ++k)
                if (k >= LMAX - L) { sd = sd + rd[k]; sc = sc + rc[k]; sz = sz + rz[k]; }   // (wave-uniform) the last L, oldest first
              const int j = i + d;
              const bool valid = j >= 0 && j < nj;
              const double *mi = a.moments + (ra0 + i) * kTrMoments, *mj = a.moments + (rb0 + (valid ? j : 0)) * kTrMoments;
              const double mix = mi[3], miy = mi[4], vi = mi[5], mjx = mj[3], mjy = mj[4], vj = mj[5];
              const double D = sd / len - (mix * mjx + miy * mjy);
              const double Cc = sc / len - (mix * mjy - miy * mjx);
              const double Z = sz / len;
              double cost = ((vi + vj) - 2.0 * sqrt(D * D + Cc * Cc)) + Z;
              if (cost < 0.0) cost = 0.0;   // (a NaN stays)
              const bool excluded = same && (d < 0 ? -d : d) < a.min_gap;
              const int64_t u = u0 + (i - i_first) / s;
              if (a.cost_out && valid && dcol + j >= 0 && dcol + j < NT) a.cost_out[(so0 + u) * NT + dcol + j] = excluded ? inf : cost;
              const bool cand = valid && !excluded && cost == cost;
              const bool any = __ballot(cand) != 0;
              const double cmin = wave_min(cand ? cost : inf);
              const double jmin = wave_min(cand && cost == cmin ? (double)j : 2147483647.0);
              if (lane == 0 && any) {
                const int k = (int)(local0 + (u - u0));
                if (bestj[k] < 0 || cmin < bestc[k]) { bestc[k] = cmin; bestj[k] = (int)jmin; }   // (ascending diagonals: the first of equals stays)
              }
            }
            wave_lds_sync();   // (the next step's target row overwrites the one lane 0 just read)
            tr_commit_row(nt, ring + ((f + d0 + kFkWave) & (kFkWave - 1)), kTrPitch, row_d, lane);
            tr_commit_row(ns, srow, 1, row_d, lane);
            wave_lds_sync();
          }
        }
      }
      e = stop;
    }
    wave_lds_sync();
    for (int k = lane; k < (int)(e1 - e0); k += kFkWave) {
      a.best_cost[(e0 + k) * n_dst + b] = bestc[k];
      a.best_frame[(e0 + k) * n_dst + b] = bestj[k];
    }
    wave_lds_sync();
  }
}

}  // namespace gmr
