// footlock_kernel.hip.h -- foot locking: remove the horizontal slide of planted feet from retargeted qpos, three launches
// (gmr_motion_footlock; the definition is the contract above gmr_footlock_input in include/gmr_amd.h).
//
// What a consumer of retargeted clips does on the host -- a loop over contact phases, a small leg IK per frame -- as a post-pass on
// qpos: per contact column the foot is pinned to the mean of its own xy over every planted run, the shift is blended out over W
// frames on both sides of a run, and a damped least-squares iteration over the column's own hinges (the leg below the first
// joint it shares with another column) moves the foot there.  Everything is float64 as written, without contraction.
//
//   a  footlock_pos_kernel    one wavefront per tile of 64 frames of one clip, rows staged through LDS (element-wise, coalesced;
//                             the same pass copies qpos to qpos_out), then lane = frame: the valid bit and the FK of every
//                             column's path -> pos_out; shift_out = (0, 0, valid ? 0 : NaN) carries the valid bit to stage b
//   b  footlock_runs_kernel   one wavefront per (clip, column), lane = frame, 64-frame tiles.  Sweep 1: the planted runs by ballot
//                             and bit scans with a carry across tiles (open run: first frame and the two partial sums); a run that
//                             ends and is long enough gets its anchor and its frames' shifts.  Sweep 2: the ramps -- the nearest
//                             run frame before (bit scan, carry) and after (bit scan, a look-ahead of at most W frames that is
//                             shared by the tiles it spans).  A frame to solve is marked by the SIGN of its shift's z (-0.0)
//   c  footlock_solve_kernel  one wavefront per (clip tile, column), lane = frame: the I fixed iterations.  The lane's path angles,
//                             start angles and Jacobian columns live in LDS as [entry][lane] (uniform entry index: no
//                             dynamically indexed register array, no bank conflict); the model's constants come through scalar
//                             loads (the column, and with it the path, is wave-uniform).  FK runs twice per iteration -- once
//                             for the foot, once for the Jacobian columns, which need the foot -- instead of parking every
//                             joint's axis and anchor.  Resets the mark to +0.0.
//
// Stage b reads shift_out elements that other lanes of the same wavefront wrote earlier in the kernel: a device-scope fence between
// the sweeps, and those loads are device-scope atomic loads (they bypass the non-coherent vector cache).
//
// Weaknesses, not engineered away: in stage c a lane reads its own row's path angles at a stride of nq * 8 bytes between lanes
// (about a dozen loads per lane and column) and writes the chain's back at the same stride; stage b is one wavefront per clip and
// column, so a launch of a few long clips fills only a few SIMDs, and it walks every clip three times.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"      // kFkWave, fk_const
#include "ik_kernel.hip.h"      // DevModel, wave_sum / wave_max
#include "motion_kernel.hip.h"  // motion_qpitch, motion_div

namespace gmr {

constexpr int kFootlockMaxCols = 8;    // contact columns per call
constexpr int kFootlockMaxChain = 16;  // hinges a column may move
constexpr int kFootlockMaxPath = 32;   // bodies between the root and a contact body, the body included
constexpr int kFootlockMaxIters = 32;

// The kernels' argument (the kernarg segment): the call, and per column the path from the root's child down to the contact body
// with the hinges that belong to the column's chain.
struct FootlockArgs {
  const DevModel *dm;            // the full body tree (gmr_evaluate's)
  const double *lo, *hi;         // [nq - 7] hinge limits in qpos order, -inf / +inf where unlimited
  const double *qpos;            // [n_frames][nq]
  const int64_t *seq_offsets;    // [n_seq + 1]
  const uint8_t *contact;        // [n_frames][C]
  int64_t n_frames;
  int n_seq, C, nq, blend, min_run, iters;
  double damping, step_cap;
  double *qpos_out, *pos, *shift;
  int32_t *runs, *locked;
  double *shift_max, *resid_max;
  int32_t *limit_frames;
  uint32_t chain_mask[kFootlockMaxCols];  // bit i: the hinge of path element i belongs to the chain
  uint8_t path_len[kFootlockMaxCols], n_chain[kFootlockMaxCols];
  uint8_t path[kFootlockMaxCols][kFootlockMaxPath];  // body indices, the root's child first
};

__device__ __forceinline__ int64_t fl_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool fl_marked(double z) { return __double_as_longlong(z) == (long long)0x8000000000000000ull; }  // -0.0
// a shift_out element another lane of this wavefront may have written earlier in the kernel
__device__ __forceinline__ double fl_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// wxyz quaternion product and rotation of a vector, the contract's operation order
__device__ __forceinline__ void fl_qmul(const double a[4], const double b[4], double o[4]) {
#pragma clang fp contract(off)
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
__device__ __forceinline__ void fl_rot(const double q[4], const double v[3], double o[3]) {
#pragma clang fp contract(off)
  const double tx = 2.0 * (q[2] * v[2] - q[3] * v[1]), ty = 2.0 * (q[3] * v[0] - q[1] * v[2]), tz = 2.0 * (q[1] * v[1] - q[2] * v[0]);
  o[0] = v[0] + q[0] * tx + (q[2] * tz - q[3] * ty);
  o[1] = v[1] + q[0] * ty + (q[3] * tx - q[1] * tz);
  o[2] = v[2] + q[0] * tz + (q[1] * ty - q[2] * tx);
}
// the root's pose out of the first seven entries of a row: the quaternion divided by its norm
__device__ __forceinline__ void fl_root(const double r[7], double xp[3], double xq[4]) {
#pragma clang fp contract(off)
  const double n = sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5] + r[6] * r[6]);
  xp[0] = r[0]; xp[1] = r[1]; xp[2] = r[2];
  xq[0] = r[3] / n; xq[1] = r[4] / n; xq[2] = r[5] / n; xq[3] = r[6] / n;
}

// Walk column c's path from the root pose (xp, xq) down to the contact body; on return xp is its origin.  theta(i, j): the angle of
// path element i (body j, a hinge); visit(i, axis, xp, xq): called behind every hinge with the body's world pose.
template <class Theta, class Visit>
__device__ __forceinline__ void fl_walk(const FootlockArgs &a, int c, double xp[3], double xq[4], Theta theta, Visit visit) {
#pragma clang fp contract(off)
  const DevModel *dm = a.dm;
  const int np = a.path_len[c];
  for (int i = 0; i < np; ++i) {
    const int j = a.path[c][i];
    const double bp[3] = {fk_const(dm->bpos, 3 * j), fk_const(dm->bpos, 3 * j + 1), fk_const(dm->bpos, 3 * j + 2)};
    const double bq[4] = {fk_const(dm->bquat, 4 * j), fk_const(dm->bquat, 4 * j + 1), fk_const(dm->bquat, 4 * j + 2), fk_const(dm->bquat, 4 * j + 3)};
    double w[3], t[4];
    fl_rot(xq, bp, w);
    xp[0] = xp[0] + w[0]; xp[1] = xp[1] + w[1]; xp[2] = xp[2] + w[2];
    fl_qmul(xq, bq, t);
    if (fk_const(dm->jtype, j) == GMR_JNT_HINGE) {
      const double ax[3] = {fk_const(dm->axis, 3 * j), fk_const(dm->axis, 3 * j + 1), fk_const(dm->axis, 3 * j + 2)};
      const double h = 0.5 * theta(i, j);
      const double sn = sin(h), cs = cos(h);
      const double jq[4] = {cs, sn * ax[0], sn * ax[1], sn * ax[2]};
      fl_qmul(t, jq, xq);
      visit(i, ax, xp, xq);
    } else {
      xq[0] = t[0]; xq[1] = t[1]; xq[2] = t[2]; xq[3] = t[3];
    }
  }
}

// ------------------------------------------------------------------ a: copy, valid bit, foot positions
// grid (n_seq, tiles per clip in flight); dynamic LDS: [64][nq | 1] doubles
__global__ void __launch_bounds__(kFkWave) footlock_pos_kernel(const FootlockArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double fl_lds[];
  const int lane = threadIdx.x;
  const int C = a.C, nq = a.nq, qp = motion_qpitch(nq);
  const int64_t r0 = fl_clamp(a.seq_offsets[blockIdx.x], 0, a.n_frames);
  const int64_t r1 = fl_clamp(a.seq_offsets[blockIdx.x + 1], r0, a.n_frames);
  const int64_t Ms = r1 - r0;
  const float inv_nq = 1.0f / (float)nq;
  for (int64_t k0 = (int64_t)blockIdx.y * kFkWave; k0 < Ms; k0 += (int64_t)gridDim.y * kFkWave) {
    const int nfb = (int)(Ms - k0 < kFkWave ? Ms - k0 : kFkWave);
    const int64_t base = (r0 + k0) * nq;
    __syncthreads();  // (the previous tile's rows are no longer read)
    for (int i = lane; i < nfb * nq; i += kFkWave) {
      const double v = a.qpos[base + i];
      a.qpos_out[base + i] = v;
      const int fr = motion_div(i, inv_nq);
      fl_lds[fr * qp + i - fr * nq] = v;
    }
    __syncthreads();
    if (lane >= nfb) continue;
    const double *my = fl_lds + lane * qp;
    bool valid = true;
    for (int i = 0; i < nq; ++i) valid = valid && __builtin_isfinite(my[i]);
    const int64_t g = r0 + k0 + lane;
    const double r[7] = {my[0], my[1], my[2], my[3], my[4], my[5], my[6]};
    for (int c = 0; c < C; ++c) {
      double xp[3], xq[4];
      fl_root(r, xp, xq);
      fl_walk(a, c, xp, xq, [&](int, int j) { return my[fk_const(a.dm->qadr, j)]; }, [](int, const double *, const double *, const double *) {});
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      double *p = a.pos + (g * C + c) * 3, *d = a.shift + (g * C + c) * 3;
      p[0] = valid ? xp[0] : nan; p[1] = valid ? xp[1] : nan; p[2] = valid ? xp[2] : nan;
      d[0] = 0.0; d[1] = 0.0; d[2] = valid ? 0.0 : nan;
    }
  }
}

// ------------------------------------------------------------------ b: runs, anchors, shifts and ramps
// grid (n_seq, C)
__global__ void __launch_bounds__(kFkWave) footlock_runs_kernel(const FootlockArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int c = blockIdx.y, C = a.C;
  const int64_t r0 = fl_clamp(a.seq_offsets[s], 0, a.n_frames);
  const int64_t r1 = fl_clamp(a.seq_offsets[s + 1], r0, a.n_frames);
  const int64_t Ms = r1 - r0, W = a.blend, min_run = a.min_run;
  const double *pos = a.pos + (r0 * C + c) * 3;  // element k: pos[3 C k]
  double *sh = a.shift + (r0 * C + c) * 3;
  const uint8_t *lab = a.contact + r0 * C + c;
  const int64_t st = 3 * (int64_t)C;
  int n_runs = 0, n_locked = 0;
  double d2max = 0.0;
  const double mark = __longlong_as_double((long long)0x8000000000000000ull);

  // ---- sweep 1: runs of L = contact && valid; anchors; the shifts inside the runs
  bool open = false;
  int64_t start = 0;
  double sx = 0.0, sy = 0.0;
  auto close = [&](int64_t first, int64_t last) {
#pragma clang fp contract(off)
    const int64_t n = last - first + 1;
    if (n < min_run) return;
    n_runs += 1;
    n_locked += (int)n;
    const double ax = sx / (double)n, ay = sy / (double)n;
    for (int64_t t0 = first & ~(int64_t)(kFkWave - 1); t0 <= last; t0 += kFkWave) {
      const int64_t k = t0 + lane;
      if (k >= first && k <= last) {
        const double dx = ax - pos[k * st], dy = ay - pos[k * st + 1];
        sh[k * st] = dx; sh[k * st + 1] = dy; sh[k * st + 2] = mark;
        const double d2 = dx * dx + dy * dy;
        d2max = d2 > d2max ? d2 : d2max;
      }
    }
  };
  for (int64_t k0 = 0; k0 < Ms; k0 += kFkWave) {
    const int64_t k = k0 + lane;
    bool L = false;
    double px = 0.0, py = 0.0;
    if (k < Ms) {
      L = sh[k * st + 2] == 0.0 && lab[k * C] != 0;  // (stage a's valid bit: NaN compares false)
      if (L) { px = pos[k * st]; py = pos[k * st + 1]; }
    }
    const u64 m = __ballot(L);
    int b = 0;
    while (b < kFkWave) {
      if (!open) {
        const u64 rest = (m >> b) << b;
        if (!rest) break;
        b = __builtin_ctzll(rest);
        open = true; start = k0 + b; sx = 0.0; sy = 0.0;
      }
      const u64 zeros = ((~m) >> b) << b;
      const int eb = zeros ? __builtin_ctzll(zeros) : kFkWave;  // the run holds the tile's frames [b, eb)
      const bool in = lane >= b && lane < eb;
      sx = sx + wave_sum(in ? px : 0.0);  // the balanced tree over the tile's 64 positions, tiles added in order
      sy = sy + wave_sum(in ? py : 0.0);
      if (eb == kFkWave) break;           // goes on in the next tile
      close(start, k0 + eb - 1);
      open = false;
      b = eb;
    }
  }
  if (open) close(start, Ms - 1);
  __threadfence();  // sweep 1's stores before sweep 2's loads of them

  // ---- sweep 2: the ramps on both sides of every run
  // Both sweeps mark with the same -0.0, and sweep 2 must only ever see sweep 1's marks (the runs).  It does, by order: tile T's
  // `inrun` ballot is taken before any ramp mark of tile T is written; a look-ahead scans tiles > T only, and those get their ramp
  // marks when they are processed, after every look-ahead that can reach them; tiles < T are read again only as shift[e].xy of a
  // run frame, which sweep 2 never writes.  Sweep 1 likewise reads a tile's valid bits before any close() has written into it.
  int64_t e_carry = -1, nf = -1, ahead = 0;
  for (int64_t k0 = 0; k0 < Ms; k0 += kFkWave) {
    const int64_t k = k0 + lane;
    const bool live = k < Ms;
    const double z = live ? fl_load(sh + k * st + 2) : 0.0;
    const u64 inrun = __ballot(live && fl_marked(z));
    const u64 below = lane ? ~0ull >> (kFkWave - lane) : 0ull;
    const u64 d1 = inrun & below, d2 = lane < kFkWave - 1 ? (inrun >> (lane + 1)) << (lane + 1) : 0ull;
    // the first run frame behind this tile, looked for at most W frames ahead; tiles share what the scan found
    if (nf >= 0 && nf < k0 + kFkWave) nf = -1;
    if (ahead < k0 + kFkWave) ahead = k0 + kFkWave;
    while (nf < 0 && ahead < Ms && ahead <= k0 + kFkWave - 1 + W) {
      const int64_t kk = ahead + lane;
      const u64 mm = __ballot(kk < Ms && fl_marked(fl_load(sh + (kk < Ms ? kk : Ms - 1) * st + 2)));
      if (mm) nf = ahead + __builtin_ctzll(mm);
      ahead += kFkWave;
    }
    const int64_t e = d1 ? k0 + 63 - __builtin_clzll(d1) : e_carry;
    const int64_t f = d2 ? k0 + __builtin_ctzll(d2) : nf;
    if (live && z == 0.0 && !fl_marked(z)) {  // valid and outside every run
      double wm = 0.0, wp = 0.0;
      if (e >= 0 && k - e <= W) { const double t = 1.0 - (double)(k - e) / (double)(W + 1); wm = t * t * (3.0 - 2.0 * t); }
      if (f >= 0 && f - k <= W) { const double t = 1.0 - (double)(f - k) / (double)(W + 1); wp = t * t * (3.0 - 2.0 * t); }
      if (wm > 0.0 || wp > 0.0) {
        double tx = 0.0, ty = 0.0, ux = 0.0, uy = 0.0;  // a side without weight adds zero
        if (wm > 0.0) { tx = wm * fl_load(sh + e * st); ty = wm * fl_load(sh + e * st + 1); }
        if (wp > 0.0) { ux = wp * fl_load(sh + f * st); uy = wp * fl_load(sh + f * st + 1); }
        const double den = wm + wp > 1.0 ? wm + wp : 1.0;
        const double dx = (tx + ux) / den, dy = (ty + uy) / den;
        sh[k * st] = dx; sh[k * st + 1] = dy; sh[k * st + 2] = mark;
        const double q2 = dx * dx + dy * dy;
        d2max = q2 > d2max ? q2 : d2max;
      }
    } else if (live && z != z) {
      sh[k * st + 2] = 0.0;  // an invalid frame: no shift
    }
    if (inrun) e_carry = k0 + 63 - __builtin_clzll(inrun);
  }
  const double dm = wave_max(d2max);
  if (lane == 0) {
    const int64_t o = s * C + c;
    if (a.runs) a.runs[o] = n_runs;
    if (a.locked) a.locked[o] = n_locked;
    if (a.shift_max) a.shift_max[o] = sqrt(dm);
    if (a.resid_max) a.resid_max[o] = 0.0;  // stage c's atomics start here
    if (a.limit_frames) a.limit_frames[o] = 0;
  }
}

// ------------------------------------------------------------------ c: the fixed iterations
// Doubles of LDS per lane for a column with np path elements and nc chain hinges: angles [np] | start angles [nc] | J [nc][3]
__host__ __device__ inline int footlock_solve_doubles(int np, int nc) { return np + 4 * nc; }

// grid (n_seq, tiles per clip in flight, C); dynamic LDS: footlock_solve_doubles of the largest column x 64 doubles
__global__ void __launch_bounds__(kFkWave) footlock_solve_kernel(const FootlockArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double fl_lds[];
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int c = blockIdx.z, C = a.C, nq = a.nq;
  const int np = a.path_len[c], nc = a.n_chain[c];
  const uint32_t mask = a.chain_mask[c];
  const DevModel *dm = a.dm;
  double *ang = fl_lds + lane;                     // [np][64]
  double *ang0 = ang + np * kFkWave;               // [nc][64]
  double *jac = ang0 + nc * kFkWave;               // [nc][3][64]
  const int64_t r0 = fl_clamp(a.seq_offsets[s], 0, a.n_frames);
  const int64_t r1 = fl_clamp(a.seq_offsets[s + 1], r0, a.n_frames);
  const int64_t Ms = r1 - r0;
  double rmax = 0.0;
  int nlim = 0;
  for (int64_t k0 = (int64_t)blockIdx.y * kFkWave; k0 < Ms; k0 += (int64_t)gridDim.y * kFkWave) {
    const int64_t k = k0 + lane, g = r0 + k;
    double *d = a.shift + (g * C + c) * 3;
    if (!(k < Ms && fl_marked(d[2]))) continue;
    d[2] = 0.0;  // the mark has been read
    const double *row = a.qpos + g * nq;
    const double r[7] = {row[0], row[1], row[2], row[3], row[4], row[5], row[6]};
    double rp[3], rq[4];
    fl_root(r, rp, rq);
    for (int i = 0, ci = 0; i < np; ++i) {
      const int j = a.path[c][i];
      const double th = fk_const(dm->jtype, j) == GMR_JNT_HINGE ? row[fk_const(dm->qadr, j)] : 0.0;
      ang[i * kFkWave] = th;
      if ((mask >> i) & 1u) { ang0[ci * kFkWave] = th; ++ci; }
    }
    const double *p0 = a.pos + (g * C + c) * 3;
    const double tgt[3] = {p0[0] + d[0], p0[1] + d[1], p0[2]};
    auto theta = [&](int i, int) { return ang[i * kFkWave]; };
    for (int it = 0; it < a.iters; ++it) {
      double xp[3] = {rp[0], rp[1], rp[2]}, xq[4] = {rq[0], rq[1], rq[2], rq[3]};
      fl_walk(a, c, xp, xq, theta, [](int, const double *, const double *, const double *) {});
      const double p[3] = {xp[0], xp[1], xp[2]};
      const double e[3] = {tgt[0] - p[0], tgt[1] - p[1], tgt[2] - p[2]};
      double g00 = 0.0, g10 = 0.0, g11 = 0.0, g20 = 0.0, g21 = 0.0, g22 = 0.0;
      int ci = 0;
      xp[0] = rp[0]; xp[1] = rp[1]; xp[2] = rp[2];
      xq[0] = rq[0]; xq[1] = rq[1]; xq[2] = rq[2]; xq[3] = rq[3];
      fl_walk(a, c, xp, xq, theta, [&](int i, const double *ax, const double *o, const double *q) {
#pragma clang fp contract(off)
        if (!((mask >> i) & 1u)) return;
        double w[3];
        fl_rot(q, ax, w);
        const double l[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
        const double j0 = w[1] * l[2] - w[2] * l[1], j1 = w[2] * l[0] - w[0] * l[2], j2 = w[0] * l[1] - w[1] * l[0];
        double *jc = jac + 3 * ci * kFkWave;
        jc[0] = j0; jc[kFkWave] = j1; jc[2 * kFkWave] = j2;
        g00 = g00 + j0 * j0; g10 = g10 + j1 * j0; g11 = g11 + j1 * j1;
        g20 = g20 + j2 * j0; g21 = g21 + j2 * j1; g22 = g22 + j2 * j2;
        ++ci;
      });
      g00 = g00 + a.damping; g11 = g11 + a.damping; g22 = g22 + a.damping;
      const double l00 = sqrt(g00), l10 = g10 / l00, l20 = g20 / l00;
      const double l11 = sqrt(g11 - l10 * l10), l21 = (g21 - l20 * l10) / l11;
      const double l22 = sqrt(g22 - l20 * l20 - l21 * l21);
      const double z0 = e[0] / l00, z1 = (e[1] - l10 * z0) / l11, z2 = (e[2] - l20 * z0 - l21 * z1) / l22;
      const double y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = (z0 - l10 * y1 - l20 * y2) / l00;
      double mx = 0.0;
      for (int n = 0; n < nc; ++n) {
        const double *jc = jac + 3 * n * kFkWave;
        const double dq = jc[0] * y0 + jc[kFkWave] * y1 + jc[2 * kFkWave] * y2;
        mx = fabs(dq) > mx ? fabs(dq) : mx;
      }
      const double scale = mx > a.step_cap ? a.step_cap / mx : 1.0;
      for (int i = 0, n = 0; i < np; ++i) {
        if (!((mask >> i) & 1u)) continue;
        const int h = fk_const(dm->qadr, (int)a.path[c][i]) - 7;
        const double *jc = jac + 3 * n * kFkWave;
        const double dq = jc[0] * y0 + jc[kFkWave] * y1 + jc[2 * kFkWave] * y2;
        const double q0 = ang0[n * kFkWave];
        const double lo = fk_const(a.lo, h), hi = fk_const(a.hi, h);
        const double lw = lo < q0 ? lo : q0, hw = hi > q0 ? hi : q0;
        double q = ang[i * kFkWave] + scale * dq;
        q = q < lw ? lw : (q > hw ? hw : q);
        ang[i * kFkWave] = q;
        ++n;
      }
    }
    {
      double xp[3] = {rp[0], rp[1], rp[2]}, xq[4] = {rq[0], rq[1], rq[2], rq[3]};
      fl_walk(a, c, xp, xq, theta, [](int, const double *, const double *, const double *) {});
      const double ex = tgt[0] - xp[0], ey = tgt[1] - xp[1], ez = tgt[2] - xp[2];
      const double res = sqrt(ex * ex + ey * ey + ez * ez);
      rmax = res > rmax ? res : rmax;
    }
    bool on_limit = false;
    double *orow = a.qpos_out + g * nq;
    for (int i = 0, n = 0; i < np; ++i) {
      if (!((mask >> i) & 1u)) continue;
      const int h = fk_const(dm->qadr, (int)a.path[c][i]) - 7;
      const double q = ang[i * kFkWave], q0 = ang0[n * kFkWave];
      const double lo = fk_const(a.lo, h), hi = fk_const(a.hi, h);
      const double lw = lo < q0 ? lo : q0, hw = hi > q0 ? hi : q0;
      on_limit = on_limit || (__builtin_isfinite(lo) && q == lw) || (__builtin_isfinite(hi) && q == hw);
      orow[7 + h] = q;
      ++n;
    }
    nlim += on_limit ? 1 : 0;
  }
  // per-clip maxima and counts are order-free: one atomic per wavefront (non-negative doubles order as their bit patterns)
  const double wmax = wave_max(rmax);
  const int wlim = (int)wave_sum((double)nlim);  // (small integers: exact)
  if (lane == 0) {
    const int64_t o = s * C + c;
    if (a.resid_max && wmax > 0.0) atomicMax(reinterpret_cast<unsigned long long *>(a.resid_max + o), (unsigned long long)__double_as_longlong(wmax));
    if (a.limit_frames && wlim) atomicAdd(a.limit_frames + o, wlim);
  }
}

}  // namespace gmr
