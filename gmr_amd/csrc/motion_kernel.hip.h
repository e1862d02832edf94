// motion_kernel.hip.h -- the dataset epilogue: solved qpos in, the four arrays of a motion file out, for several models in one grid.
//
// Replaces the post-processing of scripts/smplx_to_robot_dataset.py:93-131 (what dataset.motions_from_qpos does with two FK
// launches and a dozen torch ops) for every clip of every group member:
//   root_rot       qpos[:, [4,5,6,3]]                      (float64 copy, wxyz -> xyzw)
//   dof_pos        qpos[:, 7:]                             (float64 copy)
//   local_body_pos fk_pos_kernel with a zero root and an identity root rotation (float32)
//   root_pos       qpos[:, :3], xy minus the clip's first-frame xy (root-origin offset), z lowered by the clip's minimum body
//                  height under the real root (the value fk_kernel<1> / gmr_fk_min_height finds) plus ground_offset
//
// Pass 1 (motion_epilogue_kernel): one wavefront per 64-frame tile of one member, found by a scan over the members' tile bases.
// The tile's qpos block (contiguous in memory) is staged in LDS with coalesced loads, one lane per element; root_rot, dof_pos and
// root_pos leave from there, one lane per output element (contiguous stores).  Each lane then runs its frame's two chains side by
// side: the identity-root chain, whose positions go into the tile image of local_body_pos, and the real-root chain, which feeds
// the per-clip z minimum only.  Both take the same hinge quaternion and the same local product lrot * jq; only the rotation of
// the local translation and the product with the parent differ.  The arithmetic is fk_kernel.hip.h's helpers in the same
// order, so local_body_pos equals gmr_fk and the minimum equals gmr_fk_min_height bit for bit.  The image leaves as in
// fk_pos_kernel<1>: linearly, 16 bytes per lane and store.
// LDS per wavefront: branch slots of both chains | max(tile image, staged qpos) | the lanes' float dof rows | first-frame xy.
// The staged qpos tile is dead once the dof rows are extracted, so the image reuses its space.
//
// Pass 2 (motion_finish_kernel, only when a member adjusts heights or wants min_z_out): z = (z - (double)low_s) + ground_offset
// over root_pos, and the decoded minima.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"
#include "member_launch.hip.h"

namespace gmr {

constexpr int kMotionHeight = 1, kMotionOrigin = 2, kMotionWantMin = 4;  // flags of an entry (the first two are GMR_MOTION_*)
constexpr int kMotionFinishThreads = 256;

// One member's arguments of a launch, read by the kernels through the constant address space.
struct MotionEntry {
  FkTree fk;
  const double *qpos;
  const int64_t *seq_offsets;  // device copy, [n_seq + 1]
  int *keys;                   // device [n_seq]: order-preserving int keys of the per-clip minimum
  double *root_pos, *root_rot, *dof_pos;
  float *local_body_pos, *min_z;
  double ground_offset;
  int64_t n_frames;
  int64_t tile_base;    // first pass-1 workgroup of this member
  int64_t finish_base;  // first pass-2 workgroup of this member
  int n_seq, flags;
};

// clip of frame f: the last s with seq_offsets[s] <= f (empty clips share their offset with the next one and are skipped)
__device__ __forceinline__ int motion_clip(const int64_t *offs, int n_seq, int64_t f) {
  int lo = 0, hi = n_seq;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// LDS words of one lane's share, and of the whole wavefront, for a member (host and device agree on this layout)
constexpr int kMotionBatch = 16;  // staging loads in flight per lane

// i / d for 0 <= i < 64 d through the float reciprocal: (i + 0.5) / d < 64 is at least 1 / (2 d) away from an integer, and the
// rounding error of the product is below 64 x 2^-23 < 1e-5 -- exact for any d the LDS limit admits (d is a row length, < 1000)
__device__ __forceinline__ int motion_div(int i, float inv_d) { return (int)(((float)i + 0.5f) * inv_d); }

__host__ __device__ inline int motion_qpitch(int nq) { return nq | 1; }      // doubles per staged qpos row (odd: conflict-free)
__host__ __device__ inline int motion_dpitch(int ndof) { return ndof | 1; }  // floats per lane's dof row
__host__ __device__ inline int64_t motion_lds_bytes(int nbody, int ndof, int nslots) {
  const int64_t slots = (int64_t)(nslots > 1 ? nslots : 1) * 14 * kFkWave * 4;
  const int64_t image = (int64_t)3 * nbody * kFkWave * 4, qstage = (int64_t)motion_qpitch(ndof + 7) * kFkWave * 8;
  return slots + (image > qstage ? image : qstage) + (int64_t)motion_dpitch(ndof) * kFkWave * 4 + 2 * kFkWave * 8;
}

__global__ void __launch_bounds__(kFkWave) motion_epilogue_kernel(const MotionEntry *__restrict__ entries, int n_entries) {
#pragma clang fp contract(off)  // fk_pos_kernel's and fk_kernel<1>'s arithmetic exactly
  extern __shared__ float fk_lds[];
  const int lane = threadIdx.x;
  const int ei = launch_member<MotionEntry, &MotionEntry::tile_base>(entries, n_entries, (int64_t)blockIdx.x);
  const MotionEntry *ep = entries + ei;
  FkTree t{};  // the fields the chain reads (fk_body, fk_const)
  t.body = motion_const(&ep->fk.body);
  t.save_slot = motion_const(&ep->fk.save_slot);
  t.nbody = motion_const(&ep->fk.nbody);
  t.ndof = motion_const(&ep->fk.ndof);
  t.nslots = motion_const(&ep->fk.nslots);
  const double *__restrict__ qpos = motion_const(&ep->qpos);
  const int64_t n_frames = motion_const(&ep->n_frames);
  const int flags = motion_const(&ep->flags);
  const int n_seq = motion_const(&ep->n_seq);
  const int64_t *offs = motion_const(&ep->seq_offsets);
  const int nbody = t.nbody, ndof = t.ndof, nq = ndof + 7, row = 3 * nbody;
  const int qp = motion_qpitch(nq), dp = motion_dpitch(ndof);
  const int64_t f0 = ((int64_t)blockIdx.x - motion_const(&ep->tile_base)) * kFkWave;
  const int nfb = (int)(n_frames - f0 < kFkWave ? n_frames - f0 : kFkWave);
  // dead lanes (last tile only) recompute the member's last frame, which is this tile's last row: as in fk_pos_kernel /
  // fk_kernel<1>, they take part in the wave-level decisions and the minimum but store nothing
  const int r = lane < nfb ? lane : nfb - 1;
  const int64_t fc = f0 + r;
  float *slots = fk_lds;
  float *img = slots + (size_t)(t.nslots > 1 ? t.nslots : 1) * 14 * kFkWave;
  double *qs = reinterpret_cast<double *>(img);  // staged qpos tile, [nfb][qp]; the image takes its place after the copies
  const int64_t image_words = (int64_t)row * kFkWave, qstage_words = (int64_t)qp * kFkWave * 2;
  float *dofs = img + (image_words > qstage_words ? image_words : qstage_words);
  double *first = reinterpret_cast<double *>(dofs + dp * kFkWave);  // [64][2] first-frame xy of each lane's clip
  // ---- stage the tile's qpos block: contiguous in memory, one element per lane and load, kMotionBatch loads in flight per lane
  // (a load-then-write loop waits out the memory latency once per element)
  {
    const double *src = qpos + f0 * nq;
    const int n = nfb * nq;
    const float inv_nq = 1.0f / (float)nq;
    for (int base = 0; base < n; base += kMotionBatch * kFkWave) {
      double v[kMotionBatch];
#pragma unroll
      for (int u = 0; u < kMotionBatch; ++u) {
        const int i = base + u * kFkWave + lane;
        v[u] = i < n ? src[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kMotionBatch; ++u) {
        const int i = base + u * kFkWave + lane;
        if (i < n) {
          const int fr = motion_div(i, inv_nq), k = i - fr * nq;
          qs[fr * qp + k] = v[u];
        }
      }
    }
  }
  // clip of this lane's frame: the tile's first clip by a wave-uniform search (scalar loads), then forward per lane
  int s = 0;
  {
    int hi = n_seq;
    while (hi - s > 1) {
      const int mid = (s + hi) >> 1;
      if (motion_const(offs + mid) <= f0) s = mid; else hi = mid;
    }
    while (s + 1 < n_seq && offs[s + 1] <= fc) ++s;
  }
  if (flags & kMotionOrigin) {  // the clip's first frame may lie in an earlier tile: read it from qpos (a broadcast within a clip)
    const int64_t a = offs[s];
    first[2 * lane] = qpos[a * nq];
    first[2 * lane + 1] = qpos[a * nq + 1];
  }
  __syncthreads();
  // ---- root_rot, dof_pos, root_pos: one output element per lane, contiguous stores
  {
    double *rr = motion_const(&ep->root_rot) + f0 * 4;
    for (int i = lane; i < nfb * 4; i += kFkWave) {
      const int fr = i >> 2, k = i & 3;
      rr[i] = qs[fr * qp + 3 + ((k + 1) & 3)];  // xyzw <- qpos[4, 5, 6, 3]
    }
    if (ndof > 0) {
      double *dd = motion_const(&ep->dof_pos) + f0 * ndof;
      const float inv_ndof = 1.0f / (float)ndof;
      for (int i = lane; i < nfb * ndof; i += kFkWave) {
        const int fr = motion_div(i, inv_ndof), k = i - fr * ndof;
        dd[i] = qs[fr * qp + 7 + k];
      }
    }
    double *rp = motion_const(&ep->root_pos) + f0 * 3;
    const bool origin = (flags & kMotionOrigin) != 0;
    for (int i = lane; i < nfb * 3; i += kFkWave) {
      const int fr = motion_div(i, 1.0f / 3.0f), k = i - fr * 3;
      const double v = qs[fr * qp + k];
      rp[i] = origin && k < 2 ? v - first[2 * fr + k] : v;  // z: raw here, adjusted in pass 2
    }
  }
  // ---- this lane's chain inputs out of the stage: float dof row, real root
  for (int k = 0; k < ndof; ++k) dofs[lane * dp + k] = (float)qs[r * qp + 7 + k];
  float cpR[3], crR[4];
#pragma unroll
  for (int i = 0; i < 3; i++) cpR[i] = (float)qs[r * qp + i];
#pragma unroll
  for (int i = 0; i < 4; i++) crR[i] = (float)qs[r * qp + 3 + ((i + 1) & 3)];
  __syncthreads();  // the stage is dead from here: the image overwrites it
  const bool want_min = (flags & (kMotionHeight | kMotionWantMin)) != 0;
  float cpI[3] = {0.f, 0.f, 0.f}, crI[4] = {0.f, 0.f, 0.f, 1.f};
  float zmin = cpR[2];
  auto save = [&](int sv) {
    float *sl = slots + (size_t)sv * 14 * kFkWave + lane;
#pragma unroll
    for (int i = 0; i < 3; i++) sl[i * kFkWave] = cpI[i];
#pragma unroll
    for (int i = 0; i < 4; i++) sl[(3 + i) * kFkWave] = crI[i];
    if (want_min) {
#pragma unroll
      for (int i = 0; i < 3; i++) sl[(7 + i) * kFkWave] = cpR[i];
#pragma unroll
      for (int i = 0; i < 4; i++) sl[(10 + i) * kFkWave] = crR[i];
    }
  };
  if (fk_const(t.save_slot, 0) >= 0) save(fk_const(t.save_slot, 0));
#pragma unroll
  for (int i = 0; i < 3; i++) img[lane * row + i] = cpI[i];
  FkBody nxt = fk_body(t, nbody > 1 ? 1 : 0);
  for (int j = 1; j < nbody; ++j) {
    const FkBody rec = nxt;
    nxt = fk_body(t, j + 1 < nbody ? j + 1 : j);  // one body ahead
    float ppI[3], prI[4], ppR[3], prR[4];
    const int src = rec.src_slot;
    if (src < 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) { ppI[i] = cpI[i]; ppR[i] = cpR[i]; }
#pragma unroll
      for (int i = 0; i < 4; i++) { prI[i] = crI[i]; prR[i] = crR[i]; }
    } else {
      const float *sl = slots + (size_t)src * 14 * kFkWave + lane;
#pragma unroll
      for (int i = 0; i < 3; i++) ppI[i] = sl[i * kFkWave];
#pragma unroll
      for (int i = 0; i < 4; i++) prI[i] = sl[(3 + i) * kFkWave];
      if (want_min) {
#pragma unroll
        for (int i = 0; i < 3; i++) ppR[i] = sl[(7 + i) * kFkWave];
#pragma unroll
        for (int i = 0; i < 4; i++) prR[i] = sl[(10 + i) * kFkWave];
      } else {
#pragma unroll
        for (int i = 0; i < 3; i++) ppR[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; i++) prR[i] = 0.f;
      }
    }
    float jq[4] = {0.f, 0.f, 0.f, 1.f};
    if (rec.dofidx >= 0) fk_hinge_quat(rec.axis, dofs[lane * dp + rec.dofidx], jq);
    const float lt[3] = {rec.lpos[0], rec.lpos[1], rec.lpos[2]};
    const float lr[4] = {rec.lrot[0], rec.lrot[1], rec.lrot[2], rec.lrot[3]};
    float tmp[4], wt[3];
    fk_quat_mul(lr, jq, tmp);  // shared by both chains
    fk_quat_rotate(prI, lt, wt);
#pragma unroll
    for (int i = 0; i < 3; i++) cpI[i] = ppI[i] + wt[i];
    fk_quat_mul(prI, tmp, crI);
    if (want_min) {
      fk_quat_rotate(prR, lt, wt);
#pragma unroll
      for (int i = 0; i < 3; i++) cpR[i] = ppR[i] + wt[i];
      fk_quat_mul(prR, tmp, crR);
      zmin = fk_min_nan(zmin, cpR[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) img[lane * row + 3 * j + i] = cpI[i];
    if (rec.save_slot >= 0) save(rec.save_slot);
  }
  __syncthreads();
  {  // the tile image, linearly: full cache lines, 16 bytes per lane and store where the destination allows it
    const int nwords = nfb * row;
    float *dst = motion_const(&ep->local_body_pos) + f0 * row;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
      const int n4 = nwords >> 2;
      for (int i = lane; i < n4; i += kFkWave)
        *reinterpret_cast<float4 *>(dst + 4 * i) = *reinterpret_cast<const float4 *>(img + 4 * i);
      done = 4 * n4;
    }
    for (int i = done + lane; i < nwords; i += kFkWave) dst[i] = img[i];
  }
  if (want_min) {  // fk_kernel<1>'s reduction: one atomic per wavefront inside one clip, one per lane across a boundary
    int* keys = motion_const(&ep->keys);
    int k = fk_min_key(zmin);
    const int s0 = __builtin_amdgcn_readfirstlane(s);
    if (__all(s == s0)) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) k = min(k, __shfl_xor(k, off));
      if (lane == 0) atomicMin(keys + s0, k);
    } else {
      atomicMin(keys + s, k);
    }
  }
}

__device__ __forceinline__ float motion_decode(int k) { return fk_key_min(k); }

// Per member: n_frames height items (members that adjust heights), then n_seq decode items (members that want min_z).
__global__ void __launch_bounds__(kMotionFinishThreads) motion_finish_kernel(const MotionEntry *__restrict__ entries, int n_entries) {
#pragma clang fp contract(off)
  const int ei = launch_member<MotionEntry, &MotionEntry::finish_base>(entries, n_entries, (int64_t)blockIdx.x);
  const MotionEntry *ep = entries + ei;
  const int flags = motion_const(&ep->flags);
  const int n_seq = motion_const(&ep->n_seq);
  const int64_t nf = (flags & kMotionHeight) ? motion_const(&ep->n_frames) : 0;
  const int64_t nd = (flags & kMotionWantMin) ? n_seq : 0;
  const int64_t i = ((int64_t)blockIdx.x - motion_const(&ep->finish_base)) * kMotionFinishThreads + threadIdx.x;
  const int *keys = motion_const(&ep->keys);
  if (i < nf) {
    const int s = motion_clip(motion_const(&ep->seq_offsets), n_seq, i);
    double *z = motion_const(&ep->root_pos) + i * 3 + 2;
    *z = (*z - (double)motion_decode(keys[s])) + motion_const(&ep->ground_offset);
  } else if (i - nf < nd) {
    motion_const(&ep->min_z)[i - nf] = motion_decode(keys[i - nf]);
  }
}

}  // namespace gmr
