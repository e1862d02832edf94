// contact_kernel.hip.h -- foot-contact labels and slide statistics of a tracking export, one launch
// (gmr_motion_contacts; the definition is the contract above gmr_contact_input in include/gmr_amd.h).
//
// What a consumer of the export does on the host in a Python loop over frames: near the ground and slow switches a body's label
// on, far or fast switches it off, anything in between keeps the previous label -- a state machine along time.
//
// One wavefront per clip, walking the clip in tiles of 64 frames, lane = frame; inside a tile a loop over the C contact columns.
// Per tile and column two ballots, on = valid && enter and off = valid && !stay, hold the frames that decide the label (enter
// implies stay: the thresholds are validated, so no frame sets both).  A lane's label is the kind of the highest set bit of
// (on | off) at or below its own lane, and the carry when there is none; the label of the frame before it is the same question
// asked strictly below the lane.  So the whole state machine of a tile is two ballots and a handful of 64-bit bit operations,
// and the only thing that crosses a tile edge is the carry.
//
// Lane c owns column c's state: body id and height offset, the carry (label, previous x and y), the counts, the sum and the
// maxima.  The column loop reads them with a uniform-index v_readlane and updates them under `lane == c` after the tile: no
// dynamically indexed register array, no scratch, no LDS.  The pair (k-1, k) is charged to frame k, so lane 0 of a tile takes
// its predecessor from the carry and every other lane from its neighbour.  Sums are reduced over the tile in the fixed order of
// the DPP tree and added tile by tile: a report is bit-reproducible.
//
// GMR_CONTACT_GROUND_CLIP_MIN is a first pass of the same wavefront over the clip's heights: a running minimum per lane with
// the NaNs counted apart (torch.min's rule: any NaN makes the minimum NaN), reduced once at the end.
//
// Weakness, not engineered away: a lane loads 12 bytes of one body at a stride of nbody * 12 bytes between lanes, six scalar
// loads per column and tile, and a launch of a few long clips fills only a few SIMDs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_kernel.hip.h"  // rdlane, wave_min / wave_max / wave_sum

namespace gmr {

constexpr int kContactMaxCols = kFkWave;  // one lane per contact column

// The kernel's argument (the kernarg segment).
struct ContactArgs {
  const float *pos, *vel;        // [n_rows][nbody][3]
  const int64_t *out_offsets;    // [n_seq + 1]
  const int32_t *body_ids;       // [n_contact]
  const double *height_offset;   // [n_contact] or NULL
  int64_t n_rows;
  int nbody, n_contact, clip_min;
  double ground_z, height_on, height_off, speed_on2, speed_off2;
  uint8_t *contact;              // [n_rows][n_contact]
  int32_t *frames, *touchdowns;  // [n_seq][n_contact]
  double *slide_sum, *slide_step_max, *depth_max;
  int32_t *airborne;             // [n_seq]
  double *base;                  // [n_seq]
};

__device__ __forceinline__ int64_t contact_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kFkWave) motion_contacts_kernel(const ContactArgs a) {
#pragma clang fp contract(off)  // the contract's arithmetic exactly
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int C = a.n_contact, nbody = a.nbody;
  const int64_t r0 = contact_clamp(a.out_offsets[s], 0, a.n_rows);
  const int64_t r1 = contact_clamp(a.out_offsets[s + 1], r0, a.n_rows);
  const int64_t Ms = r1 - r0;
  // column state, lane c = column c
  const int my_body = lane < C ? a.body_ids[lane] : 0;
  const double my_hoff = (lane < C && a.height_offset) ? a.height_offset[lane] : 0.0;
  int my_label = 0, my_frames = 0, my_touch = 0;
  float my_px = 0.0f, my_py = 0.0f;
  double my_sum = 0.0, my_d2max = 0.0, my_depth = 0.0;
  int airborne = 0;

  double base = a.ground_z;
  if (a.clip_min) {
    double mn = __longlong_as_double(0x7ff0000000000000ll);  // +inf
    bool nan_seen = false;
    for (int64_t k0 = 0; k0 < Ms; k0 += kFkWave) {
      const bool valid = k0 + lane < Ms;
      const int64_t g = r0 + k0 + lane;
      for (int c = 0; c < C; ++c) {
        const int j = __builtin_amdgcn_readlane(my_body, c);
        const double hoff = rdlane(my_hoff, c);
        if (valid) {
          const double hc = (double)a.pos[(g * nbody + j) * 3 + 2] - hoff;
          nan_seen = nan_seen || hc != hc;
          mn = hc < mn ? hc : mn;
        }
      }
    }
    const double m = wave_min(mn);  // (no lane holds a NaN: those were counted apart)
    base = (Ms == 0 || __ballot(nan_seen) != 0) ? __longlong_as_double(0x7ff8000000000000ll) : m;
  }

  for (int64_t k0 = 0; k0 < Ms; k0 += kFkWave) {
    const bool valid = k0 + lane < Ms;
    const int64_t g = r0 + k0 + lane;
    const u64 at_or_below = ~0ull >> (63 - lane), below = lane ? ~0ull >> (64 - lane) : 0ull;
    bool any = false;
    for (int c = 0; c < C; ++c) {
      const int j = __builtin_amdgcn_readlane(my_body, c);
      const double hoff = rdlane(my_hoff, c);
      float x = 0.0f, y = 0.0f, z = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f;
      if (valid) {
        const float *p = a.pos + (g * nbody + j) * 3, *v = a.vel + (g * nbody + j) * 3;
        x = p[0]; y = p[1]; z = p[2];
        vx = v[0]; vy = v[1]; vz = v[2];
      }
      const double hc = (double)z - hoff;
      const double h = hc - base;
      const double dvx = (double)vx, dvy = (double)vy, dvz = (double)vz;
      const double s2 = (dvx * dvx + dvy * dvy) + dvz * dvz;
      const bool enter = h <= a.height_on && s2 <= a.speed_on2;
      const bool stay = h <= a.height_off && s2 <= a.speed_off2;
      const u64 on = __ballot(valid && enter), off = __ballot(valid && !stay);
      const u64 dec = on | off;
      const int carry = __builtin_amdgcn_readlane(my_label, c);
      // the last decisive frame at or below this lane, and strictly below it
      const u64 d0 = dec & at_or_below, d1 = dec & below;
      const int label = d0 ? (int)((on >> (63 - __builtin_clzll(d0))) & 1ull) : carry;
      const int prev = d1 ? (int)((on >> (63 - __builtin_clzll(d1))) & 1ull) : carry;
      if (valid && a.contact) a.contact[g * C + c] = (uint8_t)label;
      any = any || (valid && label);
      const int n_frames = __popcll(__ballot(valid && label));
      const int n_touch = __popcll(__ballot(valid && label && !prev));
      // the pair (k-1, k), charged to frame k: the neighbour's x and y, lane 0 from the carry
      float xp = __shfl_up(x, 1), yp = __shfl_up(y, 1);
      const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_px), c));
      const float cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_py), c));
      if (lane == 0) { xp = cx; yp = cy; }
      const bool pair = valid && label && prev;  // (frame 0 of a clip: prev is the initial carry, 0)
      const double dx = (double)x - (double)xp, dy = (double)y - (double)yp;
      const double d2 = dx * dx + dy * dy;
      const double t_sum = wave_sum(pair ? sqrt(d2) : 0.0);
      const double t_d2 = wave_max(pair ? d2 : 0.0);      // (fmax: a NaN is not a maximum)
      const double t_dep = wave_max(valid ? base - hc : 0.0);
      const int new_carry = dec ? (int)((on >> (63 - __builtin_clzll(dec))) & 1ull) : carry;
      const float lx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
      const float ly = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), 63));
      if (lane == c) {
        my_label = new_carry;
        my_px = lx; my_py = ly;  // (read by the next tile only, which exists only behind a full one)
        my_frames += n_frames;
        my_touch += n_touch;
        my_sum = my_sum + t_sum;
        my_d2max = t_d2 > my_d2max ? t_d2 : my_d2max;
        my_depth = t_dep > my_depth ? t_dep : my_depth;
      }
    }
    airborne += __popcll(__ballot(valid && !any));
  }

  if (lane < C) {
    const int64_t o = s * C + lane;
    if (a.frames) a.frames[o] = my_frames;
    if (a.touchdowns) a.touchdowns[o] = my_touch;
    if (a.slide_sum) a.slide_sum[o] = my_sum;
    if (a.slide_step_max) a.slide_step_max[o] = sqrt(my_d2max);
    if (a.depth_max) a.depth_max[o] = my_depth;
  }
  if (lane == 0) {
    if (a.airborne) a.airborne[s] = airborne;
    if (a.base) a.base[s] = base;
  }
}

}  // namespace gmr
