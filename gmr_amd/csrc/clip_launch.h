// clip_launch.h -- the launch arithmetic of the clip-wise motion calls (foot locking, inverse dynamics, self-collision, mirror,
// compose, transition search, retiming): grids, environment overrides and the body tree's parent / depth bytes.
//
// Plain C++17, host only, no HIP include: api.hip and a stand-alone host test share these functions.  The constants (target
// wavefronts, tiles, limits) stay with their kernels; the callers pass them in.
//
// The grid rule.  A clip-wise kernel takes the grid (clips, wavefronts per clip); a wavefront strides over its clip's units -- frame
// slots of `groups` frames side by side, or tiles of rows -- so its set-up (depth, subtree end, its body's and capsules' constants,
// staged tables) is paid once for many frames.  The host aims at about `target` wavefronts in the whole launch (8 192: four rounds of
// a 256-CU device at two wavefronts per SIMD; 16 384 for the row kernels: 256 CUs x 32 slots, twice over), gives a clip at most one
// wavefront per unit of the MEAN clip -- the clips' lengths live on the device, a longer clip makes its wavefronts walk further --
// and never leaves gridDim.y's range: 2 048 clips x 3 000 frames run 4 wavefronts of 750 frames each.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace gmr {

constexpr int64_t kGridYMax = 65535;  // gridDim.y and gridDim.z

inline int64_t clip_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Wavefronts per clip: max(1, min(ceil(target / n_clips), mean_units, 65535)), n_clips >= 1.
inline unsigned clip_waves(int64_t target, int64_t n_clips, int64_t mean_units) {
  return (unsigned)std::max<int64_t>(1, std::min({clip_ceil_div(target, n_clips), mean_units, kGridYMax}));
}
// Units of the mean clip.  Frame slots at `groups` frames side by side (chain_geom), rounded over the whole call first ...
inline int64_t mean_clip_slots(int64_t n_frames, int groups, int64_t n_clips) { return clip_ceil_div(clip_ceil_div(n_frames, groups), n_clips); }
// ... and tiles of `tile` rows of the mean clip (kernel b of the transition search: tile = kFkWave; retiming's apply kernel: the
// mean clip's OUTPUT rows).
inline int64_t mean_clip_tiles(int64_t n_rows, int64_t n_clips, int tile) { return clip_ceil_div(clip_ceil_div(n_rows, n_clips), tile); }

// Foot locking's own rule, over the `tile`-frame tiles (kFkWave) of its kernels a and c: four times the mean clip's tiles in flight
// per clip, so that long clips stride and short ones launch few idle wavefronts; never more than the call has.  n_seq >= 1.
inline unsigned footlock_clip_waves(int64_t n_frames, int64_t n_seq, int tile) {
  const int64_t tiles = clip_ceil_div(n_frames, tile);
  return (unsigned)std::min({tiles, 4 * clip_ceil_div(tiles, n_seq), kGridYMax});
}

// Kernel c of the transition search: one wavefront per work item (a run of `tile` sources, a target clip), at most max_waves
// (kTrPairWaves); each strides over the items.
inline unsigned transitions_pair_waves(int64_t n_sources, int tile, int64_t n_dst, int64_t max_waves) {
  return (unsigned)std::max<int64_t>(1, std::min(clip_ceil_div(n_sources, tile) * n_dst, max_waves));
}

// An integer override from the environment, read on every call (the tests change it between calls): the variable's leading base-10
// number when it lies in [lo, hi], else `unset` -- as for a variable that is not set, is empty or holds no number.
inline long env_int(const char *name, long lo, long hi, long unset) {
  const char *e = getenv(name);
  if (!e) return unset;
  const long v = strtol(e, nullptr, 10);
  return v >= lo && v <= hi ? v : unset;
}

// Where the self-collision pair indices live: in LDS while the table fits (n_pairs <= lds_max), else re-read from L2.  The variable
// `name` (GMR_AMD_COLLISION_PAIRS = lds / global) can only force global: a value that starts with 'g'.
inline bool collision_pairs_in_lds(const char *name, int64_t n_pairs, int64_t lds_max) {
  const char *e = getenv(name);
  return n_pairs <= lds_max && !(e && e[0] == 'g');
}

// The body tree as the body-per-lane kernels read it from their argument: parent8[b] (0xff for the root) and depth8[b].  nbody <= 64
// (the callers refuse more), and a parent precedes its child: model creation checked that for every blob (check_tree, model_plan.h).
inline void tree_parent_depth(const int32_t *parent, int nbody, uint8_t *parent8, uint8_t *depth8) {
  for (int b = 0; b < nbody; ++b) {
    parent8[b] = parent[b] < 0 ? 0xff : (uint8_t)parent[b];
    depth8[b] = parent[b] < 0 ? 0 : (uint8_t)(depth8[parent[b]] + 1);
  }
}

// Depth-first order -- the parent of b is b - 1 or one of its ancestors -- which is more than model creation asks: the first body
// that does not follow its parent's subtree, or 0 where every body does.
inline int tree_first_not_depth_first(const int32_t *parent, int nbody) {
  for (int b = 1; b < nbody; ++b) {
    int j = b - 1;
    while (j >= 0 && j != parent[b]) j = parent[j];
    if (j < 0) return b;
  }
  return 0;
}

}  // namespace gmr
