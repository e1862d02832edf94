// target_blocks.h -- who prepares what when the IK kernel prepares the targets of several frames in one pass (ik_kernel.hip.h,
// "Target blocks" in DESIGN 4.2): the lane -> (frame, slot) mapping of a block and the image of the LDS ring a frame reads.
//
// Plain C++17, host and device, no HIP include: the kernel and a stand-alone host test share these few functions.
//   - a block starts at every frame kf with (kf - kf0) a multiple of kTargetBlockFrames, kf0 = first frame of the wavefront's run
//     (a slice's first frame in a sliced launch, else 0), and covers frames kf .. min(kf + 3, kend - 1);
//   - lane 16 j + s prepares frame kf + j, slot s; lanes with s >= nslot or a frame at or behind kend do nothing (no load, no store);
//   - frame kf reads image (kf - kf0) & 3 of the ring, which is the j of the lanes that prepared it.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GMR_TB_HD __host__ __device__
#else
#define GMR_TB_HD
#endif

namespace gmr {

constexpr int kTargetBlockFrames = 4;  // frames per block = images in the ring
constexpr int kTargetBlockLanes = 16;  // lanes per frame of a block: 64 / kTargetBlockFrames, so nslot <= 16

struct TargetBlockLane {
  int frame, slot, image;  // the frame (in the item) and slot this lane prepares, and the ring image it writes
  bool on;                 // false: the lane issues no load and no store
};

GMR_TB_HD inline bool target_block_starts(int kf0, int kf) { return ((kf - kf0) & (kTargetBlockFrames - 1)) == 0; }

GMR_TB_HD inline int target_block_image(int kf0, int kf) { return (kf - kf0) & (kTargetBlockFrames - 1); }

// kf: the block's first frame (target_block_starts(kf0, kf)); kend: one past the last frame of the run.
GMR_TB_HD inline TargetBlockLane target_block_lane(int lane, int nslot, int kf, int kend) {
  TargetBlockLane t;
  t.image = lane / kTargetBlockLanes;
  t.slot = lane % kTargetBlockLanes;
  t.frame = kf + t.image;
  t.on = t.slot < nslot && t.frame < kend;
  return t;
}

}  // namespace gmr
