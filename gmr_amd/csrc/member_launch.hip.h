// member_launch.hip.h -- what the member-wise kernels (motion, track, lowpass, report) share: one grid runs over the workgroups
// of all members of a call, every member's arguments are one entry of an array in device memory, and a workgroup finds its
// member by the entries' workgroup bases.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmr {

// *p through the constant address space: launch arguments that no kernel of the launch writes
template <class T>
__device__ __forceinline__ T motion_const(const T *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
#else
  return *p;
#endif
}

// member of workgroup `blk`: the last entry whose base is <= blk (entries in member order, bases non-decreasing)
template <class Entry, int64_t Entry::*BASE>
__device__ __forceinline__ int launch_member(const Entry *entries, int n_entries, int64_t blk) {
  int e = 0;
  while (e + 1 < n_entries) {
    if (blk < motion_const(&(entries[e + 1].*BASE))) break;
    ++e;
  }
  return e;
}

}  // namespace gmr
