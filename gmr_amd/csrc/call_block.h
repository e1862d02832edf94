// call_block.h -- the layout of one block of device memory that a call fills from the host: the model image, and the
// stream-ordered scratch of a member-wise call (entries, clip offsets, plans, then what only the device writes).
//
// Host only, plain C++17, no HIP: reserve arrays, get typed handles (offsets, not pointers), write the uploaded ones through the
// block's zero-initialised host image, and resolve handles to device pointers through the view that on(base) returns -- there is
// no other way to a device pointer, so none exists before the block's address does.
//   - every array starts on a 16-byte boundary;
//   - the device-only arrays lie behind all uploaded ones, whatever the order of the reservations, so the upload is the one
//     contiguous prefix image() / uploaded_bytes().
// Allocation and the copy are the caller's (api.hip: send_call_block, gmr_model_create).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace gmr {

class CallBlock {
  static size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

 public:
  template <class T> struct Uploaded { size_t at = 0, n = 0; };    // `at`: bytes from the block's start
  template <class T> struct DeviceOnly { size_t at = 0, n = 0; };  // `at`: bytes from the start of the device-only tail

  // An uploaded array of n elements of T, zero until written through (*this)[handle].
  template <class T>
  Uploaded<T> uploaded(size_t n) {
    if (placed_) abort();
    const size_t at = align16(image_.size());
    image_.resize(at + n * sizeof(T), 0);
    return {at, n};
  }
  // An uploaded copy of src[0 .. n), in an array of at least min_n elements.
  template <class T>
  Uploaded<T> put(const T *src, size_t n, size_t min_n = 0) {
    const Uploaded<T> h = uploaded<T>(n > min_n ? n : min_n);
    if (n) memcpy(image_.data() + h.at, src, n * sizeof(T));
    return h;
  }
  template <class T>
  Uploaded<T> put(const std::vector<T> &v, size_t min_n = 0) { return put(v.data(), v.size(), min_n); }
  // An array of n elements of T that only the device reads and writes: no host image, not uploaded.
  template <class T>
  DeviceOnly<T> device_only(size_t n) {
    if (placed_) abort();
    const size_t at = align16(tail_);
    tail_ = at + n * sizeof(T);
    return {at, n};
  }

  // The host image of an uploaded array.  The pointer holds until the next reservation.
  template <class T>
  T *operator[](Uploaded<T> h) { return reinterpret_cast<T *>(image_.data() + h.at); }

  const void *image() const { return image_.data(); }
  size_t uploaded_bytes() const { return image_.size(); }
  size_t total_bytes() const { return tail_ ? align16(image_.size()) + tail_ : image_.size(); }

  // The block at device address `base` (16-byte aligned, total_bytes() long): handles to device pointers.
  class Device {
    uint8_t *base_;
    size_t tail_at_;
    friend class CallBlock;
    Device(void *base, size_t tail_at) : base_(static_cast<uint8_t *>(base)), tail_at_(tail_at) {}

   public:
    template <class T> T *operator()(Uploaded<T> h) const { return reinterpret_cast<T *>(base_ + h.at); }
    template <class T> T *operator()(DeviceOnly<T> h) const { return reinterpret_cast<T *>(base_ + tail_at_ + h.at); }
  };
  // Every reservation comes before this (one made later aborts: it would move the tail under the view's feet).
  Device on(void *base) {
    placed_ = true;
    return Device(base, align16(image_.size()));
  }

 private:
  std::vector<uint8_t> image_;  // the uploaded prefix
  size_t tail_ = 0;             // bytes of the device-only tail
  bool placed_ = false;
};

}  // namespace gmr
