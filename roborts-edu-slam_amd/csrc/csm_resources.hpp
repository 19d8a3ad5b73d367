// csm_resources.hpp — what owns device memory, pinned host memory, events and
// streams on the host side: one move-only buffer template over an allocation
// policy, and two move-only handle types. A struct made of them (LaunchSlot,
// GridState in csm_host.hpp; csm_gridmap) frees itself, moves and swaps whole.
//
// Buffer's logic needs no HIP: with CSM_RESOURCES_NO_HIP defined the header
// stops before the HIP policies (tests/cpp/resources_check.cpp instantiates
// Buffer over a counting malloc / free policy).
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>

namespace csm {

// Capacity to allocate for a buffer that must hold `bytes` and holds `cap`
// now: at least 64 KiB, and half as much again as before (at most 256 MiB
// more than asked), so per-scan sizes that creep up (a scan's points and
// endpoints) do not reallocate scan after scan — hipFree / hipHostFree
// synchronise the device, a few hundred microseconds in the online path.
inline size_t grow_bytes(size_t bytes, size_t cap) {
  size_t want = bytes < ((size_t)64 << 10) ? ((size_t)64 << 10) : bytes;
  if (cap) {
    size_t more = cap + cap / 2, lim = bytes + ((size_t)256 << 20);
    if (more > lim) more = lim;
    if (more > want) want = more;
  }
  return want;
}

}  // namespace csm

namespace csmh {

// Mem: `Status`, `kOk`, static Status alloc(void**, size_t, flags...) and
// static void free(void*). Contents are never kept across a reallocation.
template <class Mem>
struct Buffer {
  using Status = typename Mem::Status;
  void* p = nullptr;
  size_t cap = 0;

  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~Buffer() { release(); }

  // room for `bytes`, grown by grow_bytes (buffers whose sizes creep up)
  template <class... Flags>
  Status ensure(size_t bytes, Flags... flags) {
    return bytes <= cap ? Mem::kOk : reallocate(csm::grow_bytes(bytes, cap), flags...);
  }
  // room for `bytes`, allocated as asked (the search's levels are gigabytes)
  template <class... Flags>
  Status ensure_exact(size_t bytes, Flags... flags) {
    return bytes <= cap ? Mem::kOk : reallocate(bytes, flags...);
  }
  void release() {
    if (p) Mem::free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }

 private:
  template <class... Flags>
  Status reallocate(size_t want, Flags... flags) {
    release();
    const Status e = Mem::alloc(&p, want, flags...);
    if (e == Mem::kOk)
      cap = want;
    else
      p = nullptr;
    return e;
  }
};

// one owner: not copyable, and moves cannot throw (std::swap, std::vector)
template <class T>
constexpr bool kMoveOnly = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
                           std::is_nothrow_move_constructible<T>::value &&
                           std::is_nothrow_move_assignable<T>::value;

}  // namespace csmh

#ifndef CSM_RESOURCES_NO_HIP
#include <hip/hip_runtime_api.h>

namespace csmh {

struct DeviceMem {
  using Status = hipError_t;
  static constexpr Status kOk = hipSuccess;
  static Status alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};

struct PinnedMem {  // flags: hipHostMallocCoherent for buffers kernels write straight into
  using Status = hipError_t;
  static constexpr Status kOk = hipSuccess;
  static Status alloc(void** p, size_t bytes, unsigned flags = hipHostMallocDefault) {
    return hipHostMalloc(p, bytes, flags);
  }
  static void free(void* p) { (void)hipHostFree(p); }
};

using DevBuf = Buffer<DeviceMem>;
using HostBuf = Buffer<PinnedMem>;  // pinned staging

// An owned HIP handle, destroyed with its owner; converts to the raw handle,
// so HIP calls and non-owning copies (PendingRun) take it as they took that.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Handle() { reset(); }
  operator H() const { return h; }
  void reset() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  // once: a handle already made is kept (hipEventDefault: a timed event)
  hipError_t create(unsigned flags) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) { return h ? hipSuccess : hipStreamCreateWithFlags(&h, flags); }
};

static_assert(kMoveOnly<DevBuf> && kMoveOnly<HostBuf> && kMoveOnly<Event> && kMoveOnly<Stream>,
              "buffers and handles have one owner");

}  // namespace csmh
#endif  // CSM_RESOURCES_NO_HIP
