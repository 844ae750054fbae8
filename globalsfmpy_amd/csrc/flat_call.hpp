// The scratch owner of the one-shot device calls (host arrays in, a few launches, host arrays out): edge_norms.hpp, spanning_tree.hpp,
// trans_filter.hpp, trans_refine.hpp, dense_check.hpp, cov_estimate.hpp, and through track_scene.hpp's TrackScene (the slots every call
// over cameras and tracks takes) triangulate.hpp and outlier_tracks.hpp.  FlatLayout lays the call's arrays out in one
// slab (plain arithmetic, no HIP: tests/cpp/flat_layout_test.cpp builds it with the host compiler alone).  FlatCall::commit then checks the
// free memory and creates a private non-blocking stream, the timing events and the slab; the destructor frees them on every path.  Nothing
// is kept between calls, nothing touches the default stream or synchronises the device: a flat call never stalls a problem's stream.
#pragma once
#include <cstddef>

namespace {

template <typename T> struct Slot { size_t off; };   // a T[count] in the slab, by its byte offset

struct FlatLayout {
  size_t total = 0;
  // Slots follow each other in take order, each on a 256-byte boundary.  A zero-count take uses no space: its slot shares the next
  // one's offset and is never dereferenced.
  template <typename T> Slot<T> take(size_t count) {
    const Slot<T> s{total};
    total += (count * sizeof(T) + 255) / 256 * 256;
    return s;
  }
};

// A problem's slab (solver_pos.hpp, solver_ba.hpp, solver_full_ba.hpp): take(ptr, count) lays the array out and, given the committed slab,
// points ptr into it; the same list of takes serves both passes
struct SlabTake {
  FlatLayout L;
  char* slab;
  template <typename E> void operator()(E*& ptr, size_t count) {
    const Slot<E> slot = L.take<E>(count);
    if (slab) ptr = (E*)(slab + slot.off);
  }
};

}  // namespace

#ifdef __HIPCC__
#include "host_common.hpp"

namespace {

struct FlatCall {
  hipStream_t s = nullptr;
  hipEvent_t ev[6] = {};   // a begin / end pair per span: the spanning tree has three spans
  int n_ev = 0, n_rec = 0;
  char* slab = nullptr;
  FlatCall() = default;
  FlatCall(const FlatCall&) = delete;
  ~FlatCall() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); if (slab) (void)hipFree(slab); if (s) (void)hipStreamDestroy(s); }

  // 0, or the status of a failure (the message is set)
  int commit(const FlatLayout& L, const char* who, int n_spans) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b < (double)L.total * 1.02 + (64u << 20))
      return fail(GSFM_ERR_HIP, std::string("not enough free device memory for ") + who + " (" + std::to_string((long long)(L.total >> 20)) + " MiB needed, " +
                                std::to_string((long long)(free_b >> 20)) + " MiB free)");
    (void)hipGetLastError();
    n_ev = std::min(2 * n_spans, 6);
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (int k = 0; k < n_ev; ++k) HIPCHK(hipEventCreate(&ev[k]));
    if (hipMalloc((void**)&slab, L.total) == hipSuccess) return 0;
    slab = nullptr; (void)hipGetLastError();
    return fail(GSFM_ERR_HIP, std::string("allocating the buffers of ") + who + " failed");
  }

  template <typename T> T* ptr(Slot<T> h) const { return (T*)(slab + h.off); }
  // count is in elements of T; the host array is of T or of T's scalar (a double4 slot takes 4 doubles per element)
  template <typename T, typename U> hipError_t upload(Slot<T> h, const U* host, size_t count) {
    static_assert(sizeof(T) % sizeof(U) == 0, "host array of another element size");
    return hipMemcpyAsync(slab + h.off, host, sizeof(T) * count, hipMemcpyHostToDevice, s);
  }
  template <typename T, typename U> hipError_t download(U* host, Slot<T> h, size_t count) {
    static_assert(sizeof(T) % sizeof(U) == 0, "host array of another element size");
    return hipMemcpyAsync(host, slab + h.off, sizeof(T) * count, hipMemcpyDeviceToHost, s);
  }
  template <typename T> hipError_t zero(Slot<T> h, size_t count) { return hipMemsetAsync(slab + h.off, 0, sizeof(T) * count, s); }

  // kernel_ms() is the device time between each begin_span() and its end_span(), summed; valid after the sync() that follows the last span
  hipError_t begin_span() { return n_rec < n_ev ? hipEventRecord(ev[n_rec++], s) : hipErrorInvalidValue; }
  hipError_t end_span() { return begin_span(); }
  hipError_t sync() { const hipError_t e = hipStreamSynchronize(s); return e != hipSuccess ? e : hipGetLastError(); }
  double kernel_ms() const {
    double sum = 0.0;
    for (int k = 0; k + 1 < n_rec; k += 2) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[k], ev[k + 1]); sum += ms; }
    return sum;
  }
};

}  // namespace
#endif
