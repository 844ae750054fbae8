// The device scalars of a Euclidean problem (solver_pos.hpp, solver_ba.hpp, solver_full_ba.hpp): scal[slot] is written by a reduction over the
// GSFM_POS_PARTS partial sums in part, in a fixed order, and read back by a copy that is waited for.  Everything is enqueued on the
// problem's stream.
#pragma once
#include "host_common.hpp"
#include "pos_kernels.hpp"

namespace {

struct DevScalars {
  hipStream_t s;
  double *part, *scal;
  // bytes from the device, waited for
  int read(void* dst, const void* src_dev, size_t bytes, const char* what) const {
    HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, s));
    return sync_stream(s, what);
  }
  int read_slot(int slot, double* v, const char* what) const { return read(v, scal + slot, 8, what); }
  // the reader that lm_loop.hpp's pcg_loop wants (slot 0 is its PCG_RZ0)
  auto pcg_reader() const { return [V = *this](int slot, double* v) { return V.read_slot(slot, v, slot == 0 ? "pcg start" : "pcg"); }; }
  void reduce(int slot, int is_max = 0) const { hipLaunchKernelGGL(k_pos_reduce, dim3(1), dim3(256), 0, s, part, scal + slot, is_max); }
  // scal[slot] = a . b over n_rows x 3 entries (mask: per row)
  void dot(const double* a, const double* b, const uint8_t* mask, size_t n_rows, int slot) const {
    hipLaunchKernelGGL(k_pos_dot, dim3(GSFM_POS_PARTS), dim3(256), 0, s, a, b, mask, 3 * n_rows, part);
    reduce(slot);
  }
  // scal[slot_gmax] = max |g| and scal[slot_xnorm2] = |x|^2 over the rows of mask
  void norms(const double* g, const double* x, const uint8_t* mask, size_t n_rows, int slot_gmax, int slot_xnorm2) const {
    hipLaunchKernelGGL(k_pos_absmax, dim3(GSFM_POS_PARTS), dim3(256), 0, s, g, mask, 3 * n_rows, part);
    reduce(slot_gmax, 1);
    dot(x, x, mask, n_rows, slot_xnorm2);
  }
};

}  // namespace
