// Host <-> device staging shared by the single, t-slab and multi-device contexts: report fields in row chunks, rollout
// and policy samples in sample chunks, and the copies of state planes between the caller's float64 arrays and device
// arrays in the context's precision.  A call that moves caller arrays through a bounded device buffer uses one of these
// helpers; nobody else computes a chunk size.  Included by pdhg_api.hip (fail, HIP_TRY) before ctx_impl.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <memory>
#include <utility>

namespace {

// the device temporaries of one call stay within these however many rows / samples the call has
constexpr size_t kReportBudget = (size_t)64 << 20;
constexpr size_t kTrajBudget = (size_t)64 << 20;

// one device allocation, freed on every way out (device >= 0: made current for the free); never copied or moved
struct DevBuf {
  void* p = nullptr;
  int device;
  explicit DevBuf(int dev = -1) : device(dev) {}
  DevBuf(const DevBuf&) = delete;
  ~DevBuf() {
    if (p && device >= 0) hipSetDevice(device);
    if (p) hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  int alloc_for(size_t bytes, const char* what) {
    if (alloc(bytes) == hipSuccess) return PDHG_OK;
    return fail(PDHG_ERR_NOMEM, "hipMalloc(%zu bytes) for the %s failed", bytes, what);
  }
};

// ---------------- report fields in row chunks ----------------
// rows [row0, row0 + nrows) within the T residual rows of a window ("the") or of a slab ("the slab's")
inline int rows_inside(int row0, int nrows, int T, const char* whose = "the") {
  if (row0 < T && nrows <= T - row0) return PDHG_OK;   // (no row0 + nrows: it may not fit an int)
  return fail(PDHG_ERR_ARG, "%d rows from row %d outside %s residual rows [0, %d)", nrows, row0, whose, T);
}

// The HJ and continuity residual planes of a row range into the caller's arrays hj / cont ([nrows][npl] each, null:
// not wanted), staged through one allocation of at most kReportBudget bytes.
struct RowChunks {
  hipStream_t stream;
  size_t npl;
  double *hj, *cont;
  // launch(c0, mc, d_hj, d_cont): rows [c0, c0 + mc) of the range into the device planes, on `stream`
  template <typename Launch>
  int run(int nrows, Launch&& launch) const {
    if (!hj && !cont) return PDHG_OK;
    const size_t per = npl * sizeof(double) * ((hj ? 1 : 0) + (cont ? 1 : 0));
    const int m = (int)std::min<size_t>((size_t)nrows, std::max<size_t>(kReportBudget / per, 1));   // rows per chunk
    DevBuf buf;
    int rc;
    if ((rc = buf.alloc_for((size_t)m * per, "report rows"))) return rc;
    double* d_hj = hj ? (double*)buf.p : nullptr;
    double* d_cont = cont ? (double*)buf.p + (hj ? (size_t)m * npl : 0) : nullptr;
    for (int c0 = 0; c0 < nrows; c0 += m) {
      const int mc = std::min(m, nrows - c0);
      if ((rc = launch(c0, mc, d_hj, d_cont))) return rc;
      const size_t nb = (size_t)mc * npl * sizeof(double);
      if (hj) HIP_TRY(hipMemcpyAsync(hj + (size_t)c0 * npl, d_hj, nb, hipMemcpyDeviceToHost, stream));
      if (cont) HIP_TRY(hipMemcpyAsync(cont + (size_t)c0 * npl, d_cont, nb, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));   // the chunk planes are reused
    }
    return PDHG_OK;
  }
};

// ---------------- rollout and policy samples in sample chunks ----------------
// Samples are staged in chunks of whole workgroups out of one allocation: the device temporaries (positions in / out,
// the chunk's noise, records or per-sample outputs) stay within kTrajBudget however many samples and rows the call
// has.  `lead` doubles come first (the policy check's partial table), then a chunk's buffers, carved by take().
struct SampleChunks {
  size_t n;                 // samples of the call
  hipStream_t stream;       // of the copies (the multi-device rollout sets it per slab: slabs may share a device)
  DevBuf buf;
  size_t m = 0;             // samples per chunk: a multiple of 256, or n
  double* base = nullptr;
  double* next = nullptr;
  SampleChunks(size_t n_, hipStream_t s, int device = -1) : n(n_), stream(s), buf(device) {}
  // per: bytes a sample takes in the chunk buffers; 0 (grid starts with the report only): the call is one chunk
  int alloc(size_t per, size_t lead, const char* what) {
    m = std::min(n, per ? std::max<size_t>(kTrajBudget / per, 256) / 256 * 256 : n);
    if (int rc = buf.alloc_for(lead * sizeof(double) + m * per, what)) return rc;
    base = (double*)buf.p;
    next = base + lead;
    return PDHG_OK;
  }
  double* take(bool on, size_t doubles) { return on ? std::exchange(next, next + doubles) : nullptr; }
  // rows [j0, j0 + rows) x samples [c0, c0 + mc) of a host array [.][n][w] to / from the same rows of the dense
  // device array [.][mc][w]; an array that is not there (null on either side) moves nothing.  d is take()'s, const
  // only in the argument block.
  int up(const double* d, const double* h, int j0, int rows, size_t c0, size_t mc, size_t w) const {
    for (int j = j0; d && h && j < j0 + rows; ++j)
      HIP_TRY(hipMemcpyAsync(const_cast<double*>(d) + (size_t)j * mc * w, h + ((size_t)j * n + c0) * w,
                             mc * w * sizeof(double), hipMemcpyHostToDevice, stream));
    return PDHG_OK;
  }
  int down(double* h, const double* d, int j0, int rows, size_t c0, size_t mc, size_t w) const {
    for (int j = j0; d && h && j < j0 + rows; ++j)
      HIP_TRY(hipMemcpyAsync(h + ((size_t)j * n + c0) * w, d + (size_t)j * mc * w, mc * w * sizeof(double),
                             hipMemcpyDeviceToHost, stream));
    return PDHG_OK;
  }
};

// The rollout's chunk: positions in and out [w_x] per sample, then what the call asked for of the noise [T][w_x], the
// position record [T + 1][w_x] and the control record [T][w_a], rows indexed by (global) step.
struct RolloutLayout {
  int T;
  size_t w_x, w_a;   // doubles per sample and row: positions / noise, controls
  bool noise, rec_x, rec_a;
  size_t per() const {   // bytes per sample
    return sizeof(double) * (2 * w_x + (noise ? (size_t)T * w_x : 0) + (rec_x ? (size_t)(T + 1) * w_x : 0) +
                             (rec_a ? (size_t)T * w_a : 0));
  }
  struct Ptrs {
    double *x_in, *x_out, *noise, *rec_x, *rec_a;
  };
  Ptrs carve(SampleChunks& st) const {   // after st.alloc(per(), ...); a braced list is evaluated in order
    return {st.take(true, st.m * w_x), st.take(true, st.m * w_x), st.take(noise, (size_t)T * st.m * w_x),
            st.take(rec_x, (size_t)(T + 1) * st.m * w_x), st.take(rec_a, (size_t)T * st.m * w_a)};
  }
};

// ---------------- state planes: the caller's float64 arrays <-> device arrays of E = float or double ----------------
// fp64 copies go straight from / to the caller's array; fp32 through `scratch` (cnt elements of E, unused for fp64;
// also_fp64: the alp interleave below needs it in either precision)
template <typename E>
std::unique_ptr<E[]> plane_scratch(size_t cnt, bool also_fp64 = false) {   // not value-initialised: filled before read
  return std::unique_ptr<E[]>(sizeof(E) == 8 && !also_fp64 ? nullptr : new E[cnt]);
}
// the caller's doubles as elements of E, for an upload (Impl::h2d): themselves, or narrowed into scratch
template <typename E>
const E* as_elems(const double* src, size_t cnt, void* scratch) {
  if constexpr (sizeof(E) == 8) {
    return src;
  } else {
    E* b = static_cast<E*>(scratch);
    for (size_t i = 0; i < cnt; ++i) b[i] = (E)src[i];
    return b;
  }
}
// device src [off, off + cnt) -> dst [0, cnt), by a synchronous copy (the caller has drained the stream)
template <typename E>
int get_plane(double* dst, const E* src, size_t off, size_t cnt, void* scratch) {
  if constexpr (sizeof(E) == 8) {
    HIP_TRY(hipMemcpy(dst, src + off, cnt * sizeof(E), hipMemcpyDeviceToHost));
  } else {
    E* b = static_cast<E*>(scratch);
    HIP_TRY(hipMemcpy(b, src + off, cnt * sizeof(E), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cnt; ++i) dst[i] = (double)b[i];
  }
  return PDHG_OK;
}
// component c of array a of the reference's alp [.][n][nc] <-> a dense run of n elements (a live component's array)
template <typename E>
void alp_gather(E* dense, const double* alp, size_t n, int nc, int a, int c) {
  for (size_t i = 0; i < n; ++i) dense[i] = (E)alp[((size_t)a * n + i) * nc + c];
}
template <typename E>
void alp_scatter(double* alp, const E* dense, size_t n, int nc, int a, int c) {
  for (size_t i = 0; i < n; ++i) alp[((size_t)a * n + i) * nc + c] = (double)dense[i];
}

}  // namespace
