// The context behind a pdhg_ctx handle: device buffers, tables, the kernel launchers and the iteration loop.
// What to launch is decided by plan_paths() (path_plan.hpp) at creation; the launchers below read the plan (pp).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "kernels_1d.hpp"
#include "kernels_2d.hpp"
#include "kernels_2d_fast.hpp"
#include "kernels_dual_lds.hpp"
#include "kernels_dual_multi.hpp"
#include "kernels_common.hpp"
#include "kernels_xslab.hpp"
#include "kernels_xt_batch.hpp"
#include "kernels_xt_dma.hpp"
#include "kernels_thomas_chunk.hpp"
#include "kernels_fs_wide.hpp"
#include "kernels_fs16.hpp"
#include "kernels_xt_f64.hpp"
#include "kernels_traj.hpp"
#include "kernels_report.hpp"
#include "kernels_policy.hpp"
#include "path_plan.hpp"

using namespace pdhg;

namespace {

template <typename R>
std::vector<cplx<R>> twiddles(int n) {
  std::vector<cplx<R>> t(n);
  for (int k = 0; k < n; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)n;
    t[k].x = (R)std::cos(a);
    t[k].y = (R)std::sin(a);
  }
  return t;
}

struct ProfEntry {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
};

// pdhg_report from one folded row of kNumSums report sums (kernels_report.hpp) over n_points points
inline pdhg_report report_from_sums(const double* h, long long n_points) {
  pdhg_report r{};
  r.n_points = n_points;
  r.n_nonfinite = (long long)h[6];
  r.n_rho_zero = (long long)h[7];
  const double n = (double)(r.n_points - r.n_nonfinite);
  if (n > 0) {
    r.hj_l1 = h[0] / n;
    r.hj_l2 = std::sqrt(h[1] / n);
    r.compl_l1 = h[3] == 0.0 ? 0.0 : h[2] / h[3];
    r.rho_mean = h[3] / n;
    r.cont_l1 = h[4] / n;
    r.cont_l2 = std::sqrt(h[5] / n);
    r.hj_max = h[8];
    r.hj_pos_max = h[9];
    r.hj_active_max = h[10];
    r.cont_max = h[11];
    r.rho_max = h[12];
    r.rho_min = -h[13];
    r.phi_max = h[14];
    r.phi_min = -h[15];
  } else {
    const double nan = std::nan("");
    r.hj_l1 = r.hj_l2 = r.hj_max = r.hj_pos_max = r.hj_active_max = r.compl_l1 = nan;
    r.cont_l1 = r.cont_l2 = r.cont_max = r.rho_min = r.rho_max = r.rho_mean = r.phi_min = r.phi_max = nan;
  }
  return r;
}

// pdhg_policy_report from one folded row of the policy check's sums (kernels_policy.hpp) over n_sample samples
inline pdhg_policy_report policy_from_sums(const double* h, long long n_sample) {
  pdhg_policy_report r{};
  r.n_sample = n_sample;
  r.n_nonfinite = (long long)h[6];
  const double n = (double)(r.n_sample - r.n_nonfinite);
  if (n > 0) {
    r.running_mean = h[0] / n;
    r.terminal_mean = h[1] / n;
    r.value_mean = h[2] / n;
    r.gap_mean = h[3] / n;
    r.gap_abs_mean = h[4] / n;
    r.gap_rms = std::sqrt(h[5] / n);
    r.cost_mean = h[7] / n;
    r.gap_abs_max = h[8];
    r.gap_hi = h[9];
    r.gap_lo = -h[10];
  } else {
    const double nan = std::nan("");
    r.cost_mean = r.value_mean = r.running_mean = r.terminal_mean = nan;
    r.gap_mean = r.gap_abs_mean = r.gap_rms = r.gap_abs_max = r.gap_lo = r.gap_hi = nan;
  }
  return r;
}

// pdhg_stats from the loop control block (rho's range is not tracked on the device)
inline void stats_from_ctrl(const Ctrl& h, pdhg_stats* st) {
  st->iters_run = h.iters;
  st->status = h.done;
  st->inner_last = h.inner_count;
  st->inner_total = h.inner_total;
  st->err1 = h.err1;
  st->err2 = h.err2;
  st->err_inner = h.err_inner;
  st->rho_min = NAN;
  st->rho_max = NAN;
  st->nan_seen = h.nan_seen;
  st->first_nan_iter = h.first_nan;
}

struct ImplBase {
  int device = 0;  // every entry point selects it before touching the context (dispatch)
  virtual ~ImplBase() {}
};

template <int V>
using IC = std::integral_constant<int, V>;

// R: the arithmetic of the state, the tables and the transforms; P: the type phi and phi_bar are held in (P = double
// with R = float is the mixed context, precision 12: kp.phi / kp.phibar stay null, px carries the double pair)
template <typename R, typename P = R>
struct Impl : ImplBase {
  using C = cplx<R>;
  using Real = R;
  static constexpr bool kMixed = !std::is_same<R, P>::value;
  static_assert(!kMixed || (sizeof(R) == 4 && sizeof(P) == 8), "mixed: float state, double phi / phi_bar");
  pdhg_problem pb{};
  hipStream_t stream = nullptr;
  KP<R> kp{};
  PhiX<R, P> px{};
  P* phi_dev() const {
    if constexpr (kMixed) return px.phi;
    else return kp.phi;
  }
  P* phibar_dev() const {
    if constexpr (kMixed) return px.phibar;
    else return kp.phibar;
  }
  C* twx = nullptr;
  C* twy = nullptr;
  std::vector<void*> allocs;
  Tuning tun = Tuning::from_env();   // the environment at creation
  PathPlan pp;                       // what runs (setup)
  int n_contig_fail = 0;   // contiguous requests that fell back to hipMalloc
  size_t dev_bytes = 0;
  double row0_sq = 0.0;
  // runtime state of the schedule
  bool outer_merged = false; // launch_dual merged this iteration's outer finalize: launch_outer skips it
  bool spec = false;         // iterate() uses the speculative schedule now (launch_dual / launch_outer / the graph)
  long long spec_iters = 0, spec_halts = 0;   // iterations enqueued speculatively / halts (path_info, tests)
  bool res_valid = false;   // p.res / p.ey hold the residual of the current (rho, alp)
  int n_cu = 256;           // compute units (persistent grids)
  C* tw256 = nullptr;             // W_256 table of the four-step stages
  double* fold_out = nullptr;
  double* prim_partials = nullptr;   // the update's partial rows when the speculative finalize merges the primal's
  int prim_merged_rows = 0;          // > 0: launch_primal left its finalize to k_finalize_dual_outer (rows to reduce)
  bool primal_done = false;
  int stop_conv = 1, stop_nan = 1;   // reference stop rules (utils_pdhg_solver.py:74-80)
  // profiling
  bool prof = false;
  std::map<std::string, ProfEntry> prof_ev;
  int* h_done = nullptr;   // pinned
  bool own_stream = true;
  // t-slab decomposition (multi-GPU): this context owns unknown rows [slab_j0, slab_j0 + T) of slab_Tg
  bool slab = false;
  int slab_j0 = 0, slab_Tg = 0;
  size_t Mspec = 0;          // spectral plane (work row) size
  R* halo_rho = nullptr;     // rho row j0+T from the next slab
  R* carry_y = nullptr;      // backward right carry (spectral plane)
  R* dsbuf = nullptr;        // [D, S1] exchange planes of this slab (2 x Mspec)
  int* long_pos = nullptr;   // neighbour exchange: per mode, index in the long-range list or -1
  int* long_idx = nullptr;   // the long-range modes (long_K of them)
  int long_K = -1;           // -1: not classified yet
  // x-slab decomposition (multi-GPU for T = 1 marching windows): this context owns global x rows
  // [xs_x0, xs_x0 + xs_nloc) of xs_nxg; its spatial arrays hold nx = xs_nloc + 16 rows (kernels_xslab.hpp)
  bool xslab = false;
  int xs_rank = 0, xs_P = 1, xs_nxg = 0, xs_nloc = 0, xs_x0 = 0;
  R* colwork = nullptr;      // [T][nbs][nxg][B]: this rank's column blocks, whole x lines
  const R* lamy_base = nullptr;
  std::vector<double> xs_local;   // x coordinates of the nx local rows (ghost / padding rows wrap periodically)

  ~Impl() override {
    if (stream) hipStreamSynchronize(stream);
    drop_graph();
    for (void* p : allocs) hipFree(p);
    for (auto& kv : prof_ev)
      for (auto& e : kv.second.ev) {
        hipEventDestroy(e.first);
        hipEventDestroy(e.second);
      }
    if (h_done) hipHostFree(h_done);
    if (stream && own_stream) hipStreamDestroy(stream);
  }

  template <typename T>
  int alloc(T** p, size_t n) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    // Large arrays of fp32 2-D contexts physically contiguous: with the default allocator the physical
    // placement of C3's 13 GB planes differs from context to context, and so did the dual / update times
    // (dual 30.3 - 35.4 ms across contexts, stable to 0.05 ms within one); contiguous planes ran 29.5 - 30.5.
    // The same placement made fp64 C3's generic residual 71 -> 91 ms and fp32 C1's update 0.12 -> 0.14 ms,
    // and C2 was neutral (interleaved A/B), hence fp32 2-D only.  Falls back to
    // hipMalloc (counted: path_info "contig_fail").
    const bool contig = tun.alloc_mode > 0 || (tun.alloc_mode == 0 && sizeof(R) == 4 && pb.ndim == 2);
    hipError_t e = hipErrorOutOfMemory;
    if (bytes >= ((size_t)64 << 20) && contig) {
      e = hipExtMallocWithFlags(&q, bytes, hipDeviceMallocContiguous);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        n_contig_fail++;
      }
    }
    if (e != hipSuccess) e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(PDHG_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    allocs.push_back(q);
    dev_bytes += bytes;
    *p = static_cast<T*>(q);
    return PDHG_OK;
  }

  // Host -> device copies on the context's stream (stream-ordered): the stream is non-blocking, so a copy on the
  // legacy null stream (hipMemcpy / hipMemset) has no ordering guarantee with the kernels enqueued on it
  int h2d(void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PDHG_OK;
  }
  size_t plane() const { return (size_t)pb.nx * (size_t)pb.ny; }

  // make the plan, fill the KP scalars, allocate, build and upload the tables
  int setup() {
    const int nx = pb.nx, ny = pb.ny, T = pb.T;
    const int nxg = xslab ? xs_nxg : nx;   // length of the x transform (global nx for an x-slab)
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    HIP_TRY(hipHostMalloc((void**)&h_done, sizeof(int), hipHostMallocDefault));
    const bool is2d = pb.ndim == 2;
    std::string why;
    const Decomp dc{slab, slab_j0, slab_Tg, xslab, xs_rank, xs_P, xs_nxg, xs_nloc, kMixed};
    if (int rc = plan_paths(pb, (int)sizeof(R), dc, tun, pp, why)) return fail(rc, "%s", why.c_str());
    const int na = pp.na;
    const bool two_sets = pp.two_sets, fs16 = pp.fs16;

    KP<R>& p = kp;
    p.egno = pb.egno;
    p.ndim = pb.ndim;
    p.bcx = pb.bc_x;
    p.bcy = pb.bc_y;
    p.nx = nx;
    p.ny = ny;
    p.T = T;
    p.na = na;
    p.inv_dx = (R)(1.0 / pb.dx);
    p.inv_dy = (R)(is2d ? 1.0 / pb.dy : 0.0);
    p.inv_dt = (R)(1.0 / pb.dt);
    p.inv_dx2 = (R)(1.0 / (pb.dx * pb.dx));
    p.inv_dy2 = (R)(is2d ? 1.0 / (pb.dy * pb.dy) : 0.0);
    p.epsl = (R)pb.epsl;
    p.c_over_dt = (R)(pb.c_on_rho / pb.dt);
    p.C = (R)pb.C;
    p.inv_n = (R)(1.0 / ((double)nxg * (double)ny));
    // t-Laplacian off-diagonal: Ct/dt^2 in 1-D (utils_precond.py:128-131); 2-D ignores Ct (:164-168)
    p.ae = (R)((is2d ? 1.0 : pb.Ct) / (pb.dt * pb.dt));
    p.half_real = pp.half_real ? 1 : 0;
    p.B = pp.B;
    p.lB = pp.lB;
    p.nb = pp.nb;
    p.rows_per_wg = 2;
    p.tile_j = pp.tile_j;
    if (is2d) {
      p.dbg = tun.dbg;
      p.nbsync = tun.nbsync;
      p.dual_order = pp.dual_order;
    }
    p.slab = slab ? 1 : 0;
    p.j0 = slab ? slab_j0 : 0;
    p.Tg = slab ? slab_Tg : T;
    p.last_slab = (p.j0 + T == p.Tg) ? 1 : 0;
    p.xt_phase = 0;
    p.row_base = 0;
    p.row_cnt = T;
    p.xl0 = xslab ? 8 : 0;
    p.xl1 = xslab ? 8 + xs_nloc : nx;

    // ---- device buffers ----
    const size_t npl = plane();
    int rc;
    if constexpr (kMixed) {
      p.phi = p.phibar = nullptr;
      if ((rc = alloc(&px.phi, (size_t)(T + 1) * npl))) return rc;
      if ((rc = alloc(&px.phibar, (size_t)(T + 1) * npl))) return rc;
      px.inv_dx = 1.0 / pb.dx;
      px.inv_dy = 1.0 / pb.dy;
      px.inv_dt = 1.0 / pb.dt;
      px.inv_dx2 = 1.0 / (pb.dx * pb.dx);
      px.inv_dy2 = 1.0 / (pb.dy * pb.dy);
      px.epsl = pb.epsl;
    } else {
      if ((rc = alloc(&p.phi, (size_t)(T + 1) * npl))) return rc;
      if ((rc = alloc(&p.phibar, (size_t)(T + 1) * npl))) return rc;
    }
    const size_t nwork = is2d ? (size_t)T * p.nb * nx * p.B : (size_t)T * nx;
    if ((rc = alloc(&p.work, nwork))) return rc;
    for (int s = 0; s < (two_sets ? 2 : 1); ++s) {
      if ((rc = alloc(&p.rho[s], (size_t)T * npl))) return rc;
      for (int a = 0; a < na; ++a)
        if ((rc = alloc(&p.alp[s][a], (size_t)T * npl))) return rc;
    }
    if (!two_sets) {
      p.rho[1] = p.rho[0];
      for (int a = 0; a < 4; ++a) p.alp[1][a] = p.alp[0][a];
    }
    for (int a = na; a < 4; ++a) p.alp[0][a] = p.alp[1][a] = nullptr;
    // rows: the kernels' partials, the fold's rows, and the update's partials of a speculative iteration (kept for the
    // merged finalize: the dual reuses the first region)
    if ((rc = alloc(&p.partials, (2 * pp.partial_rows + kFoldRows) * kNumSums))) return rc;
    fold_out = p.partials + pp.partial_rows * kNumSums;
    prim_partials = fold_out + kFoldRows * kNumSums;
    if ((rc = alloc(&p.ctrl, 1))) return rc;
    if (pp.glb_line) {   // 2 lines of nx complex per concurrent workgroup (gx1 >= gx4)
      C* g = nullptr;
      if ((rc = alloc(&g, (size_t)pp.gx1 * 2 * nx))) return rc;
      p.gscr = g;
    }
    p.res = p.ex = p.ey = nullptr;
    p.rspec = nullptr;
    if (pp.fuse_res && is2d) {
      if ((rc = alloc(&p.res, (size_t)T * npl))) return rc;
      if ((rc = alloc(&p.ex, (size_t)T * (nx / 8) * 2 * ny))) return rc;
      if ((rc = alloc(&p.ey, (size_t)T * nx * (ny / (64 * pp.dual_ypl)) * 2))) return rc;
    } else if (pp.fuse_res) {   // 1-D: residual rows + the wave-edge terms [2][T][nx/64]
      if ((rc = alloc(&p.res, (size_t)T * npl))) return rc;
      if ((rc = alloc(&p.ex, (size_t)2 * T * (nx / 64)))) return rc;
    }
    // the task-order spectrum reuses the fused residual's R plane: a task's spectrum run [x0 rows, all ky] is exactly
    // the region its R rows occupy, and the residual kernel holds those rows in registers before it stores the run
    if (pp.tc_spec) {
      if (pp.fuse_res) p.rspec = p.res;
      else if ((rc = alloc(&p.rspec, nwork))) return rc;
    }
    if (xslab && (rc = alloc(&colwork, (size_t)T * pp.xs_nbs * nxg * p.B))) return rc;
    if (slab) {
      Mspec = (size_t)p.nb * nx * p.B;
      if ((rc = alloc(&halo_rho, npl))) return rc;
      if ((rc = alloc(&carry_y, Mspec))) return rc;
      if ((rc = alloc(&dsbuf, 2 * Mspec))) return rc;
      HIP_TRY(hipMemsetAsync(halo_rho, 0, npl * sizeof(R), stream));
      HIP_TRY(hipMemsetAsync(carry_y, 0, Mspec * sizeof(R), stream));
      p.rho_halo = p.last_slab ? nullptr : halo_rho;
      p.carry_y = carry_y;
    }
    HIP_TRY(hipMemsetAsync(p.ctrl, 0, sizeof(Ctrl), stream));

    // ---- coefficient / symbol tables (host fp64 -> R) ----
    std::vector<R> ax(nx), ay(std::max(ny, 1)), lamx(nxg), d0(nxg);
    grid_x.assign(pb.xs, pb.xs + nx);   // fp64 copies for trajectories(): the caller's arrays need not outlive create
    if (is2d) grid_y.assign(pb.ys, pb.ys + ny);
    for (int i = 0; i < nx; ++i) {
      const double x = pb.xs[i];
      ax[i] = (R)(pb.egno == 3 ? x : (x - 1.0) * (x - 1.0) + 0.1);   // set_fns.py:145 / :117-118 / :98
    }
    if (is2d)
      for (int i = 0; i < ny; ++i) {
        const double y = pb.ys[i];
        ay[i] = (R)((y - 1.0) * (y - 1.0) + 0.1);
      }
    // Laplacian symbol = FFT of the periodic stencil (utils_precond.py:42-71), real part.
    // bc (1,0) (egno 3): fv = fft_y(dct_x(lap)) = DCT-II(x stencil)[kx] + 2 cos(pi kx/2nx) * lam_y[ky]
    // -- the reference transforms the periodic stencil array with the DCT, and DCT-II(e_0) = 2 cos(.)
    const bool dct_x = is2d && pb.bc_x == 1;
    std::vector<R> cx(nxg, (R)1);
    std::vector<C> dctw;
    for (int k = 0; k < nxg; ++k) {
      double l = -2.0 * (1.0 - std::cos(2.0 * M_PI * k / nxg)) / (pb.dx * pb.dx);
      if (dct_x) {
        auto c2 = [&](int n) { return 2.0 * std::cos(M_PI * k * (2.0 * n + 1.0) / (2.0 * nxg)); };
        l = (-2.0 * c2(0) + c2(1) + c2(nxg - 1)) / (pb.dx * pb.dx);
        cx[k] = (R)c2(0);
      }
      lamx[k] = (R)l;
      d0[k] = (R)std::pow(pb.C - l, pb.pow_);   // 1-D thomas_b = (C - fv)^pow, :125-126
    }
    if (fs16) {   // chunk-major spectrum of kernels_fs16.hpp: mode k1 + 16 k2 at position 4096 k1 + k2
      std::vector<R> d0p(nxg);
      for (int k1 = 0; k1 < 16; ++k1)
        for (int k2 = 0; k2 < kF16N2; ++k2) d0p[(size_t)k1 * kF16N2 + k2] = d0[k1 + 16 * k2];
      d0.swap(d0p);
    }
    if (dct_x) {
      dctw.resize(nxg);
      for (int k = 0; k < nxg; ++k) {
        dctw[k].x = (R)std::cos(-M_PI * k / (2.0 * nxg));
        dctw[k].y = (R)std::sin(-M_PI * k / (2.0 * nxg));
      }
    }
    R *d_ax, *d_ay, *d_lamx, *d_lamy, *d_d0;
    if ((rc = alloc(&d_ax, nx))) return rc;
    if ((rc = alloc(&d_ay, std::max(ny, 1)))) return rc;
    if ((rc = alloc(&d_lamx, nxg))) return rc;
    if ((rc = alloc(&d_d0, nxg))) return rc;
    H2D(d_ax, ax.data(), nx * sizeof(R));
    H2D(d_ay, ay.data(), ay.size() * sizeof(R));
    H2D(d_lamx, lamx.data(), nxg * sizeof(R));
    H2D(d_d0, d0.data(), nxg * sizeof(R));
    const int nyp = is2d ? p.nb * p.B : 1;
    std::vector<R> lamy(nyp, (R)0);
    if (is2d)
      for (int k = 0; k < ny; ++k) lamy[k] = (R)(-2.0 * (1.0 - std::cos(2.0 * M_PI * k / ny)) / (pb.dy * pb.dy));
    if ((rc = alloc(&d_lamy, nyp))) return rc;
    H2D(d_lamy, lamy.data(), nyp * sizeof(R));
    {
      R* d_cx;
      if ((rc = alloc(&d_cx, nxg))) return rc;
      H2D(d_cx, cx.data(), nxg * sizeof(R));
      p.cx = d_cx;
      p.dctw = nullptr;
      if (dct_x) {
        C* d_w;
        if ((rc = alloc(&d_w, nxg))) return rc;
        H2D(d_w, dctw.data(), nxg * sizeof(C));
        p.dctw = d_w;
      }
    }
    p.ax = d_ax;
    p.ay = d_ay;
    p.lamx = d_lamx;
    p.lamy = d_lamy;
    lamy_base = d_lamy;
    p.d0_1d = d_d0;
    {
      auto t = twiddles<R>(nxg);
      if ((rc = alloc(&twx, nxg))) return rc;
      H2D(twx, t.data(), nxg * sizeof(C));
    }
    if (pp.fourstep) {
      auto t = twiddles<R>(256);
      if ((rc = alloc(&tw256, 256))) return rc;
      H2D(tw256, t.data(), 256 * sizeof(C));
    }
    if (is2d) {
      auto t = twiddles<R>(ny);
      if ((rc = alloc(&twy, ny))) return rc;
      H2D(twy, t.data(), ny * sizeof(C));
    }
    return PDHG_OK;
  }

  // ---------------- launch helpers ----------------
  std::vector<const void*> lds_done;
  template <typename K>
  int ensure_lds(K kern, size_t bytes) {
    const void* f = reinterpret_cast<const void*>(kern);
    for (const void* q : lds_done)
      if (q == f) return PDHG_OK;
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    lds_done.push_back(f);
    return PDHG_OK;
  }
  // one kernel on the context's stream; lds > 0: dynamic LDS bytes (the attribute is set once per kernel and
  // context), 0: a kernel with static LDS or none
  template <typename K, typename... A>
  int launch(K kern, dim3 grid, dim3 block, size_t lds, A&&... args) {
    if (lds > 0)
      if (int rc = ensure_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, std::forward<A>(args)...);
    HIP_TRY(hipGetLastError());
    return PDHG_OK;
  }
  // fn(IC<E>) for the context's egno in 1..Max (Max = 2 where no egno 3 kernel exists: 1-D, the fused residual)
  template <int Max, typename Fn>
  int with_egno(Fn&& fn) {
    static_assert(Max == 2 || Max == 3, "egno lift");
    if (pb.egno == 1) return fn(IC<1>{});
    if constexpr (Max == 3) {
      if (pb.egno == 3) return fn(IC<3>{});
    }
    return fn(IC<2>{});
  }

  // FFT policy dispatch: compile-time sizes for the hot power-of-two lengths (fp32),
  // runtime mixed-radix plan otherwise.
  template <typename Fn>
  int with_line_fft(const FFTPlan& pl, Fn&& fn) {
    if (pp.glb_line) return fn(FFTGlb{pl, 1});   // 1-D lines beyond LDS
    if constexpr (sizeof(R) == 8) {
      if (pp.ip_rows && &pl == &pp.ply) return fn(FFTIp<8192, 1024>{});   // the row kernels' 1024 threads (nt_row)
    }
    if constexpr (sizeof(R) == 4) {
      if (pl.pow2) {
        switch (pl.n) {
          case 256: return fn(FFTFx<256, 1>{});
          case 512: return fn(FFTFx<512, 1>{});
          case 1024: return fn(FFTFx<1024, 1>{});
          case 2048: return fn(FFTFx<2048, 1>{});
          case 4096: return fn(FFTFx<4096, 1>{});
          case 8192: return fn(FFTFx<8192, 1>{});
          default: break;
        }
      }
    }
    return fn(FFTRt{pl, 1});
  }
  // a KernelChoice as one switch value: every launcher below has one case, with one launch line, per instantiation
  static constexpr unsigned long long ck(int family, int n = 0, int a = 0, int b = 0, int c = 0) {
    using U = unsigned long long;
    return ((U)family << 56) | ((U)n << 40) | ((U)a << 28) | ((U)b << 14) | (U)c;
  }
  static unsigned long long ck(const KernelChoice& k) { return ck(k.family, k.n, k.a, k.b, k.c); }
  // a (family, shape) the stage's switch does not know is an error, never another kernel
  int no_kernel(const char* stage, const KernelChoice& k) {
    return fail(PDHG_ERR_STATE, "%s: no kernel for family %d with shape (%d, %d, %d, %d), %d threads", stage, k.family,
                k.n, k.a, k.b, k.c, k.threads);
  }

  template <typename Fn>
  int with_xt_fft(Fn&& fn) {
    const int nl = kp.B / 2;
    if constexpr (sizeof(R) == 4) {
      if (pp.plx.pow2) {
        const int n = pp.plx.n;
        if (n == 4096 && nl == 1) return fn(FFTFx<4096, 1>{});
        if (n == 2048 && nl == 2) return fn(FFTFx<2048, 2>{});
        if (n == 1024 && nl == 4) return fn(FFTFx<1024, 4>{});
        if (n == 512 && nl == 8) return fn(FFTFx<512, 8>{});
        if (n == 256 && nl == 8) return fn(FFTFx<256, 8>{});
      }
    }
    return fn(FFTRt{pp.plx, nl});
  }

  // ---------------- profiling ----------------
  struct ProfScope {
    Impl* im;
    ProfEntry* e = nullptr;
    ProfScope(Impl* i, const char* cls) : im(i) {
      if (!im->prof) return;
      e = &im->prof_ev[cls];
      if (e->used == e->ev.size()) {
        hipEvent_t a, b;
        hipEventCreate(&a);
        hipEventCreate(&b);
        e->ev.push_back({a, b});
      }
      hipEventRecord(e->ev[e->used].first, im->stream);
    }
    ~ProfScope() {
      if (!e) return;
      hipEventRecord(e->ev[e->used].second, im->stream);
      e->used++;
    }
  };

  // ---------------- primal: residual ----------------
  // the fused residual kernel over time rows [lo, hi) (launch_residual's fused branch); persistent grids, one
  // workgroup per CU (LDS)
  int launch_fused_residual(const KP<R>& p, int lo, int hi) {
    const KernelChoice& k = pp.res_fused;
    const dim3 g(std::min((pb.nx / std::max(k.a, 1)) * (hi - lo), n_cu));
    return with_egno<2>([&](auto eg) {
      constexpr int E = decltype(eg)::value;
      auto go = [&](auto kern) { return launch(kern, g, dim3(k.threads), k.lds, p, twy); };
      if constexpr (sizeof(R) == 4) switch (ck(k)) {
        case ck(RES_FUSED, 256, 8, 64): return go(k_res_fwdy_fused_2d<E, 256, 8, 64>);
        case ck(RES_FUSED, 512, 8, 128): return go(k_res_fwdy_fused_2d<E, 512, 8, 128>);
        case ck(RES_FUSED, 1024, 8, 256): return go(k_res_fwdy_fused_2d<E, 1024, 8, 256>);
        case ck(RES_FUSED, 2048, 8, 512): return go(k_res_fwdy_fused_2d<E, 2048, 8, 512>);
        case ck(RES_FUSED, 4096, 8, 1024): return go(k_res_fwdy_fused_2d<E, 4096, 8, 1024>);
        case ck(RES_FUSED, 4096, 8, 512): return go(k_res_fwdy_fused_2d<E, 4096, 8, 512>);
        case ck(RES_FUSED, 8192, 4, 1024): return go(k_res_fwdy_fused_2d<E, 8192, 4, 1024>);
        case ck(RES_FUSED, 8192, 4, 512): return go(k_res_fwdy_fused_2d<E, 8192, 4, 512>);
      } else switch (ck(k)) {
        case ck(RES_FUSED64, 8192, 2, 512): return go(k_res_fwdy_fused_2d<E, 8192, 2, 512, double>);
        case ck(RES_FUSED64, 2048, 4, 512): return go(k_res_fwdy_fused_2d<E, 2048, 4, 512, double>);
        case ck(RES_FUSED64, 4096, 4, 512): return go(k_res_fwdy_fused_2d<E, 4096, 4, 512, double>);
        case ck(RES_FUSED64, 4096, 4, 1024): return go(k_res_fwdy_fused_2d<E, 4096, 4, 1024, double>);
      }
      return no_kernel("res_fused", k);
    });
  }

  // C4's task-order residual spectrum (p.rspec) of time rows [lo, hi) into the blocked layout of `work`
  int launch_spec_to_blocked(const KP<R>& p, int lo, int hi) {
    const int RWt = sizeof(R) == 8 ? 2 : 4, XQ = pb.nx / RWt, NK = p.nb;   // 16-B elements: RWt reals
    if (XQ % 32 || NK % 64) return fail(PDHG_ERR_STATE, "task-order transpose needs nx/%d %% 32 == 0", RWt);
    KP<R> q = p;
    q.row_base = lo;
    return launch(k_res_fwdy_fused_transpose_2d<R>, dim3(NK / 64, XQ / 32, hi - lo), dim3(256), 0, q, XQ, NK);
  }

  // residual + forward y transform over time rows [lo, hi) (2-D).  The generic kernels only run the
  // whole window (lo = 0, hi = T).
  int launch_residual(KP<R> p, int lo, int hi) {
    if (hi <= lo) return PDHG_OK;
    const KernelChoice& k = pp.res;
    const bool fused = pp.res_fused.family && res_valid && (slab || (lo == 0 && hi == pb.T));
    if (!fused && k.family == RES_GENERIC && (lo != 0 || hi != pb.T))
      return fail(PDHG_ERR_UNSUPPORTED, "row-range residual needs the fast row kernels");
    ProfScope ps(this, "residual");
    p.row_base = lo;
    p.row_cnt = hi - lo;
    if (fused) {
      // C4 (half-real x blocks, B = 1): the fused residual stores its spectrum in task order over the R rows it was
      // formed from (full 128-B lines instead of 16-B chunks of the blocked layout), and k_spec_to_blocked_2d
      // transposes it into the x kernel's blocked layout
      if (pp.to_c4) p.rspec = p.res;
      // the task-order spectrum is stored over the R rows it was formed from (p.rspec == p.res): once the launch
      // that ends the window has run, R is gone until the next fused dual sweep forms it again
      if (p.rspec != nullptr && p.rspec == p.res && hi == pb.T) res_valid = false;
      if (int rc = launch_fused_residual(p, lo, hi)) return rc;
      return pp.to_c4 ? launch_spec_to_blocked(p, lo, hi) : (int)PDHG_OK;
    }
    return with_egno<3>([&](auto eg) {
      constexpr int E = decltype(eg)::value;
      if (k.family == RES_GENERIC)
        return with_line_fft(pp.ply, [&](auto f) {
          using F = decltype(f);
          if (k.b == 256) return launch(k_res_fwdy_2d<R, E, F, 256>, dim3(pp.gx1), dim3(k.threads), k.lds, p, f, twy);
          return launch(k_res_fwdy_2d<R, E, F, 1024>, dim3(pp.gx1), dim3(k.threads), k.lds, p, f, twy);
        });
      auto go = [&](auto kern) {
        return launch(kern, dim3((pb.nx / std::max(k.a, 1)) * (hi - lo)), dim3(k.threads), k.lds, p, twy);
      };
      if constexpr (sizeof(R) == 4) switch (ck(k)) {
        case ck(RES_FAST, 256, 8, 64): return go(k_res_fwdy_fast_2d<E, 256, 8, 64>);
        case ck(RES_FAST, 512, 8, 128): return go(k_res_fwdy_fast_2d<E, 512, 8, 128>);
        case ck(RES_FAST, 1024, 8, 256): return go(k_res_fwdy_fast_2d<E, 1024, 8, 256>);
        case ck(RES_FAST, 2048, 8, 512): return go(k_res_fwdy_fast_2d<E, 2048, 8, 512>);
        case ck(RES_FAST, 2048, 4, 256): return go(k_res_fwdy_fast_2d<E, 2048, 4, 256>);
        case ck(RES_FAST, 4096, 8, 1024): return go(k_res_fwdy_fast_2d<E, 4096, 8, 1024>);
        case ck(RES_FAST, 4096, 4, 512): return go(k_res_fwdy_fast_2d<E, 4096, 4, 512>);
        case ck(RES_FAST, 8192, 4, 1024): return go(k_res_fwdy_fast_2d<E, 8192, 4, 1024>);
      } else switch (ck(k)) {
        case ck(RES_FAST64, 4096, 4, 512): return go(k_res_fwdy_fast_2d<E, 4096, 4, 512, double>);
        case ck(RES_FAST64, 2048, 4, 256): return go(k_res_fwdy_fast_2d<E, 2048, 4, 256, double>);
        case ck(RES_FAST64, 2048, 4, 512): return go(k_res_fwdy_fast_2d<E, 2048, 4, 512, double>);
      }
      return no_kernel("res", k);
    });
  }

  // ---------------- primal: x transform + t-solve ----------------
  int launch_thomas_1d(const KP<R>& p) {
    if (!pp.thomas_chunk) return launch(k_thomas_1d<R>, dim3((pb.nx + 255) / 256), dim3(256), 0, p);
    if constexpr (sizeof(R) == 4) {   // one 32-row chunk per wave
      const int NP = (pb.T + 31) / 32;
      return launch(k_thomas_chunk_1d<32, 1, R>, dim3((pb.nx + 63) / 64), dim3(64 * NP), 0, p);
    } else {                           // one 16-row chunk per half-wave (32 modes per workgroup)
      const int NP = (pb.T + 15) / 16;
      return launch(k_thomas_chunk_1d<16, 2, R>, dim3((pb.nx + 31) / 32), dim3(64 * ((NP + 1) / 2)), 0, p);
    }
  }

  // x transform + Thomas in t + inverse x transform of the spectral blocks in p.work (p.nx-point lines,
  // p.nb blocks); p.xt_phase selects the sweeps (t-slab)
  int launch_precond(const KP<R>& p, int nblk = -1) {   // nblk: blocks [p.b0, p.b0 + nblk) (default: all)
    if (nblk < 0) nblk = p.nb - p.b0;
    ProfScope ps(this, "precond");
    const KernelChoice& k = pp.xt_one_row.family ? pp.xt_one_row : pp.xt;   // a one-row window has no t carries
    auto go = [&](auto kern) { return launch(kern, dim3(nblk), dim3(k.threads), k.lds, p, twx); };
    if (k.family == XT_GENERIC)
      return with_xt_fft([&](auto f) {
        return launch(k_precond_xt_2d<R, decltype(f)>, dim3(nblk), dim3(k.threads), k.lds, p, f, twx);
      });
    if constexpr (sizeof(R) == 4) switch (ck(k)) {
      case ck(XT1_F32, 4096, 1, 512): return go(k_precond_x_t1_2d<4096, 1, 512>);
      case ck(XT1_F32, 2048, 2, 512): return go(k_precond_x_t1_2d<2048, 2, 512>);
      case ck(XT1_F32, 1024, 4, 512): return go(k_precond_x_t1_2d<1024, 4, 512>);
      case ck(XT1_F32, 512, 8, 512): return go(k_precond_x_t1_2d<512, 8, 512>);
      case ck(XT_DMA_HR, 4096): return go(k_precond_xt_dma_2d<4096, true>);
      case ck(XT_DMA, 4096): return go(k_precond_xt_dma_2d<4096>);
      case ck(XT_BATCH, 4096, 1, 2, 0): return go(k_precond_xt_batch_2d<4096, 1, 2, 0, 512>);
      case ck(XT_BATCH, 4096, 1, 4, 2): return go(k_precond_xt_batch_2d<4096, 1, 4, 2>);
      case ck(XT_BATCH, 4096, 1, 4, 0): return go(k_precond_xt_batch_2d<4096, 1>);
      case ck(XT_BATCH, 2048, 2, 4, 0): return go(k_precond_xt_batch_2d<2048, 2>);
      case ck(XT_BATCH, 1024, 4, 4, 0): return go(k_precond_xt_batch_2d<1024, 4>);
      case ck(XT_BATCH, 512, 8, 4, 0): return go(k_precond_xt_batch_2d<512, 8>);
      case ck(XT_WS, 4096, 1, 1): return go(k_precond_xt_ws_2d<4096, 1, true>);
      case ck(XT_WS, 4096, 1, 0): return go(k_precond_xt_ws_2d<4096, 1>);
      case ck(XT_WS, 2048, 2, 0): return go(k_precond_xt_ws_2d<2048, 2>);
      case ck(XT_WS, 1024, 4, 0): return go(k_precond_xt_ws_2d<1024, 4>);
      case ck(XT_WS, 512, 8, 0): return go(k_precond_xt_ws_2d<512, 8>);
      case ck(XT_FAST, 4096, 1, 512): return go(k_precond_xt_fast_2d<4096, 1, 512>);
      case ck(XT_FAST, 2048, 2, 512): return go(k_precond_xt_fast_2d<2048, 2, 512>);
      case ck(XT_FAST, 1024, 4, 512): return go(k_precond_xt_fast_2d<1024, 4, 512>);
      case ck(XT_FAST, 512, 8, 512): return go(k_precond_xt_fast_2d<512, 8, 512>);
    } else switch (ck(k)) {   // XT_F64's c: BPR 1 | TC 2 | DMA 4
      case ck(XT1_F64_G16, 4096, 1, 512): return go(k_precond_x_t1_2d<4096, 1, 512, double, true>);
      case ck(XT1_F64, 4096, 1, 512): return go(k_precond_x_t1_2d<4096, 1, 512, double>);
      case ck(XT1_F64_G16, 2048, 1, 256): return go(k_precond_x_t1_2d<2048, 1, 256, double, true>);
      case ck(XT1_F64, 2048, 1, 256): return go(k_precond_x_t1_2d<2048, 1, 256, double>);
      case ck(XT1_F64, 1024, 2, 512): return go(k_precond_x_t1_2d<1024, 2, 512, double>);
      case ck(XT1_F64, 512, 4, 512): return go(k_precond_x_t1_2d<512, 4, 512, double>);
      case ck(XT_F64, 4096, 512, 1, 0): return go(k_precond_xt_f64_2d<4096, 512, true>);
      case ck(XT_F64, 1024, 256, 0, 1): return go(k_precond_xt_f64_2d<1024, 256, false, true>);
      case ck(XT_F64, 512, 128, 0, 1): return go(k_precond_xt_f64_2d<512, 128, false, true>);
      case ck(XT_F64, 2048, 256, 0, 0): return go(k_precond_xt_f64_2d<2048, 256, false, false>);
      case ck(XT_F64, 2048, 256, 0, 1): return go(k_precond_xt_f64_2d<2048, 256, false, true>);
      case ck(XT_F64, 2048, 1024, 0, 1): return go(k_precond_xt_f64_2d<2048, 1024, false, true>);
      case ck(XT_F64, 2048, 512, 0, 1): return go(k_precond_xt_f64_2d<2048, 512, false, true>);
      case ck(XT_F64, 4096, 512, 0, 1 | 2 | 4): return go(k_precond_xt_f64_2d<4096, 512, false, true, true, true>);
      case ck(XT_F64, 4096, 512, 0, 1 | 4): return go(k_precond_xt_f64_2d<4096, 512, false, true, false, true>);
      case ck(XT_F64, 4096, 512, 0, 1 | 2): return go(k_precond_xt_f64_2d<4096, 512, false, true, true>);
      case ck(XT_F64, 4096, 512, 0, 1): return go(k_precond_xt_f64_2d<4096, 512, false, true>);
      case ck(XT_F64, 4096, 512, 0, 2): return go(k_precond_xt_f64_2d<4096, 512, false, false, true>);
      case ck(XT_F64, 4096, 512, 0, 0): return go(k_precond_xt_f64_2d<4096, 512>);
    }
    return no_kernel(pp.xt_one_row.family ? "xt_one_row" : "xt", k);
  }

  // ---------------- primal: update ----------------
  // inverse transforms + phi / phi_bar update of a 2-D window; returns its partial-row count through upd_rows
  int launch_update_2d(const KP<R>& p, int& upd_rows) {
    ProfScope ps(this, "update");
    const KernelChoice& k = pp.upd;
    auto run = [&](auto kern, dim3 g, auto... fft) {   // the mixed kernels take the double phi pair (px) last
      if constexpr (kMixed) return launch(kern, g, dim3(k.threads), k.lds, p, fft..., twy, px);
      else return launch(kern, g, dim3(k.threads), k.lds, p, fft..., twy);
    };
    if (k.family == (kMixed ? UPD_GENERIC_MIXED : UPD_GENERIC)) {
      upd_rows = pp.gx4 * pp.g4;
      return with_line_fft(pp.ply, [&](auto f) {
        using F = decltype(f);
        if constexpr (kMixed) {
          if (k.b == 256) return run(k_invy_update_mixed_2d<F, 256>, dim3(pp.gx4), f);
          return run(k_invy_update_mixed_2d<F, 1024>, dim3(pp.gx4), f);
        } else {
          if (k.b == 256) return run(k_invy_update_2d<R, F, 256>, dim3(pp.gx4), f);
          return run(k_invy_update_2d<R, F, 1024>, dim3(pp.gx4), f);
        }
      });
    }
    upd_rows = pp.g_fast_upd;
    auto go = [&](auto kern) { return run(kern, dim3(pp.g_fast_upd)); };
    if constexpr (kMixed) switch (ck(k)) {   // the fp32 shapes with double phi rows; one PF (kMixedUpdPF) at 512 threads
      case ck(UPD_FAST_MIXED, 256, 8, 64): return go(k_invy_update_fast_mixed_2d<256, 8, 64>);
      case ck(UPD_FAST_MIXED, 512, 8, 128): return go(k_invy_update_fast_mixed_2d<512, 8, 128>);
      case ck(UPD_FAST_MIXED, 1024, 8, 256): return go(k_invy_update_fast_mixed_2d<1024, 8, 256>);
      case ck(UPD_FAST_MIXED, 2048, 8, 512): return go(k_invy_update_fast_mixed_2d<2048, 8, 512>);
      case ck(UPD_FAST_MIXED, 2048, 4, 256): return go(k_invy_update_fast_mixed_2d<2048, 4, 256>);
      case ck(UPD_FAST_MIXED, 4096, 8, 1024): return go(k_invy_update_fast_mixed_2d<4096, 8, 1024>);
      case ck(UPD_FAST_MIXED, 4096, 8, 512, kMixedUpdPF): return go(k_invy_update_fast_mixed_2d<4096, 8, 512, kMixedUpdPF>);
      case ck(UPD_FAST_MIXED, 4096, 4, 512): return go(k_invy_update_fast_mixed_2d<4096, 4, 512>);
      case ck(UPD_FAST_MIXED, 8192, 4, 1024): return go(k_invy_update_fast_mixed_2d<8192, 4, 1024>);
    } else if constexpr (sizeof(R) == 4) switch (ck(k)) {
      case ck(UPD_FAST, 256, 8, 64): return go(k_invy_update_fast_2d<256, 8, 64>);
      case ck(UPD_FAST, 512, 8, 128): return go(k_invy_update_fast_2d<512, 8, 128>);
      case ck(UPD_FAST, 1024, 8, 256): return go(k_invy_update_fast_2d<1024, 8, 256>);
      case ck(UPD_FAST, 2048, 8, 512): return go(k_invy_update_fast_2d<2048, 8, 512>);
      case ck(UPD_FAST, 2048, 4, 256): return go(k_invy_update_fast_2d<2048, 4, 256>);
      case ck(UPD_FAST, 4096, 8, 1024): return go(k_invy_update_fast_2d<4096, 8, 1024>);
      case ck(UPD_FAST, 4096, 8, 512, 1): return go(k_invy_update_fast_2d<4096, 8, 512, 1>);
      case ck(UPD_FAST, 4096, 8, 512, 2): return go(k_invy_update_fast_2d<4096, 8, 512, 2>);
      case ck(UPD_FAST, 4096, 8, 512, 3): return go(k_invy_update_fast_2d<4096, 8, 512, 3>);
      case ck(UPD_FAST, 4096, 8, 512, 4): return go(k_invy_update_fast_2d<4096, 8, 512, 4>);
      case ck(UPD_FAST, 4096, 4, 512): return go(k_invy_update_fast_2d<4096, 4, 512>);
      case ck(UPD_FAST, 8192, 4, 1024): return go(k_invy_update_fast_2d<8192, 4, 1024>);
    } else switch (ck(k)) {
      case ck(UPD_T1_G16, 2048, 4, 256, 2): return go(k_invy_update_fast_2d<2048, 4, 256, 2, double, true>);
      case ck(UPD_T1_G16, 2048, 4, 256, 4): return go(k_invy_update_fast_2d<2048, 4, 256, 4, double, true>);
      case ck(UPD_PAIR64, 4096, 0, 512, 2): return go(k_invy_update_pair_2d<4096, 512, 2>);
      case ck(UPD_PAIR64, 4096, 0, 512, 3): return go(k_invy_update_pair_2d<4096, 512, 3>);
      case ck(UPD_PAIR64, 4096, 0, 512, 4): return go(k_invy_update_pair_2d<4096, 512, 4>);
      case ck(UPD_PAIR64, 2048, 0, 512, 2): return go(k_invy_update_pair_2d<2048, 512, 2>);
      case ck(UPD_PAIR64, 2048, 0, 512, 3): return go(k_invy_update_pair_2d<2048, 512, 3>);
      case ck(UPD_PAIR64, 2048, 0, 512, 4): return go(k_invy_update_pair_2d<2048, 512, 4>);
      case ck(UPD_FAST64, 4096, 4, 512, 4): return go(k_invy_update_fast_2d<4096, 4, 512, 4, double>);
      case ck(UPD_FAST64, 2048, 4, 512, 4): return go(k_invy_update_fast_2d<2048, 4, 512, 4, double>);
      case ck(UPD_8192, 8192, 2, 512, 2): return go(k_invy_update_fast_2d<8192, 2, 512, 2, double>);
    }
    return no_kernel("upd", k);
  }

  // stages: 1 residual (+ forward y transform), 2 x transform + Thomas (sweeps per xt_phase: 0 both,
  // 1 forward, 2 backward), 4 inverse transforms + phi/phi_bar update + primal sums.  sums_out != null
  // (t-slab mode): the primal sums go to that vector (all-reduced by the caller) instead of ctrl.
  int launch_primal(R tau, int stages = 7, int xt_phase = 0, double* sums_out = nullptr) {
    KP<R> p = kp;
    p.tau = tau;
    p.xt_phase = xt_phase;
    const int T = pb.T;
    int rc;
    if (pb.ndim == 2) {
      if ((stages & 1) && (rc = launch_residual(p, 0, T))) return rc;
      if ((stages & 2) && (rc = launch_precond(p))) return rc;
      if (!(stages & 4)) return PDHG_OK;
      // speculative schedule: the update's sums go to their own rows and k_finalize_dual_outer reduces them (the
      // same rows in the same order as k_finalize_primal), one launch fewer
      const bool prim_merge = spec && pp.fin_merge && !pp.dual_multi && !sums_out;
      if (prim_merge) p.partials = prim_partials;
      int upd_rows = 0;
      if ((rc = launch_update_2d(p, upd_rows))) return rc;
      if (sums_out)
        return launch(k_reduce_vec, dim3(1), dim3(1024), 0, p.partials, upd_rows, 3, kp.j0 == 0 ? row0_sq : 0.0,
                      sums_out);
      if (prim_merge) {
        prim_merged_rows = upd_rows;
        return PDHG_OK;
      }
      return launch(k_finalize_primal, dim3(1), dim3(1024), 0, p.partials, upd_rows, 1, p.ctrl);
    }
    if constexpr (kMixed) return fail(PDHG_ERR_STATE, "mixed context is 2-D only");
    if (pp.fourstep) return launch_fourstep_1d(p);
    {
      ProfScope ps(this, "residual");
      rc = with_line_fft(pp.plx, [&](auto f) {
        using F = decltype(f);
        return with_egno<2>([&](auto eg) {
          return launch(k_res_fwdx_1d<R, decltype(eg)::value, F>, dim3(pp.gx1), dim3(pp.nt1d), pp.lds_res, p, f, twx);
        });
      });
      if (rc) return rc;
    }
    {
      ProfScope ps(this, "precond");
      if ((rc = launch_thomas_1d(p))) return rc;
    }
    {
      ProfScope ps(this, "update");
      rc = with_line_fft(pp.plx, [&](auto f) {
        return launch(k_invx_update_1d<R, decltype(f)>, dim3(pp.gx4), dim3(pp.nt1d), pp.lds_res, p, f, twx);
      });
      if (rc) return rc;
    }
    return launch(k_finalize_primal, dim3(1), dim3(1024), 0, p.partials, pp.gx4, 1, p.ctrl);
  }

  // ---------------- primal: 1-D four-step forms (nx = 65536) ----------------
  // residual + DHT, Thomas, inverse DHT + update; the 16 x 4096 split, the wide-tile stages (fp32) or 16-column tiles
  int launch_fourstep_1d(const KP<R>& p) {
    if (pp.fs16) return launch_fs16_1d(p);
    if constexpr (sizeof(R) == 4) {
      const int npairs = (pb.T + 1) / 2;
      float2* Y = reinterpret_cast<float2*>(p.gscr);
      const bool wide = pp.fs_wide;   // kernels_fs_wide.hpp: 4 + 5 workgroups per row pair (else 16 + 9)
      // 16-column tiles: 1024 threads (16 waves) so the load / unpack loops keep more rows in flight
      const size_t lds1 = wide ? (size_t)(64 * kFwLine + twlds_size(256)) * sizeof(C) : (size_t)2 * 256 * 16 * sizeof(C);
      const size_t lds2 = wide ? lds1 : 2 * lds1;
      const dim3 g1(wide ? 4 : 16, npairs), g2(wide ? 5 : 9, npairs), b(1024);
      int rc;
      {
        ProfScope ps(this, "residual");
        rc = with_egno<2>([&](auto eg) {
          constexpr int E = decltype(eg)::value;
          if (wide) return launch(k_fs1w_1d<0, E>, g1, b, lds1, p, tw256, twx, Y);
          return launch(k_fs1_1d<0, E>, g1, b, lds1, p, tw256, twx, Y);
        });
        if (rc) return rc;
        if ((rc = wide ? launch(k_fs2w_1d<0>, g2, b, lds2, p, tw256, Y) : launch(k_fs2_1d<0>, g2, b, lds2, p, tw256, Y)))
          return rc;
      }
      {
        ProfScope ps(this, "precond");
        if ((rc = launch_thomas_1d(p))) return rc;
      }
      {
        ProfScope ps(this, "update");
        if ((rc = wide ? launch(k_fs1w_1d<1, 1>, g1, b, lds1, p, tw256, twx, Y)
                       : launch(k_fs1_1d<1, 1>, g1, b, lds1, p, tw256, twx, Y)))
          return rc;
        if ((rc = wide ? launch(k_fs2w_1d<1>, g2, b, lds2, p, tw256, Y) : launch(k_fs2_1d<1>, g2, b, lds2, p, tw256, Y)))
          return rc;
      }
      return launch(k_finalize_primal, dim3(1), dim3(1024), 0, p.partials, (int)g2.x * npairs, 1, p.ctrl);
    }
    return PDHG_OK;
  }

  // the same as 16 x 4096 with a chunk-major spectrum (kernels_fs16.hpp): 16 + 8 workgroups per row pair
  // forward, 8 + 8 inverse
  int launch_fs16_1d(const KP<R>& p) {
    const int npairs = (pb.T + 1) / 2;
    const size_t ldsb = (size_t)(2 * kF16Line + twlds_size(kF16N2)) * sizeof(C);
    C* Y = reinterpret_cast<C*>(p.gscr);
    int rc;
    {
      ProfScope ps(this, "residual");
      const dim3 ga(kF16N2 / 256, npairs);
      if (pp.fuse_res && res_valid)   // the residual rows the last dual sweep formed (k_dual_1d_fr)
        rc = launch(k_f16a_fwd_fused_1d<R>, ga, dim3(256), 0, p, twx, Y, pp.jchunk_1d);
      else
        rc = with_egno<2>([&](auto eg) {
          constexpr int E = decltype(eg)::value;
          if (pp.f16_group == 4) return launch(k_f16a_fwd_1d<E, 4, R>, ga, dim3(256), 0, p, twx, Y);
          if (pp.f16_group == 8) return launch(k_f16a_fwd_1d<E, 8, R>, ga, dim3(256), 0, p, twx, Y);
          return launch(k_f16a_fwd_1d<E, 16, R>, ga, dim3(256), 0, p, twx, Y);
        });
      if (rc) return rc;
      if ((rc = launch(k_f16b_fwd_1d<R>, dim3(8, npairs), dim3(512), ldsb, p, twx, Y))) return rc;
    }
    {
      ProfScope ps(this, "precond");
      if ((rc = launch_thomas_1d(p))) return rc;
    }
    {
      ProfScope ps(this, "update");
      if ((rc = launch(k_f16b_inv_1d<R>, dim3(8, npairs), dim3(512), ldsb, p, twx, Y))) return rc;
      if ((rc = launch(k_f16a_inv_1d<R>, dim3(kF16N2 / 2 / 256, npairs), dim3(256), 0, p, twx, Y))) return rc;
    }
    return launch(k_finalize_primal, dim3(1), dim3(1024), 0, p.partials, 8 * npairs, 1, p.ctrl);
  }

  // ---------------- dual ----------------
  // the row-per-thread / LDS-row dual over time rows [lo, hi); its partials start at block row zbase
  int launch_dual_fast(const KP<R>& p, int lo = 0, int hi = -1, int zbase = 0) {
    if (hi < 0) hi = pb.T;
    if (hi <= lo) return PDHG_OK;
    const dim3 g(pp.gxd, pp.gyd, (hi - lo + pp.jchunk_d - 1) / pp.jchunk_d);
    // the sweep that also forms the next residual: in place, one time chunk, the whole window (a t-slab: its rows)
    res_valid = pp.dual_fused.family && p.inplace && g.z == 1 && (slab || (lo == 0 && hi == pb.T));
    const KernelChoice& k = res_valid ? pp.dual_fused : pp.dual;
    return with_egno<3>([&](auto eg) {
      constexpr int E = decltype(eg)::value;
      auto go = [&](auto kern) {
        if constexpr (kMixed) return launch(kern, g, dim3(k.threads), 0, p, pp.jchunk_d, lo, hi, zbase, px);
        else return launch(kern, g, dim3(k.threads), 0, p, pp.jchunk_d, lo, hi, zbase);
      };
      if constexpr (kMixed) switch (ck(k)) {   // row-per-thread only (plan_paths: dual_rx = 0, no fused residual)
        case ck(DUAL_ROW_MIXED, 0, 1): return go(k_dual_fast_mixed_2d<E, 1>);
        case ck(DUAL_ROW_MIXED, 0, 0): return go(k_dual_fast_mixed_2d<E>);
      } else if constexpr (sizeof(R) == 4) switch (ck(k)) {
        case ck(DUAL_LDS_FR, 0, 8, 4):
          if constexpr (E != 3) return go(k_dual_lds_2d<E, 8, true>);
          break;
        case ck(DUAL_LDS, 0, 4, 4): return go(k_dual_lds_2d<E, 4>);
        case ck(DUAL_LDS, 0, 8, 4): return go(k_dual_lds_2d<E, 8>);
        case ck(DUAL_LDS, 0, 16, 4): return go(k_dual_lds_2d<E, 16>);
        case ck(DUAL_ROW, 0, 1): return go(k_dual_fast_2d<E, float, 1>);
        case ck(DUAL_ROW, 0, 0): return go(k_dual_fast_2d<E>);
      } else switch (ck(k)) {
        case ck(DUAL_LDS_FR, 0, 8, 2):
          if constexpr (E != 3) return go(k_dual_lds_2d<E, 8, true, double, 2>);
          break;
        case ck(DUAL_LDS, 0, 8, 2): return go(k_dual_lds_2d<E, 8, false, double, 2>);
        case ck(DUAL_LDS, 0, 8, 4): return go(k_dual_lds_2d<E, 8, false, double>);
        case ck(DUAL_ROW, 0, 2): return go(k_dual_fast_2d<E, double, 2>);
        case ck(DUAL_ROW, 0, 1): return go(k_dual_fast_2d<E, double, 1>);
        case ck(DUAL_ROW, 0, 0): return go(k_dual_fast_2d<E, double>);
      }
      return no_kernel(res_valid ? "dual_fused" : "dual", k);
    });
  }

  // the dual loop in chunks of kMultiSub sub-iterations + a final pass when the exit falls inside a chunk
  // (kernels_dual_multi.hpp); k in [2, kDualMultiMax].  slo0 = 1: the head form's rest after sub-iteration 0
  int launch_dual_multi(const KP<R>& p, int k, double eps, int slo0 = 0) {
    // head form: runs of 4 x rows per workgroup (its passes mostly return at once; fewer workgroups to retire)
    const int xrun = (slo0 > 0 && pb.nx % pp.head_xrun == 0) ? pp.head_xrun : 1;
    const int gx = (pb.nx + xrun - 1) / xrun;
    const dim3 g(gx, pp.gyd, pp.gzd), b(pp.NTd);
    const int rows = gx * pp.gyd * pp.gzd;
    constexpr int NS = kMultiSub;
    return with_egno<3>([&](auto eg) {
      constexpr int E = decltype(eg)::value;
      int rc;
      // one chunk (FINAL false) or final pass of the context's phi type
      auto pass = [&](auto fin, int slo) {
        constexpr bool FIN = decltype(fin)::value != 0;
        if constexpr (kMixed)
          return launch(k_dual_multi_mixed_2d<E, NS, FIN>, g, b, 0, p, slo, k, rows, pp.jchunk_d, 0, pb.T, 0, xrun, px);
        else
          return launch(k_dual_multi_2d<E, R, NS, FIN>, g, b, 0, p, slo, k, rows, pp.jchunk_d, 0, pb.T, 0, xrun);
      };
      for (int slo = slo0; slo < k; slo += NS) {
        if ((rc = pass(IC<0>{}, slo))) return rc;
        if ((rc = launch(k_finalize_dual_multi, dim3(1), dim3(1024), 0, p.partials, rows, std::min(NS, k - slo), slo, k,
                         pp.na, pp.n_dead, eps, p.ctrl)))
          return rc;
      }
      return pass(IC<1>{}, 0);
    });
  }

  // one sub-iteration's sweep of the whole window; returns its partial-row count through nrows
  int launch_dual_sweep(const KP<R>& p, int& nrows) {
    ProfScope ps(this, "dual");
    const dim3 g(pp.gx5, pp.g5);
    nrows = pp.gx5 * pp.g5;
    if (pb.ndim == 2 && pp.dual.family != (kMixed ? DUAL_POINT_MIXED : DUAL_POINT)) {
      nrows = pp.gxd * pp.gyd * pp.gzd;
      return launch_dual_fast(p);
    }
    if constexpr (kMixed) {
      if (pb.ndim != 2) return fail(PDHG_ERR_STATE, "mixed context is 2-D only");
      return with_egno<3>([&](auto eg) { return launch(k_dual_mixed_2d<decltype(eg)::value>, g, dim3(256), 0, p, px); });
    }
    if (pb.ndim == 2)
      return with_egno<3>([&](auto eg) { return launch(k_dual_2d<R, decltype(eg)::value>, g, dim3(256), 0, p); });
    if (pp.fuse_res && p.inplace) {   // the sweep also forms the next residual (k_dual_1d_fr)
      nrows = (pb.nx / 256) * pp.gz_1d;
      const int rc = with_egno<2>([&](auto eg) {
        return launch(k_dual_1d_fr<R, decltype(eg)::value>, dim3(pb.nx / 256, pp.gz_1d), dim3(256), 0, p, pp.jchunk_1d);
      });
      res_valid = true;
      return rc;
    }
    res_valid = false;
    return with_egno<2>([&](auto eg) { return launch(k_dual_1d<R, decltype(eg)::value>, g, dim3(256), 0, p); });
  }

  int launch_dual(R sigma, double eps, int k) {
    KP<R> p = kp;
    p.sigma = sigma;
    p.inplace = (k <= 1) ? 1 : 0;
    if (!p.inplace && !pp.two_sets)
      return fail(PDHG_ERR_STATE, "rho_alp_iters=%d needs a context created with rho_alp_iters > 1", k);
    if (pp.dual_multi && k > 1 && k <= kDualMultiMax) {
      ProfScope ps(this, "dual");
      return launch_dual_multi(p, k, eps);
    }
    // head form: sub-iteration 0 below, then the chunks from sub-iteration 1
    const bool head = pp.dual_head && k > 1 && k <= kDualMultiMax;
    const dim3 one(1), b(1024);
    int rc;
    for (int s = 0; s < (head ? 1 : k); ++s) {
      p.sub = s;
      int nrows_d = 0;
      if ((rc = launch_dual_sweep(p, nrows_d))) return rc;
      const double* rows = p.partials;
      int nrows = nrows_d;
      if (nrows_d > 2 * kFoldRows * 16) {   // one workgroup reading ~1 MiB of rows took 45-65 us at C1 / C3
        const int chunk = (nrows_d + kFoldRows - 1) / kFoldRows;
        if (pp.fold_fin) {   // fold + finalize in one launch (the last workgroup finalizes)
          if ((rc = launch(k_fold_finalize_dual, dim3(kFoldRows), b, 0, p.partials, nrows_d, chunk, fold_out, pp.na,
                           pp.n_dead, eps, s, p.ctrl)))
            return rc;
          continue;
        }
        if ((rc = launch(k_fold_partials, dim3(kFoldRows), b, 0, p.partials, nrows_d, 3 + 3 * pp.na, chunk, fold_out,
                         p.ctrl)))
          return rc;
        rows = fold_out;
        nrows = kFoldRows;
      }
      if (head && spec && s == 0 && k > 1 && pp.k1_outer && !pp.dual_multi && pp.fin_merge) {
        // the speculative iteration's dual and outer finalizes in one launch; launch_outer then launches nothing
        rc = launch(k_finalize_dual_outer, one, b, 0, prim_partials, prim_merged_rows, rows, nrows, pp.na, pp.n_dead,
                    eps, 1, stop_conv, stop_nan, p.ctrl);
        prim_merged_rows = 0;
        outer_merged = true;
      } else {
        rc = launch(k_finalize_dual, one, b, 0, rows, nrows, pp.na, pp.n_dead, eps, s, p.ctrl, (head && spec) ? 1 : 0);
      }
      if (rc) return rc;
    }
    if (head && !spec) return launch_dual_tail(sigma, eps, k);   // spec: only when sub-iteration 0 did not exit
    return PDHG_OK;
  }
  // the head form's rest of the dual loop: chunk passes from sub-iteration 1 (+ their finalizes, the final pass)
  int launch_dual_tail(R sigma, double eps, int k) {
    KP<R> p = kp;
    p.sigma = sigma;
    p.inplace = 0;
    ProfScope ps(this, "dual");
    return launch_dual_multi(p, k, eps, 1);
  }

  int launch_outer(double eps, int k) {
    if (outer_merged) {   // k_finalize_dual_outer ran it (speculative schedule)
      outer_merged = false;
      return PDHG_OK;
    }
    int rows = 0;
    // the chunked dual loop keeps no sub-iteration-0 outer sums (its tables hold 2 + 2 na sums), so only the
    // per-sub-iteration kernels skip the outer pass after a one-sub-iteration loop
    const int k1_skip = (pp.k1_outer && !pp.dual_multi) ? 1 : 0;
    if (k > 1) {
      // spec: the iteration reaches here only after a one-sub-iteration loop, whose outer-sum pass returns at once
      if (!spec)
        if (int rc = launch(k_outer_sums<R>, dim3(pp.g_outer), dim3(256), 0, kp, (size_t)pb.T * plane(), k1_skip))
          return rc;
      rows = pp.g_outer;
    }
    return launch(k_finalize_outer, dim3(1), dim3(1024), 0, kp.partials, rows, pp.na, eps, k > 1 ? 1 : 0, stop_conv,
                  stop_nan, kp.ctrl, k > 1 ? k1_skip : 0);
  }
  int reset_ctrl() {
    // zero everything except `cur` (which buffer set holds the state)
    Ctrl h{};
    int cur = 0;
    HIP_TRY(hipMemcpyAsync(&cur, &kp.ctrl->cur, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    h.cur = cur;
    h.row0_sq = row0_sq;
    HIP_TRY(hipMemcpyAsync(kp.ctrl, &h, sizeof(Ctrl), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PDHG_OK;
  }

  int read_ctrl(Ctrl& h) {
    HIP_TRY(hipMemcpyAsync(&h, kp.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PDHG_OK;
  }

  // ---------------- iteration chunks replayed from a HIP graph ----------------
  // The launch chain of `window` outer iterations (primal, <= k dual sub-iterations, outer tests: 8-12
  // kernels each) is captured once per (tau, sigma, eps, k) and replayed with one hipGraphLaunch, so the
  // host issues one call per window instead of ~10 per iteration -- the marching default's T = 1 windows
  // and small grids are launch-bound (utils_pdhg_solver.py:166-212 runs up to N_maxiter iterations per
  // window).  The device-side stop flags (Ctrl) make the kernels after convergence no-ops, exactly as in the
  // eager loop, so a replayed chunk needs no host decision.  Captured only with the fused residual valid
  // (or not in use) so every captured primal is the steady-state one; off while profiling (per-launch
  // events) and with PDHG_GRAPH=0.
  hipGraphExec_t gexec = nullptr;
  double g_tau = 0, g_sigma = 0, g_eps = 0;
  int g_k = 0, g_window = 0, g_stop = -1, g_spec = -1;
  bool use_graph = true;
  bool warm = false;   // one eager iteration ran (kernel attributes set outside any capture)
  void drop_graph() {
    if (gexec) hipGraphExecDestroy(gexec);
    gexec = nullptr;
  }
  int launch_iteration(double tau, double sigma, double eps, int k) {
    int rc;
    if ((rc = launch_primal((R)tau))) return rc;
    if ((rc = launch_dual((R)sigma, eps, k))) return rc;
    return launch_outer(eps, k);
  }
  int ensure_graph(double tau, double sigma, double eps, int k, int window) {
    const int stop = stop_conv * 2 + stop_nan;   // kernel arguments of k_finalize_outer
    if (gexec && g_tau == tau && g_sigma == sigma && g_eps == eps && g_k == k && g_window == window && g_stop == stop &&
        g_spec == (int)spec)
      return PDHG_OK;
    drop_graph();
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    int rc = PDHG_OK;
    for (int i = 0; i < window && rc == PDHG_OK; ++i) rc = launch_iteration(tau, sigma, eps, k);
    hipError_t e = hipStreamEndCapture(stream, &g);
    if (rc) {
      if (g) hipGraphDestroy(g);
      return rc;
    }
    HIP_TRY(e);
    e = hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) {
      gexec = nullptr;
      return fail(PDHG_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    g_tau = tau;
    g_sigma = sigma;
    g_eps = eps;
    g_k = k;
    g_window = window;
    g_stop = stop;
    g_spec = (int)spec;
    return PDHG_OK;
  }

  // A speculative iteration halted after sub-iteration 0 (done = kHaltTail): wait for the no-op launches behind it,
  // re-arm, and run the rest of its dual loop and its outer tests (launch_dual's tail + launch_outer of the full
  // schedule).  h: the control block after it (iters counts the completed iterations, the halted one included).
  int finish_halted(double sigma, double eps, int k, Ctrl& h) {
    int rc;
    HIP_TRY(hipStreamSynchronize(stream));
    int zero = 0;
    HIP_TRY(hipMemcpyAsync(&kp.ctrl->done, &zero, sizeof(int), hipMemcpyHostToDevice, stream));
    spec = false;
    if ((rc = launch_dual_tail((R)sigma, eps, k))) return rc;
    if ((rc = launch_outer(eps, k))) return rc;
    return read_ctrl(h);   // synchronizes (zero stays valid until the copy ran)
  }

  int iterate(int n, double tau, double sigma, double eps, int k, pdhg_stats* st) {
    int rc;
    if ((rc = reset_ctrl())) return rc;
    const int window = 8;   // host runs at most 2*window iterations ahead of the device
    std::vector<hipEvent_t> evs;
    const IterTuning it = IterTuning::from_env();
    if (it.graph) use_graph = *it.graph != 0;
    // Speculative one-sub-iteration schedule (the head form, rho_alp_iters > 1): C2's T = 1 marching windows exit the
    // dual loop after sub-iteration 0 in nearly every iteration, and the rest of the loop (chunk passes, finalizes,
    // final pass, outer-sum pass: 6 launches) then only returns at once.  After a window of iterations that all ran
    // one sub-iteration, the host enqueues iterations without those launches; an iteration whose loop does not exit
    // after sub-iteration 0 halts (done = kHaltTail, every later kernel returns), and the host runs the rest of its
    // loop and its outer tests -- the launches the full schedule would have made, in the same order -- then goes on
    // with the full schedule for a few windows.  Same kernels on the same data: the states are the full schedule's
    // bit for bit.  PDHG_SPEC=0 keeps the full schedule.
    const bool spec_able = pp.spec_ok && pp.dual_head && k > 1 && k <= kDualMultiMax;
    const bool spec_force = spec_able && it.spec_force;   // tests: speculate from the first iteration on
    spec = spec_force;
    struct SpecOff {   // every return path leaves the full schedule for the drop-in update_* calls
      bool& s;
      ~SpecOff() { s = false; }
    } spec_off{spec};
    int cool = 0;
    long long last_iters = 0, last_inner = 0;
    auto drain_events = [&]() {
      for (auto e : evs) hipEventDestroy(e);
      evs.clear();
    };
    for (int i = 0; i < n;) {
      // a whole window from the graph when one fits and the state allows it; otherwise one eager iteration
      const bool steady = !pp.fuse_res || res_valid;
      if (use_graph && warm && !prof && steady && i % window == 0 && n - i >= window) {
        if ((rc = ensure_graph(tau, sigma, eps, k, window))) return rc;
        HIP_TRY(hipGraphLaunch(gexec, stream));
        i += window;
        if (spec) spec_iters += window;
      } else {
        if ((rc = launch_iteration(tau, sigma, eps, k))) return rc;
        warm = true;
        ++i;
        if (spec) ++spec_iters;
      }
      const bool check = i % window == 0 && i < n;
      if (!check) continue;
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(e, stream));
      evs.push_back(e);
      if (evs.size() < 2) continue;
      HIP_TRY(hipEventSynchronize(evs[evs.size() - 2]));
      Ctrl h;
      HIP_TRY(hipMemcpy(&h, kp.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));
      if (h.done == kHaltTail) {
        ++spec_halts;
        if ((rc = finish_halted(sigma, eps, k, h))) return rc;
        drain_events();
        i = h.iters;              // the halted iteration is complete; the ones enqueued after it were no-ops
        spec = spec_force;
        cool = spec_force ? 0 : 4;   // windows on the full schedule before speculating again
        last_iters = h.iters;
        last_inner = h.inner_total;
        if (h.done) break;
        continue;
      }
      if (h.done) break;
      if (spec_able) {   // the checked window's iterations all ran one sub-iteration: speculate from here on
        const long long d_it = h.iters - last_iters, d_in = h.inner_total - last_inner;
        if (cool > 0) --cool;
        else if (!spec && d_it > 0 && d_in == d_it) spec = true;
        last_iters = h.iters;
        last_inner = h.inner_total;
      }
    }
    drain_events();
    Ctrl h;
    if ((rc = read_ctrl(h))) return rc;
    while (h.done == kHaltTail) {   // a halt in the last windows: finish it and run what is left
      ++spec_halts;
      if ((rc = finish_halted(sigma, eps, k, h))) return rc;
      spec = false;
      for (int i = h.iters; i < n && !h.done; ++i) {
        if ((rc = launch_iteration(tau, sigma, eps, k))) return rc;
        if ((i + 1) % window == 0 && (rc = read_ctrl(h))) return rc;
      }
      if ((rc = read_ctrl(h))) return rc;
    }
    spec = false;
    if (st) stats_from_ctrl(h, st);
    primal_done = false;
    return PDHG_OK;
  }

  // ---------------- t-slab phases (multi-GPU; the caller moves planes between slabs) ----------------
  // One outer iteration of a slab (include/pdhg.h): slab_residual(rows without the rho halo) ||
  // [rho halo] -> slab_residual(the halo row) -> slab_forward -> [allgather D, S1] -> slab_fixup ->
  // slab_backward -> [allreduce sums] -> slab_primal_finalize -> slab_dual(rows without the phi_bar
  // halo) || [phi_bar halo] -> slab_dual(the halo row + sums) -> [allreduce] -> slab_dual_finalize ->
  // ... -> slab_outer -> [allreduce] -> slab_outer_finalize.  With one slab this is iterate().
  int need_slab() const { return slab ? PDHG_OK : fail(PDHG_ERR_STATE, "not a t-slab context"); }
  int slab_G(R* out) {   // [G, S2] (iteration-invariant)
    return launch(k_slab_sums<R>, dim3((unsigned)((Mspec + 255) / 256)), dim3(256), 0, kp, 0, out, (size_t)0, Mspec);
  }
  // residual rows: parts bit 0 = the rows that do not read the rho halo, bit 1 = the row that does
  // (the last row, unless this is the window's last slab)
  int slab_residual(int parts) {
    const bool rows = pp.fast_rows || pp.res64;   // row-range residual kernels (else the whole slab after the halo)
    const int T = pb.T, split = (rows && !kp.last_slab) ? T - 1 : (rows ? T : 0);
    int rc;
    if ((parts & 1) && (rc = launch_residual(kp, 0, split))) return rc;
    if ((parts & 2) && (rc = launch_residual(kp, split, T))) return rc;
    return PDHG_OK;
  }
  int slab_forward(R tau) { return slab_forward_part(tau, 0, 1); }
  // part `part` of `nparts` of the column blocks: blocks [b0, b1), spectral modes [m0, m1)
  void part_range(int part, int nparts, int& b0, int& b1, size_t& m0, size_t& m1) const {
    b0 = (int)((long long)kp.nb * part / nparts);
    b1 = (int)((long long)kp.nb * (part + 1) / nparts);
    const size_t Mb = (size_t)pb.nx * kp.B;
    m0 = b0 * Mb;
    m1 = b1 * Mb;
  }
  // zero-carry forward sweep + [D, S1] of one part of the column blocks (after both residual parts)
  int slab_forward_part(R tau, int part, int nparts) {
    int b0, b1;
    size_t m0, m1;
    part_range(part, nparts, b0, b1, m0, m1);
    if (b1 <= b0) return PDHG_OK;
    KP<R> p = kp;
    p.tau = tau;
    p.xt_phase = 1;
    p.b0 = b0;
    int rc = launch_precond(p, b1 - b0);
    if (rc) return rc;
    return launch(k_slab_sums<R>, dim3((unsigned)((m1 - m0 + 255) / 256)), dim3(256), 0, kp, 1, dsbuf, m0, m1);
  }
  int slab_carry_out_part(void* dst, int part, int nparts) {   // [D, S1] modes [m0, m1) into dst (2 planes)
    int b0, b1;
    size_t m0, m1;
    part_range(part, nparts, b0, b1, m0, m1);
    if (m1 <= m0) return PDHG_OK;
    R* d = static_cast<R*>(dst);
    HIP_TRY(hipMemcpyAsync(d + m0, dsbuf + m0, (m1 - m0) * sizeof(R), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d + Mspec + m0, dsbuf + Mspec + m0, (m1 - m0) * sizeof(R), hipMemcpyDeviceToDevice, stream));
    return PDHG_OK;
  }
  int slab_backward_part(R tau, int part, int nparts) {   // carry-corrected backward sweep of one part
    int b0, b1;
    size_t m0, m1;
    part_range(part, nparts, b0, b1, m0, m1);
    if (b1 <= b0) return PDHG_OK;
    KP<R> p = kp;
    p.tau = tau;
    p.xt_phase = 2;
    p.b0 = b0;
    return launch_precond(p, b1 - b0);
  }
  int slab_update(R tau, double* sums) { return launch_primal(tau, 4, 0, sums); }   // after every part
  // classify the modes once from everybody's [G, S2]: long-range where some slab's gain G >= delta
  int slab_long_modes(const R* allGS, int nranks, double delta, int* K_out) {
    R* gmax = nullptr;
    HIP_TRY(hipMalloc(&gmax, Mspec * sizeof(R)));
    hipLaunchKernelGGL((k_slab_gmax<R>), dim3((unsigned)((Mspec + 255) / 256)), dim3(256), 0, stream, allGS, Mspec,
                       nranks, gmax);
    std::vector<R> h(Mspec);
    hipError_t e = hipMemcpyAsync(h.data(), gmax, Mspec * sizeof(R), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    hipFree(gmax);
    HIP_TRY(e);
    std::vector<int> pos(Mspec), idx;
    for (size_t m = 0; m < Mspec; ++m) {
      const bool lng = !((double)h[m] < delta);   // NaN counts as long (exact path)
      pos[m] = lng ? (int)idx.size() : -1;
      if (lng) idx.push_back((int)m);
    }
    int rc;
    if (!long_pos && (rc = alloc(&long_pos, Mspec))) return rc;
    if (long_idx) {   // re-classification: drop the old list
      hipFree(long_idx);
      allocs.erase(std::find(allocs.begin(), allocs.end(), (void*)long_idx));
      long_idx = nullptr;
    }
    if (!idx.empty() && (rc = alloc(&long_idx, idx.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(long_pos, pos.data(), Mspec * sizeof(int), hipMemcpyHostToDevice, stream));
    if (!idx.empty())
      HIP_TRY(hipMemcpyAsync(long_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    long_K = (int)idx.size();
    *K_out = long_K;
    return PDHG_OK;
  }
  int slab_fixup_nb(const R* D_left, const R* S1_right, const R* allLong, const R* allGS, int rank, int nranks,
                    int part = 0, int nparts = 1) {
    if (long_K < 0) return fail(PDHG_ERR_STATE, "pdhg_slab_long_modes has not been called");
    int b0, b1;
    size_t m0, m1;
    part_range(part, nparts, b0, b1, m0, m1);
    if (m1 <= m0) return PDHG_OK;
    return launch(k_slab_fix_nb<R>, dim3((unsigned)((m1 - m0 + 255) / 256)), dim3(256), 0, kp, dsbuf, D_left, S1_right, allLong, long_pos, long_K, allGS, rank, nranks, carry_y, m0, m1);
  }
  int slab_fixup(const R* allDS, const R* allGS, int rank, int nranks) {
    return launch(k_slab_fix<R>, dim3((unsigned)((Mspec + 255) / 256)), dim3(256), 0, kp, allDS, allGS, rank, nranks, carry_y);
  }
  int slab_backward(R tau, double* sums) { return launch_primal(tau, 2 | 4, 2, sums); }
  int slab_primal_finalize(const double* sums) {
    return launch(k_finalize_primal, dim3(1), dim3(1024), 0, sums, 1, 0, kp.ctrl);
  }
  // dual rows: parts bit 0 = the rows that do not read the phi_bar halo, bit 1 = the row that does
  // (row 0, unless this is the window's first slab) followed by the sum reduction into `sums`
  int slab_dual(R sigma, int k, int sub, double* sums, int parts) {
    KP<R> p = kp;
    p.sigma = sigma;
    p.inplace = (k <= 1) ? 1 : 0;
    p.sub = sub;
    if (!p.inplace && !pp.two_sets)
      return fail(PDHG_ERR_STATE, "rho_alp_iters=%d needs a context created with rho_alp_iters > 1", k);
    const int T = pb.T, split = pp.fast_dual ? (kp.j0 > 0 ? 1 : 0) : T;   // halo rows [0, split)
    const int gz_in = pp.fast_dual ? (T - split + pp.jchunk_d - 1) / pp.jchunk_d : 0;
    int rc;
    if ((parts & 1) && pp.fast_dual) {
      ProfScope ps(this, "dual");
      if ((rc = launch_dual_fast(p, split, T, 0))) return rc;
    }
    if (!(parts & 2)) return PDHG_OK;
    int nrows_d;
    if (pp.fast_dual) {
      if (split > 0) {
        ProfScope ps(this, "dual");
        if ((rc = launch_dual_fast(p, 0, split, gz_in))) return rc;
      }
      nrows_d = pp.gxd * pp.gyd * (gz_in + (split > 0 ? 1 : 0));
    } else {
      ProfScope ps(this, "dual");
      rc = with_egno<3>([&](auto eg) {
        return launch(k_dual_2d<R, decltype(eg)::value>, dim3(pp.gx5, pp.g5), dim3(256), 0, p);
      });
      if (rc) return rc;
      nrows_d = pp.gx5 * pp.g5;
    }
    return launch(k_reduce_vec, dim3(1), dim3(1024), 0, p.partials, nrows_d, 3 + 3 * pp.na, 0.0, sums);
  }
  int slab_dual_finalize(double eps, int sub, const double* sums) {
    return launch(k_finalize_dual, dim3(1), dim3(1024), 0, sums, 1, pp.na, pp.n_dead, eps, sub, kp.ctrl, 0);
  }
  int slab_outer(int k, double* sums) {
    if (k <= 1) return PDHG_OK;
    if (int rc = launch(k_outer_sums<R>, dim3(pp.g_outer), dim3(256), 0, kp, (size_t)pb.T * plane(), 0)) return rc;
    return launch(k_reduce_vec, dim3(1), dim3(1024), 0, kp.partials, pp.g_outer, kNumSums, 0.0, sums);
  }
  int slab_outer_finalize(double eps, int k, const double* sums) {
    return launch(k_finalize_outer, dim3(1), dim3(1024), 0, sums, k > 1 ? 1 : 0, pp.na, eps, k > 1 ? 1 : 0, stop_conv,
                  stop_nan, kp.ctrl, 0);
  }
  // planes out: 0 rho row 0 (current set), 1 phi_bar row T, 2 [D, S1] (2 spectral planes),
  // 3 [D, S1] of the long-range modes (2 x long_K), 4 phi row T (the next slab's report halo)
  int slab_plane_out(int which, void* dst) {
    const size_t npl = plane();
    switch (which) {
      case 0: return launch(k_copy_cur_rho<R>, dim3(1024), dim3(256), 0, kp, (R*)dst, npl);
      case 1: HIP_TRY(hipMemcpyAsync(dst, kp.phibar + (size_t)pb.T * npl, npl * sizeof(R), hipMemcpyDeviceToDevice, stream)); break;
      case 2: HIP_TRY(hipMemcpyAsync(dst, dsbuf, 2 * Mspec * sizeof(R), hipMemcpyDeviceToDevice, stream)); break;
      case 3:
        if (long_K < 0) return fail(PDHG_ERR_STATE, "pdhg_slab_long_modes has not been called");
        if (long_K > 0)
          return launch(k_slab_gather_long<R>, dim3((unsigned)((long_K + 255) / 256)), dim3(256), 0, dsbuf, Mspec,
                        long_idx, long_K, (R*)dst);
        break;
      case 4: HIP_TRY(hipMemcpyAsync(dst, kp.phi + (size_t)pb.T * npl, npl * sizeof(R), hipMemcpyDeviceToDevice, stream)); break;
      default: return fail(PDHG_ERR_ARG, "unknown plane %d", which);
    }
    return PDHG_OK;
  }
  // planes in: 0 rho halo (next slab's rho row 0), 1 phi_bar row 0 (previous slab's phi_bar row T)
  int slab_plane_in(int which, const void* src) {
    const size_t npl = plane();
    switch (which) {
      case 0: HIP_TRY(hipMemcpyAsync(halo_rho, src, npl * sizeof(R), hipMemcpyDeviceToDevice, stream)); break;
      case 1: HIP_TRY(hipMemcpyAsync(kp.phibar, src, npl * sizeof(R), hipMemcpyDeviceToDevice, stream)); break;
      default: return fail(PDHG_ERR_ARG, "unknown plane %d", which);
    }
    return PDHG_OK;
  }
  int set_stream(hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(stream));
    if (own_stream) HIP_TRY(hipStreamDestroy(stream));
    stream = s;
    own_stream = false;
    return PDHG_OK;
  }
  // ---------------- x-slab phases (multi-GPU for T = 1 windows; the caller moves data between ranks) ------------
  // One outer iteration (include/pdhg.h): halo_out(0) -> [allgather] -> halo_in(0) -> residual ->
  // wire(0) -> [all-to-all] -> wire(1) -> precond -> wire(2) -> [all-to-all] -> wire(3) -> update(sums) ->
  // halo_out(1) -> [allgather] || [allreduce sums] -> primal_finalize -> halo_in(1) -> dual ... as a t-slab.
  int need_xslab() const { return xslab ? PDHG_OK : fail(PDHG_ERR_STATE, "not an x-slab context"); }
  KP<R> col_params() const {   // the x transform of this rank's column blocks (whole x lines)
    KP<R> q = kp;
    q.nx = xs_nxg;
    q.nb = pp.xs_nbs;
    q.work = colwork;
    q.lamy = lamy_base + (size_t)xs_rank * pp.xs_nbs * kp.B;
    q.xt_phase = 0;
    q.xl0 = 0;
    q.xl1 = xs_nxg;
    return q;
  }
  size_t xs_chunk() const { return (size_t)pb.T * pp.xs_nbs * xs_nloc * kp.B; }   // wire floats per rank pair
  size_t xs_halo_elems(int which) const { return (size_t)2 * (which == 0 ? 1 + pp.na : 1) * pb.T * pb.ny; }
  int xs_wire(int stage, void* buf) {
    // 0: rows -> wire (after the residual), 1: wire -> cols, 2: cols -> wire (after the precond), 3: wire -> rows
    const size_t L = (size_t)xs_nloc * kp.B;
    const size_t total4 = xs_chunk() * xs_P / 4;
    const unsigned g = (unsigned)std::max<size_t>(1, std::min<size_t>((total4 + 255) / 256, 8192));
    R* S = static_cast<R*>(buf);
    if (stage == 0 || stage == 3)
      return launch(k_xs_rows_wire<R>, dim3(g), dim3(256), 0, kp.work, S, stage == 0 ? 0 : 1, xs_P, pb.T, kp.nb,
                    pp.xs_nbs, pb.nx, kp.xl0, kp.B, L);
    if (stage == 1 || stage == 2)
      return launch(k_xs_cols_wire<R>, dim3(g), dim3(256), 0, colwork, S, stage == 2 ? 0 : 1, xs_P, pb.T, pp.xs_nbs,
                    xs_nxg, xs_nloc, kp.B, L);
    return fail(PDHG_ERR_ARG, "unknown wire stage %d", stage);
  }
  int xs_halo_out(int which, void* dst) {
    if (which != 0 && which != 1) return fail(PDHG_ERR_ARG, "unknown halo %d", which);
    const unsigned g = (unsigned)std::max<size_t>(1, std::min<size_t>((xs_halo_elems(which) + 255) / 256, 4096));
    return launch(k_xs_halo_out<R>, dim3(g), dim3(256), 0, kp, which, static_cast<R*>(dst));
  }
  int xs_halo_in(int which, const void* left, const void* right) {
    if (which != 0 && which != 1) return fail(PDHG_ERR_ARG, "unknown halo %d", which);
    const unsigned g = (unsigned)std::max<size_t>(1, std::min<size_t>((xs_halo_elems(which) + 255) / 256, 4096));
    // Neumann x edges (bc_x 1): the first slab's left ghost and the last slab's right ghost replicate the slab's own
    // edge row instead of the ring neighbour's
    const int own_l = (pb.bc_x == 1 && xs_x0 == 0) ? 1 : 0, own_r = (pb.bc_x == 1 && xs_x0 + xs_nloc == xs_nxg) ? 1 : 0;
    const int rc = launch(k_xs_halo_in<R>, dim3(g), dim3(256), 0, kp, which, static_cast<const R*>(left),
                          static_cast<const R*>(right), own_l, own_r);
    if (which == 0) res_valid = false;
    return rc;
  }
  int xs_residual() { return launch_residual(kp, 0, pb.T); }
  int xs_precond() { return launch_precond(col_params()); }
  int xs_update(R tau, double* sums) { return launch_primal(tau, 4, 0, sums); }

  int slab_status(pdhg_stats* st) {
    Ctrl h;
    int rc;
    if ((rc = read_ctrl(h))) return rc;
    stats_from_ctrl(h, st);
    return PDHG_OK;
  }

  // ---------------- state ----------------
  bool live(int a, int comp, int n_ctrl) const {   // which (array, component) is stored
    if (pb.ndim == 1 || pb.egno == 3) return a < 2 && comp == 0;
    (void)n_ctrl;
    return (a < 2) ? comp == 0 : comp == 1;
  }
  int n_ctrl() const { return (pb.ndim == 1 || pb.egno == 3) ? 1 : 2; }
  int n_alp_ref() const { return pb.ndim == 1 ? 2 : 4; }

  template <typename E>
  void compute_row0_sq(const std::vector<E>& row0) {
    double s = 0.0;   // live rows only (x-slab: [xl0, xl1) of the padded local rows)
    const size_t ny = pb.ny;
    for (size_t i = (size_t)kp.xl0 * ny; i < (size_t)kp.xl1 * ny; ++i) s += (double)row0[i] * (double)row0[i];
    row0_sq = s;
  }

  int set_state(const double* phi, const double* rho, const double* alp) {
    res_valid = false;
    const size_t npl = plane();
    const int T = pb.T;
    // the parts given overwrite the CURRENT buffer set (two sets when rho_alp_iters > 1), so a part passed as null
    // keeps the device's values -- window marching re-seeds phi alone when rho / alp are already resident
    int cur = 0;
    HIP_TRY(hipMemcpyAsync(&cur, &kp.ctrl->cur, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const size_t nphi = (size_t)(T + 1) * npl, n = (size_t)T * npl;
    const auto buf = plane_scratch<R>(nphi, alp != nullptr);
    if (phi) {   // narrowed once for both copies (mixed: phi as given, full doubles)
      const P* src = as_elems<P>(phi, nphi, buf.get());
      H2D(phi_dev(), src, nphi * sizeof(P));
      H2D(phibar_dev(), src, nphi * sizeof(P));
      compute_row0_sq(std::vector<P>(src, src + npl));
    }
    if (rho) H2D(kp.rho[cur], as_elems<R>(rho, n, buf.get()), n * sizeof(R));
    if (alp) {
      const int nc = n_ctrl(), nar = n_alp_ref();
      for (int a = 0; a < nar; ++a)
        for (int c = 0; c < nc; ++c)
          if (!live(a, c, nc))
            for (size_t i = 0; i < n; ++i)
              if (alp[((size_t)a * n + i) * nc + c] != 0.0)
                return fail(PDHG_ERR_UNSUPPORTED,
                            "alp[%d][...][%d] is a dead control component (identically zero in the reference "
                            "examples) but holds non-zero values; only live components are stored", a, c);
      for (int a = 0; a < nar; ++a)
        for (int c = 0; c < nc; ++c) {
          if (!live(a, c, nc)) continue;
          alp_gather(buf.get(), alp, n, nc, a, c);
          H2D(kp.alp[cur][a], buf.get(), n * sizeof(R));
        }
    }
    Ctrl h{};
    h.cur = cur;
    h.row0_sq = row0_sq;
    H2D(kp.ctrl, &h, sizeof(Ctrl));
    primal_done = false;
    return PDHG_OK;
  }

  int set_phi_bar(const double* pbar) {
    const size_t n = (size_t)(pb.T + 1) * plane();
    const auto buf = plane_scratch<P>(n);
    H2D(phibar_dev(), as_elems<P>(pbar, n, buf.get()), n * sizeof(P));
    return PDHG_OK;
  }

  int get_phi_bar(double* pbar) {
    HIP_TRY(hipStreamSynchronize(stream));
    const size_t n = (size_t)(pb.T + 1) * plane();
    return get_plane(pbar, (const P*)phibar_dev(), 0, n, plane_scratch<P>(n).get());
  }

  int get_work(double* out, size_t count) {
    HIP_TRY(hipStreamSynchronize(stream));
    const size_t nwork = pb.ndim == 2 ? (size_t)pb.T * kp.nb * pb.nx * kp.B : (size_t)pb.T * pb.nx;
    if (count > nwork) return fail(PDHG_ERR_ARG, "work buffer holds %zu elements", nwork);
    return get_plane(out, (const R*)kp.work, 0, count, plane_scratch<R>(count).get());
  }

  // rows [row0, row0 + rows_phi) of phi / phi_bar and [row0, row0 + rows) of rho / alp into the reference layouts
  // (alp [nar][rows][nx][ny][nc], its dead components zero), from the current buffer set
  int rows_out(int row0, int rows_phi, int rows, double* phi, double* pbar, double* rho, double* alp) {
    HIP_TRY(hipStreamSynchronize(stream));
    Ctrl h;
    int rc;
    if ((rc = read_ctrl(h))) return rc;
    const size_t npl = plane(), nphi = (size_t)rows_phi * npl, n = (size_t)rows * npl, off = (size_t)row0 * npl;
    const auto buf = plane_scratch<R>(std::max(nphi, n), alp != nullptr);
    if (phi && (rc = get_plane(phi, (const P*)phi_dev(), off, nphi, buf.get()))) return rc;
    if (pbar && (rc = get_plane(pbar, (const P*)phibar_dev(), off, nphi, buf.get()))) return rc;
    if (rho && (rc = get_plane(rho, (const R*)kp.rho[h.cur], off, n, buf.get()))) return rc;
    if (alp) {
      const int nc = n_ctrl(), nar = n_alp_ref();
      std::memset(alp, 0, sizeof(double) * n * nc * nar);
      for (int a = 0; a < nar; ++a)
        for (int c = 0; c < nc; ++c) {
          if (!live(a, c, nc)) continue;
          HIP_TRY(hipMemcpy(buf.get(), kp.alp[h.cur][a] + off, n * sizeof(R), hipMemcpyDeviceToHost));
          alp_scatter(alp, buf.get(), n, nc, a, c);
        }
    }
    return PDHG_OK;
  }
  // the whole window: phi [T+1], rho / alp [T]
  int get_state(double* phi, double* rho, double* alp) { return rows_out(0, pb.T + 1, pb.T, phi, nullptr, rho, alp); }
  // rows [row0, row0 + nrows) of phi / phi_bar ([T+1]) and rho / alp ([T])
  int get_rows(int row0, int nrows, double* phi, double* pbar, double* rho, double* alp) {
    const int T = pb.T;
    if (row0 < 0 || nrows < 1 || row0 + nrows > T + 1 || ((rho || alp) && row0 + nrows > T))
      return fail(PDHG_ERR_ARG, "rows [%d, %d) outside phi [0, %d) / rho, alp [0, %d)", row0, row0 + nrows, T + 1, T);
    return rows_out(row0, nrows, nrows, phi, pbar, rho, alp);
  }

  // ---------------- closed-loop trajectories (kernels_traj.hpp; include/pdhg.h pdhg_trajectories) ----------------
  // Samples are staged in chunks (staging.hpp SampleChunks; the rollout's chunk: RolloutLayout).
  std::vector<double> grid_x, grid_y;   // the grid coordinates in fp64 (kp.ax / kp.ay hold f coefficients in R)
  double* d_xs64 = nullptr;             // ... on the device, uploaded by the first call
  double* d_ys64 = nullptr;
  // the grid checks of a rollout and the fp64 grid on the device (uploaded by the first call)
  int traj_ready(const pdhg_traj_opts& o) {
    const int nd = pb.ndim;
    const double Px = o.x_period, Py = nd == 2 ? o.y_period : 1.0;
    // the grids the reference builds (run_example.py:273-287): ascending, within one period
    for (int i = 1; i < pb.nx; ++i)
      if (!(grid_x[i] > grid_x[i - 1])) return fail(PDHG_ERR_UNSUPPORTED, "trajectories need an ascending x grid");
    for (int i = 1; nd == 2 && i < pb.ny; ++i)
      if (!(grid_y[i] > grid_y[i - 1])) return fail(PDHG_ERR_UNSUPPORTED, "trajectories need an ascending y grid");
    if (!(grid_x[pb.nx - 1] - grid_x[0] < Px) || (nd == 2 && !(grid_y[pb.ny - 1] - grid_y[0] < Py)))
      return fail(PDHG_ERR_UNSUPPORTED, "the grid spans a period or more");
    if (nd == 1 && !(grid_x[0] >= 0.0 && grid_x[pb.nx - 1] < Px))
      return fail(PDHG_ERR_UNSUPPORTED, "1-D trajectories need the grid in [0, x_period) (jnp.interp period=)");
    int rc;
    if (!d_xs64) {
      if ((rc = alloc(&d_xs64, pb.nx))) return rc;
      H2D(d_xs64, grid_x.data(), pb.nx * sizeof(double));
      if (nd == 2) {
        if ((rc = alloc(&d_ys64, pb.ny))) return rc;
        H2D(d_ys64, grid_y.data(), pb.ny * sizeof(double));
      }
    }
    return PDHG_OK;
  }
  // the kernel parameters of this context's T rows (samples, positions, noise and records are the caller's)
  TrajP<R> traj_params(const pdhg_traj_opts& o, int noise_mode) const {
    const int nd = pb.ndim;
    TrajP<R> a{};
    a.nx = pb.nx;
    a.ny = pb.ny;
    a.T = pb.T;
    a.step0 = 0;
    a.bcx = pb.bc_x;
    a.method = o.method;
    a.center_x = o.center_x ? 1 : 0;
    a.center_y = o.center_y ? 1 : 0;
    a.noise_mode = noise_mode;
    a.seed = o.seed;
    a.Px = o.x_period;
    a.Py = nd == 2 ? o.y_period : 1.0;
    a.dt = pb.dt;
    a.sq = std::sqrt(2 * pb.epsl * pb.dt);
    a.inv_dx = 1.0 / pb.dx;
    a.inv_dy = nd == 2 ? 1.0 / pb.dy : 0.0;
    a.xs = d_xs64;
    a.ys = d_ys64;
    for (int s = 0; s < 2; ++s)
      for (int k = 0; k < 4; ++k) a.alp[s][k] = kp.alp[s][k];
    a.ctrl = kp.ctrl;
    return a;
  }
  int launch_traj(const TrajP<R>& a) {
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    if (pb.ndim == 1) return with_egno<2>([&](auto E) { return launch(k_traj_1d<R, decltype(E)::value>, grid, block, 0, a); });
    return with_egno<3>([&](auto E) { return launch(k_traj_2d<R, decltype(E)::value>, grid, block, 0, a); });
  }
  // pdhg_slab_trajectories: this slab's T steps of a longer rollout, global steps [step0, step0 + T); every buffer is
  // a device pointer used on the context's stream (noise and records indexed by global step, kernels_traj.hpp)
  int slab_trajectories(const pdhg_traj_opts& o, int step0, unsigned long long n, const double* d_x_in,
                        const double* d_noise, double* d_x_out, double* d_rec_x, double* d_rec_a) {
    int rc;
    if ((rc = traj_ready(o))) return rc;
    TrajP<R> a = traj_params(o, pb.epsl > 0 ? (d_noise ? 1 : 2) : 0);
    a.step0 = step0;
    a.n = n;
    a.s0 = (unsigned long long)o.sample_offset;
    a.x_in = d_x_in;
    a.noise = d_noise;
    a.x_out = d_x_out;
    a.rec_x = d_rec_x;
    a.rec_a = d_rec_a;
    return launch_traj(a);
  }
  int trajectories(const pdhg_traj_opts& o, const double* x_init, const double* noise, double* x_final, double* traj_x,
                   double* traj_alp) {
    if (slab || xslab)
      return fail(PDHG_ERR_UNSUPPORTED, "trajectories need the whole window in one context (not a t-slab / x-slab)");
    const int nd = pb.ndim, nc = n_ctrl(), T = pb.T;
    int rc;
    if ((rc = traj_ready(o))) return rc;
    const bool noisy = pb.epsl > 0;
    const size_t n = (size_t)o.n_sample;
    const RolloutLayout lay{T, (size_t)nd, (size_t)nc, noisy && noise, traj_x != nullptr, traj_alp != nullptr};
    const size_t w_x = lay.w_x, w_a = lay.w_a;
    SampleChunks st(n, stream);
    if ((rc = st.alloc(lay.per(), 0, "trajectory chunk"))) return rc;
    const RolloutLayout::Ptrs d = lay.carve(st);
    TrajP<R> a = traj_params(o, noisy ? (noise ? 1 : 2) : 0);
    a.x_in = d.x_in;
    a.x_out = d.x_out;
    a.noise = d.noise;
    a.rec_x = d.rec_x;
    a.rec_a = d.rec_a;
    for (size_t c0 = 0; c0 < n; c0 += st.m) {
      const size_t mc = std::min(st.m, n - c0);
      if ((rc = st.up(d.x_in, x_init, 0, 1, c0, mc, w_x)) || (rc = st.up(d.noise, noise, 0, T, c0, mc, w_x))) return rc;
      a.n = mc;
      a.s0 = (unsigned long long)o.sample_offset + c0;
      if ((rc = launch_traj(a))) return rc;
      if ((rc = st.down(x_final, d.x_out, 0, 1, c0, mc, w_x)) || (rc = st.down(traj_x, d.rec_x, 0, T + 1, c0, mc, w_x)) ||
          (rc = st.down(traj_alp, d.rec_a, 0, T, c0, mc, w_a)))
        return rc;
      HIP_TRY(hipStreamSynchronize(stream));   // the chunk buffers are reused
    }
    return PDHG_OK;
  }

  // ---------------- policy check (kernels_policy.hpp; include/pdhg.h pdhg_policy_eval) ----------------
  // Read-only on the state, as the report.  The samples are staged like the rollout's, in one allocation that also
  // holds the call's table of partial rows (one per workgroup of the whole call, then the folded row).  A null output
  // takes no bytes; with grid starts no start array exists at all.
  int launch_policy(const PolP<R, P>& a) {
    const dim3 grid((unsigned)((a.t.n + 255) / 256)), block(256);
    if (pb.ndim == 1)
      return with_egno<2>([&](auto E) { return launch(k_policy_1d<R, P, decltype(E)::value>, grid, block, 0, a); });
    return with_egno<3>([&](auto E) { return launch(k_policy_2d<R, P, decltype(E)::value>, grid, block, 0, a); });
  }
  int policy_eval(const pdhg_policy_opts& po, const double* x_init, const double* noise, pdhg_policy_report* report,
                  double* running, double* terminal, double* value, double* x_final) {
    if (slab || xslab)
      return fail(PDHG_ERR_UNSUPPORTED, "the policy check needs the whole window in one context, not %s context",
                  slab ? "a t-slab" : "an x-slab");
    const pdhg_traj_opts& o = po.traj;
    const int nd = pb.ndim, T = pb.T;
    size_t n = (size_t)o.n_sample;
    unsigned long long gny = 1;
    if (!x_init) {
      gny = nd == 2 ? (unsigned long long)((pb.ny + po.stride_y - 1) / po.stride_y) : 1;
      const size_t count = (size_t)((pb.nx + po.stride_x - 1) / po.stride_x) * (size_t)gny;
      if (o.n_sample != 0 && n != count)
        return fail(PDHG_ERR_ARG, "n_sample %lld, but the strided grid has %zu starts (n_sample: that or 0)",
                    o.n_sample, count);
      n = count;
    }
    const size_t nwg = (n + 255) / 256;
    if (nwg >= (size_t)1 << 31) return fail(PDHG_ERR_ARG, "n_sample %zu is more than 2^31 workgroups of 256", n);
    int rc;
    if ((rc = traj_ready(o))) return rc;
    const bool noisy = pb.epsl > 0;
    const size_t w_x = (size_t)nd;   // doubles per sample and row
    const size_t per = sizeof(double) * ((x_init ? w_x : 0) + (x_final ? w_x : 0) +
                                         (noisy && noise ? (size_t)T * w_x : 0) + (running ? 1 : 0) +
                                         (terminal ? 1 : 0) + (value ? 1 : 0));
    SampleChunks st(n, stream);
    if ((rc = st.alloc(per, (nwg + 1) * kNumSums, "policy check"))) return rc;
    PolP<R, P> a{};
    a.t = traj_params(o, noisy ? (noise ? 1 : 2) : 0);
    a.t.x_in = st.take(x_init != nullptr, st.m * w_x);
    a.t.x_out = st.take(x_final != nullptr, st.m * w_x);
    a.t.noise = st.take(noisy && noise, (size_t)T * st.m * w_x);
    a.phi = phi_dev();
    a.terminal = po.terminal;
    a.grid_starts = x_init ? 0 : 1;
    a.stride_x = x_init ? 1 : po.stride_x;
    a.stride_y = x_init || nd == 1 ? 1 : po.stride_y;
    a.gny = gny;
    a.running = st.take(running != nullptr, st.m);
    a.term = st.take(terminal != nullptr, st.m);
    a.value = st.take(value != nullptr, st.m);
    a.partials = st.base;
    for (size_t c0 = 0; c0 < n; c0 += st.m) {
      const size_t mc = std::min(st.m, n - c0);
      if ((rc = st.up(a.t.x_in, x_init, 0, 1, c0, mc, w_x)) || (rc = st.up(a.t.noise, noise, 0, T, c0, mc, w_x))) return rc;
      a.t.n = mc;
      a.t.s0 = (unsigned long long)o.sample_offset + c0;
      a.g0 = c0;
      if ((rc = launch_policy(a))) return rc;
      if ((rc = st.down(x_final, a.t.x_out, 0, 1, c0, mc, w_x)) || (rc = st.down(running, a.running, 0, 1, c0, mc, 1)) ||
          (rc = st.down(terminal, a.term, 0, 1, c0, mc, 1)) || (rc = st.down(value, a.value, 0, 1, c0, mc, 1)))
        return rc;
      HIP_TRY(hipStreamSynchronize(stream));   // the chunk buffers are reused
    }
    if (!report) return PDHG_OK;
    double* d_fold = st.base + nwg * kNumSums;
    if ((rc = launch(k_report_finalize, dim3(1), dim3(1024), 0, (const double*)st.base, (int)nwg, d_fold))) return rc;
    double h[kNumSums];
    HIP_TRY(hipMemcpyAsync(h, d_fold, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *report = policy_from_sums(h, (long long)n);
    return PDHG_OK;
  }

  // ---------------- solution report (kernels_report.hpp; include/pdhg.h pdhg_report_state / _rows) ----------------
  // Read-only on everything the iteration owns: the kernels take kp by value and write only the report's own partial
  // table (allocated by the first call) and, for report_rows, staged field planes of at most kReportBudget bytes (staging.hpp RowChunks).
  // y per lane of the tile kernel: 16-B loads of phi (fp64 and mixed: 2 doubles; the mixed kernel spilled 70 VGPRs
  // at 4 and ran behind the per-point kernel), fp32: 4 floats
  static constexpr int kRepYpl = sizeof(P) == 8 ? 2 : 4;
  double* rep_partials = nullptr;   // [rows of the largest launch: report_rows_cap][kNumSums], then the folded row
  int rep_cap = 0;
  P* rep_phi_halo = nullptr;        // t-slab with j0 > 0: phi row 0 = the previous slab's phi row T, staged per call
  struct RepGrid {
    dim3 grid, block;
    int rows, jchunk;
  };
  int report_tiles() const { return (pb.nx / 8) * (pb.ny / (64 * kRepYpl)); }
  // time chunks the tile kernel starts with for nj rows: enough for report_wgs workgroups where the tiles are few
  int report_chunks(int nj) const {
    const int tiles = report_tiles();
    return std::max(1, std::min(nj, (pp.report_wgs + tiles - 1) / tiles));
  }
  // launch shape over nj time rows
  RepGrid report_grid(int nj) const {
    RepGrid g{};
    g.jchunk = nj;
    if (pb.ndim == 2 && pp.report_tile) {
      const int gx = pb.nx / 8, gy = pb.ny / (64 * kRepYpl), tiles = gx * gy;
      int gz = report_chunks(nj);
      g.jchunk = (nj + gz - 1) / gz;
      gz = (nj + g.jchunk - 1) / g.jchunk;   // whole chunks, the last one ragged: <= report_chunks(nj)
      g.grid = dim3(gx, gy, gz);
      g.block = dim3(512);
      g.rows = tiles * gz;
      return g;
    }
    const int n = pb.ndim == 2 ? pb.ny : pb.nx;                  // threads along the contiguous axis
    const long long lines = pb.ndim == 2 ? (long long)nj * pb.nx : nj;
    const int gx = (n + 255) / 256;
    const int G = (int)std::max<long long>(1, std::min<long long>(lines, 8192 / gx));
    g.grid = dim3(gx, G);
    g.block = dim3(256);
    g.rows = gx * G;
    return g;
  }
  // Partial rows of the largest launch over any row range of the window.  The tile grid's chunk count after rounding
  // to whole chunks is not monotone in nj (T = 5 with 4 chunks wanted runs 3 chunks of 2 rows, a 4-row range 4 of 1),
  // so the bound is the count before rounding at nj = T, which is; the per-point grids grow with nj.
  int report_rows_cap() const {
    if (pb.ndim == 2 && pp.report_tile) return report_tiles() * report_chunks(pb.T);
    return report_grid(pb.T).rows;
  }
  // slab_call: through pdhg_slab_report / pdhg_slab_report_rows, whose caller supplies the halo planes
  int report_ready(bool slab_call = false) {
    if (xslab || (slab && !slab_call))
      return fail(PDHG_ERR_UNSUPPORTED, "the report needs the whole window in one context (a t-slab's / x-slab's "
                                        "halo rows are not resident)");
    if (!rep_partials) {
      rep_cap = report_rows_cap();
      if (int rc = alloc(&rep_partials, (size_t)(rep_cap + 1) * kNumSums)) return rc;
      if (slab && slab_j0 > 0)
        if (int rc = alloc(&rep_phi_halo, plane())) return rc;
    }
    return PDHG_OK;
  }
  // the pass over time rows [j0, j1): a partial row per workgroup, the field rows into d_hj / d_cont where given
  int launch_report(int j0, int j1, double* d_hj, double* d_cont, int* rows) {
    const RepGrid g = report_grid(j1 - j0);
    if (g.rows > rep_cap) return fail(PDHG_ERR_STATE, "report table of %d rows for a launch of %d", rep_cap, g.rows);
    *rows = g.rows;
    const RepP rp{j0, j1, g.jchunk, d_hj, d_cont, rep_partials, rep_phi_halo};
    if (pb.ndim == 1)
      return with_egno<2>([&](auto E) { return launch(k_report_1d<R, decltype(E)::value>, g.grid, g.block, 0, kp, rp); });
    if (pp.report_tile)
      return with_egno<3>([&](auto E) {
        return launch(k_report_tile_2d<R, decltype(E)::value, kRepYpl, P>, g.grid, g.block, 0, kp, px, rp);
      });
    return with_egno<3>(
        [&](auto E) { return launch(k_report_2d<R, decltype(E)::value, P>, g.grid, g.block, 0, kp, px, rp); });
  }
  int report_state(pdhg_report* out) {
    int rc, rows = 0;
    if ((rc = report_ready())) return rc;
    double* d_out = rep_partials + (size_t)rep_cap * kNumSums;
    {
      ProfScope ps(this, "report");
      if ((rc = launch_report(0, pb.T, nullptr, nullptr, &rows))) return rc;
      if ((rc = launch(k_report_finalize, dim3(1), dim3(1024), 0, (const double*)rep_partials, rows, d_out))) return rc;
    }
    double h[kNumSums];
    HIP_TRY(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out = report_from_sums(h, (long long)pb.T * pb.nx * pb.ny);
    return PDHG_OK;
  }
  // ---- the report on a t-slab (pdhg_slab_report / pdhg_slab_report_rows; pdhg_multi.hpp folds the slabs) ----
  // phi_prev: the previous slab's phi row T (device, phi's type), staged into the report's own plane; the caller has
  // delivered the next slab's fresh rho row 0 through plane_in(0).  Everything is enqueued on the context's stream.
  int slab_report_halo(const void* phi_prev) {
    if (int rc = report_ready(true)) return rc;
    if (slab_j0 == 0) return PDHG_OK;
    if (!phi_prev) return fail(PDHG_ERR_ARG, "a slab after the first needs the previous slab's phi row T");
    HIP_TRY(hipMemcpyAsync(rep_phi_halo, phi_prev, plane() * sizeof(P), hipMemcpyDeviceToDevice, stream));
    return PDHG_OK;
  }
  int slab_report(const void* phi_prev, double* d_sums) {
    int rc, rows = 0;
    if ((rc = slab_report_halo(phi_prev))) return rc;
    ProfScope ps(this, "report");
    if ((rc = launch_report(0, pb.T, nullptr, nullptr, &rows))) return rc;
    return launch(k_report_finalize, dim3(1), dim3(1024), 0, (const double*)rep_partials, rows, d_sums);
  }
  int slab_report_rows(const void* phi_prev, int row0, int nrows, double* d_hj, double* d_cont) {
    int rc, rows = 0;
    if ((rc = rows_inside(row0, nrows, pb.T, "the slab's")) || (rc = slab_report_halo(phi_prev))) return rc;
    if (!d_hj && !d_cont) return PDHG_OK;
    return launch_report(row0, row0 + nrows, d_hj, d_cont, &rows);
  }
  int report_rows(int row0, int nrows, double* hj, double* cont) {
    int rc;
    if ((rc = report_ready()) || (rc = rows_inside(row0, nrows, pb.T))) return rc;
    return RowChunks{stream, plane(), hj, cont}.run(nrows, [&](int c0, int mc, double* d_hj, double* d_cont) {
      int rows = 0;
      return launch_report(row0 + c0, row0 + c0 + mc, d_hj, d_cont, &rows);
    });
  }

  int init_state(const double* g) {
    res_valid = false;
    const size_t npl = plane();
    const int T = pb.T;
    std::vector<P> row(npl);   // phi's type (mixed: g as given)
    for (size_t i = 0; i < npl; ++i) row[i] = (P)g[i];
    compute_row0_sq(row);
    DevBuf d_row;   // freed on every way out
    HIP_TRY(d_row.alloc(npl * sizeof(P)));
    H2D(d_row.p, row.data(), npl * sizeof(P));
    const dim3 grid(4096), block(256);
    const size_t n = (size_t)T * npl;
    int rc;
    if ((rc = launch(k_bcast_rows<P>, grid, block, 0, phi_dev(), (const P*)d_row.p, npl, T + 1)) ||
        (rc = launch(k_bcast_rows<P>, grid, block, 0, phibar_dev(), (const P*)d_row.p, npl, T + 1)) ||
        (rc = launch(k_fill<R>, grid, block, 0, kp.rho[0], n, (R)pb.c_on_rho)))
      return rc;
    for (int a = 0; a < pp.na; ++a)
      if ((rc = launch(k_fill<R>, grid, block, 0, kp.alp[0][a], n, (R)0))) return rc;
    HIP_TRY(hipStreamSynchronize(stream));   // d_row is read until here
    Ctrl h{};
    h.row0_sq = row0_sq;
    H2D(kp.ctrl, &h, sizeof(Ctrl));
    primal_done = false;
    return PDHG_OK;
  }

  int update_primal(double tau) {
    int rc;
    if ((rc = reset_ctrl())) return rc;
    if ((rc = launch_primal((R)tau))) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    primal_done = true;
    return PDHG_OK;
  }

  int update_dual(double sigma, double eps, int k, int* inner_used) {
    int rc;
    Ctrl h;
    if ((rc = read_ctrl(h))) return rc;
    h.done = 0;
    h.inner_done = 0;
    h.inner_count = 0;
    h.kstar_found = 0;
    H2D(kp.ctrl, &h, sizeof(Ctrl));
    if ((rc = launch_dual((R)sigma, eps, k))) return rc;
    if (primal_done) {
      if ((rc = launch_outer(eps, k))) return rc;
    } else if (k > 1) {
      // no primal in this pairing: still move the state to the current buffer set
      hipLaunchKernelGGL(k_finalize_outer, dim3(1), dim3(1024), 0, stream, kp.partials, 0, pp.na, -1.0, 1, 0, 0, kp.ctrl);
    }
    if ((rc = read_ctrl(h))) return rc;
    if (inner_used) *inner_used = h.inner_count;
    primal_done = false;
    return PDHG_OK;
  }

  int errors(double* e1, double* e2) {
    Ctrl h;
    int rc;
    if ((rc = read_ctrl(h))) return rc;
    if (e1) *e1 = h.err1;
    if (e2) *e2 = h.err2;
    return PDHG_OK;
  }

  double algorithmic_bytes(int k, const std::string& cls) const {
    const double N = (double)pb.T * (double)(kp.xl1 - kp.xl0) * (double)pb.ny;   // live rows (x-slab)
    const double S = (double)sizeof(R);
    const double X = (double)sizeof(P) - S;   // mixed: the extra bytes of a phi / phi_bar element (else 0)
    const bool d2 = pb.ndim == 2;
    const double nr = 1.0 + pp.na;   // rho + live alp arrays
    if (cls == "iteration") {
      // 2-D 4N(14 + 11k + 5[k>1]), 1-D 4N(12 + 7k + 3[k>1]); generalised to S and na
      // (of those, phi / phi_bar: 3 in the update and 1 per dual sub-iteration)
      if (d2) return S * N * (14.0 + 11.0 * k + 5.0 * (k > 1)) + X * N * (3.0 + k);
      return S * N * (12.0 + 7.0 * k + 3.0 * (k > 1));
    }
    // fused residual: the dual also writes the residual rows (+1), the tile-edge row terms (2 rows per 8)
    // and the strip-edge column terms (2 per 256); the residual kernel reads them and writes the spectrum
    const double edge = !pp.fuse_res ? 0.0 : d2 ? 2.0 / 8.0 + 2.0 / (64.0 * pp.dual_ypl) : 2.0 / 64.0;   // 1-D: per wave
    if (cls == "dual") return S * N * (1.0 + 2.0 * nr + (pp.fuse_res ? 1.0 + edge : 0.0)) + X * N;
    if (cls == "residual") return S * N * (pp.fuse_res ? 2.0 + edge : nr + 1.0);
    if (cls == "precond") return S * N * (d2 ? 4.0 : 2.0);   // 2-D: x-DHT+Thomas fwd (2N) + bwd+x-DHT (2N)
    if (cls == "update") return S * N * 4.0 + X * N * 3.0;   // read U, phi; write phi, phi_bar
    return -1.0;
  }
};

}  // namespace
