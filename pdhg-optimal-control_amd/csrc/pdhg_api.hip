// The C boundary of libpdhg (include/pdhg.h): status + error text, handles, dispatch on the context's precision,
// and the extern "C" entry points.  The context itself is ctx_impl.hpp; what it runs is decided in path_plan.hpp from
// the environment overrides of tuning.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <string>

#include "../../include/pdhg.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return fail(PDHG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
// stream-ordered host -> device copy inside Impl (Impl::h2d)
#define H2D(d, s, n)                        \
  do {                                      \
    const int rc_h2d_ = h2d((d), (s), (n)); \
    if (rc_h2d_) return rc_h2d_;            \
  } while (0)

}  // namespace

#include "staging.hpp"
#include "ctx_impl.hpp"

namespace {

// handle tags: a pdhg_ctx* and a pdhg_multi* both start with one; an entry point rejects the other kind
constexpr uint32_t kCtxMagic = 0x50444843u;    // "PDHC"
constexpr uint32_t kMultiMagic = 0x5044484du;  // "PDHM"

constexpr int kMixedPrecision = 12;   // pdhg_problem.precision: fp32 state, fp64 phi / phi_bar (single 2-D contexts)

struct CtxBox {
  uint32_t magic = kCtxMagic;
  int precision;
  std::unique_ptr<ImplBase> impl;
};

// the context behind a handle, with its device made current (a thread may drive contexts on several GPUs:
// every kernel launch, allocation and hipFuncSetAttribute of the call then lands on the context's device)
CtxBox* ctx_box(pdhg_ctx* ctx) {
  if (!ctx) return nullptr;
  CtxBox* b = reinterpret_cast<CtxBox*>(ctx);
  if (b->magic != kCtxMagic || !b->impl) return nullptr;
  if (hipSetDevice(b->impl->device) != hipSuccess) return nullptr;
  return b;
}

template <typename F>
int dispatch(pdhg_ctx* ctx, F&& f) {
  CtxBox* b = ctx_box(ctx);
  if (!b) return fail(PDHG_ERR_ARG, "null or foreign context handle");
  if (b->precision == 8) return f(*static_cast<Impl<double>*>(b->impl.get()));
  if (b->precision == kMixedPrecision) return f(*static_cast<Impl<float, double>*>(b->impl.get()));
  return f(*static_cast<Impl<float>*>(b->impl.get()));
}

// phases shared by the t-slab and x-slab contexts (begin, finalizers, dual, outer, status)
template <typename F>
int phase_dispatch(pdhg_ctx* ctx, F&& f) {
  return dispatch(ctx, [&](auto& im) {
    if (!im.slab && !im.xslab) return fail(PDHG_ERR_STATE, "not a t-slab / x-slab context");
    return f(im);
  });
}

template <typename F>
int xslab_dispatch(pdhg_ctx* ctx, F&& f) {
  return dispatch(ctx, [&](auto& im) {
    int rc = im.need_xslab();
    return rc ? rc : f(im);
  });
}

// t-slab contexts are fp32 or fp64 (the reference's arithmetic); planes crossing this ABI are in the context's
// precision (RealOf)
template <typename F>
int slab_dispatch(pdhg_ctx* ctx, F&& f) {
  return dispatch(ctx, [&](auto& im) {
    int rc = im.need_slab();
    return rc ? rc : f(im);
  });
}
template <typename I>
using RealOf = typename std::remove_reference<I>::type::Real;

// the multi-device context (pdhg_multi.hpp): the done flag of a slab's control block, read by a synchronous
// copy that does not wait for the slab's stream (the caller synchronised on an event recorded after the
// iteration it wants), and the device a slab computes on
int slab_done_flag(pdhg_ctx* ctx, int* done) {
  return slab_dispatch(ctx, [&](auto& im) {
    HIP_TRY(hipMemcpy(im.h_done, &im.kp.ctrl->done, sizeof(int), hipMemcpyDeviceToHost));
    *done = *im.h_done;
    return (int)PDHG_OK;
  });
}
int slab_device(pdhg_ctx* ctx, int* device) {
  return slab_dispatch(ctx, [&](auto& im) {
    int d = -1;
    HIP_TRY(hipGetDevice(&d));
    *device = d;
    return (int)PDHG_OK;
  });
}

// the option checks every rollout and the policy check share (ndim 2: the periods of both axes; n_may_be_zero: grid
// starts, where n_sample 0 stands for the strided grid's count)
int check_traj_opts(const pdhg_traj_opts& o, int ndim, bool n_may_be_zero) {
  if (o.n_sample < (n_may_be_zero ? 0 : 1))
    return fail(PDHG_ERR_ARG, n_may_be_zero ? "n_sample must be 0 or the strided grid's count" : "n_sample must be >= 1");
  if (o.sample_offset < 0) return fail(PDHG_ERR_ARG, "sample_offset must be >= 0");
  if (o.method != 0 && o.method != 1) return fail(PDHG_ERR_ARG, "method %d: 0 linear or 1 nearest", o.method);
  if (!(o.x_period > 0) || (ndim == 2 && !(o.y_period > 0))) return fail(PDHG_ERR_ARG, "periods must be > 0");
  return PDHG_OK;
}
// the row range of the three report-rows entry points (its upper end is checked against the context's rows)
int check_row_range(int row0, int nrows) {
  return row0 < 0 || nrows < 1 ? fail(PDHG_ERR_ARG, "bad row range: row0 %d, nrows %d", row0, nrows) : (int)PDHG_OK;
}

// the problem checks of pdhg_create (before any device is touched) and pdhg_plan_info
int validate_problem(const pdhg_problem& p) {
  if (p.ndim != 1 && p.ndim != 2) return fail(PDHG_ERR_ARG, "ndim %d not implemented", p.ndim);
  if (p.egno < 1 || p.egno > 3) return fail(PDHG_ERR_ARG, "egno %d not implemented", p.egno);
  if (p.egno == 3 && p.ndim != 2) return fail(PDHG_ERR_ARG, "egno 3 requires ndim 2 (set_fns.py:96)");
  if (p.nx < 3 || (p.ndim == 2 && p.ny < 3)) return fail(PDHG_ERR_ARG, "grid must be at least 3 points per axis");
  if (p.ndim == 1 && p.ny != 1) return fail(PDHG_ERR_ARG, "ndim 1 requires ny == 1");
  if (p.T < 1) return fail(PDHG_ERR_ARG, "T must be >= 1");
  if (!(p.dx > 0) || !(p.dt > 0) || (p.ndim == 2 && !(p.dy > 0))) return fail(PDHG_ERR_ARG, "grid spacings must be > 0");
  if (!p.xs || (p.ndim == 2 && !p.ys)) return fail(PDHG_ERR_ARG, "grid coordinates required");
  if (p.precision != 4 && p.precision != 8 && p.precision != kMixedPrecision)
    return fail(PDHG_ERR_ARG, "precision must be 4, 8 or 12 (mixed)");
  if (p.precision == kMixedPrecision && p.ndim != 2)
    return fail(PDHG_ERR_UNSUPPORTED, "mixed precision (12) is implemented for 2-D contexts only");
  if (p.rho_alp_iters < 1) return fail(PDHG_ERR_ARG, "rho_alp_iters must be >= 1");
  // preconditioner boundary conditions (utils_precond.py:121-124, :157-163)
  if (p.ndim == 1 && p.bc_x != 0) return fail(PDHG_ERR_UNSUPPORTED, "H1_precond_1d supports bc=0 only");
  if (p.ndim == 2 && !((p.bc_x == 0 || p.bc_x == 1) && p.bc_y == 0))
    return fail(PDHG_ERR_UNSUPPORTED, "bc (%d,%d): H1_precond_2d supports (0,0) and (1,0) only "
                                      "(utils_precond.py:157-163)", p.bc_x, p.bc_y);
  if (p.ndim == 1 && p.Ct < 0) return fail(PDHG_ERR_ARG, "Ct must be >= 0");
  // C u - Lap u (utils_precond.py:151: "C = 0 and 1 are both fine"); a negative or non-finite C makes
  // dd = (C - lam) dt^2 negative or NaN at the low modes and the pivots' square root NaN without an error
  if (!(p.C >= 0) || !std::isfinite(p.C)) return fail(PDHG_ERR_ARG, "C must be finite and >= 0 (got %g)", p.C);
  return PDHG_OK;
}

// a single context of one Impl type in its box (kept there on failure too: the box's destructor frees it)
template <typename I>
int make_impl(CtxBox& box, const pdhg_problem& p, int device) {
  auto im = std::make_unique<I>();
  im->pb = p;
  im->device = device;
  const int rc = im->setup();
  box.impl = std::move(im);
  return rc;
}

}  // namespace

extern "C" {

const char* pdhg_last_error(void) { return g_err.c_str(); }
#ifndef PDHG_BUILD_ID
#define PDHG_BUILD_ID "unknown"
#endif
__attribute__((used)) static const char kBuildTag[] = "PDHG_BUILD_ID=" PDHG_BUILD_ID;   // read by build()
const char* pdhg_build_id(void) { return kBuildTag + 14; }
int pdhg_abi_version(void) { return PDHG_ABI_VERSION; }

int pdhg_device_count(int* count) {
  if (!count) return fail(PDHG_ERR_ARG, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  *count = (e == hipSuccess) ? n : 0;
  return PDHG_OK;
}

int pdhg_create(const pdhg_problem* prob, int device, pdhg_ctx** out) {
  if (!prob || !out) return fail(PDHG_ERR_ARG, "null argument");
  *out = nullptr;
  const pdhg_problem& p = *prob;
  int rc;
  if ((rc = validate_problem(p))) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PDHG_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(PDHG_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
  auto box = std::make_unique<CtxBox>();
  box->precision = p.precision;
  if (p.precision == 8) rc = make_impl<Impl<double>>(*box, p, device);
  else if (p.precision == kMixedPrecision) rc = make_impl<Impl<float, double>>(*box, p, device);
  else rc = make_impl<Impl<float>>(*box, p, device);
  if (rc) return rc;
  *out = reinterpret_cast<pdhg_ctx*>(box.release());
  return PDHG_OK;
}

int pdhg_destroy(pdhg_ctx* ctx) {
  if (!ctx) return PDHG_OK;
  CtxBox* b = ctx_box(ctx);
  if (!b) return fail(PDHG_ERR_ARG, "foreign context handle");
  b->magic = 0;
  delete b;
  return PDHG_OK;
}

int pdhg_set_state(pdhg_ctx* ctx, const double* phi, const double* rho, const double* alp) {
  return dispatch(ctx, [&](auto& im) { return im.set_state(phi, rho, alp); });
}
int pdhg_get_state(pdhg_ctx* ctx, double* phi, double* rho, double* alp) {
  return dispatch(ctx, [&](auto& im) { return im.get_state(phi, rho, alp); });
}
int pdhg_get_phi_bar(pdhg_ctx* ctx, double* phi_bar) {
  if (!phi_bar) return fail(PDHG_ERR_ARG, "null phi_bar");
  return dispatch(ctx, [&](auto& im) { return im.get_phi_bar(phi_bar); });
}
int pdhg_get_work(pdhg_ctx* ctx, double* out, long long count) {
  if (!out) return fail(PDHG_ERR_ARG, "null out");
  return dispatch(ctx, [&](auto& im) { return im.get_work(out, count < 0 ? 0 : (size_t)count); });
}
int pdhg_set_phi_bar(pdhg_ctx* ctx, const double* phi_bar) {
  if (!phi_bar) return fail(PDHG_ERR_ARG, "null phi_bar");
  return dispatch(ctx, [&](auto& im) { return im.set_phi_bar(phi_bar); });
}
int pdhg_get_rows(pdhg_ctx* ctx, int row0, int nrows, double* phi, double* phi_bar, double* rho, double* alp) {
  return dispatch(ctx, [&](auto& im) { return im.get_rows(row0, nrows, phi, phi_bar, rho, alp); });
}
int pdhg_init_state(pdhg_ctx* ctx, const double* g) {
  if (!g) return fail(PDHG_ERR_ARG, "null g");
  return dispatch(ctx, [&](auto& im) { return im.init_state(g); });
}
int pdhg_update_primal(pdhg_ctx* ctx, double tau) {
  return dispatch(ctx, [&](auto& im) { return im.update_primal(tau); });
}
int pdhg_update_dual(pdhg_ctx* ctx, double sigma, double eps, int rho_alp_iters, int* inner_used) {
  if (rho_alp_iters < 1) return fail(PDHG_ERR_ARG, "rho_alp_iters must be >= 1");
  return dispatch(ctx, [&](auto& im) { return im.update_dual(sigma, eps, rho_alp_iters, inner_used); });
}
int pdhg_errors(pdhg_ctx* ctx, double* err1, double* err2) {
  return dispatch(ctx, [&](auto& im) { return im.errors(err1, err2); });
}
int pdhg_inner_error(pdhg_ctx* ctx, double* err) {
  if (!err) return fail(PDHG_ERR_ARG, "null err");
  return dispatch(ctx, [&](auto& im) {
    Ctrl h;
    int rc = im.read_ctrl(h);
    if (rc) return rc;
    *err = h.err_inner;
    return (int)PDHG_OK;
  });
}
int pdhg_iterate(pdhg_ctx* ctx, int n_iters, double tau, double sigma, double eps, int rho_alp_iters,
                 pdhg_stats* out) {
  if (n_iters < 0 || rho_alp_iters < 1) return fail(PDHG_ERR_ARG, "bad iteration counts");
  return dispatch(ctx, [&](auto& im) { return im.iterate(n_iters, tau, sigma, eps, rho_alp_iters, out); });
}
int pdhg_set_stop_rules(pdhg_ctx* ctx, int stop_on_converge, int stop_on_nan) {
  return dispatch(ctx, [&](auto& im) {
    im.stop_conv = stop_on_converge ? 1 : 0;
    im.stop_nan = stop_on_nan ? 1 : 0;
    return (int)PDHG_OK;
  });
}
int pdhg_synchronize(pdhg_ctx* ctx) {
  return dispatch(ctx, [&](auto& im) {
    HIP_TRY(hipStreamSynchronize(im.stream));
    return (int)PDHG_OK;
  });
}
int pdhg_device_bytes(pdhg_ctx* ctx, unsigned long long* bytes) {
  if (!bytes) return fail(PDHG_ERR_ARG, "null bytes");
  return dispatch(ctx, [&](auto& im) {
    *bytes = im.dev_bytes;
    return (int)PDHG_OK;
  });
}
int pdhg_path_info(pdhg_ctx* ctx, const char* key, int* value) {
  if (!key || !value) return fail(PDHG_ERR_ARG, "null argument");
  return dispatch(ctx, [&](auto& im) {
    const std::string k(key);
    if (plan_key(im.pp, im.pb, (int)sizeof(RealOf<decltype(im)>), k, value)) return (int)PDHG_OK;   // creation-time keys
    if (k == "contig_fail") *value = im.n_contig_fail;
    else if (k == "spec_iters") *value = (int)std::min<long long>(im.spec_iters, INT_MAX);   // speculative iterations so
    else if (k == "spec_halts") *value = (int)std::min<long long>(im.spec_halts, INT_MAX);   // far, and halts (cumulative)
    else if (k == "graph") *value = im.use_graph ? 1 : 0;   // iteration windows replayed from a HIP graph
    else if (k == "graph_window") *value = im.gexec ? im.g_window : 0;   // 0: no graph captured yet
    else return fail(PDHG_ERR_ARG, "unknown path key %s", key);
    return (int)PDHG_OK;
  });
}
int pdhg_plan_info(const pdhg_problem* prob, const char* key, int* value) {
  if (!prob || !key || !value) return fail(PDHG_ERR_ARG, "null argument");
  int rc;
  if ((rc = validate_problem(*prob))) return rc;
  PathPlan pl;
  std::string why;
  Decomp dc{};
  dc.mixed = prob->precision == kMixedPrecision;
  const int S = dc.mixed ? 4 : prob->precision;   // a mixed context plans as fp32
  if ((rc = plan_paths(*prob, S, dc, Tuning::from_env(), pl, why))) return fail(rc, "%s", why.c_str());
  if (plan_key(pl, *prob, S, key, value)) return PDHG_OK;
  return fail(PDHG_ERR_ARG, "path key %s is unknown or a runtime counter of a context", key);
}
int pdhg_profile_enable(pdhg_ctx* ctx, int enable) {
  return dispatch(ctx, [&](auto& im) {
    HIP_TRY(hipStreamSynchronize(im.stream));
    im.prof = enable != 0;
    for (auto& kv : im.prof_ev) kv.second.used = 0;
    return (int)PDHG_OK;
  });
}
int pdhg_profile_query(pdhg_ctx* ctx, const char* cls, double* total_ms, int* launches) {
  if (!cls || !total_ms || !launches) return fail(PDHG_ERR_ARG, "null argument");
  return dispatch(ctx, [&](auto& im) {
    HIP_TRY(hipStreamSynchronize(im.stream));
    *total_ms = 0.0;
    *launches = 0;
    auto it = im.prof_ev.find(cls);
    if (it == im.prof_ev.end()) return (int)PDHG_OK;
    for (size_t i = 0; i < it->second.used; ++i) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, it->second.ev[i].first, it->second.ev[i].second));
      *total_ms += ms;
    }
    *launches = (int)it->second.used;
    return (int)PDHG_OK;
  });
}
int pdhg_algorithmic_bytes(pdhg_ctx* ctx, int k, const char* cls, double* bytes) {
  if (!cls || !bytes) return fail(PDHG_ERR_ARG, "null argument");
  return dispatch(ctx, [&](auto& im) {
    *bytes = im.algorithmic_bytes(k, cls);
    return *bytes < 0 ? fail(PDHG_ERR_ARG, "unknown kernel class %s", cls) : (int)PDHG_OK;
  });
}

/* ---------------- closed-loop trajectories ---------------- */
int pdhg_trajectories(pdhg_ctx* ctx, const pdhg_traj_opts* opts, const double* x_init, const double* noise,
                      double* x_final, double* traj_x, double* traj_alp) {
  if (ctx && reinterpret_cast<const CtxBox*>(ctx)->magic == kMultiMagic)
    return fail(PDHG_ERR_UNSUPPORTED, "trajectories need a single context (pdhg_create), not a multi-device one");
  if (!opts || !x_init) return fail(PDHG_ERR_ARG, "null opts or x_init");
  return dispatch(ctx, [&](auto& im) {
    const int rc = check_traj_opts(*opts, im.pb.ndim, false);
    return rc ? rc : im.trajectories(*opts, x_init, noise, x_final, traj_x, traj_alp);
  });
}

/* ---------------- policy check ---------------- */
int pdhg_policy_eval(pdhg_ctx* ctx, const pdhg_policy_opts* opts, const double* x_init, const double* noise,
                     pdhg_policy_report* report, double* running, double* terminal, double* value,
                     double* x_final) {
  if (!ctx || !opts) return fail(PDHG_ERR_ARG, "null context or opts");
  if (reinterpret_cast<const CtxBox*>(ctx)->magic == kMultiMagic)
    return fail(PDHG_ERR_UNSUPPORTED, "the policy check needs a single context (pdhg_create), not a multi-device one");
  const pdhg_traj_opts& o = opts->traj;
  if (opts->terminal != 0 && opts->terminal != 1)
    return fail(PDHG_ERR_ARG, "terminal %d: 0 phi row 0 at x_final or 1 none", opts->terminal);
  if (!report && !running && !terminal && !value && !x_final)
    return fail(PDHG_ERR_ARG, "report and every output are null: nothing to compute");
  return dispatch(ctx, [&](auto& im) {
    if (int rc = check_traj_opts(o, im.pb.ndim, !x_init)) return rc;
    if (!x_init && (opts->stride_x < 1 || (im.pb.ndim == 2 && opts->stride_y < 1)))
      return fail(PDHG_ERR_ARG, "grid starts need strides >= 1, not (%d, %d)", opts->stride_x, opts->stride_y);
    return im.policy_eval(*opts, x_init, noise, report, running, terminal, value, x_final);
  });
}

/* ---------------- solution report ---------------- */
int pdhg_report_state(pdhg_ctx* ctx, pdhg_report* out) {
  if (!ctx || !out) return fail(PDHG_ERR_ARG, "null context or report");
  if (reinterpret_cast<const CtxBox*>(ctx)->magic == kMultiMagic)
    return fail(PDHG_ERR_UNSUPPORTED, "the report needs a single context (pdhg_create), not a multi-device one");
  return dispatch(ctx, [&](auto& im) { return im.report_state(out); });
}
int pdhg_report_rows(pdhg_ctx* ctx, int row0, int nrows, double* hj, double* cont) {
  if (!ctx) return fail(PDHG_ERR_ARG, "null context");
  if (int rc = check_row_range(row0, nrows)) return rc;
  if (reinterpret_cast<const CtxBox*>(ctx)->magic == kMultiMagic)
    return fail(PDHG_ERR_UNSUPPORTED, "the report needs a single context (pdhg_create), not a multi-device one");
  return dispatch(ctx, [&](auto& im) { return im.report_rows(row0, nrows, hj, cont); });
}

/* ---------------- t-slab decomposition ---------------- */
int pdhg_create_slab(const pdhg_problem* prob, int j0, int T_total, int device, pdhg_ctx** out) {
  if (!prob || !out) return fail(PDHG_ERR_ARG, "null argument");
  *out = nullptr;
  if (j0 < 0 || prob->T < 1 || j0 + prob->T > T_total)
    return fail(PDHG_ERR_ARG, "slab rows [%d, %d) outside the window of %d rows", j0, j0 + prob->T, T_total);
  if (prob->ndim != 2) return fail(PDHG_ERR_UNSUPPORTED, "t-slab decomposition is 2-D only");
  if (prob->precision == kMixedPrecision)
    return fail(PDHG_ERR_UNSUPPORTED, "mixed precision (12) is implemented for single contexts only (no t-slab)");
  // validate the rest exactly like pdhg_create, then rebuild as a slab (fp32, or fp64 = the reference's arithmetic,
  // jaxsrc/update_fns_in_pdhg.py:10)
  pdhg_ctx* probe = nullptr;
  pdhg_problem q = *prob;
  q.T = 1;
  int rc = pdhg_create(&q, device, &probe);
  if (rc) return rc;
  pdhg_destroy(probe);
  auto box = std::make_unique<CtxBox>();
  box->precision = prob->precision;
  auto build = [&](auto tag) {
    using Rt = decltype(tag);
    auto im = std::make_unique<Impl<Rt>>();
    im->pb = *prob;
    im->device = device;
    im->slab = true;
    im->slab_j0 = j0;
    im->slab_Tg = T_total;
    const int r = im->setup();
    box->impl = std::move(im);
    return r;
  };
  rc = prob->precision == 8 ? build(0.0) : build(0.f);
  if (rc) return rc;
  *out = reinterpret_cast<pdhg_ctx*>(box.release());
  return PDHG_OK;
}

int pdhg_set_stream(pdhg_ctx* ctx, void* hip_stream) {   // null = the device's default stream
  return dispatch(ctx, [&](auto& im) { return im.set_stream(static_cast<hipStream_t>(hip_stream)); });
}
int pdhg_slab_begin(pdhg_ctx* ctx) {
  return phase_dispatch(ctx, [&](auto& im) { return im.reset_ctrl(); });
}
int pdhg_slab_carry_gain(pdhg_ctx* ctx, void* GS_out) {
  if (!GS_out) return fail(PDHG_ERR_ARG, "null plane");
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_G(static_cast<RealOf<decltype(im)>*>(GS_out)); });
}
int pdhg_slab_residual(pdhg_ctx* ctx, int parts) {
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_residual(parts); });
}
int pdhg_slab_forward(pdhg_ctx* ctx, double tau) {
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_forward((RealOf<decltype(im)>)tau); });
}
int pdhg_slab_fixup(pdhg_ctx* ctx, const void* all_DS, const void* all_GS, int rank, int nranks) {
  if (!all_DS || !all_GS) return fail(PDHG_ERR_ARG, "null carry planes");
  if (rank < 0 || rank >= nranks) return fail(PDHG_ERR_ARG, "rank %d of %d", rank, nranks);
  return slab_dispatch(ctx, [&](auto& im) {
    return im.slab_fixup(static_cast<const RealOf<decltype(im)>*>(all_DS), static_cast<const RealOf<decltype(im)>*>(all_GS), rank, nranks);
  });
}
int pdhg_slab_long_modes(pdhg_ctx* ctx, const void* all_GS, int nranks, double delta, int* K) {
  if (!all_GS || !K || nranks < 1) return fail(PDHG_ERR_ARG, "null plane / count or nranks < 1");
  return slab_dispatch(ctx, [&](auto& im) {
    return im.slab_long_modes(static_cast<const RealOf<decltype(im)>*>(all_GS), nranks, delta, K);
  });
}
int pdhg_slab_fixup_nb(pdhg_ctx* ctx, const void* D_left, const void* S1_right, const void* all_long,
                       const void* all_GS, int rank, int nranks) {
  if (!D_left || !S1_right || !all_GS || rank < 0 || rank >= nranks)
    return fail(PDHG_ERR_ARG, "null plane or rank %d outside [0, %d)", rank, nranks);
  return slab_dispatch(ctx, [&](auto& im) {
    return im.slab_fixup_nb(static_cast<const RealOf<decltype(im)>*>(D_left), static_cast<const RealOf<decltype(im)>*>(S1_right),
                            static_cast<const RealOf<decltype(im)>*>(all_long), static_cast<const RealOf<decltype(im)>*>(all_GS), rank, nranks);
  });
}
int pdhg_slab_backward(pdhg_ctx* ctx, double tau, double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_backward((RealOf<decltype(im)>)tau, sums); });
}
int pdhg_slab_primal_finalize(pdhg_ctx* ctx, const double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return phase_dispatch(ctx, [&](auto& im) { return im.slab_primal_finalize(sums); });
}
int pdhg_slab_dual(pdhg_ctx* ctx, double sigma, int rho_alp_iters, int sub, double* sums, int parts) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return phase_dispatch(ctx, [&](auto& im) { return im.slab_dual((RealOf<decltype(im)>)sigma, rho_alp_iters, sub, sums, parts); });
}
int pdhg_slab_dual_finalize(pdhg_ctx* ctx, double eps, int sub, const double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return phase_dispatch(ctx, [&](auto& im) { return im.slab_dual_finalize(eps, sub, sums); });
}
int pdhg_slab_outer(pdhg_ctx* ctx, int rho_alp_iters, double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return phase_dispatch(ctx, [&](auto& im) { return im.slab_outer(rho_alp_iters, sums); });
}
int pdhg_slab_outer_finalize(pdhg_ctx* ctx, double eps, int rho_alp_iters, const double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return phase_dispatch(ctx, [&](auto& im) { return im.slab_outer_finalize(eps, rho_alp_iters, sums); });
}
int pdhg_slab_plane_out(pdhg_ctx* ctx, int which, void* dst) {
  if (!dst) return fail(PDHG_ERR_ARG, "null plane");
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_plane_out(which, dst); });
}
int pdhg_slab_plane_in(pdhg_ctx* ctx, int which, const void* src) {
  if (!src) return fail(PDHG_ERR_ARG, "null plane");
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_plane_in(which, src); });
}
/* the report and the rollout on a t-slab: the pieces pdhg_multi_report_state / _report_rows / _trajectories and
 * pdhg_amd.slab.SlabRunner.report chain across slabs */
int pdhg_slab_report(pdhg_ctx* ctx, const void* phi_prev_rowT, double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_report(phi_prev_rowT, sums); });
}
int pdhg_slab_report_rows(pdhg_ctx* ctx, const void* phi_prev_rowT, int row0_local, int nrows, double* d_hj,
                          double* d_cont) {
  if (int rc = check_row_range(row0_local, nrows)) return rc;
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_report_rows(phi_prev_rowT, row0_local, nrows, d_hj, d_cont); });
}
int pdhg_slab_trajectories(pdhg_ctx* ctx, const pdhg_traj_opts* opts, int step0, long long n, const double* d_x_in,
                           const double* d_noise, double* d_x_out, double* d_rec_x, double* d_rec_a) {
  if (!opts || !d_x_in || !d_x_out) return fail(PDHG_ERR_ARG, "null opts, x_in or x_out");
  if (n < 1 || step0 < 0) return fail(PDHG_ERR_ARG, "n must be >= 1 and step0 >= 0");
  pdhg_traj_opts o = *opts;
  o.n_sample = n;   // the samples of this launch (opts->n_sample is not read); a t-slab is always 2-D
  if (int rc = check_traj_opts(o, 2, false)) return rc;
  return slab_dispatch(ctx, [&](auto& im) {
    if (step0 > im.slab_Tg - im.slab_j0 - im.pb.T)
      return fail(PDHG_ERR_ARG, "step0 %d: the slabs after this one hold %d rows", step0, im.slab_Tg - im.slab_j0 - im.pb.T);
    return im.slab_trajectories(o, step0, (unsigned long long)n, d_x_in, d_noise, d_x_out, d_rec_x, d_rec_a);
  });
}
int pdhg_slab_status(pdhg_ctx* ctx, pdhg_stats* st) {
  if (!st) return fail(PDHG_ERR_ARG, "null stats");
  return phase_dispatch(ctx, [&](auto& im) { return im.slab_status(st); });
}
int pdhg_slab_plane_size(pdhg_ctx* ctx, unsigned long long* spatial, unsigned long long* spectral) {
  if (!spatial || !spectral) return fail(PDHG_ERR_ARG, "null argument");
  return slab_dispatch(ctx, [&](auto& im) {
    *spatial = im.plane();
    *spectral = im.Mspec;
    return (int)PDHG_OK;
  });
}

/* ---------------- x-slab decomposition ---------------- */
int pdhg_create_xslab(const pdhg_problem* prob, int rank, int nranks, int device, pdhg_ctx** out) {
  if (!prob || !out) return fail(PDHG_ERR_ARG, "null argument");
  *out = nullptr;
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PDHG_ERR_ARG, "rank %d of %d", rank, nranks);
  if (prob->ndim != 2) return fail(PDHG_ERR_UNSUPPORTED, "x-slab decomposition is 2-D only");
  if (prob->precision == kMixedPrecision)
    return fail(PDHG_ERR_UNSUPPORTED, "mixed precision (12) is implemented for single contexts only (no x-slab)");
  // bc (0,0), or egno 3's (1,0): Neumann x edges -- the first / last slab's outer ghost row replicates its own edge
  // row (nb_index bc 1), the transposed x lines take the DCT of the generic x kernel
  if (prob->bc_y != 0 || (prob->bc_x != 0 && prob->bc_x != 1))
    return fail(PDHG_ERR_UNSUPPORTED, "x-slab decomposition needs bc (0,0) or (1,0)");
  if (prob->nx % nranks || (prob->nx / nranks) % 8)
    return fail(PDHG_ERR_UNSUPPORTED, "nx=%d must split into %d slabs of a multiple of 8 rows", prob->nx, nranks);
  // validate the rest exactly like pdhg_create (one row of the global grid), then build the slab
  pdhg_ctx* probe = nullptr;
  pdhg_problem q = *prob;
  q.T = 1;
  int rc = pdhg_create(&q, device, &probe);
  if (rc) return rc;
  pdhg_destroy(probe);
  const int nloc = prob->nx / nranks, nxl = nloc + 16, x0 = rank * nloc;
  auto box = std::make_unique<CtxBox>();
  box->precision = prob->precision;
  // fp32, or fp64 = the reference's arithmetic (jaxsrc/update_fns_in_pdhg.py:10): the x-slab kernels, the fp64 row
  // kernels (ny = 2048 / 4096) and the fp64 duals honour the live-row bounds; the column blocks go through the
  // generic x kernel
  auto build = [&](auto tag) {
    using Rt = decltype(tag);
    auto im = std::make_unique<Impl<Rt>>();
    im->xslab = true;
    im->xs_rank = rank;
    im->xs_P = nranks;
    im->xs_nxg = prob->nx;
    im->xs_nloc = nloc;
    im->xs_x0 = x0;
    im->xs_local.resize(nxl);
    for (int i = 0; i < nxl; ++i) {   // local row i = global row x0 - 8 + i (periodic; clamped at Neumann edges)
      const int gi = x0 - 8 + i;
      const int g = prob->bc_x == 1 ? std::min(std::max(gi, 0), prob->nx - 1) : ((gi % prob->nx) + prob->nx) % prob->nx;
      im->xs_local[i] = prob->xs[g];
    }
    im->pb = *prob;
    im->pb.nx = nxl;
    im->pb.xs = im->xs_local.data();
    im->device = device;
    const int r = im->setup();
    box->impl = std::move(im);
    return r;
  };
  rc = prob->precision == 8 ? build(0.0) : build(0.f);
  if (rc) return rc;
  *out = reinterpret_cast<pdhg_ctx*>(box.release());
  return PDHG_OK;
}
int pdhg_xslab_layout(pdhg_ctx* ctx, int* x0, int* nloc, int* nx_local, int* xl0) {
  if (!x0 || !nloc || !nx_local || !xl0) return fail(PDHG_ERR_ARG, "null argument");
  return xslab_dispatch(ctx, [&](auto& im) {
    *x0 = im.xs_x0;
    *nloc = im.xs_nloc;
    *nx_local = im.pb.nx;
    *xl0 = im.kp.xl0;
    return (int)PDHG_OK;
  });
}
int pdhg_xslab_sizes(pdhg_ctx* ctx, unsigned long long* wire, unsigned long long* halo_state,
                     unsigned long long* halo_phibar) {
  if (!wire || !halo_state || !halo_phibar) return fail(PDHG_ERR_ARG, "null argument");
  return xslab_dispatch(ctx, [&](auto& im) {
    *wire = im.xs_chunk() * im.xs_P;
    *halo_state = im.xs_halo_elems(0);
    *halo_phibar = im.xs_halo_elems(1);
    return (int)PDHG_OK;
  });
}
int pdhg_xslab_halo_out(pdhg_ctx* ctx, int which, void* dst) {
  if (!dst) return fail(PDHG_ERR_ARG, "null buffer");
  return xslab_dispatch(ctx, [&](auto& im) { return im.xs_halo_out(which, dst); });
}
int pdhg_xslab_halo_in(pdhg_ctx* ctx, int which, const void* from_left, const void* from_right) {
  if (!from_left || !from_right) return fail(PDHG_ERR_ARG, "null buffer");
  return xslab_dispatch(ctx, [&](auto& im) { return im.xs_halo_in(which, from_left, from_right); });
}
int pdhg_xslab_residual(pdhg_ctx* ctx) {
  return xslab_dispatch(ctx, [&](auto& im) { return im.xs_residual(); });
}
int pdhg_xslab_wire(pdhg_ctx* ctx, int stage, void* buf) {
  if (!buf) return fail(PDHG_ERR_ARG, "null buffer");
  return xslab_dispatch(ctx, [&](auto& im) { return im.xs_wire(stage, buf); });
}
int pdhg_xslab_precond(pdhg_ctx* ctx) {
  return xslab_dispatch(ctx, [&](auto& im) { return im.xs_precond(); });
}
int pdhg_xslab_update(pdhg_ctx* ctx, double tau, double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return xslab_dispatch(ctx, [&](auto& im) { return im.xs_update((RealOf<decltype(im)>)tau, sums); });
}

int pdhg_slab_part_modes(pdhg_ctx* ctx, int part, int nparts, unsigned long long* m0, unsigned long long* m1) {
  if (!m0 || !m1 || nparts < 1 || part < 0 || part >= nparts) return fail(PDHG_ERR_ARG, "part %d of %d", part, nparts);
  return slab_dispatch(ctx, [&](auto& im) {
    int b0, b1;
    size_t a, b;
    im.part_range(part, nparts, b0, b1, a, b);
    *m0 = a;
    *m1 = b;
    return (int)PDHG_OK;
  });
}
int pdhg_slab_forward_part(pdhg_ctx* ctx, double tau, int part, int nparts) {
  if (nparts < 1 || part < 0 || part >= nparts) return fail(PDHG_ERR_ARG, "part %d of %d", part, nparts);
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_forward_part((RealOf<decltype(im)>)tau, part, nparts); });
}
int pdhg_slab_carry_out_part(pdhg_ctx* ctx, void* dst, int part, int nparts) {
  if (!dst || nparts < 1 || part < 0 || part >= nparts) return fail(PDHG_ERR_ARG, "null plane or part %d of %d", part, nparts);
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_carry_out_part(dst, part, nparts); });
}
int pdhg_slab_fixup_nb_part(pdhg_ctx* ctx, const void* D_left, const void* S1_right, const void* all_long,
                            const void* all_GS, int rank, int nranks, int part, int nparts) {
  if (!D_left || !S1_right || !all_GS || rank < 0 || rank >= nranks || nparts < 1 || part < 0 || part >= nparts)
    return fail(PDHG_ERR_ARG, "null plane, rank %d of %d or part %d of %d", rank, nranks, part, nparts);
  return slab_dispatch(ctx, [&](auto& im) {
    return im.slab_fixup_nb(static_cast<const RealOf<decltype(im)>*>(D_left), static_cast<const RealOf<decltype(im)>*>(S1_right),
                            static_cast<const RealOf<decltype(im)>*>(all_long), static_cast<const RealOf<decltype(im)>*>(all_GS), rank, nranks,
                            part, nparts);
  });
}
int pdhg_slab_backward_part(pdhg_ctx* ctx, double tau, int part, int nparts) {
  if (nparts < 1 || part < 0 || part >= nparts) return fail(PDHG_ERR_ARG, "part %d of %d", part, nparts);
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_backward_part((RealOf<decltype(im)>)tau, part, nparts); });
}
int pdhg_slab_update(pdhg_ctx* ctx, double tau, double* sums) {
  if (!sums) return fail(PDHG_ERR_ARG, "null sums");
  return slab_dispatch(ctx, [&](auto& im) { return im.slab_update((RealOf<decltype(im)>)tau, sums); });
}

}  // extern "C"

#include "pdhg_multi.hpp"   // multi-device context over the t-slab entry points above
