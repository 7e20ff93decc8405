// Policy check (include/pdhg.h pdhg_policy_eval): does following the resident feedback alp cost what phi says?
// phi row 0 is the terminal cost g, row j the value with j dt to go, and the controls of row j act between phi rows
// j and j+1, so for a path started at x0 with T rows to go the window's dynamic-programming identity is
//   sum_steps dt L(alp(x, t)) + phi_0(x_T)  ~  phi_T(x0)          (in expectation when epsl > 0).
// One thread per sample, the time loop inside, as k_traj_*: the path is the rollout's own -- each step is the same
// function, traj_step_1d / traj_step_2d of kernels_traj.hpp, which also hands back the interpolated controls a_k and
// f_k -- so x_final equals pdhg_trajectories' bit for bit.  Beside the path a sample carries
//   value    = I_lin[phi row T](x0)
//   running  = running + dt * l  per step,  l = sum_k keep_k lag(a_k a_k)  over the interpolated control arrays a_k,
//              keep_k the rollout's sign split of f_k = fval(a_k, coef): f >= 0 for arrays 0 / 2, f < 0 for 1 / 3
//              (a component the split drops moves nothing and costs nothing)
//   terminal = I_lin[phi row 0](x_T), or 0.0 (PolP::terminal == 1)
// I_lin is linear interpolation on the rollout's cells with its weights, whatever method the controls use;
// phi is read in the type the context stores it (P) and widened before any arithmetic.
//
// Reduction without atomics: a workgroup folds its 256 samples in block_reduce_store_report's fixed order into row
// g0 / 256 + blockIdx.x of the partial table -- the workgroup's number in the whole call, not in the chunk -- and
// k_report_finalize folds the table after the last chunk: the result does not depend on the chunk staging.
//   sums    [0] running  [1] terminal  [2] value  [3] gap  [4] |gap|  [5] gap^2  [6] non-finite samples (any of
//           running, terminal, value not finite; left out of everything else)  [7] cost
//   extrema [8] max |gap|  [9] max gap  [10] max -gap  [11..15] unused (-inf)
// with cost = running + terminal, gap = cost - value.
#pragma once
#include "kernels_report.hpp"
#include "kernels_traj.hpp"

namespace pdhg {

template <typename R, typename P>
struct PolP {
  TrajP<R> t;                // the rollout's block; x_in is null with grid starts, x_out may be null, records unused
  const P* phi;              // [T+1][nx][ny]
  int terminal;              // 0: phi row 0 at x_final, 1: none
  int grid_starts;           // sample g starts at node (xs[(g / gny) stride_x], ys[(g % gny) stride_y])
  int stride_x, stride_y;
  unsigned long long gny;    // ceil(ny / stride_y); 1 in 1-D
  unsigned long long g0;     // index in the call of this launch's sample 0 (a multiple of 256)
  double* running;           // [n] each, or null
  double* term;
  double* value;
  double* partials;          // [workgroups of the call][kNumSums]
};

// one sample into the workgroup's row; threads past the launch's last sample add nothing
__device__ __forceinline__ void pol_accum(RepAcc& a, bool live, double running, double term, double value) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < kRepSums; ++i) {
    a.s[i] = 0.0;
    a.m[i] = -__builtin_huge_val();
  }
  a.m[0] = 0.0;
  if (!live) return;
  if (!(rep_finite(running) && rep_finite(term) && rep_finite(value))) {
    a.s[6] = 1.0;
    return;
  }
  const double cost = running + term;
  const double gap = cost - value;
  a.s[0] = running;
  a.s[1] = term;
  a.s[2] = value;
  a.s[3] = gap;
  a.s[4] = fabs(gap);
  a.s[5] = gap * gap;
  a.s[7] = cost;
  a.m[0] = fabs(gap);
  a.m[1] = gap;
  a.m[2] = -gap;
}

// I_lin[f](x, y): bilinear on the rollout's cells
template <typename R, typename P>
__device__ __forceinline__ double pol_phi_2d(const TrajP<R>& p, const P* __restrict__ f, double x, double y) {
#pragma clang fp contract(off)
  const TrajCell cx = traj_locate(x, p.xs, p.nx, p.Px, p.inv_dx, p.bcx, p.center_x);
  const TrajCell cy = traj_locate(y, p.ys, p.ny, p.Py, p.inv_dy, 0, p.center_y);
  const P v[4] = {f[(size_t)cx.j0 * p.ny + cy.j0], f[(size_t)cx.j1 * p.ny + cy.j0],
                  f[(size_t)cx.j0 * p.ny + cy.j1], f[(size_t)cx.j1 * p.ny + cy.j1]};
  return traj_bilinear(cx, cy, v);
}

// I_lin[f](x) in 1-D: the rollout's linear cell
template <typename R, typename P>
__device__ __forceinline__ double pol_phi_1d(const TrajP<R>& p, const P* __restrict__ f, double x) {
#pragma clang fp contract(off)
  const TrajCell c = traj_cell_1d(traj_pmod(x, p.Px), p.xs, p.nx, p.Px, p.inv_dx);
  const P v0 = f[c.j0], v1 = f[c.j1];
  return (double)v0 + c.u * ((double)v1 - (double)v0);
}

// the step cost of one control array: keep * L(a^2)
template <int EGNO>
__device__ __forceinline__ double pol_cost(double a, double f, bool right) {
#pragma clang fp contract(off)
  const bool keep = right ? (f >= 0.0) : (f < 0.0);
  return (keep ? 1.0 : 0.0) * lag<double, EGNO>(a * a);
}

template <typename R, typename P, int EGNO>
__global__ void __launch_bounds__(256) k_policy_2d(PolP<R, P> q) {
#pragma clang fp contract(off)
  const TrajP<R>& p = q.t;
  const unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s < p.n;
  constexpr int NA = EGNO == 3 ? 2 : 4;
  double running = 0.0, term = 0.0, value = 0.0;
  if (live) {
    const int cur = p.ctrl->cur;
    const R* __restrict__ A[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) A[a] = cur ? p.alp[1][a] : p.alp[0][a];
    double x, y;
    if (q.grid_starts) {
      const unsigned long long g = q.g0 + s;
      x = p.xs[(size_t)(g / q.gny) * q.stride_x];
      y = p.ys[(size_t)(g % q.gny) * q.stride_y];
    } else {
      x = p.x_in[2 * s];
      y = p.x_in[2 * s + 1];
    }
    value = pol_phi_2d(p, q.phi + (size_t)p.T * ((size_t)p.nx * (size_t)p.ny), x, y);
    for (int ind = 0; ind < p.T; ++ind) {
      double al[NA], f[NA];
      traj_step_2d<R, EGNO>(p, A, ind, s, x, y, al, f);
      double l = pol_cost<EGNO>(al[0], f[0], true) + pol_cost<EGNO>(al[1], f[1], false);
      if constexpr (NA == 4) l = (l + pol_cost<EGNO>(al[2], f[2], true)) + pol_cost<EGNO>(al[3], f[3], false);
      running = running + p.dt * l;
    }
    if (q.terminal == 0) term = pol_phi_2d(p, q.phi, x, y);
    if (p.x_out) {
      p.x_out[2 * s] = x;
      p.x_out[2 * s + 1] = y;
    }
    if (q.running) q.running[s] = running;
    if (q.term) q.term[s] = term;
    if (q.value) q.value[s] = value;
  }
  RepAcc acc;
  pol_accum(acc, live, running, term, value);
  block_reduce_store_report(acc, q.partials, (int)(q.g0 / 256 + blockIdx.x));
}

template <typename R, typename P, int EGNO>
__global__ void __launch_bounds__(256) k_policy_1d(PolP<R, P> q) {
#pragma clang fp contract(off)
  const TrajP<R>& p = q.t;
  const unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s < p.n;
  double running = 0.0, term = 0.0, value = 0.0;
  if (live) {
    const int cur = p.ctrl->cur;
    const R* __restrict__ A0 = cur ? p.alp[1][0] : p.alp[0][0];
    const R* __restrict__ A1 = cur ? p.alp[1][1] : p.alp[0][1];
    double x = q.grid_starts ? p.xs[(size_t)(q.g0 + s) * q.stride_x] : p.x_in[s];
    value = pol_phi_1d(p, q.phi + (size_t)p.T * (size_t)p.nx, x);
    for (int ind = 0; ind < p.T; ++ind) {
      double al[2], f[2];
      traj_step_1d<R, EGNO>(p, A0, A1, ind, s, x, al, f);
      const double l = pol_cost<EGNO>(al[0], f[0], true) + pol_cost<EGNO>(al[1], f[1], false);
      running = running + p.dt * l;
    }
    if (q.terminal == 0) term = pol_phi_1d(p, q.phi, x);
    if (p.x_out) p.x_out[s] = x;
    if (q.running) q.running[s] = running;
    if (q.term) q.term[s] = term;
    if (q.value) q.value[s] = value;
  }
  RepAcc acc;
  pol_accum(acc, live, running, term, value);
  block_reduce_store_report(acc, q.partials, (int)(q.g0 / 256 + blockIdx.x));
}

}  // namespace pdhg
