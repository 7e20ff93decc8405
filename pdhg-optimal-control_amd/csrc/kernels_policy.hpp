// Policy check (include/pdhg.h pdhg_policy_eval): does following the resident feedback alp cost what phi says?
// phi row 0 is the terminal cost g, row j the value with j dt to go, and the controls of row j act between phi rows
// j and j+1, so for a path started at x0 with T rows to go the window's dynamic-programming identity is
//   sum_steps dt L(alp(x, t)) + phi_0(x_T)  ~  phi_T(x0)          (in expectation when epsl > 0).
// One thread per sample, the time loop inside, as k_traj_*: the path is the rollout's own -- the same helpers
// (traj_locate, traj_pmod, traj_coef, traj_normals of kernels_traj.hpp), the same statements in the same order,
// compiled without fma contraction -- so x_final equals pdhg_trajectories' bit for bit.  Beside the path a sample
// carries
//   value    = I_lin[phi row T](x0)
//   running  = running + dt * l  per step,  l = sum_k keep_k lag(a_k a_k)  over the interpolated control arrays a_k,
//              keep_k the rollout's sign split of f_k = fval(a_k, coef): f >= 0 for arrays 0 / 2, f < 0 for 1 / 3
//              (a component the split drops moves nothing and costs nothing)
//   terminal = I_lin[phi row 0](x_T), or 0.0 (PolP::terminal == 1)
// I_lin is linear interpolation with the rollout's cell location and extension, whatever method the controls use;
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

// bilinear phi at the cells traj_locate found, weights formed as k_traj_2d forms them
template <typename P>
__device__ __forceinline__ double pol_phi_2d(const P* __restrict__ f, const TrajCell& cx, const TrajCell& cy, int ny) {
#pragma clang fp contract(off)
  const P v00 = f[(size_t)cx.j0 * ny + cy.j0], v10 = f[(size_t)cx.j1 * ny + cy.j0];
  const P v01 = f[(size_t)cx.j0 * ny + cy.j1], v11 = f[(size_t)cx.j1 * ny + cy.j1];
  const double u = cx.u, w = cy.u;
  const double w00 = (1.0 - u) * (1.0 - w), w10 = u * (1.0 - w), w01 = (1.0 - u) * w, w11 = u * w;
  return w00 * (double)v00 + w10 * (double)v10 + w01 * (double)v01 + w11 * (double)v11;
}

// 1-D phi by the linear branch of k_traj_1d: the cell before node 0 and after node n-1 closes the period
template <typename P>
__device__ __forceinline__ double pol_phi_1d(const P* __restrict__ f, const double* __restrict__ g, int n, double Px,
                                             double inv_dx, double x) {
#pragma clang fp contract(off)
  const double xm = traj_pmod(x, Px);
  int j = (int)fmin(fmax((xm - g[0]) * inv_dx, 0.0), (double)(n - 1));
  while (j > 0 && xm < g[j]) --j;
  while (j < n - 1 && xm > g[j + 1]) ++j;
  int j0 = j, j1 = j + 1;
  double lo = g[j], hi;
  if (xm < g[0]) {
    j0 = n - 1;
    j1 = 0;
    lo = g[n - 1] - Px;
    hi = g[0];
  } else if (j1 < n) {
    hi = g[j1];
  } else {
    j1 = 0;
    hi = g[0] + Px;
  }
  const P v0 = f[j0], v1 = f[j1];
  const double w = hi > lo ? (xm - lo) / (hi - lo) : 0.0;
  return (double)v0 + w * ((double)v1 - (double)v0);
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
    const size_t npl = (size_t)p.nx * (size_t)p.ny;
    double x, y;
    if (q.grid_starts) {
      const unsigned long long g = q.g0 + s;
      x = p.xs[(size_t)(g / q.gny) * q.stride_x];
      y = p.ys[(size_t)(g % q.gny) * q.stride_y];
    } else {
      x = p.x_in[2 * s];
      y = p.x_in[2 * s + 1];
    }
    {
      const TrajCell cx = traj_locate(x, p.xs, p.nx, p.Px, p.inv_dx, p.bcx, p.center_x);
      const TrajCell cy = traj_locate(y, p.ys, p.ny, p.Py, p.inv_dy, 0, p.center_y);
      value = pol_phi_2d(q.phi + (size_t)p.T * npl, cx, cy, p.ny);
    }
    for (int ind = 0; ind < p.T; ++ind) {
      const size_t row = (size_t)(p.T - 1 - ind) * npl;
      const int step = p.step0 + ind;
      const TrajCell cx = traj_locate(x, p.xs, p.nx, p.Px, p.inv_dx, p.bcx, p.center_x);
      const TrajCell cy = traj_locate(y, p.ys, p.ny, p.Py, p.inv_dy, 0, p.center_y);
      double nz0 = 0.0, nz1 = 0.0;
      if (p.noise_mode == 1) {
        const size_t o = ((size_t)step * p.n + s) * 2;
        nz0 = p.noise[o];
        nz1 = p.noise[o + 1];
      }
      double al[NA];
      if (p.method == 1) {   // nearest node per axis, ties to the lower node
        const size_t o = row + (size_t)(cx.u > 0.5 ? cx.j1 : cx.j0) * p.ny + (size_t)(cy.u > 0.5 ? cy.j1 : cy.j0);
        R v[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) v[a] = A[a][o];
#pragma unroll
        for (int a = 0; a < NA; ++a) al[a] = (double)v[a];
      } else {               // bilinear: every corner of every array is loaded before the first use
        const size_t o00 = row + (size_t)cx.j0 * p.ny + cy.j0, o10 = row + (size_t)cx.j1 * p.ny + cy.j0;
        const size_t o01 = row + (size_t)cx.j0 * p.ny + cy.j1, o11 = row + (size_t)cx.j1 * p.ny + cy.j1;
        R v[NA][4];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          v[a][0] = A[a][o00];
          v[a][1] = A[a][o10];
          v[a][2] = A[a][o01];
          v[a][3] = A[a][o11];
        }
        const double u = cx.u, w = cy.u;
        const double w00 = (1.0 - u) * (1.0 - w), w10 = u * (1.0 - w), w01 = (1.0 - u) * w, w11 = u * w;
#pragma unroll
        for (int a = 0; a < NA; ++a)
          al[a] = w00 * (double)v[a][0] + w10 * (double)v[a][1] + w01 * (double)v[a][2] + w11 * (double)v[a][3];
      }
      if (p.noise_mode == 2) traj_normals(p.seed, p.s0 + s, step, 0, nz0, nz1);
      // f sees x mod P on a periodic axis and the raw coordinate on a Neumann axis, as in the rollout
      const double xf = p.bcx == 0 ? traj_pmod(x, p.Px) : x;
      double vx, vy, l;
      if constexpr (EGNO == 3) {
        const double f0 = fval<double, 3>(al[0], 0.0), f1 = fval<double, 3>(al[1], 0.0);
        vx = fpos(f0) + fneg(f1);
        vy = fpos(xf) + fneg(xf);
        l = pol_cost<3>(al[0], f0, true) + pol_cost<3>(al[1], f1, false);
      } else {
        const double ax = traj_coef(xf), ay = traj_coef(traj_pmod(y, p.Py));
        const double f0 = fval<double, EGNO>(al[0], ax), f1 = fval<double, EGNO>(al[1], ax);
        const double f2 = fval<double, EGNO>(al[2], ay), f3 = fval<double, EGNO>(al[3], ay);
        vx = fpos(f0) + fneg(f1);
        vy = fpos(f2) + fneg(f3);
        l = pol_cost<EGNO>(al[0], f0, true) + pol_cost<EGNO>(al[1], f1, false);
        l = l + pol_cost<EGNO>(al[2], f2, true);
        l = l + pol_cost<EGNO>(al[3], f3, false);
      }
      running = running + p.dt * l;
      x = x + vx * p.dt;
      y = y + vy * p.dt;
      if (p.noise_mode) {
        x = x + p.sq * nz0;
        y = y + p.sq * nz1;
      }
    }
    if (q.terminal == 0) {
      const TrajCell cx = traj_locate(x, p.xs, p.nx, p.Px, p.inv_dx, p.bcx, p.center_x);
      const TrajCell cy = traj_locate(y, p.ys, p.ny, p.Py, p.inv_dy, 0, p.center_y);
      term = pol_phi_2d(q.phi, cx, cy, p.ny);
    }
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
    const int cur = p.ctrl->cur, n = p.nx;
    const R* __restrict__ A0 = cur ? p.alp[1][0] : p.alp[0][0];
    const R* __restrict__ A1 = cur ? p.alp[1][1] : p.alp[0][1];
    const double* __restrict__ g = p.xs;
    double x = q.grid_starts ? g[(size_t)(q.g0 + s) * q.stride_x] : p.x_in[s];
    value = pol_phi_1d(q.phi + (size_t)p.T * (size_t)n, g, n, p.Px, p.inv_dx, x);
    for (int ind = 0; ind < p.T; ++ind) {
      const size_t row = (size_t)(p.T - 1 - ind) * (size_t)n;
      const int step = p.step0 + ind;
      const double xm = traj_pmod(x, p.Px);
      double nz = 0.0, nz_unused;
      if (p.noise_mode == 1) nz = p.noise[(size_t)step * p.n + s];
      int j = (int)fmin(fmax((xm - g[0]) * p.inv_dx, 0.0), (double)(n - 1));
      double a1, a2;
      if (p.method == 1) {
        while (j > 0 && fabs(g[j - 1] - xm) <= fabs(g[j] - xm)) --j;      // ties: the first index
        while (j < n - 1 && fabs(g[j + 1] - xm) < fabs(g[j] - xm)) ++j;
        const R v1 = A0[row + j], v2 = A1[row + j];
        a1 = (double)v1;
        a2 = (double)v2;
      } else {
        while (j > 0 && xm < g[j]) --j;
        while (j < n - 1 && xm > g[j + 1]) ++j;
        int j0 = j, j1 = j + 1;
        double lo = g[j], hi;
        if (xm < g[0]) {          // before node 0: from the last node of the previous period
          j0 = n - 1;
          j1 = 0;
          lo = g[n - 1] - p.Px;
          hi = g[0];
        } else if (j1 < n) {
          hi = g[j1];
        } else {                  // after the last node: to node 0 of the next period
          j1 = 0;
          hi = g[0] + p.Px;
        }
        const R v10 = A0[row + j0], v11 = A0[row + j1], v20 = A1[row + j0], v21 = A1[row + j1];
        const double w = hi > lo ? (xm - lo) / (hi - lo) : 0.0;
        a1 = (double)v10 + w * ((double)v11 - (double)v10);
        a2 = (double)v20 + w * ((double)v21 - (double)v20);
      }
      if (p.noise_mode == 2) traj_normals(p.seed, p.s0 + s, step, 0, nz, nz_unused);
      const double a = traj_coef(xm);
      const double f1 = fval<double, EGNO>(a1, a), f2 = fval<double, EGNO>(a2, a);
      const double vel = fpos(f1) + fneg(f2);
      const double l = pol_cost<EGNO>(a1, f1, true) + pol_cost<EGNO>(a2, f2, false);
      running = running + p.dt * l;
      x = x + vel * p.dt;
      if (p.noise_mode) x = x + p.sq * nz;
    }
    if (q.terminal == 0) term = pol_phi_1d(q.phi, g, n, p.Px, p.inv_dx, x);
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
