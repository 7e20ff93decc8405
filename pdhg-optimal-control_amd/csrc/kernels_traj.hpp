// Closed-loop trajectory rollout from the resident controls (jaxsrc/run_example.py:18-155, used at :342-393):
//   dx = f(alp(x, t), x, t) dt + sqrt(2 epsl) dW,   explicit Euler-Maruyama over the window's T rows.
// One thread per sample, the time loop inside the kernel: samples are independent, so there is no barrier and no
// LDS.  Step ind reads alp row T-1-ind (the PDE runs backward from the terminal cost: the reference's alp[:, ::-1],
// run_example.py:347).  Positions, weights and the update are fp64 in every context precision (the work is a
// handful of gathers per step; the arithmetic is free); alp is read in the type the context stores it.
//
// The interpolation restates oracle/traj_oracle.py point-wise.  Discrete choices (cell, nearest node, sign split of
// f) must fall as they do on the host, so the position arithmetic is compiled without fma contraction and in the
// oracle's operation order.
//
// One time step is one function, traj_step_1d / traj_step_2d, called by the rollout and by the policy check
// (kernels_policy.hpp): their paths are the same bits by construction.  Two things keep the bits when this text is
// edited.  `#pragma clang fp contract(off)` is lexical: every helper carries it in its own body, or the compiler may
// fuse across its statements.  And the build has no fast-math, so with contraction off an fp64 result is fixed by its
// expression tree, not by scheduling or registers: keep the operand order of the weights and sums, and widen R / P to
// double before any arithmetic.  The generated code may change; the results may not.
//
// Noise: a staged array of standard normals [T][n][ndim], or Philox4x32-10 + Box-Muller on the device:
//   key     = (seed low word, seed high word)
//   counter = (sample low word, sample high word, step, axis pair)        sample = global sample index
//   r0..r3  = Philox4x32-10(counter, key)
//   u1 = (((r0 << 32 | r1) >> 11) + 1) * 2^-53   in (0, 1]
//   u2 =  ((r2 << 32 | r3) >> 11)      * 2^-53   in [0, 1)
//   z(axis 2p) = sqrt(-2 ln u1) cos(2 pi u2),  z(axis 2p+1) = sqrt(-2 ln u1) sin(2 pi u2)
// a pure function of (seed, sample, step, axis): independent of the launch shape and of the chunking.
//
// A t-slab (pdhg_slab_trajectories) marches its own T rows of a longer rollout: local step ind is global step
// step0 + ind -- the Philox step word, the row of a staged noise array and the row of the records, which are the
// whole rollout's arrays.  step0 = 0 on a context that holds the whole window.
#pragma once
#include "params.hpp"

namespace pdhg {

template <typename R>
struct TrajP {
  int nx, ny, T;
  int step0;                 // global step of local step 0 (t-slab: the rows of the rollout already marched)
  int bcx;                   // 0 periodic, 1 Neumann (edge value outside the grid); y is periodic
  int method;                // 0 linear, 1 nearest
  int center_x, center_y;    // the period cell is [-P/2, P/2) instead of [0, P)
  int noise_mode;            // 0 none (epsl = 0), 1 staged array, 2 Philox on the device
  unsigned long long n;      // samples of this launch
  unsigned long long s0;     // global index of this launch's sample 0 (Philox counter)
  unsigned long long seed;
  double Px, Py, dt, sq;     // periods, time step, sqrt(2 epsl dt)
  double inv_dx, inv_dy;
  const double* xs;          // [nx] grid coordinates in fp64
  const double* ys;          // [ny]
  const R* alp[2][4];        // both buffer sets; the kernel picks ctrl->cur
  const Ctrl* ctrl;
  const double* x_in;        // [n][ndim]
  const double* noise;       // [steps][n][ndim] by global step (noise_mode 1)
  double* x_out;             // [n][ndim]
  double* rec_x;             // [steps+1][n][ndim] by global step, or null; row 0 is written where step0 == 0
  double* rec_a;             // [steps][n][n_ctrl] by global step, or null
};

// ---- Philox4x32-10 (Salmon et al., SC'11) ----
struct Philox4 {
  uint32_t v[4];
};
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                          uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the two standard normals of (seed, sample, step, axis pair)
__device__ __forceinline__ void traj_normals(unsigned long long seed, unsigned long long sample, int step, int pair,
                                             double& z0, double& z1) {
#pragma clang fp contract(off)
  const Philox4 r = philox4x32_10((uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)step, (uint32_t)pair,
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t a = ((uint64_t)r.v[0] << 32) | r.v[1], b = ((uint64_t)r.v[2] << 32) | r.v[3];
  const double u1 = (double)((a >> 11) + 1) * 0x1.0p-53, u2 = (double)(b >> 11) * 0x1.0p-53;
  const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
  z0 = rad * cos(ang);
  z1 = rad * sin(ang);
}

// Python's x % P for P > 0: fmod, moved into [0, P)
__device__ __forceinline__ double traj_pmod(double x, double P) {
#pragma clang fp contract(off)
  double m = fmod(x, P);
  if (m < 0.0) m += P;
  return m;
}

// a(x) = (x - 1)^2 + 0.1, the f coefficient of egno 1 / 2 (set_fns.py:117-118, :145) at a sample position
__device__ __forceinline__ double traj_coef(double x) {
#pragma clang fp contract(off)
  const double d = x - 1.0;
  return d * d + 0.1;
}

// One axis of the point-wise boundary extension (extend_bdry_2d, run_example.py:54-114, as
// traj_oracle.VirtualExtension): copy k of the grid has its nodes at g[j] + k P.  The cell holding x is
// [lo, hi] = nodes (k, j) and (k, j+1) -- or (k+1, 0) after the last node; u = (x - lo) / (hi - lo); j0 / j1 are the
// grid indices whose values stand at the two nodes: wrapped on a periodic axis, the edge index outside copy 0 on a
// Neumann axis.  Indices are clamped to [0, n): no position (NaN and infinities included) reads outside the grid.
struct TrajCell {
  int j0, j1;
  double u;
};
__device__ __forceinline__ TrajCell traj_locate(double x, const double* __restrict__ g, int n, double P, double inv_h,
                                                int bc, int center) {
#pragma clang fp contract(off)
  double k = floor(x / P + (center ? 0.5 : 0.0));   // the reference's copy index (lb / ub of extend_bdry_2d)
  if (x < g[0] + k * P) k -= 1.0;                   // below the copy's first node: the previous copy's last cell
  else if (x > g[0] + (k + 1.0) * P) k += 1.0;
  const double base = k * P;
  const double jf = fmin(fmax((x - (g[0] + base)) * inv_h, 0.0), (double)(n - 1));   // fmax drops a NaN
  int j = (int)jf;
  while (j > 0 && x < g[j] + base) --j;             // the grid is ascending: exact for any spacing
  while (j < n - 1 && x > g[j + 1] + base) ++j;
  const double lo = g[j] + base, hi = (j + 1 < n) ? g[j + 1] + base : g[0] + (k + 1.0) * P;
  TrajCell c;
  c.u = (x - lo) / (hi - lo);
  if (bc == 0) {
    c.j0 = j;
    c.j1 = (j + 1 < n) ? j + 1 : 0;
  } else if (k == 0.0) {
    c.j0 = j;
    c.j1 = (j + 1 < n) ? j + 1 : n - 1;
  } else {
    c.j0 = c.j1 = (k < 0.0) ? 0 : n - 1;
  }
  return c;
}

// Bilinear value on two cells from the corners v = (00, 10, 01, 11), first index x: the four weights and the sum in
// this operand order, corners widened before any arithmetic.  Callers load every corner (of every array) first.
template <typename V>
__device__ __forceinline__ double traj_bilinear(const TrajCell& cx, const TrajCell& cy, const V (&v)[4]) {
#pragma clang fp contract(off)
  const double u = cx.u, w = cy.u;
  const double w00 = (1.0 - u) * (1.0 - w), w10 = u * (1.0 - w), w01 = (1.0 - u) * w, w11 = u * w;
  return w00 * (double)v[0] + w10 * (double)v[1] + w01 * (double)v[2] + w11 * (double)v[3];
}

// 1-D linear cell of xm = x mod P (jnp.interp(period=P), run_example.py:18-52): the cell before node 0 (from the last
// node of the previous period) and after node n-1 (to node 0 of the next) closes the period; u is the weight of j1
__device__ __forceinline__ TrajCell traj_cell_1d(double xm, const double* __restrict__ g, int n, double P,
                                                 double inv_h) {
#pragma clang fp contract(off)
  int j = (int)fmin(fmax((xm - g[0]) * inv_h, 0.0), (double)(n - 1));
  while (j > 0 && xm < g[j]) --j;
  while (j < n - 1 && xm > g[j + 1]) ++j;
  const bool before = xm < g[0], after = j + 1 >= n;
  const double lo = before ? g[n - 1] - P : g[j];
  const double hi = before ? g[0] : after ? g[0] + P : g[j + 1];
  TrajCell c;
  c.j0 = before ? n - 1 : j;
  c.j1 = before || after ? 0 : j + 1;
  c.u = hi > lo ? (xm - lo) / (hi - lo) : 0.0;
  return c;
}

// ---- one time step of one sample: the only text of the marching arithmetic (k_traj_*, k_policy_*) ----
// Local step ind of launch sample s: locates the cell(s), reads or draws the noise, interpolates the arrays A by
// p.method into al[], forms f[k] = fval(al[k], coef) and advances the position in two roundings: x + v dt, + sq nz.
// 2-D: alp arrays 0, 1 drive x (a1x for f >= 0, a2x for f < 0), 2, 3 drive y; egno 3 stores 0, 1 only (set_fns.py:98).
template <typename R, int EGNO, int NA>
__device__ __forceinline__ void traj_step_2d(const TrajP<R>& p, const R* const __restrict__ (&A)[NA], int ind,
                                             unsigned long long s, double& x, double& y, double (&al)[NA],
                                             double (&f)[NA]) {
#pragma clang fp contract(off)
  const size_t row = (size_t)(p.T - 1 - ind) * ((size_t)p.nx * (size_t)p.ny);
  const int step = p.step0 + ind;
  const TrajCell cx = traj_locate(x, p.xs, p.nx, p.Px, p.inv_dx, p.bcx, p.center_x);
  const TrajCell cy = traj_locate(y, p.ys, p.ny, p.Py, p.inv_dy, 0, p.center_y);
  double nz0 = 0.0, nz1 = 0.0;
  if (p.noise_mode == 1) {
    const size_t o = ((size_t)step * p.n + s) * 2;
    nz0 = p.noise[o];
    nz1 = p.noise[o + 1];
  }
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
#pragma unroll
    for (int a = 0; a < NA; ++a) al[a] = traj_bilinear(cx, cy, v[a]);
  }
  if (p.noise_mode == 2) traj_normals(p.seed, p.s0 + s, step, 0, nz0, nz1);
  // f sees x mod P on a periodic axis and the raw coordinate on a Neumann axis (run_example.py:139-145)
  const double xf = p.bcx == 0 ? traj_pmod(x, p.Px) : x;
  double ax = 0.0, ay = 0.0;   // egno 3: f = (alp, x) takes no coefficient, and y drifts with x
  if constexpr (EGNO != 3) ax = traj_coef(xf), ay = traj_coef(traj_pmod(y, p.Py));
#pragma unroll
  for (int a = 0; a < NA; ++a) f[a] = fval<double, EGNO>(al[a], a < 2 ? ax : ay);
  const double vx = fpos(f[0]) + fneg(f[1]);
  const double vy = EGNO == 3 ? fpos(xf) + fneg(xf) : fpos(f[NA - 2]) + fneg(f[NA - 1]);
  x = x + vx * p.dt;
  y = y + vy * p.dt;
  if (p.noise_mode) {
    x = x + p.sq * nz0;
    y = y + p.sq * nz1;
  }
}

// 1-D (compute_traj_1d, run_example.py:18-52).  The grid is the reference's: ascending in [0, P).
//   linear : traj_cell_1d;
//   nearest: argmin |x_arr - x mod P|, first index on ties, with no wrap: past the last node's midpoint to the
//            period's end it stays the last node.
template <typename R, int EGNO>
__device__ __forceinline__ void traj_step_1d(const TrajP<R>& p, const R* __restrict__ A0, const R* __restrict__ A1,
                                             int ind, unsigned long long s, double& x, double (&al)[2],
                                             double (&f)[2]) {
#pragma clang fp contract(off)
  const int n = p.nx;
  const double* __restrict__ g = p.xs;
  const size_t row = (size_t)(p.T - 1 - ind) * (size_t)n;
  const int step = p.step0 + ind;
  const double xm = traj_pmod(x, p.Px);
  double nz = 0.0, nz_unused;
  if (p.noise_mode == 1) nz = p.noise[(size_t)step * p.n + s];
  if (p.method == 1) {
    int j = (int)fmin(fmax((xm - g[0]) * p.inv_dx, 0.0), (double)(n - 1));
    while (j > 0 && fabs(g[j - 1] - xm) <= fabs(g[j] - xm)) --j;      // ties: the first index
    while (j < n - 1 && fabs(g[j + 1] - xm) < fabs(g[j] - xm)) ++j;
    const R v1 = A0[row + j], v2 = A1[row + j];
    al[0] = (double)v1;
    al[1] = (double)v2;
  } else {
    const TrajCell c = traj_cell_1d(xm, g, n, p.Px, p.inv_dx);
    const R v10 = A0[row + c.j0], v11 = A0[row + c.j1], v20 = A1[row + c.j0], v21 = A1[row + c.j1];
    al[0] = (double)v10 + c.u * ((double)v11 - (double)v10);
    al[1] = (double)v20 + c.u * ((double)v21 - (double)v20);
  }
  if (p.noise_mode == 2) traj_normals(p.seed, p.s0 + s, step, 0, nz, nz_unused);
  const double a = traj_coef(xm);
  f[0] = fval<double, EGNO>(al[0], a);
  f[1] = fval<double, EGNO>(al[1], a);
  const double vel = fpos(f[0]) + fneg(f[1]);
  x = x + vel * p.dt;
  if (p.noise_mode) x = x + p.sq * nz;
}

// The rollout: start, the step loop and the records, [step][sample][...] so that a wave's stores are contiguous.
template <typename R, int EGNO>
__global__ void __launch_bounds__(256) k_traj_2d(TrajP<R> p) {
#pragma clang fp contract(off)
  const unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= p.n) return;
  constexpr int NA = EGNO == 3 ? 2 : 4, NC = EGNO == 3 ? 1 : 2;
  const int cur = p.ctrl->cur;
  const R* __restrict__ A[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) A[a] = cur ? p.alp[1][a] : p.alp[0][a];   // no dynamic index into the argument block
  double x = p.x_in[2 * s], y = p.x_in[2 * s + 1];
  if (p.rec_x && p.step0 == 0) {
    p.rec_x[2 * s] = x;
    p.rec_x[2 * s + 1] = y;
  }
  for (int ind = 0; ind < p.T; ++ind) {
    const int step = p.step0 + ind;
    double al[NA], f[NA];
    traj_step_2d<R, EGNO>(p, A, ind, s, x, y, al, f);
    if (p.rec_a) {
      double* ra = p.rec_a + ((size_t)step * p.n + s) * NC;
      ra[0] = al[0] + al[1];
      if constexpr (NC == 2) ra[1] = al[2] + al[3];
    }
    if (p.rec_x) {
      double* rx = p.rec_x + ((size_t)(step + 1) * p.n + s) * 2;
      rx[0] = x;
      rx[1] = y;
    }
  }
  p.x_out[2 * s] = x;
  p.x_out[2 * s + 1] = y;
}

template <typename R, int EGNO>
__global__ void __launch_bounds__(256) k_traj_1d(TrajP<R> p) {
#pragma clang fp contract(off)
  const unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= p.n) return;
  const int cur = p.ctrl->cur;
  const R* __restrict__ A0 = cur ? p.alp[1][0] : p.alp[0][0];
  const R* __restrict__ A1 = cur ? p.alp[1][1] : p.alp[0][1];
  double x = p.x_in[s];
  if (p.rec_x && p.step0 == 0) p.rec_x[s] = x;
  for (int ind = 0; ind < p.T; ++ind) {
    const int step = p.step0 + ind;
    double al[2], f[2];
    traj_step_1d<R, EGNO>(p, A0, A1, ind, s, x, al, f);
    if (p.rec_a) p.rec_a[(size_t)step * p.n + s] = al[0] + al[1];
    if (p.rec_x) p.rec_x[(size_t)(step + 1) * p.n + s] = x;
  }
  p.x_out[s] = x;
}

}  // namespace pdhg
