// Solution report (include/pdhg.h: pdhg_report_state / pdhg_report_rows): one read-only pass over the resident
// state that forms, at every point (j, x, y), j = 0..T-1,
//   r = HJ residual row j           Dt phi - eps Lap phi - f(alp) . D phi - L(alp)   (update_fns_in_pdhg.py:49-70)
//   c = continuity residual row j+1 of the reference's [T+1] array                   (update_fns_in_pdhg.py:72-96)
// from phi (not phi_bar) and the current rho / alp set, with the iteration's own device functions (dual_pre, fval,
// fpos, fneg, lag, cont_residual_*), and reduces them with rho row j and phi row j+1 into one row of kNumSums
// doubles per workgroup:
//   sums    [0] sum |r|  [1] sum r^2  [2] sum rho |r|  [3] sum rho  [4] sum |c|  [5] sum c^2
//           [6] non-finite points (any of r, c, rho, phi not finite; left out of everything else)  [7] points rho == 0
//   extrema [8] max |r|  [9] max max(r, 0)  [10] max |r| where rho > 0  [11] max |c|
//           [12] max rho  [13] max -rho  [14] max phi  [15] max -phi
// k_report_finalize folds the rows in a fixed order (sums added, extrema maximised; no atomics).  Nothing the
// iteration reads is written: the table is the report's own (RepP::partials, not KP::partials).
//
//   k_report_2d / k_report_1d   one thread per point, neighbours through nb_index: any shape and bc
//   k_report_tile_2d            8 rows x (64 YPL) columns per workgroup marching over t (nx % 8 == 0, ny % 256 == 0,
//                               bc_y periodic, bc_x periodic or Neumann): every array is read once per point
// A t-slab (KP::slab, rows [j0, j0 + T) of Tg; pdhg_slab_report) holds two of a pass's planes elsewhere: rho row T is
// the next slab's rho row 0 (KP::rho_halo, delivered by the caller; zero on the window's last slab, which alone adds
// c_on_rho / dt) and, for j0 > 0, phi row 0 is the previous slab's phi row T: the iteration maintains phi_bar row 0
// only, so it is read from RepP::phi_halo, a plane the report owns, never written into the slab's phi.
#pragma once
#include <type_traits>
#include "kernels_1d.hpp"
#include "kernels_2d.hpp"
#include "kernels_2d_fast.hpp"

namespace pdhg {

constexpr int kRepSums = 8;   // sums, then as many extrema: one kNumSums row
static_assert(2 * kRepSums == kNumSums, "one partial row");

struct RepP {
  int j0, j1;         // time rows [j0, j1) of this launch
  int jchunk;         // tile kernel: rows per workgroup along t (blockIdx.z)
  double* hj;         // [j1 - j0][nx][ny] field rows, or null
  double* cont;       // likewise
  double* partials;   // [workgroups][kNumSums]
  const void* phi_halo;   // t-slab with KP::j0 > 0: phi row 0 (the previous slab's phi row T) [nx][ny] in phi's type
};

struct RepAcc {
  double s[kRepSums], m[kRepSums];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < kRepSums; ++i) s[i] = 0.0;
    // maxima of non-negative quantities start at 0 (no point with rho > 0: hj_active_max = 0); ranges at -inf
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = 0.0;
#pragma unroll
    for (int i = 4; i < kRepSums; ++i) m[i] = -__builtin_huge_val();
  }
};

__device__ __forceinline__ bool rep_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

template <typename R, typename P>
__device__ __forceinline__ void rep_accum(RepAcc& a, R r, R c, R rho, P phi) {
  const double rd = (double)r, cd = (double)c, rh = (double)rho, ph = (double)phi;
  if (!(rep_finite(rd) && rep_finite(cd) && rep_finite(rh) && rep_finite(ph))) {
    a.s[6] += 1.0;
    return;
  }
  const double ar = fabs(rd), ac = fabs(cd);
  a.s[0] += ar;
  a.s[1] += rd * rd;
  a.s[2] += rh * ar;
  a.s[3] += rh;
  a.s[4] += ac;
  a.s[5] += cd * cd;
  if (rh == 0.0) a.s[7] += 1.0;
  a.m[0] = fmax(a.m[0], ar);
  a.m[1] = fmax(a.m[1], rd);
  if (rh > 0.0) a.m[2] = fmax(a.m[2], ar);
  a.m[3] = fmax(a.m[3], ac);
  a.m[4] = fmax(a.m[4], rh);
  a.m[5] = fmax(a.m[5], -rh);
  a.m[6] = fmax(a.m[6], ph);
  a.m[7] = fmax(a.m[7], -ph);
}

// block_reduce_store's sibling for a report row: the sums added, the extrema maximised, both in fixed order
__device__ __forceinline__ void block_reduce_store_report(RepAcc& a, double* __restrict__ partials, int row) {
  __shared__ double red[16][kNumSums];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x >> 6;
  const int nw = (blockDim.x + kWave - 1) >> 6;
#pragma unroll
  for (int i = 0; i < kRepSums; ++i) {
    double x = a.s[i], y = a.m[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      x += __shfl_xor(x, o, kWave);
      y = fmax(y, __shfl_xor(y, o, kWave));
    }
    a.s[i] = x;
    a.m[i] = y;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kRepSums; ++i) {
      red[wid][i] = a.s[i];
      red[wid][kRepSums + i] = a.m[i];
    }
  }
  __syncthreads();
  if (threadIdx.x < kNumSums) {
    double acc = red[0][threadIdx.x];
    for (int w = 1; w < nw; ++w)
      acc = threadIdx.x < kRepSums ? acc + red[w][threadIdx.x] : fmax(acc, red[w][threadIdx.x]);
    partials[(size_t)row * kNumSums + threadIdx.x] = acc;
  }
  __syncthreads();
}

// one workgroup of 1024: thread t folds column t % 16 of rows t / 16, t / 16 + 64, ..., then column c's 64 partial
// results are folded by thread c, both in fixed order
__global__ void __launch_bounds__(1024) k_report_finalize(const double* __restrict__ partials, int nrows,
                                                         double* __restrict__ out) {
  __shared__ double red[64][kNumSums];
  const int c = threadIdx.x & (kNumSums - 1), g = threadIdx.x >> 4;
  const bool sum = c < kRepSums;
  double acc = sum ? 0.0 : -__builtin_huge_val();
  for (int r = g; r < nrows; r += 64) {
    const double v = partials[(size_t)r * kNumSums + c];
    acc = sum ? acc + v : fmax(acc, v);
  }
  red[g][c] = acc;
  __syncthreads();
  if (threadIdx.x < kNumSums) {
    double t = red[0][c];
    for (int i = 1; i < 64; ++i) t = sum ? t + red[i][c] : fmax(t, red[i][c]);
    out[c] = t;
  }
}

// HJ residual at one point from phi row j+1 at (x, y) (pc), its 4 neighbours and row j (f0c): the one-sided
// differences and the time / eps terms as dual_pre forms them (a mixed context: in double on the PhiX reciprocals,
// rounded to float once, as dual_point_x), then the f and L terms of the stored controls `a`
template <typename R, int EGNO, typename P>
__device__ __forceinline__ R hj_point(const KP<R>& p, const PhiX<R, P>& px, P pc, P pxm, P pxp, P pym, P pyp, P f0c,
                                      const R* a, R axc, R ayc) {
  DualPre<R> d;
  if constexpr (std::is_same<R, P>::value) {
    d = dual_pre<R>(p, pc, pxm, pxp, pym, pyp, f0c);
  } else {
    const DualPre<P> dd = dual_pre<P>(px, pc, pxm, pxp, pym, pyp, f0c);
    d = DualPre<R>{(R)dd.DxR, (R)dd.DxL, (R)dd.DyR, (R)dd.DyL, (R)dd.vec0};
  }
  const R f1x = fpos<R>(fval<R, EGNO>(a[0], axc));
  const R f2x = fneg<R>(fval<R, EGNO>(a[1], axc));
  R f1y, f2y, L;
  if constexpr (EGNO == 3) {
    f1y = fpos<R>(axc);
    f2y = fneg<R>(axc);
    L = lag<R, EGNO>(a[0] * a[0]) + lag<R, EGNO>(a[1] * a[1]);
  } else {
    f1y = fpos<R>(fval<R, EGNO>(a[2], ayc));
    f2y = fneg<R>(fval<R, EGNO>(a[3], ayc));
    L = lag<R, EGNO>(a[0] * a[0]) + lag<R, EGNO>(a[1] * a[1]) + lag<R, EGNO>(a[2] * a[2]) +
        lag<R, EGNO>(a[3] * a[3]);
  }
  R vec = d.vec0 - (d.DxR * f1x + d.DxL * f2x + d.DyR * f1y + d.DyL * f2y);
  return vec - L;
}

// grid: (ceil(ny/256), G), the G workgroup rows striding over the (j1 - j0) * nx (j, x) rows; block 256
template <typename R, int EGNO, typename P>
__global__ void __launch_bounds__(256) k_report_2d(KP<R> p, PhiX<R, P> px, RepP rp) {
  constexpr int NA = (EGNO == 3) ? 2 : 4;
  const int cur = p.ctrl->cur;
  const R* rho = p.rho[cur];
  const R* alp[4] = {p.alp[cur][0], p.alp[cur][1], p.alp[cur][2], p.alp[cur][3]};
  const int nx = p.nx, ny = p.ny;
  const size_t plane = (size_t)nx * ny;
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  const int ym = nb_index(y - 1, ny, p.bcy), yp = nb_index(y + 1, ny, p.bcy);
  const R ayc = (y < ny) ? p.ay[y] : (R)0;
  const P* phi = phi_of(p, px);
  RepAcc acc;
  acc.init();
  const int row1 = rp.j1 * nx;
  for (int row = rp.j0 * nx + blockIdx.y; row < row1 && y < ny; row += gridDim.y) {
    const int j = row / nx;
    const int x = row - j * nx;
    const size_t c = (size_t)x * ny + y;
    const P* f1 = phi + (size_t)(j + 1) * plane;
    const P* f0 = (j == 0 && p.j0 > 0) ? static_cast<const P*>(rp.phi_halo) : phi + (size_t)j * plane;
    const int xm = nb_index(x - 1, nx, p.bcx), xp = nb_index(x + 1, nx, p.bcx);
    const P pc = f1[c];
    const P pxm = (xm >= 0) ? f1[(size_t)xm * ny + y] : (P)0;
    const P pxp = (xp >= 0) ? f1[(size_t)xp * ny + y] : (P)0;
    const P pym = (ym >= 0) ? f1[(size_t)x * ny + ym] : (P)0;
    const P pyp = (yp >= 0) ? f1[(size_t)x * ny + yp] : (P)0;
    const size_t o = (size_t)j * plane + c;
    R a[4];
#pragma unroll
    for (int i = 0; i < NA; ++i) a[i] = alp[i][o];
    const R r = hj_point<R, EGNO, P>(p, px, pc, pxm, pxp, pym, pyp, f0[c], a, p.ax[x], ayc);
    const R cr = cont_residual_2d<R, EGNO>(p, rho, alp, j, x, y);
    rep_accum<R, P>(acc, r, cr, rho[o], pc);
    const size_t oo = (size_t)(j - rp.j0) * plane + c;
    if (rp.hj) rp.hj[oo] = (double)r;
    if (rp.cont) rp.cont[oo] = (double)cr;
  }
  block_reduce_store_report(acc, rp.partials, blockIdx.y * gridDim.x + blockIdx.x);
}

// grid: (ceil(nx/256), G) striding over the time rows [j0, j1); block 256
template <typename R, int EGNO>
__global__ void __launch_bounds__(256) k_report_1d(KP<R> p, RepP rp) {
  const int cur = p.ctrl->cur;
  const R* rho = p.rho[cur];
  const R* a1 = p.alp[cur][0];
  const R* a2 = p.alp[cur][1];
  const int nx = p.nx;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  RepAcc acc;
  acc.init();
  if (x < nx) {
    const int xm = nb_index(x - 1, nx, p.bcx), xp = nb_index(x + 1, nx, p.bcx);
    const R a = p.ax[x];
    for (int j = rp.j0 + blockIdx.y; j < rp.j1; j += gridDim.y) {
      const R* f1 = p.phi + (size_t)(j + 1) * nx;
      const R* f0 = p.phi + (size_t)j * nx;
      const R pc = f1[x];
      const R pxm = (xm >= 0) ? f1[xm] : (R)0;
      const R pxp = (xp >= 0) ? f1[xp] : (R)0;
      const R DxR = (pxp - pc) * p.inv_dx;
      const R DxL = (pc - pxm) * p.inv_dx;
      const size_t o = (size_t)j * nx + x;
      const R b1 = a1[o], b2 = a2[o];
      const R f1v = fpos<R>(fval<R, EGNO>(b1, a));
      const R f2v = fneg<R>(fval<R, EGNO>(b2, a));
      const R L = lag<R, EGNO>(b1 * b1) + lag<R, EGNO>(b2 * b2);
      R vec = (pc - f0[x]) * p.inv_dt;
      if (p.epsl != (R)0) vec = vec - p.epsl * ((pxp + pxm - (R)2 * pc) * p.inv_dx2);
      vec = vec - (DxR * f1v + DxL * f2v);
      vec = vec - L;
      const R cr = cont_residual_1d<R, EGNO>(p, rho, a1, a2, j, x);
      rep_accum<R, R>(acc, vec, cr, rho[o], pc);
      const size_t oo = (size_t)(j - rp.j0) * nx + x;
      if (rp.hj) rp.hj[oo] = (double)vec;
      if (rp.cont) rp.cont[oo] = (double)cr;
    }
  }
  block_reduce_store_report(acc, rp.partials, blockIdx.y * gridDim.x + blockIdx.x);
}

// The hot path.  grid (nx/8, ny/(64 YPL), Z); block 512 = 8 waves: wave r owns row x0 + r and 64 YPL consecutive y
// (YPL per lane, 16-B loads), workgroup z marches rows [j0 + z jchunk, ...) of the launch.
//   per step j a lane loads phi row j+1, rho row j+1 and the alp rows j at its own points; phi row j+1 is the next
//   step's row j and rho row j+1 the next step's rho (kept in registers), so each array is read once;
//   y -/+ 1: the adjacent lanes (DPP wave shifts); the strip's two outer columns: one scalar load each;
//   x -/+ 1: the rows of phi, rho and the x fluxes m1x = (rho+1e-4) f+(a1x), m2x = (rho+1e-4) f-(a2x) go through LDS;
//            the tile's halo rows x0-1 / x0+8 (wrapped when periodic, clamped when Neumann: nb_index) are loaded and
//            their flux formed by the first / last wave.
// The loads of step j+1 are issued before step j's values are used and are taken over at the end of the step; the
// barriers wait for LDS only (lds_sync), so those loads stay in flight across them.
template <typename R, int EGNO, int YPL, typename P>
__global__ void __launch_bounds__(512) k_report_tile_2d(KP<R> p, PhiX<R, P> px, RepP rp) {
  constexpr int RX = 8;
  constexpr int NA = (EGNO == 3) ? 2 : 4;
  constexpr int YW = 64 * YPL;
  using VP = VY<P, YPL>;
  using VR = VY<R, YPL>;
  __shared__ __align__(16) VP sphi[RX + 2][64];   // phi row j+1 of rows x0-1 .. x0+8
  __shared__ __align__(16) VR srho[RX + 2][64];   // rho row j likewise
  __shared__ __align__(16) VR sm1[RX + 1][64];    // m1x of rows x0-1 .. x0+7
  __shared__ __align__(16) VR sm2[RX + 1][64];    // m2x of rows x0 .. x0+8
  const int cur_set = p.ctrl->cur;
  const int nx = p.nx, ny = p.ny, T = p.T;
  const size_t plane = (size_t)nx * ny;
  const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int x0 = blockIdx.x * RX, x = x0 + r;
  const int y = blockIdx.y * YW + YPL * lane;
  const int j0 = rp.j0 + blockIdx.z * rp.jchunk;
  const int j1 = min(rp.j1, j0 + rp.jchunk);
  const bool has_h = (r == 0) || (r == RX - 1);                                       // wave-uniform
  const int xh = (r == 0) ? nb_index(x0 - 1, nx, p.bcx) : nb_index(x0 + RX, nx, p.bcx);   // bc_x 0 / 1: never -1
  const size_t rxc = (size_t)x * ny, rxh = (size_t)xh * ny;
  const int hslot = (r == 0) ? 0 : RX + 1;
  const int yw0 = blockIdx.y * YW;
  const int ywm = (yw0 == 0) ? ny - 1 : yw0 - 1, ywp = (yw0 + YW == ny) ? 0 : yw0 + YW;   // bc_y periodic
  const VR ay4 = ldy<YPL>(p.ay + y);
  const R axc = p.ax[x], axh = p.ax[xh];
  const R aym = p.ay[ywm], ayp = p.ay[ywp];
  const P* phi = phi_of(p, px);
  const R* rho = p.rho[cur_set];
  const R* al[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) al[a] = p.alp[cur_set][a];
  const bool use_eps = p.epsl != (R)0;
  struct Rho {   // a rho row at this lane's points, the halo row's (edge waves) and the strip's outer columns
    VR c, h;
    R el, er;
  };
  struct In {
    VP pc, ph;   // phi row j+1: own points, halo row
    P pel, per;  // ... the strip's outer columns
    Rho rn;      // rho row j+1 (zero past the window)
    VR a[NA], ah;   // alp rows j; halo row: a1x (first wave) or a2x (last wave)
    R ael, aer;     // a1y at column ywm, a2y at column ywp (egno 1 / 2)
  };
  auto load_rho = [&](int j) {
    Rho q;
    if (j < T || !p.last_slab) {   // uniform; row T of a slab: the next slab's row 0
      const R* rj = (j < T) ? rho + (size_t)j * plane : p.rho_halo;
      q.c = ldy<YPL>(rj + rxc + y);
      q.h = has_h ? ldy<YPL>(rj + rxh + y) : zy<R, YPL>();
      q.el = rj[rxc + ywm];
      q.er = rj[rxc + ywp];
    } else {   // the window's rho_T = 0 (Dt_increasedim)
      q.c = q.h = zy<R, YPL>();
      q.el = q.er = (R)0;
    }
    return q;
  };
  auto load = [&](int j) {
    In in;
    const P* f1 = phi + (size_t)(j + 1) * plane;
    in.pc = ldy<YPL>(f1 + rxc + y);
    in.ph = has_h ? ldy<YPL>(f1 + rxh + y) : zy<P, YPL>();
    in.pel = f1[rxc + ywm];
    in.per = f1[rxc + ywp];
    in.rn = load_rho(j + 1);
    const size_t o = (size_t)j * plane;
#pragma unroll
    for (int a = 0; a < NA; ++a) in.a[a] = ldy<YPL>(al[a] + o + rxc + y);
    in.ah = has_h ? ldy<YPL>(al[r == 0 ? 0 : 1] + o + rxh + y) : zy<R, YPL>();
    if constexpr (EGNO != 3) {
      in.ael = al[2][o + rxc + ywm];
      in.aer = al[3][o + rxc + ywp];
    } else {
      in.ael = in.aer = (R)0;
    }
    return in;
  };
  RepAcc acc;
  acc.init();
  if (j0 < j1) {
    // phi row j; a slab's row 0 from the report's halo plane (uniform)
    const P* f0p = (j0 == 0 && p.j0 > 0) ? static_cast<const P*>(rp.phi_halo) : phi + (size_t)j0 * plane;
    VP f0 = ldy<YPL>(f0p + rxc + y);
    Rho rj = load_rho(j0);                                  // rho row j
    In cur = load(j0), nxt = cur;
    // One loop body for every step: a row's values do not depend on where its step falls in a workgroup's chunk
    // (two inlined copies of the body, one per register set, were contracted differently by the compiler: the rows of
    // a range that cut the window elsewhere differed in the last bit).
#pragma unroll 1
    for (int j = j0; j < j1; ++j) {
      if (j + 1 < j1) nxt = load(j + 1);   // uniform; in flight across this step
      // ---- this row's x fluxes and rows into LDS ----
      VR m1x, m2x;
      R m1y[YPL], m2y[YPL];
#pragma unroll
      for (int e = 0; e < YPL; ++e) {
        const R r0 = f4(rj.c, e);
        f4set(m1x, e, m1f<EGNO, R>(r0, f4(cur.a[0], e), axc));
        f4set(m2x, e, m2f<EGNO, R>(r0, f4(cur.a[1], e), axc));
        if constexpr (EGNO == 3) {   // f_y = the x coordinate for both y controls
          m1y[e] = (r0 + (R)1e-4) * fpos<R>(axc);
          m2y[e] = (r0 + (R)1e-4) * fneg<R>(axc);
        } else {
          m1y[e] = m1f<EGNO, R>(r0, f4(cur.a[2], e), f4(ay4, e));
          m2y[e] = m2f<EGNO, R>(r0, f4(cur.a[3], e), f4(ay4, e));
        }
      }
      sphi[r + 1][lane] = cur.pc;
      srho[r + 1][lane] = rj.c;
      sm1[r + 1][lane] = m1x;
      sm2[r][lane] = m2x;
      if (has_h) {
        VR mh;
#pragma unroll
        for (int e = 0; e < YPL; ++e)
          f4set(mh, e, r == 0 ? m1f<EGNO, R>(f4(rj.h, e), f4(cur.ah, e), axh)
                              : m2f<EGNO, R>(f4(rj.h, e), f4(cur.ah, e), axh));
        sphi[hslot][lane] = cur.ph;
        srho[hslot][lane] = rj.h;
        if (r == 0) sm1[0][lane] = mh;
        else sm2[RX][lane] = mh;
      }
      lds_sync();
      const VP pm = sphi[r][lane], pp = sphi[r + 2][lane];
      const VR rm = srho[r][lane], rpl = srho[r + 2][lane];
      const VR m1m = sm1[r][lane], m2p = sm2[r + 1][lane];
      // ---- y neighbours from the adjacent lanes; the strip's outer columns from the scalar loads ----
      const P pyl = lane_from_prev(f4(cur.pc, YPL - 1), cur.pel), pyr = lane_from_next(f4(cur.pc, 0), cur.per);
      const R ryl = lane_from_prev(f4(rj.c, YPL - 1), rj.el), ryr = lane_from_next(f4(rj.c, 0), rj.er);
      R e1, e2;
      if constexpr (EGNO == 3) {
        e1 = (rj.el + (R)1e-4) * fpos<R>(axc);
        e2 = (rj.er + (R)1e-4) * fneg<R>(axc);
      } else {
        e1 = m1f<EGNO, R>(rj.el, cur.ael, aym);
        e2 = m2f<EGNO, R>(rj.er, cur.aer, ayp);
      }
      const R m1yl = lane_from_prev(m1y[YPL - 1], e1), m2yr = lane_from_next(m2y[0], e2);
      const bool last = (j == T - 1) && p.last_slab;   // the window's last row
      const size_t oo = (size_t)(j - rp.j0) * plane + rxc + y;
#pragma unroll
      for (int e = 0; e < YPL; ++e) {
        const P c = f4(cur.pc, e);
        const P lft = e == 0 ? pyl : f4(cur.pc, e - 1);
        const P rgt = e == YPL - 1 ? pyr : f4(cur.pc, e + 1);
        R a[4];
#pragma unroll
        for (int i = 0; i < NA; ++i) a[i] = f4(cur.a[i], e);
        const R hr = hj_point<R, EGNO, P>(p, px, c, f4(pm, e), f4(pp, e), lft, rgt, f4(f0, e), a, axc, f4(ay4, e));
        // the continuity residual in cont_residual_2d's operation order
        const R r0 = f4(rj.c, e);
        R res = (f4(cur.rn.c, e) - r0) * p.inv_dt;
        if (use_eps) {
          const R rym = e == 0 ? ryl : f4(rj.c, e - 1), ryp = e == YPL - 1 ? ryr : f4(rj.c, e + 1);
          res = res + p.epsl * ((f4(rpl, e) + f4(rm, e) - (R)2 * r0) * p.inv_dx2);
          res = res + p.epsl * ((ryp + rym - (R)2 * r0) * p.inv_dy2);
        }
        const R m1ym = e == 0 ? m1yl : m1y[e - 1], m2yp = e == YPL - 1 ? m2yr : m2y[e + 1];
        const R div = (f4(m1x, e) - f4(m1m, e)) * p.inv_dx + (f4(m2p, e) - f4(m2x, e)) * p.inv_dx +
                      (m1y[e] - m1ym) * p.inv_dy + (m2yp - m2y[e]) * p.inv_dy;
        res = res - div;
        if (last) res = res + p.c_over_dt;
        rep_accum<R, P>(acc, hr, res, r0, c);
        // pdhg_report_rows only (uniform): stored point by point, so the reducing pass keeps no field registers
        if (rp.hj) rp.hj[oo + e] = (double)hr;
        if (rp.cont) rp.cont[oo + e] = (double)res;
      }
      f0 = cur.pc;
      rj = cur.rn;
      lds_sync();   // every wave has read this step's rows before the next step overwrites them
      cur = nxt;    // the next row, loaded while this step computed
    }
  }
  block_reduce_store_report(acc, rp.partials, (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

}  // namespace pdhg
