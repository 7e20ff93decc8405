// Which kernels a context runs and with what geometry: decided once, at context creation, by plan_paths() -- a pure
// function of the problem, the precision, the decomposition and the Tuning (no device, no environment).  The
// launchers (ctx_impl.hpp) switch on the plan's KernelChoice per stage and re-test nothing; pdhg_path_info /
// pdhg_plan_info answer from the same choices.
// The decisions are ordered: a later one reads the earlier ones' values (marked "reads" below).
#pragma once

#include <cstdio>
#include <string>

#include "../../include/pdhg.h"
#include "fft_lds.hpp"
#include "kernels_dual_multi.hpp"
#include "kernels_fs16.hpp"
#include "tuning.hpp"

namespace pdhg {

constexpr size_t kLdsBytes = 160 * 1024;
constexpr int kMultiSub = 5;    // sub-iterations one chunk pass of the dual loop runs (kernels_dual_multi.hpp)
// mixed update at 512 threads: old-phi row pairs (doubles) in flight; 238 VGPRs, no spill at 4 (fp32: 228), the same
// 2 waves per SIMD at 1 .. 4, so the fp32 default depth
constexpr int kMixedUpdPF = 4;
constexpr int kFoldRows = 64;   // rows of the first fold level (k_fold_partials) after the partial table

inline FFTPlan make_plan(int n, bool& ok) {
  FFTPlan pl{};
  pl.n = n;
  pl.pow2 = (n > 0) && ((n & (n - 1)) == 0);
  int m = n, np = 0;
  ok = true;
  auto push = [&](int r) {
    if (np >= kMaxPass) { ok = false; return; }
    pl.radix[np++] = r;
  };
  for (int r : {16, 8, 4, 2})
    while (m % r == 0 && m > 1) { push(r); m /= r; }
  while (m % 3 == 0) { push(3); m /= 3; }
  for (int f = 5; m > 1; f += 2)
    while (m % f == 0) { push(f); m /= f; }
  pl.npass = np;
  return pl;
}

// single context, or one part of a multi-GPU decomposition
struct Decomp {
  bool slab = false;    // t-slab: this context owns unknown rows [j0, j0 + T) of a window of Tg
  int j0 = 0, Tg = 0;
  bool xslab = false;   // x-slab: global x rows [rank * nloc, (rank + 1) * nloc) of nxg; pb.nx = nloc + 16 local rows
  int rank = 0, P = 1, nxg = 0, nloc = 0;
  bool mixed = false;   // precision 12: S = 4 with phi and phi_bar in double (single 2-D contexts)
};

// The kernel one 2-D stage launches: its family (the stage's enum below; 0: the stage has no such kernel), the
// family's template integers (0 where unused), the block size and the dynamic LDS bytes as launched (0: static / none)
struct KernelChoice {
  int family = 0;
  int n = 0, a = 0, b = 0, c = 0;
  int threads = 0;
  size_t lds = 0;
};
// The family codes are the values of the "<stage>_kernel" keys (include/pdhg.h); n, a, b, c
// are the template integers the launcher's case names, in the kernel's own order where the family has one.
// x transform.  fp32: XT_FAST <n, NL, NT>, XT_WS <n, NL, HR>, XT_BATCH <n, NL, RB, RPRE> (RB = 2: 512 threads), XT_DMA
// and XT_DMA_HR (nx = 8192) <4096>; fp64 XT_F64 <n, NT, HR, flags>: BPR 1 | TC 2 | DMA 4; XT_GENERIC: the runtime-radix
// kernel (with_xt_fft).  One-row windows: XT1_* <n, NL, NT> of k_precond_x_t1_2d (fp32, fp64, fp64 with G16)
enum XtKernel { XT_NONE, XT_FAST, XT_WS, XT_BATCH, XT_DMA, XT_DMA_HR, XT_F64, XT_GENERIC, XT1_F32, XT1_F64, XT1_F64_G16 };
// residual <n, RW, NT>: fp32 / fp64 fast rows, unfused and fused; RES_GENERIC b: the kernel's thread bound (256 / 1024)
enum ResKernel { RES_NONE, RES_GENERIC, RES_FAST, RES_FAST64, RES_FUSED, RES_FUSED64 };
// update <n, RW, NT, PF> (PF 0: the kernel's default): fp32 and mixed fast rows, the fp64 4-row kernel, its one-row
// G16 form, the 8-row task pairs <n, -, NT, PF>, the 2-row tasks at ny = 8192; UPD_GENERIC*: b as RES_GENERIC
enum UpdKernel { UPD_NONE, UPD_GENERIC, UPD_GENERIC_MIXED, UPD_FAST, UPD_FAST_MIXED, UPD_FAST64, UPD_T1_G16,
                 UPD_PAIR64, UPD_8192 };
// dual sweep: per point, row per thread (a: ONE), x rows through LDS (a: RX, b: YPL), ... forming the residual too
enum DualKernel { DUAL_NONE, DUAL_POINT, DUAL_POINT_MIXED, DUAL_ROW, DUAL_ROW_MIXED, DUAL_LDS, DUAL_LDS_FR };

struct PathPlan {
  // what each 2-D stage launches (set at the end of the decision it belongs to; the launchers switch on these).
  // xt_one_row: T = 1 single or x-slab contexts; res_fused / dual_fused: while the fused residual is valid / formed
  KernelChoice xt, xt_one_row, res, res_fused, upd, dual, dual_fused;
  FFTPlan plx{}, ply{};   // x (global length) and y line transforms
  int na = 0, n_dead = 0;
  bool mixed = false;     // fp32 state and kernels, phi / phi_bar double (the mixed update and dual kernels)
  bool two_sets = false;  // rho_alp_iters > 1: two (rho, alp) buffer sets
  // spectral blocks (KP::B / lB / nb / half_real / tile_j)
  int B = 1, lB = 0, nb = 1, tile_j = 0;
  bool half_real = false;         // 2-D nx = 8192: one real column per x-transform block
  int xs_nbs = 0;                 // x-slab: column blocks of this rank
  // launch geometry
  int NT2 = 512;
  int gx1 = 0, gx4 = 0, g4 = 1, gx5 = 0, g5 = 1, g_outer = 1;
  int head_xrun = 4;              // x rows per workgroup of the head form's chunk passes
  int nt_row = 256;               // threads of the generic 2-D row kernels (k_res_fwdy_2d, k_invy_update_2d)
  int NTd = 256, gxd = 0, gyd = 0, gzd = 0, jchunk_d = 1;
  int gz_1d = 1, jchunk_1d = 1;   // 1-D fused residual (k_dual_1d_fr): time chunks of the dual sweep
  int nt1d = 256;                 // 1-D residual / update block size (1024 on the global-scratch path)
  int RWf = 8, NTf = 1024, g_fast_upd = 1;   // fast row kernels: rows per workgroup, threads, update grid
  size_t partial_rows = 0;
  size_t lds_res = 0;             // LDS bytes of the generic row kernels and the 1-D line kernels
  // dual
  bool fast_dual = false;         // row-per-thread / LDS-row time-marching dual instead of the per-point kernel
  int dual_rx = 0;                // > 0: k_dual_lds_2d with dual_rx x rows per workgroup (x neighbours through LDS)
  int dual_ypl = 4;               // y per lane of k_dual_lds_2d (fp64: 4 or 2)
  int dual_order = 0;             // workgroup -> tile order of k_dual_lds_2d (dual_order.hpp: 0 x-fastest, XB > 0 band)
  bool dual_multi = false;        // rho_alp_iters > 1: the dual loop in chunks of sub-iterations
  bool dual_head = false;         // ... below 2^25 points: sub-iteration 0 alone, the rest in chunks
  bool k1_outer = true;           // one-sub-iteration loops skip the outer-sum pass
  bool fold_fin = false;          // fold + finalize of a folded partial table in one launch
  bool spec_ok = false;           // iterate() may use the speculative one-sub-iteration schedule (head form)
  bool fin_merge = true;          // ... with its dual and outer finalizes in one launch
  // fused residual: the dual sweep also forms the next primal's residual rows (k_dual_lds_2d FR / k_dual_1d_fr), the
  // residual kernel only completes the tile-edge terms and transforms
  bool fuse_res = false;
  // row kernels
  bool fast_rows = false;         // fp32, power-of-two ny: RWf rows per workgroup, NTf threads
  bool res64 = false;             // fp64 residual and update through the fast row kernels (4-row groups)
  bool ip_rows = false;           // fp64 ny = 8192: generic row kernels on one padded in-place line (FFTIp)
  bool upd8192 = false;           // fp64 ny = 8192, half-real x: update through the fast row kernel on 2-row tasks
  bool tc_spec = false;           // fp64 C3: residual spectrum in task order (KP::rspec)
  bool to_c4 = false;             // C4 (half-real x blocks): fused residual in task order + transpose
  // x transform
  bool f64_xt = false;            // fp64: in-place line + register carries (k_precond_xt_f64_2d)
  // 1-D
  bool glb_line = false;          // line FFTs over global scratch (nx beyond LDS)
  bool fourstep = false;          // nx = 65536: four-step DHT
  bool fs_wide = true;            // ... with 64-column / 32-row tiles (k_fs1w_1d / k_fs2w_1d)
  bool fs16 = false;              // ... as a 16 x 4096 split with a chunk-major spectrum (kernels_fs16.hpp)
  int f16_group = 16;             // rows n1 per load group of k_f16a_fwd_1d
  bool thomas_chunk = false;      // t-solve in chunks of rows (k_thomas_chunk_1d)
  // solution report (kernels_report.hpp)
  bool report_tile = false;       // k_report_tile_2d (8-row tiles marching over t) instead of the per-point kernel
  int report_wgs = 1024;          // ... workgroups it aims for: fewer tiles than that split the window into time chunks
};

// S = sizeof(real) (4 / 8; a mixed context plans as S = 4 with dc.mixed).  pb is the context's own problem (an
// x-slab's has its local rows).  Returns PDHG_OK, or PDHG_ERR_UNSUPPORTED with the reason in err.
inline int plan_paths(const pdhg_problem& pb, int S, const Decomp& dc, const Tuning& tn, PathPlan& pl,
                      std::string& err) {
  auto fail = [&err](int code, const char* fmt, auto... args) {
    if constexpr (sizeof...(args) == 0) {
      err = fmt;
    } else {
      char buf[512];
      snprintf(buf, sizeof(buf), fmt, args...);
      err = buf;
    }
    return code;
  };
  pl = PathPlan{};
  if (dc.mixed && (S != 4 || pb.ndim != 2 || dc.slab || dc.xslab))
    return fail(PDHG_ERR_UNSUPPORTED, "mixed precision (12) is implemented for single 2-D contexts only");
  pl.mixed = dc.mixed;
  const int nx = pb.nx, ny = pb.ny, T = pb.T;
  const int nxg = dc.xslab ? dc.nxg : nx;   // length of the x transform (global nx for an x-slab)
  const bool is2d = pb.ndim == 2, slab = dc.slab, xslab = dc.xslab;
  const size_t csz = 2 * (size_t)S;
  pl.na = (pb.ndim == 1 || pb.egno == 3) ? 2 : 4;
  pl.n_dead = (pb.ndim == 2 && pb.egno == 3) ? 2 : 0;
  const bool two_sets = pl.two_sets = pb.rho_alp_iters > 1;
  bool ok1 = true, ok2 = true;
  pl.plx = make_plan(nxg, ok1);
  if (is2d) pl.ply = make_plan(ny, ok2);
  if (!ok1 || !ok2) return fail(PDHG_ERR_UNSUPPORTED, "FFT plan too deep for nx=%d ny=%d", nxg, ny);

  if (is2d) {
    // spectral block width B: contiguous [nx][B] slabs; the x-transform workgroup holds
    // M = nx*B modes with 5*M*sizeof(R) bytes of LDS (FFT ping-pong + Thomas carries)
    const size_t cap = (S == 4) ? 8192 : 4096;
    int B = 16;
    while (B > 2 && (size_t)nxg * B > cap) B >>= 1;
    int nyp = 2;
    while (nyp < ny) nyp <<= 1;
    if (B > nyp) B = nyp;
    // fp64 nx = 512 / 1024 with T > 1: one column pair per block (B = 2) for the fp64 x kernel below (the generic
    // kernel would take B = 8 / 4 with its carries in global memory); T = 1 keeps the one-row kernel's B
    // (a t-slab takes the window's row count, so every slab of one window gets the same layout: a 1-row slab of a
    // longer window must not keep B = 8 / 4 while its neighbours exchange B = 2 carry planes)
    const bool xt64_on = tn.xt64.value_or(1) != 0;
    const bool f64_small = S == 8 && pb.bc_x == 0 && (slab ? dc.Tg : T) > 1 && (nxg == 1024 || nxg == 512) &&
                           ny % 2 == 0 && xt64_on;
    if (f64_small) B = 2;
    // fp32 nx = 8192 (C4): one real column per block, packed into a 4096-point FFT (half_real)
    // fp64 nx = 8192 (C4's grid in the reference's precision): the same half-real split in k_precond_xt_f64_2d<HR>
    pl.half_real = nxg == 8192 && pb.bc_x == 0 && (S == 4 || !xslab);
    if (pl.half_real) B = 1;
    // fp64 nx = 4096 (C3's grid in the reference's precision): k_precond_xt_f64_2d keeps the carries in
    // registers, so the column pair (B = 2) fits LDS although 5 M reals would not
    // (t-slab phases too: kernels_xt_f64.hpp)
    // fp64 nx = 2048 (C2's grid): the same kernel with b' in registers (BPR) instead of the generic runtime-radix
    // kernel's global carries (10.97 ms at C2, 0.15 of the HBM roofline, round 4)
    // (reads B, half_real, f64_small)
    pl.f64_xt = S == 8 && pb.bc_x == 0 &&
                (((nxg == 4096 || nxg == 2048) && B == 2) || (nxg == 8192 && pl.half_real) || f64_small) && xt64_on;
    // nx = 4096 column pairs on single contexts (t-slab phases, x-slabs and the half-real blocks keep the LDS b'
    // line): b' / x in registers, and in the 64 KiB that frees the forward rows staged by LDS DMA, the first
    // radix-16 pass out of place (PDHG_XT64_DMA; PDHG_XT64_BPR=1 with PDHG_XT64_DMA=0: the register form alone,
    // A/B -- the DMA form cannot run without it, its staging line is the LDS b' line's space)
    // (reads f64_xt, half_real, B)
    const bool bpr_ok = pl.f64_xt && nxg == 4096 && B == 2 && !pl.half_real && !slab && !xslab;
    const bool dma_ok = bpr_ok && tn.xt64_dma.value_or(1) != 0;
    const bool xt64_bpr = bpr_ok && tn.xt64_bpr.value_or(dma_ok ? 1 : 0) != 0;
    const bool xt64_dma = dma_ok && xt64_bpr;
    // fp64 one-row windows at a power-of-two nx: the carry-free transform needs only the padded lines
    const bool t1_xt64 = S == 8 && T == 1 && pb.bc_x == 0 && !pl.half_real && !slab && pl.plx.pow2 &&
                         nxg >= 512 && nxg <= 4096 && nxg * (B / 2) == (nxg == 4096 ? 4096 : 2048);
    // fp64 unfused residual's threads at ny = 2048: 256 on one-row windows (two 4-wave workgroups per CU, 225 VGPRs;
    // C2's T = 1 residual 54 -> 47 us), 512 otherwise (C2's T = 100 unfused residual 4.66 vs 4.94 ms at 256)
    const int res64_nt2048 = tn.res64_nt2048.value_or(T == 1 ? 256 : 512);
    // steady marching iteration 0.2196 (512 threads) / 0.2150 (PF 4) / 0.2131 ms (PF 2)
    const int upd_t1 = T == 1 ? tn.upd_t1.value_or(2) : 0;
    if (!pl.half_real && !pl.f64_xt && (size_t)nxg * B > cap)
      return fail(PDHG_ERR_UNSUPPORTED, "nx=%d too large for the x-transform slab (max %zu in this precision)", nxg,
                  cap / 2);
    pl.B = B;
    while ((1 << pl.lB) < B) ++pl.lB;
    pl.nb = (ny + B - 1) / B;
    pl.lds_res = 2 * (size_t)ny * csz;
    const int nmodes = nxg * B;
    // fp64 ny = 8192 (C4's y extent in the reference's precision): the generic row kernels transform the row pair
    // in place in one padded line (FFTIp, 136 KiB) instead of a Stockham ping-pong of two (256 KiB)
    pl.ip_rows = S == 8 && ny == 8192 && pl.lds_res > kLdsBytes && !xslab;
    if (pl.ip_rows) pl.lds_res = (size_t)Pad<8192>::LINE * csz;
    // ... and the update through the fast row kernel on 2-row tasks when the x blocks are half-real (B = 1)
    pl.upd8192 = pl.ip_rows && pl.half_real && nx % 2 == 0 && tn.upd8192.value_or(1) != 0;
    if (pl.upd8192) pl.g_fast_upd = std::min((nx / 2) * T, 2048);
    if (pl.lds_res > kLdsBytes) return fail(PDHG_ERR_UNSUPPORTED, "ny=%d exceeds the LDS row transform", ny);
    {   // generic row kernels: when the LDS admits few workgroups per CU (fp64 ny = 4096: one), wider
        // workgroups keep >= 16 waves per CU in flight for the residual's scattered loads
      const int wg = (int)std::max<size_t>(1, kLdsBytes / std::max<size_t>(pl.lds_res, 1));
      pl.nt_row = std::min(1024, 256 * std::max(1, 4 / wg));
    }
    pl.NT2 = std::min(512, ((nmodes + 63) / 64) * 64);
    pl.gx1 = ((nx + 1) / 2) * T;                      // row-pair tasks (flat grid)
    pl.gx4 = (int)std::min<long long>((long long)pl.gx1, 4096);
    pl.gx5 = (ny + 255) / 256;
    pl.g5 = std::max(1, std::min(T * nx, 8192 / std::max(1, pl.gx5)));
    pl.k1_outer = tn.k1_outer;
    pl.fold_fin = tn.fold_fin;
    // short windows (the reference's T = 1 marching default): few time rows per workgroup leave little to
    // pipeline over t, so occupancy decides.  Measured on C3's grid (bench --config c3w1/c3w4/c3w8): the
    // single-role x-transform kernel beats the warp-specialised one up to T = 8 at least (T = 1: 0.18 vs
    // 0.24 ms, T = 8: 0.79 vs 0.84 ms); the row-per-thread dual (146 VGPRs, 3 waves/SIMD) without the
    // fused residual beats the fused 8-row sweep (200 VGPRs, 2 waves/SIMD) at T = 1 (0.31 vs 0.41 ms),
    // ties at T = 4 and loses from T = 8 on.
    const bool short_win = T < tn.short_t_xt, short_dual = T < tn.short_t_dual;
    const int NL = B / 2;
    const size_t pad4k = 4096 + 4096 / 16;   // a padded line of 4096 complex
    // the generic runtime-radix kernel unless a fast form below applies: FFT ping-pong + Thomas carries
    pl.xt = {XT_GENERIC, 0, 0, 0, 0, pl.NT2, (size_t)5 * nmodes * S};
    bool fast_xt = false;   // fp32 power-of-two nx: the fast x kernels
    if (pl.half_real && S == 4) {
      fast_xt = true;
      // the LDS-DMA staged x transform on half-real blocks (k_precond_xt_dma_2d<4096, true>, static LDS) for windows
      // of >= 4 rows: c4w50 x transform 28.4 ms with the warp-specialised kernel (round 4, 1.9 TB/s)
      if (tn.xt_dma_hr ? *tn.xt_dma_hr != 0 : T >= 4) pl.xt = {XT_DMA_HR, 4096, 0, 0, 0, 1024, 0};
      else pl.xt = {XT_WS, 4096, 1, 1, 0, 512, (2 * pad4k + 816 + 4096) * csz};   // + split twiddles
    } else if (S == 4 && pl.plx.pow2 && nxg * NL == 4096 && nxg >= 512 && pb.bc_x == 0) {
      fast_xt = true;
      // the other widths spill registers in the warp-specialised form
      const bool ws_xt = tn.xt_ws ? *tn.xt_ws != 0 : (nxg == 4096) && !short_win;
      // row-batched x transform (k_precond_xt_batch_2d): 4 rows per transform, 1024 threads.  Measured at C3
      // (nx = 4096, T = 200): 16.2 -> 14.5 ms against the warp-specialised kernel; at C2 (nx = 2048,
      // T = 100) 2.07 -> 1.82 ms against the single-role one.  nx = 1024 / 512 spill in it: not selected.
      const bool batch_xt = tn.xt_batch ? *tn.xt_batch != 0 : (nxg == 4096 || nxg == 2048) && T >= 4;
      const size_t tw = twlds_size(nxg);
      if (batch_xt && nxg == 4096 && tn.xt_dma.value_or(1) != 0)
        // LDS-DMA staged rows (k_precond_xt_dma_2d, static LDS) at nx = 4096: C3 14.24 -> 13.52 ms
        pl.xt = {XT_DMA, 4096, 0, 0, 0, 1024, 0};
      else if (batch_xt && nxg == 4096 && tn.xt_pair)   // RB = 2 rows, 512 threads: two workgroups per CU
        pl.xt = {XT_BATCH, 4096, 1, 2, 0, 512, (2 * pad4k + tw) * csz};
      else if (batch_xt)
        pl.xt = {XT_BATCH, nxg, NL, 4, (nxg == 4096 && tn.xt_rpre == 2) ? 2 : 0, 1024, (4 * pad4k + tw) * csz};
      else if (ws_xt)
        pl.xt = {XT_WS, nxg, NL, 0, 0, 512, (2 * pad4k + 816) * csz};
      else   // padded FFT buffer + theta, E, b' (float2 per item) + twiddle seeds (TwLds<nx>)
        pl.xt = {XT_FAST, nxg, NL, 512, 0, 512, (pad4k + 3 * 4096 + 816) * csz};
    }
    // fp64: the forms of k_precond_xt_f64_2d (reads f64_xt, half_real, xt64_bpr, xt64_dma; tc_spec sets TC below)
    if (pl.f64_xt) {
      const size_t tw4k = TwLds<4096>::SIZE;
      if (pl.half_real)   // nx = 8192: one real column per block + the split-twiddle tables
        pl.xt = {XT_F64, 4096, 512, 1, 0, 512, (Pad<4096>::LINE + tw4k + 4096 + 128) * csz};
      else if (nxg == 1024)   // b' in registers, 4 items per thread
        pl.xt = {XT_F64, 1024, 256, 0, 1, 256, (size_t)(Pad<1024>::LINE + TwLds<1024>::SIZE) * csz};
      else if (nxg == 512)
        pl.xt = {XT_F64, 512, 128, 0, 1, 128, (size_t)(Pad<512>::LINE + TwLds<512>::SIZE) * csz};
      else if (nxg == 2048) {   // b' in registers (IT = 4 at 512 threads; PDHG_XT64_VAR: A/B of the shapes)
        const size_t bpr = (size_t)(Pad<2048>::LINE + TwLds<2048>::SIZE) * csz;
        const int v = tn.xt64_var;   // 1: 256 threads with b' in LDS, 2: 256, 3: 1024
        const int nt = (v == 1 || v == 2) ? 256 : v == 3 ? 1024 : 512;
        pl.xt = {XT_F64, 2048, nt, 0, v == 1 ? 0 : 1, nt, v == 1 ? bpr + 2048 * csz : bpr};
      } else if (xt64_dma)   // b' in registers, forward rows staged by LDS DMA: static LDS (kernels_xt_f64.hpp, DMA)
        pl.xt = {XT_F64, 4096, 512, 0, 1 | 4, 512, 0};
      else if (xt64_bpr)   // b' in registers alone (A/B: spills in the forward sweep)
        pl.xt = {XT_F64, 4096, 512, 0, 1, 512, (Pad<4096>::LINE + tw4k) * csz};
      else
        pl.xt = {XT_F64, 4096, 512, 0, 0, 512, (Pad<4096>::LINE + tw4k + 4096) * csz};
    }
    // one-row windows (T = 1 single and x-slab contexts; a t-slab runs its phases): the carry-free x transform
    // k_precond_x_t1_2d on the padded lines + twiddle seeds, two workgroups per CU.  fp64 (the reference's marching
    // default in its own precision; C2 marching, nx = 2048, B = 2: the generic kernel took 156 us per launch, this one
    // 28 us, 67 MB read + 67 MB written: 4.8 TB/s), G16 at nx = 2048 / 4096: only the first twiddled pass's 48 seeds
    // in LDS, so 4 (nx = 2048, 256 threads; 512: 28.06 vs 27.64 us) or 2 (nx = 4096) workgroups fit a CU, not 3 / 1
    // (reads fast_xt, half_real, t1_xt64)
    if (T == 1 && !slab && tn.t1_xt) {
      const size_t lines = (size_t)NL * (nxg + nxg / 16);
      const bool g16 = tn.t1_g16 && (nxg == 2048 || nxg == 4096);
      if (S == 4 && fast_xt && !pl.half_real)
        pl.xt_one_row = {XT1_F32, nxg, NL, 512, 0, 512, (lines + twlds_size(nxg)) * csz};
      else if (t1_xt64)
        pl.xt_one_row = {g16 ? XT1_F64_G16 : XT1_F64, nxg, NL, nxg == 2048 ? 256 : 512, 0, nxg == 2048 ? 256 : 512,
                         (lines + (g16 ? 48 : twlds_size(nxg))) * csz};
    }
    // fp64: the row-per-thread time-marching dual (k_dual_fast_2d<EGNO, double>) instead of the generic
    // per-point kernel, which re-reads every phi_bar neighbour (fp64 C3: 248 GB fetched for 161 GB of reads).
    // Measured at fp64 C3 (same box, profiles/r04_ab_dual64_*.json): 52.7 vs 59.3 ms per dual, 6.61 vs 6.44
    // it/s.  PDHG_DUAL64=0 keeps the generic kernel.  The LDS-row and fused variants are fp32.
    const bool dual64 = S == 8 && ny % 256 == 0 && tn.dual64.value_or(1) != 0;
    int dual_one = 1;
    if ((S == 4 || dual64) && ny % 256 == 0) {
      pl.fast_dual = true;
      // x rows through LDS (k_dual_lds_2d) for the fused-residual sweep; a context created for
      // rho_alp_iters > 1 (no fused residual) sweeps row-per-thread: measured at C3 with rho_alp_iters = 10,
      // k_dual_fast_2d 25.7 ms per sub-iteration against 38.1 for k_dual_lds_2d (2 waves per SIMD)
      // fp64 (k_dual_lds_2d<EGNO, 8, false, double>, 230 VGPRs, no spill): the phi_bar x neighbours through LDS
      // instead of the row-per-thread kernel's 1.25x re-reads from L2 (fp64 C3: 200 GB fetched for 161 GB of reads)
      pl.dual_rx = (nx % 8 == 0 && !short_dual && !two_sets) ? 8 : 0;
      if (tn.dual_rx) {   // 0 = row-per-thread kernel
        const int v = *tn.dual_rx;
        if (v == 0 || (((S == 4 && (v == 4 || v == 16)) || v == 8) && nx % v == 0)) pl.dual_rx = v;
      }
      // mixed: the row-per-thread sweep (k_dual_lds_2d stages phi_bar rows through LDS in R), hence no fused residual
      if (dc.mixed) pl.dual_rx = 0;
      if (S == 8 && pl.dual_rx == 8 && tn.dual_ypl.value_or(0) == 2) pl.dual_ypl = 2;
      dual_one = tn.dual_one;
      pl.NTd = pl.dual_rx ? pl.dual_rx * 64 : std::min(256, ny / 4);
      pl.gxd = pl.dual_rx ? nx / pl.dual_rx : nx;
      pl.gyd = pl.dual_rx ? ny / (64 * pl.dual_ypl) : (ny / 4 + pl.NTd - 1) / pl.NTd;
      const int nJ0 = std::max(1, std::min(T, (2048 + pl.gxd * pl.gyd - 1) / (pl.gxd * pl.gyd)));
      pl.jchunk_d = (T + nJ0 - 1) / nJ0;
      pl.gzd = (T + pl.jchunk_d - 1) / pl.jchunk_d;
    }
    // k_dual_fast_2d<.., ONE> on one-row workgroups (0: the marching form; fp64 2: 4 waves per SIMD)
    dual_one = (pl.fast_dual && !pl.dual_rx && pl.jchunk_d == 1) ? (dual_one == 2 && S == 8 && !dc.mixed ? 2 : dual_one != 0)
                                                                 : 0;
    // generic row kernels (the line FFT policy: with_line_fft), replaced below where the fast rows apply
    pl.res = {RES_GENERIC, 0, 0, pl.nt_row <= 256 ? 256 : 1024, 0, pl.nt_row, pl.lds_res};
    pl.upd = {dc.mixed ? UPD_GENERIC_MIXED : UPD_GENERIC, 0, 0, pl.nt_row <= 256 ? 256 : 1024, 0, pl.nt_row, pl.lds_res};
    size_t lds_fast_tw = 0;   // fp32 fast rows: the lines + the persistent kernels' twiddle seeds
    if (S == 4 && pl.ply.pow2 && ny >= 256 && ny <= 8192) {
      pl.RWf = (ny == 8192) ? 4 : 8;
      pl.NTf = std::min(1024, ny / 4);
      if (tn.rows_var == 1 && (ny == 4096 || ny == 2048)) {   // 4 rows / block, 2 blocks per CU
        pl.RWf = 4;
        pl.NTf = ny / 8;
      }
      if (nx % pl.RWf == 0 && (pl.RWf * B) % 4 == 0) {
        pl.fast_rows = true;
        // residual task tiles of 8 time rows x 4 row groups (rows past the last whole tile run untiled)
        pl.tile_j = ((nx / pl.RWf) % 4 == 0) ? 8 : 1;
        if (tn.tile_j) {
          const int v = *tn.tile_j;
          if (v >= 1 && (v == 1 || (nx / pl.RWf) % 4 == 0)) pl.tile_j = v;
        }
        const size_t lds_fast = (size_t)(pl.RWf / 2) * (ny + ny / 16) * csz;
        // + the twiddle-seed table of the persistent kernels (fused residual, update; ny <= 4096)
        lds_fast_tw = lds_fast + (ny <= 4096 ? (size_t)twlds_size(ny) * csz : 0);
        pl.g_fast_upd = std::min((nx / pl.RWf) * T, 2048);
        pl.res = {RES_FAST, ny, pl.RWf, pl.NTf, 0, pl.NTf, lds_fast};
        // ny = 4096 8-row update with 512 threads (PDHG_HALF_NT bit 1) and PF old-phi row pairs in flight (1..4;
        // mixed: kMixedUpdPF)
        const bool half = pl.NTf == 1024 && pl.RWf == 8 && (tn.half_nt & 2);
        const int pf = dc.mixed ? kMixedUpdPF : (tn.upd_pf >= 2 && tn.upd_pf <= 4) ? tn.upd_pf : 1;
        const int nt = half ? 512 : pl.NTf;
        pl.upd = {dc.mixed ? UPD_FAST_MIXED : UPD_FAST, ny, pl.RWf, nt, half ? pf : 0, nt, lds_fast_tw};
      }
    }
    // fp64 residual: the fast row kernel on 4-row groups (2 complex lines of 4096 doubles = 136 KiB of LDS),
    // rows read once per group over the sliding 3-row window, instead of the generic row-pair kernel's
    // per-point neighbour re-reads (fp64 C3: 204 GB moved against 80.5 GB algorithmic)
    size_t lds_upd64 = 0;
    if (S == 8 && pl.ply.pow2 && (ny == 2048 || ny == 4096) && nx % 4 == 0) {
      pl.res64 = tn.res64.value_or(1) != 0;
      if (pl.res64) {
        pl.tile_j = ((nx / 4) % 4 == 0) ? 8 : 1;
        // 1024 threads cap the fp64 rows at 128 VGPRs (spills): 512, or res64_nt2048 at ny = 2048
        const size_t lds_res64 = (size_t)2 * (ny + ny / 16) * csz;
        const int nt = ny == 2048 && res64_nt2048 == 256 ? 256 : 512;
        pl.res = {RES_FAST64, ny, 4, nt, 0, nt, lds_res64};
        // the update through the fast row kernel too: + the twiddle-seed table (152 KiB at ny = 4096)
        lds_upd64 = lds_res64 + (size_t)twlds_size(ny) * csz;
        pl.g_fast_upd = std::min((nx / 4) * T, 2048);
        // the update on pairs of x-adjacent 4-row tasks (k_invy_update_pair_2d: whole 128-B spectrum lines, the second
        // task's half held in registers across the first; bitwise the 4-row kernel's phi' / phi_bar): single contexts
        // with an even task count per time row, whole column blocks of 2 .. 16 columns.  One-row windows at ny = 2048
        // keep their 256-thread forms (upd_t1), x-slabs (ghost rows) and t-slabs the 4-row kernel.  C3 fp64
        // headline, alternating with the parent: update 21.73 - 21.86 -> 20.35 - 20.58 ms, step 115.34 -> 114.07 ms
        // (profiles/headline_upd64_pair.txt).  Interleaved A/B: c3w100 update 10.75 -> 10.47 ms, c3w25 2.753 -> 2.791
        // (a loss), so by default windows of >= 100 rows only; PDHG_UPD_PAIR=1 any window, =0 the 4-row kernel
        // (reads B, upd_t1)
        const bool pair_ok = !slab && !xslab && (nx / 4) % 2 == 0 && T >= 1 && B >= 2 && B <= 16 && ny % B == 0 &&
                             !(ny == 2048 && upd_t1 > 0);
        const bool upd64_pair = pair_ok && (tn.upd_pair ? *tn.upd_pair != 0 : T >= 100);
        if (upd64_pair) pl.g_fast_upd = std::min((nx / 8) * T, 2048);   // the pair count's grid and partial rows
        if (tn.upd_grid) pl.g_fast_upd = std::min(pl.g_fast_upd, *tn.upd_grid);
        if (ny == 2048 && upd_t1 > 0)   // one-row windows: 256 threads, two workgroups per CU (G16 seeds); PF 2 / 4
          pl.upd = {UPD_T1_G16, 2048, 4, 256, upd_t1 == 2 ? 2 : 4, 256, lds_res64 + 48 * csz};
        else if (upd64_pair)   // its old-phi row pairs in flight (2..4)
          pl.upd = {UPD_PAIR64, ny, 0, 512, tn.upd_pair_pf, 512, lds_upd64};
        else
          pl.upd = {UPD_FAST64, ny, 4, 512, 4, 512, lds_upd64};
      }
    }
    if (pl.upd8192)   // (its decision is above, with ip_rows) 2-row tasks on one padded line
      pl.upd = {UPD_8192, 8192, 2, 512, 2, 512, (size_t)Pad<8192>::LINE * csz};
    // fp64 C3 shape: the residual spectrum handed to the x transform in task order (p.rspec; one contiguous run per
    // 4-row task instead of 64-B chunks of the blocked layout), the x kernel's forward sweep reading it
    // Interleaved A/B (round 5): C3's T = 200 118.8 -> 118.3 ms; its 25-row slab share (8 GPUs) 16.05 -> 16.35 ms
    // (the x kernel's 64-B reads cost relatively more on short windows), so windows of >= 100 rows only
    // (never on one-row windows: the T = 1 x kernel reads the blocked work buffer)
    // (reads res64, f64_xt, half_real, B, t1_xt64)
    const bool tc_ok = S == 8 && pl.res64 && ny == 4096 && pl.f64_xt && !pl.half_real && nxg == 4096 && B == 2 &&
                       !xslab && T > 1 && !t1_xt64;
    pl.tc_spec = tc_ok && (tn.tc_spec ? *tn.tc_spec != 0 : T >= 100);
    if (pl.tc_spec) pl.xt.c |= 2;   // the nx = 4096 forms of k_precond_xt_f64_2d with the task-order input (TC)
    // fused residual: fp32 fast kernels with 8-row tiles on both sides, rho_alp_iters = 1 (in place),
    // periodic bc, egno 1/2, single context; each dual workgroup must march the whole window (the
    // residual row j needs rho'_{j+1}), so only grids with enough (x, y) tiles to fill the chip
    // (PDHG_FUSE_RES=1 forces it for any eligible size, =0 turns it off)
    // fp64: the sweep k_dual_lds_2d<.., double, YPL = 2> (128-column strips, 211 VGPRs) and the residual in
    // half-tile tasks of 4 rows (k_res_fwdy_fused_2d<.., 4, 512, double>, the lines + twiddles fill the LDS)
    // fp32 ny = 8192 (C4's y extent): the 4-row fast kernels, so the residual runs half-tile tasks as in fp64
    // fp64 ny = 8192 (C4): the row pairs of the generic kernels (ip_rows) for the unfused residual and the update,
    // the fused residual on quarter-tile tasks (one line of 8192 complex doubles)
    // (reads fast_rows, RWf, res64, ip_rows, fast_dual, dual_rx, gxd, gyd; overwrites dual_ypl, gyd, jchunk_d, gzd)
    const bool fr_rows = S == 4 ? (pl.fast_rows && (pl.RWf == 8 || (pl.RWf == 4 && ny == 8192)))
                                : ((pl.res64 && (ny == 4096 || ny == 2048)) || (pl.ip_rows && ny == 8192));
    if (pl.fast_dual && pl.dual_rx == 8 && fr_rows && pb.bc_x == 0 && pb.bc_y == 0 && pb.egno != 3 && !two_sets &&
        !xslab) {
      // fp32 ny = 8192 (4-row half-tile tasks, 16-B chunks of the B = 1 spectrum): round 4 measured it neutral
      // (residual 31.2 -> 25.9 ms, dual 26.7 -> 31.3); with the XCD-ordered tasks (round 5, interleaved A/B at
      // c4w50) the fused residual runs 22.9 ms against 30.3 unfused, step 88.25 -> 85.64 ms: on by default
      pl.fuse_res = tn.fuse_res ? *tn.fuse_res != 0 : pl.gxd * pl.gyd >= 1024;
      if (pl.fuse_res) {
        if (S == 8) {
          pl.dual_ypl = 2;
          pl.gyd = ny / 128;
        }
        pl.jchunk_d = T;
        pl.gzd = 1;
        // the residual kernel that completes the rows the sweep formed: fp32 the fast rows' shape (ny = 4096 / 8192
        // with 512 threads per PDHG_HALF_NT bit 0); fp64 4-row tasks (ny = 4096: PDHG_RES64_NT=1024, A/B: 16 waves per
        // CU, GPT = 1), at ny = 8192 quarter-tile tasks on one padded line of 8192 complex doubles
        const int nt = S == 4 ? ((pl.NTf == 1024 && (tn.half_nt & 1)) ? 512 : pl.NTf) : ny == 4096 ? tn.res64_nt : 512;
        if (S == 4) pl.res_fused = {RES_FUSED, ny, pl.RWf, nt, 0, nt, lds_fast_tw};
        else if (ny == 8192) pl.res_fused = {RES_FUSED64, 8192, 2, nt, 0, nt, (size_t)Pad<8192>::LINE * csz};
        else pl.res_fused = {RES_FUSED64, ny, 4, nt, 0, nt, lds_upd64};
        pl.dual_fused = {DUAL_LDS_FR, 0, 8, pl.dual_ypl, 0, pl.NTd, 0};
      }
    }
    // the sweep without the fused residual (reads fast_dual, dual_rx, dual_one and dual_ypl after the overwrite)
    if (!pl.fast_dual) pl.dual = {dc.mixed ? DUAL_POINT_MIXED : DUAL_POINT, 0, 0, 0, 0, 256, 0};
    else if (pl.dual_rx) pl.dual = {DUAL_LDS, 0, pl.dual_rx, pl.dual_ypl, 0, pl.NTd, 0};
    else pl.dual = {dc.mixed ? DUAL_ROW_MIXED : DUAL_ROW, 0, dual_one, 0, 0, pl.NTd, 0};
    // workgroup -> tile order of k_dual_lds_2d (PDHG_DUAL_ORDER; dual_order.hpp): the band order (XB = 1, each XCD's
    // workgroups across whole grid rows) for the fused sweep on the 2048^2 and 4096^2 grids, where every freshly
    // created context ran the dual below the x-fastest order's median (interleaved A/B, 4 contexts each,
    // profiles/r07_ab_dual_order_*.txt): C3 fp64 61.19 -> 59.76 ms, C3 fp32 31.34 -> 28.14, c3w100 fp64 30.69 -> 29.63,
    // c3w25 fp64 8.33 -> 7.52, C2 fp64 9.89 -> 8.18, C2 fp32 4.52 -> 4.16 (XB = 2 / 4 within the spread of XB = 1).
    // ny = 8192 (c4w50: fp64 58.32 -> 57.94, fp32 29.97 -> 29.38 median, but one band context of four above the
    // median in each) keeps the x-fastest order, as do the sweeps without the fused residual (not measured) and the
    // t-slab and x-slab contexts, the multi-device ones included (measured on single contexts only)
    // (reads dual_rx, fuse_res, gxd, gyd)
    const bool band_dflt = pl.fuse_res && pl.gxd * pl.gyd >= 1024 && (ny == 2048 || ny == 4096);
    pl.dual_order = (pl.dual_rx && !slab && !xslab) ? tn.dual_order.value_or(band_dflt ? 1 : 0) : 0;
    // C4 (ny = 8192 with half-real x blocks, B = 1): the fused residual's task-order spectrum + a transpose into the
    // blocked layout instead of 16-B chunk stores (fp64 RW = 2 / fp32 RW = 4 tasks: 16-B elements)
    pl.to_c4 = pl.fuse_res && pl.half_real && B == 1 && ny == 8192 && !xslab &&
               (S == 8 ? pl.ip_rows : (pl.fast_rows && pl.RWf == 4)) && (nx % (S == 8 ? 64 : 128)) == 0 &&
               tn.c4_to.value_or(1) != 0;
  } else {
    pl.lds_res = 2 * (size_t)nx * csz;
    pl.gx1 = (T + 1) / 2;
    pl.gx4 = std::min(pl.gx1, 2048);
    if (pl.lds_res > kLdsBytes) {   // lines beyond LDS (C1: nx = 65536): Stockham passes over global scratch
      pl.glb_line = true;
      pl.lds_res = 0;
      pl.nt1d = 1024;
      // fp32 nx = 65536 (C1): four-step DHT over 16 + 9 workgroups of 1024 threads per row pair instead of
      // one workgroup per pair (T = 400 gave 200 workgroups for 256 CUs): 1.41 -> 1.12 ms per iteration
      // fp64 nx = 65536: the same 16 x 4096 split (kernels_fs16.hpp on complex doubles) instead of the
      // generic Stockham passes over global scratch (fp64 C1: 3.9x the algorithmic bytes)
      pl.fourstep = nx == 65536 && tn.fourstep.value_or(1) != 0;
      pl.fs_wide = tn.fs_wide;
      pl.fs16 = pl.fourstep && tn.fs16.value_or(1) != 0;
      if (S == 8 && !pl.fs16) pl.fourstep = false;   // the other four-step forms are fp32
      pl.f16_group = tn.f16_group;
    }
    pl.gx5 = (nx + 255) / 256;
    pl.g5 = std::max(1, std::min(T, 8192 / std::max(1, pl.gx5)));
    // chunked t-solve: one wave per 32-row chunk of 64 modes (T <= 512, Ct != 0)
    pl.thomas_chunk = pb.Ct != 0.0 && T <= 16 * 32 && tn.thomas_chunk.value_or(1) != 0;
    // fused 1-D residual (C1's 16 x 4096 path, rho_alp_iters = 1, periodic x): the dual sweep forms the residual
    // rows (k_dual_1d_fr), stage A reads them (k_f16a_fwd_fused_1d); 8 time chunks of the sweep (reads fs16)
    pl.fuse_res = pl.fs16 && pb.bc_x == 0 && !two_sets && pb.egno != 3 && nx % 256 == 0 &&
                  tn.fuse_res1d.value_or(1) != 0;
    pl.gz_1d = std::min(tn.fr1d_chunks, T);
    pl.jchunk_1d = (T + pl.gz_1d - 1) / pl.gz_1d;
    pl.gz_1d = (T + pl.jchunk_1d - 1) / pl.jchunk_1d;
  }
  // the report's tile kernel: whole 8-row x 256-column tiles, y periodic, x periodic or Neumann (its halo rows wrap
  // or clamp); single contexts (a slab's halo rows are not resident: the report refuses those)
  pl.report_tile = is2d && nx % 8 == 0 && ny % 256 == 0 && pb.bc_y == 0 && (pb.bc_x == 0 || pb.bc_x == 1) && !xslab &&
                   tn.report_tile.value_or(1) != 0;   // (a t-slab's pass: pdhg_slab_report)
  pl.report_wgs = tn.report_wgs;
  pl.g_outer = tn.g_outer;
  pl.head_xrun = tn.head_xrun;
  // rho_alp_iters > 1 on the row-per-thread dual grid, single contexts: the dual loop in chunk passes of
  // kMultiSub sub-iterations in registers (+ a final pass when the exit falls inside a chunk)
  // Only where a pass is bandwidth-bound: C2's T = 1 marching windows (4 M points, the loop exiting after a few
  // sub-iterations) ran 30.5 s with the chunks against 22.9 s per sub-iteration (launch-bound: the chunk computes
  // 5 sub-iterations and the final pass re-runs k*), C2's T = 100 window 22.1 vs 10.5 it/s and C3 5.80 vs
  // 3.00 it/s (round 4, fp64 / fp32, rho_alp_iters = 10)
  const bool multi_ok = is2d && two_sets && pl.fast_dual && pl.dual_rx == 0 && !slab && !xslab &&
                        pb.rho_alp_iters <= kDualMultiMax;
  pl.dual_multi = multi_ok && (tn.dual_multi ? *tn.dual_multi != 0 : (double)T * nx * ny >= (double)(1 << 25));
  // below that: the head form (sub-iteration 0 per-sub-iteration, the rest in chunks).  C2's marching windows exit
  // after sub-iteration 0 in nearly every outer iteration, where 18 returning launches cost ~0.2 ms
  pl.dual_head = multi_ok && !pl.dual_multi && tn.dual_head.value_or(1) != 0;
  // the speculative schedule of iterate() needs the head form's one-sub-iteration shortcuts (k1_outer) and the
  // two-launch fold / finalize (the halt flag is set by k_finalize_dual); reads dual_head, k1_outer, fold_fin
  pl.spec_ok = pl.dual_head && pl.k1_outer && !pl.fold_fin && tn.spec.value_or(1) != 0;
  pl.fin_merge = tn.fin_merge;
  // (reads the dual grid after the fused residual's overwrite)
  pl.partial_rows = std::max<size_t>(
      {(size_t)pl.gx4 * pl.g4, (size_t)pl.gx5 * pl.g5, (size_t)pl.g_outer, (size_t)pl.g_fast_upd,
       (size_t)pl.gxd * pl.gyd * (pl.gzd + 1), pl.fourstep ? (size_t)9 * ((T + 1) / 2) : 1, 1,
       (pl.dual_multi || pl.dual_head) ? (size_t)kMultiSub * pl.gxd * pl.gyd * pl.gzd : (size_t)1});
  if (xslab) {
    // the row kernels that skip the ghost / padding rows: fp32 fast rows (ny in [256, 8192]), fp64 4-row kernels
    if (!(is2d && (S == 4 ? pl.fast_rows : pl.res64) && pl.fast_dual && (pb.bc_x == 0 || pb.bc_x == 1) &&
          pb.bc_y == 0))
      return fail(PDHG_ERR_UNSUPPORTED, "x-slab decomposition needs ndim 2, bc (0,0) or (1,0) and a power-of-two ny "
                                        "in [256, 8192] (fp32) or ny = 2048 / 4096 (fp64) (fast row and dual kernels)");
    if (pl.nb % dc.P) return fail(PDHG_ERR_UNSUPPORTED, "%d column blocks do not split over %d ranks", pl.nb, dc.P);
    pl.xs_nbs = pl.nb / dc.P;
  }
  // t-slab phases: the fast DHT x kernels (power-of-two nx 512 - 8192), the fp64 x kernel (nx = 4096, and 8192
  // half-real) or the generic runtime-radix kernel (any nx, the DCT of egno 3's bc (1, 0)).  fp32 needs the
  // fast row kernels; fp64 splits the residual's halo row off with the 4-row kernels (ny 2048 / 4096) and runs
  // the generic row kernels over the whole slab after the halo otherwise
  if (slab && !(is2d && (pl.fast_rows || S == 8)))
    return fail(PDHG_ERR_UNSUPPORTED, "t-slab decomposition needs ndim 2 and, in fp32, a power-of-two ny in "
                                      "[256, 8192] (fast row kernels)");
  return PDHG_OK;
}

// the creation-time keys of pdhg_path_info / pdhg_plan_info (S = sizeof(real), pb: the context's own problem).  What
// runs is read off the stage's KernelChoice; "<stage>_kernel" is its family code, "<stage>_shape" its threads
inline bool plan_key(const PathPlan& pl, const pdhg_problem& pb, int S, const std::string& k, int* value) {
  const KernelChoice *stage[] = {&pl.xt, &pl.xt_one_row, &pl.res, &pl.res_fused, &pl.upd, &pl.dual, &pl.dual_fused};
  const char* stage_name[] = {"xt", "xt_one_row", "res", "res_fused", "upd", "dual", "dual_fused"};
  for (int i = 0; i < 7; ++i) {
    if (k == std::string(stage_name[i]) + "_kernel") return *value = stage[i]->family, true;
    if (k == std::string(stage_name[i]) + "_shape") return *value = stage[i]->threads, true;
    const int shape[] = {stage[i]->n, stage[i]->a, stage[i]->b, stage[i]->c};   // "<stage>_n" / "_a" / "_b" / "_c"
    for (int j = 0; j < 4; ++j)
      if (k == std::string(stage_name[i]) + "_" + "nabc"[j]) return *value = shape[j], true;
  }
  const bool lds_dual = pl.dual.family == DUAL_LDS, xt64_4k = pl.xt.family == XT_F64 && pl.xt.n == 4096 && !pl.xt.b;
  const bool fast_upd = pl.upd.family == UPD_FAST || pl.upd.family == UPD_FAST_MIXED;
  if (k == "fused_residual") *value = pl.fuse_res ? 1 : 0;
  else if (k == "mixed") *value = pl.mixed ? 1 : 0;   // precision 12; the other keys: the fp32 kernels chosen
  else if (k == "fast_rows") *value = pl.fast_rows ? 1 : 0;
  else if (k == "res64") *value = pl.res64 ? 1 : 0;
  else if (k == "dual_multi") *value = pl.dual_multi ? 1 : 0;   // rho_alp_iters > 1: chunked dual passes
  else if (k == "dual_head") *value = pl.dual_head ? 1 : 0;     // ... sub-iteration 0 alone, then the chunks
  else if (k == "spec") *value = pl.spec_ok ? 1 : 0;   // iterate(): speculative one-sub-iteration schedule allowed
  else if (k == "dual64") *value = (S == 8 && pl.fast_dual) ? 1 : 0;
  else if (k == "fast_dual") *value = lds_dual ? pl.dual.a : pl.dual.family >= DUAL_ROW ? 0 : -1;
  else if (k == "dual_ypl") *value = lds_dual ? pl.dual.b : 0;
  // fp64 4-row residual threads: the fused kernel's where PDHG_RES64_NT=1024 applies, else the unfused kernel's
  else if (k == "res64_nt")
    *value = pl.res.family != RES_FAST64 ? 0 : pl.res_fused.threads == 1024 ? 1024 : pl.res.threads;
  else if (k == "upd_t1") *value = pl.upd.family == UPD_T1_G16 ? (pl.upd.c == 2 ? 2 : 1) : 0;
  // (an x-slab context answers "t1_g16" and "fast_xt" 4 for its local row count, as it always has)
  else if (k == "t1_g16") *value = (pl.xt_one_row.family == XT1_F64_G16 && pb.nx == pl.xt_one_row.n) ? 1 : 0;
  else if (k == "dual_one") *value = (pl.dual.family == DUAL_ROW || pl.dual.family == DUAL_ROW_MIXED) && pl.dual.a;
  else if (k == "fast_xt")   // the window kernel's fp32 fast family (XT_FAST .. XT_DMA_HR are the key's codes 1 .. 5)
    *value = pl.xt.family > XT_DMA_HR ? 0 : (pl.xt.family == XT_DMA && pb.nx != 4096) ? (int)XT_BATCH : pl.xt.family;
  else if (k == "half_real") *value = pl.half_real ? 1 : 0;
  else if (k == "fourstep") *value = pl.fourstep ? 1 : 0;
  else if (k == "glb_line") *value = pl.glb_line ? 1 : 0;
  else if (k == "ip_rows") *value = pl.ip_rows ? 1 : 0;   // fp64 ny = 8192 row pairs in one padded line
  else if (k == "upd8192") *value = pl.upd.family == UPD_8192;   // fp64 ny = 8192: 2-row fast update
  else if (k == "upd64_pair") *value = pl.upd.family == UPD_PAIR64;   // fp64 ny = 2048 / 4096: update on 8-row task pairs
  else if (k == "upd_grid") *value = pl.g_fast_upd;   // workgroups of the fast update kernels
  else if (k == "tc_spec") *value = pl.tc_spec ? 1 : 0;   // fp64 C3: task-order residual spectrum
  else if (k == "to_c4") *value = pl.to_c4 ? 1 : 0;       // C4: task-order residual spectrum + transpose
  else if (k == "thomas_chunk") *value = pl.thomas_chunk ? 1 : 0;
  else if (k == "fs_wide") *value = (pl.fourstep && pl.fs_wide && !pl.fs16) ? 1 : 0;
  else if (k == "fs16") *value = pl.fs16 ? 1 : 0;
  else if (k == "rows_rw") *value = pl.res.family == RES_FAST ? pl.res.a : 0;   // rows per fast row-kernel workgroup
  else if (k == "row_threads") *value = pl.nt_row;
  // fp32 fast rows as launched: the fused residual's threads where it runs, else the unfused kernel's
  else if (k == "res_threads")
    *value = pl.res.family != RES_FAST ? 0 : pl.res_fused.family ? pl.res_fused.threads : pl.res.threads;
  else if (k == "upd_threads") *value = fast_upd ? pl.upd.threads : 0;
  else if (k == "f64_xt") *value = pl.f64_xt ? 1 : 0;   // fp64 nx = 512 .. 8192 x transform (kernels_xt_f64.hpp)
  else if (k == "xt64_dma") *value = xt64_4k && (pl.xt.c & 4);   // ... nx = 4096: forward rows by LDS DMA, b' in registers
  else if (k == "xt64_bpr") *value = xt64_4k && (pl.xt.c & 1);        // ... nx = 4096: b' / x in registers
  else if (k == "t1_xt64") *value = pl.xt_one_row.family == XT1_F64 || pl.xt_one_row.family == XT1_F64_G16;   // fp64 T = 1: carry-free x transform
  else if (k == "report_tile") *value = pl.report_tile ? 1 : 0;         // pdhg_report_state: the tile kernel
  else if (k == "report_wgs") *value = pl.report_tile ? pl.report_wgs : 0;   // ... its workgroup target
  else return false;
  return true;
}

}  // namespace pdhg
