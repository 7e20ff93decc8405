// Every PDHG_* environment override, read in one place.  Tuning::from_env() runs once per context creation,
// IterTuning::from_env() once per iterate() call, MultiTuning::from_env() once per multi-device context; nothing
// is cached across calls (a process may change its environment between contexts).  plan_paths() (path_plan.hpp)
// turns a Tuning into decisions; no other file of csrc/ reads the environment.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <optional>

namespace pdhg {

using EnvInt = std::optional<int>;   // unset: plan_paths() keeps the default it derives from the problem

inline EnvInt env_int(const char* name) {
  const char* e = getenv(name);
  return e ? EnvInt(atoi(e)) : EnvInt();
}
inline int env_int(const char* name, int dflt) { return env_int(name).value_or(dflt); }
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

// context creation
struct Tuning {
  // PDHG_ALLOC: "contig" (1) / "none" (-1) override the default (contiguous planes for fp32 2-D contexts only)
  int alloc_mode = 0;

  // ---- 2-D x transform ----
  EnvInt xt64;             // PDHG_XT64=0: fp64 generic runtime-radix x kernel instead of k_precond_xt_f64_2d (A/B)
  int xt64_var = 0;        // PDHG_XT64_VAR: nx = 2048 shapes of it (1: 256 threads, b' in LDS; 2: 256; 3: 1024; A/B)
  EnvInt xt64_dma;         // PDHG_XT64_DMA=0: its nx = 4096 form without LDS-DMA staged forward rows (default on)
  EnvInt xt64_bpr;         // PDHG_XT64_BPR: ... b' / x in registers (default: with the DMA form, which needs it; A/B)
  bool t1_xt = true;       // PDHG_T1_XT=0: T = 1 windows without the carry-free x transform (k_precond_x_t1_2d)
  bool t1_g16 = true;      // PDHG_T1_G16=0: its fp64 form with every twiddle seed in LDS (A/B)
  int short_t_xt = 16;     // PDHG_SHORT_T_XT: windows below this take the single-role x kernel (0: never)
  EnvInt xt_ws;            // PDHG_XT_WS: warp-specialised x kernel (default: nx = 4096 on longer windows)
  EnvInt xt_batch;         // PDHG_XT_BATCH: row-batched x kernel (default: nx = 4096 / 2048, T >= 4)
  int xt_rpre = 0;         // PDHG_XT_RPRE: rows prefetched across the FFT of the batched kernel (2; measured loser)
  bool xt_pair = false;    // PDHG_XT_PAIR=1: batched x transform as 2 rows x 512 threads (measured loser)
  EnvInt xt_dma;           // PDHG_XT_DMA: LDS-DMA staged rows at nx = 4096 (default on: C3 14.24 -> 13.52 ms)
  EnvInt xt_dma_hr;        // PDHG_XT_DMA_HR=0: warp-specialised half-real kernel instead (default: DMA for T >= 4)

  // ---- 2-D row kernels ----
  EnvInt upd_t1;           // PDHG_UPD_T1: fp64 ny = 2048 update on one-row windows (0: 512 threads, 1: PF 4, 2: PF 2)
  EnvInt res64_nt2048;     // PDHG_RES64_NT2048: fp64 unfused residual threads at ny = 2048 (256 / 512; A/B)
  EnvInt upd8192;          // PDHG_UPD8192=0: fp64 ny = 8192 update through the generic kernel (A/B)
  EnvInt upd_pair;         // PDHG_UPD_PAIR: fp64 ny = 2048 / 4096 update on 8-row task pairs (k_invy_update_pair_2d; default: T >= 100)
  int upd_pair_pf = 4;     // PDHG_UPD_PAIR_PF: ... its old-phi row pairs in flight (2..4)
  EnvInt upd_grid;         // PDHG_UPD_GRID: at most this many workgroups in the fp64 4-row / 8-row update (tests)
  int rows_var = 0;        // PDHG_ROWS_VAR=1: fp32 ny = 2048 / 4096 rows as 4 rows per block (measured loser)
  int half_nt = 3;         // PDHG_HALF_NT: ny = 4096 rows with 512 threads (bit 0 fused residual, bit 1 update)
  // PDHG_RES64_NT=1024: fp64 fused residual threads at ny = 4096 (GPT = 1, 128 VGPRs + 108 B of spills; interleaved
  // A/B at C3 fp64, round 5: 17.1 vs 15.5 ms, so 512 stays)
  int res64_nt = 512;
  int upd_pf = 4;          // PDHG_UPD_PF: update kernel (512 threads): old-phi row pairs in flight (1..4)
  EnvInt tile_j;           // PDHG_TILE_J: time rows per residual task tile (default 8 where the row groups tile)
  EnvInt res64;            // PDHG_RES64=0: fp64 generic row-pair residual / update
  EnvInt tc_spec;          // PDHG_TC_SPEC: fp64 C3 residual spectrum in task order (default: windows of >= 100 rows)
  EnvInt fuse_res;         // PDHG_FUSE_RES: 1 forces the fused residual for any eligible size, 0 turns it off
  EnvInt c4_to;            // PDHG_C4_TO=0: C4's fused residual stores blocked 16-B chunks (A/B)

  // ---- 2-D dual ----
  int short_t_dual = 3;    // PDHG_SHORT_T: windows below this sweep row-per-thread (0: never)
  EnvInt dual64;           // PDHG_DUAL64=0: fp64 generic per-point dual kernel
  EnvInt dual_rx;          // PDHG_DUAL_RX: x rows per workgroup of k_dual_lds_2d (0: row-per-thread kernel)
  EnvInt dual_ypl;         // PDHG_DUAL_YPL=2: fp64 LDS dual with 2 y per lane
  int dual_one = 1;        // PDHG_DUAL_ONE: one-row workgroups of k_dual_fast_2d (0 marching form, 2 fp64 4 waves/SIMD)
  // PDHG_DUAL_NBSYNC=1: k_dual_lds_2d step sync through neighbour counts instead of the block barrier.  Bitwise the
  // same results; measured (round 4, interleaved A/B at C3): fp32 dual 31.16 -> 31.85 ms, fp64 60.39 -> 60.39 ms,
  // so the barrier is not what bounds the sweep and the default stays the barrier
  bool nbsync = false;
  // PDHG_DUAL_ORDER: workgroup -> tile order of k_dual_lds_2d (dual_order.hpp).  0: x-fastest (one y strip resident
  // at a time); 1 / 2 / 4: band order with XB = 1 / 2 / 4 x tiles per band (an XCD's workgroups cover whole grid rows)
  EnvInt dual_order;
  int dbg = 0;            // PDHG_DBG: timing experiments only (KP::dbg)

  // ---- 1-D ----
  EnvInt fourstep;         // PDHG_FOURSTEP=0: nx = 65536 through the generic global-scratch passes
  bool fs_wide = true;     // PDHG_FS_WIDE=0: fp32 four-step DHT with 16-column tiles
  EnvInt fs16;             // PDHG_FS16=0: the 256 x 256 four-step forms instead of the 16 x 4096 split
  int f16_group = 16;      // PDHG_F16_GROUP: rows n1 per load group of k_f16a_fwd_1d (4, 8, 16; 16 measured best)
  EnvInt fuse_res1d;       // PDHG_FUSE_RES1D=0: 1-D residual unfused (A/B)
  int fr1d_chunks = 8;     // PDHG_FR1D_CHUNKS: time chunks of the 1-D fused dual sweep (1..32)
  EnvInt thomas_chunk;     // PDHG_THOMAS_CHUNK=0: one-thread-per-mode t-solve

  // ---- sums, rho_alp_iters > 1 ----
  bool k1_outer = true;    // PDHG_K1_OUTER=0: always run the outer-sum pass after a one-sub-iteration loop
  bool fold_fin = false;   // PDHG_FOLD_FIN=1: fold + finalize of a folded partial table in one launch
  int g_outer = 2048;      // PDHG_G_OUTER: workgroups of k_outer_sums (64..4096)
  int head_xrun = 4;       // PDHG_HEAD_XRUN: x rows per workgroup of the head form's chunk passes (>= 1)
  EnvInt dual_multi;       // PDHG_DUAL_MULTI: the dual loop in chunk passes (default: from 2^25 points; A/B, tests)
  EnvInt dual_head;        // PDHG_DUAL_HEAD: ... the head form below that (A/B, tests)
  EnvInt spec;             // PDHG_SPEC=0: iterate() never uses the speculative schedule (A/B, tests)
  bool fin_merge = true;   // PDHG_FIN_MERGE=0: its dual and outer finalizes as two launches (A/B, tests)

  // ---- solution report ----
  EnvInt report_tile;      // PDHG_REPORT_TILE=0: the per-point report kernel instead of the 8-row tile (A/B, tests)
  // PDHG_REPORT_WGS: workgroups the tile kernel aims for; grids with fewer tiles split the window into time chunks
  // (>= 1; 1 = every tile marches the whole window, which is how the tests reach the march on small grids)
  int report_wgs = 1024;

  static Tuning from_env() {
    Tuning t;
    if (const char* e = getenv("PDHG_ALLOC")) t.alloc_mode = !strcmp(e, "contig") ? 1 : !strcmp(e, "none") ? -1 : 0;
    t.xt64 = env_int("PDHG_XT64");
    t.xt64_var = env_int("PDHG_XT64_VAR", t.xt64_var);
    t.xt64_dma = env_int("PDHG_XT64_DMA");
    t.xt64_bpr = env_int("PDHG_XT64_BPR");
    t.t1_xt = env_flag("PDHG_T1_XT", t.t1_xt);
    t.t1_g16 = env_flag("PDHG_T1_G16", t.t1_g16);
    t.short_t_xt = env_int("PDHG_SHORT_T_XT", t.short_t_xt);
    t.xt_ws = env_int("PDHG_XT_WS");
    t.xt_batch = env_int("PDHG_XT_BATCH");
    t.xt_rpre = env_int("PDHG_XT_RPRE", t.xt_rpre);
    t.xt_pair = env_flag("PDHG_XT_PAIR", t.xt_pair);
    t.xt_dma = env_int("PDHG_XT_DMA");
    t.xt_dma_hr = env_int("PDHG_XT_DMA_HR");
    t.upd_t1 = env_int("PDHG_UPD_T1");
    if ((t.res64_nt2048 = env_int("PDHG_RES64_NT2048"))) t.res64_nt2048 = *t.res64_nt2048 == 256 ? 256 : 512;
    t.upd8192 = env_int("PDHG_UPD8192");
    t.upd_pair = env_int("PDHG_UPD_PAIR");
    t.upd_pair_pf = std::max(2, std::min(4, env_int("PDHG_UPD_PAIR_PF", t.upd_pair_pf)));
    if ((t.upd_grid = env_int("PDHG_UPD_GRID"))) t.upd_grid = std::max(1, *t.upd_grid);
    t.rows_var = env_int("PDHG_ROWS_VAR", t.rows_var);
    t.half_nt = env_int("PDHG_HALF_NT", t.half_nt);
    t.res64_nt = env_int("PDHG_RES64_NT", t.res64_nt) == 1024 ? 1024 : 512;
    t.upd_pf = env_int("PDHG_UPD_PF", t.upd_pf);
    t.tile_j = env_int("PDHG_TILE_J");
    t.res64 = env_int("PDHG_RES64");
    t.tc_spec = env_int("PDHG_TC_SPEC");
    t.fuse_res = env_int("PDHG_FUSE_RES");
    t.c4_to = env_int("PDHG_C4_TO");
    t.short_t_dual = env_int("PDHG_SHORT_T", t.short_t_dual);
    t.dual64 = env_int("PDHG_DUAL64");
    t.dual_rx = env_int("PDHG_DUAL_RX");
    t.dual_ypl = env_int("PDHG_DUAL_YPL");
    t.dual_one = env_int("PDHG_DUAL_ONE", t.dual_one);
    t.nbsync = env_flag("PDHG_DUAL_NBSYNC", t.nbsync);
    if ((t.dual_order = env_int("PDHG_DUAL_ORDER")) && *t.dual_order != 1 && *t.dual_order != 2 && *t.dual_order != 4)
      t.dual_order = 0;
    t.dbg = env_int("PDHG_DBG", t.dbg);
    t.fourstep = env_int("PDHG_FOURSTEP");
    t.fs_wide = env_flag("PDHG_FS_WIDE", t.fs_wide);
    t.fs16 = env_int("PDHG_FS16");
    t.f16_group = env_int("PDHG_F16_GROUP", t.f16_group);
    t.fuse_res1d = env_int("PDHG_FUSE_RES1D");
    t.fr1d_chunks = std::max(1, std::min(32, env_int("PDHG_FR1D_CHUNKS", t.fr1d_chunks)));
    t.thomas_chunk = env_int("PDHG_THOMAS_CHUNK");
    t.k1_outer = env_flag("PDHG_K1_OUTER", t.k1_outer);
    t.fold_fin = env_flag("PDHG_FOLD_FIN", t.fold_fin);
    t.g_outer = std::max(64, std::min(4096, env_int("PDHG_G_OUTER", t.g_outer)));
    t.head_xrun = std::max(1, env_int("PDHG_HEAD_XRUN", t.head_xrun));
    t.dual_multi = env_int("PDHG_DUAL_MULTI");
    t.dual_head = env_int("PDHG_DUAL_HEAD");
    t.spec = env_int("PDHG_SPEC");
    t.fin_merge = env_flag("PDHG_FIN_MERGE", t.fin_merge);
    t.report_tile = env_int("PDHG_REPORT_TILE");
    t.report_wgs = std::max(1, env_int("PDHG_REPORT_WGS", t.report_wgs));
    return t;
  }
};

// every iterate() call
struct IterTuning {
  EnvInt graph;              // PDHG_GRAPH=0: no HIP-graph replay of iteration windows (sticks to the context once set)
  // PDHG_SPEC_FORCE=1 (tests): speculate from the first iteration and again right after every halt, so the halt /
  // finish path runs as often as the loop needs more than one sub-iteration
  bool spec_force = false;

  static IterTuning from_env() {
    IterTuning t;
    t.graph = env_int("PDHG_GRAPH");
    t.spec_force = env_flag("PDHG_SPEC_FORCE", t.spec_force);
    return t;
  }
};

// multi-device context creation (pdhg_multi.hpp)
struct MultiTuning {
  int parts = 2;             // PDHG_MULTI_PARTS: column-block parts of the carry exchange (>= 1)
  bool kcopy = false;        // PDHG_MULTI_KCOPY=1: same-device plane copies as a kernel (diagnostic)
  int sync_mask = 0;         // PDHG_MULTI_SYNC: full barrier at these step() marks, bit i = mark i (diagnostic)
  bool one_stream = false;   // PDHG_MULTI_ONESTREAM=1: planes received on the main stream (diagnostic)
  bool step_fence = false;   // PDHG_MULTI_STEP_FENCE=1: every stream waits for the previous step's end
  bool peer_fold = false;    // PDHG_MULTI_PEER_FOLD=1: per-device peer fold of the sums (opt-in)

  static MultiTuning from_env() {
    MultiTuning t;
    t.parts = std::max(1, env_int("PDHG_MULTI_PARTS", t.parts));
    t.kcopy = env_flag("PDHG_MULTI_KCOPY", t.kcopy);
    if (const char* e = getenv("PDHG_MULTI_SYNC")) t.sync_mask = (int)strtol(e, nullptr, 0);
    t.one_stream = env_flag("PDHG_MULTI_ONESTREAM", t.one_stream);
    t.step_fence = env_flag("PDHG_MULTI_STEP_FENCE", t.step_fence);
    t.peer_fold = env_flag("PDHG_MULTI_PEER_FOLD", t.peer_fold);
    return t;
  }
};

}  // namespace pdhg
