/*
 * pdhg.h — C ABI of the MI355X-native PDHG iteration for Hamilton–Jacobi
 * optimal-control PDEs (drop-in for the hot path of
 * TingweiMeng/PDHG-optimal-control, jaxsrc/).
 *
 * Plain C types only: host pointers + sizes, an opaque context that owns all
 * device (HBM) memory.  Bound from Python with ctypes by
 * pdhg-optimal-control_amd/pdhg_amd/_native.py; any other FFI (cffi, a C++
 * caller) can bind the same symbols.  See INTEGRATION.md.
 *
 * Reference interfaces replaced (file:line in jaxsrc/):
 *   pdhg_create              problem setup done by solve_HJ            run_example.py:157-191
 *                            + set_up_example_fns / compute_Dxx_fft_fv set_fns.py:52-166, utils/utils_precond.py:42-71
 *   pdhg_set_state/get_state the (phi, rho, alp) arrays passed between the jitted updates
 *                                                                       utils/utils_pdhg_solver.py:48-50, 96-98 (returns)
 *   pdhg_update_primal       update_primal_1d / update_primal_2d      update_fns_in_pdhg.py:135-147
 *                            (+ phi_bar = 2 phi' - phi and err1 sums,  utils/utils_pdhg_solver.py:55, 58)
 *   pdhg_update_dual         update_dual_alternative (<= rho_alp_iters update_fns_in_pdhg.py:167-180
 *                            calls of update_dual_oneiter :150-165)
 *   pdhg_iterate             the body of PDHG_solver_oneiter's loop    utils/utils_pdhg_solver.py:51-88
 *                            (primal, extrapolation, dual, err1/err2, convergence and NaN stop tests)
 *
 * Return convention: every function returns PDHG_OK (0) or a negative
 * pdhg_status; pdhg_last_error() gives the message (thread-local).
 * Threading: a context is single-caller.  It drives one GPU on its own HIP
 * stream (every entry point makes the context's device current first).  Multi-GPU:
 * either one process per GPU with a t-slab / x-slab context each and the caller's
 * communicator (pdhg_create_slab, pdhg_create_xslab; pdhg_amd/slab.py over RCCL), or
 * one host thread over a device list (pdhg_create_multi).  See DESIGN.md §7.
 * The two post-processing passes -- the solution report and the closed-loop trajectories -- run on single contexts
 * (pdhg_report_state / pdhg_report_rows / pdhg_trajectories), on multi-device contexts (pdhg_multi_report_state /
 * pdhg_multi_report_rows / pdhg_multi_trajectories) and slab by slab on t-slab contexts (pdhg_slab_report /
 * pdhg_slab_report_rows / pdhg_slab_trajectories, chained by the caller: pdhg_amd/slab.py SlabRunner.report);
 * x-slab contexts have neither.  A third pass, the policy check (pdhg_policy_eval: the closed-loop cost of the
 * controls against phi), runs on single contexts only.
 */
#ifndef PDHG_MI355X_H
#define PDHG_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

#define PDHG_ABI_VERSION 1

typedef enum pdhg_status {
  PDHG_OK = 0,
  PDHG_ERR_ARG = -1,          /* bad argument (null pointer, size, value)            */
  PDHG_ERR_UNSUPPORTED = -2,  /* (egno, ndim, bc) or size combination not supported  */
  PDHG_ERR_HIP = -3,          /* HIP runtime error (message has the HIP error string) */
  PDHG_ERR_STATE = -4,        /* call order / state error (e.g. dual before primal)   */
  PDHG_ERR_NOMEM = -5         /* device allocation failed                             */
} pdhg_status;

/* Problem description: one PDHG time window of T unknown time rows
 * (T = time_step_per_PDHG - 1, utils/utils_pdhg_solver.py:121-137).
 * Mirrors the static arguments of the reference's jitted updates. */
typedef struct pdhg_problem {
  int egno;          /* example 1, 2 or 3                          set_fns.py:52            */
  int ndim;          /* 1 or 2                                                              */
  int bc_x, bc_y;    /* 0 periodic, 1 Neumann (egno 3: bc_x = 1)   run_example.py:229-240   */
  int nx, ny;        /* grid; ny = 1 when ndim == 1                                         */
  int T;             /* unknown time rows: phi is [T+1, nx(,ny)], rho / alp are [T, ...]    */
  int precision;     /* 4 = fp32 (throughput), 8 = fp64 (the reference's arithmetic; bench.py's
                        default), 12 = mixed: fp32 state, tables and transforms with phi and
                        phi_bar held, differenced and updated in fp64 (single 2-D contexts:
                        pdhg_create; ndim 1, the slab and multi-device creates return
                        PDHG_ERR_UNSUPPORTED).  Any other value: PDHG_ERR_ARG               */
  int rho_alp_iters; /* max dual sub-iterations per outer iteration (reference: 10)         */
  int reserved0;
  double dx, dy, dt;
  double epsl;       /* viscosity epsilon                                                   */
  double c_on_rho;   /* c in R_T += c/dt                           update_fns_in_pdhg.py:80 */
  double C, pow_, Ct;/* preconditioner; pow_ and Ct are honoured in 1-D only, as the
                        reference (update_fns_in_pdhg.py:146)                              */
  const double* xs;  /* [nx] grid x coordinates (x_arr[0,:,0(,0)])                         */
  const double* ys;  /* [ny] grid y coordinates (x_arr[0,0,:,1]); NULL when ndim == 1      */
} pdhg_problem;

typedef struct pdhg_stats {
  int iters_run;     /* outer iterations executed by this call (incl. the stopping one)     */
  int status;        /* 0 = ran all n_iters, 1 = converged (err1<eps && err2<eps), 2 = NaN  */
  int inner_last;    /* dual sub-iterations of the last executed outer iteration            */
  int inner_total;   /* dual sub-iterations summed over this call                            */
  double err1;       /* primal error ||phi'-phi||/||phi|| of the last executed iteration     */
  double err2;       /* dual error (utils/utils_pdhg_solver.py:60-68)                         */
  double err_inner;  /* last dual sub-iteration error (update_fns_in_pdhg.py:162-164)        */
  double rho_min, rho_max; /* not computed (NaN); pdhg_report_state / pdhg_multi_report_state give the rho range */
  int nan_seen;      /* a NaN appeared in phi' or rho' during this call                        */
  int first_nan_iter; /* iteration of this call (1-based) whose phi' or rho' first held a NaN; 0: none */
} pdhg_stats;

typedef struct pdhg_ctx pdhg_ctx;

const char* pdhg_last_error(void);
int pdhg_abi_version(void);

/* Number of HIP devices visible (0 when no GPU / no driver). */
int pdhg_device_count(int* count);

/* Allocates all device buffers for the window.  device = HIP ordinal. */
int pdhg_create(const pdhg_problem* prob, int device, pdhg_ctx** out);
int pdhg_destroy(pdhg_ctx* ctx);

/* State in the reference layout, float64 host arrays (C order):
 *   phi [T+1][nx][ny], rho [T][nx][ny],
 *   alp: n_alp arrays (2 in 1-D, 4 in 2-D) each [T][nx][ny][n_ctrl]
 *        (n_ctrl = 1 in 1-D and for egno 3, 2 otherwise), passed as one
 *        contiguous [n_alp][T][nx][ny][n_ctrl] block.
 * Only the live control components are stored on the device:
 * set_state fails with PDHG_ERR_UNSUPPORTED if a dead component is non-zero;
 * get_state writes zeros there.  A null array is not transferred: set_state overwrites the given parts of the
 * current state and keeps the device's values of the others (window marching re-seeds phi alone when rho / alp
 * are the ones the device holds); it resets the iteration / stop bookkeeping either way. */
/* A mixed context (precision 12) moves phi and phi_bar as full doubles in every call below (set_state followed by
 * get_state returns phi bit for bit); rho and alp round to float as in an fp32 context. */
int pdhg_set_state(pdhg_ctx* ctx, const double* phi, const double* rho, const double* alp);
int pdhg_get_state(pdhg_ctx* ctx, double* phi, double* rho, double* alp);
int pdhg_get_phi_bar(pdhg_ctx* ctx, double* phi_bar);   /* [T+1][nx][ny] */
/* The spectral work buffer as the last primal update left it: the preconditioner's output (x kernel's inverse
 * transform rows) in its blocked layout, `count` leading elements converted to double (count <= the buffer's
 * T * nb * nx * B elements in 2-D, T * nx in 1-D; single contexts).  For tests that pin the x kernels' output itself. */
int pdhg_get_work(pdhg_ctx* ctx, double* out, long long count);
/* Rows [row0, row0 + nrows) of the state in the reference layouts (a window of 3.4e9 points per array, C3's and
 * C4's, does not fit a host copy): phi / phi_bar rows of [T+1] -> [nrows][nx][ny], rho rows of [T] -> [nrows][nx][ny],
 * alp -> [n_alp][nrows][nx][ny][n_ctrl] (dead components zero).  Null pointers are skipped; rho / alp need
 * row0 + nrows <= T.  Same values as the matching rows of pdhg_get_state / pdhg_get_phi_bar. */
int pdhg_get_rows(pdhg_ctx* ctx, int row0, int nrows, double* phi, double* phi_bar, double* rho, double* alp);
/* phi_bar input of the drop-in dual update (update_dual_oneiter's first argument). */
int pdhg_set_phi_bar(pdhg_ctx* ctx, const double* phi_bar);

/* The reference's PDHG_multi_step initial state for a window
 * (utils/utils_pdhg_solver.py:123-137): every phi row = g, rho = c_on_rho,
 * alp = 0.  g: [nx][ny] host float64.  Built on the device (HBM-resident). */
int pdhg_init_state(pdhg_ctx* ctx, const double* g);

/* One primal update: phi <- phi + tau * H1^{-1}(cont_residual(rho, alp));
 * also forms phi_bar = 2 phi' - phi and the err1 sums. */
int pdhg_update_primal(pdhg_ctx* ctx, double tau);

/* update_dual_alternative: up to rho_alp_iters sub-iterations with early exit
 * at err < eps; *inner_used receives the sub-iterations executed. */
int pdhg_update_dual(pdhg_ctx* ctx, double sigma, double eps, int rho_alp_iters, int* inner_used);

/* Errors of the last primal+dual pair (err1, err2) as utils_pdhg_solver.py:58-68. */
int pdhg_errors(pdhg_ctx* ctx, double* err1, double* err2);

/* Error of the last dual sub-iteration (update_fns_in_pdhg.py:162-164), the value
 * update_dual_oneiter returns as its third output. */
int pdhg_inner_error(pdhg_ctx* ctx, double* err);

/* Up to n_iters outer iterations on the device with the reference's stop
 * rules (converged, then NaN).  tau = stepsz/1.5, sigma = stepsz*1.5
 * (utils_pdhg_solver.py:44-46).  No host synchronisation per iteration. */
int pdhg_iterate(pdhg_ctx* ctx, int n_iters, double tau, double sigma, double eps, int rho_alp_iters,
                 pdhg_stats* out);

/* Stop rules of pdhg_iterate (default: both on, as the reference).  Benchmarks may turn the NaN
 * stop off so a diverging configuration still executes exactly n_iters iterations. */
int pdhg_set_stop_rules(pdhg_ctx* ctx, int stop_on_converge, int stop_on_nan);

/* Blocks until the context's stream is idle. */
int pdhg_synchronize(pdhg_ctx* ctx);

/* Device bytes held by the context. */
int pdhg_device_bytes(pdhg_ctx* ctx, unsigned long long* bytes);

/* Which kernel variant a context selected (no reference counterpart; tests and benches assert the fast
 * paths engaged): "fused_residual" 1/0 (the dual sweep forms the next residual, k_dual_lds_2d FR; fp32 and
 * fp64 -- fp64 on 128-column strips with 4-row residual tasks, 2-row tasks at ny = 8192; fp32 ny = 8192 on 4-row
 * tasks),
 * "fast_rows" 1/0 (fp32 8/4-row y-transform kernels), "fast_dual" (-1 generic, 0 row-per-thread,
 * RX rows through LDS), "dual_ypl" (y per lane of the LDS dual: 4, or 2 for fp64 with PDHG_DUAL_YPL=2;
 * 0 without it), "fast_xt" (0 generic, 1 single-role, 2 warp-specialised, 3 row-batched,
 * 4 row-batched with LDS-DMA staging x-transform, 5 its half-real form at nx = 8192), "half_real", "fourstep", "fs16" (1-D nx = 65536 as
 * 16 x 4096, fp32 and fp64), "fs_wide", "glb_line", "thomas_chunk" (1-D t-solve in chunks: 32 rows per wave
 * fp32, 16 rows per half-wave fp64), "rows_rw", "res_threads", "upd_threads",
 * "row_threads" (threads of the generic row kernels), "res64" 1/0 (fp64 residual and update through the
 * 4-row fast kernels, ny = 2048 / 4096), "contig_fail" (large arrays of an fp32 2-D context that fell back
 * from a physically contiguous allocation to hipMalloc; environment PDHG_ALLOC=contig|none overrides the
 * contiguous-for-fp32-2-D default), "dual64" 1/0 (fp64 contexts: the row-per-thread time-marching dual
 * k_dual_fast_2d<EGNO, double>, or with nx % 8 == 0 and T >= 3 the LDS-row sweep k_dual_lds_2d<EGNO, 8, .., double>;
 * default on where ny % 256 == 0, environment PDHG_DUAL64=0 selects the generic per-point kernel), "f64_xt" 1/0 (fp64
 * nx = 512 ... 8192: k_precond_xt_f64_2d; PDHG_XT64=0 the generic kernel), "xt64_dma" 1/0 (its nx = 4096
 * column-pair form on single contexts with the forward rows staged by LDS DMA and b' in registers; PDHG_XT64_DMA=0
 * off; "xt64_bpr" 1/0: b' in registers, PDHG_XT64_BPR), "ip_rows" 1/0 (fp64 ny = 8192: row pairs in
 * one padded line), "upd8192" 1/0 (fp64 ny = 8192 with half-real x blocks: the 2-row fast update), "upd64_pair" 1/0
 * (fp64 ny = 2048 / 4096 on single contexts with nx % 8 == 0: the update on pairs of 4-row tasks,
 * k_invy_update_pair_2d, phi' and phi_bar bitwise the 4-row kernel's; default on windows of >= 100 rows, PDHG_UPD_PAIR=1 / 0 forces it on / off), "upd_grid" (workgroups
 * of the fast update kernels as launched; PDHG_UPD_GRID caps the fp64 4-row / 8-row ones, tests), "tc_spec" 1/0
 * (fp64 C3 shape, windows of >= 100 rows: the residual spectrum in task order), "t1_xt64" 1/0 (fp64 one-row windows at a power-of-two nx in
 * 512..4096: the carry-free k_precond_x_t1_2d<..., double>; PDHG_T1_XT=0 off), "graph" 1/0 (pdhg_iterate replays
 * windows of iterations from a captured HIP graph; default on, environment PDHG_GRAPH=0 launches every
 * iteration eagerly), "graph_window" (iterations per replayed graph), "mixed" 1/0 (precision 12: fp32 state with
 * fp64 phi / phi_bar; the other keys then answer for the fp32 kernels chosen -- "fast_dual" 0 and "fused_residual" 0
 * always, the dual being the row-per-thread sweep or the generic per-point kernel -- and "dual64" is 0).
 *
 * The kernel each 2-D stage launches (the launchers switch on exactly these; 1-D contexts answer 0): "<stage>_kernel"
 * is the family code below, "<stage>_shape" the threads per workgroup as launched, and "<stage>_n", "<stage>_a",
 * "<stage>_b", "<stage>_c" the family's template integers (line length; lines or rows per workgroup / ONE / RX; thread
 * bound, RB or YPL; PF, RPRE or the fp64 x kernel's BPR 1 | TC 2 | DMA 4 flags; 0 where unused), for the stages
 *   "xt" (x transform of a window): 1 single-role k_precond_xt_fast_2d, 2 warp-specialised k_precond_xt_ws_2d,
 *     3 row-batched k_precond_xt_batch_2d, 4 k_precond_xt_dma_2d, 5 its half-real form (1 .. 5 are "fast_xt"'s codes),
 *     6 fp64 k_precond_xt_f64_2d, 7 the generic runtime-radix k_precond_xt_2d;
 *   "xt_one_row" (T = 1 windows of single and x-slab contexts; 0: the window kernel runs): k_precond_x_t1_2d in
 *     8 fp32, 9 fp64, 10 fp64 with the G16 twiddle seeds;
 *   "res" (residual without the fused sweep) and "res_fused" (0: none; the kernel that completes the rows the fused dual
 *     sweep formed): 1 generic k_res_fwdy_2d, 2 fp32 k_res_fwdy_fast_2d, 3 its fp64 4-row form, 4 fp32
 *     k_res_fwdy_fused_2d, 5 its fp64 form;
 *   "upd": 1 generic k_invy_update_2d, 2 k_invy_update_mixed_2d, 3 fp32 k_invy_update_fast_2d, 4 k_invy_update_fast_mixed_2d,
 *     5 the fp64 4-row k_invy_update_fast_2d, 6 its one-row form with G16 seeds, 7 k_invy_update_pair_2d, 8 the 2-row
 *     tasks at ny = 8192;
 *   "dual" and "dual_fused" (0: none; the sweep that also forms the next residual): 1 per-point k_dual_2d,
 *     2 k_dual_mixed_2d, 3 row-per-thread k_dual_fast_2d, 4 k_dual_fast_mixed_2d, 5 k_dual_lds_2d, 6 its FR form.
 * The older "as launched" keys ("fast_xt", "t1_xt64", "t1_g16", "xt64_dma", "xt64_bpr", "rows_rw", "res_threads",
 * "upd_threads", "res64_nt", "upd_t1", "upd64_pair", "upd8192", "fast_dual", "dual_ypl", "dual_one") are read off the
 * same choices.  New keys do not change PDHG_ABI_VERSION (no struct, no signature). */
int pdhg_path_info(pdhg_ctx* ctx, const char* key, int* value);
/* The same keys for the single context pdhg_create would build from `prob` under the current environment, without a
 * device: the problem is validated as in pdhg_create (same status codes) and the kernel paths are planned, nothing is
 * created.  The runtime counters ("contig_fail", "spec_iters", "spec_halts", "graph", "graph_window") belong to a
 * context and return PDHG_ERR_ARG here. */
int pdhg_plan_info(const pdhg_problem* prob, const char* key, int* value);

/* Per-launch kernel timing for the benchmark: HIP events recorded on the
 * context's stream around every launch of the named kernel class
 * ("dual", "precond_fwd", "precond_bwd", "residual", "update") while
 * enabled.  Returns the accumulated milliseconds and launch count. */
int pdhg_profile_enable(pdhg_ctx* ctx, int enable);
int pdhg_profile_query(pdhg_ctx* ctx, const char* kernel_class, double* total_ms, int* launches);

/* Algorithmic HBM bytes of one outer iteration for k dual
 * sub-iterations, and of one launch of the named kernel class.  A mixed context prices phi / phi_bar at 8 bytes
 * and everything else at 4 (update 28 N, dual 48 N against 16 N / 44 N in fp32 and 32 N / 88 N in fp64). */
int pdhg_algorithmic_bytes(pdhg_ctx* ctx, int k, const char* kernel_class, double* bytes);

/* ---------------- closed-loop trajectories from the resident controls ----------------
 * Replaces compute_traj_1d / extend_bdry_2d / compute_traj_2d (run_example.py:18-155, used at :342-393) for windows
 * whose alp does not fit a host copy: n_sample paths of dx = f(alp(x, t), x, t) dt + sqrt(2 epsl) dW are marched
 * through the context's T rows on the device, explicit Euler-Maruyama with the context's dt and epsl.  Step
 * ind = 0 .. T-1 interpolates row T-1-ind of the current alp set (the reference's alp[:, ::-1], :347: the PDE runs
 * backward from the terminal cost) and forms the velocity with the f >= 0 / f < 0 split of get_f_vals_1d / _2d.
 * Positions and the update are float64 in every context precision; alp is read as the context stores it.
 * Interpolation (method 0 linear, 1 nearest) as the reference's:
 *   1-D linear   jnp.interp(x, x_arr, alp, period = x_period);
 *   1-D nearest  argmin |x_arr - x mod P|, first index on ties, no wrap (past the last node's midpoint the last
 *                node, not node 0); the 1-D grid lies in [0, x_period);
 *   2-D          extend_bdry_2d evaluated point-wise: periodic axes wrap, a Neumann axis (bc_x = 1) repeats its edge
 *                value outside the grid, center_x / center_y give the period cell [-P/2, P/2) instead of [0, P);
 *                bilinear, or the nearer node per axis with ties to the lower one (scipy interpn).
 * f is evaluated at x mod P on periodic axes and at the raw coordinate on the Neumann axis (:139-145).
 * Noise (only when the context's epsl > 0): `noise` = standard normals [T][n_sample][ndim] drawn by the caller (the
 * reference's per-step np.random.normal order), or NULL for the device generator: Philox4x32-10 with
 *   key = (seed low, seed high 32 bits), counter = (s low, s high, step, axis pair),  s = sample_offset + sample index,
 *   u1 = (((r0 << 32 | r1) >> 11) + 1) 2^-53,  u2 = ((r2 << 32 | r3) >> 11) 2^-53,
 *   z[axis 2p] = sqrt(-2 ln u1) cos(2 pi u2),  z[axis 2p+1] = sqrt(-2 ln u1) sin(2 pi u2)   (1-D uses z[0]),
 * a pure function of (seed, s, step, axis): splitting a run into calls with sample_offset, or the internal staging in
 * sample chunks, does not change a path.
 * Arrays are host float64, C order: x_init [n_sample][ndim]; outputs, each optional (NULL: neither allocated nor
 * copied): x_final [n_sample][ndim], traj_x [T+1][n_sample][ndim] (row 0 = x_init), traj_alp [T][n_sample][n_ctrl]
 * (the sum of the 2 / 4 interpolated arrays).  Device temporaries are staged in sample chunks of a fixed budget.
 * x_final of one call is a valid x_init of the next: windows are chained in control time, the context holding the
 * later PDE rows first.  Single contexts of pdhg_create (precision 4, 8, 12); t-slab, x-slab and multi-device
 * handles return PDHG_ERR_UNSUPPORTED from this entry point (a multi-device context: pdhg_multi_trajectories; a
 * t-slab: pdhg_slab_trajectories).  PDHG_ERR_ARG: null opts / x_init, n_sample < 1, unknown method, a period <= 0. */
typedef struct pdhg_traj_opts {
  long long n_sample;
  long long sample_offset;      /* global index of this call's sample 0 in the device noise stream (>= 0) */
  unsigned long long seed;      /* device noise stream */
  int method;                   /* 0 linear, 1 nearest */
  int center_x, center_y;
  int reserved0;
  double x_period, y_period;    /* y_period is ignored when ndim == 1 */
} pdhg_traj_opts;
int pdhg_trajectories(pdhg_ctx* ctx, const pdhg_traj_opts* opts, const double* x_init, const double* noise,
                      double* x_final, double* traj_x, double* traj_alp);

/* ---------------- policy check: closed-loop cost of the resident controls against phi ----------------
 * Does following the computed feedback alp cost what phi says it costs?  phi row 0 is the terminal cost g, phi row j
 * the value with j dt to go, and the controls of row j act between phi rows j and j+1.  So for a path started at x0
 * with the window's T rows to go,
 *   sum over steps of dt L(alp(x, t))  +  phi_0(x_T)   ~   phi_T(x0)        (in expectation when epsl > 0):
 * the dynamic-programming identity of the window, a test of phi and alp together along characteristics (the report's
 * residual norms are local).  It holds window by window in PDHG_multi_step, each window's row 0 being the previous
 * window's last row.  One read-only device pass; per sample, all in float64 without fma contraction:
 *   value    = I[phi row T](x0)
 *   the path is pdhg_trajectories' own: with the same x_init, method, periods, centring and noise (or seed /
 *              sample_offset) x_final equals its x_final bit for bit;
 *   step ind = 0 .. T-1 (alp row T-1-ind; control time runs against PDE time), a_k the interpolated control arrays the
 *              rollout forms and f_k = f(a_k) their velocities:
 *                l = sum_k keep_k L(a_k),   L(a) = a^2 / 2 (egno 1, 3) or 0 a^2 (egno 2),   summed in array order,
 *              keep_k the rollout's sign split: f_k >= 0 for arrays 0 and 2, f_k < 0 for arrays 1 and 3 (egno 3 stores
 *              arrays 0 and 1 only) -- a component the split drops moves nothing and costs nothing;
 *   running  = 0.0, then running = running + dt * l, step by step;
 *   terminal = I[phi row 0](x_T) with opts->terminal == 0; 0.0 with opts->terminal == 1, for a caller who chains
 *              windows (running of the later rows first, started at its x_final) or evaluates g in closed form;
 *   cost = running + terminal,   gap = cost - value     (gap > 0: the policy costs more than phi promises).
 * I[row](x) is linear interpolation of a phi row with the rollout's cell location and boundary extension, whatever
 * `method` the controls use: 2-D bilinear with periodic axes wrapped, the Neumann axis repeating its edge value and
 * center_x / center_y honoured; 1-D jnp.interp(period = x_period).  phi is read in the type the context stores it
 * (float in fp32 contexts, double in fp64 and mixed ones) and widened before any arithmetic.
 * Starts: x_init [n_sample][ndim] (host float64), or NULL for grid starts: every stride_x-th (and stride_y-th) node,
 * (xs[i stride_x], ys[j stride_y]) at sample index i ceil(ny / stride_y) + j; traj.n_sample is then 0 or that count, no
 * start array crosses PCIe and the per-sample outputs are a field over the strided grid.  noise as pdhg_trajectories.
 * Outputs, each optional (NULL: neither allocated nor copied): report; running, terminal, value [n_sample];
 * x_final [n_sample][ndim].  Statistics: a sample with any of running, terminal, value not finite counts in
 * n_nonfinite and is left out of every mean and extremum; means divide by n_sample - n_nonfinite; if that is 0 every
 * double of the report is NaN.  The accumulation has a fixed order (a row of partial sums per 256 samples, numbered
 * through the whole call, folded after the last staging chunk; no atomics): the report is a pure function of the
 * inputs, whatever the chunking, and a repeated call returns the same bits.
 * The call leaves the state, phi_bar, the iteration's buffers, its stop bookkeeping and a captured graph untouched.
 * Device temporaries (the staging chunks of pdhg_trajectories' budget and 128 bytes per 256 samples) live for the
 * call only.  Single contexts of pdhg_create (precision 4, 8, 12); t-slab, x-slab and multi-device handles return
 * PDHG_ERR_UNSUPPORTED, as do the grids pdhg_trajectories refuses.  PDHG_ERR_ARG: null ctx / opts, unknown method, a
 * period <= 0, terminal not 0 / 1, sample_offset < 0, x_init == NULL with a stride < 1 or with n_sample neither 0 nor
 * the strided grid's count, x_init != NULL with n_sample < 1, report and every output NULL. */
typedef struct pdhg_policy_opts {
  pdhg_traj_opts traj;     /* samples, method, periods, centring, noise stream: as pdhg_trajectories */
  int terminal;            /* 0: phi row 0 interpolated at x_final, 1: none */
  int stride_x, stride_y;  /* grid starts (x_init == NULL): every stride-th node; stride_y ignored in 1-D */
  int reserved0;
} pdhg_policy_opts;
typedef struct pdhg_policy_report {
  long long n_sample, n_nonfinite;            /* non-finite: any of running, terminal, value not finite */
  double cost_mean, value_mean, running_mean, terminal_mean;
  double gap_mean, gap_abs_mean, gap_rms, gap_abs_max, gap_lo, gap_hi;   /* over the finite samples */
} pdhg_policy_report;
int pdhg_policy_eval(pdhg_ctx* ctx, const pdhg_policy_opts* opts, const double* x_init, const double* noise,
                     pdhg_policy_report* report, double* running, double* terminal, double* value,
                     double* x_final);

/* ---------------- solution report: HJ and continuity residual norms of the resident state ----------------
 * Replaces evaluating compute_HJ_residual_1d / _2d (update_fns_in_pdhg.py:49-70) and compute_cont_residual_1d / _2d
 * (:72-96) on the returned arrays, for windows that do not fit a host copy.  One read-only device pass over phi (not
 * phi_bar) and the current rho / alp set.  Point (j, x, y), j = 0 .. T-1, pairs HJ residual row j,
 *   r = Dt phi - epsl Lap phi - f(alp) . D phi - L(alp)     (<= 0 everywhere and = 0 where rho > 0 at the saddle point),
 * rho row j, phi row j+1 and continuity residual row j+1 of the reference's [T+1] array, c (= 0 at the saddle point: it
 * is what the primal step adds to phi; the window's last row carries + c_on_rho / dt).  r and c are formed in the
 * context's precision with the iteration's own device functions (a mixed context: the phi differences and the time /
 * epsl terms in double, rounded to float once, as its dual step); the accumulation is fp64 in a fixed order (no
 * atomics: a call repeats bit for bit).
 * A point where any of r, c, rho, phi is not finite counts in n_nonfinite and is left out of every sum, mean, maximum
 * and minimum; means divide by n_points - n_nonfinite; if that is 0 every double is NaN.
 * Both calls leave the state, phi_bar, the iteration's buffers, its stop bookkeeping and a captured graph untouched.
 * The first call on a context allocates the report's own table of partial rows (128 bytes per workgroup of the
 * largest launch: up to a few MiB on the largest grids), which pdhg_device_bytes counts from then on.
 * Single contexts of pdhg_create (precision 4, 8, 12; ndim 1 and 2); t-slab, x-slab and multi-device handles return
 * PDHG_ERR_UNSUPPORTED from these two entry points (their halo rows are not resident; a multi-device context:
 * pdhg_multi_report_state / _rows, a t-slab: pdhg_slab_report / _rows).  PDHG_ERR_ARG: null ctx / out, a bad row range.
 * Path key "report_tile" 1/0 (pdhg_path_info / pdhg_plan_info): the 8-row tile kernel that reads every array once
 * (2-D, nx % 8 == 0, ny % 256 == 0, bc (0,0) or (1,0)); environment PDHG_REPORT_TILE=0 selects the per-point kernel.
 * "report_wgs": the workgroups the tile kernel aims for (grids with fewer tiles split the window into time chunks;
 * default 1024, environment PDHG_REPORT_WGS; 0 without the tile kernel). */
typedef struct pdhg_report {
  long long n_points;     /* T * nx * ny */
  long long n_nonfinite;  /* points left out of everything below */
  long long n_rho_zero;   /* finite points with rho == 0 */
  long long reserved0;
  double hj_l1, hj_l2, hj_max;   /* mean |r|, sqrt(mean r^2), max |r| */
  double hj_pos_max;             /* max of max(r, 0): violation of r <= 0 */
  double hj_active_max;          /* max |r| over points with rho > 0 (0 when there is none) */
  double compl_l1;               /* sum rho |r| / sum rho (0 when sum rho == 0) */
  double cont_l1, cont_l2, cont_max;
  double rho_min, rho_max, rho_mean;
  double phi_min, phi_max;       /* over the unknown rows 1..T */
} pdhg_report;
int pdhg_report_state(pdhg_ctx* ctx, pdhg_report* out);
/* Rows [row0, row0 + nrows) (row0 >= 0, nrows >= 1, row0 + nrows <= T) of the two fields, host float64
 * [nrows][nx][ny]; a null pointer is skipped.  The values pdhg_report_state reduces (the device planes are staged in
 * row chunks of a fixed budget). */
int pdhg_report_rows(pdhg_ctx* ctx, int row0, int nrows, double* hj, double* cont);

/* ---------------- t-slab decomposition (multi-GPU) ----------------
 * New capability: the reference (JAX, single device, README.md:6) has no distributed path.  A window's
 * T_total unknown time rows are split into contiguous slabs, one context (one GPU) each; a slab context
 * owns rows [j0, j0 + p->T) (its phi arrays hold p->T + 1 rows: row 0 is global phi row j0).  The
 * caller moves planes between slabs (RCCL; pdhg_amd/slab.py) and runs one outer iteration of
 * utils_pdhg_solver.py:51-88 as:
 *   plane_out(0, rho row 0) -> [to the previous slab] || residual(1)     (halo overlapped with interior rows)
 *   -> plane_in(0, next slab's rho row 0) -> residual(2) -> forward(tau) -> plane_out(2, [D, S1])
 *   -> [allgather] -> fixup(allDS, allGS, rank, n) -> backward(tau, sums) -> [allreduce sums]
 *   -> primal_finalize(sums) -> plane_out(1, phi_bar row T) -> [to the next slab]
 *      || dual(sigma, k, 0, sums, 1)                                        (halo overlapped with interior rows)
 *   -> plane_in(1, previous slab's phi_bar row T) -> dual(sigma, k, 0, sums, 2) -> [allreduce]
 *   -> dual_finalize(eps, 0, sums) -> per further sub-iteration s: dual(sigma, k, s, sums, 3) -> [allreduce]
 *   -> dual_finalize(eps, s, sums) -> outer(k, sums) -> [allreduce when k > 1] -> outer_finalize(eps, k, sums).
 * Neighbour-exchange form (pdhg_amd.slab default): instead of the allgather of full [D, S1] planes,
 * classify the modes once (pdhg_slab_long_modes: long-range where some slab's gain G >= delta, a few
 * thousand low frequencies), then per iteration send D to the next slab and S1 to the previous one
 * (point to point), allgather only plane_out(3) = [D, S1] of the long-range modes, and call
 * fixup_nb(D from the previous slab, S1 from the next, allLong, allGS, rank, n).  The terms dropped for
 * the other modes are below delta relative (oracle/slab_oracle.py thomas_slabs_neighbour).
 * `parts` bit 0 = the rows that do not read a halo plane, bit 1 = the row that does (residual: the last
 * row unless this is the window's last slab; dual: row 0 unless it is the first slab, then the sums).
 * The Thomas recurrences are affine in the carries entering a slab (oracle/slab_oracle.py): D = the
 * zero-carry forward sweep's last row, S1 = sum P'_k b0_k; allGS: every slab's [G, S2]
 * (pdhg_slab_carry_gain, iteration-invariant, gather once).  Planes are device pointers in the context's
 * precision (float for p->precision 4, double for 8; D/S1 and G/S2 are pairs of spectral planes, see
 * pdhg_slab_plane_size); sums are device vectors of 16 doubles.
 * All calls enqueue on the context's stream (pdhg_set_stream to share the caller's).
 * ndim 2.  fp32: a power-of-two ny in [256, 8192] (the residual's halo-row split runs the fast row kernels).
 * fp64 (the reference's arithmetic, jaxsrc/update_fns_in_pdhg.py:10): any ny; ny = 2048 / 4096 split the halo row
 * off with the 4-row kernels, other ny run the generic row kernels over the whole slab after the halo.  Any nx
 * the single context supports: the fast DHT x kernels (fp32), the fp64 nx = 4096 kernel and its half-real
 * nx = 8192 form (kernels_xt_f64.hpp), or the generic runtime-radix kernel (other nx, and egno 3's bc (1,0) DCT
 * along x, jaxsrc/utils/utils_precond.py:159-174). */
int pdhg_create_slab(const pdhg_problem* p, int j0, int T_total, int device, pdhg_ctx** out);
int pdhg_set_stream(pdhg_ctx* ctx, void* hip_stream);
int pdhg_slab_plane_size(pdhg_ctx* ctx, unsigned long long* spatial, unsigned long long* spectral);
int pdhg_slab_begin(pdhg_ctx* ctx);                                       /* reset the device loop control */
int pdhg_slab_carry_gain(pdhg_ctx* ctx, void* GS_out);                    /* [G, S2], 2 spectral planes */
int pdhg_slab_residual(pdhg_ctx* ctx, int parts);                          /* residual + y-DHT of rows */
int pdhg_slab_forward(pdhg_ctx* ctx, double tau);                          /* x-DHT + forward sweep, [D, S1] */
int pdhg_slab_fixup(pdhg_ctx* ctx, const void* all_DS, const void* all_GS, int rank, int nranks);
int pdhg_slab_long_modes(pdhg_ctx* ctx, const void* all_GS, int nranks, double delta, int* K);
int pdhg_slab_fixup_nb(pdhg_ctx* ctx, const void* D_left, const void* S1_right, const void* all_long,
                       const void* all_GS, int rank, int nranks);
int pdhg_slab_backward(pdhg_ctx* ctx, double tau, double* sums);           /* backward + inverse + update */
int pdhg_slab_primal_finalize(pdhg_ctx* ctx, const double* sums);
int pdhg_slab_dual(pdhg_ctx* ctx, double sigma, int rho_alp_iters, int sub, double* sums, int parts);
int pdhg_slab_dual_finalize(pdhg_ctx* ctx, double eps, int sub, const double* sums);
int pdhg_slab_outer(pdhg_ctx* ctx, int rho_alp_iters, double* sums);
int pdhg_slab_outer_finalize(pdhg_ctx* ctx, double eps, int rho_alp_iters, const double* sums);
int pdhg_slab_plane_out(pdhg_ctx* ctx, int which, void* dst); /* 0 rho row 0, 1 phi_bar row T, 2 [D, S1],
                                                                 3 [D, S1] of the long-range modes,
                                                                 4 phi row T (the next slab's report halo) */
int pdhg_slab_plane_in(pdhg_ctx* ctx, int which, const void* src); /* 0 rho halo, 1 phi_bar row 0 */
int pdhg_slab_status(pdhg_ctx* ctx, pdhg_stats* st);
/* Partitioned carry exchange (pdhg_amd.slab default): the column blocks are split into nparts parts so the
 * neighbour planes of part q travel while part q+1 sweeps forward and part q-1 sweeps backward:
 *   per part: forward_part -> carry_out_part(DS) -> [D -> next slab, S1 -> previous slab, modes part_modes]
 *   plane_out(3) -> [allgather long-range modes]
 *   per part: [wait for its planes] -> fixup_nb_part -> backward_part;   then update(tau, sums).
 * forward_part(q, n) over all q equals slab_forward; backward_part over all q + update equals slab_backward. */
int pdhg_slab_part_modes(pdhg_ctx* ctx, int part, int nparts, unsigned long long* m0, unsigned long long* m1);
int pdhg_slab_forward_part(pdhg_ctx* ctx, double tau, int part, int nparts);
int pdhg_slab_carry_out_part(pdhg_ctx* ctx, void* dst, int part, int nparts);   /* [D, S1] planes, modes of part */
int pdhg_slab_fixup_nb_part(pdhg_ctx* ctx, const void* D_left, const void* S1_right, const void* all_long,
                            const void* all_GS, int rank, int nranks, int part, int nparts);
int pdhg_slab_backward_part(pdhg_ctx* ctx, double tau, int part, int nparts);
int pdhg_slab_update(pdhg_ctx* ctx, double tau, double* sums);            /* inverse y + update + sums */
/* The solution report and the trajectories slab by slab (what pdhg_multi_report_state / _report_rows / _trajectories
 * chain; pdhg_report_state, pdhg_report_rows and pdhg_trajectories themselves stay refused on a t-slab).  Every
 * pointer below is a device pointer used on the context's stream; nothing is staged through the host and nothing
 * synchronises (the first report call allocates the partial table and, on a slab with j0 > 0, one plane in phi's type
 * for the phi halo, both counted by pdhg_device_bytes; the first trajectory call uploads the grid coordinates).  All
 * three leave the state, phi_bar and the loop control untouched.
 * Report: residual row j of a slab owning global rows [j0, j0 + T) reads two planes the slab does not hold fresh:
 *   rho row T   = the next slab's rho row 0.  The slab's halo is stale after the last dual sweep: before the pass the
 *                 caller delivers it again, next slab plane_out(0) -> [move] -> plane_in(0) (not on the last slab, whose
 *                 row T is the window's zero row and which alone adds c_on_rho / dt);
 *   phi row 0   = the previous slab's phi row T when j0 > 0 (the iteration maintains phi_bar row 0 only):
 *                 previous slab plane_out(4) -> [move] -> phi_prev_rowT here (null on the first slab); it is copied
 *                 into the report's own plane, never into the slab's phi.
 * pdhg_slab_report: one pass over the slab's rows folded to one row of 16 doubles in `sums`:
 *   [0] sum |r| [1] sum r^2 [2] sum rho |r| [3] sum rho [4] sum |c| [5] sum c^2 [6] non-finite points [7] points
 *   rho == 0; [8] max |r| [9] max max(r, 0) [10] max |r| where rho > 0 [11] max |c| [12] max rho [13] max -rho
 *   [14] max phi [15] max -phi.
 * The window's report folds the slabs' rows IN SLAB ORDER (columns 0-7 added, 8-15 maximised; an all-reduce has no
 * fixed order) and is then pdhg_report's arithmetic with n_points = T_total nx ny.
 * pdhg_slab_report_rows: rows [row0_local, row0_local + nrows) of the slab's two fields into device planes
 * [nrows][nx][ny] of doubles (a null plane is skipped).  The values are bit for bit the single context's rows on the
 * same state (same device functions, same operand order).
 * pdhg_slab_trajectories: the slab's T steps of a rollout over T_total rows.  Control time runs against PDE time, so
 * the LAST slab marches first (step0 = 0) and a slab's step0 = the rows of the slabs after it; its local step ind
 * reads its row T-1-ind and is global step step0 + ind: the Philox step word, the row of d_noise
 * ([T_total][n][2], or null: device generator when epsl > 0) and the row of the records d_rec_x [T_total+1][n][2]
 * (rows step0+1 .. step0+T written; row 0 too when step0 = 0) and d_rec_a [T_total][n][n_ctrl] (rows step0 ..
 * step0+T-1), each optional.  n = the samples of this launch (opts->n_sample is not read), opts->sample_offset = the
 * global index of its sample 0; d_x_in / d_x_out [n][2] (they may be the same buffer).  d_x_out of one slab is d_x_in
 * of the slab before it.  PDHG_ERR_ARG: null opts / positions, n < 1, step0 outside [0, rows after this slab], a bad
 * method or period. */
int pdhg_slab_report(pdhg_ctx* ctx, const void* phi_prev_rowT, double* sums);
int pdhg_slab_report_rows(pdhg_ctx* ctx, const void* phi_prev_rowT, int row0_local, int nrows, double* d_hj,
                          double* d_cont);
int pdhg_slab_trajectories(pdhg_ctx* ctx, const pdhg_traj_opts* opts, int step0, long long n, const double* d_x_in,
                           const double* d_noise, double* d_x_out, double* d_rec_x, double* d_rec_a);

/* ---------------- x-slab decomposition (multi-GPU for T = 1 marching windows) -----------
 * New capability (the reference has no distributed path).  The reference's default marches windows of
 * T = time_step_per_PDHG - 1 = 1 rows (run_example.py:425, utils_pdhg_solver.py:121-206), which a t-slab
 * cannot split; an x-slab splits the GLOBAL grid's nx rows into nranks contiguous slabs of nloc = nx/nranks
 * rows (a multiple of 8), one context per GPU.  `p` describes the global problem (nx, xs global).  The
 * context's spatial arrays are local: nx_local = nloc + 16 rows, row i = global row (x0 - xl0 + i) mod nx,
 * live rows [xl0, xl0 + nloc) (xl0 = 8); pdhg_set_state / get_state / init_state take and return arrays of
 * that shape (ghost and padding rows filled from the global arrays by periodic wrap).  One outer iteration
 * of utils_pdhg_solver.py:51-88:
 *   halo_out(0, buf) -> [allgather] -> halo_in(0, left's, right's) -> residual -> wire(0, send)
 *   -> [all-to-all] -> wire(1, recv) -> precond -> wire(2, send) -> [all-to-all] -> wire(3, recv)
 *   -> update(tau, sums) -> halo_out(1, buf) -> [allgather] || [allreduce sums] -> slab_primal_finalize(sums)
 *   -> halo_in(1, left's, right's) -> slab_dual(sigma, k, s, sums, 3) -> [allreduce] -> slab_dual_finalize ...
 *   -> slab_outer -> [allreduce when k > 1] -> slab_outer_finalize   (the t-slab phase functions).
 * halo_out: [2][nq][T][ny] (nq = 1 + live controls for which 0 = rho/alp of the current set, 1 for
 * which 1 = phi_bar rows 1..T); side 0 = the first live row (to the left neighbour), side 1 = the last.
 * halo_in takes the left neighbour's and the right neighbour's halo_out buffers (periodic ring).
 * wire: [nranks][T][nb/nranks][nloc][B] elements (pdhg_xslab_sizes), chunk q = for / from rank q; stage 0
 * packs the y-transformed rows, 1 unpacks the received rows into whole x lines, 2 packs the
 * preconditioned lines, 3 unpacks them back into rows.  Halo and wire elements are in the context's precision
 * (float for p->precision 4, double for 8 = the reference's arithmetic).  ndim 2, bc (0,0) or egno 3's (1,0) (the
 * outer slabs' outer ghost rows replicate their edge row), (ny/B) % nranks == 0; fp32: a power-of-two ny in
 * [256, 8192]; fp64: ny = 2048 or 4096 (the fp64 4-row row kernels) and nx != 8192. */
int pdhg_create_xslab(const pdhg_problem* p, int rank, int nranks, int device, pdhg_ctx** out);
int pdhg_xslab_layout(pdhg_ctx* ctx, int* x0, int* nloc, int* nx_local, int* xl0);
int pdhg_xslab_sizes(pdhg_ctx* ctx, unsigned long long* wire, unsigned long long* halo_state,
                     unsigned long long* halo_phibar);                     /* element counts */
int pdhg_xslab_halo_out(pdhg_ctx* ctx, int which, void* dst);
int pdhg_xslab_halo_in(pdhg_ctx* ctx, int which, const void* from_left, const void* from_right);
int pdhg_xslab_residual(pdhg_ctx* ctx);                                    /* residual + y-DHT, local rows */
int pdhg_xslab_wire(pdhg_ctx* ctx, int stage, void* buf);
int pdhg_xslab_precond(pdhg_ctx* ctx);                                     /* x-DHT, Thomas, inverse x-DHT */
int pdhg_xslab_update(pdhg_ctx* ctx, double tau, double* sums);            /* inverse y-DHT + update + sums */

/* ---------------- multi-device context (create over a device list) ----------------
 * Replaces the single-device pdhg_create of the drop-in for callers that bring no communicator: one host
 * thread drives ndev t-slab contexts (pdhg_create_slab, one per listed device; a device may repeat) through
 * the choreography above, with planes moved device to device by hipMemcpyPeerAsync (xGMI) and the stop-test
 * sums folded in slab order on the first device, so a C / Go / Java caller gets the multi-GPU window without
 * re-implementing pdhg_amd/slab.py or linking RCCL.  The window's rows [0, p->T) are split near-equally
 * (the first T % ndev slabs get one more row).  State arrays are the WHOLE window in the reference layouts
 * (as pdhg_set_state / pdhg_get_state).  Same support as the t-slab (fp32 or fp64, ndim 2, bc (0,0) or egno 3's
 * (1,0)).  The stop-test sums are gathered on the first device, folded in slab order and copied back; with
 * PDHG_MULTI_PEER_FOLD=1 (and peer access between every device pair) each device folds them from its peers'
 * buffers instead (opt-in until validated on separate devices).
 * Keys of pdhg_multi_info: "ndev", "long_modes", "rows:<i>" (rows of slab i), "peer_fold". */
typedef struct pdhg_multi pdhg_multi;
int pdhg_create_multi(const pdhg_problem* p, const int* devices, int ndev, pdhg_multi** out);
int pdhg_multi_destroy(pdhg_multi* m);
int pdhg_multi_set_state(pdhg_multi* m, const double* phi, const double* rho, const double* alp);
int pdhg_multi_get_state(pdhg_multi* m, double* phi, double* rho, double* alp);
int pdhg_multi_init_state(pdhg_multi* m, const double* g);        /* pdhg_init_state on every slab */
int pdhg_multi_iterate(pdhg_multi* m, int n_iters, double tau, double sigma, double eps, int rho_alp_iters,
                       pdhg_stats* out);                          /* utils_pdhg_solver.py:51-88 on all slabs */
int pdhg_multi_set_stop_rules(pdhg_multi* m, int stop_on_converge, int stop_on_nan);
int pdhg_multi_synchronize(pdhg_multi* m);
int pdhg_multi_info(pdhg_multi* m, const char* key, int* value);   /* + "parts", "device:<i>" */
/* The solution report and the trajectories of the whole window (contracts, layouts and values of pdhg_report_state /
 * pdhg_report_rows / pdhg_trajectories with T = p->T; host arrays).  All three drain the slab streams, leave the
 * states, phi_bar, the loop control and the long-range classification untouched and return with every stream idle.
 * report_state: rho row 0 of slab r+1 is delivered to slab r's halo and phi row T of slab r-1 to slab r's report,
 * device to device, then every slab runs pdhg_slab_report on its own device and stream; the ndev rows are folded on
 * the host in slab order (a repeated call returns the same bits).  Counts and extrema equal the single context's on the
 * same state; the six sum-derived fields differ from it by the re-association of fp64 sums only.
 * report_rows: GLOBAL rows [row0, row0 + nrows) (a range may span slabs), staged per slab in row chunks of the single
 * context's budget; bit for bit the single context's rows.
 * trajectories: per sample chunk (the single context's budget rule with T = p->T) the positions enter the last slab at
 * step 0 and are handed slab to slab device to device; each slab uploads its steps' noise rows and returns its steps'
 * record rows.  Bit for bit the single context's paths on the same controls.
 * Run so far with every slab on one device only (devices = {0, 0, ...}), like the rest of this context. */
int pdhg_multi_report_state(pdhg_multi* m, pdhg_report* out);
int pdhg_multi_report_rows(pdhg_multi* m, int row0, int nrows, double* hj, double* cont);
int pdhg_multi_trajectories(pdhg_multi* m, const pdhg_traj_opts* opts, const double* x_init, const double* noise,
                            double* x_final, double* traj_x, double* traj_alp);
/* Per-phase timing of the choreography (events on slab 0's main stream, cross-slab waits included) while
 * enabled; phases "residual", "forward", "backward", "allreduce", "dual", "outer", "step". */
int pdhg_multi_profile(pdhg_multi* m, int enable);
int pdhg_multi_phase_ms(pdhg_multi* m, const char* phase, double* total_ms, int* steps);

/* Identity of the built library: a hash of the sources it was compiled from (build() compares it with
 * the tree and rebuilds on a mismatch, so a stale libpdhg.so is never what the tests load). */
const char* pdhg_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_MI355X_H */
