"""The 2-D H1 preconditioner's solve parameter on every x kernel (pytest -m gpu).

Every 2-D x kernel forms its own dd = (C - lam_x - lam_y) dt^2 and branches on it by hand (the theta -> 0 limit of
the zero mode at C = 0, the converged-pivot switch at kf = floor(20 / min theta) of the fp64 kernel).  The other GPU
tests run 2-D with C = 1 and dt = 1 / max(T, 40) only; here one primal update from the seeded rough state runs over

  PARAMS   (C, dt) in {(0, 1/40), (0, 1/400), (0, 1/2), (100, 1/40), (1, 1/400), (1, 1/2)}
           fp64 kernels also (1e10, 1/2): theta > 20 in every mode, every wave converged from row 0 (kf = 0)
  T        {1, 2, 3, 6, 13}; the batched / LDS-DMA fp32 forms (4 rows per transform, T >= 4) {4, 5, 6, 7, 13}: a whole
           batch, a batch + 1 / 2 / 3 rows, three batches + 1

on the smallest shape that selects each kernel (KERNELS below; ny = 32 selects every power-of-two kernel), every
selection asserted through pdhg_path_info.  Where a one-row window runs the carry-free k_precond_x_t1_2d whatever
multi-row kernel the plan names (nx = 512 .. 4096, not the half-real nx = 8192), T = 1 is left to the t1_* entries
of the same nx, which run it; the multi-row entries there take T in {2, 3, 6, 13}.

Checks, U = (phi' - phi) / tau against the float64 oracle (pinned at these parameters by test_precond2d_host.py):
  fp64   rel L2 of U < 1e-10 (test_gpu_parity.py's bar) and the per-mode measure (_precond_support.per_mode) < 1e-10;
         the nx = 4096 A/B forms and the one-row kernel's two twiddle-seed forms bitwise equal to the default form.
  fp32   the calibrated pattern of test_precond_1d_parameters: e32 = the oracle executed in float32 against the
         float64 oracle on the same case; phi' < max(1e-6, K32 e32_phi), U < max(5e-4, K32 e32_U), per-mode measure
         < K32 x the float32 oracle's per-mode measure, K32 = 4.  For the per-mode measure the device's U is taken
         from the float32-rounded phi the device holds (as the float32 oracle's is), so both carry the same
         ulp(phi) / tau recovery noise in the high modes.
  mixed  the fp32 kernels with phi in float64: the fp32 bounds.
Every measured value, its bound and e32 go to parity_log.

Tiers: default = every kernel at (0, 1/40) and (100, 1/40) with two T each, and the whole PARAMS x T grid on the
benchmarked kernels (the three fp64 nx = 4096 forms, the fp32 LDS-DMA form); the rest is the extended tier.
"""
import collections

import numpy as np
import pytest

from _precond_support import TAU, exact_symbol, oracle_update, oracle_update32, per_mode, residual, residual32
from _problems import device_ctx, make_problem, oracle_fns, rel

import pdhg_oracle as O

pytestmark = pytest.mark.gpu

SIGMA = 0.1 * 1.5
K32 = 4.0
PARAMS = [(0.0, 1 / 40), (0.0, 1 / 400), (0.0, 1 / 2), (100.0, 1 / 40), (1.0, 1 / 400), (1.0, 1 / 2)]
PARAMS64 = PARAMS + [(1e10, 1 / 2)]
DEFAULT_PARAMS = [(0.0, 1 / 40), (100.0, 1 / 40)]
T_ALL, T_MULTI, T_BATCH, T_ONE = (1, 2, 3, 6, 13), (2, 3, 6, 13), (4, 5, 6, 7, 13), (1,)

Kernel = collections.namedtuple("Kernel", "prec egno nx ny Ts default_Ts variants bench")
_B0 = {"PDHG_XT_BATCH": "0"}


def _k(prec, egno, nx, ny, Ts, default_Ts, variants, bench=False):
    """variants: [(environment, expected pdhg_path_info values)], the first the form compared with the oracle's
    bounds first; all of them are, and fp64 ones must agree bitwise."""
    return Kernel(prec, egno, nx, ny, Ts, default_Ts, variants, bench)


_GEN = [({}, {"fast_xt": 0, "f64_xt": 0, "t1_xt64": 0, "half_real": 0})]
_F64_4096 = [({}, {"f64_xt": 1, "xt64_dma": 1, "xt64_bpr": 1}),
             ({"PDHG_XT64_DMA": "0"}, {"f64_xt": 1, "xt64_dma": 0, "xt64_bpr": 0}),
             ({"PDHG_XT64_DMA": "0", "PDHG_XT64_BPR": "1"}, {"f64_xt": 1, "xt64_dma": 0, "xt64_bpr": 1})]
KERNELS = {
    # ---- generic runtime-radix k_precond_xt_2d (the DCT of egno 3's bc (1, 0) included)
    "gen32_64x48": _k("fp32", 2, 64, 48, T_ALL, (1, 6), _GEN),
    "gen32_20x18": _k("fp32", 1, 20, 18, T_ALL, (2, 13), _GEN),            # radix 5 / 3
    "gen32_15x17": _k("fp32", 2, 15, 17, T_ALL, (3, 6), _GEN),             # odd nx, odd ny
    "dct32_16x12": _k("fp32", 3, 16, 12, T_ALL, (1, 13), _GEN),
    "dct32_64x48": _k("fp32", 3, 64, 48, T_ALL, (2, 6), _GEN),
    "gen64_64x48": _k("fp64", 2, 64, 48, T_ALL, (1, 6), _GEN),
    "gen64_20x18": _k("fp64", 1, 20, 18, T_ALL, (2, 13), _GEN),
    "gen64_15x17": _k("fp64", 2, 15, 17, T_ALL, (3, 6), _GEN),
    "gen64_256x32": _k("fp64", 1, 256, 32, T_ALL, (1, 13), _GEN),
    "dct64_16x12": _k("fp64", 3, 16, 12, T_ALL, (1, 13), _GEN),
    "dct64_64x48": _k("fp64", 3, 64, 48, T_ALL, (2, 6), _GEN),
    # ---- fp32 single-role k_precond_xt_fast_2d (fast_xt = 1)
    "fast1_512": _k("fp32", 2, 512, 32, T_MULTI, (2, 13), [(_B0, {"fast_xt": 1})]),
    "fast1_1024": _k("fp32", 1, 1024, 32, T_MULTI, (3, 6), [(_B0, {"fast_xt": 1})]),
    "fast1_2048": _k("fp32", 2, 2048, 32, T_MULTI, (2, 13), [(_B0, {"fast_xt": 1})]),
    "fast1_4096": _k("fp32", 2, 4096, 32, T_MULTI, (3,), [(_B0, {"fast_xt": 1, "xt_n": 4096})]),
    # ---- fp32 warp-specialised k_precond_xt_ws_2d (fast_xt = 2); PDHG_SHORT_T_XT=0 selects it below T = 16
    **{"ws_{}".format(n): _k("fp32", 2, n, 32, T_MULTI, (3,), [({"PDHG_XT_BATCH": "0", "PDHG_XT_WS": "1"},
                                                                         {"fast_xt": 2, "xt_kernel": 2, "xt_n": n})])
       for n in (512, 1024, 2048)},   # the narrower widths, selectable with PDHG_XT_WS=1 only
    "ws_4096": _k("fp32", 2, 4096, 32, T_MULTI, (3, 13),
                  [({"PDHG_XT_BATCH": "0", "PDHG_SHORT_T_XT": "0"}, {"fast_xt": 2, "half_real": 0})]),
    "ws_hr_8192": _k("fp32", 2, 8192, 32, T_ALL, (1, 6), [({"PDHG_XT_DMA_HR": "0"}, {"fast_xt": 2, "half_real": 1})]),
    # ---- fp32 row-batched k_precond_xt_batch_2d (fast_xt = 3)
    "batch_2048": _k("fp32", 2, 2048, 32, T_BATCH, (5, 6), [({}, {"fast_xt": 3})]),
    "batch_4096": _k("fp32", 1, 4096, 32, T_BATCH, (4, 7), [({"PDHG_XT_DMA": "0"}, {"fast_xt": 3})]),
    **{"batch_{}".format(n): _k("fp32", 2, n, 32, T_BATCH, (5,), [({"PDHG_XT_BATCH": "1"}, {"fast_xt": 3, "xt_n": n})])
       for n in (512, 1024)},   # selectable with PDHG_XT_BATCH=1 only
    "batch_4096_pair": _k("fp32", 2, 4096, 32, T_BATCH, (5,), [({"PDHG_XT_DMA": "0", "PDHG_XT_PAIR": "1"},
                                                                   {"fast_xt": 3, "xt_b": 2, "xt_shape": 512})]),
    "batch_4096_rpre2": _k("fp32", 2, 4096, 32, T_BATCH, (5,), [({"PDHG_XT_DMA": "0", "PDHG_XT_RPRE": "2"},
                                                                    {"fast_xt": 3, "xt_b": 4, "xt_c": 2})]),
    # ---- fp32 LDS-DMA k_precond_xt_dma_2d (fast_xt = 4; half-real 5)
    "dma_4096": _k("fp32", 2, 4096, 32, T_BATCH, T_BATCH, [({}, {"fast_xt": 4, "half_real": 0})], bench=True),
    "dma_hr_8192": _k("fp32", 2, 8192, 32, T_BATCH, (5, 13), [({}, {"fast_xt": 5, "half_real": 1})]),
    # ---- one-row windows: k_precond_x_t1_2d (fp64: both twiddle-seed forms; G16 exists at nx = 2048 / 4096)
    "t1_32_512": _k("fp32", 2, 512, 32, T_ONE, T_ONE, [({}, {"fast_xt": 1, "half_real": 0})]),
    "t1_32_1024": _k("fp32", 1, 1024, 32, T_ONE, T_ONE, [({}, {"fast_xt": 1, "half_real": 0})]),
    "t1_32_2048": _k("fp32", 2, 2048, 32, T_ONE, T_ONE, [({}, {"fast_xt": 1, "half_real": 0})]),
    "t1_32_4096": _k("fp32", 2, 4096, 32, T_ONE, T_ONE, [({}, {"fast_xt": 1, "half_real": 0})]),
    "t1_64_512": _k("fp64", 2, 512, 32, T_ONE, T_ONE, [({}, {"t1_xt64": 1, "t1_g16": 0})]),
    "t1_64_1024": _k("fp64", 1, 1024, 32, T_ONE, T_ONE, [({}, {"t1_xt64": 1, "t1_g16": 0})]),
    "t1_64_2048": _k("fp64", 2, 2048, 32, T_ONE, T_ONE, [({}, {"t1_xt64": 1, "t1_g16": 1}),
                                                         ({"PDHG_T1_G16": "0"}, {"t1_xt64": 1, "t1_g16": 0})]),
    "t1_64_4096": _k("fp64", 2, 4096, 32, T_ONE, T_ONE, [({}, {"t1_xt64": 1, "t1_g16": 1}),
                                                         ({"PDHG_T1_G16": "0"}, {"t1_xt64": 1, "t1_g16": 0})]),
    # ---- fp64 k_precond_xt_f64_2d
    "f64_512": _k("fp64", 2, 512, 32, T_MULTI, (2, 13), [({}, {"f64_xt": 1, "t1_xt64": 0})]),
    "f64_1024": _k("fp64", 1, 1024, 32, T_MULTI, (3, 6), [({}, {"f64_xt": 1, "t1_xt64": 0})]),
    "f64_2048_v0": _k("fp64", 2, 2048, 32, T_MULTI, (2, 13), [({}, {"f64_xt": 1})]),
    "f64_2048_v1": _k("fp64", 2, 2048, 32, T_MULTI, (3, 6), [({"PDHG_XT64_VAR": "1"}, {"f64_xt": 1})]),
    "f64_2048_v2": _k("fp64", 2, 2048, 32, T_MULTI, (2, 13), [({"PDHG_XT64_VAR": "2"}, {"f64_xt": 1})]),
    "f64_2048_v3": _k("fp64", 2, 2048, 32, T_MULTI, (3, 6), [({"PDHG_XT64_VAR": "3"}, {"f64_xt": 1})]),
    "f64_hr_8192": _k("fp64", 2, 8192, 32, T_ALL, (1, 6), [({}, {"f64_xt": 1, "half_real": 1, "t1_xt64": 0})]),
    # nx = 4096: the LDS-DMA form (default), the old form, b' in registers alone
    "f64_4096": _k("fp64", 2, 4096, 32, T_MULTI, T_MULTI, _F64_4096, bench=True),
    # ---- mixed precision: the fp32 kernels, phi / phi_bar in float64
    "mixed_4096": _k("mixed", 2, 4096, 32, T_BATCH, (5, 6), [({}, {"mixed": 1, "fast_xt": 4})]),
    "mixed_64x48": _k("mixed", 2, 64, 48, T_ALL, (1, 6), [({}, {"mixed": 1, "fast_xt": 0})]),
}


def _cid(name, C, dt, T):
    return "{}-C{:g}_dt{:g}-T{}".format(name, C, dt, T)


def _primal_cases():
    out = []
    for name, k in KERNELS.items():
        for C, dt in (PARAMS64 if k.prec == "fp64" else PARAMS):
            for T in k.Ts:
                dflt = k.bench or ((C, dt) in DEFAULT_PARAMS and T in k.default_Ts)
                out.append((name, C, dt, T, dflt))
    # shape-major, so that the kernels of one shape share the cached oracle runs
    out.sort(key=lambda c: (KERNELS[c[0]].egno, KERNELS[c[0]].nx, KERNELS[c[0]].ny, c[2], c[3], c[1]))
    return [pytest.param(n, C, dt, T, id=_cid(n, C, dt, T), marks=() if dflt else (pytest.mark.extended,))
            for n, C, dt, T, dflt in out]


_ORACLE = collections.OrderedDict()   # (shape, dt, T) -> problem, residuals and oracle runs per C, the last few


def _case(k, C, dt, T):
    """The problem and its oracle updates, computed once per (shape, dt, T, C) and left unchanged; the continuity
    residual, which does not depend on C, once per (shape, dt, T).  The float32 oracle run (the fp32 calibration) is
    added when a float32 kernel first asks for it."""
    key = (k.egno, k.nx, k.ny, dt, T)
    s = _ORACLE.get(key)
    if s is None:
        P = make_problem(k.egno, 2, k.nx, k.ny, T, 0.0, dt=dt)
        s = _ORACLE[key] = {"P": P, "src": residual(P), "src32": None, "C": {}}
        while len(_ORACLE) > 2:
            _ORACLE.popitem(last=False)
    P = s["P"]
    c = s["C"].get(C)
    if c is None:
        phi_o, U_o = oracle_update(P, C, s["src"])
        c = s["C"][C] = {"P": P, "phi_o": phi_o, "U_o": U_o}
    if k.prec != "fp64" and "e32" not in c:
        if s["src32"] is None:
            s["src32"] = residual32(P)
        phi_32, U_32 = oracle_update32(P, C, s["src32"])
        c["e32"] = {"phi": rel(phi_32, c["phi_o"]), "U": rel(U_32, c["U_o"]), "pm": per_mode(U_32, c["U_o"], P["bc"])}
    return c


def _run(k, P, C, env, expect, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = device_ctx(P, k.prec, C=C)
    try:
        for key, v in expect.items():
            assert ctx.path_info(key) == v, (key, ctx.path_info(key), v)
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        ctx.update_primal(TAU)
        phi_d = ctx.get_state()[0]
    finally:
        ctx.close()
        for key in env:
            monkeypatch.delenv(key)
    return phi_d


@pytest.mark.parametrize("name,C,dt,T", _primal_cases())
def test_primal_parameters(native, monkeypatch, parity_log, name, C, dt, T):
    """One update_primal from the seeded state at (C, dt, T) on the kernel `name` of KERNELS: the bounds of the module
    docstring.

    fp32 (MI355X, 640 cases): no case needed more than K32 = 4 where K32 x e32 is the bound.  Largest device / e32
    ratios: per-mode 2.55 (gen32_15x17, C = 0, dt = 1/2, T = 13); U 4.19 and phi' 4.14, the same on all four nx = 4096
    forms (ws, batched, DMA, mixed) at C = 0, dt = 1/2, T = 13, where the fixed floors hold (U 1.2e-4 < 5e-4, phi'
    6.0e-7 < 1e-6).

    fp64: every kernel but the half-real nx = 8192 one stays inside 1e-10 (worst U 4.1e-11, f64_4096 at C = 0,
    dt = 1/2, T = 2; worst per-mode 7.4e-11, t1_64_4096 at C = 0, dt = 1/2).  f64_hr_8192 MISSES the bound in 11
    extended-tier cases, and the cause is the oracle's symbol, not the kernel: at dt = 1/2 with C = 0 and C = 1, every
    T (U 1.4e-10 - 2.2e-10, per-mode 3.7e-10 - 5.4e-10), and at (0, 1/40), T = 13 in the per-mode measure alone
    (2.0e-10; U 5.7e-11).  The oracle's fv is the FFT of the stencil, whose roundoff is absolute (3e-8 at dx = 2/8192;
    _precond_support.exact_symbol); at dt = 1/2 the diagonal's 2/dt^2 = 8 no longer hides it in the low modes.  The
    float64 oracle itself moves by U 2.2e-10 / per-mode 5.5e-10 on this case (by 4.0e-11 / 5.6e-11 at nx = 4096) when
    fv is replaced by the closed-form symbol; the kernel forms the symbol in closed form.  Such a case logs its
    distance from the oracle run on the closed-form symbol ("U_exact_fv", "pm_exact_fv") before it fails -- measured
    on these 11: U 2.4e-12 - 4.6e-12, per-mode 1.6e-11 - 2.4e-11 -- and the assertion stays on the oracle as the
    reference runs it."""
    k = KERNELS[name]
    c = _case(k, C, dt, T)
    P, phi_o, U_o = c["P"], c["phi_o"], c["U_o"]
    outs = []
    for vi, (env, expect) in enumerate(k.variants):
        phi_d = _run(k, P, C, env, expect, monkeypatch)
        outs.append(phi_d)
        assert np.isfinite(phi_d).all()
        U_d = (phi_d - P["phi"]) / TAU
        case = _cid(name, C, dt, T) + ("" if vi == 0 else "+" + ",".join("{}={}".format(*kv) for kv in env.items()))
        if k.prec == "fp64":
            m = {"U": rel(U_d, U_o), "pm": per_mode(U_d, U_o, P["bc"])}
            b = {"U": 1e-10, "pm": 1e-10}
            extra = {}
            if not all(m[q] < b[q] for q in m) and tuple(P["bc"]) == (0, 0):   # diagnostic: see the docstring
                U_x = oracle_update(dict(P, fv=exact_symbol(P)), C, _ORACLE[(k.egno, k.nx, k.ny, dt, T)]["src"])[1]
                extra = {"U_exact_fv": rel(U_d, U_x), "pm_exact_fv": per_mode(U_d, U_x, P["bc"])}
                print("P2D exact-symbol diagnostic {}: {}".format(case, extra), flush=True)
            parity_log("test_primal_parameters", case, m, b, prec=k.prec, **extra)
            assert np.array_equal(phi_d[0], P["phi"][0])
        else:
            e32 = c["e32"]
            # the phi the device holds: float32-rounded in fp32, the float64 input in mixed precision
            phi_held = P["phi"].astype(np.float32).astype(np.float64) if k.prec == "fp32" else P["phi"]
            m = {"phi": rel(phi_d, phi_o), "U": rel(U_d, U_o), "pm": per_mode((phi_d - phi_held) / TAU, U_o, P["bc"])}
            b = {"phi": max(1e-6, K32 * e32["phi"]), "U": max(5e-4, K32 * e32["U"]), "pm": K32 * e32["pm"]}
            parity_log("test_primal_parameters", case, m, b, prec=k.prec, e32=e32,
                       ratio={q: m[q] / e32[q] for q in m})
            assert np.array_equal(phi_d[0], phi_held[0])
        print("P2D {} {}: {} | bounds {}".format(k.prec, case, " ".join("{}={:.2e}".format(q, v) for q, v in m.items()),
                                                 " ".join("{}={:.2e}".format(q, v) for q, v in b.items())), flush=True)
        assert all(m[q] < b[q] for q in m), (case, m, b)
    if k.prec == "fp64":   # the A/B forms run the same arithmetic per mode in another schedule
        for vi in range(1, len(outs)):
            assert np.array_equal(outs[vi], outs[0]), (name, k.variants[vi][0], rel(outs[vi], outs[0]))


# ---- three iterations with the zero mode undamped: the dual and the primal interact as in the oracle's loop
ITER_T = {T_ALL: 6, T_MULTI: 6, T_BATCH: 6, T_ONE: 1}
ITER_CASES = [pytest.param(n, id=n, marks=() if (k.bench or n in ("gen32_64x48", "gen64_64x48", "dct64_16x12"))
                           else (pytest.mark.extended,)) for n, k in KERNELS.items()]


@pytest.mark.parametrize("name", ITER_CASES)
def test_iterate_3_undamped_zero_mode(native, monkeypatch, parity_log, name):
    """3 iterations of iterate() at (C, dt) = (0, 1/40) on every kernel against the oracle's loop, at the bars of
    test_iterate_10 (fp64: phi 1e-11, rho 1e-10, err1 / err2 1e-8; fp32 and mixed: phi 1e-5, rho 2e-4, err1 1e-2)."""
    k = KERNELS[name]
    C, dt, T, n = 0.0, 1 / 40, ITER_T[k.Ts], 3
    P = make_problem(k.egno, 2, k.nx, k.ny, T, 0.0, dt=dt)
    primal, dual = oracle_fns(P, C=C)
    phi, rho, alp = P["phi"], P["rho"], P["alp"]
    for _ in range(n):
        phi_n = primal(phi, rho, 70.0, alp, TAU, dt, P["dsp"], P["fns"], P["fv"], 0.0, P["x_arr"], None)
        rho_n, alp_n = dual(2 * phi_n - phi, rho, 70.0, alp, SIGMA, dt, P["dsp"], 0.0, P["fns"], P["x_arr"], None, 2,
                            -1.0)
        e1_o, e2_o = O.outer_errors(phi, phi_n, rho, rho_n, alp, alp_n)
        phi, rho, alp = phi_n, rho_n, alp_n
    env, expect = k.variants[0]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = device_ctx(P, k.prec, C=C)
    try:
        for key, v in expect.items():
            assert ctx.path_info(key) == v, (key, ctx.path_info(key), v)
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        st = ctx.iterate(n, TAU, SIGMA, -1.0, 1)
        phi_d, rho_d, _ = ctx.get_state()
    finally:
        ctx.close()
    assert st["iters_run"] == n and st["status"] == 0, st
    m = {"phi": rel(phi_d, phi), "rho": rel(rho_d, rho), "err1": abs(st["err1"] - e1_o) / e1_o}
    if k.prec == "fp64":
        m["err2"] = abs(st["err2"] - e2_o) / e2_o
        b = {"phi": 1e-11, "rho": 1e-10, "err1": 1e-8, "err2": 1e-8}
    else:
        b = {"phi": 1e-5, "rho": 2e-4, "err1": 1e-2}
    parity_log("test_iterate_3_undamped_zero_mode", name, m, b, prec=k.prec, T=T)
    assert all(m[q] < b[q] for q in m), (name, m, b)


# ---- drop-in path
def test_dropin_solve_parameter(native):
    """update_fns_in_pdhg.update_primal_2d(..., C=0.0) and make_update_fns(2, bc, C=0.0, precision="fp64") on 16 x 12
    against the oracle; the same problem with C = 1 and then C = 0 must differ, each matching its own oracle, and the
    context cache must hold one context per C (a C = 0 call must not reuse the C = 1 context)."""
    from pdhg_amd import set_fns, update_fns_in_pdhg as U, utils_pdhg_solver as S
    prev = U.get_precision()
    U.set_precision("fp64")
    U.clear_cache()
    try:
        P = make_problem(2, 2, 16, 12, 3, 0.0)
        fns = set_fns.set_up_example_fns(2, 2, 0)
        args = (P["phi"], P["rho"], 70.0, P["alp"], TAU, P["dt"], P["dsp"])
        out, ora = {}, {}
        for C in (1.0, 0.0):
            out[C] = U.update_primal_2d(*args, fns, P["fv"], 0.0, P["x_arr"], None, P["bc"], C=C)
            ora[C] = oracle_update(P, C)[0]
            assert len(U._CACHE) == (1 if C == 1.0 else 2)
        for C in (1.0, 0.0):
            assert rel((out[C] - P["phi"]) / TAU, (ora[C] - P["phi"]) / TAU) < 1e-10
        # the two results differ as the oracle's do: the oracle's difference is far above the parity bar (so a C = 0
        # call answered from the C = 1 context could not pass the line above), and the device's difference follows
        # it to the two 1e-10 bars (triangle inequality)
        d_dev, d_o = out[0.0] - out[1.0], ora[0.0] - ora[1.0]
        n_u = max(np.linalg.norm(ora[C] - P["phi"]) for C in (0.0, 1.0))
        assert np.linalg.norm(d_o) > 1e4 * 1e-10 * n_u
        assert rel(d_dev, d_o) < 2 * 1e-10 * n_u / np.linalg.norm(d_o)
        assert sorted(key[8] for key in U._CACHE) == [0.0, 1.0]   # the C of each cached context
        fp, _ = S.make_update_fns(2, P["bc"], C=0.0, rho_alp_iters=1, precision="fp64")
        phi_f = fp(*args, fns, P["fv"], 0.0, P["x_arr"], None)
        assert np.array_equal(phi_f, out[0.0]) and len(U._CACHE) == 2   # the C = 0 context again
    finally:
        U.set_precision(prev)
        U.clear_cache()
