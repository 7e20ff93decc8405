"""The fp64 x transform at nx = 4096 with the forward rows staged by LDS DMA and b' in registers
(k_precond_xt_f64_2d<4096, 512, false, BPR, TC, DMA>, kernels_xt_f64.hpp) against the same build with
PDHG_XT64_DMA=0 (b' in LDS, rows through registers).

The DMA form does the same arithmetic in the same order -- the first radix-16 pass reads the staged line instead of
the padded one and writes the same positions, everything after it is the same code -- so phi', phi_bar and the
preconditioner's output (the work buffer, pdhg_get_work) must agree BITWISE, on every column block: the seeded state
is non-constant, so every mode carries signal, the block with ky = 0 (lowest modes: the unconverged recurrence for
many rows) and the blocks around ky = ny / 2 (converged by row 1) included.  phi' is also held to the float64 oracle
(H1_precond_2d through update_primal_2d) at test_gpu_xt64.py's 1e-9.

Shapes.  Blocked input: nx = 4096, ny = 16 (the plan takes it: 8 column blocks), T = 1 (the Neumann row alone; the
one-row kernel is switched off so the kernel under test runs it), 2 (one DMA in flight), 3 (an edge step after a
counted step) and 5 (the steady loop).  Task-order input: the plan offers the task-order spectrum at ny = 4096 only
(path_plan.hpp tc_ok: the 4-row residual kernels that write it are the ny = 4096 ones), so nx = 4096, ny = 2048,
T = 3 with PDHG_TC_SPEC=1 and the fused residual runs the blocked input (asserted: tc_spec == 0) and the same window
at ny = 4096 runs the task-order one (tc_spec == 1); both run two iterations, so the second primal reads what the
dual sweep's residual produced."""
import numpy as np
import pytest

from _problems import device_ctx, make_problem, oracle_fns, rel

pytestmark = pytest.mark.gpu

TAU, SIGMA = 0.1 / 1.5, 0.1 * 1.5


def _oracle_phi1(P):
    primal, _ = oracle_fns(P)
    return primal(P["phi"], P["rho"], 70.0, P["alp"], TAU, P["dt"], P["dsp"], P["fns"], P["fv"], 0.0, P["x_arr"], None)


def _pair(P, monkeypatch, expect, iters, first=True):
    """{flag: arrays} for PDHG_XT64_DMA = 1 / 0: phi', phi_bar and the work buffer after one update_primal from the
    seeded state, then (iters > 0: phi' alone from the first call, the host copies of a 4096^2 window being the
    test's cost; first = False: not even that) all three after `iters` iterations and one more update_primal."""
    nwork = P["T"] * P["nx"] * P["ny"]   # [T][nb][nx][B], nb B = ny
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("PDHG_XT64_DMA", flag)
        ctx = device_ctx(P, "fp64")
        try:
            want = dict(expect, f64_xt=1, xt64_dma=int(flag), xt64_bpr=int(flag))
            got = {k: ctx.path_info(k) for k in want}
            assert got == want, (flag, got)
            ctx.set_state(P["phi"], P["rho"], P["alp"])
            if first:
                ctx.update_primal(TAU)
                res = [ctx.get_state(rho=False, alp=False)[0]]
                res += [ctx.get_phi_bar(), ctx.get_work(nwork)] if not iters else [res[0], res[0]]   # (large grids: once)
            else:
                res = [np.ones(1)] * 3
            if iters:
                ctx.set_state(P["phi"], P["rho"], P["alp"])
                ctx.iterate(iters, TAU, SIGMA, -1.0, 1)
                ctx.update_primal(TAU)
                res += [ctx.get_state(rho=False, alp=False)[0], ctx.get_phi_bar(), ctx.get_work(nwork)]
            out[flag] = res
        finally:
            ctx.close()
    return out


NAMES = ("phi1", "phi_bar1", "work1", "phi_n", "phi_bar_n", "work_n")


def _assert_pair(out, phi_o, parity_log, test, case):
    m = {} if phi_o is None else {"primal_vs_oracle": rel(out["1"][0], phi_o), "old_vs_oracle": rel(out["0"][0], phi_o)}
    for name, a, b in zip(NAMES, out["1"], out["0"]):
        m["diff_" + name] = float(np.max(np.abs(a - b)))
        assert np.all(np.isfinite(a)) and float(np.max(np.abs(a))) > 0.0, name
    print(test, case, m)
    parity_log(test, case, m, {k: (1e-9 if "oracle" in k else 0.0) for k in m})
    assert phi_o is None or m["primal_vs_oracle"] <= 1e-9, m
    for name, a, b in zip(NAMES, out["1"], out["0"]):
        assert np.array_equal(a, b), (name, m)


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_blocked_input_bitwise(native, monkeypatch, parity_log, T):
    if T == 1:
        monkeypatch.setenv("PDHG_T1_XT", "0")   # the window kernel on the one-row window
    P = make_problem(2, 2, 4096, 16, T, 0.0, seeded=True)
    out = _pair(P, monkeypatch, {"tc_spec": 0, "t1_xt64": 0} if T == 1 else {"tc_spec": 0}, iters=0)
    _assert_pair(out, _oracle_phi1(P), parity_log, "test_blocked_input_bitwise", "4096x16_T{}".format(T))


@pytest.mark.parametrize("ny,tc", [(2048, 0), (4096, 1)], ids=["ny2048_blocked", "ny4096_task_order"])
def test_fused_residual_two_iterations_bitwise(native, monkeypatch, parity_log, ny, tc):
    monkeypatch.setenv("PDHG_TC_SPEC", "1")
    monkeypatch.setenv("PDHG_FUSE_RES", "1")
    P = make_problem(2, 2, 4096, ny, 3, 0.0, seeded=True)
    # ny = 4096 (this file's addition to the set shapes) leaves the oracle to the ny = 2048 case and the C3 fixtures
    # of test_gpu_configs.py: at 4096^2 the oracle and the extra host copies alone take ten seconds
    out = _pair(P, monkeypatch, {"tc_spec": tc, "fused_residual": 1}, iters=2, first=ny == 2048)
    _assert_pair(out, _oracle_phi1(P) if ny == 2048 else None, parity_log, "test_fused_residual_two_iterations_bitwise",
                 "4096x{}_T3_tc{}".format(ny, tc))


def test_half_real_and_slab_keep_the_lds_form(native, monkeypatch):
    """C4's nx = 8192 (half-real blocks) and the t-slab phases select the form with b' in LDS and rows through
    registers, whatever PDHG_XT64_DMA says."""
    from pdhg_amd.slab import SlabContext
    monkeypatch.setenv("PDHG_XT64_DMA", "1")
    P = make_problem(2, 2, 8192, 16, 3, 0.0, seeded=False)
    ctx = device_ctx(P, "fp64")
    try:
        got = {k: ctx.path_info(k) for k in ("f64_xt", "half_real", "xt64_dma", "xt64_bpr")}
        assert got == {"f64_xt": 1, "half_real": 1, "xt64_dma": 0, "xt64_bpr": 0}, got
    finally:
        ctx.close()
    P = make_problem(2, 2, 4096, 16, 6, 0.0, seeded=False)
    slabs = [SlabContext(r, 2, 6, 2, 4096, 16, P["dx"], P["dy"], P["dt"], P["xs"], P["ys"], epsl=0.0,
                         rho_alp_iters=1, precision="fp64") for r in range(2)]
    try:
        for s in slabs:
            got = {k: s.path_info(k) for k in ("f64_xt", "xt64_dma", "xt64_bpr")}
            assert got == {"f64_xt": 1, "xt64_dma": 0, "xt64_bpr": 0}, got
    finally:
        for s in slabs:
            s.close()
