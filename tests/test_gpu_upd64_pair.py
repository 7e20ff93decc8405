"""The fp64 update on pairs of x-adjacent 4-row tasks (k_invy_update_pair_2d, kernels_2d_fast.hpp; path key
"upd64_pair") against the same build with PDHG_UPD_PAIR=0 (k_invy_update_fast_2d<N, 4, 512, 4, double>).

The paired form puts the same spectrum values into the same LDS positions and runs the 4-row kernel's transform and
update text on them, so phi' and phi_bar must agree BITWISE: after one primal update from the seeded state (every mode
carries signal) and after three full iterations (the second and third primal read what the dual sweep's residual
made of the first one's phi_bar).  A workgroup sums other tasks than in the 4-row form, so err1 -- sqrt of a ratio of
two sums of n = T nx ny non-negative terms, each sum off by at most n 2^-53 relative whatever the order -- is held to
2 n 2^-53 relative; err2 (the dual's sums, from bitwise equal inputs) to the same bound.  One shape per template is
also held to the float64 oracle at test_gpu_configs.py's fp64 bound (1e-9 relative L2 on phi).

Shapes (nx, ny, T); ny is fixed by the templates, nx and T stay small (column blocks of B = 16), but for one case at
nx = 2048, which has the workload's B = 2 blocks (128-B lines, the two-element unpack; test_gpu_res64.py's shape):
  (8, 4096, 1)    one pair per time row, one time row
  (16, 4096, 3)   two pairs, several time rows
  (40, 4096, 2)   a pair count that is no power of two; again with PDHG_UPD_GRID=3 (fewer workgroups than pairs or
                  tasks, so both forms stride over their work: 10 pairs / 20 tasks on 3 workgroups)
  (8, 2048, 2), (24, 2048, 3)   the ny = 2048 template (8 loads per thread)
  (2048, 2048, 2) column blocks of B = 2, more pairs than one wave of workgroups per CU
  (12, 4096, 2)   nx / 4 odd: upd64_pair == 0 whatever PDHG_UPD_PAIR says, the 4-row kernel runs"""
import numpy as np
import pytest

from _problems import device_ctx, make_problem, oracle_fns, rel

pytestmark = pytest.mark.gpu

TAU, SIGMA = 0.1 / 1.5, 0.1 * 1.5
EGNO, EPSL = 2, 0.1
# (nx, ny, T, PDHG_UPD_GRID or None, held to the oracle)
PAIRED = [(8, 4096, 1, None, True), (16, 4096, 3, None, False), (40, 4096, 2, None, False), (40, 4096, 2, 3, False),
          (8, 2048, 2, None, True), (24, 2048, 3, None, False), (2048, 2048, 2, None, False)]
IDS = ["{}x{}_T{}{}".format(c[0], c[1], c[2], "_grid{}".format(c[3]) if c[3] else "") for c in PAIRED]


def _run(P, monkeypatch, flag, want_pair, grid=None, pf=4):
    """phi' and phi_bar after one update_primal from the seeded state, then the stop statistics of the first iteration
    from it and phi, phi_bar and the statistics after the third, with PDHG_UPD_PAIR = flag."""
    monkeypatch.setenv("PDHG_UPD_PAIR", flag)
    ctx = device_ctx(P, "fp64")
    try:
        got = {k: ctx.path_info(k) for k in ("res64", "upd64_pair")}
        assert got == {"res64": 1, "upd64_pair": want_pair}, (flag, got)
        if want_pair:   # k_invy_update_pair_2d<ny, 512, PF>
            got = {k: ctx.path_info(k) for k in ("upd_kernel", "upd_n", "upd_c")}
            assert got == {"upd_kernel": 7, "upd_n": P["ny"], "upd_c": pf}, got
        if grid is not None:
            assert ctx.path_info("upd_grid") == grid
        ctx.set_stop_rules(converge=False, nan=False)
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        ctx.update_primal(TAU)
        out = {"phi1": ctx.get_state(rho=False, alp=False)[0], "phi_bar1": ctx.get_phi_bar()}
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        st = ctx.iterate(1, TAU, SIGMA, -1.0, 1)   # (the stop statistics are finalized by iterate, not update_primal)
        assert st["iters_run"] == 1 and not st["nan_seen"], st
        out.update(err1_1=st["err1"], err2_1=st["err2"])
        st = ctx.iterate(2, TAU, SIGMA, -1.0, 1)
        assert st["iters_run"] == 2 and not st["nan_seen"], st
        out.update(phi3=ctx.get_state(rho=False, alp=False)[0], phi_bar3=ctx.get_phi_bar(), err1_3=st["err1"],
                   err2_3=st["err2"])
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("case", PAIRED, ids=IDS)
def test_pair_form_bitwise(native, monkeypatch, parity_log, case):
    nx, ny, T, grid, oracle = case
    if grid is not None:
        monkeypatch.setenv("PDHG_UPD_GRID", str(grid))
    P = make_problem(EGNO, 2, nx, ny, T, EPSL, seeded=True)
    new = _run(P, monkeypatch, "1", 1, grid)
    old = _run(P, monkeypatch, "0", 0, grid)
    bound = 2.0 * T * nx * ny * 2.0 ** -53
    m = {}
    for k in ("phi1", "phi_bar1", "phi3", "phi_bar3"):
        assert np.all(np.isfinite(new[k])) and float(np.max(np.abs(new[k]))) > 0.0, k
        m["diff_" + k] = float(np.max(np.abs(new[k] - old[k])))
    for k in ("err1_1", "err2_1", "err1_3", "err2_3"):
        assert np.isfinite(old[k]) and old[k] > 0.0, (k, old[k])
        m["rel_" + k] = abs(new[k] - old[k]) / abs(old[k])
    bounds = {k: (bound if k.startswith("rel_") else 0.0) for k in m}
    if oracle:
        primal, _ = oracle_fns(P)
        phi_o = primal(P["phi"], P["rho"], 70.0, P["alp"], TAU, P["dt"], P["dsp"], P["fns"], P["fv"], EPSL, P["x_arr"],
                       None)
        m["phi_vs_oracle"] = rel(new["phi1"], phi_o)
        bounds["phi_vs_oracle"] = 1e-9
    print("test_pair_form_bitwise", IDS[PAIRED.index(case)], m)
    parity_log("test_pair_form_bitwise", IDS[PAIRED.index(case)], m, bounds)
    for k in ("phi1", "phi_bar1", "phi3", "phi_bar3"):
        assert np.array_equal(new[k], old[k]), (k, m)
    for k in ("err1_1", "err2_1", "err1_3", "err2_3"):
        assert m["rel_" + k] <= bound, (k, m, bound)
    if oracle:
        assert m["phi_vs_oracle"] <= 1e-9, m


@pytest.mark.parametrize("ny", [2048, 4096])
@pytest.mark.parametrize("pf", [2, 3])
def test_pair_prefetch_depths_bitwise(native, monkeypatch, ny, pf):
    """PDHG_UPD_PAIR_PF = 2 / 3 (old-phi row pairs in flight; the default is 4): the depth changes when rows are loaded,
    not what is computed, so phi' and phi_bar are the 4-row kernel's bit for bit, as in test_pair_form_bitwise."""
    monkeypatch.setenv("PDHG_UPD_PAIR_PF", str(pf))
    P = make_problem(EGNO, 2, 16, ny, 3, EPSL, seeded=True)
    new = _run(P, monkeypatch, "1", 1, pf=pf)
    old = _run(P, monkeypatch, "0", 0)
    for k in ("phi1", "phi_bar1", "phi3", "phi_bar3"):
        assert np.all(np.isfinite(new[k])) and float(np.max(np.abs(new[k]))) > 0.0, k
        assert np.array_equal(new[k], old[k]), k


def test_odd_task_count_keeps_the_four_row_kernel(native, monkeypatch, parity_log):
    """nx = 12: three 4-row tasks per time row do not pair up; the plan reports upd64_pair == 0 with PDHG_UPD_PAIR=1 and
    unset, and the update (the 4-row kernel) meets the oracle."""
    P = make_problem(EGNO, 2, 12, 4096, 2, EPSL, seeded=True)
    forced = _run(P, monkeypatch, "1", 0)
    monkeypatch.delenv("PDHG_UPD_PAIR")
    ctx = device_ctx(P, "fp64")
    try:
        assert ctx.path_info("upd64_pair") == 0
    finally:
        ctx.close()
    primal, _ = oracle_fns(P)
    phi_o = primal(P["phi"], P["rho"], 70.0, P["alp"], TAU, P["dt"], P["dsp"], P["fns"], P["fv"], EPSL, P["x_arr"], None)
    e = rel(forced["phi1"], phi_o)
    parity_log("test_odd_task_count", "12x4096_T2", {"phi_vs_oracle": e}, {"phi_vs_oracle": 1e-9})
    assert e <= 1e-9


def test_default_by_window_length(native, monkeypatch):
    """With PDHG_UPD_PAIR unset, windows of >= 100 rows with an even task count take the paired form and shorter ones
    the 4-row kernel (the measured threshold: DESIGN.md section 4); forced on, one-row windows at ny = 2048 still keep
    their 256-thread kernels (upd_t1)."""
    for flag, (nx, ny, T), want in ((None, (8, 2048, 100), {"upd64_pair": 1}), (None, (8, 4096, 3), {"upd64_pair": 0}),
                                    ("1", (8, 2048, 1), {"upd64_pair": 0, "upd_t1": 2})):
        if flag is None:
            monkeypatch.delenv("PDHG_UPD_PAIR", raising=False)
        else:
            monkeypatch.setenv("PDHG_UPD_PAIR", flag)
        ctx = device_ctx(make_problem(EGNO, 2, nx, ny, T, EPSL, seeded=False), "fp64")
        try:
            got = {k: ctx.path_info(k) for k in want}
            assert got == want, (nx, ny, T, got)
        finally:
            ctx.close()
