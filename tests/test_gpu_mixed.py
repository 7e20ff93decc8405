"""Mixed precision contexts (precision "mixed" / 12: fp32 state, tables and transforms, phi and phi_bar held,
differenced and updated in float64) against the float64 oracle (pytest -m gpu).

Bounds.  The device is compared with the float64 oracle by relative L2 per quantity; the bound is
max(floor, K32 x e_mixed) with K32 = 4 (tests/test_gpu_configs.py) and e_mixed the distance of the CPU emulation of
the mixed arithmetic (tests/_mixed_emul.py) from the same oracle run, computed here at the test's own shape and
iteration count -- never from the device's output.  Floors: phi 1e-9; rho and alp the fp32 floors of
tests/test_gpu_configs.py (rho 2e-4 from the seeded state, 1e-5 from the reference state; alp 1e-3 / 1e-4).
From the reference state after one iteration -- the point at which the shape discriminates (e32(rho) 1.0e-4 against
e_mixed(rho) 4.6e-8, tests/test_mixed_host.py::test_parity_shape_discriminates) -- the device's rho must also be
below e32(rho) / 4: what the mixed path is for (measured 3.4e-8).  The seeded rough state checks parity only: at
dx = 2/4096 it is violently unstable (|tau U| rms 0.14, 3e2, 6e5 over the three iterations), rho' is dominated by
epsl Lap of the noise, and the two emulations sit at the same error at T = 3 (after 3 iterations e32 1.5e-5,
e_mixed 2.5e-5, device 2.1e-5).  At T = 1 the emulation's e_mixed(rho) = 4.3e-7 after 3 iterations is a property of
its FFT's rounding pattern, not of the arithmetic: white noise of half a float32 ulp (3e-8 relative) added to its U
moves it to 2.4e-5, which is what the device gives (2.4e-5, e32 2.7e-5); the fp32 floor covers it.
"""
import numpy as np
import pytest

import pdhg_oracle as O
import _mixed_emul as E
from _problems import device_ctx, make_problem, rel

pytestmark = pytest.mark.gpu

TAU, SIGMA = E.TAU, E.SIGMA
K32 = 4.0
PERIOD = 256 * 2.0 / 4096   # 256 x 256 with dx = dy = 2/4096: sigma epsl 8 / dx^2 = 5e5 at epsl = 0.1


def _floors(seeded):
    f = {"phi": 1e-9, "rho": 2e-4 if seeded else 1e-5}
    f.update({"alp{}".format(a): (1e-3 if seeded else 1e-4) for a in range(4)})
    return f


def _measure(P, state, ref):
    m = {"phi": rel(state[0], ref[0]), "rho": rel(state[1], ref[1])}
    for a, (x, y) in enumerate(zip(E.live(P, state[2]), E.live(P, ref[2]))):
        m["alp{}".format(a)] = rel(x, y)
    return m


def _check(parity_log, test, case, P, seeded, dev_state, iters, need_gain=False, emul=None):
    """dev_state against the float64 oracle after `iters` iterations (emul: E.errors' result for that count, where one
    emulated run serves several checks); returns the measured errors."""
    ref, e_mixed, e32 = emul or E.errors(P, iters)
    floors = _floors(seeded)
    m = _measure(P, dev_state, ref)
    bounds = {q: max(floors[q], K32 * e_mixed[q]) for q in m}
    gain = e32["rho"] >= 10 * e_mixed["rho"]
    if need_gain:
        bounds["rho"] = min(bounds["rho"], e32["rho"] / 4)
    print("{} {} iters {}: measured {} bounds {} e_mixed {} e32 {}".format(
        test, case, iters, *({k: "{:.2e}".format(v) for k, v in d.items()} for d in (m, bounds, e_mixed, e32))))
    parity_log(test, "{}_it{}".format(case, iters), m, bounds, e_mixed=e_mixed, e32=e32)
    assert gain or not need_gain, (e32["rho"], e_mixed["rho"])
    for q in m:
        assert m[q] < bounds[q], (q, m[q], bounds[q], e_mixed[q], e32[q])
    return m


def test_round_trip(native):
    """phi and phi_bar cross the ABI as full doubles (bits below float precision survive set_state -> get_state,
    get_rows, get_phi_bar, set_phi_bar and init_state); rho and alp come back as their float roundings."""
    P = make_problem(2, 2, 20, 18, 3, 0.1)
    rng = np.random.default_rng(11)
    phi = P["phi"] * (1.0 + 2.0 ** -40 * rng.integers(1, 1 << 12, P["phi"].shape))
    assert not np.array_equal(phi, phi.astype(np.float32).astype(np.float64))
    ctx = device_ctx(P, "mixed")
    try:
        assert ctx.path_info("mixed") == 1
        ctx.set_state(phi, P["rho"], P["alp"])
        phi_d, rho_d, alp_d = ctx.get_state()
        assert np.array_equal(phi_d, phi)
        assert np.array_equal(ctx.get_phi_bar(), phi)
        assert np.array_equal(rho_d, P["rho"].astype(np.float32).astype(np.float64))
        for a_d, a in zip(alp_d, P["alp"]):
            assert np.array_equal(a_d, a.astype(np.float32).astype(np.float64))
        ph, pb, rh, al = ctx.get_rows(1, 2, phi=True, phi_bar=True, rho=True, alp=True)
        assert np.array_equal(ph, phi[1:3]) and np.array_equal(pb, phi[1:3])
        assert np.array_equal(rh, rho_d[1:3]) and all(np.array_equal(x, y[1:3]) for x, y in zip(al, alp_d))
        pbar = phi[::-1].copy()
        ctx.set_phi_bar(pbar)
        assert np.array_equal(ctx.get_phi_bar(), pbar) and np.array_equal(ctx.get_state()[0], phi)
        g = phi[2]
        ctx.init_state(g)
        phi_i, rho_i, _ = ctx.get_state()
        assert all(np.array_equal(row, g) for row in phi_i) and np.array_equal(ctx.get_phi_bar(), phi_i)
        assert np.array_equal(rho_i, np.full_like(rho_i, 70.0))
        # a dead control component is refused as in fp32 contexts
        bad = [a.copy() for a in P["alp"]]
        bad[0][..., 1] = 1.0
        from pdhg_amd._native import PDHGUnsupported
        with pytest.raises(PDHGUnsupported):
            ctx.set_state(phi, P["rho"], bad)
    finally:
        ctx.close()


def _run_three(P, ctx):
    """one primal + one dual, then two further iterations through pdhg_iterate; the states after 1 and 3 iterations"""
    ctx.set_state(P["phi"], P["rho"], P["alp"])
    ctx.update_primal(TAU)
    used = ctx.update_dual(SIGMA, -1.0, 1)
    assert used == 1
    s1 = ctx.get_state()
    st = ctx.iterate(2, TAU, SIGMA, -1.0, 1)
    assert st["iters_run"] == 2 and st["status"] == 0, st
    return s1, ctx.get_state()


# T = 3 and T = 1 run the dual's ONE form (256 x rows x 1 y chunk: up to 8 time chunks, so one row per workgroup up to
# T = 8); T = 9 is the smallest window whose workgroups march over 2 rows (the marching form, ONE = 0)
@pytest.mark.parametrize("T,seeded", [(3, True), (3, False), (1, True), (1, False), (9, False)],
                         ids=["T3-seeded", "T3-ref", "T1-seeded", "T1-ref", "T9_march-ref"])
def test_parity_fast_kernels(native, parity_log, T, seeded):
    """egno 2, 256 x 256, epsl 0.1, dx = 2/4096: the fast-row update and the row-per-thread dual (its ONE form, and at
    T = 9 its marching form) in their mixed forms, after 1 and after 3 iterations."""
    P = make_problem(2, 2, 256, 256, T, 0.1, seeded=seeded, period=PERIOD)
    ctx = device_ctx(P, "mixed")
    try:
        info = {k: ctx.path_info(k) for k in ("mixed", "fast_rows", "fast_dual", "fused_residual", "dual_one", "dual64")}
        assert info == {"mixed": 1, "fast_rows": 1, "fast_dual": 0, "fused_residual": 0, "dual_one": int(T <= 8),
                        "dual64": 0}, info
        s1, s3 = _run_three(P, ctx)
    finally:
        ctx.close()
    case = "e2_256x256_T{}_{}".format(T, "seeded" if seeded else "ref")
    # the reference state after one iteration is the discriminating case: the gain over fp32 is required there
    emul = E.errors(P, (1, 3))
    _check(parity_log, "test_gpu_mixed/fast", case, P, seeded, s1, 1, need_gain=not seeded, emul=emul[1])
    _check(parity_log, "test_gpu_mixed/fast", case, P, seeded, s3, 3, emul=emul[3])


@pytest.mark.parametrize("egno", [1, 3])
@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "ref"])
def test_parity_generic_kernels(native, parity_log, egno, seeded):
    """20 x 18 (mixed radix; egno 3: bc (1, 0), the DCT along x), T = 3, epsl 0.1: the generic update and per-point dual
    in their mixed forms."""
    P = make_problem(egno, 2, 20, 18, 3, 0.1, seeded=seeded)
    ctx = device_ctx(P, "mixed")
    try:
        info = {k: ctx.path_info(k) for k in ("mixed", "fast_rows", "fast_dual", "fused_residual")}
        assert info == {"mixed": 1, "fast_rows": 0, "fast_dual": -1, "fused_residual": 0}, info
        s1, s3 = _run_three(P, ctx)
    finally:
        ctx.close()
    case = "e{}_20x18_T3_{}".format(egno, "seeded" if seeded else "ref")
    emul = E.errors(P, (1, 3))
    _check(parity_log, "test_gpu_mixed/generic", case, P, seeded, s1, 1, emul=emul[1])
    _check(parity_log, "test_gpu_mixed/generic", case, P, seeded, s3, 3, emul=emul[3])


def _dual_ctx(P, monkeypatch, form):
    """form: "head" (the default below 2^25 points), "multi" (every sub-iteration in chunks), "sub" (the
    per-sub-iteration kernels throughout)"""
    monkeypatch.setenv("PDHG_DUAL_MULTI", "1" if form == "multi" else "0")
    monkeypatch.setenv("PDHG_DUAL_HEAD", "1" if form == "head" else "0")
    ctx = device_ctx(P, "mixed", rho_alp_iters=10)
    assert (ctx.path_info("dual_multi"), ctx.path_info("dual_head")) == (int(form == "multi"), int(form == "head"))
    assert ctx.path_info("mixed") == 1 and ctx.path_info("fast_dual") == 0
    return ctx


K10 = dict(egno=2, ndim=2, nx=256, ny=256, T=3, epsl=0.1)


def _k10_problem():
    P = make_problem(K10["egno"], 2, K10["nx"], K10["ny"], K10["T"], K10["epsl"])
    phi_bar = P["phi"] + 0.02 * np.random.default_rng(5).standard_normal(P["phi"].shape)
    return P, phi_bar


@pytest.mark.parametrize("form", ["head", "multi"])
def test_k10_dual_vs_oracle(native, monkeypatch, parity_log, form):
    """rho_alp_iters = 10 at 256 x 256 (the reference default): update_dual through the head form (planned at this
    size) and the chunked form (PDHG_DUAL_MULTI=1) against the oracle's update_dual_alternative -- the same
    sub-iteration count, rho / alp within max(floor, 4 x e_mixed) of the emulated loop."""
    P, phi_bar = _k10_problem()
    floors = _floors(True)
    ctx = _dual_ctx(P, monkeypatch, form)
    try:
        for eps in (1e-3, 1e-6):
            def loop(variant):
                n = []
                _, rho, alp = E.start_state(P, variant)
                pb = phi_bar if variant != "f32" else phi_bar.astype(np.float32)
                x_arr = P["x_arr"].astype(rho.dtype)
                with E.patched(variant):
                    r, a = O.update_dual_alternative(pb, rho, 70.0, alp, SIGMA, P["dt"], P["dsp"], P["epsl"], P["fns"],
                                                     x_arr, None, 2, P["bc"], rho_alp_iters=10, eps=eps, stats=n)
                return r.astype(np.float64), a, n[0]
            rho_o, alp_o, n_o = loop("f64")
            rho_m, alp_m, n_m = loop("mixed")
            assert n_m == n_o   # the emulated loop exits where the oracle's does: the count is well defined
            ctx.set_state(P["phi"], P["rho"], P["alp"])
            ctx.set_phi_bar(phi_bar)
            used = ctx.update_dual(SIGMA, eps, 10)
            _, rho_d, alp_d = ctx.get_state()
            assert used == n_o, (used, n_o)
            m = {"rho": rel(rho_d, rho_o)}
            b = {"rho": max(floors["rho"], K32 * rel(rho_m, rho_o))}
            for i, (d, e, o) in enumerate(zip(E.live(P, alp_d), E.live(P, alp_m), E.live(P, alp_o))):
                m["alp{}".format(i)] = rel(d, o)
                b["alp{}".format(i)] = max(floors["alp0"], K32 * rel(e, o))
            print("k10", form, eps, used, m, b)
            parity_log("test_gpu_mixed/k10", "{}_eps{}".format(form, eps), m, b, inner=used)
            for q in m:
                assert m[q] < b[q], (q, m[q], b[q])
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["multi", "head"])
def test_k10_chunked_matches_per_sub_iteration(native, monkeypatch, form):
    """4 outer iterations with rho_alp_iters = 10: the chunked forms against the per-sub-iteration mixed kernels -- the
    same iteration counts, states to the fp32 rounding tolerance of tests/test_gpu_dual_multi.py (1e-5)."""
    P = make_problem(2, 2, 256, 256, 3, 1e-3)
    out = []
    for f in ("sub", form):
        ctx = _dual_ctx(P, monkeypatch, f)
        try:
            ctx.set_state(P["phi"], P["rho"], P["alp"])
            st = ctx.iterate(4, TAU, SIGMA, 1e-6, 10)
            out.append((ctx.get_state(), st))
        finally:
            ctx.close()
    (s0, st0), (s1, st1) = out
    assert st1["iters_run"] == st0["iters_run"] == 4 and st1["inner_total"] == st0["inner_total"], (st0, st1)
    for a, b in zip((s1[0], s1[1]) + tuple(s1[2]), (s0[0], s0[1]) + tuple(s0[2])):
        assert rel(a, b) < 1e-5


def test_stop_on_convergence(native):
    """A converging small window stops with status 1 within one iteration of the float64 oracle's count."""
    P = make_problem(1, 2, 16, 16, 1, 0.0, seeded=False)
    eps = 1e-3
    primal, dual = O.make_update_fns(2, P["bc"], rho_alp_iters=1)
    phi, rho, alp = P["phi"], P["rho"], P["alp"]
    n_o = None
    for i in range(5000):
        pn = primal(phi, rho, 70.0, alp, TAU, P["dt"], P["dsp"], P["fns"], P["fv"], 0.0, P["x_arr"], None)
        rn, an = dual(2 * pn - phi, rho, 70.0, alp, SIGMA, P["dt"], P["dsp"], 0.0, P["fns"], P["x_arr"], None, 2, -1.0)
        e1, e2 = O.outer_errors(phi, pn, rho, rn, alp, an)
        phi, rho, alp = pn, rn, an
        if e1 < eps and e2 < eps:
            n_o = i + 1
            break
    assert n_o is not None and n_o > 16
    ctx = device_ctx(P, "mixed")
    try:
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        st = ctx.iterate(5000, TAU, SIGMA, eps, 1)
        assert st["status"] == 1 and abs(st["iters_run"] - n_o) <= 1, (st, n_o)
        assert st["err1"] < eps and st["err2"] < eps and not st["nan_seen"]
        assert rel(ctx.get_state()[0], phi) < 1e-5
    finally:
        ctx.close()


def test_stop_on_nan_in_phi(native):
    """A NaN seeded into phi reaches the update's sums: status 2 at the first iteration."""
    P = make_problem(2, 2, 256, 256, 2, 0.0)
    phi = P["phi"].copy()
    phi[1, 7, 9] = np.nan
    ctx = device_ctx(P, "mixed")
    try:
        ctx.set_state(phi, P["rho"], P["alp"])
        st = ctx.iterate(20, TAU, SIGMA, 1e-6, 1)
        assert st["status"] == 2 and st["iters_run"] == 1 and st["nan_seen"] == 1 and st["first_nan_iter"] == 1, st
    finally:
        ctx.close()


@pytest.mark.parametrize("iters", [6, 24])
def test_graph_replay_is_bitwise_eager(native, monkeypatch, iters):
    """pdhg_iterate with PDHG_GRAPH=0 and with the default (windows of 8 iterations replayed from a HIP graph once one
    eager iteration ran: 24 iterations replay two windows, 6 stay eager) leave the same state bit for bit."""
    P = make_problem(2, 2, 256, 256, 2, 0.0)
    out = []
    for graph in ("0", None):
        if graph is None:
            monkeypatch.delenv("PDHG_GRAPH", raising=False)
        else:
            monkeypatch.setenv("PDHG_GRAPH", graph)
        ctx = device_ctx(P, "mixed")
        try:
            ctx.set_stop_rules(False, False)
            ctx.set_state(P["phi"], P["rho"], P["alp"])
            st = ctx.iterate(iters, TAU, SIGMA, 1e-6, 1)
            assert st["iters_run"] == iters
            out.append((ctx.get_state(), ctx.get_phi_bar(), st, ctx.path_info("graph_window")))
        finally:
            ctx.close()
    (s0, pb0, st0, w0), (s1, pb1, st1, w1) = out
    assert w0 == 0 and w1 == (8 if iters >= 16 else 0)
    assert np.array_equal(pb0, pb1, equal_nan=True)
    for a, b in zip((s0[0], s0[1]) + tuple(s0[2]), (s1[0], s1[1]) + tuple(s1[2])):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal([st0["err1"], st0["err2"]], [st1["err1"], st1["err2"]], equal_nan=True)


def test_profiling_and_bytes(native):
    """Profiling classes and the algorithmic bytes of a mixed context: phi / phi_bar at 8 bytes, the rest at 4."""
    P = make_problem(2, 2, 256, 256, 2, 0.1)
    ctx = device_ctx(P, "mixed")
    try:
        N = 2 * 256 * 256
        assert ctx.algorithmic_bytes(1, "update") == 28 * N and ctx.algorithmic_bytes(1, "dual") == 48 * N
        assert ctx.algorithmic_bytes(1, "residual") == 4 * 6 * N and ctx.algorithmic_bytes(1, "precond") == 16 * N
        assert ctx.algorithmic_bytes(1, "iteration") == 4 * N * 25 + 4 * N * 4
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        ctx.profile_enable(True)
        ctx.iterate(2, TAU, SIGMA, -1.0, 1)
        for cls in ("residual", "precond", "update", "dual"):
            ms, n = ctx.profile_query(cls)
            assert n == 2 and ms > 0, (cls, ms, n)
    finally:
        ctx.close()


def test_dropin_functions(native, parity_log):
    """make_update_fns(..., precision="mixed"): one primal and one dual through the reference-shaped functions at
    20 x 18, held to the generic kernels' bound."""
    from pdhg_amd import set_fns, update_fns_in_pdhg as U, utils_pdhg_solver as S
    P = make_problem(1, 2, 20, 18, 3, 0.1)
    fns = set_fns.set_up_example_fns(1, 2, 0)
    fp, fd = S.make_update_fns(2, P["bc"], rho_alp_iters=1, precision="mixed")
    try:
        phi_d = fp(P["phi"], P["rho"], 70.0, P["alp"], TAU, P["dt"], P["dsp"], fns, P["fv"], P["epsl"], P["x_arr"], None)
        rho_d, alp_d = fd(2 * phi_d - P["phi"], P["rho"], 70.0, P["alp"], SIGMA, P["dt"], P["dsp"], P["epsl"], fns,
                          P["x_arr"], None, 2, -1.0)
        assert any(k[13] == "mixed" for k in U._CACHE)   # the functions ran on a mixed context
    finally:
        U.clear_cache()
    _check(parity_log, "test_gpu_mixed/dropin", "e1_20x18_T3_seeded", P, True, (phi_d, rho_d, alp_d), 1)
