"""The policy check on the device (include/pdhg.h pdhg_policy_eval, csrc/kernels_policy.hpp): the closed-loop cost of
the resident controls against phi, against a per-sample restatement of the definition on the trajectory oracle
(tests/_policy_support.py).

The state is set directly (random alp with the dead components zero, a random phi, rho = 1).  The oracle is fed the
arrays get_state returns, so the float rounding of the stored state is on both sides and the comparison is fp64
against fp64, held to the bound the NumPy trajectory module meets against the same oracle (rtol 1e-11, atol 1e-12)."""
import ctypes

import numpy as np
import pytest

import _policy_support as PS
import _traj_support as S

pytestmark = pytest.mark.gpu

PARITY = [(1, e, m, p) for e, m in S.CASES_1D for p in ("fp32", "fp64")] + \
         [(2, e, m, p) for e, m in S.CASES_2D for p in ("fp32", "fp64")] + [(2, 2, "nearest", "mixed")]
ALL = ("running", "terminal", "value", "x_final")


def _check(name, got, ref):
    dev = S.deviation(got, ref)
    print("{}: max |got - ref| / (atol + rtol |ref|) = {:.3e}".format(name, dev))
    assert np.shape(got) == np.shape(ref), (name, np.shape(got), np.shape(ref))
    assert np.allclose(got, ref, rtol=S.RTOL, atol=S.ATOL), (name, dev)


def _yp(P):
    return S.P_SPACE if P["ndim"] == 2 else None


def _eval(ctx, P, x0, method="linear", **kw):
    kw.setdefault("outputs", ALL)
    return ctx.policy_eval(x0, method=method, x_period=S.P_SPACE, y_period=_yp(P), center=P["center"], **kw)


def _state(ctx):
    phi, _, alp = ctx.get_state(rho=False)
    return phi, np.stack(alp)


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _g(P):
    import pdhg_oracle as O
    return O.set_up_J(P["egno"], P["ndim"], (S.P_SPACE, S.P_SPACE))(P["x_arr"])[0]


def _parity(ctx, P, method, epsl, x0):
    phi, alp = _state(ctx)
    noise = S.noise_for(P, len(x0)) if epsl > 0 else None
    for terminal in ("phi0", "none"):
        ref = PS.oracle_policy(P, phi, alp, x0, epsl, method, noise, terminal)
        S.assert_margins(P, alp, ref["traj_x"], method)
        got = _eval(ctx, P, x0, method, noise=noise, terminal=terminal)
        for k in ALL:
            _check("{} {}".format(terminal, k), got[k], ref[k])
        PS.assert_report_matches_fold(got, got["running"], got["terminal"], got["value"])
    return got


# ---- 1 ----
@pytest.mark.parametrize("epsl", [0.0, 0.1])
@pytest.mark.parametrize("ndim,egno,method,precision", PARITY, ids=["{}d_e{}_{}_{}".format(*c) for c in PARITY])
def test_policy_matches_oracle(native, ndim, egno, method, precision, epsl):
    P = S.problem(egno, ndim)
    ctx = S.make_ctx(P, precision, epsl)
    try:
        PS.load_state(ctx, PS.random_phi(P), S.random_alp(P))
        phi, alp = _state(ctx)
        assert np.array_equal(alp, S.rounded(S.random_alp(P), precision))
        assert np.array_equal(phi, S.rounded(PS.random_phi(P), "fp32" if precision == "fp32" else "fp64"))
        got = _parity(ctx, P, method, epsl, P["x0"])
    finally:
        ctx.close()
    assert egno == 2 or np.abs(got["running"]).max() > 1e-3


# ---- 2 ----
@pytest.mark.parametrize("ndim,egno,method,precision", [(1, 2, "nearest", "fp32"), (1, 1, "linear", "fp64"),
                                                        (2, 1, "linear", "fp32"), (2, 3, "linear", "fp64"),
                                                        (2, 2, "nearest", "mixed")])
def test_path_is_the_rollouts(native, ndim, egno, method, precision):
    P = S.problem(egno, ndim)
    x0, noise = P["x0"], S.noise_for(P, len(P["x0"]))
    ctx = S.make_ctx(P, precision, 0.1)
    try:
        PS.load_state(ctx, PS.random_phi(P), S.random_alp(P))
        for kw in (dict(noise=noise), dict(seed=9, sample_offset=3)):
            _, _, xf = ctx.trajectories(x0, method, S.P_SPACE, _yp(P), P["center"], record=(), **kw)
            got = _eval(ctx, P, x0, method, outputs=("x_final",), **kw)
            assert np.array_equal(got["x_final"], xf) and not np.array_equal(xf, x0)
    finally:
        ctx.close()


# ---- 3 ----
@pytest.mark.parametrize("ndim,egno,method,precision", [(1, 1, "linear", "fp64"), (1, 2, "nearest", "fp32"),
                                                        (2, 1, "linear", "fp32"), (2, 3, "linear", "fp64"),
                                                        (2, 3, "linear", "fp32")])
def test_initial_state_has_no_gap(native, ndim, egno, method, precision):
    """alp = 0 and every phi row = g.  egno 1 / 2: f = -a alp = 0, so nothing moves, nothing costs, and both ends read
    the same numbers: running == 0, terminal == value bit for bit, every gap statistic 0.0.
    egno 3 (starts beyond the Neumann x edges): f = (alp, x), so with alp = 0 a sample still drifts in y with velocity
    x and terminal == value cannot hold -- the path is the rollout's by definition.  What holds exactly there:
    nothing costs, x does not move, and since all phi rows are the same plane, the terminal read at x_final is bit for
    bit the value a second call reads when it starts there."""
    P = S.problem(egno, ndim)
    ctx = S.make_ctx(P, precision, 0.0)
    try:
        ctx.init_state(_g(P))
        got = _eval(ctx, P, P["x0"], method)
        again = _eval(ctx, P, got["x_final"], method)
    finally:
        ctx.close()
    assert np.array_equal(got["running"], np.zeros(len(P["x0"])))
    assert got["n_sample"] == len(P["x0"]) and got["n_nonfinite"] == 0 and np.ptp(got["value"]) > 0.1
    assert np.array_equal(got["terminal"], again["value"])
    if egno == 3:
        assert np.array_equal(got["x_final"][:, 0], P["x0"][:, 0]) and np.abs(P["x0"][:, 0]).max() > 1.0
        y = P["x0"][:, 1]
        for _ in range(P["T"]):
            y = y + P["x0"][:, 0] * P["dt"]
        assert np.array_equal(got["x_final"][:, 1], y)
        assert got["gap_abs_max"] == np.abs(got["terminal"] - got["value"]).max() > 0
        return
    assert np.array_equal(got["terminal"], got["value"])
    assert np.array_equal(got["x_final"], P["x0"])
    assert got["gap_abs_max"] == 0.0 and got["gap_lo"] == 0.0 and got["gap_hi"] == 0.0 and got["gap_rms"] == 0.0
    assert got["gap_mean"] == 0.0 and got["gap_abs_mean"] == 0.0 and got["cost_mean"] == got["value_mean"]


# ---- 4 ----
@pytest.mark.parametrize("ndim,egno", [(1, 1), (2, 1)])
def test_reduction_is_the_fold_of_the_samples(native, ndim, egno):
    P = S.problem(egno, ndim)
    n = 785                                    # 3 full workgroups and a ragged one
    x0 = np.random.default_rng(2).uniform(-1.0, 3.0, (n, 2) if ndim == 2 else n)
    ctx = S.make_ctx(P, "fp32", 0.1)
    try:
        PS.load_state(ctx, PS.random_phi(P), S.random_alp(P))
        a = _eval(ctx, P, x0, seed=9)
        b = _eval(ctx, P, x0, seed=9)
        only = _eval(ctx, P, x0, seed=9, outputs=())
    finally:
        ctx.close()
    PS.assert_report_matches_fold(a, a["running"], a["terminal"], a["value"])
    from pdhg_amd._native import POLICY_FIELDS
    assert a["n_sample"] == n and a["gap_abs_max"] > 0
    assert {k: a[k] for k in POLICY_FIELDS} == {k: b[k] for k in POLICY_FIELDS} == only
    _same(a, b)


# ---- 5 ----
@pytest.mark.parametrize("n", [400000, 600000])
def test_sample_chunks_change_nothing(native, n):
    """n = 400000 as the rollout's chunk test; at 600000 samples the staged noise (4 x 2 doubles per sample beside the
    7 of positions and outputs: 120 bytes against the 64 MiB budget) no longer fits one chunk."""
    P = S.problem(1, 2)
    rng = np.random.default_rng(2)
    x0 = rng.uniform(-1.0, 3.0, (n, 2))
    noise = rng.standard_normal((P["T"], n, 2))
    h = n // 2
    ctx = S.make_ctx(P, "fp32", 0.1)
    try:
        PS.load_state(ctx, PS.random_phi(P), S.random_alp(P))
        whole = _eval(ctx, P, x0, noise=noise)
        parts = [_eval(ctx, P, x0[a:b], noise=noise[:, a:b]) for a, b in ((0, h), (h, n))]
        dwhole = _eval(ctx, P, x0, seed=9)
        dparts = [_eval(ctx, P, x0[a:b], seed=9, sample_offset=a) for a, b in ((0, h), (h, n))]
    finally:
        ctx.close()
    for w, (lo, hi) in ((whole, parts), (dwhole, dparts)):
        for k in ALL:
            assert np.array_equal(np.concatenate([lo[k], hi[k]]), w[k]), k
        PS.assert_report_matches_fold(w, w["running"], w["terminal"], w["value"])
    assert not np.array_equal(whole["x_final"], dwhole["x_final"])


# ---- 6 ----
def test_nonfinite_samples_are_counted_and_left_out(native):
    P = S.problem(1, 2)
    ix, iy = 5, 4
    node = np.array([P["xs"][ix], P["ys"][iy]])
    rng = np.random.default_rng(2)
    # starts in the four cells round the node (and their periodic images), then starts anywhere
    x0 = np.concatenate([node + rng.uniform(-0.9, 0.9, (40, 2)) * [P["dx"], P["dy"]],
                         node + [2.0, -2.0] + rng.uniform(-0.9, 0.9, (8, 2)) * [P["dx"], P["dy"]],
                         rng.uniform(-1.0, 3.0, (300, 2))])
    from pdhg_amd.policy import policy_from_arrays
    from pdhg_amd.set_fns import set_up_example_fns
    fns = set_up_example_fns(1, 2, 0)
    ctx = S.make_ctx(P, "fp64", 0.0)
    try:
        alp = S.random_alp(P)
        seen = {}
        for row in (P["T"], 0):
            phi = PS.random_phi(P)
            phi[row, ix, iy] = np.nan
            PS.load_state(ctx, phi, alp)
            for terminal in ("phi0", "none"):
                got = _eval(ctx, P, x0, terminal=terminal)
                host = policy_from_arrays(phi, tuple(alp), fns, x0, P["x_arr"], P["dt"], S.P_SPACE, S.P_SPACE, P["bc"],
                                          P["center"], 0.0, "linear", None, terminal)
                assert np.isfinite(got["x_final"]).all() and np.isfinite(got["running"]).all()
                bad = ~(np.isfinite(host["running"]) & np.isfinite(host["terminal"]) & np.isfinite(host["value"]))
                dev_bad = ~(np.isfinite(got["running"]) & np.isfinite(got["terminal"]) & np.isfinite(got["value"]))
                assert np.array_equal(bad, dev_bad)
                assert got["n_nonfinite"] == int(bad.sum()) == host["n_nonfinite"] and got["n_sample"] == len(x0)
                PS.assert_report_matches_fold(got, got["running"], got["terminal"], got["value"])
                for k in ("running", "terminal", "value"):
                    _check(k, got[k][~bad], host[k][~bad])
                seen[(row, terminal)] = int(bad.sum())
    finally:
        ctx.close()
    print("non-finite samples:", seen)
    assert 48 <= seen[(P["T"], "phi0")] == seen[(P["T"], "none")] < len(x0) // 2     # the value's cell
    assert 0 < seen[(0, "phi0")] < len(x0) // 2 and seen[(0, "none")] == 0           # the terminal's cell


# ---- 7 ----
@pytest.mark.parametrize("ndim,egno,stride,precision", [(2, 1, (4, 3), "fp32"), (2, 3, (4, 3), "fp64"),
                                                        (2, 1, (5, 5), "mixed"), (1, 1, 8, "fp32"),
                                                        (1, 2, 5, "fp64")])
def test_grid_starts(native, ndim, egno, stride, precision):
    P = S.problem(egno, ndim)
    method = "nearest" if egno == 2 else "linear"
    ctx = S.make_ctx(P, precision, 0.1)
    try:
        PS.load_state(ctx, PS.random_phi(P), S.random_alp(P))
        phi, _ = _state(ctx)
        if ndim == 2:
            ii, jj = np.arange(0, P["nx"], stride[0]), np.arange(0, P["ny"], stride[1])
            x0 = np.stack([np.repeat(P["xs"][ii], len(jj)), np.tile(P["ys"][jj], len(ii))], axis=-1)
            nodes = phi[P["T"]][np.ix_(ii, jj)].reshape(-1)
        else:
            ii = np.arange(0, P["nx"], stride)
            x0, nodes = P["xs"][ii], phi[P["T"]][ii]
        kw = dict(method=method, x_period=S.P_SPACE, y_period=_yp(P), center=P["center"], seed=9, outputs=ALL)
        grid = ctx.policy_eval(stride=stride, **kw)
        explicit = ctx.policy_eval(x0, **kw)
    finally:
        ctx.close()
    from pdhg_amd._native import POLICY_FIELDS
    _same(grid, explicit)
    assert {k: grid[k] for k in POLICY_FIELDS} == {k: explicit[k] for k in POLICY_FIELDS}
    assert grid["n_sample"] == len(x0) and np.array_equal(grid["value"], nodes)
    assert not np.array_equal(grid["x_final"], x0)


# ---- 8 ----
def test_windows_chain(native):
    """Rows [2, 4) without a terminal, then rows [0, 2) from where they ended: the 4-row check."""
    P = S.problem(1, 2)
    phi, alp = PS.random_phi(P), S.random_alp(P)
    x0, noise = P["x0"], S.noise_for(P, len(P["x0"]))
    whole, late, early = S.make_ctx(P, "fp32", 0.1), S.make_ctx(P, "fp32", 0.1, T=2), S.make_ctx(P, "fp32", 0.1, T=2)
    try:
        PS.load_state(whole, phi, alp)
        PS.load_state(late, phi[2:5], alp[:, 2:4])
        PS.load_state(early, phi[0:3], alp[:, 0:2])
        w = _eval(whole, P, x0, noise=noise)
        a = _eval(late, P, x0, noise=noise[:2], terminal="none")
        b = _eval(early, P, a["x_final"], noise=noise[2:])
    finally:
        for c in (whole, late, early):
            c.close()
    assert np.array_equal(b["x_final"], w["x_final"]) and np.array_equal(b["terminal"], w["terminal"])
    assert np.array_equal(a["value"], w["value"]) and not a["terminal"].any()
    # the four step costs are added as ((l0 + l1) + l2) + l3 in one call and (l0 + l1) + (l2 + l3) in two
    err = np.abs((a["running"] + b["running"]) - w["running"])
    print("chained running against the 4-row one: max {:.3e}".format(err.max()))
    assert np.all(err <= P["T"] * 2.0 ** -52 * np.abs(w["running"])) and w["running"].max() > 0


# ---- 9 ----
def test_policy_reads_current_alp_set(native):
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, "fp64", 0.1, rho_alp_iters=2)
    try:
        ctx.init_state(_g(P))
        st = ctx.iterate(3, 0.1 / 1.5, 0.1 * 1.5, -1.0, 2)
        assert st["iters_run"] == 3
        assert np.abs(_state(ctx)[1]).max() > 0
        _parity(ctx, P, "linear", 0.1, P["x0"])
    finally:
        ctx.close()


# ---- 10 ----
def _raw(ctx, n_sample=4, method=0, terminal=0, stride=(1, 1), x_period=S.P_SPACE, grid=False, outputs=True,
         opts=True, handle=True):
    from pdhg_amd import _native as N
    po = N.pdhg_policy_opts()
    po.traj.n_sample, po.traj.method, po.traj.x_period, po.traj.y_period = n_sample, method, x_period, S.P_SPACE
    po.terminal, po.stride_x, po.stride_y = terminal, stride[0], stride[1]
    n = max(n_sample, 1) if not grid else 16 * 12
    x0, run = np.zeros((n, 2)), np.empty(n)
    rep = N.pdhg_policy_report()
    rc = ctx._lib.pdhg_policy_eval(ctx._h if handle else None, ctypes.byref(po) if opts else None,
                                   None if grid else N.dptr(x0), None, ctypes.byref(rep) if outputs else None,
                                   N.dptr(run) if outputs else None, None, None, None)
    return rc, ctx._lib.pdhg_last_error().decode()


def test_refusals(native):
    from pdhg_amd.multi import MultiContext
    from pdhg_amd.slab import SlabContext
    from _problems import make_problem
    N = native
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, "fp32", 0.0)
    try:
        PS.load_state(ctx, PS.random_phi(P), S.random_alp(P))
        assert _raw(ctx)[0] == N.PDHG_OK
        assert _raw(ctx, n_sample=0, grid=True, stride=(4, 3))[0] == N.PDHG_OK
        assert _raw(ctx, n_sample=16, grid=True, stride=(4, 3))[0] == N.PDHG_OK
        for kw in (dict(handle=False), dict(opts=False), dict(method=2), dict(method=-1), dict(x_period=0.0),
                   dict(terminal=2), dict(terminal=-1), dict(grid=True, stride=(0, 1)), dict(grid=True, stride=(2, 0)),
                   dict(n_sample=0), dict(n_sample=-3), dict(grid=True, n_sample=15, stride=(4, 3)),
                   dict(grid=True, n_sample=-1, stride=(4, 3)), dict(outputs=False)):
            rc, msg = _raw(ctx, **kw)
            assert rc == N.PDHG_ERR_ARG and msg, (kw, rc, msg)
    finally:
        ctx.close()
    Q = make_problem(1, 2, 512, 256, 6, 0.0)
    slab = SlabContext(0, 2, 6, 1, 512, 256, Q["dx"], Q["dy"], Q["dt"], Q["xs"], Q["ys"])
    try:
        rc, msg = _raw(slab)
        assert rc == N.PDHG_ERR_UNSUPPORTED and "t-slab" in msg
        with pytest.raises(N.PDHGUnsupported):
            slab.policy_eval(np.zeros((4, 2)), x_period=S.P_SPACE, y_period=S.P_SPACE)
    finally:
        slab.close()
    m = MultiContext(1, 512, 256, 4, Q["dx"], Q["dy"], Q["dt"], Q["xs"], Q["ys"], devices=[0, 0])
    try:
        rc, msg = _raw(m)
        assert rc == N.PDHG_ERR_UNSUPPORTED and "multi-device" in msg
        with pytest.raises(N.PDHGUnsupported):
            m.policy_eval(np.zeros((4, 2)), x_period=S.P_SPACE, y_period=S.P_SPACE)
    finally:
        m.close()


# ---- 11 ----
@pytest.mark.parametrize("precision,k", [("fp32", 1), ("fp64", 2), ("mixed", 1)])
def test_state_is_untouched(native, precision, k):
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, precision, 0.1, rho_alp_iters=k)
    try:
        ctx.init_state(_g(P))
        ctx.iterate(3, 0.1 / 1.5, 0.1 * 1.5, -1.0, k)

        def snap():
            phi, rho, alp = ctx.get_state()
            return [phi, rho, np.stack(alp), ctx.get_phi_bar(), np.array(ctx.errors())]
        before = snap()
        _eval(ctx, P, P["x0"], seed=3)
        ctx.policy_eval(stride=(4, 3), x_period=S.P_SPACE, y_period=S.P_SPACE, terminal="none", outputs=())
        after = snap()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        # ... and the iteration goes on as it would have
        twin = S.make_ctx(P, precision, 0.1, rho_alp_iters=k)
        try:
            twin.init_state(_g(P))
            twin.iterate(3, 0.1 / 1.5, 0.1 * 1.5, -1.0, k)
            s1, s2 = ctx.iterate(2, 0.1 / 1.5, 0.1 * 1.5, -1.0, k), twin.iterate(2, 0.1 / 1.5, 0.1 * 1.5, -1.0, k)
            assert (s1["err1"], s1["err2"]) == (s2["err1"], s2["err2"])
            assert np.array_equal(ctx.get_state()[0], twin.get_state()[0])
        finally:
            twin.close()
    finally:
        ctx.close()


# ---- 12 ----
@pytest.mark.parametrize("ndim,n", [(1, 9), (2, 5)])
def test_solved_problem(native, ndim, n):
    """Recorded, not asserted: the gap of a converged window (egno 1, epsl = 0, dt = 0.1, T = 4; fp64, 10 dual
    sub-iterations, stop rule 1e-6), printed for DESIGN.md section 4f.  Measured on one MI355X:
      1-D nx = 32, 9 starts, 12127 iterations: gap mean -9.5e-3, mean |gap| 7.2e-2, rms 1.16e-1, max |gap| 2.80e-1
                                               (phi = g on every row, same alp: max |gap| 9.70e-1)
      2-D 16 x 12, 25 starts, 14335 iterations: gap mean +3.2e-2, mean |gap| 1.57e-1, rms 1.96e-1, max |gap| 5.50e-1
                                               (phi = g on every row, same alp: max |gap| 1.31)
    Asserted are two conditions: the device report is the NumPy definition's on the downloaded state, and the
    converged phi explains the cost of its controls better than the initial phi (every row g) does."""
    from pdhg_amd.policy import format_policy, policy_from_arrays, run_policy_check
    from pdhg_amd.set_fns import set_up_example_fns
    from pdhg_amd.trajectories import trajectory_samples
    from pdhg_amd._native import POLICY_FIELDS
    P = S.problem(1, ndim)
    ctx = S.make_ctx(P, "fp64", 0.0, rho_alp_iters=10)
    try:
        g = _g(P)
        ctx.init_state(g)
        st = ctx.iterate(100000, 0.1 / 1.5, 0.1 * 1.5, 1e-6, 10)
        print("{}-D: stopped with status {} after {} iterations".format(ndim, st["status"], st["iters_run"]))
        assert st["status"] == 1
        rep = run_policy_check(ctx, 1, ndim, S.P_SPACE, S.P_SPACE, 0.0, n)
        print("{}-D converged: {}".format(ndim, format_policy(rep)))
        phi, rho, alp = ctx.get_state()
        x0 = trajectory_samples(1, ndim, n, S.P_SPACE, S.P_SPACE, 0.0)
        host = policy_from_arrays(phi, alp, set_up_example_fns(1, ndim, 0), x0, P["x_arr"], P["dt"], S.P_SPACE,
                                  S.P_SPACE, P["bc"], P["center"], 0.0, "linear")
        for k in POLICY_FIELDS:
            _check(k, rep[k], host[k])
        ctx.set_state(np.repeat(g[None], P["T"] + 1, axis=0), rho, alp)
        start = run_policy_check(ctx, 1, ndim, S.P_SPACE, S.P_SPACE, 0.0, n)
        print("{}-D phi = g on every row: {}".format(ndim, format_policy(start)))
    finally:
        ctx.close()
    assert rep["n_nonfinite"] == 0 and rep["gap_abs_max"] < start["gap_abs_max"]
