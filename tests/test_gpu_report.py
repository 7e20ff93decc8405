"""Solution report on the device (pdhg_report_state / pdhg_report_rows) against the host definitions
(pdhg_amd.report, themselves pinned to the oracle in test_report_host.py).

Field bound.  |dev - ref| <= 64 u S pointwise: u the unit roundoff of the context's arithmetic (2^-53 fp64, 2^-24 fp32
and mixed), S the sum of the absolute values of the terms of r (of c) at the point -- the forward error bound of a sum
of a dozen rounded products (each term carries a few roundings: its difference, the reciprocal of the spacing, the
coefficient table, the product) with a factor of 4 to spare.  The reference is evaluated in float64 on what get_state
returns, so the storage rounding is on both sides.  For a mixed context the phi differences and the time / eps terms
are formed in double and rounded once: that part counts as one term, |Dt phi - eps Lap phi|."""
import ctypes

import numpy as np
import pytest

import pdhg_oracle as O
from _report_support import setup as _setup, state as _state

pytestmark = pytest.mark.gpu

U_OF = {"fp64": 2.0 ** -53, "fp32": 2.0 ** -24, "mixed": 2.0 ** -24}
DT, C_RHO = 0.05, 70.0


def _ctx(egno, ndim, nx, ny, T, prec, epsl, k=1):
    from pdhg_amd.context import PDHGContext
    x_arr = O.make_grid(ndim, nx, ny, egno)
    xs = x_arr[0, :, 0] if ndim == 1 else x_arr[0, :, 0, 0]
    ys = None if ndim == 1 else x_arr[0, 0, :, 1]
    return PDHGContext(egno, ndim, nx, ny, T, 2.0 / nx, 2.0 / ny, DT, xs, ys, epsl=epsl, c_on_rho=C_RHO,
                       precision=prec, rho_alp_iters=k)


def _nb(a, s, axis, bc):
    """The neighbour at index + s along axis: periodic wrap or the Neumann stencil's repeated edge value."""
    if bc == 0:
        return np.roll(a, -s, axis=axis)
    idx = np.clip(np.arange(a.shape[axis]) + s, 0, a.shape[axis] - 1)
    return np.take(a, idx, axis=axis)


def _term_sums(case, phi, rho, alp, fns, dsp, epsl, x_arr, bc, mixed):
    """(S_r, S_c): the sums of the absolute values of the terms of the two residuals at every point."""
    egno, ndim, nx, ny, T = case
    bcs = (bc,) if ndim == 1 else tuple(bc)
    f = (O.get_f_vals_1d if ndim == 1 else O.get_f_vals_2d)(fns.f_fn, alp, x_arr, None)
    p1, p0 = np.abs(phi[1:]), np.abs(phi[:-1])
    if mixed:
        v = (phi[1:] - phi[:-1]) / DT
        for ax in range(ndim):
            q = phi[1:]
            v = v - epsl * (_nb(q, 1, ax + 1, bcs[ax]) + _nb(q, -1, ax + 1, bcs[ax]) - 2 * q) / dsp[ax] ** 2
        s_r = np.abs(v)
    else:
        s_r = (p1 + p0) / DT
    for ax in range(ndim):
        up, dn = _nb(p1, 1, ax + 1, bcs[ax]), _nb(p1, -1, ax + 1, bcs[ax])
        if not mixed:
            s_r = s_r + epsl * (up + dn + 2 * p1) / dsp[ax] ** 2
            s_r = s_r + (up + p1) / dsp[ax] * np.abs(f[2 * ax]) + (p1 + dn) / dsp[ax] * np.abs(f[2 * ax + 1])
        else:
            q = phi[1:]
            s_r = s_r + np.abs((_nb(q, 1, ax + 1, bcs[ax]) - q) / dsp[ax] * f[2 * ax]) + \
                np.abs((q - _nb(q, -1, ax + 1, bcs[ax])) / dsp[ax] * f[2 * ax + 1])
    s_r = s_r + np.abs(fns.numerical_L_fn(alp, x_arr, None))
    r = np.abs(rho)
    nxt = np.concatenate([r[1:], np.zeros_like(r[0:1])], axis=0)
    s_c = (nxt + r) / DT
    s_c[-1] += C_RHO / DT
    for ax in range(ndim):
        s_c = s_c + epsl * (_nb(r, 1, ax + 1, bcs[ax]) + _nb(r, -1, ax + 1, bcs[ax]) + 2 * r) / dsp[ax] ** 2
        m1, m2 = np.abs((rho + 1e-4) * f[2 * ax]), np.abs((rho + 1e-4) * f[2 * ax + 1])
        s_c = s_c + (m1 + _nb(m1, -1, ax + 1, bcs[ax])) / dsp[ax] + (m2 + _nb(m2, 1, ax + 1, bcs[ax])) / dsp[ax]
    return s_r, s_c


def _reference(case, ctx, epsl):
    """The host report on get_state's arrays: (dict, hj, cont, S_r, S_c, state)."""
    from pdhg_amd.report import report_from_arrays
    x_arr, bc, dsp, fns = _setup(*case)
    phi, rho, alp = ctx.get_state()
    with np.errstate(invalid="ignore"):
        d, hj, cont = report_from_arrays(phi, rho, alp, fns, DT, dsp, C_RHO, epsl, x_arr, None, bc, fields=True)
        s_r, s_c = _term_sums(case, phi, rho, alp, fns, dsp, epsl, x_arr, bc, ctx.precision == "mixed")
    return d, hj, cont, s_r, s_c, (phi, rho, alp)


def _ratio(dev, ref, s, u):
    """max |dev - ref| / (u S) over the finite points; where S = 0 (every term zero) the two must be equal."""
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(dev), ok)
    diff, bound = np.abs(dev - ref)[ok], (u * s)[ok]
    q = np.where(diff == 0, 0.0, diff / np.where(bound > 0, bound, 1.0))
    q = np.where((bound == 0) & (diff != 0), np.inf, q)
    return float(np.max(q)) if ok.any() else 0.0


def _check_stats(d, hj, cont, rho, phi1):
    """report() against NumPy over the device's own field rows: counts and extrema exactly, sums to 1e-12 (beyond
    2.5e4 points to 2 n 2^-53, the worst case of two fp64 summations of n terms of one sign in different orders)."""
    from pdhg_amd.report import report_from_fields
    with np.errstate(invalid="ignore"):
        want = report_from_fields(hj, cont, rho, phi1)
    exact = ("n_points", "n_nonfinite", "n_rho_zero", "hj_max", "hj_pos_max", "hj_active_max", "cont_max", "rho_min",
             "rho_max", "phi_min", "phi_max")
    assert set(d) == set(want)
    for k in want:
        if isinstance(want[k], float) and np.isnan(want[k]):
            assert np.isnan(d[k]), k
        elif k in exact:
            assert d[k] == want[k], (k, d[k], want[k])
        else:   # fp64 accumulation of <= 2.5e4 points in a different order
            rel = 1e-12 if hj.size <= 25000 else 2 * hj.size * 2.0 ** -53
            assert d[k] == pytest.approx(want[k], rel=rel, abs=0), (k, d[k], want[k])


def _check(case, ctx, epsl, parity_log, name, tile):
    """Fields to the bound, statistics to NumPy; returns the device fields."""
    T = case[4]
    assert ctx.path_info("report_tile") == tile
    d_ref, hj_ref, cont_ref, s_r, s_c, (phi, rho, alp) = _reference(case, ctx, epsl)
    hj, cont = ctx.residual_rows(0, T)
    u = U_OF[ctx.precision]
    q_r, q_c = _ratio(hj, hj_ref, s_r, u), _ratio(cont, cont_ref, s_c, u)
    print("{}: max |dev - ref| / (u S): hj {:.3g} cont {:.3g}".format(name, q_r, q_c))
    parity_log("test_gpu_report", name, {"hj_ratio": q_r, "cont_ratio": q_c}, {"hj_ratio": 64.0, "cont_ratio": 64.0})
    assert q_r <= 64.0 and q_c <= 64.0, (name, q_r, q_c)
    _check_stats(ctx.report(), hj, cont, rho, phi[1:])
    return hj, cont, s_r, s_c


# egno, ndim, nx, ny, T, report_tile
SHAPES = {
    "generic": ((1, 2, 12, 20, 3), 0),
    "tile": ((1, 2, 16, 512, 3), 1),       # two x tiles x two (fp64, mixed: four) y strips
    "tile_T1": ((2, 2, 16, 512, 1), 1),    # one-row windows
    "egno3": ((3, 2, 16, 256, 2), 1),      # the Neumann x edge falls on tile edges
    "line32": ((1, 1, 32, 1, 4), 0),
    "line1024": ((2, 1, 1024, 1, 3), 0),   # more than one workgroup along x
}
FIELD_CASES = [(s, p, e) for s in SHAPES for e in (0.0, 0.1)
               for p in (("fp32", "fp64", "mixed") if SHAPES[s][0][1] == 2 else ("fp32", "fp64"))]


def _tile_and_generic(case, prec, epsl, parity_log, monkeypatch, name, wgs=None, seed=7, nan_at=None):
    """The tile kernel and the per-point kernel on the same state: each to the bound against the host reference (fields,
    statistics), and the two against each other to the same bound.  wgs: PDHG_REPORT_WGS of the tile context.
    Returns the tile context's (hj, cont) and its report."""
    monkeypatch.delenv("PDHG_REPORT_TILE", raising=False)
    monkeypatch.delenv("PDHG_REPORT_WGS", raising=False)
    if wgs is not None:
        monkeypatch.setenv("PDHG_REPORT_WGS", str(wgs))
    st = _state(*case, seed=seed)
    if nan_at is not None:
        st[0][nan_at] = np.nan
    ctx = _ctx(*case, prec, epsl)
    monkeypatch.setenv("PDHG_REPORT_TILE", "0")
    gen = _ctx(*case, prec, epsl)
    try:
        if wgs is not None:
            assert ctx.path_info("report_wgs") == wgs
        ctx.set_state(*st)
        gen.set_state(*st)
        hj, cont, s_r, s_c = _check(case, ctx, epsl, parity_log, name, 1)
        hj_g, cont_g, _, _ = _check(case, gen, epsl, parity_log, name + "/generic", 0)
        u = U_OF[prec]
        q_r, q_c = _ratio(hj, hj_g, s_r, u), _ratio(cont, cont_g, s_c, u)
        parity_log("test_gpu_report", name + "/tile_vs_generic", {"hj_ratio": q_r, "cont_ratio": q_c},
                   {"hj_ratio": 64.0, "cont_ratio": 64.0})
        assert q_r <= 64.0 and q_c <= 64.0, (name, q_r, q_c)
        T = case[4]
        if T > 2:   # a row range inside the window: the same values
            h2, c2 = ctx.residual_rows(1, T - 1)
            assert np.array_equal(h2, hj[1:], equal_nan=True) and np.array_equal(c2, cont[1:], equal_nan=True)
            assert ctx.residual_rows(2, 1, hj=False)[0] is None
        return hj, cont, ctx.report()
    finally:
        ctx.close()
        gen.close()


@pytest.mark.parametrize("shape, prec, epsl", FIELD_CASES)
def test_fields_and_statistics(native, parity_log, monkeypatch, shape, prec, epsl):
    case, tile = SHAPES[shape]
    name = "{}/{}/eps{}".format(shape, prec, epsl)
    if tile:
        _tile_and_generic(case, prec, epsl, parity_log, monkeypatch, name)
        return
    monkeypatch.delenv("PDHG_REPORT_TILE", raising=False)
    ctx = _ctx(*case, prec, epsl)
    try:
        ctx.set_state(*_state(*case, seed=7))
        hj, cont, s_r, s_c = _check(case, ctx, epsl, parity_log, name, 0)
        if case[4] > 2:
            h2, c2 = ctx.residual_rows(1, 2)
            assert np.array_equal(h2, hj[1:3]) and np.array_equal(c2, cont[1:3])
    finally:
        ctx.close()


def _tiles(case, prec):
    return (case[2] // 8) * (case[3] // (64 * (4 if prec == "fp32" else 2)))


# The march over t.  With the default target of 1024 workgroups the small shapes above give every workgroup one time
# row; PDHG_REPORT_WGS makes a workgroup carry phi row j+1 into row j and rho row j+1 into row j over several steps,
# alternate its two register sets and re-use its LDS rows:
#   "whole": one chunk of the whole window (T = 5: an odd count, the loop's single-step tail; T = 4: an even one);
#   "ragged": two chunks wanted, so T = 5 runs chunks of 3 and 2 rows (the row-range call over 4 rows: 2 and 2).
MARCH_CASES = [(s, T, p, m) for s in ("tile", "egno3") for T in (5, 4) for p in ("fp32", "fp64", "mixed")
               for m in ("whole", "ragged") if not (T == 4 and m == "ragged")]


@pytest.mark.parametrize("shape, T, prec, mode", MARCH_CASES)
def test_tile_marches_over_t(native, parity_log, monkeypatch, shape, T, prec, mode):
    case = SHAPES[shape][0][:4] + (T,)
    wgs = 1 if mode == "whole" else 2 * _tiles(case, prec)
    name = "{}/T{}/{}/march_{}".format(shape, T, prec, mode)
    _tile_and_generic(case, prec, 0.1, parity_log, monkeypatch, name, wgs=wgs)


def test_tile_march_with_nan(native, parity_log, monkeypatch):
    """A NaN met in the middle of a march: the carried rows hand it to the next step's time difference only."""
    case = SHAPES["tile"][0][:4] + (5,)
    hj, cont, d = _tile_and_generic(case, "fp64", 0.1, parity_log, monkeypatch, "tile/T5/fp64/march_nan", wgs=1,
                                    nan_at=(3, 8, 0))
    assert d["n_nonfinite"] == int((~np.isfinite(hj)).sum()) == 6   # HJ row 2: the 5-point stencil; row 3: one point


@pytest.mark.parametrize("prec, nx, ny, T, wgs", [("fp64", 512, 512, 5, None), ("fp32", 512, 512, 17, None),
                                                  ("fp32", 16, 512, 5, 16), ("fp32", 16, 512, 9, 16)])
def test_table_holds_every_row_range(native, monkeypatch, prec, nx, ny, T, wgs):
    """The report's partial table is sized for the largest launch over any row range.  The tile grid's chunk count
    is not monotone in the rows of a launch: with 4 chunks wanted (256 tiles of 512 x 512 in fp64 against the target
    of 1024; 4 tiles against 16 in the small cases), T = 5 runs 3 chunks of 2 rows but a 4-row range 4 chunks of 1, and
    T = 9 3 chunks of 3 but an 8-row range 4 of 2.  fp32 512 x 512 (128 tiles, 8 chunks wanted), T = 17: the whole
    window runs 6 chunks of 3, but its field planes are staged 16 rows at a time and those run 8 chunks of 2.  Every
    range [row0, row0 + nrows) of the small windows is asked for."""
    from pdhg_amd.report import report_from_fields
    monkeypatch.delenv("PDHG_REPORT_TILE", raising=False)
    monkeypatch.delenv("PDHG_REPORT_WGS", raising=False)
    if wgs:
        monkeypatch.setenv("PDHG_REPORT_WGS", str(wgs))
    case = (1, 2, nx, ny, T)
    assert _tiles(case, prec) >= 128 if not wgs else 4 * _tiles(case, prec) == wgs
    ctx = _ctx(*case, prec, 0.0)
    try:
        assert ctx.path_info("report_tile") == 1
        ctx.set_state(*_state(*case, seed=5))
        hj, cont = ctx.residual_rows(0, T)
        assert np.isfinite(hj).all() and np.isfinite(cont).all()
        ranges = [(0, T - 1), (1, T - 1), (T - 1, 1)] if not wgs else \
            [(r0, n) for r0 in range(T) for n in range(1, T - r0 + 1)]
        for r0, n in ranges:
            h, c = ctx.residual_rows(r0, n)
            assert np.array_equal(h, hj[r0:r0 + n]) and np.array_equal(c, cont[r0:r0 + n]), (r0, n)
        phi, rho, _ = ctx.get_state(alp=False)
        _check_stats(ctx.report(), hj, cont, rho, phi[1:])
        assert report_from_fields(hj, cont, rho, phi[1:])["n_points"] == T * nx * ny
    finally:
        ctx.close()


def test_bad_row_ranges(native):
    N = native
    ctx = _ctx(1, 2, 12, 20, 3, "fp32", 0.0)
    try:
        buf = np.zeros((4, 12, 20))
        for row0, nrows in ((0, 4), (3, 1), (-1, 1), (0, 0)):
            rc = ctx._lib.pdhg_report_rows(ctx._h, row0, nrows, N.dptr(buf), None)
            assert rc == N.PDHG_ERR_ARG and ctx._lib.pdhg_last_error(), (row0, nrows)
        assert ctx._lib.pdhg_report_state(ctx._h, None) == N.PDHG_ERR_ARG
        assert ctx._lib.pdhg_report_rows(ctx._h, 0, 3, None, None) == N.PDHG_OK   # null pointers are skipped
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_closed_form_after_init_state(native, prec):
    """init_state(g), egno 1: phi rows = g, rho = c, alp = 0, so r = -eps Lap_h g with g = sin(2 pi x/P) +
    sin(2 pi y/P), an eigenfunction pair of the stencil: r = eps (lx sin(2 pi x/P) + ly sin(2 pi y/P)),
    l = 2 (1 - cos(2 pi d/P)) / d^2; c = 0 (the window's last row: -c/dt + c/dt)."""
    nx, ny, T, epsl, P = 16, 256, 2, 0.1, 2.0
    ctx = _ctx(1, 2, nx, ny, T, prec, epsl)
    try:
        x_arr = O.make_grid(2, nx, ny, 1)
        sx, sy = np.sin(2 * np.pi * x_arr[0, ..., 0] / P), np.sin(2 * np.pi * x_arr[0, ..., 1] / P)
        ctx.init_state(sx + sy)
        d = ctx.report()
        dx, dy = 2.0 / nx, 2.0 / ny
        lx, ly = 2 * (1 - np.cos(2 * np.pi * dx / P)) / dx ** 2, 2 * (1 - np.cos(2 * np.pi * dy / P)) / dy ** 2
        want = np.max(np.abs(epsl * (lx * sx + ly * sy)))
        g = np.abs(sx + sy)
        s = 2 * g / DT + epsl * 4 * np.max(g) * (1 / dx ** 2 + 1 / dy ** 2)   # the terms of r: all of phi's
        tol = 64 * U_OF[prec] * np.max(s)
        assert ctx.path_info("report_tile") == 1
        assert abs(d["hj_max"] - want) <= tol, (d["hj_max"], want, tol)
        assert abs(d["hj_pos_max"] - want) <= tol and abs(d["hj_active_max"] - d["hj_max"]) == 0
        assert d["rho_min"] == d["rho_max"] == d["rho_mean"] == C_RHO and d["n_rho_zero"] == 0
        assert d["n_nonfinite"] == 0 and d["n_points"] == T * nx * ny
        assert d["cont_max"] <= 64 * U_OF[prec] * 2 * C_RHO / DT
        assert d["phi_max"] == pytest.approx(np.max(sx + sy), rel=4 * U_OF[prec])
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", ["generic", "tile"])
def test_nan_in_phi(native, parity_log, shape):
    """One NaN in phi: the points the reference field marks are counted out; the rest is NumPy's over the others."""
    case, tile = SHAPES[shape]
    ctx = _ctx(*case, "fp64", 0.1)
    try:
        phi, rho, alp = _state(*case, seed=11)
        phi[2, 8, 0] = np.nan   # row 2: HJ rows 1 (stencil, incl. the wrapped y neighbour and a tile edge) and 2
        ctx.set_state(phi, rho, alp)
        d_ref, hj_ref, cont_ref, _, _, _ = _reference(case, ctx, 0.1)
        _check(case, ctx, 0.1, parity_log, shape + "/nan", tile)
        d = ctx.report()
        assert d["n_nonfinite"] == d_ref["n_nonfinite"] == int((~np.isfinite(hj_ref)).sum()) == 6
        all_bad = np.full_like(phi, np.nan)
        ctx.set_state(all_bad, rho, alp)
        d = ctx.report()
        assert d["n_nonfinite"] == d["n_points"] and d["n_rho_zero"] == 0
        assert all(np.isnan(v) for k, v in d.items() if not k.startswith("n_"))
    finally:
        ctx.close()


@pytest.mark.parametrize("shape, prec", [("generic", "fp64"), ("tile", "fp64"), ("tile", "fp32"), ("line32", "fp64")])
def test_current_set_after_iterations(native, parity_log, shape, prec):
    """rho_alp_iters = 2: the state alternates between two buffer sets; the report reads the current one."""
    case, tile = SHAPES[shape]
    egno, ndim, nx, ny, T = case
    ctx = _ctx(*case, prec, 0.0, k=2)
    try:
        from pdhg_amd import set_fns
        g = set_fns.set_up_J(egno, ndim, (2.0, 2.0)[:ndim])(O.make_grid(ndim, nx, ny, egno))
        ctx.init_state(g)
        for n in (1, 2):   # an odd and an even count of set flips
            st = ctx.iterate(n, 0.1 / 1.5, 0.1 * 1.5, -1.0, 2)
            assert st["iters_run"] == n and st["status"] == 0
            _check(case, ctx, 0.0, parity_log, "{}/{}/k2/iters{}".format(shape, prec, n), tile)
    finally:
        ctx.close()


def _snapshot(ctx):
    return ctx.get_state() + (ctx.get_phi_bar(),)


def _same(a, b):
    flat = lambda s: [s[0], s[1]] + list(s[2]) + [s[3]]  # noqa: E731
    return all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))


# prec, ny, T, rho_alp_iters, the path key that must be on
SIDE_CASES = [("fp64", 2048, 4, 1, "fused_residual"),   # the fp64 fused residual needs the 4-row kernels of ny = 2048
              ("fp32", 512, 4, 1, "fused_residual"),
              ("fp64", 512, 4, 1, None),                # the shape as given: no fp64 fused residual at ny = 512
              ("fp64", 512, 1, 10, "spec")]


@pytest.mark.parametrize("prec, ny, T, k, key", SIDE_CASES)
def test_no_side_effects(native, monkeypatch, prec, ny, T, k, key):
    """iterate(3), report(), residual_rows, iterate(3) ends in the stats and state of iterate(6), bit for bit: with
    the fused residual engaged (PDHG_SHORT_T=0, PDHG_FUSE_RES=1; its plane and "consumed" flag live across iterations)
    in fp64 and fp32, and on a T = 1, rho_alp_iters = 10 marching context (captured graph + speculative schedule)."""
    monkeypatch.setenv("PDHG_SHORT_T", "0")
    monkeypatch.setenv("PDHG_FUSE_RES", "1")
    case = (1, 2, 16, ny, T)
    from pdhg_amd import set_fns
    g = set_fns.set_up_J(1, 2, (2.0, 2.0))(O.make_grid(2, 16, ny, 1))
    tau, sigma = 0.1 / 1.5, 0.1 * 1.5
    keys = ("status", "inner_last", "err1", "err2", "err_inner", "nan_seen", "first_nan_iter")
    a, b = _ctx(*case, prec, 0.1, k=k), _ctx(*case, prec, 0.1, k=k)
    try:
        assert a.path_info("fused_residual") == (1 if key == "fused_residual" else 0)
        if key:
            assert a.path_info(key) == 1 and b.path_info(key) == 1
        assert a.path_info("report_tile") == 1
        a.init_state(g)
        b.init_state(g)
        sa = a.iterate(3, tau, sigma, -1.0, k)
        r1 = a.report()
        rows1 = a.residual_rows(0, T)
        assert a.report() == r1   # deterministic, and the report does not disturb itself
        sa2 = a.iterate(3, tau, sigma, -1.0, k)
        sb = b.iterate(6, tau, sigma, -1.0, k)
        assert sa["iters_run"] == sa2["iters_run"] == 3 and sb["iters_run"] == 6
        assert {q: sa2[q] for q in keys} == {q: sb[q] for q in keys}
        assert sa["inner_total"] + sa2["inner_total"] == sb["inner_total"]
        assert _same(_snapshot(a), _snapshot(b))
        assert a.report() == b.report() and a.report() != r1
        assert np.isfinite(rows1[0]).all()
    finally:
        a.close()
        b.close()


def test_decomposed_handles_are_refused(native):
    from pdhg_amd.multi import MultiContext
    from pdhg_amd.slab import SlabContext
    from pdhg_amd.xslab import XSlabContext
    N = native
    xs, ys = np.linspace(0, 2, 512, endpoint=False), np.linspace(0, 2, 256, endpoint=False)
    dx, dy = 2.0 / 512, 2.0 / 256
    for make in (lambda: SlabContext(0, 2, 6, 1, 512, 256, dx, dy, DT, xs, ys),
                 lambda: XSlabContext(0, 2, 1, 512, 256, 1, dx, dy, DT, xs, ys)):
        c = make()
        try:
            with pytest.raises(N.PDHGUnsupported):
                c.report()
            with pytest.raises(N.PDHGUnsupported):
                c.residual_rows(0, 1)
        finally:
            c.close()
    m = MultiContext(1, 512, 256, 4, dx, dy, DT, xs, ys, devices=[0, 0])
    try:
        rep = N.pdhg_report()
        buf = np.zeros((1, 512, 256))
        assert m._lib.pdhg_report_state(m._h, ctypes.byref(rep)) == N.PDHG_ERR_UNSUPPORTED
        assert m._lib.pdhg_report_rows(m._h, 0, 1, N.dptr(buf), None) == N.PDHG_ERR_UNSUPPORTED
        with pytest.raises(N.PDHGUnsupported):
            N.check(m._lib.pdhg_report_state(m._h, ctypes.byref(rep)))
    finally:
        m.close()


def test_dropin_report_keyword(native):
    from pdhg_amd import set_fns, update_fns_in_pdhg as U, utils_pdhg_solver as S
    nx, T, dt = 160, 1, 1.0 / 40   # C0: egno 1, 1-D, nx = 160, nt = 41, the reference's one-row windows
    x_arr = O.make_grid(1, nx, 1, 1)
    fns = set_fns.set_up_example_fns(1, 1, 0)
    g = set_fns.set_up_J(1, 1, (2.0,))(x_arr)
    phi0, rho0 = np.repeat(g, T + 1, axis=0), np.full((T, nx), C_RHO)
    alp0 = tuple(np.zeros((T, nx, 1)) for _ in range(2))
    fp, fd = S.make_update_fns(1, 0, rho_alp_iters=10, precision="fp64")
    args = (fp, fd, fns, phi0, rho0, alp0, x_arr, None, 1, dt, (2.0 / nx,), C_RHO)
    kw = dict(stepsz_param=0.1, N_maxiter=40, print_freq=1000, eps=1e-6, verbose=False)
    try:
        s = []
        S.PDHG_solver_oneiter(*args, stats=s, report=True, **kw)
        ctx = U.get_context(U._spec(fns), T, (nx,), dt, (2.0 / nx,), 0.0, x_arr, 0, 1.0, 1.0, 1.0, C_RHO, 10, "fp64")
        assert s[-1]["report"] == ctx.report() and s[-1]["report"]["n_points"] == T * nx
        assert s[-1]["report"]["hj_max"] > 0
        s2 = []
        S.PDHG_solver_oneiter(*args, stats=s2, **kw)
        assert "report" not in s2[-1] and {q: v for q, v in s[-1].items() if q != "report"} == s2[-1]
    finally:
        U.clear_cache()
