"""The solution report on decomposed windows: pdhg_multi_report_state / pdhg_multi_report_rows (MultiContext.report /
.residual_rows), the slab primitives beneath them (pdhg_slab_report / _report_rows, plane_out(4)) and
SlabRunner.report().

Yardstick: the single context on the identical state.  A slab's pass runs the single context's kernels with the same
device functions and operand order; the two planes a slab does not hold (rho row T = the next slab's rho row 0, phi
row 0 = the previous slab's phi row T) are moved, not recomputed.  So the fields are bit for bit the single context's,
counts and extrema are equal, and the six sum-derived statistics differ by the re-association of fp64 sums only:
relative 2 n_points 2^-53, the a-priori bound for two summations of n non-negative terms in different orders (rho >= 0
in the seeded states; |r|, r^2, |c|, c^2 are non-negative).  One fp64 case is also held to the host reference with the
bound and helpers of test_gpu_report.py.

Shapes: 16 x 512 runs the tile kernel (two x tiles, two or more y strips; PDHG_REPORT_TILE=0: the per-point kernel on
the same shape); 20 x 256 (nx % 8 != 0) the per-point kernel, fp64 only -- an fp32 t-slab of this shape is refused by
pdhg_create_slab itself.  Splits: T = 7 over 3 slabs (rows 3 / 2 / 2, a middle slab with both halos), T = 4 over 2
(2 / 2) and T = 4 over 3 (2 / 1 / 1: one-row slabs, where the phi halo and the rho halo meet in one step)."""
import ctypes

import numpy as np
import pytest

import pdhg_oracle as O
from _report_support import state as _state

pytestmark = pytest.mark.gpu

DT, C_RHO = 0.05, 70.0
TAU, SIGMA = 0.1 / 1.5, 0.1 * 1.5
SPLITS = {"T7x3": (7, [0, 0, 0]), "T4x2": (4, [0, 0]), "T4x3": (4, [0, 0, 0])}
PHYS = {"e2": (2, 0.1), "e3": (3, 0.0)}       # egno 2 at epsl = 0.1; egno 3 (bc (1, 0), two controls) at epsl = 0
# shape: (nx, ny, report_tile of the single context, PDHG_REPORT_TILE, precisions)
SHAPES = {"tile": (16, 512, 1, None, ("fp32", "fp64")), "tile_off": (16, 512, 0, "0", ("fp32", "fp64")),
          "point": (20, 256, 0, None, ("fp64",))}
EXACT = ("n_points", "n_nonfinite", "n_rho_zero", "hj_max", "hj_pos_max", "hj_active_max", "cont_max", "rho_min",
         "rho_max", "phi_min", "phi_max")
SUMS = ("hj_l1", "hj_l2", "compl_l1", "cont_l1", "cont_l2", "rho_mean")


def _bounds(T, P):
    from pdhg_amd.slab import slab_bounds
    return slab_bounds(T, P)


def _grid(egno, nx, ny):
    x_arr = O.make_grid(2, nx, ny, egno)
    return x_arr, x_arr[0, :, 0, 0], x_arr[0, 0, :, 1]


def _single(egno, nx, ny, T, prec, epsl, k=1):
    from pdhg_amd.context import PDHGContext
    _, xs, ys = _grid(egno, nx, ny)
    return PDHGContext(egno, 2, nx, ny, T, 2.0 / nx, 2.0 / ny, DT, xs, ys, epsl=epsl, c_on_rho=C_RHO, precision=prec,
                       rho_alp_iters=k)


def _multi(egno, nx, ny, T, prec, epsl, devices, k=1):
    from pdhg_amd.multi import MultiContext
    _, xs, ys = _grid(egno, nx, ny)
    return MultiContext(egno, nx, ny, T, 2.0 / nx, 2.0 / ny, DT, xs, ys, devices=devices, epsl=epsl, c_on_rho=C_RHO,
                        precision=prec, rho_alp_iters=k)


def _env(monkeypatch, tile_env):
    monkeypatch.delenv("PDHG_REPORT_WGS", raising=False)
    if tile_env is None:
        monkeypatch.delenv("PDHG_REPORT_TILE", raising=False)
    else:
        monkeypatch.setenv("PDHG_REPORT_TILE", tile_env)


def _same_rows(name, got, want, bounds=None):
    """Bitwise equality of field rows; a failure names the first global row that differs and whose slab edge it is."""
    if np.array_equal(got, want, equal_nan=True):
        return
    bad = [j for j in range(want.shape[0]) if not np.array_equal(got[j], want[j], equal_nan=True)]
    edge = ""
    if bounds:
        edge = " (slab rows {}: first rows {}, last rows {})".format(bounds, [b[0] for b in bounds],
                                                                    [b[1] - 1 for b in bounds])
    raise AssertionError("{}: rows {} differ, max |diff| {:.3e}{}".format(
        name, bad, float(np.nanmax(np.abs(got[bad] - want[bad]))), edge))


def _same_stats(d, ref):
    assert set(d) == set(ref)
    n = ref["n_points"]
    for k in EXACT:
        if isinstance(ref[k], float) and np.isnan(ref[k]):
            assert np.isnan(d[k]), k
        else:
            assert d[k] == ref[k], (k, d[k], ref[k])
    for k in SUMS:
        if np.isnan(ref[k]):
            assert np.isnan(d[k]), k
        else:
            print("{}: multi {!r} single {!r} rel {:.3e} (bound {:.3e})".format(
                k, d[k], ref[k], abs(d[k] - ref[k]) / max(abs(ref[k]), 1e-300), 2 * n * 2.0 ** -53))
            assert d[k] == pytest.approx(ref[k], rel=2 * n * 2.0 ** -53, abs=0), (k, d[k], ref[k])


FIELD_CASES = [(sh, ph, sp, pr) for sh in SHAPES for ph in PHYS for sp in SPLITS for pr in SHAPES[sh][4]]


@pytest.mark.parametrize("shape, phys, split, prec", FIELD_CASES)
def test_fields_and_statistics_equal_single_context(native, monkeypatch, shape, phys, split, prec):
    """(1), (2): the seeded state in a single and a multi-device context: both fields bitwise, counts and extrema
    equal, the sum-derived fields to the reorder bound, a repeated call bitwise."""
    nx, ny, tile, tile_env, _ = SHAPES[shape]
    egno, epsl = PHYS[phys]
    T, devs = SPLITS[split]
    _env(monkeypatch, tile_env)
    st = _state(egno, 2, nx, ny, T, seed=7)
    ctx, m = _single(egno, nx, ny, T, prec, epsl), _multi(egno, nx, ny, T, prec, epsl, devs)
    try:
        assert ctx.path_info("report_tile") == tile
        assert [m.info("rows:%d" % r) for r in range(len(devs))] == [b - a for a, b in _bounds(T, len(devs))]
        ctx.set_state(*st)
        m.set_state(*st)
        hj, cont = ctx.residual_rows(0, T)
        hj_m, cont_m = m.residual_rows(0, T)
        assert np.isfinite(hj).all() and np.isfinite(cont).all()
        _same_rows("hj", hj_m, hj, _bounds(T, len(devs)))
        _same_rows("cont", cont_m, cont, _bounds(T, len(devs)))
        d = m.report()
        _same_stats(d, ctx.report())
        assert d["n_points"] == T * nx * ny and d["n_rho_zero"] > 0
        assert m.report() == d
    finally:
        ctx.close()
        m.close()


def _iterated(monkeypatch, k, tile_env=None):
    """(3): a multi-device context after 3 iterations from init_state; its state in a fresh single context."""
    from pdhg_amd import set_fns
    _env(monkeypatch, tile_env)
    egno, epsl, nx, ny = 2, 0.1, 16, 512
    T, devs = SPLITS["T7x3"]
    g = set_fns.set_up_J(egno, 2, (2.0, 2.0))(_grid(egno, nx, ny)[0])
    m = _multi(egno, nx, ny, T, "fp64", epsl, devs, k=k)
    ctx = _single(egno, nx, ny, T, "fp64", epsl, k=k)
    m.init_state(g)
    st = m.iterate(3, TAU, SIGMA, -1.0, k)
    assert st["iters_run"] == 3 and st["status"] == 0
    ctx.set_state(*m.get_state())
    return m, ctx, T, _bounds(T, len(devs))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("tile_env", [None, "0"], ids=["tile", "point"])
def test_halos_are_fresh_after_iterations(native, monkeypatch, k, tile_env):
    """(3): after iterations a slab's rho halo is stale (it holds the row before the last dual sweep) and its phi row
    0 is not maintained at all: a report that read either would differ from the single context in the continuity row
    at each slab's last row, or in the HJ row at each slab's first row.  k = 2 on a rho_alp_iters = 2 context: the
    device-selected current buffer set is the second one."""
    m, ctx, T, bounds = _iterated(monkeypatch, k, tile_env)
    try:
        hj, cont = ctx.residual_rows(0, T)
        hj_m, cont_m = m.residual_rows(0, T)
        assert np.abs(hj).max() > 0 and np.abs(cont).max() > 0
        for a, b in bounds[:-1]:
            assert np.array_equal(cont_m[b - 1], cont[b - 1]), \
                "continuity row {} (last row of slab [{}, {})): stale rho halo?".format(b - 1, a, b)
        for a, b in bounds[1:]:
            assert np.array_equal(hj_m[a], hj[a]), \
                "HJ row {} (first row of slab [{}, {})): stale or unmaintained phi row 0?".format(a, a, b)
        _same_rows("hj", hj_m, hj, bounds)
        _same_rows("cont", cont_m, cont, bounds)
        _same_stats(m.report(), ctx.report())
    finally:
        m.close()
        ctx.close()


def test_fields_against_host_reference(native, parity_log, monkeypatch):
    """(4): one fp64 case of (1) against the host definitions, with test_gpu_report.py's helpers and bound."""
    import test_gpu_report as R
    _env(monkeypatch, None)
    egno, epsl = PHYS["e2"]
    nx, ny = 16, 512
    T, devs = SPLITS["T7x3"]
    case = (egno, 2, nx, ny, T)
    assert (R.DT, R.C_RHO) == (DT, C_RHO)
    m = _multi(egno, nx, ny, T, "fp64", epsl, devs)
    try:
        m.set_state(*_state(*case, seed=7))
        _, hj_ref, cont_ref, s_r, s_c, _ = R._reference(case, m, epsl)
        hj, cont = m.residual_rows(0, T)
        u = R.U_OF["fp64"]
        q_r, q_c = R._ratio(hj, hj_ref, s_r, u), R._ratio(cont, cont_ref, s_c, u)
        print("max |dev - ref| / (u S): hj {:.3g} cont {:.3g}".format(q_r, q_c))
        parity_log("test_gpu_multi_report", "tile/T7x3/fp64/eps0.1", {"hj_ratio": q_r, "cont_ratio": q_c},
                   {"hj_ratio": 64.0, "cont_ratio": 64.0})
        assert q_r <= 64.0 and q_c <= 64.0, (q_r, q_c)
    finally:
        m.close()


@pytest.mark.parametrize("tile_env", [None, "0"], ids=["tile", "point"])
def test_nan_on_a_slab_boundary(native, monkeypatch, tile_env):
    """(5): a NaN in phi at global row 3 of T = 7 over 3 slabs: slab 0's row T and the phi halo of slab 1."""
    _env(monkeypatch, tile_env)
    egno, epsl = PHYS["e2"]
    nx, ny = 16, 512
    T, devs = SPLITS["T7x3"]
    assert _bounds(T, len(devs))[1][0] == 3
    phi, rho, alp = _state(egno, 2, nx, ny, T, seed=11)
    phi[3, 8, 0] = np.nan
    ctx, m = _single(egno, nx, ny, T, "fp64", epsl), _multi(egno, nx, ny, T, "fp64", epsl, devs)
    try:
        ctx.set_state(phi, rho, alp)
        m.set_state(phi, rho, alp)
        hj, cont = ctx.residual_rows(0, T)
        hj_m, cont_m = m.residual_rows(0, T)
        _same_rows("hj", hj_m, hj)
        _same_rows("cont", cont_m, cont)
        d, ref = m.report(), ctx.report()
        assert d["n_nonfinite"] == ref["n_nonfinite"] == int((~np.isfinite(hj)).sum()) == 6
        _same_stats(d, ref)
    finally:
        ctx.close()
        m.close()


def test_row_ranges(native, monkeypatch):
    """(6): ranges inside one slab, across two slab boundaries and of one boundary row; bad ranges."""
    N = native
    _env(monkeypatch, None)
    egno, epsl = PHYS["e2"]
    nx, ny = 16, 512
    T, devs = SPLITS["T7x3"]           # slabs [0, 3), [3, 5), [5, 7)
    m = _multi(egno, nx, ny, T, "fp32", epsl, devs)
    try:
        m.set_state(*_state(egno, 2, nx, ny, T, seed=5))
        hj, cont = m.residual_rows(0, T)
        for r0, n in ((1, 1), (0, 2), (2, 4), (3, 1), (4, 3), (6, 1)):
            h, c = m.residual_rows(r0, n)
            assert np.array_equal(h, hj[r0:r0 + n]) and np.array_equal(c, cont[r0:r0 + n]), (r0, n)
        h, c = m.residual_rows(2, 4, hj=False)
        assert h is None and np.array_equal(c, cont[2:6])
        buf = np.zeros((T + 1, nx, ny))
        for r0, n in ((0, T + 1), (T, 1), (-1, 1), (0, 0), (3, T - 2)):
            rc = m._lib.pdhg_multi_report_rows(m._h, r0, n, N.dptr(buf), None)
            assert rc == N.PDHG_ERR_ARG and m._lib.pdhg_last_error(), (r0, n)
        assert m._lib.pdhg_multi_report_state(m._h, None) == N.PDHG_ERR_ARG
        assert m._lib.pdhg_multi_report_rows(m._h, 0, T, None, None) == N.PDHG_OK   # null pointers are skipped
    finally:
        m.close()


def test_row_chunks_inside_a_slab(native, monkeypatch):
    """(6b): slabs with more rows than one staging chunk holds.  512 x 512 with both fields takes 2 * 512 * 512 * 8 B
    = 4 MiB per row against the 64 MiB staging budget: 16 rows per chunk, so each 18-row slab of T = 36 over two slabs
    runs a chunk of 16 rows and one of 2.  The whole window, and a range across the slab boundary (row 18) and a chunk
    boundary (15 + 16 = 31 lies in slab 1's first chunk [18, 34); slab 0 contributes [15, 18)), against the single
    context's rows, bit for bit."""
    _env(monkeypatch, None)
    egno, epsl = PHYS["e2"]
    nx = ny = 512
    T, devs = 36, [0, 0]
    assert (64 << 20) // (2 * nx * ny * 8) == 16
    st = _state(egno, 2, nx, ny, T, seed=7)
    ctx, m = _single(egno, nx, ny, T, "fp32", epsl), _multi(egno, nx, ny, T, "fp32", epsl, devs)
    try:
        assert [m.info("rows:%d" % r) for r in range(2)] == [18, 18]      # more than the 16 rows of a chunk
        ctx.set_state(*st)
        m.set_state(*st)
        for r0, n in ((0, T), (15, 20)):
            hj, cont = ctx.residual_rows(r0, n)
            h, c = m.residual_rows(r0, n)
            assert hj.shape == (n, nx, ny) and np.isfinite(hj).all() and np.isfinite(cont).all()
            assert np.array_equal(h, hj) and np.array_equal(c, cont), (r0, n)
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_no_side_effects(native, monkeypatch, prec):
    """(7): iterate(2), report + residual_rows + trajectories, iterate(2) ends in the state and the stop statistics
    of iterate(4), bit for bit."""
    from pdhg_amd import set_fns
    _env(monkeypatch, None)
    egno, epsl = PHYS["e2"]
    nx, ny = 16, 512
    T, devs = SPLITS["T7x3"]
    g = set_fns.set_up_J(egno, 2, (2.0, 2.0))(_grid(egno, nx, ny)[0])
    keys = ("status", "inner_last", "err1", "err2", "err_inner", "nan_seen", "first_nan_iter")
    a, b = _multi(egno, nx, ny, T, prec, epsl, devs), _multi(egno, nx, ny, T, prec, epsl, devs)
    try:
        a.init_state(g)
        b.init_state(g)
        sa = a.iterate(2, TAU, SIGMA, -1.0, 1)
        r1 = a.report()
        rows = a.residual_rows(0, T)
        x0 = np.random.default_rng(3).uniform(-1.0, 3.0, (300, 2))
        ta, tx, xf = a.trajectories(x0, "linear", 2.0, 2.0, seed=4)
        assert a.report() == r1 and np.isfinite(rows[0]).all() and np.isfinite(xf).all()
        sa2 = a.iterate(2, TAU, SIGMA, -1.0, 1)
        sb = b.iterate(4, TAU, SIGMA, -1.0, 1)
        assert sa["iters_run"] == sa2["iters_run"] == 2 and sb["iters_run"] == 4
        assert {q: sa2[q] for q in keys} == {q: sb[q] for q in keys}
        assert sa["inner_total"] + sa2["inner_total"] == sb["inner_total"]
        pa, pb = a.get_state(), b.get_state()
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
        assert all(np.array_equal(u, v) for u, v in zip(pa[2], pb[2]))
        assert a.report() == b.report() and a.report() != r1
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_slab_runner_report_equals_multi_context(native, monkeypatch, prec):
    """(8): SlabRunner.report() over LocalComm: the same slabs, kernels and slab-ordered fold as the multi-device
    context, so the same dict; pdhg_device_bytes counts the report's table and the phi halo plane."""
    import torch
    from pdhg_amd.slab import LocalComm, SlabContext, SlabRunner, slab_bounds, split_state
    _env(monkeypatch, None)
    egno, epsl = PHYS["e2"]
    nx, ny = 16, 512
    T, devs = SPLITS["T7x3"]
    nr = len(devs)
    _, xs, ys = _grid(egno, nx, ny)
    st = _state(egno, 2, nx, ny, T, seed=7)
    m = _multi(egno, nx, ny, T, prec, epsl, devs)
    slabs = [SlabContext(r, nr, T, egno, nx, ny, 2.0 / nx, 2.0 / ny, DT, xs, ys, epsl=epsl, c_on_rho=C_RHO,
                         precision=prec) for r in range(nr)]
    try:
        m.set_state(*st)
        for s, part in zip(slabs, split_state(*st, slab_bounds(T, nr))):
            s.set_state(*part)
        runner = SlabRunner(slabs, LocalComm(nr))
        before = [s.device_bytes() for s in slabs]
        d = runner.report()
        torch.cuda.synchronize()
        assert d == m.report() and runner.report() == d
        esz = 8 if prec == "fp64" else 4
        grew = [s.device_bytes() - b for s, b in zip(slabs, before)]
        plane = nx * ny * esz          # the first slab allocates the table alone, the others the phi halo plane too
        assert 0 < grew[0] < plane and grew[1] == grew[2] and plane < grew[1] < 2 * plane, (grew, plane)
        for s in slabs:   # the inherited single-context calls stay refused on a slab
            with pytest.raises(native.PDHGUnsupported):
                s.report()
    finally:
        m.close()
        for s in slabs:
            s.close()


def test_slab_entry_points_check_their_arguments(native):
    N = native
    egno, epsl = PHYS["e2"]
    ctx = _single(egno, 16, 512, 4, "fp32", epsl)
    try:
        sums = (ctypes.c_double * 16)()
        assert ctx._lib.pdhg_slab_report(ctx._h, None, sums) == N.PDHG_ERR_STATE        # not a t-slab context
        assert ctx._lib.pdhg_slab_report_rows(ctx._h, None, 0, 1, None, None) == N.PDHG_ERR_STATE
        assert ctx._lib.pdhg_slab_report(ctx._h, None, None) == N.PDHG_ERR_ARG
        assert ctx._lib.pdhg_slab_report_rows(ctx._h, None, -1, 1, None, None) == N.PDHG_ERR_ARG
        assert ctx._lib.pdhg_multi_report_state(ctx._h, ctypes.byref(N.pdhg_report())) == N.PDHG_ERR_ARG
    finally:
        ctx.close()
