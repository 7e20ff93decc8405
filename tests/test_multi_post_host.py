"""The report and the trajectories on decomposed windows, the parts that need no device: the new symbols in the header,
the binding and the library, their argument checks that come before any device is touched, the Python surface, and the
host side of SlabRunner.report() -- the slab-ordered fold of the slabs' rows of 16 sums and pdhg_report's arithmetic
on the folded row (pdhg_amd.report.fold_report_rows / report_from_sums) against NumPy over the same fields."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

NEW = ("pdhg_slab_report", "pdhg_slab_report_rows", "pdhg_slab_trajectories", "pdhg_multi_report_state",
       "pdhg_multi_report_rows", "pdhg_multi_trajectories")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


def test_new_symbols_are_declared_bound_and_exported(lib):
    import test_abi
    declared = test_abi.header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pdhg_\w+)", out))
    L = lib.load()
    for f in NEW:
        assert f in declared and f in lib.EXPORTS and f in exported, f
        assert getattr(L, f).restype is ctypes.c_int and getattr(L, f).argtypes


def test_argument_checks_before_any_device(lib):
    L = lib.load()
    rep, sums = lib.pdhg_report(), (ctypes.c_double * 16)()
    o = lib.pdhg_traj_opts()
    o.n_sample, o.x_period, o.y_period = 4, 2.0, 2.0
    x = np.zeros((4, 2))
    for rc in (L.pdhg_multi_report_state(None, ctypes.byref(rep)), L.pdhg_multi_report_rows(None, 0, 1, None, None),
               L.pdhg_multi_trajectories(None, ctypes.byref(o), lib.dptr(x), None, None, None, None),
               L.pdhg_slab_report(None, None, sums), L.pdhg_slab_report(None, None, None),
               L.pdhg_slab_report_rows(None, None, 0, 1, None, None),
               L.pdhg_slab_trajectories(None, ctypes.byref(o), 0, 4, sums, None, sums, None, None),
               L.pdhg_slab_trajectories(None, None, 0, 4, sums, None, sums, None, None)):
        assert rc == lib.PDHG_ERR_ARG and L.pdhg_last_error().decode()
    # a handle of the other kind is recognised by its tag, not dereferenced further
    fake = (ctypes.c_uint32 * 16)()
    assert L.pdhg_multi_report_state(ctypes.cast(fake, ctypes.c_void_p), ctypes.byref(rep)) == lib.PDHG_ERR_ARG


def test_python_surface():
    import inspect
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.multi import MultiContext
    from pdhg_amd.slab import PHI_LAST, SlabContext, SlabRunner
    for name in ("report", "residual_rows", "trajectories"):
        want = inspect.signature(getattr(PDHGContext, name))
        assert inspect.signature(getattr(MultiContext, name)) == want, name
        # a slab keeps the single context's (refused) calls: nothing of that name is defined on SlabContext itself
        assert name not in vars(SlabContext), name
    assert {"report_partial", "report_rows_partial", "trajectories_partial"} <= set(vars(SlabContext))
    assert "report" in vars(SlabRunner) and "trajectories" not in vars(SlabRunner)
    assert PHI_LAST == 4


def _fields(rng, T, nx, ny, nan_at=None):
    hj, cont = rng.standard_normal((T, nx, ny)), rng.standard_normal((T, nx, ny))
    rho = np.maximum(rng.standard_normal((T, nx, ny)) + 0.5, 0.0)
    phi = rng.standard_normal((T, nx, ny))
    if nan_at is not None:
        phi[nan_at] = np.nan
    return hj, cont, rho, phi


def _sums_row(hj, cont, rho, phi):
    """One slab's row of the 16 sums as csrc/kernels_report.hpp defines them (rep_accum, RepAcc::init)."""
    ok = np.isfinite(hj) & np.isfinite(cont) & np.isfinite(rho) & np.isfinite(phi)
    r, c, q, p = hj[ok], cont[ok], rho[ok], phi[ok]
    a = np.abs(r)
    mx = lambda v, init: float(v.max()) if v.size else init  # noqa: E731
    return [a.sum(), (r * r).sum(), (q * a).sum(), q.sum(), np.abs(c).sum(), (c * c).sum(), float((~ok).sum()),
            float((q == 0).sum()), mx(a, 0.0), max(mx(r, 0.0), 0.0), mx(a[q > 0], 0.0), mx(np.abs(c), 0.0),
            mx(q, -np.inf), mx(-q, -np.inf), mx(p, -np.inf), mx(-p, -np.inf)]


@pytest.mark.parametrize("nan_at", [None, (3, 2, 1)])
def test_slab_ordered_fold_gives_the_window_report(nan_at):
    """Rows of T = 7 over slabs 3 / 2 / 2, folded in slab order: counts and extrema are NumPy's over the whole window,
    the sum-derived fields agree to 2 n 2^-53 relative (two fp64 summations of n terms of one sign in different
    orders); a slab without a finite point contributes its initial values."""
    from pdhg_amd.report import fold_report_rows, report_from_fields, report_from_sums
    from pdhg_amd.slab import slab_bounds
    T, nx, ny = 7, 5, 6
    hj, cont, rho, phi = _fields(np.random.default_rng(1), T, nx, ny, nan_at)
    rows = [_sums_row(hj[a:b], cont[a:b], rho[a:b], phi[a:b]) for a, b in slab_bounds(T, 3)]
    d = report_from_sums(fold_report_rows(rows), T * nx * ny)
    want = report_from_fields(hj, cont, rho, phi)
    assert set(d) == set(want)
    for k, v in want.items():
        if k in ("hj_l1", "hj_l2", "compl_l1", "cont_l1", "cont_l2", "rho_mean"):
            assert d[k] == pytest.approx(v, rel=2 * T * nx * ny * 2.0 ** -53, abs=0), k
        else:
            assert d[k] == v, (k, d[k], v)
    assert d["n_nonfinite"] == (0 if nan_at is None else 1)
    # all points of the middle slab non-finite: it adds nothing but its count
    bad = phi.copy()
    bad[3:5] = np.nan
    rows = [_sums_row(hj[a:b], cont[a:b], rho[a:b], bad[a:b]) for a, b in slab_bounds(T, 3)]
    d = report_from_sums(fold_report_rows(rows), T * nx * ny)
    want = report_from_fields(hj, cont, rho, bad)
    assert d["n_nonfinite"] == want["n_nonfinite"] == 2 * nx * ny and d["phi_max"] == want["phi_max"]
    assert d["rho_min"] == want["rho_min"] and d["hj_max"] == want["hj_max"]
    # no finite point at all: every double is NaN, as pdhg_report_state
    rows = [_sums_row(hj[a:b], cont[a:b], rho[a:b], np.full_like(phi[a:b], np.nan)) for a, b in slab_bounds(T, 3)]
    d = report_from_sums(fold_report_rows(rows), T * nx * ny)
    assert d["n_nonfinite"] == d["n_points"] and all(np.isnan(v) for k, v in d.items() if not k.startswith("n_"))


def test_fold_order_is_the_slab_order():
    """The fold adds the rows one after the other from slab 0: with terms of very different size the result is the
    left-to-right sum, not a pairwise or sorted one."""
    from pdhg_amd.report import fold_report_rows
    rows = np.zeros((3, 16))
    rows[:, 0] = (1.0, 2.0 ** -53, 2.0 ** -53)
    rows[:, 8:] = -np.inf
    rows[:, 12] = (1.0, 3.0, 2.0)
    f = fold_report_rows(rows)
    assert f[0] == 1.0 and f[12] == 3.0            # (1 + e) + e = 1 in fp64; e + e + 1 would be 1 + 2^-52
    assert fold_report_rows(rows[::-1])[0] == 1.0 + 2.0 ** -52
