"""Solution report without a GPU: the ABI struct and argument checks, the "report_tile" plan key, and the host
definitions (pdhg_amd.report) against the oracle's compute_HJ_residual_* / compute_cont_residual_* and a direct NumPy
evaluation of the statistics."""
import ctypes

import numpy as np
import pytest

import pdhg_oracle as O
from _report_support import setup as _setup, state as _state


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


def test_struct_layout(lib):
    assert ctypes.sizeof(lib.pdhg_report) == 144 == 4 * 8 + 14 * 8
    assert len(lib.REPORT_FIELDS) == 17 and "reserved0" not in lib.REPORT_FIELDS


def test_null_and_bad_arguments(lib):
    L = lib.load()
    rep = lib.pdhg_report()
    buf = np.zeros(4)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))   # not a context: no magic
    for rc in (L.pdhg_report_state(None, ctypes.byref(rep)), L.pdhg_report_state(fake, None),
               L.pdhg_report_state(fake, ctypes.byref(rep)),
               L.pdhg_report_rows(None, 0, 1, lib.dptr(buf), None), L.pdhg_report_rows(fake, -1, 1, None, None),
               L.pdhg_report_rows(fake, 0, 0, None, None), L.pdhg_report_rows(fake, 0, 1, lib.dptr(buf), None)):
        assert rc == lib.PDHG_ERR_ARG
        assert L.pdhg_last_error()


def _problem(lib, egno, ndim, nx, ny, T, precision=4):
    ny = ny if ndim == 2 else 1
    xs, ys = np.linspace(0, 2, nx, endpoint=False), np.linspace(0, 2, ny, endpoint=False)
    p = lib.pdhg_problem()
    p.egno, p.ndim, p.nx, p.ny, p.T, p.precision, p.rho_alp_iters = egno, ndim, nx, ny, T, precision, 1
    bc = O.default_bc(egno, ndim)
    p.bc_x, p.bc_y = (bc, 0) if ndim == 1 else bc
    p.dx, p.dy, p.dt, p.C, p.pow_, p.Ct, p.c_on_rho = 2 / nx, 2 / ny, 0.025, 1.0, 1.0, 1.0, 70.0
    p.xs, p.ys = lib.dptr(xs), lib.dptr(ys)
    return p, (xs, ys)


def _plan(lib, p, key="report_tile"):
    v = ctypes.c_int(-12345)
    rc = lib.load().pdhg_plan_info(ctypes.byref(p), key.encode(), ctypes.byref(v))
    assert rc == lib.PDHG_OK, lib.load().pdhg_last_error()
    return v.value


@pytest.mark.parametrize("shape, expect", [((1, 2, 16, 512, 3), 1), ((3, 2, 16, 256, 2), 1), ((1, 2, 12, 20, 3), 0),
                                           ((1, 2, 16, 384, 3), 0), ((1, 2, 12, 512, 3), 0), ((1, 1, 1024, 1, 3), 0)])
def test_plan_key(lib, monkeypatch, shape, expect):
    monkeypatch.delenv("PDHG_REPORT_TILE", raising=False)
    for prec in (4, 8) + ((12,) if shape[1] == 2 else ()):
        p, keep = _problem(lib, *shape, precision=prec)
        assert _plan(lib, p) == expect
    monkeypatch.delenv("PDHG_REPORT_WGS", raising=False)
    p, keep = _problem(lib, *shape)
    assert _plan(lib, p, "report_wgs") == (1024 if expect else 0)
    monkeypatch.setenv("PDHG_REPORT_WGS", "16")
    assert _plan(lib, p, "report_wgs") == (16 if expect else 0)
    monkeypatch.setenv("PDHG_REPORT_TILE", "0")
    assert _plan(lib, p) == 0 and _plan(lib, p, "report_wgs") == 0


CASES = [(1, 1, 20, 1, 4), (2, 1, 20, 1, 1), (1, 2, 10, 12, 3), (2, 2, 10, 12, 2), (3, 2, 10, 12, 3)]


def _oracle_fields(ndim, phi, rho, alp, dt, dsp, fns, c, epsl, x_arr, bc):
    hjf = O.compute_HJ_residual_1d if ndim == 1 else O.compute_HJ_residual_2d
    cf = O.compute_cont_residual_1d if ndim == 1 else O.compute_cont_residual_2d
    return (hjf(phi, alp, dt, dsp, fns, epsl, x_arr, None, bc),
            cf(rho, alp, dt, dsp, fns, c, epsl, x_arr, None, bc)[1:])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("epsl", [0.0, 0.1])
def test_fields_equal_the_oracle(lib, case, epsl):
    from pdhg_amd.report import report_from_arrays
    egno, ndim, nx, ny, T = case
    x_arr, bc, dsp, fns = _setup(*case)
    phi, rho, alp = _state(*case)
    dt, c = 0.05, 70.0
    d, hj, cont = report_from_arrays(phi, rho, alp, fns, dt, dsp, c, epsl, x_arr, None, bc, fields=True)
    hj_o, cont_o = _oracle_fields(ndim, phi, rho, alp, dt, dsp, fns, c, epsl, x_arr, bc)
    assert np.array_equal(hj, hj_o) and np.array_equal(cont, cont_o)
    assert np.abs(hj).max() > 0 and np.abs(cont).max() > 0 and (rho == 0).any()
    # the package's own example functions give the same fields
    from pdhg_amd import set_fns
    d2 = report_from_arrays(phi, rho, alp, set_fns.set_up_example_fns(egno, ndim, 0), dt, dsp, c, epsl, x_arr, None, bc)
    assert d2 == pytest.approx(d, rel=1e-12, abs=1e-12)


def _direct_stats(hj, cont, rho, phi1):
    ok = np.isfinite(hj) & np.isfinite(cont) & np.isfinite(rho) & np.isfinite(phi1)
    r, c, q, p = hj[ok], cont[ok], rho[ok], phi1[ok]
    n = r.size
    d = {"n_points": hj.size, "n_nonfinite": hj.size - n, "n_rho_zero": int(np.count_nonzero(q == 0))}
    if n:
        d.update(hj_l1=np.mean(np.abs(r)), hj_l2=np.sqrt(np.mean(r ** 2)), hj_max=np.max(np.abs(r)),
                 hj_pos_max=max(r.max(), 0.0), hj_active_max=np.abs(r[q > 0]).max(),
                 compl_l1=np.sum(q * np.abs(r)) / np.sum(q), cont_l1=np.mean(np.abs(c)),
                 cont_l2=np.sqrt(np.mean(c ** 2)), cont_max=np.max(np.abs(c)), rho_min=q.min(), rho_max=q.max(),
                 rho_mean=q.mean(), phi_min=p.min(), phi_max=p.max())
    return d


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]])
def test_statistics_equal_numpy(lib, case):
    from pdhg_amd.report import format_report, report_from_arrays
    egno, ndim, nx, ny, T = case
    x_arr, bc, dsp, fns = _setup(*case)
    phi, rho, alp = _state(*case, seed=3)
    args = (fns, 0.05, dsp, 70.0, 0.1, x_arr, None, bc)
    d = report_from_arrays(phi, rho, alp, *args)
    hj, cont = _oracle_fields(ndim, phi, rho, alp, 0.05, dsp, fns, 70.0, 0.1, x_arr, bc)
    want = _direct_stats(hj, cont, rho, phi[1:])
    assert set(d) == set(lib.REPORT_FIELDS) == set(want)
    assert d["n_nonfinite"] == 0 and d["n_rho_zero"] > 0 and d["hj_pos_max"] > 0
    for k in want:
        assert d[k] == pytest.approx(want[k], rel=1e-13, abs=0), k
    assert str(d["n_points"]) in format_report(d) and "\n" not in format_report(d)
    # one NaN in phi: the points whose stencil reads it drop out, the rest is NumPy's over the finite points
    phi_n = phi.copy()
    phi_n[(1,) + (3,) * ndim] = np.nan
    with np.errstate(invalid="ignore"):
        d = report_from_arrays(phi_n, rho, alp, *args)
        hj, cont = _oracle_fields(ndim, phi_n, rho, alp, 0.05, dsp, fns, 70.0, 0.1, x_arr, bc)
    want = _direct_stats(hj, cont, rho, phi_n[1:])
    assert 0 < want["n_nonfinite"] < 12
    for k in want:
        assert d[k] == pytest.approx(want[k], rel=1e-13, abs=0), k
    # every point non-finite: counts, and every double NaN
    with np.errstate(invalid="ignore"):
        d = report_from_arrays(np.full_like(phi, np.inf), rho, alp, *args)
    assert d["n_nonfinite"] == d["n_points"] == rho.size and d["n_rho_zero"] == 0
    assert all(np.isnan(d[k]) for k in lib.REPORT_FIELDS if not k.startswith("n_"))
