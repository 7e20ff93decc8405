"""Solution report on the host: the definitions behind ``PDHGContext.report`` in NumPy, for host-sized states.

``report_from_arrays`` evaluates the reference's two residuals on (phi, rho, alp) arrays and reduces them exactly as
``pdhg_report_state`` does on the device (include/pdhg.h): point (j, x, y), j = 0..T-1, pairs HJ residual row j, rho
row j, phi row j+1 and continuity residual row j+1.

* HJ residual  ``r = Dt phi - epsl Lap phi - f(alp) . D phi - L(alp)``   (update_fns_in_pdhg.py:49-70); at the saddle
  point r <= 0 everywhere and r = 0 where rho > 0.
* continuity residual ``c``  (update_fns_in_pdhg.py:72-96, rows 1..T of its [T+1] array; the last row carries
  ``+ c_on_rho / dt``); 0 at the saddle point: it is what the primal step adds to phi.

The stencils are utils_diff_op.py's (bc 0 periodic, 1 Neumann, 2 Dirichlet).
"""
import numpy as np

from ._native import REPORT_FIELDS
from .update_fns_in_pdhg import get_f_vals_1d, get_f_vals_2d


def _edge(a, axis, sl):
    idx = [slice(None)] * a.ndim
    idx[axis] = sl
    return a[tuple(idx)]


def _zero(a, axis):
    return np.zeros_like(_edge(a, axis, slice(0, 1)))


def _d_right(a, d, bc, axis):           # utils_diff_op.py:9-23, :93-107
    if bc == 0:
        out = np.roll(a, -1, axis=axis) - a
    elif bc == 1:
        out = np.concatenate([_edge(a, axis, slice(1, None)) - _edge(a, axis, slice(None, -1)), _zero(a, axis)], axis=axis)
    elif bc == 2:
        out = np.concatenate([_edge(a, axis, slice(1, None)), _zero(a, axis)], axis=axis) - a
    else:
        raise NotImplementedError("bc {}".format(bc))
    return out / d


def _d_left(a, d, bc, axis):            # utils_diff_op.py:51-65, :135-149
    if bc == 0:
        out = a - np.roll(a, 1, axis=axis)
    elif bc == 1:
        out = np.concatenate([_zero(a, axis), _edge(a, axis, slice(1, None)) - _edge(a, axis, slice(None, -1))], axis=axis)
    elif bc == 2:
        out = a - np.concatenate([_zero(a, axis), _edge(a, axis, slice(None, -1))], axis=axis)
    else:
        raise NotImplementedError("bc {}".format(bc))
    return out / d


def _d_second(a, d, bc, axis):          # utils_diff_op.py:208-226, :255-273
    if bc == 0:
        up, dn = np.roll(a, -1, axis=axis), np.roll(a, 1, axis=axis)
    elif bc == 1:
        up = np.concatenate([_edge(a, axis, slice(1, None)), _edge(a, axis, slice(-1, None))], axis=axis)
        dn = np.concatenate([_edge(a, axis, slice(0, 1)), _edge(a, axis, slice(None, -1))], axis=axis)
    elif bc == 2:
        up = np.concatenate([_edge(a, axis, slice(1, None)), _zero(a, axis)], axis=axis)
        dn = np.concatenate([_zero(a, axis), _edge(a, axis, slice(None, -1))], axis=axis)
    else:
        raise NotImplementedError("bc {}".format(bc))
    return (up + dn - 2 * a) / d ** 2


def _bcs(bc, ndim):
    return (bc,) if ndim == 1 else tuple(bc)


def hj_residual(phi, alp, dt, dspatial, fns_dict, epsl, x_arr, t_arr, bc):
    """compute_HJ_residual_1d / _2d (update_fns_in_pdhg.py:49-70): [T, nx(, ny)] from phi [T+1, ...]."""
    phi = np.asarray(phi, dtype=np.float64)
    ndim = phi.ndim - 1
    bcs = _bcs(bc, ndim)
    L = fns_dict.numerical_L_fn(alp, x_arr, t_arr)
    f = (get_f_vals_1d if ndim == 1 else get_f_vals_2d)(fns_dict.f_fn, alp, x_arr, t_arr)
    vec = (phi[1:] - phi[:-1]) / dt
    for ax in range(ndim):
        vec = vec - epsl * _d_second(phi, dspatial[ax], bcs[ax], ax + 1)[1:]
    adv = 0
    for ax in range(ndim):
        term = _d_right(phi, dspatial[ax], bcs[ax], ax + 1)[1:] * f[2 * ax]
        adv = term if ax == 0 else adv + term
        adv = adv + _d_left(phi, dspatial[ax], bcs[ax], ax + 1)[1:] * f[2 * ax + 1]
    return vec - adv - L


def cont_residual(rho, alp, dt, dspatial, fns_dict, c_on_rho, epsl, x_arr, t_arr, bc):
    """Rows 1..T of compute_cont_residual_1d / _2d (update_fns_in_pdhg.py:72-96; its row 0 is identically zero):
    [T, nx(, ny)], the row the preconditioner consumes for unknown row j at index j."""
    rho = np.asarray(rho, dtype=np.float64)
    ndim = rho.ndim - 1
    bcs = _bcs(bc, ndim)
    f = (get_f_vals_1d if ndim == 1 else get_f_vals_2d)(fns_dict.f_fn, alp, x_arr, t_arr)
    m = [(rho + 1e-4) * fi for fi in f]
    nxt = np.concatenate([rho[1:], np.zeros_like(rho[0:1])], axis=0)
    res = (nxt - rho) / dt
    for ax in range(ndim):
        res = res + epsl * _d_second(rho, dspatial[ax], bcs[ax], ax + 1)
    div = 0
    for ax in range(ndim):
        term = _d_left(m[2 * ax], dspatial[ax], bcs[ax], ax + 1)
        div = term if ax == 0 else div + term
        div = div + _d_right(m[2 * ax + 1], dspatial[ax], bcs[ax], ax + 1)
    res = res - div
    res[-1] = res[-1] + c_on_rho / dt
    return res


def report_from_fields(hj, cont, rho, phi_rows):
    """The statistics of pdhg_report from the two field arrays, rho [T, ...] and phi rows 1..T (all the same shape)."""
    hj, cont, rho, phi_rows = (np.asarray(a, dtype=np.float64) for a in (hj, cont, rho, phi_rows))
    ok = np.isfinite(hj) & np.isfinite(cont) & np.isfinite(rho) & np.isfinite(phi_rows)
    n = int(ok.sum())
    d = dict.fromkeys(REPORT_FIELDS, float("nan"))
    d["n_points"] = int(hj.size)
    d["n_nonfinite"] = int(hj.size) - n
    r, c, q, p = hj[ok], cont[ok], rho[ok], phi_rows[ok]
    d["n_rho_zero"] = int((q == 0).sum())
    if n == 0:
        return d
    a = np.abs(r)
    s_rho = float(q.sum())
    d.update(hj_l1=float(a.sum()) / n, hj_l2=float(np.sqrt((r * r).sum() / n)), hj_max=float(a.max()),
             hj_pos_max=float(np.maximum(r, 0.0).max()),
             hj_active_max=float(a[q > 0].max()) if np.any(q > 0) else 0.0,
             compl_l1=float((q * a).sum()) / s_rho if s_rho != 0 else 0.0,
             cont_l1=float(np.abs(c).sum()) / n, cont_l2=float(np.sqrt((c * c).sum() / n)),
             cont_max=float(np.abs(c).max()), rho_min=float(q.min()), rho_max=float(q.max()), rho_mean=s_rho / n,
             phi_min=float(p.min()), phi_max=float(p.max()))
    return d


def fold_report_rows(rows):
    """Fold per-slab rows of the report's 16 sums (pdhg_slab_report) in the order given -- slab order: columns 0-7
    are sums (added), 8-15 extrema (maximised; the minima are stored negated).  A fixed order, unlike an all-reduce."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 16)
    out = rows[0].copy()
    for row in rows[1:]:
        out[:8] = out[:8] + row[:8]
        out[8:] = np.fmax(out[8:], row[8:])
    return out


def report_from_sums(h, n_points):
    """pdhg_report's fields from one folded row of the 16 sums over n_points points (the arithmetic of
    pdhg_report_state / pdhg_multi_report_state, operation for operation)."""
    h = [float(v) for v in h]
    d = dict.fromkeys(REPORT_FIELDS, float("nan"))
    d["n_points"], d["n_nonfinite"], d["n_rho_zero"] = int(n_points), int(h[6]), int(h[7])
    n = float(d["n_points"] - d["n_nonfinite"])
    if n > 0:
        d.update(hj_l1=h[0] / n, hj_l2=float(np.sqrt(h[1] / n)), compl_l1=0.0 if h[3] == 0.0 else h[2] / h[3],
                 rho_mean=h[3] / n, cont_l1=h[4] / n, cont_l2=float(np.sqrt(h[5] / n)), hj_max=h[8], hj_pos_max=h[9],
                 hj_active_max=h[10], cont_max=h[11], rho_max=h[12], rho_min=-h[13], phi_max=h[14], phi_min=-h[15])
    return d


def report_from_arrays(phi, rho, alp, fns_dict, dt, dspatial, c_on_rho, epsl, x_arr, t_arr, bc, fields=False):
    """PDHGContext.report's dict from host arrays in the reference layouts (phi [T+1, ...], rho [T, ...], alp the tuple
    of 2 / 4 control arrays).  fields=True returns (dict, hj [T, ...], cont [T, ...]) -- what
    PDHGContext.residual_rows(0, T) returns."""
    phi = np.asarray(phi, dtype=np.float64)
    rho = np.asarray(rho, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        hj = hj_residual(phi, alp, dt, dspatial, fns_dict, epsl, x_arr, t_arr, bc)
        cont = cont_residual(rho, alp, dt, dspatial, fns_dict, c_on_rho, epsl, x_arr, t_arr, bc)
        d = report_from_fields(hj, cont, rho, phi[1:])
    return (d, hj, cont) if fields else d


def format_report(d):
    """One line: the residual norms and ranges of a report dict."""
    return ("HJ |r| l1 {hj_l1:.3e} l2 {hj_l2:.3e} max {hj_max:.3e} (r>0 max {hj_pos_max:.3e}, rho>0 max "
            "{hj_active_max:.3e}, rho-weighted {compl_l1:.3e}); cont |c| l1 {cont_l1:.3e} l2 {cont_l2:.3e} max "
            "{cont_max:.3e}; rho [{rho_min:.3e}, {rho_max:.3e}] mean {rho_mean:.3e}, {n_rho_zero} zero; phi "
            "[{phi_min:.3e}, {phi_max:.3e}]; {n_nonfinite} of {n_points} points non-finite").format(**d)
