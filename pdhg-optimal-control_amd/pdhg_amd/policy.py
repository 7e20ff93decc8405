"""Policy check on the host: the definition behind ``PDHGContext.policy_eval`` in NumPy, for host-sized states.

Does following the computed feedback alp cost what phi says it costs?  phi row 0 is the terminal cost g, phi row j the
value with j dt to go, and the controls of row j act between phi rows j and j+1, so for a path started at x0 with the
window's T rows to go

    sum over steps of dt L(alp(x, t))  +  phi_0(x_T)   ~   phi_T(x0)          (in expectation when epsl > 0),

the dynamic-programming identity of the window (include/pdhg.h, pdhg_policy_eval).  Per sample

* ``value    = I[phi row T](x0)``;
* the path is the rollout's (``trajectories.compute_traj_1d`` / ``_2d`` on alp reversed in time);
* ``running  = sum_steps dt * sum_k keep_k L(a_k)`` over the interpolated control arrays a_k, keep_k the sign split of
  f(a_k) (f >= 0 for arrays 0 / 2, f < 0 for arrays 1 / 3): a component the split drops moves nothing and costs nothing;
* ``terminal = I[phi row 0](x_T)``, or 0 with ``terminal="none"``;
* ``cost = running + terminal``, ``gap = cost - value``.

``I`` is linear interpolation with the rollout's boundary extension, whatever method the controls use.
``policy_from_arrays`` is to ``PDHGContext.policy_eval`` what ``report.report_from_arrays`` is to
``PDHGContext.report``.
"""
import numpy as np
from scipy import interpolate

from . import trajectories as TR
from ._native import POLICY_FIELDS


class _Replay:
    """The rng argument of compute_traj_*: replays a [T, n, ndim] array of normals step by step (zeros without one)."""

    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def normal(self, size):
        z = np.zeros(size) if self.noise is None else np.asarray(self.noise[self.i], dtype=np.float64).reshape(size)
        self.i += 1
        return z


def _interp_2d(fields, pos, x1, x2, x_period, y_period, bc, center, method):
    """fields [K, nx, ny, C] at pos [n, 2] as compute_traj_2d interpolates alp: the grid extended over the positions'
    range (extend_bdry_2d), then interpn.  -> K arrays [n, C]."""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    g1, a = TR.extend_bdry_2d(x1, lo[0], hi[0], fields, x_period, axis=1, bc=bc[0], center=center[0])
    g2, a = TR.extend_bdry_2d(x2, lo[1], hi[1], a, y_period, axis=2, bc=bc[1], center=center[1])
    return tuple(interpolate.interpn((g1, g2), a[k], pos, method=method) for k in range(a.shape[0]))


def _phi_at(row, pos, ndim, x1, x2, x_period, y_period, bc, center):
    if ndim == 1:
        return np.interp(pos, x1, row, period=x_period)
    return _interp_2d(row[None, :, :, None], pos, x1, x2, x_period, y_period, bc, center, "linear")[0][:, 0]


def policy_report_from_samples(running, terminal, value):
    """pdhg_policy_report's fields from per-sample arrays: a sample with any of the three not finite counts in
    n_nonfinite and is left out; with no finite sample every double is NaN."""
    running, terminal, value = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (running, terminal, value))
    ok = np.isfinite(running) & np.isfinite(terminal) & np.isfinite(value)
    d = dict.fromkeys(POLICY_FIELDS, float("nan"))
    d["n_sample"], d["n_nonfinite"] = int(running.size), int(running.size - ok.sum())
    n = int(ok.sum())
    if n == 0:
        return d
    r, t, v = running[ok], terminal[ok], value[ok]
    cost = r + t
    gap = cost - v
    d.update(cost_mean=float(cost.sum()) / n, value_mean=float(v.sum()) / n, running_mean=float(r.sum()) / n,
             terminal_mean=float(t.sum()) / n, gap_mean=float(gap.sum()) / n, gap_abs_mean=float(np.abs(gap).sum()) / n,
             gap_rms=float(np.sqrt((gap * gap).sum() / n)), gap_abs_max=float(np.abs(gap).max()),
             gap_lo=float(gap.min()), gap_hi=float(gap.max()))
    return d


def policy_from_arrays(phi, alp, fns_dict, x_init, x_arr, dt, x_period, y_period=None, bc=None,
                       center=(False, False), epsl=0.0, method="linear", noise=None, terminal="phi0"):
    """PDHGContext.policy_eval's dict from host arrays in the reference layouts: phi [T+1, nx(, ny)], alp the 2 / 4
    control arrays [T, nx(, ny), n_ctrl] in PDE time order, x_arr the reference's grid array, x_init [n(, 2)], noise
    the [T, n, ndim] standard normals of the steps (None: zeros).  Carries the report's fields and running, terminal,
    value [n] and x_final [n(, 2)]."""
    if terminal not in ("phi0", "none"):
        raise ValueError("terminal must be 'phi0' or 'none', not {!r}".format(terminal))
    phi = np.asarray(phi, dtype=np.float64)
    alp = np.asarray(alp, dtype=np.float64)
    ndim = phi.ndim - 1
    T = phi.shape[0] - 1
    alp_c = alp[:, ::-1]                      # control time runs against PDE time
    t_arr = np.arange(T + 1) * float(dt)
    x0 = np.asarray(x_init, dtype=np.float64)
    x_arr = np.asarray(x_arr, dtype=np.float64)
    rng = _Replay(noise)
    if ndim == 1:
        x1, x2 = x_arr[0, :, 0], None
        _, traj_x = TR.compute_traj_1d(x0, alp_c[..., 0], fns_dict.f_fn, T + 1, x1, t_arr, x_period, T * dt, epsl,
                                       method, rng=rng)
    else:
        x1, x2 = x_arr[0, :, 0, 0], x_arr[0, 0, :, 1]
        bc = tuple(bc)
        _, traj_x = TR.compute_traj_2d(x0, alp_c, fns_dict.f_fn, T + 1, x1, x2, t_arr, x_period, y_period, T * dt, bc,
                                       center, epsl, method, rng=rng)
    with np.errstate(invalid="ignore", over="ignore"):
        value = _phi_at(phi[T], traj_x[0], ndim, x1, x2, x_period, y_period, bc, center)
        running = np.zeros(x0.shape[0])
        for ind in range(T):
            pos = traj_x[ind]
            t = T * dt - t_arr[ind]
            if ndim == 1:
                if method == "linear":
                    a = [np.interp(pos, x1, alp_c[k, ind, :, 0], period=x_period)[:, None] for k in range(2)]
                else:
                    idx = np.abs(x1 - (pos % x_period)[..., None]).argmin(axis=-1)
                    a = [alp_c[k, ind, idx, 0][:, None] for k in range(2)]
                x_in = pos[:, None] % x_period
                f = [fns_dict.f_fn(a[k], x_in, t)[..., 0] for k in range(2)]
            else:
                a = _interp_2d(alp_c[:, ind], pos, x1, x2, x_period, y_period, bc, center, method)
                if bc[0] == 0:
                    x_in = pos % np.array([x_period, y_period])
                else:
                    x_in = np.stack([pos[:, 0], pos[:, 1] % y_period], axis=-1)
                f = [fns_dict.f_fn(a[k], x_in, t)[..., 0 if k < 2 else 1] for k in range(4)]
            keep = [(fk >= 0.0) if k % 2 == 0 else (fk < 0.0) for k, fk in enumerate(f)]
            # L(0) = 0, so the masked cost is L of the masked controls, summed in array order
            ell = fns_dict.numerical_L_fn(tuple(ak * kk[:, None] for ak, kk in zip(a, keep)), x_in, t)
            running = running + dt * ell
        x_final = traj_x[T]
        term = _phi_at(phi[0], x_final, ndim, x1, x2, x_period, y_period, bc, center) if terminal == "phi0" \
            else np.zeros_like(running)
        d = policy_report_from_samples(running, term, value)
    d.update(running=running, terminal=term, value=value, x_final=x_final)
    return d


def format_policy(d):
    """One line: the closed-loop cost against the value of a policy dict."""
    return ("policy gap (cost - value) mean {gap_mean:+.3e} |.| mean {gap_abs_mean:.3e} rms {gap_rms:.3e} max "
            "{gap_abs_max:.3e} in [{gap_lo:+.3e}, {gap_hi:+.3e}]; cost {cost_mean:.6e} = running {running_mean:.6e} + "
            "terminal {terminal_mean:.6e}, value {value_mean:.6e}; {n_nonfinite} of {n_sample} samples "
            "non-finite").format(**d)


def run_policy_check(ctx, egno, ndim, x_period, y_period, epsl, n, seed=0):
    """The policy check from run_example's trajectory starts (trajectories.trajectory_samples), with the method and
    centring run_trajectories_device chooses; with epsl > 0 the device noise stream keyed by `seed`.  Returns the
    report dict (no per-sample arrays)."""
    x0 = TR.trajectory_samples(egno, ndim, n, x_period, y_period, epsl)
    method = "nearest" if egno == 2 else "linear"
    center = (egno == 3, egno == 3)
    return ctx.policy_eval(x0, method=method, x_period=x_period, y_period=y_period if ndim == 2 else None,
                           center=center, seed=seed, outputs=())
