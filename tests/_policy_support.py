"""Shared pieces of the policy-check tests: a per-sample restatement of pdhg_policy_eval's definition
(include/pdhg.h) on the trajectory oracle, and the summation bound of its statistics."""
import numpy as np

import traj_oracle as TO

import _traj_support as S

STATS_SUM = {"running_mean": "running", "terminal_mean": "terminal", "value_mean": "value", "cost_mean": "cost",
             "gap_mean": "gap", "gap_abs_mean": "gap_abs"}


def lag(egno, a):
    """L of one control component (set_fns.py:26-49): a^2 / 2, or the indicator's 0 a^2 of egno 2."""
    return 0.0 * (a * a) if egno == 2 else (a * a) / 2


def _phi_lin(P, row, pos_all, x):
    """Linear interpolation of one phi row at one position with the rollout's extension (pos_all: the positions the
    extended grid has to cover)."""
    if P["ndim"] == 1:
        return TO.interp_periodic(float(x), P["xs"], row, S.P_SPACE)
    lo, hi = pos_all.min(axis=0), pos_all.max(axis=0)
    e1 = TO.VirtualExtension(P["xs"], lo[0], hi[0], S.P_SPACE, P["bc"][0], P["center"][0])
    e2 = TO.VirtualExtension(P["ys"], lo[1], hi[1], S.P_SPACE, P["bc"][1], P["center"][1])
    return float(TO.interp2(row[..., None], e1, e2, x[0], x[1], "linear")[0])


def oracle_policy(P, phi, alp, x0, epsl, method, noise, terminal):
    """The definition sample by sample.  The positions are traj_oracle's rollout; every control array is interpolated
    again at them (as _traj_support.assert_margins does) for its f, its side of the sign split and its cost; phi is
    interpolated with the same linear routines.  terminal: "phi0" or "none".  Returns a dict of running, terminal,
    value [n], x_final and traj_x (for assert_margins)."""
    phi, alp = np.asarray(phi, dtype=np.float64), np.asarray(alp, dtype=np.float64)
    T, ndim, egno, dt = alp.shape[1], P["ndim"], P["egno"], P["dt"]
    _, traj_x = S.oracle_traj(P, alp, x0, epsl, method, noise)
    alp_c = alp[:, ::-1]
    pos = np.asarray(traj_x).reshape(T + 1, -1, ndim)
    n = pos.shape[1]
    running, term, value = np.zeros(n), np.zeros(n), np.zeros(n)
    for s in range(n):
        value[s] = _phi_lin(P, phi[T], pos[0], pos[0, s] if ndim == 2 else pos[0, s, 0])
        run = 0.0
        for ind in range(T):
            if ndim == 1:
                x = pos[ind, s, 0]
                if method == "linear":
                    a = [TO.interp_periodic(x, P["xs"], alp_c[k, ind, :, 0], S.P_SPACE) for k in range(2)]
                else:
                    j = TO.nearest_index(x, P["xs"], S.P_SPACE)
                    a = [alp_c[k, ind, j, 0] for k in range(2)]
                xm = np.array([[x % S.P_SPACE]])
                f = [float(P["f_fn"](np.array([[v]]), xm, 0.0)[0, 0]) for v in a]
            else:
                x, y = pos[ind, s]
                lo, hi = pos[ind].min(axis=0), pos[ind].max(axis=0)
                e1 = TO.VirtualExtension(P["xs"], lo[0], hi[0], S.P_SPACE, P["bc"][0], P["center"][0])
                e2 = TO.VirtualExtension(P["ys"], lo[1], hi[1], S.P_SPACE, P["bc"][1], P["center"][1])
                c = [TO.interp2(alp_c[k, ind], e1, e2, x, y, method) for k in range(2 if egno == 3 else 4)]
                xin = np.array([[x % S.P_SPACE if P["bc"][0] == 0 else x, y % S.P_SPACE]])
                f = [float(P["f_fn"](c[k][None, :], xin, 0.0)[0, 0 if k < 2 else 1]) for k in range(len(c))]
                a = [float(c[k][0 if k < 2 else 1]) for k in range(len(c))]   # the live component of array k
            ell = 0.0
            for k, (ak, fk) in enumerate(zip(a, f)):
                keep = (fk >= 0.0) if k % 2 == 0 else (fk < 0.0)
                ell = ell + (1.0 if keep else 0.0) * lag(egno, float(ak))
            run = run + dt * ell
        running[s] = run
        if terminal == "phi0":
            term[s] = _phi_lin(P, phi[0], pos[T], pos[T, s] if ndim == 2 else pos[T, s, 0])
    return dict(running=running, terminal=term, value=value, x_final=np.asarray(traj_x)[-1], traj_x=traj_x)


def random_phi(P, T=None):
    """A random phi so that both interpolated rows discriminate."""
    T = P["T"] if T is None else T
    sp = (P["nx"],) if P["ndim"] == 1 else (P["nx"], P["ny"])
    return np.random.default_rng(5).standard_normal((T + 1,) + sp)


def load_state(ctx, phi, alp):
    """The given phi and controls with rho = 1: nothing but the policy check runs."""
    ctx.set_state(phi, np.ones(alp.shape[1:-1]), tuple(alp))


def sample_terms(running, terminal, value):
    """The finite samples' terms of every summed statistic, as policy_report_from_samples forms them."""
    running, terminal, value = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (running, terminal, value))
    ok = np.isfinite(running) & np.isfinite(terminal) & np.isfinite(value)
    r, t, v = running[ok], terminal[ok], value[ok]
    cost = r + t
    gap = cost - v
    return dict(running=r, terminal=t, value=v, cost=cost, gap=gap, gap_abs=np.abs(gap), gap_sq=gap * gap)


def assert_report_matches_fold(rep, running, terminal, value):
    """A device report against the host fold of the per-sample arrays it came with.  Counts and extrema are exact.
    Two fp64 summations of the same n terms in different orders are each within (n - 1) 2^-53 sum |x_i| of the exact
    sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, to first order), so the means differ by at
    most 2 n 2^-53 sum |x_i| / n; gap_rms is compared through its square: the division, the square root and squaring it
    back round three times, (1 + 2^-53)^3 on each side, so 8 2^-53 relative covers both sides."""
    from pdhg_amd.policy import policy_report_from_samples
    want = policy_report_from_samples(running, terminal, value)
    for k in ("n_sample", "n_nonfinite", "gap_abs_max", "gap_lo", "gap_hi"):
        assert rep[k] == want[k], (k, rep[k], want[k])
    terms = sample_terms(running, terminal, value)
    n = terms["gap"].size
    assert n == want["n_sample"] - want["n_nonfinite"] and n > 0
    for k, name in STATS_SUM.items():
        bound = 2 * n * 2.0 ** -53 * float(np.abs(terms[name]).sum()) / n
        print("{}: device {!r} host {!r} |diff| {:.3e} (bound {:.3e})".format(k, rep[k], want[k],
                                                                              abs(rep[k] - want[k]), bound))
        assert abs(rep[k] - want[k]) <= bound, (k, rep[k], want[k], bound)
    bound = 2 * n * 2.0 ** -53 * float(terms["gap_sq"].sum()) / n + 8 * 2.0 ** -53 * want["gap_rms"] ** 2
    diff = abs(rep["gap_rms"] ** 2 - want["gap_rms"] ** 2)
    print("gap_rms^2: |diff| {:.3e} (bound {:.3e})".format(diff, bound))
    assert diff <= bound, (rep["gap_rms"], want["gap_rms"], bound)
