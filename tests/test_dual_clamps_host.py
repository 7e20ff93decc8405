"""The reference side of the dual-step clamp tests, without a device (tests/_dual_support.py).

1. update_dual_oneiter (the float64 oracle, update_fns_in_pdhg.py:150-165) at the clamp state against a per-point
   restatement of the formulas in np.longdouble, written with explicit index arithmetic (none of the oracle's
   difference operators): every output point within 8 * 2^-53 * S.  1-D and 2-D; egno 1, 2, 3; bc 0 and (1, 0);
   T = 1 and T > 1; epsl 0 and 0.1.
2. The conditions of every case test_gpu_dual_clamps.py runs: every branch class of the reference state (rho
   projected / kept, every live control masked / kept, egno 2's controls clipped low / clipped high / interior) holds
   >= 5 % of the points, and <= 1 % of an array's points lie within the margin K r 2^-24 S of a threshold.
"""
import numpy as np
import pytest

import _dual_support as D
from _problems import make_problem

L = np.longdouble

PIN = [
    # egno, ndim, nx, ny, T, epsl
    (1, 1, 16, 1, 1, 0.0), (2, 1, 17, 1, 4, 0.1), (1, 1, 17, 1, 3, 0.1), (2, 1, 16, 1, 1, 0.0),
    (1, 2, 16, 12, 1, 0.1), (2, 2, 15, 17, 3, 0.1), (2, 2, 16, 12, 1, 0.0), (1, 2, 15, 17, 2, 0.0),
    (3, 2, 16, 12, 3, 0.1), (3, 2, 15, 17, 1, 0.0),
]
IDS = ["e{}d{}_{}x{}_T{}_eps{}".format(*c) for c in PIN]


def _nb(i, n, bc):
    """Index of the neighbour i of an axis of length n (periodic wrap), or None outside a Neumann edge."""
    if 0 <= i < n:
        return i
    return i % n if bc == 0 else None


def restate(P, rho, alp, phi_bar, sigma):
    """(rho', live controls) of one dual step, point by point in np.longdouble from the formulas of
    update_fns_in_pdhg.py:99-133 / :58-70 and set_fns.py:63-160."""
    egno, ndim, T = P["egno"], P["ndim"], P["T"]
    nx, ny = P["nx"], (P["ny"] if ndim == 2 else 1)
    bcx, bcy = (P["bc"], 0) if ndim == 1 else P["bc"]
    dx, dt, epsl, sg = L(P["dsp"][0]), L(P["dt"]), L(P["epsl"]), L(sigma)
    dy = L(P["dsp"][1]) if ndim == 2 else L(1)
    pb = phi_bar.reshape(T + 1, nx, ny).astype(L)
    rh = rho.reshape(T, nx, ny).astype(L)
    comps = D.live_components(P)
    al = [alp[k][..., c].reshape(T, nx, ny).astype(L) for k, c in enumerate(comps) if c is not None]
    xs = np.asarray(P["xs"], dtype=L)
    ys = np.asarray(P["ys"], dtype=L) if ndim == 2 else None
    rho_n = np.zeros((T, nx, ny), dtype=L)
    alp_n = [np.zeros((T, nx, ny), dtype=L) for _ in al]
    for j in range(T):
        for x in range(nx):
            for y in range(ny):
                c = pb[j + 1, x, y]
                xp, xm = _nb(x + 1, nx, bcx), _nb(x - 1, nx, bcx)
                DxR = (pb[j + 1, xp, y] - c) / dx if xp is not None else L(0)
                DxL = (c - pb[j + 1, xm, y]) / dx if xm is not None else L(0)
                # Dxx: the Neumann edge mirrors the point itself
                lap = (pb[j + 1, x if xp is None else xp, y] + pb[j + 1, x if xm is None else xm, y] - 2 * c) / dx ** 2
                diffs = [DxR, DxL]
                if ndim == 2:
                    yp, ym = _nb(y + 1, ny, bcy), _nb(y - 1, ny, bcy)
                    diffs += [(pb[j + 1, x, yp] - c) / dy, (c - pb[j + 1, x, ym]) / dy]
                    lap = lap + (pb[j + 1, x, yp] + pb[j + 1, x, ym] - 2 * c) / dy ** 2
                p = (rh[j, x, y] + L(1e-4)) / sg
                hj, lag = L(0), L(0)
                for k in range(len(al)):
                    d, old, right = diffs[k], al[k][j, x, y], k % 2 == 0
                    if egno == 3:
                        n = (-d + p * old) / (1 + p)
                        f = n
                    else:
                        a = ((xs[x] if k < 2 else ys[y]) - 1) ** 2 + L(0.1)
                        if egno == 1:
                            n = (d * a + p * old) / (1 + p)
                        else:
                            n = min(L(1), max(L(-1), d * a / p + old))
                        f = -a * n
                    if not (f >= 0 if right else f < 0):
                        n, f = L(0), L(0)
                    alp_n[k][j, x, y] = n
                    hj = hj + d * f
                    if egno != 2:
                        lag = lag + n * n / 2
                if egno == 3:   # f_y is the x coordinate: its positive part on DyR, its negative part on DyL
                    hj = hj + diffs[2] * max(xs[x], L(0)) + diffs[3] * min(xs[x], L(0))
                vec = (c - pb[j, x, y]) / dt - epsl * lap - hj - lag
                rho_n[j, x, y] = max(rh[j, x, y] + sg * vec, L(0))
    shape = rho.shape
    return rho_n.reshape(shape), [a.reshape(shape) for a in alp_n]


@pytest.mark.parametrize("case", PIN, ids=IDS)
def test_oracle_dual_step_pinned_to_longdouble_restatement(case):
    assert np.finfo(L).eps < 1e-18, "np.longdouble carries no more than float64 here"
    P = make_problem(*case)
    rho, alp, phi_bar = D.clamp_state(P)
    ref = D.reference(P, rho, alp, phi_bar)
    rho_l, alp_l = restate(P, rho, alp, phi_bar, D.SIGMA)
    worst = {"rho": float(np.max(np.abs(ref["rho"] - rho_l) / (D.U64 * ref["S_rho"])))}
    for i, (o, a_l, S) in enumerate(zip(ref["alp"], alp_l, ref["S_alp"])):
        worst["alp{}".format(i)] = float(np.max(np.abs(o - a_l) / (D.U64 * S)))
    print(case, worst)
    assert max(worst.values()) <= 8.0, worst
    # the restatement takes the same branches where the oracle decides by a margin
    sh = D.branch_shares(P, ref)
    assert abs(float(np.mean(rho_l == 0)) - sh["rho_projected"]) <= 0.01


def gpu_cases():
    """(egno, ndim, nx, ny, T, epsl) of every case of test_gpu_dual_clamps.py, once each."""
    import test_gpu_dual_clamps as G
    return sorted(set(G.all_problem_cases()))


@pytest.mark.parametrize("case", gpu_cases(), ids=lambda c: "e{}d{}_{}x{}_T{}_eps{}".format(*c))
def test_gpu_cases_fire_every_branch(case):
    """The reference state of every GPU case: the branch shares and the margin cap (with the float32 margin, the
    widest), as the GPU tests assert again before they compare."""
    P = make_problem(*case)
    rho, alp, phi_bar = D.clamp_state(P)
    r = D.calibrate(P, rho, alp, phi_bar)
    ref = D.reference(P, *D.round_inputs("fp32", rho, alp, phi_bar))
    sh, ms = D.assert_conditions(P, ref, r, D.U32)
    print(case, "r = {:.2f}".format(r), sh, ms)
    assert 0.0 < r < np.inf
