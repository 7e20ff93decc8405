"""Shared pieces of the dual-step clamp tests (test_dual_clamps_host.py, test_gpu_dual_clamps.py).

The dual step (update_fns_in_pdhg.py:150-165) holds three non-smooth operations: the projection
rho' = max(rho + sigma vec, 0), egno 2's clip of the control to [-1, 1] and the sign masks of the controls.  From
make_problem's seeded state only the masks fire.  clamp_state() is a state from which every branch fires at a fixed
share of the points; reference() runs the float64 oracle on it and returns, next to the oracle's outputs, the values
the oracle decided on (before the projection, the clip and the mask) and the point-wise scale S of every output.

All three operations are continuous (n [n <= 0] = min(n, 0)), so a point-wise bound holds at every point:
|d - o64| <= K r u S, with u the unit roundoff of the device's precision, S the output's formula with every term
replaced by its absolute value and every difference by the sum of absolute values, r the float32 oracle's own
largest |o32 - o64| / (2^-24 S) on the same case (calibrate) and K = 4 (the project's K32).  Where the reference
decides by more than m = K r u S the device's value is checked exactly (check_device).
"""
import numpy as np

import pdhg_oracle as O

SIGMA = 0.1 * 1.5
TAU = 0.1 / 1.5
SEED = 11
K = 4.0
U32, U64 = 2.0 ** -24, 2.0 ** -53
MIN_SHARE = 0.05     # every branch class of the reference state holds at least this share of the points
MAX_MARGIN = 0.01    # at most this share of an array's points within m of a threshold


def live_components(P):
    """Per control array: the index of its live component, None for a dead array (egno 3's y controls)."""
    if P["ndim"] == 1:
        return [0, 0]
    return [0, 0, None, None] if P["egno"] == 3 else [0, 0, 1, 1]


def clamp_state(P, seed=SEED):
    """(rho, alp, phi_bar), float64, a function of P's shapes and P["phi"] only.
    rho: 25 % exactly 0, 25 % 10^U(-6, 0), the rest 70 U(0.5, 1.5); every live control component 1.5 N(0, 1), the dead
    ones exactly 0; phi_bar = phi + 0.5 min(1, 64 min(dx, dy)) N(0, 1)."""
    rng = np.random.default_rng(seed)
    shape = P["rho"].shape
    cls = rng.uniform(size=shape)
    small = 10.0 ** rng.uniform(-6.0, 0.0, shape)
    big = 70.0 * rng.uniform(0.5, 1.5, shape)
    rho = np.where(cls < 0.25, 0.0, np.where(cls < 0.5, small, big))
    alp = [np.zeros_like(a) for a in P["alp"]]
    for a, comp in zip(alp, live_components(P)):
        if comp is not None:
            a[..., comp] = 1.5 * rng.standard_normal(shape)
    # the noise's one-sided differences are ~ amp / dx: beyond 1 / dx = 64 the amplitude follows dx, or egno 2 would
    # clip all but 1.6 % of the controls at nx = 65536 (D a / p ~ 50 even at rho = 70) and leave no interior class
    amp = 0.5 * min(1.0, 64.0 * min(P["dsp"]))
    phi_bar = P["phi"] + amp * rng.standard_normal(P["phi"].shape)
    return rho, tuple(alp), phi_bar


def round_inputs(prec, rho, alp, phi_bar):
    """The state as the device of this precision holds it, as float64 arrays: fp32 rounds everything to float32,
    mixed everything but phi_bar, fp64 nothing."""
    r32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    if prec == "fp64":
        return rho, tuple(alp), phi_bar
    return r32(rho), tuple(r32(a) for a in alp), (phi_bar if prec == "mixed" else r32(phi_bar))


def oracle_step(P, rho, alp, phi_bar, sigma=SIGMA, dtype=np.float64):
    """update_dual_oneiter executed in dtype (every input cast first): (rho', alp', err)."""
    f = dtype
    rho_n, alp_n, err = O.update_dual_oneiter(phi_bar.astype(f), rho.astype(f), 70.0, tuple(a.astype(f) for a in alp),
                                              sigma, P["dt"], P["dsp"], P["epsl"], P["x_arr"].astype(f), None, P["bc"],
                                              P["fns"], P["ndim"])
    assert rho_n.dtype == f and all(a.dtype == f for a in alp_n)
    return rho_n, alp_n, err


# ---- |.| forms of the oracle's difference operators (rows 1.. of phi_bar, as the *_decreasedim operators)
def _abs_first(A, d, bc, axis, right):
    """(|p[i+1]| + |p[i]|) / d (right) or (|p[i]| + |p[i-1]|) / d (left); 0 where a Neumann edge takes no difference."""
    if bc == 0:
        return (np.roll(A, -1 if right else 1, axis=axis) + A) / d
    assert bc == 1
    s = O._take(A, slice(1, None), axis) + O._take(A, slice(None, -1), axis)
    z = O._zeros_like_slice(A, axis)
    return np.concatenate([s, z] if right else [z, s], axis=axis) / d


def _abs_second(A, d, bc, axis):
    """(|p[i+1]| + |p[i-1]| + 2 |p[i]|) / d^2, the Neumann edge mirrored as Dxx's."""
    if bc == 0:
        ip1, im1 = np.roll(A, -1, axis=axis), np.roll(A, 1, axis=axis)
    else:
        assert bc == 1
        ip1 = np.concatenate([O._take(A, slice(1, None), axis), O._take(A, slice(-1, None), axis)], axis=axis)
        im1 = np.concatenate([O._take(A, slice(0, 1), axis), O._take(A, slice(None, -1), axis)], axis=axis)
    return (ip1 + im1 + 2 * A) / d ** 2


def _controls(P):
    """Per live control: (array index, component, axis of its difference, right?, coefficient a [1, nx(, ny)])."""
    x = P["x_arr"]
    if P["ndim"] == 1:
        ax = (x[..., 0] - 1.0) ** 2 + 0.1
        return [(0, 0, 1, True, ax), (1, 0, 1, False, ax)]
    if P["egno"] == 3:
        one = np.ones_like(x[..., 0])
        return [(0, 0, 1, True, one), (1, 0, 1, False, one)]
    ax = (x[..., 0] - 1.0) ** 2 + 0.1
    ay = (x[..., 1] - 1.0) ** 2 + 0.1
    return [(0, 0, 1, True, ax), (1, 0, 1, False, ax), (2, 1, 2, True, ay), (3, 1, 2, False, ay)]


def reference(P, rho, alp, phi_bar, sigma=SIGMA):
    """The float64 oracle's dual step of (rho, alp, phi_bar) and what it decided on.  A dict:
      rho, alp (the live component of every live control, a list), err   -- update_dual_oneiter's outputs
      alp_full      the oracle's whole control arrays (the dead components included)
      rho_pre       rho + sigma vec, before the projection
      pre           per live control: the value before the clip (egno 2) or before the mask
      n, keep       per live control: the value the mask multiplies (after the clip) and the mask
      drop_sign     per live control: +1 / -1, the sign of n on the dropped side of its mask
      S_rho, S_alp  the point-wise scales
    The decided-on values are formed with the oracle's own operators and asserted to reproduce its outputs."""
    egno, ndim, bc = P["egno"], P["ndim"], P["bc"]
    bcs = (bc,) if ndim == 1 else tuple(bc)
    rho_o, alp_o, err = oracle_step(P, rho, alp, phi_bar, sigma)
    pb1 = phi_bar[1:]
    p = (rho + 1e-4) / sigma
    D = {(1, True): O.Dx_right_decreasedim(phi_bar, P["dsp"][0], bcs[0]),
         (1, False): O.Dx_left_decreasedim(phi_bar, P["dsp"][0], bcs[0])}
    if ndim == 2:
        D[(2, True)] = O.Dy_right_decreasedim(phi_bar, P["dsp"][1], bcs[1])
        D[(2, False)] = O.Dy_left_decreasedim(phi_bar, P["dsp"][1], bcs[1])
    A1 = np.abs(pb1)
    Dabs = {(ax, rt): _abs_first(A1, P["dsp"][ax - 1], bcs[ax - 1], ax, rt) for (ax, rt) in D}
    out = dict(rho=rho_o, err=err, alp_full=alp_o, alp=[], pre=[], n=[], keep=[], drop_sign=[], S_alp=[])
    with np.errstate(invalid="ignore"):
        for k, comp, axis, right, a in _controls(P):
            d, da, old = D[(axis, right)], Dabs[(axis, right)], alp[k][..., comp]
            if egno == 1:
                pre = (d * a + p * old) / (1 + p)
                n, f, S = pre, -(a * pre), (da * a + p * np.abs(old)) / (1 + p)
            elif egno == 2:
                pre = d * a / p + old
                n = np.minimum(1.0, np.maximum(-1.0, pre))
                f, S = -(a * n), da * a / p + np.abs(old)
            else:
                pre = (-d + p * old) / (1 + p)
                n, f, S = pre, pre, (da + p * np.abs(old)) / (1 + p)
            keep = (f >= 0.0) if right else (f < 0.0)
            got = alp_o[k][..., comp]
            assert np.array_equal(n * keep, got, equal_nan=True), "control {}: not the oracle's value".format(k)
            out["alp"].append(got)
            out["pre"].append(pre)
            out["n"].append(n)
            out["keep"].append(keep)
            # kept side of alp1: f >= 0, of alp2: f < 0; f = -a n (a > 0) for egno 1 / 2, f = n for egno 3
            out["drop_sign"].append((1.0 if right else -1.0) * (-1.0 if egno == 3 else 1.0))
            out["S_alp"].append(S)
        # rho: the oracle's HJ residual at its own alp'
        hj = O.compute_HJ_residual_1d if ndim == 1 else O.compute_HJ_residual_2d
        out["rho_pre"] = rho + sigma * hj(phi_bar, alp_o, P["dt"], P["dsp"], P["fns"], P["epsl"], P["x_arr"], None, bc)
        assert np.array_equal(np.maximum(out["rho_pre"], 0.0), rho_o, equal_nan=True)
        if ndim == 1:
            fs = O.get_f_vals_1d(P["fns"].f_fn, alp_o, P["x_arr"], None)
            keys = [(1, True), (1, False)]
        else:
            fs = O.get_f_vals_2d(P["fns"].f_fn, alp_o, P["x_arr"], None)
            keys = [(1, True), (1, False), (2, True), (2, False)]
        S = (A1 + np.abs(phi_bar[:-1])) / P["dt"]
        for ax in range(1, ndim + 1):
            S = S + P["epsl"] * _abs_second(A1, P["dsp"][ax - 1], bcs[ax - 1], ax)
        for key, f in zip(keys, fs):
            S = S + Dabs[key] * np.abs(f)
        S = S + P["fns"].numerical_L_fn(alp_o, P["x_arr"], None)
        out["S_rho"] = np.abs(rho) + sigma * S
    return out


def _ratio(diff, S, u):
    """|diff| / (u S) over the points where the reference is finite (0 where S = 0 = diff)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(diff) / (u * S)
    q = np.where((S == 0) & (diff == 0), 0.0, q)
    return q


def calibrate(P, rho, alp, phi_bar, sigma=SIGMA):
    """r: the largest |o32 - o64| / (2^-24 S) over points and arrays, both oracles on the float32-rounded state."""
    r_rho, r_alp, r_pb = round_inputs("fp32", rho, alp, phi_bar)
    ref = reference(P, r_rho, r_alp, r_pb, sigma)
    rho32, alp32, _ = oracle_step(P, r_rho, r_alp, r_pb, sigma, np.float32)
    qs = [_ratio(rho32.astype(np.float64) - ref["rho"], ref["S_rho"], U32)]
    for (k, comp, _, _, _), o, S in zip(_controls(P), ref["alp"], ref["S_alp"]):
        qs.append(_ratio(alp32[k][..., comp].astype(np.float64) - o, S, U32))
    fin = [q[np.isfinite(q)] for q in qs]
    return float(max(q.max() for q in fin if q.size))


def margins(P, ref, r, u):
    """Per array ("rho", "alp0", ...): the boolean array of the points within m = K r u S of a threshold."""
    out = {}
    with np.errstate(invalid="ignore"):
        out["rho"] = np.abs(ref["rho_pre"]) <= K * r * u * ref["S_rho"]
        for i, (pre, n, S) in enumerate(zip(ref["pre"], ref["n"], ref["S_alp"])):
            m = K * r * u * S
            near = np.abs(pre) <= m       # the mask decides on the sign of n, which is the sign of pre (see check_device)
            if P["egno"] == 2:
                near = near | (np.abs(pre - 1.0) <= m) | (np.abs(pre + 1.0) <= m)
            out["alp{}".format(i)] = near
    return out


def margin_share(P, ref, r, u):
    return {k: float(np.mean(v)) for k, v in margins(P, ref, r, u).items()}


def branch_shares(P, ref):
    """Share of the points in every branch class that exists for the egno, from the float64 oracle alone."""
    sh = {"rho_projected": float(np.mean(ref["rho"] == 0.0)), "rho_kept": float(np.mean(ref["rho"] > 0.0))}
    for i, keep in enumerate(ref["keep"]):
        sh["alp{}_masked".format(i)] = float(np.mean(~keep))
        sh["alp{}_kept".format(i)] = float(np.mean(keep))
    if P["egno"] == 2:
        a = np.stack(ref["alp"])
        kept = np.stack(ref["keep"])
        sh["clip_low"] = float(np.mean(kept & (a == -1.0)))
        sh["clip_high"] = float(np.mean(kept & (a == 1.0)))
        sh["clip_interior"] = float(np.mean(kept & (np.abs(a) < 1.0)))
    return sh


def assert_conditions(P, ref, r, u=U32):
    """The conditions a case must meet to test anything: every branch class >= 5 % of the points, and <= 1 % of every
    array's points within a margin.  Returns (branch shares, margin shares)."""
    sh = branch_shares(P, ref)
    for k, v in sh.items():
        assert v >= MIN_SHARE, "branch class {} holds {:.3f} of the points: {}".format(k, v, sh)
    ms = margin_share(P, ref, r, u)
    for k, v in ms.items():
        assert v <= MAX_MARGIN, "{}: {:.4f} of the points within a margin".format(k, v)
    return sh, ms


def seam_mask(shape, rx=8, strip=256):
    """The seam points of the tiled kernels over [T, nx(, ny)]: first and last row of every rx-row tile, first and
    last column of every strip, time rows 0 and T - 1."""
    m = np.zeros(shape, dtype=bool)
    m[0] = m[-1] = True
    x = np.arange(shape[1])
    m[:, (x % rx == 0) | (x % rx == rx - 1)] = True
    if len(shape) == 3:
        y = np.arange(shape[2])
        m[:, :, (y % strip == 0) | (y % strip == strip - 1)] = True
    return m


def check_device(P, ref, r, u, rho_d, alp_d, seam=None, pointwise=True):
    """Holds the device's (rho', alp') to the reference: the NaN sets equal, |d - o| <= K r u S at every finite point,
    and the exact values where the reference decides by more than m = K r u S.  Returns the measured maxima of
    |d - o| / (u S) per array, over the seam and the interior points when a seam mask is given, and the failures; the
    caller logs the figures before it asserts.  pointwise = False (a state several steps from the reference's input):
    the NaN sets, the exact values and the dead components only."""
    comps = [(k, comp) for k, comp, _, _, _ in _controls(P)]
    dev = {"rho": rho_d}
    refs = {"rho": (ref["rho"], ref["S_rho"])}
    for i, (k, comp) in enumerate(comps):
        dev["alp{}".format(i)] = alp_d[k][..., comp]
        refs["alp{}".format(i)] = (ref["alp"][i], ref["S_alp"][i])
    measured, fails = {}, []
    for name, d in dev.items():
        o, S = refs[name]
        nan_o, nan_d = np.isnan(o), np.isnan(d)
        if not np.array_equal(nan_o, nan_d):
            fails.append("{}: NaN set differs ({} on the device, {} in the oracle)".format(name, nan_d.sum(), nan_o.sum()))
        q = _ratio(np.where(nan_o, 0.0, d - o), np.where(nan_o, 1.0, S), u)
        q = np.where(nan_o, 0.0, np.where(np.isnan(q), np.inf, q))
        measured[name] = float(q.max())
        if seam is not None:
            measured[name + "_seam"] = float(q[seam].max())
            measured[name + "_interior"] = float(q[~seam].max()) if (~seam).any() else 0.0
        if pointwise and not (q <= K * r).all():
            i = np.unravel_index(np.argmax(q), q.shape)
            fails.append("{}: |d - o| / (u S) = {:.3g} > K r = {:.3g} at {} (d {!r}, o {!r}, S {:.3g}); {} points over"
                         .format(name, q.max(), K * r, i, d[i], o[i], S[i], int((q > K * r).sum())))
    # exact values where the reference decides by a margin
    with np.errstate(invalid="ignore"):
        m = K * r * u * ref["S_rho"]
        sel = ref["rho_pre"] < -m
        if not (dev["rho"][sel] == 0.0).all():
            fails.append("rho: {} points projected by a margin are not 0".format(int((dev["rho"][sel] != 0.0).sum())))
        for i in range(len(comps)):
            d, pre, n, S = dev["alp{}".format(i)], ref["pre"][i], ref["n"][i], ref["S_alp"][i]
            m = K * r * u * S
            ds = ref["drop_sign"][i]
            # the mask decides on the sign of n; the clip keeps the sign, so that is the sign of pre, whose distance
            # from 0 is on S's scale (after the clip |n| <= 1 however large S = |D| a / p is on a fine grid)
            dropped = ds * pre > m
            kept = ds * pre < -m
            if not (d[dropped] == 0.0).all():
                fails.append("alp{}: {} points masked by a margin are not 0".format(i, int((d[dropped] != 0.0).sum())))
            if P["egno"] == 2:
                hi, lo = kept & (pre > 1.0 + m), kept & (pre < -1.0 - m)
                if not (d[hi] == 1.0).all():
                    fails.append("alp{}: {} points clipped high by a margin are not 1".format(i, int((d[hi] != 1.0).sum())))
                if not (d[lo] == -1.0).all():
                    fails.append("alp{}: {} points clipped low by a margin are not -1".format(i, int((d[lo] != -1.0).sum())))
    # the dead components are exactly 0.  The device stores the live ones only and get_state fills in zeros; the
    # oracle's dead component is 0 * D + p * 0, a NaN where D or p is one -- and there the same array's live component
    # is a NaN too (asserted), so the control's set of NaN points, compared above, is the same either way
    for k, comp in enumerate(live_components(P)):
        for c in range(alp_d[k].shape[-1]):
            if c == comp:
                continue
            o = ref["alp_full"][k][..., c]
            assert ((o == 0.0) | np.isnan(o)).all()
            if comp is not None:
                assert not (np.isnan(o) & ~np.isnan(ref["alp_full"][k][..., comp])).any()
            if not (alp_d[k][..., c] == 0.0).all():
                fails.append("alp[{}][..., {}]: dead component is not 0".format(k, c))
    return measured, fails

