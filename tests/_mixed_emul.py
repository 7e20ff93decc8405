"""CPU emulation of the mixed-precision context (precision 12) on the float64 oracle, at a test's own shape.

The oracle (oracle/pdhg_oracle.py) is NumPy code that computes in the dtype of its inputs, so holding chosen
quantities in float32 emulates a device arithmetic -- the method of tests/golden/precision_study.py:
  mixed  phi and phi_bar float64, their finite differences (Dx / Dy one-sided, Dxx, Dyy, Dt) formed in float64 and
         rounded to float32 once; rho, alp, the residual, the preconditioner (FFTs + Thomas) and the grid float32;
         phi' = phi + tau U with U float32 widened (precision_study's "phi64")
  f32    everything float32 (complex64 FFTs and Thomas)
  f64    the oracle as it is
The oracle module is patched only inside `patched()` and always restored; it is imported, never edited.

run(P, variant, ...) runs outer iterations (one primal, one dual of k sub-iterations); errors(P, ...) gives
e_mixed and e32: the relative L2 distances of the two emulations from the float64 run, per quantity.
"""
import contextlib

import numpy as np

import pdhg_oracle as O
from _problems import oracle_fns, rel

F32, F64 = np.float32, np.float64
TAU, SIGMA = 0.1 / 1.5, 0.1 * 1.5
_PHI_DIFFS = ["Dx_right_decreasedim", "Dx_left_decreasedim", "Dy_right_decreasedim", "Dy_left_decreasedim",
              "Dxx_decreasedim", "Dyy_decreasedim", "Dt_decreasedim"]


@contextlib.contextmanager
def patched(variant):
    """mixed: the oracle's differences of phi_bar return float32 (formed in the float64 of their argument)."""
    orig = {n: getattr(O, n) for n in _PHI_DIFFS}
    try:
        if variant == "mixed":
            for n, f in orig.items():
                setattr(O, n, (lambda f: lambda phi, *a: f(phi, *a).astype(F32))(f))
        yield
    finally:
        for n, f in orig.items():
            setattr(O, n, f)


def live(P, alp):
    """The stored component of each control array (the dead ones are identically zero)."""
    if P["ndim"] == 1 or P["egno"] == 3:
        return [np.asarray(a)[..., 0] for a in alp[:2]]
    return [np.asarray(a)[..., 0 if i < 2 else 1] for i, a in enumerate(alp)]


def start_state(P, variant, phi=None, rho=None, alp=None):
    """The state as the variant's context holds it after set_state: mixed keeps phi, rounds rho / alp to float32."""
    phi = P["phi"] if phi is None else phi
    rho = P["rho"] if rho is None else rho
    alp = P["alp"] if alp is None else alp
    if variant == "f64":
        return phi.astype(F64), rho.astype(F64), tuple(a.astype(F64) for a in alp)
    return (phi.astype(F64 if variant == "mixed" else F32), rho.astype(F32), tuple(a.astype(F32) for a in alp))


def run(P, variant, iters, k=1, eps=-1.0, state=None, tau=TAU, sigma=SIGMA, inner=None, keep=(), first_u=None):
    """`iters` outer iterations from `state` (default: P's); returns (phi, rho, alp) as float64 arrays -- with
    keep = (i, ...) a dict of them after those iteration counts instead.
    inner: a list that receives the dual sub-iteration count of every outer iteration.
    first_u: a list that receives U1 = (phi1 - phi0) / tau of the first primal update (float64), formed as a test
    forms it from a context's phi before and after update_primal."""
    primal, dual = oracle_fns(P, rho_alp_iters=k, stats=inner)
    phi, rho, alp = start_state(P, variant, *(state or ()))
    lo = F64 if variant == "f64" else F32
    x_arr = P["x_arr"].astype(lo)
    out = {}
    with patched(variant):
        for i in range(iters):
            u = primal(phi, rho, 70.0, alp, tau, P["dt"], P["dsp"], P["fns"], P["fv"], P["epsl"], x_arr, None)
            phi_n = u.astype(phi.dtype)
            if i == 0 and first_u is not None:
                first_u.append((phi_n.astype(F64) - phi.astype(F64)) / tau)
            rho, alp = dual(2 * phi_n - phi, rho, 70.0, alp, sigma, P["dt"], P["dsp"], P["epsl"], P["fns"], x_arr,
                            None, P["ndim"], eps)
            rho, alp = rho.astype(lo), tuple(a.astype(lo) for a in alp)
            phi = phi_n
            if i + 1 in keep or i + 1 == iters:
                out[i + 1] = (phi.astype(F64), rho.astype(F64), tuple(a.astype(F64) for a in alp))
    return out if keep else out[iters]


def errors(P, iters, k=1, eps=-1.0, state=None, f32=True, u1=None):
    """(ref, e_mixed, e32): the float64 run's (phi, rho, alp) and, per quantity ("phi", "rho", "alp0" ..), the relative
    L2 distance of the mixed and of the all-float32 emulation from it after `iters` iterations.  iters a tuple: one
    run to its largest count, and a dict {count: (ref, e_mixed, e32)}.
    f32 = False leaves the all-float32 run out (e32 is None then: a check that does not read it saves a third of
    the time).  u1: a dict that receives the first primal update, "ref" (the float64 run's U1) and "e_mixed" (the
    mixed emulation's relative L2 distance from it)."""
    counts = tuple(iters) if isinstance(iters, (tuple, list)) else (iters,)
    variants = ("f64", "mixed") + (("f32",) if f32 else ())
    first = {v: [] for v in variants}
    runs = {v: run(P, v, max(counts), k, eps, state, keep=counts, first_u=first[v]) for v in variants}
    if u1 is not None:
        u1["ref"] = first["f64"][0]
        u1["e_mixed"] = rel(first["mixed"][0], first["f64"][0])
    res = {}
    for n in counts:
        ref = runs["f64"][n]
        out = []
        for variant in variants[1:]:
            r = runs[variant][n]
            e = {"phi": rel(r[0], ref[0]), "rho": rel(r[1], ref[1])}
            for a, (x, y) in enumerate(zip(live(P, r[2]), live(P, ref[2]))):
                e["alp{}".format(a)] = rel(x, y)
            out.append(e)
        res[n] = (ref, out[0], out[1] if f32 else None)
    return res if isinstance(iters, (tuple, list)) else res[iters]
