"""Shared pieces of the 2-D preconditioner parameter tests (test_precond2d_host.py, test_gpu_precond2d.py):
the per-mode error measure, the continuity residual of a problem, and H1_precond_2d with its t-solve in
np.longdouble."""
import numpy as np
import scipy.fft as sfft

import pdhg_oracle as O

TAU = 0.1 / 1.5


def spectrum(U, bc):
    """Rows 1..T of U = (phi' - phi) / tau in the basis the preconditioner solves in: fft2 over (x, y) for bc (0, 0),
    the DCT-II along x and the FFT along y for bc (1, 0), as H1_precond_2d transforms its source."""
    U = np.asarray(U, dtype=np.float64)[1:]
    if tuple(bc) == (0, 0):
        return sfft.fft2(U, axes=(1, 2))
    return sfft.fft(sfft.dct(U, axis=1), axis=2)


def per_mode(U_dev, U_ref, bc):
    """max over modes m of e[m] / (n[m] + median n): e[m] the L2 norm over the time rows of the spectra's difference,
    n[m] that of the reference spectrum.  The relative L2 norm of U is dominated by the low modes (the zero mode alone
    carries 1 % - 99 % of max |U| on 64 x 16); this measure weighs every mode by its own size.  The median is the floor:
    from the seeded rough state the residual spectrum is flat, so it sits at a high mode's small gain."""
    S_ref = spectrum(U_ref, bc)
    e = np.linalg.norm(spectrum(U_dev, bc) - S_ref, axis=0)
    n = np.linalg.norm(S_ref, axis=0)
    return float(np.max(e / (n + np.median(n))))


def residual(P):
    """The primal update's source term (the continuity residual, [T + 1, nx, ny]) of the problem's state."""
    return O.compute_cont_residual_2d(P["rho"], P["alp"], P["dt"], P["dsp"], P["fns"], 70.0, P["epsl"], P["x_arr"], None,
                                      P["bc"])


def precond_longdouble(source, fv, dt, bc, C):
    """H1_precond_2d with the t-solve per mode in np.longdouble: diagonal C - fv + 2/dt^2 (last row + 1/dt^2),
    off-diagonals -1/dt^2, u_0 = 0, by textbook elimination (not the oracle's scan form).  The transforms stay
    float64 (scipy)."""
    L, CL = np.longdouble, np.clongdouble
    periodic = tuple(bc) == (0, 0)
    if periodic:
        v = sfft.fft2(source[1:], axes=(1, 2))
    else:
        v = sfft.fft(sfft.dct(source[1:], axis=1), axis=2)
    T = v.shape[0]
    o = L(1) / (L(dt) * L(dt))
    base = L(C) - np.asarray(fv).astype(CL)
    d = [base + (2 * o if j < T - 1 else o) for j in range(T)]
    b = [v[j].astype(CL) for j in range(T)]
    for j in range(1, T):               # eliminate the sub-diagonal -o
        w = -o / d[j - 1]
        d[j] = d[j] + w * o             # d_j - w * (upper = -o)
        b[j] = b[j] - w * b[j - 1]
    x = [None] * T
    x[T - 1] = b[T - 1] / d[T - 1]
    for j in range(T - 2, -1, -1):
        x[j] = (b[j] + o * x[j + 1]) / d[j]
    part = np.stack(x).astype(np.complex128)
    if periodic:
        upd = sfft.ifft2(part, axes=(1, 2)).real
    else:
        upd = sfft.idct(sfft.ifft(part, axis=2).real, axis=1)
    return np.concatenate([np.zeros((1,) + upd.shape[1:]), upd], axis=0)


def exact_symbol(P):
    """The Laplacian symbol of bc (0, 0) in closed form, -4/dx^2 sin^2(pi kx/nx) - 4/dy^2 sin^2(pi ky/ny), evaluated
    in np.longdouble and rounded once.  The oracle's fv is the FFT of the stencil, as the reference forms it
    (utils_precond.py:42-71): its roundoff is absolute, ~ eps log(n) / dx^2 (3e-8 at nx = 8192, dx = 2/8192), which
    the low modes feel once 2/dt^2 no longer dominates the diagonal.  A diagnostic, not a reference of any test."""
    L = np.longdouble
    pi = L(np.pi) + L(1.2246467991473532e-16)
    nx, ny = P["nsp"]
    lx = -4 / L(P["dx"]) ** 2 * np.sin(pi * np.arange(nx, dtype=L) / nx) ** 2
    ly = -4 / L(P["dy"]) ** 2 * np.sin(pi * np.arange(ny, dtype=L) / ny) ** 2
    return (lx[:, None] + ly[None, :]).astype(np.float64).astype(np.complex128)


def residual32(P):
    """residual() executed in float32 (every input cast first)."""
    f = np.float32
    out = O.compute_cont_residual_2d(P["rho"].astype(f), tuple(a.astype(f) for a in P["alp"]), P["dt"], P["dsp"],
                                     P["fns"], 70.0, P["epsl"], P["x_arr"].astype(f), None, P["bc"])
    assert out.dtype == f
    return out


def oracle_update(P, C, src=None):
    """(phi', U): the float64 oracle's primal update of the problem's state -- update_primal_2d's
    phi + tau * H1_precond_2d(continuity residual) -- and U = (phi' - phi) / tau.  src: the residual, which does not
    depend on C, when the caller kept it."""
    src = residual(P) if src is None else src
    phi_o = P["phi"] + TAU * O.H1_precond_2d(src, P["fv"], P["dt"], P["bc"], C=C)
    return phi_o, (phi_o - P["phi"]) / TAU


def oracle_update32(P, C, src32=None):
    """oracle_update executed in float32 (complex64 transforms and t-solve): the calibration of the fp32 bounds, as in
    test_precond_1d_parameters."""
    src32 = residual32(P) if src32 is None else src32
    phi0 = P["phi"].astype(np.float32)
    phi_32 = phi0 + TAU * O.H1_precond_2d(src32, P["fv"], P["dt"], P["bc"], C=C)
    assert phi_32.dtype == np.float32
    return phi_32, (phi_32 - phi0) / TAU
