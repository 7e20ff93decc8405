"""State read-back: pdhg_get_rows against pdhg_get_state, and both against what pdhg_set_state was given.

get_state and get_rows are one host routine over a row range (phi has T + 1 rows, rho and alp T; get_rows also returns
phi_bar), so every row range must be the matching slice of the whole state, bit for bit: no arithmetic lies between the
device arrays and the caller's, only a copy and, in fp32, a widening.  What set_state stores is the caller's float64
value rounded to the context's type: exact in fp64, the float32 rounding in fp32, and in mixed contexts phi exact
(held in float64) with rho and alp rounded.  The cases cover the two live-component maps of the 2-D controls (egno 1:
component 0 of arrays 0 / 1 and component 1 of arrays 2 / 3; egno 3: one component, arrays 2 / 3 dead), a 1-D context,
and a context whose current buffer set is the second one (rho_alp_iters = 2 after one iteration)."""
import numpy as np
import pytest

import pdhg_oracle as O
from _report_support import state as _state

pytestmark = pytest.mark.gpu

T = 3
TAU, SIGMA = 0.1 / 1.5, 0.1 * 1.5
# egno, ndim, nx, ny, precision, rho_alp_iters (2: one iteration runs first, so the second buffer set is current)
CASES = [(1, 2, 64, 64, "fp32", 1), (1, 2, 64, 64, "fp64", 1), (1, 2, 64, 64, "mixed", 1),
         (3, 2, 64, 64, "fp32", 1), (3, 2, 64, 64, "fp64", 1), (3, 2, 64, 64, "mixed", 1),
         (2, 1, 256, 1, "fp32", 1), (2, 1, 256, 1, "fp64", 1), (1, 2, 64, 64, "fp32", 2)]


def _context(egno, ndim, nx, ny, prec, k):
    from pdhg_amd.context import PDHGContext
    x_arr = O.make_grid(ndim, nx, ny, egno)
    if ndim == 1:
        xs, ys, dy = x_arr[0, :, 0], None, 0.0
    else:
        xs, ys, dy = x_arr[0, :, 0, 0], x_arr[0, 0, :, 1], 2.0 / ny
    ctx = PDHGContext(egno, ndim, nx, ny, T, 2.0 / nx, dy, 1.0 / T, xs, ys, epsl=0.1 if egno == 2 else 0.0,
                      precision=prec, rho_alp_iters=k)
    if k > 1:   # one iteration from the reference's initial state: the state moves to the second buffer set
        g = O.set_up_J(egno, ndim, (2.0, 2.0))(x_arr)
        sp = g.shape[1:]
        ctx.set_state(np.repeat(g, T + 1, axis=0), np.full((T,) + sp, 70.0),
                      tuple(np.zeros((T,) + sp + (ctx.n_ctrl,)) for _ in range(ctx.n_alp)))
        st = ctx.iterate(1, TAU, SIGMA, -1.0, k)
        assert st["iters_run"] == 1, st
    return ctx


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("egno, ndim, nx, ny, prec, k", CASES)
def test_rows_are_slices_of_the_state(native, egno, ndim, nx, ny, prec, k):
    phi, rho, alp = _state(egno, ndim, nx, ny, T, seed=3)
    assert not np.array_equal(phi, _f32(phi))          # the float32 rounding is visible
    ctx = _context(egno, ndim, nx, ny, prec, k)
    try:
        ctx.set_state(phi, rho, alp)
        phi_d, rho_d, alp_d = ctx.get_state()
        # what was set, after the context's rounding
        assert np.array_equal(phi_d, phi if prec in ("fp64", "mixed") else _f32(phi))
        assert np.array_equal(rho_d, rho if prec == "fp64" else _f32(rho))
        assert len(alp_d) == len(alp)
        for a_d, a in zip(alp_d, alp):
            assert np.array_equal(a_d, a if prec == "fp64" else _f32(a))
        pbar_d = ctx.get_phi_bar()
        assert np.array_equal(pbar_d, phi_d)           # set_state writes phi to phi_bar too
        for row0, n in ((0, T), (1, 1)):
            ph, pb, rh, al = ctx.get_rows(row0, n, phi=True, phi_bar=True, rho=True, alp=True)
            assert np.array_equal(ph, phi_d[row0:row0 + n]) and np.array_equal(pb, pbar_d[row0:row0 + n]), (row0, n)
            assert np.array_equal(rh, rho_d[row0:row0 + n]), (row0, n)
            assert len(al) == len(alp_d) and all(np.array_equal(x, y[row0:row0 + n]) for x, y in zip(al, alp_d)), \
                (row0, n)
        ph, pb, rh, al = ctx.get_rows(T, 1, phi=True, phi_bar=True, rho=False, alp=False)   # phi's last row: phi only
        assert np.array_equal(ph, phi_d[T:]) and np.array_equal(pb, pbar_d[T:]) and rh is None and al is None
        with pytest.raises(native.PDHGError):          # rho / alp have no row T
            ctx.get_rows(T, 1)
        # a dead control component is refused wherever the layout has one (1-D: every component is live)
        dead = [(a, c) for a in range(ctx.n_alp) for c in range(ctx.n_ctrl) if not alp[a][..., c].any()]
        assert bool(dead) == (ndim == 2)
        for a, c in dead[:1]:
            bad = [v.copy() for v in alp]
            bad[a][1, ..., c] = 1.0
            with pytest.raises(native.PDHGUnsupported):
                ctx.set_state(phi, rho, bad)
    finally:
        ctx.close()
