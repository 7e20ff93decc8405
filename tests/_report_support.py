"""Shared by the report tests (test_report_host.py, test_gpu_report.py): the problem pieces and a random state."""
import numpy as np

import pdhg_oracle as O


def setup(egno, ndim, nx, ny, T):
    """(x_arr, bc, dspatial, fns) of the example on the [0, 2) grid (egno 3: centred, bc (1, 0))."""
    x_arr = O.make_grid(ndim, nx, ny, egno)
    bc = O.default_bc(egno, ndim)
    dsp = (2.0 / nx,) if ndim == 1 else (2.0 / nx, 2.0 / ny)
    return x_arr, bc, dsp, O.set_up_example_fns(egno, ndim, 0)


def state(egno, ndim, nx, ny, T, seed=0):
    """A random state in the reference layouts: phi random, rho >= 0 with exact zeros at about 30 % of the points, alp
    of both signs (so both the f >= 0 and the f < 0 masks fire), dead control components zero."""
    rng = np.random.default_rng(seed)
    sp = (nx,) if ndim == 1 else (nx, ny)
    phi = rng.standard_normal((T + 1,) + sp)
    rho = np.maximum(rng.standard_normal((T,) + sp) + 0.5, 0.0) * 3
    nc = 1 if (ndim == 1 or egno == 3) else 2
    alp = []
    for a in range(2 if ndim == 1 else 4):
        v = np.zeros((T,) + sp + (nc,))
        if egno == 3:
            if a < 2:
                v[..., 0] = rng.standard_normal((T,) + sp)
        else:
            v[..., a // 2 if ndim == 2 else 0] = rng.standard_normal((T,) + sp)
        alp.append(v)
    return phi, rho, tuple(alp)
