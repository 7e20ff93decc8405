"""The float64 oracle's H1_precond_2d (oracle/pdhg_oracle.py, utils_precond.py:142-178) at the solve parameters the GPU
tests of test_gpu_precond2d.py hold the kernels to -- C = 0 (the undamped zero mode), large C, and time steps from
1/400 to 1/2 -- against the same tridiagonal systems solved per mode in np.longdouble.  No GPU."""
import numpy as np
import pytest

import pdhg_oracle as O
from _precond_support import per_mode, precond_longdouble, residual
from _problems import make_problem, rel

CS = [0.0, 1.0, 100.0]
DTS = [1 / 400, 1 / 40, 1 / 2]
TS = [12, 64]
CASES = [(1, C, dt, T) for T in TS for dt in DTS for C in CS] + [(3, 0.0, 1 / 40, 12)]


@pytest.mark.parametrize("egno,C,dt,T", CASES, ids=["e{}_C{:g}_dt{:g}_T{}".format(*c) for c in CASES])
def test_oracle_matches_longdouble_thomas(egno, C, dt, T):
    """64 x 16, bc (0, 0) (egno 1) and one bc (1, 0) case (egno 3), the seeded rough state's continuity residual as
    the source.  The oracle must be finite with no floating-point warning (np.errstate(all="raise")) and within 1e-12
    of the long-double solve in relative L2 and in the per-mode measure (_precond_support.per_mode): 100x under the
    1e-10 the fp64 kernels are held to against it.

    Measured over these 19 cases (x86-64, 80-bit long double): relative L2 at most 3.7e-14 and the per-mode measure at
    most 9.0e-14, both at T = 64, dt = 1/400, C = 0 (C = 1 there: 3.7e-14 / 8.5e-14; C = 100: 1.8e-14 / 4.9e-14); at
    dt = 1/40 and 1/2 both stay under 3e-14, at T = 12 under 8e-15.  The bc (1, 0) case: 9.8e-16 / 2.8e-15."""
    P = make_problem(egno, 2, 64, 16, T, 0.0, dt=dt)
    src = residual(P)
    with np.errstate(all="raise"):
        U = O.H1_precond_2d(src, P["fv"], dt, P["bc"], C=C)
    assert np.isfinite(U).all()
    U_l = precond_longdouble(src, P["fv"], dt, P["bc"], C)
    e, pm = rel(U, U_l), per_mode(U, U_l, P["bc"])
    print("ORACLE2D e{} C={:g} dt={:g} T={}: rel {:.2e} per-mode {:.2e}".format(egno, C, dt, T, e, pm))
    assert np.array_equal(U[0], np.zeros_like(U[0]))
    assert e <= 1e-12, e
    assert pm <= 1e-12, pm


def test_parameters_change_the_solution():
    """C and dt reach the solve: the zero mode of U moves by more than 1 % between C = 0 and C = 1, and U differs
    between dt = 1/40 and 1/400 (a measure that could not tell the parameters apart would pin nothing)."""
    P = make_problem(1, 2, 64, 16, 12, 0.0, dt=1 / 40)
    src = residual(P)
    U0, U1 = (O.H1_precond_2d(src, P["fv"], P["dt"], P["bc"], C=C) for C in (0.0, 1.0))
    z0, z1 = U0[1:].sum(axis=(1, 2)), U1[1:].sum(axis=(1, 2))
    assert np.linalg.norm(z0 - z1) > 1e-2 * np.linalg.norm(z1)
    assert per_mode(U0, U1, P["bc"]) > 1e-3
    assert rel(O.H1_precond_2d(src, P["fv"], 1 / 400, P["bc"], C=1.0), U1) > 1e-2
