"""The dual sweep's workgroup -> tile order (PDHG_DUAL_ORDER, csrc/dual_order.hpp): the band order (XB = 1, 2, 4)
against the x-fastest order 0 in the same process, 3 outer iterations from the seeded state.  The order only changes
which workgroup computes a tile; every tile writes the rows, the edge terms and the partial row it writes under
order 0, so phi, rho, the four alp and the returned sums are bitwise equal.

Shapes: the smallest grids of tiles at which the mapping can go wrong -- 8 x 2 (one tile per XCD slot, the strip
wrap at both ends), 5 tiles along x (not a multiple of 8: the tail), 16 x 4 (two rounds per XCD: a band's x neighbour
comes from another round; XB = 2 is a real band there).  The fp32 fused sweep (256-column strips) reaches those grids
at ny = 512 / 1024.  The fp64 fused residual exists for ny = 2048 / 4096 / 8192 only (path_plan.hpp: the 4-row
residual kernels), so at the small ny the plan runs the fp64 sweep without it (or, at ny = 384, the per-point kernel,
which has no tile order); those cases stay as the comparison of whatever the plan selects, and the fp64 fused sweep
is covered at ny = 2048 (16 strips) with the same three x extents.  One fp64 fused case is also held to the float64
oracle at the fp64 bound of test_gpu_fused (phi, rho <= 1e-9), so the comparison is not two equal wrong answers."""
import numpy as np
import pytest

from _problems import device_ctx, make_problem, rel
from test_gpu_parity import SIGMA, TAU, _oracle_iterate

pytestmark = pytest.mark.gpu

N_ITERS = 3
BANDS = ("1", "2", "4")
FORCE = {"PDHG_FUSE_RES": "1", "PDHG_DUAL_RX": "8"}


def _run(P, precision, order, monkeypatch, env, k=1):
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    monkeypatch.setenv("PDHG_DUAL_ORDER", order)
    ctx = device_ctx(P, precision, rho_alp_iters=k)
    try:
        info = {key: ctx.path_info(key) for key in ("fused_residual", "fast_dual", "dual_ypl")}
        ctx.set_state(P["phi"], P["rho"], P["alp"])
        st = ctx.iterate(N_ITERS, TAU, SIGMA, -1.0, k)
        return ctx.get_state(), st, info
    finally:
        ctx.close()


def _bitwise(P, precision, monkeypatch, env=FORCE, k=1, expect=None):
    """Order 0 once, then every band order against it; returns order 0's state."""
    s0, st0, info0 = _run(P, precision, "0", monkeypatch, env, k)
    print("plan", precision, (P["nx"], P["ny"], P["T"]), info0)
    if expect is not None:
        assert {key: info0[key] for key in expect} == expect, info0
    assert st0["iters_run"] == N_ITERS
    for band in BANDS:
        s1, st1, info1 = _run(P, precision, band, monkeypatch, env, k)
        assert info1 == info0
        assert np.array_equal(s1[0], s0[0]), ("phi", band)
        assert np.array_equal(s1[1], s0[1]), ("rho", band)
        assert len(s1[2]) == 4
        for a, (x, y) in enumerate(zip(s1[2], s0[2])):
            assert np.array_equal(x, y), ("alp", a, band)
        for key in ("err1", "err2", "iters_run"):
            assert st1[key] == st0[key], (key, band, st1[key], st0[key])
    return s0, st0


# egno, ndim, nx, ny, T, epsl
FP64_SMALL = [(1, 2, 64, 256, 3, 0.0), (1, 2, 40, 384, 3, 0.0), (2, 2, 128, 512, 5, 0.1)]
FP64_FR = [(1, 2, 64, 2048, 3, 0.0), (1, 2, 40, 2048, 3, 0.0), (2, 2, 128, 2048, 5, 0.1)]
FP32_FR = [(1, 2, 64, 512, 3, 0.0), (1, 2, 40, 512, 3, 0.0), (2, 2, 128, 1024, 5, 0.1)]
_ids = lambda cs: ["e{}_{}x{}_T{}".format(c[0], c[2], c[3], c[4]) for c in cs]  # noqa: E731


@pytest.mark.parametrize("case", FP64_SMALL, ids=_ids(FP64_SMALL))
def test_fp64_small_grids(native, monkeypatch, case):
    """The small fp64 shapes under PDHG_FUSE_RES=1, PDHG_DUAL_RX=8: no fused residual at these ny (see above), so
    k_dual_lds_2d<.., 8, false, double> on 256-column strips (ny = 384: the per-point kernel)."""
    _bitwise(make_problem(*case), "fp64", monkeypatch, expect={"fused_residual": 0})


@pytest.mark.parametrize("case", FP64_FR, ids=_ids(FP64_FR))
def test_fp64_fused_sweep(native, monkeypatch, case):
    """k_dual_lds_2d<.., 8, true, double, 2>: grids of 8 x 16, 5 x 16 (the tail) and 16 x 16 tiles (two rounds per
    XCD, eps = 0.1 so the eps terms of p.ex / p.ey count)."""
    _bitwise(make_problem(*case), "fp64", monkeypatch, expect={"fused_residual": 1, "fast_dual": 8, "dual_ypl": 2})


def test_fp64_fused_sweep_vs_oracle(native, monkeypatch):
    P = make_problem(*FP64_FR[0])
    phi_o, rho_o, _, _, _ = _oracle_iterate(P, N_ITERS)
    s1, _, info = _run(P, "fp64", "1", monkeypatch, FORCE)
    assert info["fused_residual"] == 1
    m = (rel(s1[0], phi_o), rel(s1[1], rho_o))
    print("band order vs oracle: phi %.3e rho %.3e" % m)
    assert m[0] <= 1e-9 and m[1] <= 1e-9, m


@pytest.mark.parametrize("case", FP32_FR, ids=_ids(FP32_FR))
def test_fp32_fused_sweep(native, monkeypatch, case):
    """k_dual_lds_2d<.., 8, true> (4 y per lane): grids of 8 x 2, 5 x 2 and 16 x 4 tiles."""
    _bitwise(make_problem(*case), "fp32", monkeypatch, expect={"fused_residual": 1, "fast_dual": 8})


@pytest.mark.parametrize("rx", [None, "8"], ids=["row_per_thread", "lds_rows"])
def test_fp64_two_sub_iterations(native, monkeypatch, rx):
    """rho_alp_iters = 2 (two buffer sets, no fused residual) at 64 x 256: the row-per-thread kernels the plan selects
    (untouched by the order), and with PDHG_DUAL_RX=8 k_dual_lds_2d without the fused residual, one launch per
    sub-iteration over 3 time chunks (blockIdx.z)."""
    env = {} if rx is None else {"PDHG_DUAL_RX": rx}
    if rx is None:
        monkeypatch.delenv("PDHG_DUAL_RX", raising=False)
    _bitwise(make_problem(1, 2, 64, 256, 3, 0.0), "fp64", monkeypatch, env=env, k=2,
             expect={"fused_residual": 0, "fast_dual": 0 if rx is None else 8})
