"""Mixed precision (pdhg_problem.precision 12: fp32 state, fp64 phi / phi_bar) without a device: the plan
(pdhg_plan_info), what is refused, the Python layers, and the condition the GPU parity shape must meet."""
import ctypes

import numpy as np
import pytest

import pdhg_oracle as O
import _mixed_emul as E
from _problems import make_problem
from test_gpu_mixed import MIXED_CASES, MIXED_LARGE, mixed_case_emulation

MIXED = 12
ENV = ("PDHG_DUAL_MULTI", "PDHG_DUAL_HEAD", "PDHG_DUAL_RX", "PDHG_FUSE_RES", "PDHG_SHORT_T", "PDHG_HALF_NT",
       "PDHG_DUAL_ONE", "PDHG_XT_BATCH", "PDHG_XT_DMA")
# the GPU parity shape (tests/test_gpu_mixed.py): 256 x 256 with the period shrunk so that dx = 2/4096, epsl = 0.1
PARITY_PERIOD = 256 * 2.0 / 4096


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _problem(lib, egno, ndim, nx, ny, T, precision, k=1):
    ny = ny if ndim == 2 else 1
    xs, ys = np.linspace(0, 2, nx, endpoint=False), np.linspace(0, 2, ny, endpoint=False)
    p = lib.pdhg_problem()
    p.egno, p.ndim, p.nx, p.ny, p.T, p.precision, p.rho_alp_iters = egno, ndim, nx, ny, T, precision, k
    bc = O.default_bc(egno, ndim)
    p.bc_x, p.bc_y = (bc, 0) if ndim == 1 else bc
    p.dx, p.dy, p.dt, p.C, p.pow_, p.Ct, p.c_on_rho = 2 / nx, 2 / ny, 1.0 / max(T, 40), 1.0, 1.0, 1.0, 70.0
    p.epsl = 0.1
    p.xs, p.ys = lib.dptr(xs), lib.dptr(ys)
    return p, (xs, ys)


def _plan(lib, p, keys):
    out = {}
    for key in keys:
        v = ctypes.c_int(-12345)
        rc = lib.load().pdhg_plan_info(ctypes.byref(p), key.encode(), ctypes.byref(v))
        assert rc == lib.PDHG_OK, (key, rc, lib.load().pdhg_last_error())
        out[key] = v.value
    return out


def test_plan_c3_mixed(lib):
    """C3's window (egno 2, 4096^2, T = 200, k = 1): the fp32 fast rows and x transform, the row-per-thread dual
    (fast_dual 0), no fused residual, dual64 0."""
    p, keep = _problem(lib, 2, 2, 4096, 4096, 200, MIXED)
    got = _plan(lib, p, ("mixed", "fused_residual", "fast_dual", "fast_rows", "fast_xt", "dual64", "upd_threads"))
    assert got["fast_xt"] != 0
    del got["fast_xt"]
    assert got == {"mixed": 1, "fused_residual": 0, "fast_dual": 0, "fast_rows": 1, "dual64": 0, "upd_threads": 512}
    # the fp32 plan of the same window differs exactly there: the LDS-row sweep with the fused residual
    p4, keep4 = _problem(lib, 2, 2, 4096, 4096, 200, 4)
    assert _plan(lib, p4, ("mixed", "fused_residual", "fast_dual")) == {"mixed": 0, "fused_residual": 1, "fast_dual": 8}


@pytest.mark.parametrize("shape", [(2, 2, 4096, 4096, 200), (2, 2, 256, 256, 3), (2, 2, 2048, 2048, 1)],
                         ids=["c3", "256x256_T3", "c2_T1"])
def test_plan_k10_as_fp32(lib, shape):
    """rho_alp_iters = 10: the chunked dual loop or its head form, chosen as for fp32."""
    keys = ("dual_multi", "dual_head", "spec", "fast_dual")
    pm, keep_m = _problem(lib, *shape, MIXED, k=10)
    p4, keep_4 = _problem(lib, *shape, 4, k=10)
    got = _plan(lib, pm, keys)
    assert got == _plan(lib, p4, keys)
    assert got["dual_multi"] + got["dual_head"] == 1 and got["fast_dual"] == 0
    assert _plan(lib, pm, ("mixed",)) == {"mixed": 1}


def test_plan_env_cannot_select_the_lds_dual(lib, monkeypatch):
    """PDHG_DUAL_RX / PDHG_FUSE_RES select the LDS-row sweep for fp32; a mixed context keeps the row-per-thread one."""
    monkeypatch.setenv("PDHG_DUAL_RX", "8")
    monkeypatch.setenv("PDHG_FUSE_RES", "1")
    p, keep = _problem(lib, 2, 2, 512, 512, 8, MIXED)
    assert _plan(lib, p, ("fast_dual", "fused_residual")) == {"fast_dual": 0, "fused_residual": 0}


def test_plan_generic_dual_where_ny_is_no_multiple_of_256(lib):
    p, keep = _problem(lib, 1, 2, 20, 18, 3, MIXED)
    assert _plan(lib, p, ("mixed", "fast_dual", "fast_rows")) == {"mixed": 1, "fast_dual": -1, "fast_rows": 0}


@pytest.mark.parametrize("precision", [4, 8])
def test_other_precisions_answer_mixed_0(lib, precision):
    p, keep = _problem(lib, 2, 2, 256, 256, 3, precision)
    assert _plan(lib, p, ("mixed",)) == {"mixed": 0}


@pytest.mark.parametrize("precision", [2, 6, 16, 0, -12])
def test_other_values_are_argument_errors(lib, precision):
    p, keep = _problem(lib, 2, 2, 256, 256, 3, precision)
    v = ctypes.c_int(0)
    assert lib.load().pdhg_plan_info(ctypes.byref(p), b"mixed", ctypes.byref(v)) == lib.PDHG_ERR_ARG


def test_1d_is_unsupported(lib):
    """Before any device is touched: pdhg_create and pdhg_plan_info give the same status."""
    L = lib.load()
    p, keep = _problem(lib, 2, 1, 256, 1, 3, MIXED)
    v, h = ctypes.c_int(0), ctypes.c_void_p()
    assert L.pdhg_plan_info(ctypes.byref(p), b"mixed", ctypes.byref(v)) == lib.PDHG_ERR_UNSUPPORTED
    assert L.pdhg_create(ctypes.byref(p), 0, ctypes.byref(h)) == lib.PDHG_ERR_UNSUPPORTED
    assert b"mixed" in L.pdhg_last_error() and not h.value


def test_decompositions_are_unsupported(lib):
    """pdhg_create_slab / _xslab / _multi refuse precision 12 before they touch a device."""
    L = lib.load()
    p, keep = _problem(lib, 2, 2, 256, 256, 4, MIXED)
    h = ctypes.c_void_p()
    assert L.pdhg_create_slab(ctypes.byref(p), 0, 4, 0, ctypes.byref(h)) == lib.PDHG_ERR_UNSUPPORTED
    assert b"mixed" in L.pdhg_last_error() and not h.value
    assert L.pdhg_create_xslab(ctypes.byref(p), 0, 2, 0, ctypes.byref(h)) == lib.PDHG_ERR_UNSUPPORTED
    assert b"mixed" in L.pdhg_last_error() and not h.value
    devs = (ctypes.c_int * 2)(0, 0)
    assert L.pdhg_create_multi(ctypes.byref(p), devs, 2, ctypes.byref(h)) == lib.PDHG_ERR_UNSUPPORTED
    assert b"mixed" in L.pdhg_last_error() and not h.value


def test_python_layers_accept_mixed(lib, monkeypatch):
    from pdhg_amd import context, run_example, update_fns_in_pdhg as U, utils_pdhg_solver as S
    seen = []
    monkeypatch.setattr(context.PDHGContext, "_create", lambda self, prob, device: seen.append(prob.precision) or None)
    xs = np.linspace(0, 2, 20, endpoint=False)
    for prec in ("mixed", 12):
        context.PDHGContext(1, 2, 20, 18, 3, 0.1, 0.1, 0.025, xs, xs[:18], epsl=0.1, precision=prec)
    assert seen == [12, 12]
    with pytest.raises(KeyError):
        context.PDHGContext(1, 2, 20, 18, 3, 0.1, 0.1, 0.025, xs, xs[:18], precision="fp16")
    before = U.get_precision()
    try:
        U.set_precision("mixed")
        assert U.get_precision() == "mixed"
    finally:
        U.set_precision(before)
    fp, fd = S.make_update_fns(2, (0, 0), rho_alp_iters=1, precision="mixed")
    assert fp._pdhg_native["precision"] == "mixed" and fd._pdhg_native is fp._pdhg_native
    assert run_example.build_parser().parse_args(["--precision", "mixed"]).precision == "mixed"


def test_decomposed_classes_raise_value_error(lib):
    from pdhg_amd.multi import MultiContext
    from pdhg_amd.slab import SlabContext
    from pdhg_amd.xslab import XSlabContext
    xs = np.linspace(0, 2, 256, endpoint=False)
    for prec in ("mixed", 12):
        with pytest.raises(ValueError):
            MultiContext(2, 256, 256, 4, 2 / 256, 2 / 256, 0.025, xs, xs, devices=[0, 0], precision=prec)
        with pytest.raises(ValueError):
            SlabContext(0, 2, 4, 2, 256, 256, 2 / 256, 2 / 256, 0.025, xs, xs, precision=prec)
        with pytest.raises(ValueError):
            XSlabContext(0, 2, 2, 256, 256, 1, 2 / 256, 2 / 256, 0.025, xs, xs, precision=prec)


@pytest.mark.parametrize("name", [n for n in MIXED_CASES if "@" not in n and n not in MIXED_LARGE])
def test_shape_cases_meet_the_caps(name):
    """The caps of tests/test_gpu_mixed.py::test_mixed_instantiation from the emulation alone, for every default-tier
    case and both of its runs: 4 e_mixed <= 1e-4 for phi and <= 10 x the floor for rho and each control,
    4 e_mixed(U1) <= 5e-3 from the seeded state, e32(rho) >= 10 e_mixed(rho) from the reference state -- so a loose
    emulation fails here, without a device, instead of passing a wrong kernel.  The two cases of millions of points
    (c3_b2_stride, halfreal_b1: 35 s and 17 s of emulation) are left to the GPU test's own pre-check, which asserts the
    same conditions through the same function.  Found over these cases: reference state e_mixed(rho) 2.9e-8 - 4.4e-8,
    e32(rho) 4.6e-5 - 7.1e-5, e_mixed(alp) <= 1.5e-7; seeded e_mixed(phi) <= 1.4e-5, rho <= 2.7e-7, alp <= 7.5e-6,
    U1 <= 1.2e-4 (ny4096_march at its epsl = 0: phi 1.7e-8, U1 3.4e-6; at epsl = 0.1 it misses the phi cap with
    2.8e-5, see MIXED_SEEDED_EPSL)."""
    for seeded in (False, True):
        P = mixed_case_emulation(name, seeded)[0]   # the caps are asserted inside this helper
        # powers of two throughout (period = max(nx, ny) 2 / 4096 over a power-of-two extent): exact in binary
        assert min(P["dx"], P["dy"]) == 2.0 / 4096


def test_parity_shape_discriminates():
    """The condition on the GPU parity shape (egno 2, 256 x 256, epsl 0.1, period 1/8: dx = 2/4096, so the dual's
    explicit sigma epsl Lap(phi_bar) amplifies phi_bar's float32 representation by sigma epsl 8 / dx^2 = 5e5): after
    one iteration from the reference state the all-float32 emulation's rho is >= 10 x further from the float64
    oracle than the mixed emulation's.  Found: e32(rho) = 1.03e-4, e_mixed(rho) = 4.6e-8, ratio 2.2e3 (T = 3;
    T = 1 likewise).  From the seeded rough state rho' is dominated by epsl Lap of the noise in phi and the two
    emulations are within a factor 1.5 after one iteration (3.2e-7 / 2.3e-7): the seeded state checks parity, the
    reference state what the mixed path is for."""
    for T in (3, 1):
        P = make_problem(2, 2, 256, 256, T, 0.1, seeded=False, period=PARITY_PERIOD)
        assert abs(P["dx"] - 2.0 / 4096) < 1e-15
        _, e_mixed, e32 = E.errors(P, 1)
        print("T = {}: e32(rho) {:.3e} e_mixed(rho) {:.3e} ratio {:.1f}".format(T, e32["rho"], e_mixed["rho"],
                                                                              e32["rho"] / e_mixed["rho"]))
        assert e32["rho"] >= 10 * e_mixed["rho"], (T, e32["rho"], e_mixed["rho"])
        assert e_mixed["rho"] < 2e-7   # float32 storage of rho, not phi_bar's representation
