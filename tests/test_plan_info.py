"""The kernel-path plan without a device (pdhg_plan_info): the path_info values the GPU tests assert on their
contexts, asserted here from the problem and the environment alone.  The expectations are those tests' own tables
(written against the GPU's behaviour); a context's pdhg_path_info answers from the same plan.  No GPU needed."""
import ctypes
import glob
import os

import numpy as np
import pytest

import pdhg_oracle as O
from test_gpu_configs import CASES, FP64_CASES, FP64_ENV, ONE_STEP
from test_gpu_mixed import MIXED_CASES, MIXED_ENV

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pdhg-optimal-control_amd", "csrc")
RUNTIME_KEYS = ("contig_fail", "spec_iters", "spec_halts", "graph", "graph_window")
# every PDHG_* variable the cases below set: cleared first, so a case sees its own environment only
ENV_USED = ("PDHG_FUSE_RES", "PDHG_XT_BATCH", "PDHG_XT_DMA", "PDHG_XT_DMA_HR", "PDHG_XT_WS", "PDHG_SHORT_T",
            "PDHG_HALF_NT", "PDHG_FS16", "PDHG_FS_WIDE", "PDHG_THOMAS_CHUNK", "PDHG_XT64", "PDHG_XT64_VAR", "PDHG_RES64",
            "PDHG_DUAL64", "PDHG_RES64_NT2048", "PDHG_UPD_T1", "PDHG_TC_SPEC", "PDHG_UPD8192", "PDHG_C4_TO",
            "PDHG_T1_XT", "PDHG_T1_G16", "PDHG_FOURSTEP", "PDHG_FUSE_RES1D", "PDHG_SPEC", "PDHG_DUAL_ONE",
            "PDHG_DUAL_HEAD", "PDHG_K1_OUTER", "PDHG_DUAL_MULTI", "PDHG_FOLD_FIN", "PDHG_ROWS_VAR", "PDHG_RES64_NT",
            "PDHG_UPD_PAIR", "PDHG_UPD_PF")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


def _problem(lib, egno, ndim, nx, ny, T, precision=4, k=1, kw=None):
    ny = ny if ndim == 2 else 1
    xs, ys = np.linspace(0, 2, nx, endpoint=False), np.linspace(0, 2, ny, endpoint=False)
    p = lib.pdhg_problem()
    p.egno, p.ndim, p.nx, p.ny, p.T, p.precision, p.rho_alp_iters = egno, ndim, nx, ny, T, precision, k
    bc = O.default_bc(egno, ndim)
    p.bc_x, p.bc_y = (bc, 0) if ndim == 1 else bc
    p.dx, p.dy, p.dt, p.C, p.pow_, p.Ct, p.c_on_rho = 2 / nx, 2 / ny, 1.0 / max(T, 40), 1.0, 1.0, 1.0, 70.0
    p.xs, p.ys = lib.dptr(xs), lib.dptr(ys)
    for key, v in (kw or {}).items():   # overrides, invalid ones included
        setattr(p, key, v)
    return p, (xs, ys)


def _plan(lib, p, key):
    v = ctypes.c_int(-12345)
    rc = lib.load().pdhg_plan_info(ctypes.byref(p), key.encode(), ctypes.byref(v))
    assert rc == lib.PDHG_OK, (key, rc, lib.load().pdhg_last_error())
    return v.value


def _check(lib, monkeypatch, env, shape, expect, precision=4, k=1):
    for name in ENV_USED:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        assert name in ENV_USED, name
        monkeypatch.setenv(name, v)
    p, keep = _problem(lib, *shape, precision=precision, k=k)
    got = {key: _plan(lib, p, key) for key in expect}
    assert got == expect, (env, shape, precision, k)


def _meta(name):
    F = np.load(os.path.join(HERE, "golden", "cfg_{}.npz".format(name.split("@")[0].split("+")[0])))
    return tuple(int(v) for v in F["meta"])   # egno, ndim, nx, ny, T


@pytest.mark.parametrize("name", sorted(CASES))
def test_config_cases_fp32(lib, monkeypatch, name):
    env, expect = CASES[name]
    _check(lib, monkeypatch, env, _meta(name), expect)


@pytest.mark.parametrize("name", sorted(FP64_CASES))
def test_config_cases_fp64(lib, monkeypatch, name):
    _check(lib, monkeypatch, FP64_ENV.get(name.partition("+")[2], {}), _meta(name), FP64_CASES[name], precision=8)


@pytest.mark.parametrize("name", sorted(MIXED_CASES))
def test_config_cases_mixed(lib, monkeypatch, name):
    """tests/test_gpu_mixed.py::test_mixed_instantiation's table (precision 12), the extended-tier cases included."""
    egno, nx, ny, T, env, expect = MIXED_CASES[name]
    assert set(MIXED_ENV) <= set(ENV_USED)
    _check(lib, monkeypatch, env, (egno, 2, nx, ny, T), expect, precision=12)


@pytest.mark.parametrize("name", sorted(ONE_STEP))
def test_one_step_cases(lib, monkeypatch, name):
    egno, nx, ny, T, env, expect = ONE_STEP[name]
    _check(lib, monkeypatch, env, (egno, 2, nx, ny, T), expect)


FR = {"PDHG_SHORT_T": "0"}   # test_gpu_fused._ctx
# (environment, (egno, ndim, nx, ny, T), precision, rho_alp_iters, expected): the fp64 expectations of test_gpu_res64,
# test_gpu_xt64, test_gpu_fused and test_gpu_parity, with those tests' grid sizes
FP64 = [
    # test_gpu_res64: CASES, res64 on / off
    *[({}, c, 8, 1, {"res64": 1}) for c in [(1, 2, 8, 2048, 3), (2, 2, 8, 4096, 3), (2, 2, 12, 2048, 2),
                                            (3, 2, 8, 2048, 2), (2, 2, 2048, 2048, 2)]],
    *[({"PDHG_RES64": "0"}, c, 8, 1, {"res64": 0}) for c in [(1, 2, 8, 2048, 3), (3, 2, 8, 2048, 2)]],
    # ... DUAL_CASES x k in (1, 3): the LDS-row dual for k = 1, nx % 8 == 0, T >= 3
    *[({"PDHG_DUAL64": "1"}, c, 8, k, {"dual64": 1, "fast_dual": 8 if (k == 1 and c[2] % 8 == 0 and c[4] >= 3) else 0})
      for k in (1, 3) for c in [(1, 2, 6, 256, 3), (2, 2, 5, 512, 3), (3, 2, 4, 256, 2), (1, 2, 16, 256, 3),
                                (2, 2, 24, 512, 4), (3, 2, 16, 256, 2)]],
    *[({"PDHG_DUAL64": "0"}, (1, 2, 16, 256, 3), 8, k, {"dual64": 0}) for k in (1, 3)],
    # ... test_res64_threads, test_update_t1_shapes
    *[({"PDHG_RES64_NT2048": nt}, c, 8, 1, {"res64_nt": int(nt)}) for nt in ("256", "512")
      for c in [(1, 2, 8, 2048, 3), (2, 2, 12, 2048, 2), (3, 2, 8, 2048, 2), (2, 2, 2048, 2048, 2)]],
    *[({"PDHG_UPD_T1": v}, c, 8, 1, {"upd_t1": int(v)}) for v in ("1", "2", "0")
      for c in [(1, 2, 8, 2048, 1), (2, 2, 2048, 2048, 1)]],
    # test_gpu_xt64
    *[({"PDHG_XT64": f}, c, 8, 1, {"f64_xt": int(f)}) for f in ("1", "0")
      for c in [(1, 2, 512, 256, 12), (2, 2, 1024, 256, 9), (2, 2, 2048, 128, 7)]],
    *[({"PDHG_FUSE_RES": fr, "PDHG_TC_SPEC": f}, (2, 2, 4096, 4096, T), 8, 1, {"tc_spec": int(f), "fused_residual": int(fr)})
      for fr, T in (("1", 6), ("0", 6), ("1", 4)) for f in ("1", "0")],
    # test_gpu_fused: FUSED64 fused / unfused, the C4 plane
    *[(dict(FR, PDHG_FUSE_RES="1"), c, 8, 1, {"fused_residual": 1, "dual_ypl": 2, ("res64" if c[3] < 8192 else "ip_rows"): 1})
      for c in [(2, 2, 32, 2048, 4), (1, 2, 16, 2048, 3), (2, 2, 24, 4096, 2), (2, 2, 32, 8192, 3), (1, 2, 24, 8192, 2),
                (2, 2, 8192, 8192, 3)]],
    *[(dict(FR, PDHG_FUSE_RES="0"), c, 8, 1, {"fused_residual": 0}) for c in [(2, 2, 32, 2048, 4), (2, 2, 8192, 8192, 3)]],
    *[({"PDHG_UPD8192": f}, (2, 2, 8192, 8192, 3), 8, 1, {"upd8192": int(f), "half_real": 1}) for f in ("1", "0")],
    *[(dict(FR, PDHG_FUSE_RES="1", PDHG_C4_TO=f), (2, 2, 8192, 8192, 3), prec, 1, {"to_c4": int(f), "half_real": 1})
      for f in ("1", "0") for prec in (8, 4)],
    # test_gpu_parity: the one-row x transform (fp32 / fp64, G16 at nx = 2048 / 4096), fp64 nx = 4096, the 1-D paths
    *[({}, c, 4, 1, {"fast_xt": 1}) for c in [(1, 2, 4096, 256, 1), (2, 2, 2048, 256, 1), (2, 2, 1024, 512, 1),
                                              (1, 2, 512, 256, 1)]],
    *[({"PDHG_T1_XT": t1, "PDHG_T1_G16": g}, c, 8, 1,
       {"t1_xt64": int(t1), "t1_g16": int(t1 == "1" and g == "1" and c[2] in (2048, 4096))})
      for t1, g in (("1", "1"), ("0", "1"), ("1", "0"))
      for c in [(1, 2, 4096, 256, 1), (2, 2, 2048, 256, 1), (2, 2, 1024, 512, 1), (1, 2, 512, 256, 1)]],
    *[({}, c, 8, 1, {"f64_xt": 1}) for c in [(2, 2, 4096, 16, 6), (1, 2, 4096, 32, 3), (2, 2, 4096, 8, 1)]],
    *[({"PDHG_FUSE_RES1D": f}, (egno, 1, 65536, 1, T), prec, 1, {"fused_residual": int(f), "fs16": 1})
      for f in ("1", "0") for prec in (8, 4) for egno, T in ((1, 100), (2, 13), (1, 1))],
    # ... the marching contexts (T = 1 windows, rho_alp_iters = 10, 256^2): speculative schedule, one-row dual
    ({"PDHG_SPEC": "1"}, (1, 2, 256, 256, 1), 8, 10, {"spec": 1, "dual_head": 1, "dual_multi": 0}),
    ({"PDHG_SPEC": "0"}, (1, 2, 256, 256, 1), 8, 10, {"spec": 0, "dual_head": 1}),
    ({"PDHG_DUAL_HEAD": "0"}, (1, 2, 256, 256, 1), 8, 10, {"spec": 0, "dual_head": 0}),
    ({"PDHG_K1_OUTER": "0"}, (1, 2, 256, 256, 1), 8, 10, {"spec": 0, "dual_head": 1}),
    *[({"PDHG_DUAL_ONE": v}, (1, 2, 256, 256, 1), 8, 10, {"dual_one": int(v != "0")}) for v in ("1", "2", "0")],
]


@pytest.mark.parametrize("i", range(len(FP64)), ids=["{}-{}x{}T{}p{}k{}".format(i, c[1][2], c[1][3], c[1][4], c[2], c[3])
                                                     for i, c in enumerate(FP64)])
def test_fp64_and_parity_cases(lib, monkeypatch, i):
    env, shape, precision, k, expect = FP64[i]
    _check(lib, monkeypatch, env, shape, expect, precision=precision, k=k)


FUSE = {"PDHG_FUSE_RES": "1"}
# The kernel choices ("<stage>_kernel" family codes of include/pdhg.h, "<stage>_shape" threads): every family of every
# stage at least once, at the smallest shapes that select it.  (environment, (egno, ndim, nx, ny, T), precision, expected)
CHOICES = [
    # x transform of a window: single-role, warp-specialised, batched, DMA, DMA half-real, fp64, generic
    ({}, (1, 2, 4096, 32, 3), 4, {"xt_kernel": 1, "xt_shape": 512, "fast_xt": 1, "xt_one_row_kernel": 0}),
    ({"PDHG_XT_WS": "1"}, (1, 2, 4096, 32, 3), 4, {"xt_kernel": 2, "xt_shape": 512, "fast_xt": 2}),
    ({}, (1, 2, 2048, 32, 4), 4, {"xt_kernel": 3, "xt_shape": 1024, "fast_xt": 3}),
    ({}, (1, 2, 4096, 32, 4), 4, {"xt_kernel": 4, "xt_shape": 1024, "fast_xt": 4}),
    ({}, (1, 2, 8192, 32, 4), 4, {"xt_kernel": 5, "xt_shape": 1024, "fast_xt": 5, "half_real": 1}),
    ({}, (1, 2, 4096, 32, 3), 8, {"xt_kernel": 6, "xt_shape": 512, "fast_xt": 0, "f64_xt": 1, "xt64_dma": 1}),
    ({}, (1, 2, 15, 17, 3), 4, {"xt_kernel": 7, "res_kernel": 1, "upd_kernel": 1, "dual_kernel": 1, "dual_shape": 256,
                                "res_fused_kernel": 0, "dual_fused_kernel": 0}),
    ({}, (1, 2, 15, 17, 3), 12, {"xt_kernel": 7, "res_kernel": 1, "upd_kernel": 2, "dual_kernel": 2}),
    # one-row windows: the fp32 kernel at the marching defaults' shapes (c3w1, c2w1; "fast_xt" keeps the window
    # kernel's code), fp64 without and with G16
    *[({}, (1, 2, n, n, 1), 4, {"xt_one_row_kernel": 8, "xt_one_row_shape": 512, "fast_xt": 1, "xt_kernel": 1})
      for n in (4096, 2048)],
    ({}, (1, 2, 1024, 32, 1), 8, {"xt_one_row_kernel": 9, "xt_one_row_shape": 512, "t1_xt64": 1, "t1_g16": 0}),
    ({}, (1, 2, 2048, 32, 1), 8, {"xt_one_row_kernel": 10, "xt_one_row_shape": 256, "t1_xt64": 1, "t1_g16": 1}),
    # rows and dual, fp32: fast rows with the LDS sweep, fused, and the row-per-thread sweep on a one-row window
    ({}, (1, 2, 16, 256, 3), 4, {"res_kernel": 2, "res_shape": 64, "res_fused_kernel": 0, "upd_kernel": 3, "upd_shape": 64,
                                 "dual_kernel": 5, "dual_shape": 512, "dual_fused_kernel": 0}),
    (FUSE, (1, 2, 16, 256, 3), 4, {"res_fused_kernel": 4, "res_fused_shape": 64, "dual_fused_kernel": 6,
                                   "dual_fused_shape": 512, "fused_residual": 1}),
    ({}, (1, 2, 16, 256, 1), 4, {"dual_kernel": 3, "dual_shape": 64, "dual_one": 1}),
    # mixed: fast rows at 512 threads, row-per-thread dual
    ({}, (1, 2, 16, 4096, 3), 12, {"res_kernel": 2, "upd_kernel": 4, "upd_shape": 512, "dual_kernel": 4}),
    # fp64 rows: 4-row kernels, the one-row update, task pairs, ny = 8192; fused, and PDHG_RES64_NT=1024
    ({}, (1, 2, 16, 2048, 3), 8, {"res_kernel": 3, "res_shape": 512, "upd_kernel": 5, "upd_shape": 512, "dual_kernel": 5}),
    ({}, (1, 2, 16, 2048, 1), 8, {"res_kernel": 3, "res_shape": 256, "upd_kernel": 6, "upd_shape": 256, "upd_t1": 2,
                                  "dual_kernel": 3}),
    ({"PDHG_UPD_PAIR": "1"}, (1, 2, 16, 2048, 3), 8, {"upd_kernel": 7, "upd_shape": 512, "upd64_pair": 1}),
    ({}, (1, 2, 8192, 8192, 3), 8, {"upd_kernel": 8, "upd_shape": 512, "res_kernel": 1, "upd8192": 1}),
    (FUSE, (1, 2, 16, 4096, 3), 8, {"res_fused_kernel": 5, "res_fused_shape": 512, "res64_nt": 512, "dual_fused_kernel": 6}),
    (dict(FUSE, PDHG_RES64_NT="1024"), (1, 2, 16, 4096, 3), 8, {"res_fused_kernel": 5, "res_fused_shape": 1024,
                                                                "res64_nt": 1024, "res_shape": 512}),
    # 1-D: no 2-D stage
    ({}, (1, 1, 4096, 1, 3), 4, {"xt_kernel": 0, "res_kernel": 0, "upd_kernel": 0, "dual_kernel": 0}),
]
FAMILIES = {"xt": range(1, 8), "xt_one_row": (0, 8, 9, 10), "res": range(0, 4), "res_fused": (0, 4, 5), "upd": range(0, 9),
            "dual": range(0, 6), "dual_fused": (0, 6)}


@pytest.mark.parametrize("i", range(len(CHOICES)), ids=["{}-{}x{}T{}p{}".format(i, c[1][2], c[1][3], c[1][4], c[2])
                                                        for i, c in enumerate(CHOICES)])
def test_kernel_choices(lib, monkeypatch, i):
    env, shape, precision, expect = CHOICES[i]
    _check(lib, monkeypatch, env, shape, expect, precision=precision)


def test_kernel_choice_table_reaches_every_family():
    for stage, codes in FAMILIES.items():
        seen = {c[3][stage + "_kernel"] for c in CHOICES if stage + "_kernel" in c[3]}
        assert seen >= set(codes), (stage, sorted(set(codes) - seen))


def test_runtime_keys_need_a_context(lib):
    p, keep = _problem(lib, 1, 2, 256, 256, 3)
    v = ctypes.c_int(0)
    for key in RUNTIME_KEYS + ("no_such_key",):
        assert lib.load().pdhg_plan_info(ctypes.byref(p), key.encode(), ctypes.byref(v)) == lib.PDHG_ERR_ARG, key
        assert lib.load().pdhg_last_error().decode()


@pytest.mark.parametrize("kw,code", [({"egno": 4}, "ARG"), ({"ndim": 3}, "ARG"), ({"T": 0}, "ARG"), ({"precision": 2}, "ARG"),
                                     ({"nx": 2}, "ARG"), ({"rho_alp_iters": 0}, "ARG"), ({"dt": 0.0}, "ARG"),
                                     ({"bc_y": 1}, "UNSUPPORTED"), ({"nx": 16384}, "UNSUPPORTED")])
def test_invalid_problem_same_code_as_create(lib, kw, code):
    """The shared validation (and the plan's own PDHG_ERR_UNSUPPORTED: nx beyond the x-transform slab): pdhg_create
    returns the same status where it gets that far without a device."""
    L = lib.load()
    p, keep = _problem(lib, 1, 2, 256, 256, 3, kw=kw)
    v, h = ctypes.c_int(0), ctypes.c_void_p()
    want = getattr(lib, "PDHG_ERR_" + code)
    assert L.pdhg_plan_info(ctypes.byref(p), b"fast_rows", ctypes.byref(v)) == want
    assert L.pdhg_last_error().decode()
    if "nx" not in kw or kw["nx"] < 3 or lib.device_count() > 0:   # the plan runs after the device check in pdhg_create
        assert L.pdhg_create(ctypes.byref(p), 0, ctypes.byref(h)) == want
    assert L.pdhg_plan_info(None, b"fast_rows", ctypes.byref(v)) == lib.PDHG_ERR_ARG


def test_environment_is_read_in_one_file():
    """Every getenv of csrc/ lives in tuning.hpp (Tuning / IterTuning / MultiTuning)."""
    hits = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*"))
                  if os.path.isfile(f) and "getenv(" in open(f, errors="replace").read())
    assert hits == ["tuning.hpp"], hits
