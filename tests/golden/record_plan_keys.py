"""Record pdhg_plan_info over a grid of problems and environments (plan_keys_parent.json; no GPU needed).
usage: python tests/golden/record_plan_keys.py LIBPDHG_SO COMMIT > tests/golden/plan_keys_parent.json

A case is [precision, ndim, egno, nx, ny, T, rho_alp_iters] and one "NAME=value" environment setting ("" for none);
its record is the list of the values of KEYS, or the return code where the problem is refused.  tests/test_plan_keys.py
replays the file's cases through plan_values() against the current library."""
import ctypes
import json
import os
import sys

import numpy as np

# every creation-time key of pdhg_path_info / pdhg_plan_info at the recording commit
KEYS = ("fused_residual", "mixed", "fast_rows", "res64", "dual_multi", "dual_head", "spec", "dual64", "fast_dual",
        "dual_ypl", "res64_nt", "upd_t1", "t1_g16", "dual_one", "fast_xt", "half_real", "fourstep", "glb_line",
        "ip_rows", "upd8192", "upd64_pair", "upd_grid", "tc_spec", "to_c4", "thomas_chunk", "fs_wide", "fs16",
        "rows_rw", "row_threads", "res_threads", "upd_threads", "f64_xt", "xt64_dma", "xt64_bpr", "t1_xt64",
        "report_tile", "report_wgs")

# every variable Tuning::from_env reads, at its documented non-default values
ENVS = {
    "PDHG_ALLOC": ("contig", "none"), "PDHG_XT64": (0,), "PDHG_XT64_VAR": (1, 2, 3), "PDHG_XT64_DMA": (0,),
    "PDHG_XT64_BPR": (0, 1), "PDHG_T1_XT": (0,), "PDHG_T1_G16": (0,), "PDHG_SHORT_T_XT": (0,), "PDHG_XT_WS": (0, 1),
    "PDHG_XT_BATCH": (0, 1), "PDHG_XT_RPRE": (2,), "PDHG_XT_PAIR": (1,), "PDHG_XT_DMA": (0,), "PDHG_XT_DMA_HR": (0, 1),
    "PDHG_UPD_T1": (0, 1), "PDHG_RES64_NT2048": (256, 512), "PDHG_UPD8192": (0,), "PDHG_UPD_PAIR": (0, 1),
    "PDHG_UPD_PAIR_PF": (2, 3), "PDHG_UPD_GRID": (64,), "PDHG_ROWS_VAR": (1,), "PDHG_HALF_NT": (0, 1, 2),
    "PDHG_RES64_NT": (1024,), "PDHG_UPD_PF": (1, 2, 3), "PDHG_TILE_J": (1,), "PDHG_RES64": (0,), "PDHG_TC_SPEC": (0, 1),
    "PDHG_FUSE_RES": (0, 1), "PDHG_C4_TO": (0,), "PDHG_SHORT_T": (0,), "PDHG_DUAL64": (0,), "PDHG_DUAL_RX": (0, 4, 16),
    "PDHG_DUAL_YPL": (2,), "PDHG_DUAL_ONE": (0, 2), "PDHG_DUAL_NBSYNC": (1,), "PDHG_DUAL_ORDER": (0, 1, 2, 4),
    "PDHG_DBG": (1,), "PDHG_FOURSTEP": (0,), "PDHG_FS_WIDE": (0,), "PDHG_FS16": (0,), "PDHG_F16_GROUP": (4, 8),
    "PDHG_FUSE_RES1D": (0,), "PDHG_FR1D_CHUNKS": (4,), "PDHG_THOMAS_CHUNK": (0,), "PDHG_K1_OUTER": (0,),
    "PDHG_FOLD_FIN": (1,), "PDHG_G_OUTER": (1024,), "PDHG_HEAD_XRUN": (2,), "PDHG_DUAL_MULTI": (0, 1),
    "PDHG_DUAL_HEAD": (0,), "PDHG_SPEC": (0,), "PDHG_FIN_MERGE": (0,), "PDHG_REPORT_TILE": (0,), "PDHG_REPORT_WGS": (1,),
}

T_ALL = (1, 2, 3, 4, 8, 16, 25, 100, 200)
# (nx, ny): the squares, 16-row strips for the row and dual kernels, 32-column strips for the x kernels, a
# non-power-of-two pair and one with nx % 8 != 0
SHAPES_2D = [(n, n) for n in (256, 512, 1024, 2048, 4096, 8192)] + [(16, n) for n in (256, 2048, 4096, 8192)] + \
            [(n, 32) for n in (512, 1024, 2048, 4096, 8192)] + [(15, 17), (12, 2048)]
NX_1D = (256, 4096, 65536, 15)
# problems every environment setting is applied to: (precision, ndim, egno, nx, ny, T, rho_alp_iters)
ENV_PROBLEMS = [(4, 2, 1, 4096, 4096, 16, 1), (4, 2, 2, 2048, 2048, 1, 1), (4, 2, 1, 8192, 8192, 4, 1),
                (4, 2, 1, 16, 4096, 3, 1), (8, 2, 1, 4096, 4096, 100, 1), (8, 2, 2, 2048, 2048, 1, 1),
                (8, 2, 1, 4096, 4096, 1, 1), (8, 2, 1, 8192, 8192, 3, 1), (8, 2, 1, 2048, 32, 3, 1),
                (12, 2, 1, 16, 4096, 3, 1), (4, 1, 1, 65536, 1, 100, 1), (8, 1, 2, 65536, 1, 100, 1),
                (8, 2, 1, 256, 256, 1, 10)]


def cases():
    out = []
    for prec in (4, 8, 12):
        for nx, ny in SHAPES_2D:
            out += [((prec, 2, 1, nx, ny, T, 1), "") for T in T_ALL]
            out += [((prec, 2, 1, nx, ny, T, 10), "") for T in (1, 3, 100)]
            out += [((prec, 2, egno, nx, ny, T, 1), "") for egno in (2, 3) for T in (1, 3)]
        for nx in NX_1D:
            out += [((prec, 1, 1, nx, 1, T, 1), "") for T in T_ALL]
            out += [((prec, 1, 2, nx, 1, T, 10), "") for T in (1, 100)]
    for name, values in ENVS.items():
        out += [(p, "{}={}".format(name, v)) for v in values for p in ENV_PROBLEMS]
    return out


def load(path):
    """libpdhg.so at path through pdhg_amd._native (its struct and signatures)."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(here)), "pdhg-optimal-control_amd"))
    from pdhg_amd import _native
    _native.LIB_PATH = path
    return _native


def plan_values(native, problem, env, keys):
    """The values of keys for one case (a list), or pdhg_plan_info's return code; env: one "NAME=value" setting or a
    dict of settings.  The process environment is left as it was found."""
    prec, ndim, egno, nx, ny, T, k = problem
    xs, ys = np.linspace(0, 2, nx, endpoint=False), np.linspace(0, 2, ny, endpoint=False)
    p = native.pdhg_problem()
    p.egno, p.ndim, p.nx, p.ny, p.T, p.precision, p.rho_alp_iters = egno, ndim, nx, ny, T, prec, k
    p.bc_x = 1 if egno == 3 else 0
    p.dx, p.dy, p.dt, p.C, p.pow_, p.Ct, p.c_on_rho = 2 / nx, 2 / ny, 1.0 / max(T, 40), 1.0, 1.0, 1.0, 70.0
    p.xs, p.ys = native.dptr(xs), native.dptr(ys)
    saved = {n: os.environ.pop(n) for n in list(os.environ) if n.startswith("PDHG_")}
    setting = dict([env.split("=", 1)] if env else []) if isinstance(env, str) else dict(env)
    try:
        os.environ.update(setting)
        L, v, out = native.load(), ctypes.c_int(0), []
        for key in keys:
            rc = L.pdhg_plan_info(ctypes.byref(p), key.encode(), ctypes.byref(v))
            if rc != native.PDHG_OK:
                return rc
            out.append(v.value)
        return out
    finally:
        for name in setting:
            os.environ.pop(name, None)
        os.environ.update(saved)


def main():
    native = load(os.path.abspath(sys.argv[1]))
    rows = [json.dumps([list(p), env, plan_values(native, p, env, KEYS)], separators=(",", ":")) for p, env in cases()]
    print('{{"commit": "{}", "keys": {}, "cases": [\n{}\n]}}'.format(sys.argv[2], json.dumps(list(KEYS)), ",\n".join(rows)))


if __name__ == "__main__":
    main()
