#!/usr/bin/env python
"""Time the solution report (pdhg_report_state) next to the same context's dual sweep.

    python scripts/bench_report.py [--shapes c2:fp32 c2:fp64 c3:fp64] [--iters 3] [--out profiles]

Per shape (c2 = 2048^2 x 100, c3 = 4096^2 x 200; egno 1, epsl 0.1) and per kernel -- the tile kernel, then the
per-point one (PDHG_REPORT_TILE=0), one context at a time in this process -- the state comes from init_state plus a
few iterations, profiled, which gives the context's own "dual" class time (pdhg_profile_query).  The report is then
called 3 times untimed and 10 times timed with the context's HIP events around its launches (class "report": the
pass and its single-workgroup finalize); the median is reported with the algorithmic bytes of both (the report reads
phi, rho and the live alp arrays once and writes nothing) and the share of the 8 TB/s HBM peak they imply.  One JSON
line per shape goes to stdout and to <out>/report_<shape>_<precision>.json.  Needs a GPU: nothing falls back.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c2": (2048, 2048, 100), "c3": (4096, 4096, 200), "tiny": (64, 256, 4)}
PEAK = 8.0e12


def measure(nx, ny, T, prec, tile, iters):
    from pdhg_amd import set_fns
    from pdhg_amd.context import PDHGContext
    os.environ["PDHG_REPORT_TILE"] = "1" if tile else "0"   # read when the context is created
    P = 2.0
    xs, ys = np.linspace(0.0, P, nx, endpoint=False), np.linspace(0.0, P, ny, endpoint=False)
    ctx = PDHGContext(1, 2, nx, ny, T, P / nx, P / ny, 1.0 / T, xs, ys, epsl=0.1, precision=prec)
    try:
        assert ctx.path_info("report_tile") == (1 if tile else 0)
        xm, ym = np.meshgrid(xs, ys, indexing="ij")
        ctx.init_state(set_fns.set_up_J(1, 2, (P, P))(np.stack([xm, ym], axis=-1)))
        ctx.iterate(1, 0.1 / 1.5, 0.1 * 1.5, -1.0, 1)           # warm-up of the iteration's kernels
        ctx.profile_enable(True)
        ctx.iterate(iters, 0.1 / 1.5, 0.1 * 1.5, -1.0, 1)
        dual_ms, dual_n = ctx.profile_query("dual")
        ctx.profile_enable(False)
        for _ in range(3):
            rep = ctx.report()
        times = []
        for _ in range(10):
            ctx.profile_enable(True)    # resets the class counters
            again = ctx.report()
            ms, n = ctx.profile_query("report")
            assert n == 1 and again == rep
            times.append(ms)
        ctx.profile_enable(False)
        word, pword = (8, 8) if prec == "fp64" else (4, 8 if prec == "mixed" else 4)
        bytes_rep = float(nx) * ny * T * (5 * word + pword)
        return {"report_ms": statistics.median(times), "report_ms_min": min(times), "report_ms_max": max(times),
                "report_bytes": bytes_rep, "dual_ms": dual_ms / max(dual_n, 1), "dual_launches": dual_n,
                "dual_bytes": ctx.algorithmic_bytes(1, "dual"), "hj_max": rep["hj_max"], "cont_max": rep["cont_max"],
                "n_nonfinite": rep["n_nonfinite"]}
    finally:
        ctx.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["c2:fp32", "c2:fp64", "c3:fp64"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args(argv)
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    if _native.device_count() < 1:
        raise SystemExit("bench_report needs a GPU")
    os.makedirs(a.out, exist_ok=True)
    for item in a.shapes:
        shape, prec = item.split(":")
        nx, ny, T = SHAPES[shape]
        row = {"metric": "report_state", "shape": shape, "precision": prec, "nx": nx, "ny": ny, "T": T}
        for name, tile in (("tile", True), ("generic", False)):
            m = measure(nx, ny, T, prec, tile, a.iters)
            m["report_TBps"] = m["report_bytes"] / (m["report_ms"] * 1e-3) / 1e12
            m["report_share_of_peak"] = m["report_bytes"] / (m["report_ms"] * 1e-3) / PEAK
            m["dual_TBps"] = m["dual_bytes"] / (m["dual_ms"] * 1e-3) / 1e12
            row[name] = m
        row["tile_not_slower_than_generic"] = row["tile"]["report_ms"] <= row["generic"]["report_ms"]
        row["tile_not_slower_than_dual"] = row["tile"]["report_ms"] <= row["tile"]["dual_ms"]
        line = json.dumps(row)
        print(line, flush=True)
        with open(os.path.join(a.out, "report_{}_{}.json".format(shape, prec)), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
