#!/usr/bin/env python
"""Time the staged read-back calls on a large window: pdhg_report_rows over the whole window (row chunks) and
pdhg_get_state (plane copies, the alp interleave).

    python scripts/staged_io_bench.py [--nx 4096 --ny 4096 --T 200 --precision fp64 --iters 2 --alp-T 8 --repeat 2]

The state comes from init_state plus a few PDHG iterations.  Each measurement is the best wall time of `--repeat` whole
calls after an untimed first one.  The reference layout of alp carries the dead components, 8 doubles per point and
row: at 4096^2 x 200 that is 215 GB of host memory, so get_state on the large window asks for phi and rho only and the
alp path is timed on a second context of --alp-T rows.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_bytes():
    """Host memory this process may still take: MemAvailable, or the memory cgroup's limit where that is lower."""
    avail = float("inf")
    with open("/proc/meminfo") as fh:
        for ln in fh:
            if ln.startswith("MemAvailable:"):
                avail = 1024.0 * int(ln.split()[1])
    try:
        with open("/sys/fs/cgroup/memory.max") as fh:
            v = fh.read().strip()
        if v != "max":
            avail = min(avail, float(v))
    except OSError:
        pass
    return avail


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--alp-T", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--epsl", type=float, default=0.1)
    ap.add_argument("--precision", default="fp64")
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args(argv)

    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import set_fns
    from pdhg_amd.context import PDHGContext

    P = 2.0
    xs = np.linspace(0.0, P, a.nx, endpoint=False)
    ys = np.linspace(0.0, P, a.ny, endpoint=False)
    xm, ym = np.meshgrid(xs, ys, indexing="ij")
    g = set_fns.set_up_J(1, 2, (P, P))(np.stack([xm, ym], axis=-1))
    del xm, ym

    def context(T):
        ctx = PDHGContext(1, 2, a.nx, a.ny, T, P / a.nx, P / a.ny, 1.0 / T, xs, ys, epsl=a.epsl,
                          precision=a.precision)
        ctx.init_state(g)
        ctx.iterate(a.iters, 0.1 / 1.5, 0.1 * 1.5, -1.0, 1)
        ctx.synchronize()
        return ctx

    def best_of(fn):
        best = float("inf")
        for rep in range(a.repeat + 1):
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            del out
            if rep > 0:
                best = min(best, dt)
        return best

    base = {"precision": a.precision, "nx": a.nx, "ny": a.ny}
    need = 2 * 8.0 * (a.T + 1) * a.nx * a.ny      # host bytes of either large call's result
    if host_bytes() < 3 * need:
        sys.exit("the large calls return {:.0f} GB each; this host offers {:.0f} GB".format(need / 1e9, host_bytes() / 1e9))
    ctx = context(a.T)
    sec = best_of(lambda: ctx.residual_rows(0, a.T))
    print(json.dumps(dict(base, T=a.T, metric="residual_rows_whole_window", seconds=sec,
                          gbytes_per_s=2 * 8.0 * a.T * a.nx * a.ny / sec / 1e9)), flush=True)
    sec = best_of(lambda: ctx.get_state(alp=False))
    print(json.dumps(dict(base, T=a.T, metric="get_state_phi_rho", seconds=sec)), flush=True)
    ctx.close()
    ctx = context(a.alp_T)
    sec = best_of(lambda: ctx.get_state())
    print(json.dumps(dict(base, T=a.alp_T, metric="get_state_with_alp", seconds=sec)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
