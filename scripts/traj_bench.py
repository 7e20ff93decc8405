#!/usr/bin/env python
"""Time the device trajectory rollout (pdhg_trajectories) on a C2-shaped fp32 window.

    python scripts/traj_bench.py [--nx 2048 --ny 2048 --T 100 --iters 3 --epsl 0.1 --samples 10000 1000000]

alp comes from init_state plus a few PDHG iterations; only x_final is asked for, so no record is allocated.  Each
sample count is run `--repeat` times and the best wall time of the whole call is reported (staging x_init to the
device and x_final back included), as samples * steps / s and as the gather bandwidth that implies: per sample and
step the bilinear rollout reads 4 arrays x 4 corners in the context's precision.  Prints one JSON line per count.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=2048)
    ap.add_argument("--ny", type=int, default=2048)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--epsl", type=float, default=0.1)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--samples", type=int, nargs="+", default=[10 ** 4, 10 ** 6])
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args(argv)

    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import set_fns
    from pdhg_amd.context import PDHGContext

    P = 2.0
    xs = np.linspace(0.0, P, a.nx, endpoint=False)
    ys = np.linspace(0.0, P, a.ny, endpoint=False)
    ctx = PDHGContext(1, 2, a.nx, a.ny, a.T, P / a.nx, P / a.ny, 1.0 / a.T, xs, ys, epsl=a.epsl,
                      precision=a.precision)
    xm, ym = np.meshgrid(xs, ys, indexing="ij")
    ctx.init_state(set_fns.set_up_J(1, 2, (P, P))(np.stack([xm, ym], axis=-1)))
    ctx.iterate(a.iters, 0.1 / 1.5, 0.1 * 1.5, -1.0, 1)
    ctx.synchronize()
    word = 8 if a.precision == "fp64" else 4
    rng = np.random.default_rng(0)
    for n in a.samples:
        x0 = rng.uniform(0.0, P, (n, 2))
        best = float("inf")
        for rep in range(a.repeat + 1):      # the first call also uploads the grid: not timed
            t0 = time.perf_counter()
            _, _, xf = ctx.trajectories(x0, "linear", P, P, record=())
            dt = time.perf_counter() - t0
            if rep > 0:
                best = min(best, dt)
        assert np.all(np.isfinite(xf))
        rate = n * a.T / best
        print(json.dumps({"metric": "traj_rollout", "precision": a.precision, "nx": a.nx, "ny": a.ny, "T": a.T,
                          "epsl": a.epsl, "samples": n, "seconds": best, "sample_steps_per_s": rate,
                          "gather_GBps": rate * 16 * word / 1e9,
                          "mean_displacement": float(np.abs(xf - x0).mean())}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
