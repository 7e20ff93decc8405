#!/usr/bin/env python
"""Time the device policy check (pdhg_policy_eval) beside the rollout it shares its path with.

    python scripts/policy_bench.py [--nx 4096 --ny 4096 --T 200 --precision fp32 --iters 3 --epsl 0.1 --stride 1]

phi and alp come from init_state plus a few PDHG iterations.  Two measurements, each the best wall time of `--repeat`
whole calls after an untimed first one (a call ends in a stream synchronise):
  * grid starts: every --stride-th node, report only -- nothing is uploaded and one row of sums comes back;
  * --samples explicit starts with the device noise stream, every per-sample output asked for, beside
    pdhg_trajectories for the same starts asking for x_final only, the two alternated in this process (their
    x_final arrays are compared bit for bit).
Prints one JSON line per measurement.
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
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--epsl", type=float, default=0.1)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args(argv)

    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import set_fns
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.policy import format_policy

    P = 2.0
    xs = np.linspace(0.0, P, a.nx, endpoint=False)
    ys = np.linspace(0.0, P, a.ny, endpoint=False)
    ctx = PDHGContext(1, 2, a.nx, a.ny, a.T, P / a.nx, P / a.ny, 1.0 / a.T, xs, ys, epsl=a.epsl,
                      precision=a.precision)
    xm, ym = np.meshgrid(xs, ys, indexing="ij")
    ctx.init_state(set_fns.set_up_J(1, 2, (P, P))(np.stack([xm, ym], axis=-1)))
    del xm, ym
    ctx.iterate(a.iters, 0.1 / 1.5, 0.1 * 1.5, -1.0, 1)
    ctx.synchronize()
    base = {"precision": a.precision, "nx": a.nx, "ny": a.ny, "T": a.T, "epsl": a.epsl}

    def best_of(fn):
        out, best = None, float("inf")
        for rep in range(a.repeat + 1):      # the first call also uploads the grid: not timed
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if rep > 0:
                best = min(best, dt)
        return out, best

    rep, sec = best_of(lambda: ctx.policy_eval(stride=a.stride, x_period=P, y_period=P, seed=1, outputs=()))
    n = rep["n_sample"]
    print(json.dumps(dict(base, metric="policy_grid_starts", stride=a.stride, samples=n, seconds=sec,
                          samples_per_s=n / sec, sample_steps_per_s=n * a.T / sec, report=format_policy(rep))),
          flush=True)

    x0 = np.random.default_rng(0).uniform(0.0, P, (a.samples, 2))
    t_pol = t_traj = float("inf")
    for rep_i in range(a.repeat + 1):
        t0 = time.perf_counter()
        pol = ctx.policy_eval(x0, x_period=P, y_period=P, seed=1, outputs=("running", "terminal", "value", "x_final"))
        t1 = time.perf_counter()
        _, _, xf = ctx.trajectories(x0, "linear", P, P, seed=1, record=())
        t2 = time.perf_counter()
        if rep_i > 0:
            t_pol, t_traj = min(t_pol, t1 - t0), min(t_traj, t2 - t1)
    assert np.array_equal(pol["x_final"], xf)
    print(json.dumps(dict(base, metric="policy_explicit_starts", samples=a.samples, policy_seconds=t_pol,
                          trajectories_seconds=t_traj, policy_samples_per_s=a.samples / t_pol,
                          trajectories_samples_per_s=a.samples / t_traj, ratio=t_pol / t_traj)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
