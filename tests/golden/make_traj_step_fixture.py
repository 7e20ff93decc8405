"""x_final of one small device-noise rollout per precision on a single context, recorded on the GPU at the commit
BEFORE the trajectory kernels gained their global step offset (TrajP::step0, csrc/kernels_traj.hpp).

A single context runs with step0 = 0, so the kernels must go on producing exactly these values: the fixture pins the
Philox counter's step word (step0 + ind), the staged-noise and record rows, and the position arithmetic, bit for
bit (tests/test_gpu_multi_traj.py::test_single_context_reproduces_recorded_paths).  The inputs are stored next to
the results, so the test needs nothing but the file.

Case: egno 1, 2-D 16 x 12 grid on [0, 2)^2, T = 4, dt = 0.1, epsl = 0.1, the random controls and the off-grid starts
of tests/_traj_support.py, linear and nearest interpolation, device noise with both key words, a sample offset past
2^32 (both sample counter words) and records on.

Run on a machine with a GPU, from a checkout of that commit with the library built:
    python tests/golden/make_traj_step_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (os.path.join(ROOT, "pdhg-optimal-control_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import _traj_support as S  # noqa: E402

EPSL = 0.1
SEED = (0x9e3779b9 << 32) | 20261020
OFFSET = (1 << 32) + 5
OUT = os.path.join(HERE, "traj_step0_single_e1_16x12_T4.npz")


def run(precision, method):
    """(traj_alp, traj_x, x_final) of the recorded call on a fresh single context."""
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, precision, EPSL)
    try:
        S.load_alp(ctx, S.random_alp(P))
        return ctx.trajectories(P["x0"], method, S.P_SPACE, S.P_SPACE, seed=SEED, sample_offset=OFFSET)
    finally:
        ctx.close()


def main(out):
    d = {"x0": S.problem(1, 2)["x0"], "alp": S.random_alp(S.problem(1, 2)),
         "seed_lo": np.uint64(SEED & 0xFFFFFFFF), "seed_hi": np.uint64(SEED >> 32), "offset": np.uint64(OFFSET)}
    for precision in ("fp32", "fp64"):
        for method in ("linear", "nearest"):
            ta, tx, xf = run(precision, method)
            assert np.isfinite(xf).all() and np.array_equal(tx[-1], xf)
            d["x_final/{}/{}".format(precision, method)] = xf
            d["traj_x/{}/{}".format(precision, method)] = tx
            d["traj_alp/{}/{}".format(precision, method)] = ta
    np.savez(out, **d)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
