"""bench.py --gpus N launches its own ranks (CPU, gloo): the driver's `bench.py --gpus N` without an
external torchrun must run N processes and report n_gpus = N (north_star: it/s at 1, 2, 4, 8 GPUs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(extra_env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_gpus2_launches_two_ranks():
    out = _run(["--gpus", "2", "--selftest"], {"PDHG_DIST_BACKEND": "gloo"})
    assert out == {"selftest": True, "n_gpus": 2, "ranks_seen": 2, "backend": "gloo"}


def test_gpus1_runs_in_process():
    out = _run(["--gpus", "1", "--selftest"])
    assert out["n_gpus"] == 1 and out["ranks_seen"] == 1


def test_gpus_mismatch_with_launcher_env_fails():
    env = {k: v for k, v in os.environ.items()}
    env.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--selftest"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_dump_sample_is_fixed_and_bounded():
    """--dump-outputs samples a large window the same way in every run (two builds are compared file for file) and
    keeps the whole dump of the largest config far below 64 MB; small windows are dumped whole."""
    sys.path.insert(0, ROOT)
    import bench
    rows, idx = bench.dump_sample(201, 4096 * 4096)
    rows2, idx2 = bench.dump_sample(201, 4096 * 4096)
    assert rows.tolist() == [0, 100, 200] and (idx == idx2).all() and (rows == rows2).all()
    assert len(idx) == bench.DUMP_POINTS and len(set(idx.tolist())) == len(idx)
    assert idx.min() >= 0 and idx.max() < 4096 * 4096 and (idx[1:] > idx[:-1]).all()
    rows, idx = bench.dump_sample(2, 160)
    assert rows.tolist() == [0, 1] and idx is None
    assert bench.dump_sample(1, 160)[0].tolist() == [0]
    # phi, rho and 4 controls of 2 components, float64, of the sampled rows
    assert bench.DUMP_ROWS * bench.DUMP_POINTS * 8 * (1 + 1 + 4 * 2) < 64e6


def test_dump_outputs_needs_the_single_gpu_context(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs",
                        str(tmp_path / "d")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--dump-outputs" in p.stderr and not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_state_it_ends_in(native, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` line carries the headline figures and none of the --full
    legs, and --dump-outputs writes the state after W + K iterations from the reference initial state: compared
    with the same iterations through a context of this process (the same kernels on the same inputs: equal)."""
    import numpy as np
    import bench
    from pdhg_amd.context import PDHGContext
    d = tmp_path / "dump"
    out = _run(["--gpus", "1", "--steps", "3", "--warmup", "2", "--config", "c0", "--dump-outputs", str(d)])
    assert out["steps"] == 3 and out["warmup"] == 2 and out["config"]["iters_executed"] == 3
    assert out["unit"] == "it/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3
    for key in ("cpu_baseline", "fp32_precision", "reference_precision", "finite_segment", "pmc_by_kernel"):
        assert key not in out
    assert out["config"]["first_nonfinite_iter"] is None and out["config"]["nonfinite_probe_iters"] == 0

    egno, ndim, epsl, nx, ny, nt = bench.CONFIGS["c0"]
    T = nt - 1
    xs, _ = bench.grid(ndim, nx, ny)
    ctx = PDHGContext(egno, ndim, nx, ny, T, 2.0 / nx, 0.0, 1.0 / T, xs, None, epsl=epsl, precision="fp64",
                      rho_alp_iters=1, device=0)
    ctx.init_state(np.sin(np.pi * xs))
    ctx.set_stop_rules(converge=True, nan=False)
    ctx.iterate(2, 0.1 / 1.5, 0.1 * 1.5, 1e-6, 1)
    st = ctx.iterate(3, 0.1 / 1.5, 0.1 * 1.5, 1e-6, 1)
    phi, rho, alp = ctx.get_state()
    ctx.close()
    rows_phi, idx = bench.dump_sample(T + 1, nx)
    rows_dual, _ = bench.dump_sample(T, nx)
    assert idx is None
    got = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))}
    assert sorted(got) == ["alp0", "alp1", "phi", "rho", "stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["phi"], phi[rows_phi]) and np.array_equal(got["rho"], rho[rows_dual])
    assert np.array_equal(got["alp0"], alp[0][rows_dual]) and np.array_equal(got["alp1"], alp[1][rows_dual])
    assert np.array_equal(got["stats"], np.array([float(st[k]) for k in bench.STAT_KEYS]))
    assert np.isfinite(got["phi"]).all() and np.abs(got["rho"] - 70.0).max() > 0.0   # the state moved


def _scale_worker(rank, world, port, out_path):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import bench
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{}".format(port), rank=rank, world_size=world)
    try:
        iters = 4
        # synthetic per-rank numbers: rank r is 1 ms slower per step, its exposed rho halo 0.1 * r ms per step
        kern = {c: {"avg_ms": 2.0 + i, "launches": iters} for i, c in enumerate(bench.KERNEL_CLASSES)}
        exch = {"halo_rho": 1.0, "exposed_halo_rho": 0.1 * rank, "exposed_carry_planes": 0.05, "allreduce": 0.02}
        rep = bench.scale_report(dist, "gloo", (20.0 + rank) * iters * 1e-3, iters, kern, exch)
        if rank == 0:
            with open(out_path, "w") as fh:
                json.dump(rep, fh)
    finally:
        dist.destroy_process_group()


def test_scale_report_gloo_world4(tmp_path):
    """The N > 1 bench line's self-check keys: world size as the process group reports it, per-rank
    step times and their max, kernel / exchange / exposed-wait times per rank, and the unexplained remainder --
    gathered over gloo at world size 4 with synthetic per-rank numbers."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "rep.json")
    mp.spawn(_scale_worker, args=(4, port, out), nprocs=4, join=True)
    with open(out) as fh:
        rep = json.load(fh)
    assert rep["world_size_reported"] == 4 and rep["backend"] == "gloo"
    assert rep["ms_per_step_by_rank"] == [20.0, 21.0, 22.0, 23.0]
    assert rep["ms_per_step_max"] == 23.0 and rep["slowest_rank"] == 3
    assert rep["kernel_ms_per_step_by_rank"]["dual"] == [5.0] * 4        # 2 + 3 ms per launch, one launch per step
    assert max(abs(a - 0.1 * r) for r, a in enumerate(rep["exchange_ms_per_step_by_rank"]["exposed_halo_rho"])) < 1e-12
    assert abs(rep["exposed_exchange_ms_by_rank"][2] - 0.25) < 1e-12
    assert abs(rep["unexplained_ms_by_rank"][3] - (23.0 - 14.0 - 0.35)) < 1e-9


def test_dual_passes_of_the_chunked_loop():
    """The chunked dual (kernels_dual_multi.hpp) moves one sub-iteration's bytes per pass: ceil(inner / 5) chunk
    passes + the final re-run when the exit falls inside a chunk -- what bench.py prices the dual class with, so no
    record reports more bytes than crossed HBM (frac 2.01 from bytes x inner count)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.dual_passes(10.0) == 2.0        # no early exit at k = 10: two chunks of 5
    assert bench.dual_passes(5.0) == 1.0
    assert bench.dual_passes(3.0) == 2.0         # exit inside the first chunk: chunk + final
    assert bench.dual_passes(7.0) == 3.0
    assert bench.dual_passes(1.0) == 2.0
