"""Closed-loop trajectories on the device (include/pdhg.h pdhg_trajectories, csrc/kernels_traj.hpp) against the
per-sample oracle restatement of run_example.py:18-155 (oracle/traj_oracle.py).

The state is set directly (random alp with the dead components zero, rho = 1, phi = 0), so only the rollout runs.
The oracle is fed the alp get_state returns: the float rounding of the stored controls is on both sides and the
comparison is fp64 against fp64, held to the bound the NumPy trajectory module meets against the same oracle
(rtol 1e-11, atol 1e-12, tests/test_trajectories.py)."""
import ctypes

import numpy as np
import pytest

import _traj_support as S

pytestmark = pytest.mark.gpu

PARITY = [(1, e, m, p) for e, m in S.CASES_1D for p in ("fp32", "fp64")] + \
         [(2, e, m, p) for e, m in S.CASES_2D for p in ("fp32", "fp64")] + [(2, 2, "nearest", "mixed")]


def _check(name, got, ref):
    dev = S.deviation(got, ref)
    print("{}: max |got - ref| / (atol + rtol |ref|) = {:.3e}".format(name, dev))
    assert np.allclose(got, ref, rtol=S.RTOL, atol=S.ATOL), (name, dev)


@pytest.mark.parametrize("epsl", [0.0, 0.1])
@pytest.mark.parametrize("ndim,egno,method,precision", PARITY,
                         ids=["{}d_e{}_{}_{}".format(*c) for c in PARITY])
def test_rollout_matches_oracle(native, ndim, egno, method, precision, epsl):
    P = S.problem(egno, ndim)
    x0 = P["x0"]
    ctx = S.make_ctx(P, precision, epsl)
    try:
        S.load_alp(ctx, S.random_alp(P))
        alp = np.stack(ctx.get_state(phi=False, rho=False)[2])
        assert np.array_equal(alp, S.rounded(S.random_alp(P), precision))
        noise = S.noise_for(P, len(x0)) if epsl > 0 else None
        ref_a, ref_x = S.oracle_traj(P, alp, x0, epsl, method, noise)
        S.assert_margins(P, alp, ref_x, method)
        ta, tx, xf = ctx.trajectories(x0, method, S.P_SPACE, S.P_SPACE if ndim == 2 else None, P["center"], noise)
    finally:
        ctx.close()
    assert ta.shape == ref_a.shape and tx.shape == ref_x.shape and xf.shape == ref_x[-1].shape
    _check("traj_x", tx, ref_x)
    _check("traj_alp", ta, ref_a)
    _check("x_final", xf, ref_x[-1])
    assert np.array_equal(xf, tx[-1]) and np.array_equal(tx[0], x0)


def test_rollout_reads_current_alp_set(native):
    """rho_alp_iters > 1 keeps two rho / alp sets and the index of the current one on the device: the rollout reads
    the set get_state reads."""
    import pdhg_oracle as O
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, "fp64", 0.1, rho_alp_iters=2)
    try:
        ctx.init_state(O.set_up_J(1, 2, (S.P_SPACE, S.P_SPACE))(P["x_arr"])[0])
        st = ctx.iterate(3, 0.1 / 1.5, 0.1 * 1.5, -1.0, 2)
        assert st["iters_run"] == 3
        alp = np.stack(ctx.get_state(phi=False, rho=False)[2])
        assert np.abs(alp).max() > 0
        noise = S.noise_for(P, len(P["x0"]))
        ref_a, ref_x = S.oracle_traj(P, alp, P["x0"], 0.1, "linear", noise)
        S.assert_margins(P, alp, ref_x, "linear")
        ta, tx, xf = ctx.trajectories(P["x0"], "linear", S.P_SPACE, S.P_SPACE, noise=noise)
    finally:
        ctx.close()
    _check("traj_x", tx, ref_x)
    _check("traj_alp", ta, ref_a)
    _check("x_final", xf, ref_x[-1])


def test_windows_chain_through_x_final(native):
    """x_final of one window is x_init of the next: rows [2, 4) then rows [0, 2) of a 4-row alp (control time runs
    against PDE time) give the 4-row rollout bit for bit."""
    P = S.problem(1, 2)
    alp = S.random_alp(P)
    x0, noise = P["x0"], S.noise_for(P, len(P["x0"]))
    whole, late, early = S.make_ctx(P, "fp32", 0.1), S.make_ctx(P, "fp32", 0.1, T=2), S.make_ctx(P, "fp32", 0.1, T=2)
    try:
        S.load_alp(whole, alp)
        S.load_alp(late, alp[:, 2:4])
        S.load_alp(early, alp[:, 0:2])
        ta, tx, xf = whole.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, noise=noise)
        ta1, tx1, xf1 = late.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, noise=noise[:2])
        ta2, tx2, xf2 = early.trajectories(xf1, "linear", S.P_SPACE, S.P_SPACE, noise=noise[2:])
    finally:
        for c in (whole, late, early):
            c.close()
    assert np.array_equal(xf2, xf)
    assert np.array_equal(np.concatenate([tx1, tx2[1:]]), tx) and np.array_equal(np.concatenate([ta1, ta2]), ta)


@pytest.mark.parametrize("ndim,egno,method", [(1, 2, "nearest"), (2, 1, "linear")])
def test_null_records_leave_x_final_unchanged(native, ndim, egno, method):
    P = S.problem(egno, ndim)
    ctx = S.make_ctx(P, "fp32", 0.1)
    try:
        S.load_alp(ctx, S.random_alp(P))
        yp = S.P_SPACE if ndim == 2 else None
        noise = S.noise_for(P, len(P["x0"]))
        ta, tx, xf = ctx.trajectories(P["x0"], method, S.P_SPACE, yp, noise=noise)
        na, nx_, nf = ctx.trajectories(P["x0"], method, S.P_SPACE, yp, noise=noise, record=())
        oa, ox, of = ctx.trajectories(P["x0"], method, S.P_SPACE, yp, noise=noise, record=("alp",))
    finally:
        ctx.close()
    assert na is None and nx_ is None and ox is None
    assert np.array_equal(nf, xf) and np.array_equal(of, xf) and np.array_equal(oa, ta)


def _raw(ctx, n_sample, method):
    from pdhg_amd import _native as N
    o = N.pdhg_traj_opts()
    o.n_sample, o.method, o.x_period, o.y_period = n_sample, method, S.P_SPACE, S.P_SPACE
    x0 = np.zeros((max(n_sample, 1), 2))
    xf = np.empty_like(x0)
    rc = ctx._lib.pdhg_trajectories(ctx._h, ctypes.byref(o), N.dptr(x0), None, N.dptr(xf), None, None)
    return rc, ctx._lib.pdhg_last_error().decode()


def test_refusals(native):
    from pdhg_amd.slab import SlabContext
    from _problems import make_problem
    N = native
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, "fp32", 0.0)
    try:
        S.load_alp(ctx, S.random_alp(P))
        assert _raw(ctx, 4, 0)[0] == N.PDHG_OK
        for n_sample, method in ((0, 0), (4, 2), (4, -1)):
            rc, msg = _raw(ctx, n_sample, method)
            assert rc == N.PDHG_ERR_ARG and msg, (n_sample, method, rc, msg)
        x0 = np.zeros((2, 2))
        o = N.pdhg_traj_opts()
        o.n_sample, o.x_period, o.y_period = 2, 0.0, S.P_SPACE
        assert ctx._lib.pdhg_trajectories(ctx._h, ctypes.byref(o), N.dptr(x0), None, None, None, None) == N.PDHG_ERR_ARG
        o.x_period = S.P_SPACE
        assert ctx._lib.pdhg_trajectories(ctx._h, None, N.dptr(x0), None, None, None, None) == N.PDHG_ERR_ARG
        assert ctx._lib.pdhg_trajectories(ctx._h, ctypes.byref(o), None, None, None, None, None) == N.PDHG_ERR_ARG
    finally:
        ctx.close()
    Q = make_problem(1, 2, 512, 256, 6, 0.0)
    slab = SlabContext(0, 2, 6, 1, 512, 256, Q["dx"], Q["dy"], Q["dt"], Q["xs"], Q["ys"])
    try:
        rc, msg = _raw(slab, 4, 0)
        assert rc == N.PDHG_ERR_UNSUPPORTED and "slab" in msg
        with pytest.raises(N.PDHGUnsupported):
            slab.trajectories(np.zeros((4, 2)), "linear", S.P_SPACE, S.P_SPACE)
    finally:
        slab.close()


# ---- the device noise stream: alp = 0 (init_state), so the increments over sqrt(2 epsl dt) are the normals ----
EPS = 0.1


@pytest.fixture(scope="module")
def noise_ctx(native):
    import pdhg_oracle as O
    P = S.problem(1, 2)
    ctx = S.make_ctx(P, "fp32", EPS)
    ctx.init_state(O.set_up_J(1, 2, (S.P_SPACE, S.P_SPACE))(P["x_arr"])[0])
    yield ctx
    ctx.close()


def _normals(ctx, n, seed, offset=0):
    x0 = np.full((n, 2), 0.5)
    _, tx, _ = ctx.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, seed=seed, record=("x",), sample_offset=offset)
    return np.diff(tx, axis=0) / S.sqrt2epsdt(EPS, S.DT)


@pytest.fixture(scope="module")
def big_run(noise_ctx):
    return _normals(noise_ctx, 65536, 5)


def test_device_noise_is_the_documented_stream(noise_ctx):
    seed = (0x9e3779b9 << 32) | 12345          # both key words in use
    z = _normals(noise_ctx, 64, seed, offset=(1 << 32) + 7)     # and both sample counter words
    samples = (1 << 32) + 7 + np.arange(64, dtype=np.uint64)
    for step in range(4):
        z0, z1 = S.device_normals(seed, samples, step)
        _check("step {} axis 0".format(step), z[step, :, 0], z0)
        _check("step {} axis 1".format(step), z[step, :, 1], z1)


def test_device_noise_seed(noise_ctx):
    a, b, c = _normals(noise_ctx, 256, 3), _normals(noise_ctx, 256, 3), _normals(noise_ctx, 256, 4)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c) and np.abs(a - c).max() > 1.0


def test_device_noise_split_calls(noise_ctx, big_run):
    """One call of 65536 samples equals two calls of 32768 with the sample offset (positions compared bit for bit
    through the same quotient)."""
    lo, hi = _normals(noise_ctx, 32768, 5), _normals(noise_ctx, 32768, 5, offset=32768)
    assert np.array_equal(np.concatenate([lo, hi], axis=1), big_run)


def test_device_noise_statistics(big_run):
    """5-sigma bounds for n independent standard normals: mean 1/sqrt(n), variance sqrt(2/n), correlation 1/sqrt(n)."""
    z = big_run
    n = z.shape[1]
    m, v = z.mean(axis=1), z.var(axis=1)
    print("max |mean| {:.3e} (bound {:.3e}), max |var - 1| {:.3e} (bound {:.3e})".format(
        np.abs(m).max(), 5 / np.sqrt(n), np.abs(v - 1).max(), 5 * np.sqrt(2 / n)))
    assert np.abs(m).max() < 5 / np.sqrt(n)
    assert np.abs(v - 1).max() < 5 * np.sqrt(2 / n)
    zc = (z - m[:, None]) / np.sqrt(v)[:, None]
    steps = max(np.abs((zc[i] * zc[i + 1]).mean(axis=0)).max() for i in range(z.shape[0] - 1))
    axes = np.abs((zc[..., 0] * zc[..., 1]).mean(axis=1)).max()
    print("max |corr| consecutive steps {:.3e}, axes {:.3e} (bound {:.3e})".format(steps, axes, 5 / np.sqrt(n)))
    assert steps < 5 / np.sqrt(n) and axes < 5 / np.sqrt(n)


def test_sample_chunks_do_not_change_a_path(native):
    """More samples than one staging chunk holds (records on: 176 bytes per sample at T = 4 against the 64 MiB
    budget), with a supplied noise array: every chunk's rows of noise, traj_x and traj_alp land where the
    unchunked calls on the two halves put them."""
    P = S.problem(1, 2)
    n = 400000
    rng = np.random.default_rng(2)
    x0 = rng.uniform(-1.0, 3.0, (n, 2))
    noise = rng.standard_normal((P["T"], n, 2))
    ctx = S.make_ctx(P, "fp32", EPS)
    try:
        S.load_alp(ctx, S.random_alp(P))
        ta, tx, xf = ctx.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, noise=noise)
        h = n // 2
        parts = [ctx.trajectories(x0[a:b], "linear", S.P_SPACE, S.P_SPACE, noise=noise[:, a:b])
                 for a, b in ((0, h), (h, n))]
        da, dx_, df = ctx.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, seed=9)
        dparts = [ctx.trajectories(x0[a:b], "linear", S.P_SPACE, S.P_SPACE, seed=9, sample_offset=a)
                  for a, b in ((0, h), (h, n))]
    finally:
        ctx.close()
    for whole, halves in (((ta, tx, xf), parts), ((da, dx_, df), dparts)):
        assert np.array_equal(np.concatenate([halves[0][0], halves[1][0]], axis=1), whole[0])
        assert np.array_equal(np.concatenate([halves[0][1], halves[1][1]], axis=1), whole[1])
        assert np.array_equal(np.concatenate([halves[0][2], halves[1][2]], axis=0), whole[2])
