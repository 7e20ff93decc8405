"""Host side of the device trajectories (CPU): the wrapper refuses bad shapes and methods before any native call,
run_trajectories_device draws its host noise in compute_traj_*'s order, and the NumPy restatement of the device
noise stream used by tests/test_gpu_traj.py reproduces Philox4x32-10's known answers."""
import ctypes

import numpy as np
import pytest

import _traj_support as S
from pdhg_amd import _native as N, context as C, set_fns, trajectories as TR


def test_philox_restatement_known_answers():
    for ctr, key, out in S.kat():
        assert tuple(int(v) for v in S.philox4x32_10(ctr, key)) == out
    z0, z1 = S.device_normals(1, np.arange(4096), 0)
    assert np.all(np.isfinite(z0)) and np.all(np.isfinite(z1))


def test_options_struct_layout():
    # 2 long long + 1 unsigned long long + 4 int + 2 double, no padding
    assert ctypes.sizeof(N.pdhg_traj_opts) == 3 * 8 + 4 * 4 + 2 * 8
    assert "pdhg_trajectories" in N.EXPORTS


class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call {} before the arguments were checked".format(name))


def _ctx(ndim, T=4):
    ctx = object.__new__(C.PDHGContext)     # no device: every native call is an error
    ctx._lib, ctx._h = _NoNative(), None
    ctx.ndim, ctx.T, ctx.n_ctrl = ndim, T, ndim
    return ctx


@pytest.mark.parametrize("ndim,kw", [
    (1, dict(x_init=np.zeros((3, 1)), method="linear", x_period=2.0)),                    # 1-D starts are [n]
    (2, dict(x_init=np.zeros(3), method="linear", x_period=2.0, y_period=2.0)),           # 2-D starts are [n, 2]
    (2, dict(x_init=np.zeros((3, 3)), method="linear", x_period=2.0, y_period=2.0)),
    (2, dict(x_init=np.zeros((0, 2)), method="linear", x_period=2.0, y_period=2.0)),      # no samples
    (1, dict(x_init=np.zeros(3), method="cubic", x_period=2.0)),
    (1, dict(x_init=np.zeros(3), method=0, x_period=2.0)),
    (1, dict(x_init=np.zeros(3), method="linear", x_period=0.0)),
    (2, dict(x_init=np.zeros((3, 2)), method="nearest", x_period=2.0)),                   # y_period missing
    (2, dict(x_init=np.zeros((3, 2)), method="nearest", x_period=2.0, y_period=-1.0)),
    (2, dict(x_init=np.zeros((3, 2)), method="linear", x_period=2.0, y_period=2.0, noise=np.zeros((4, 3)))),
    (2, dict(x_init=np.zeros((3, 2)), method="linear", x_period=2.0, y_period=2.0, noise=np.zeros((5, 3, 2)))),
    (1, dict(x_init=np.zeros(3), method="linear", x_period=2.0, noise=np.zeros((4, 2)))),
    (1, dict(x_init=np.zeros(3), method="linear", x_period=2.0, record=("x", "rho"))),
    (1, dict(x_init=np.zeros(3), method="linear", x_period=2.0, seed=-1)),
    (1, dict(x_init=np.zeros(3), method="linear", x_period=2.0, sample_offset=-1)),
    (2, dict(x_init=np.zeros((3, 2)), method="linear", x_period=2.0, y_period=2.0, center=(True,))),
])
def test_wrapper_refuses_before_native(ndim, kw):
    with pytest.raises(ValueError):
        _ctx(ndim).trajectories(**kw)


def test_wrapper_arguments():
    o, x0, noise, rec_x, rec_a = C.traj_arguments(1, 4, [0.1, 0.2, 0.3], "nearest", 2.0, noise=np.ones((4, 3)),
                                                  record="x", seed=(1 << 64) - 1, sample_offset=5)
    assert (o.n_sample, o.method, o.sample_offset, o.seed) == (3, 1, 5, (1 << 64) - 1)
    assert x0.shape == (3, 1) and noise.shape == (4, 3, 1) and rec_x and not rec_a
    o, x0, noise, rec_x, rec_a = C.traj_arguments(2, 4, np.zeros((5, 2)), "linear", 2.0, 3.0, center=(True, False))
    assert (o.n_sample, o.method, o.center_x, o.center_y, o.x_period, o.y_period) == (5, 0, 1, 0, 2.0, 3.0)
    assert noise is None and rec_x and rec_a


class _Recorder:
    """Stands in for a context: answers trajectories() with the host functions on a host alp, the way the device
    does on its resident one."""

    def __init__(self, egno, ndim, alp, x_arr, dt, epsl, bc):
        self.egno, self.ndim, self.alp, self.x_arr, self.dt, self.epsl, self.bc = egno, ndim, alp, x_arr, dt, epsl, bc
        self.T = alp.shape[1]
        self.calls = []

    def trajectories(self, x_init, method, x_period, y_period=None, center=(False, False), noise=None, seed=0):
        self.calls.append(dict(method=method, center=tuple(center), noise=noise, seed=seed, y_period=y_period))
        it = iter(noise) if noise is not None else None

        class Replay:
            def normal(self, size):
                return next(it).reshape(size)
        fns = set_fns.set_up_example_fns(self.egno, self.ndim, 0)
        t_arr = np.arange(self.T + 1) * self.dt
        alp_c = self.alp[:, ::-1]
        rng = Replay() if noise is not None else None
        if self.ndim == 1:
            ta, tx = TR.compute_traj_1d(x_init, alp_c[..., 0], fns.f_fn, self.T + 1, self.x_arr[0, :, 0], t_arr,
                                        x_period, self.T * self.dt, self.epsl, method, rng=rng)
        else:
            ta, tx = TR.compute_traj_2d(x_init, alp_c, fns.f_fn, self.T + 1, self.x_arr[0, :, 0, 0],
                                        self.x_arr[0, 0, :, 1], t_arr, x_period, y_period, self.T * self.dt, self.bc,
                                        center, self.epsl, method, rng=rng)
        return ta, tx, tx[-1]


@pytest.mark.parametrize("egno,ndim", [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2)])
def test_run_trajectories_device_draws_noise_like_the_host(egno, ndim):
    P = S.problem(egno, ndim)
    alp, epsl, n = S.random_alp(P), 0.1, 3
    fns = set_fns.set_up_example_fns(egno, ndim, 0)
    t_arr = np.arange(P["T"] + 1) * P["dt"]
    ref_a, ref_x = TR.run_trajectories(egno, ndim, alp, fns, P["T"] + 1, P["x_arr"], t_arr, S.P_SPACE, S.P_SPACE,
                                       P["T"] * P["dt"], P["bc"], epsl, n, rng=np.random.default_rng(4))
    rec = _Recorder(egno, ndim, alp, P["x_arr"], P["dt"], epsl, P["bc"])
    ta, tx = TR.run_trajectories_device(rec, egno, ndim, S.P_SPACE, S.P_SPACE, epsl, n, rng=np.random.default_rng(4))
    call = rec.calls[0]
    assert call["method"] == ("nearest" if egno == 2 else "linear") and call["center"] == (egno == 3, egno == 3)
    assert call["noise"].shape == (P["T"], len(ref_x[0]), ndim)
    assert np.array_equal(tx, ref_x) and np.array_equal(ta, ref_a)
    # no generator: the device stream, keyed by the seed
    rec = _Recorder(egno, ndim, alp, P["x_arr"], P["dt"], 0.0, P["bc"])
    TR.run_trajectories_device(rec, egno, ndim, S.P_SPACE, S.P_SPACE, epsl, n, seed=17)
    assert rec.calls[0]["noise"] is None and rec.calls[0]["seed"] == 17
