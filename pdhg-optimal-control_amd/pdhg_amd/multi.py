"""MultiContext: one PDHG window over a list of devices, driven by the library's own host thread.

The C ABI's multi-device context (include/pdhg.h, ``pdhg_create_multi``; SURVEY.md 8(b)'s
``pdhg_create(prob, devices, ndev)``) splits the window's T rows into one t-slab per listed device and
runs the slab choreography natively (``csrc/pdhg_multi.hpp``: device-to-device plane copies over xGMI on
per-slab side streams, per-neighbour events, fixed-order sum folds), so a caller needs no communicator.
``pdhg_amd.slab`` is the one-process-per-GPU form of the same algorithm (RCCL through torch.distributed),
used by ``bench.py --gpus N``.  Arrays are the whole window in the reference layouts, as for PDHGContext.

The handle is a ``pdhg_multi*``, not a ``pdhg_ctx*``: this class therefore does not derive from
PDHGContext, and offers only the whole-window calls the multi-device ABI has (state, iterate, stop rules,
synchronize, info, and the two read-only passes over the resident state: report / residual_rows and
trajectories, with PDHGContext's signatures and return values).  The library also rejects a foreign handle passed
to a ``pdhg_ctx`` entry point.  Like the rest of this context, the two passes have been run with every slab on one
device only (``devices=[0] * n``).
"""
import ctypes

import numpy as np

from . import _native as N
from .context import policy_arguments, traj_arguments


class MultiContext:
    def __init__(self, egno, nx, ny, T, dx, dy, dt, xs, ys, devices=(0, 0), epsl=0.0, c_on_rho=70.0,
                 precision="fp32", rho_alp_iters=1):
        if precision in ("mixed", 12):
            raise ValueError("precision 'mixed' is implemented for the single context (PDHGContext) only")
        if precision not in ("fp32", "fp64", 4, 8):
            raise ValueError("precision must be fp32 or fp64")
        self._lib = N.load()
        self.egno, self.ndim, self.nx, self.ny, self.T = int(egno), 2, int(nx), int(ny), int(T)
        self.n_ctrl = 1 if egno == 3 else 2
        self.n_alp = 4
        self.rho_alp_iters = int(rho_alp_iters)
        self._xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(-1)
        self._ys = np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
        bcx = 1 if egno == 3 else 0
        prob = N.pdhg_problem()
        prob.egno, prob.ndim, prob.bc_x, prob.bc_y = self.egno, 2, bcx, 0
        prob.nx, prob.ny, prob.T = self.nx, self.ny, self.T
        prob.precision = {"fp32": 4, "fp64": 8, 4: 4, 8: 8}[precision]   # fp64: the reference's arithmetic
        self.precision = precision
        prob.rho_alp_iters = self.rho_alp_iters
        prob.dx, prob.dy, prob.dt = float(dx), float(dy), float(dt)
        prob.epsl, prob.c_on_rho = float(epsl), float(c_on_rho)
        prob.C, prob.pow_, prob.Ct = 1.0, 1.0, 1.0
        prob.xs, prob.ys = N.dptr(self._xs), N.dptr(self._ys)
        self._prob = prob
        self._devices = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self._ndev = len(devices)
        h = ctypes.c_void_p()
        N.check(self._lib.pdhg_create_multi(ctypes.byref(prob), self._devices, self._ndev, ctypes.byref(h)))
        self._h = h

    @property
    def _space(self):
        return (self.nx, self.ny)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pdhg_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, phi=None, rho=None, alp=None):
        phi = None if phi is None else np.ascontiguousarray(phi, dtype=np.float64).reshape((self.T + 1,) + self._space)
        rho = None if rho is None else np.ascontiguousarray(rho, dtype=np.float64).reshape((self.T,) + self._space)
        if alp is not None:
            alp = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float64) for a in alp], axis=0))
            alp = alp.reshape((self.n_alp, self.T) + self._space + (self.n_ctrl,))
        N.check(self._lib.pdhg_multi_set_state(self._h, N.dptr(phi), N.dptr(rho), N.dptr(alp)))

    def init_state(self, g):
        """The reference initial state (phi = g on every row, rho = c_on_rho, alp = 0) on every slab."""
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self._space)
        N.check(self._lib.pdhg_multi_init_state(self._h, N.dptr(g)))

    def get_state(self):
        phi = np.empty((self.T + 1,) + self._space)
        rho = np.empty((self.T,) + self._space)
        alp = np.empty((self.n_alp, self.T) + self._space + (self.n_ctrl,))
        N.check(self._lib.pdhg_multi_get_state(self._h, N.dptr(phi), N.dptr(rho), N.dptr(alp)))
        return phi, rho, tuple(alp[i] for i in range(self.n_alp))

    def iterate(self, n_iters, tau, sigma, eps, rho_alp_iters):
        st = N.pdhg_stats()
        N.check(self._lib.pdhg_multi_iterate(self._h, int(n_iters), float(tau), float(sigma), float(eps),
                                             int(rho_alp_iters), ctypes.byref(st)))
        return {"iters_run": st.iters_run, "status": st.status, "inner_last": st.inner_last,
                "inner_total": st.inner_total, "err1": st.err1, "err2": st.err2, "err_inner": st.err_inner,
                "nan_seen": st.nan_seen, "first_nan_iter": st.first_nan_iter}

    # ---- read-only passes over the resident state (pdhg_multi_report_state / _report_rows / _trajectories) ----
    def report(self):
        """PDHGContext.report for the whole window: every slab's pass on its own device, the slabs' sums folded in
        slab order (a repeated call returns the same bits)."""
        r = N.pdhg_report()
        N.check(self._lib.pdhg_multi_report_state(self._h, ctypes.byref(r)))
        return {f: getattr(r, f) for f in N.REPORT_FIELDS}

    def residual_rows(self, row0, nrows, hj=True, cont=True):
        """PDHGContext.residual_rows over global rows [row0, row0 + nrows) (a range may span slabs)."""
        f = lambda on: np.empty((int(nrows),) + self._space) if on and nrows >= 1 else None  # noqa: E731
        h, c = f(hj), f(cont)
        N.check(self._lib.pdhg_multi_report_rows(self._h, int(row0), int(nrows), N.dptr(h), N.dptr(c)))
        return h, c

    def trajectories(self, x_init, method, x_period, y_period=None, center=(False, False), noise=None, seed=0,
                     record=("x", "alp"), sample_offset=0):
        """PDHGContext.trajectories through the window's T rows: the samples march through the slabs from the last
        to the first, handed on device to device.  (traj_alp [T, n, n_ctrl], traj_x [T+1, n, 2], x_final [n, 2])."""
        o, x0, noise, rec_x, rec_a = traj_arguments(2, self.T, x_init, method, x_period, y_period, center, noise,
                                                    record, seed, sample_offset)
        n = x0.shape[0]
        x_final = np.empty((n, 2))
        traj_x = np.empty((self.T + 1, n, 2)) if rec_x else None
        traj_alp = np.empty((self.T, n, self.n_ctrl)) if rec_a else None
        N.check(self._lib.pdhg_multi_trajectories(self._h, ctypes.byref(o), N.dptr(x0), N.dptr(noise),
                                                  N.dptr(x_final), N.dptr(traj_x), N.dptr(traj_alp)))
        return traj_alp, traj_x, x_final

    def policy_eval(self, x_init=None, stride=None, method="linear", x_period=2.0, y_period=None,
                    center=(False, False), noise=None, seed=0, sample_offset=0, terminal="phi0",
                    outputs=("running", "terminal", "value")):
        """PDHGContext.policy_eval's signature; the policy check runs on single contexts only, so after the argument
        checks the library refuses this handle (PDHGUnsupported)."""
        po, x0, noise, _, _ = policy_arguments(2, self.T, self.nx, self.ny, x_init, stride, method, x_period, y_period,
                                               center, noise, seed, sample_offset, terminal, outputs)
        r = N.pdhg_policy_report()
        N.check(self._lib.pdhg_policy_eval(self._h, ctypes.byref(po), N.dptr(x0), N.dptr(noise), ctypes.byref(r),
                                           None, None, None, None))
        raise AssertionError("pdhg_policy_eval accepted a multi-device handle")

    def set_stop_rules(self, converge=True, nan=True):
        N.check(self._lib.pdhg_multi_set_stop_rules(self._h, 1 if converge else 0, 1 if nan else 0))

    def synchronize(self):
        N.check(self._lib.pdhg_multi_synchronize(self._h))

    def info(self, key):
        v = ctypes.c_int()
        N.check(self._lib.pdhg_multi_info(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def phase_ms(self, reset=True):
        """{phase: total ms} recorded on slab 0's streams since profiling was switched on
        (pdhg_multi_profile): per-phase cost of the slab choreography."""
        out = {}
        for key in ("residual", "forward", "backward", "allreduce", "dual", "outer", "step"):
            ms = ctypes.c_double()
            n = ctypes.c_int()
            N.check(self._lib.pdhg_multi_phase_ms(self._h, key.encode(), ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[key] = ms.value
        if reset:
            N.check(self._lib.pdhg_multi_profile(self._h, 1))
        return out

    def profile(self, on=True):
        N.check(self._lib.pdhg_multi_profile(self._h, 1 if on else 0))
