"""PDHGContext: one PDHG time window resident in HBM, driven through the C ABI.

This is the object behind the reference-shaped functions in
``update_fns_in_pdhg`` and ``utils_pdhg_solver``.  All arrays crossing this
boundary are float64 NumPy arrays in the reference's layouts
(``utils_pdhg_solver.py:18-24``):

* phi  ``[T+1, nx]``            or ``[T+1, nx, ny]``
* rho  ``[T, nx]``              or ``[T, nx, ny]``
* alp  tuple of 2 ``[T, nx, 1]`` or 4 ``[T, nx, ny, n_ctrl]`` arrays
"""
import ctypes

import numpy as np

from . import _native as N


def traj_arguments(ndim, T, x_init, method, x_period, y_period=None, center=(False, False), noise=None,
                   record=("x", "alp"), seed=0, sample_offset=0):
    """Checked arguments of PDHGContext.trajectories, before any native call: (options struct, x_init [n, ndim],
    noise [T, n, ndim] or None, record_x, record_alp).  Raises ValueError on a shape or value the library would
    refuse, with the shapes spelled out."""
    if method not in N.TRAJ_METHODS:
        raise ValueError("method must be 'linear' or 'nearest', not {!r}".format(method))
    record = (record,) if isinstance(record, str) else tuple(record or ())
    if set(record) - {"x", "alp"}:
        raise ValueError("record takes 'x' and / or 'alp', not {!r}".format(record))
    x0 = np.ascontiguousarray(x_init, dtype=np.float64)
    want = "[n_sample]" if ndim == 1 else "[n_sample, 2]"
    if x0.ndim != ndim or (ndim == 2 and x0.shape[1] != 2) or x0.shape[0] < 1:
        raise ValueError("x_init must be {} with n_sample >= 1, not {}".format(want, x0.shape))
    n = x0.shape[0]
    if ndim == 2 and y_period is None:
        raise ValueError("y_period is required in 2-D")
    if not (x_period > 0) or (ndim == 2 and not (y_period > 0)):
        raise ValueError("periods must be > 0")
    if len(tuple(center)) != 2:
        raise ValueError("center is a pair (center_x, center_y)")
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
        if noise.shape not in ((T, n, ndim),) + (((T, n),) if ndim == 1 else ()):
            raise ValueError("noise must be [T, n_sample, ndim] = {}, not {}".format((T, n, ndim), noise.shape))
        noise = noise.reshape(T, n, ndim)
    if seed < 0 or seed >= 1 << 64 or sample_offset < 0:
        raise ValueError("seed must fit 64 unsigned bits and sample_offset be >= 0")
    o = N.pdhg_traj_opts()
    o.n_sample, o.sample_offset, o.seed, o.method = n, int(sample_offset), int(seed), N.TRAJ_METHODS[method]
    o.center_x, o.center_y = int(bool(center[0])), int(bool(center[1]))
    o.x_period, o.y_period = float(x_period), float(y_period if ndim == 2 else 0.0)
    return o, x0.reshape(n, ndim), noise, "x" in record, "alp" in record


POLICY_OUTPUTS = ("running", "terminal", "value", "x_final")


def policy_arguments(ndim, T, nx, ny, x_init, stride, method, x_period, y_period=None, center=(False, False),
                     noise=None, seed=0, sample_offset=0, terminal="phi0", outputs=("running", "terminal", "value")):
    """Checked arguments of PDHGContext.policy_eval, before any native call: (options struct, x_init [n, ndim] or None
    for grid starts, noise [T, n, ndim] or None, n, the outputs asked for).  Raises ValueError on a shape or value the
    library would refuse, with the shapes spelled out."""
    if terminal not in N.POLICY_TERMINAL:
        raise ValueError("terminal must be 'phi0' or 'none', not {!r}".format(terminal))
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs or ())
    if set(outputs) - set(POLICY_OUTPUTS):
        raise ValueError("outputs takes {}, not {!r}".format(" / ".join(POLICY_OUTPUTS), outputs))
    po = N.pdhg_policy_opts()
    po.terminal = N.POLICY_TERMINAL[terminal]
    if x_init is None:
        if stride is None:
            raise ValueError("give x_init [n_sample{}] or a stride for grid starts".format("" if ndim == 1 else ", 2"))
        st = (stride,) * ndim if np.ndim(stride) == 0 else tuple(stride)
        if len(st) != ndim or any(int(v) != v or v < 1 for v in st):
            raise ValueError("stride must be {} integer(s) >= 1, not {!r}".format(ndim, stride))
        st = tuple(int(v) for v in st)
        n = -(-nx // st[0]) * (-(-ny // st[1]) if ndim == 2 else 1)
        # the rollout's own checks, on a start array of the right length that is never uploaded
        x_chk = np.zeros((n,) + (() if ndim == 1 else (2,)))
        po.stride_x, po.stride_y = st[0], st[1] if ndim == 2 else 1
    else:
        if stride is not None:
            raise ValueError("stride selects grid starts: it cannot be combined with x_init")
        x_chk = x_init
        po.stride_x = po.stride_y = 1
    o, x0, noise, _, _ = traj_arguments(ndim, T, x_chk, method, x_period, y_period, center, noise, (), seed,
                                        sample_offset)
    po.traj = o
    return po, (None if x_init is None else x0), noise, x0.shape[0], outputs


class PDHGContext:
    def __init__(self, egno, ndim, nx, ny, T, dx, dy, dt, xs, ys=None, epsl=0.0, c_on_rho=70.0, bc=None,
                 C=1.0, pow=1.0, Ct=1.0, precision="fp32", rho_alp_iters=1, device=0):
        self._lib = N.load()
        if bc is None:
            bc = 0 if ndim == 1 else ((1, 0) if egno == 3 else (0, 0))
        bcx, bcy = (bc, 0) if ndim == 1 else tuple(bc)
        self.egno, self.ndim, self.nx, self.ny, self.T = int(egno), int(ndim), int(nx), int(ny if ndim == 2 else 1), int(T)
        self.n_ctrl = 1 if (ndim == 1 or egno == 3) else 2
        self.n_alp = 2 if ndim == 1 else 4
        self.precision = precision
        self._xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(-1)
        self._ys = None if ndim == 1 else np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
        prob = N.pdhg_problem()
        prob.egno, prob.ndim, prob.bc_x, prob.bc_y = self.egno, self.ndim, int(bcx), int(bcy)
        prob.nx, prob.ny, prob.T = self.nx, self.ny, self.T
        # "mixed" (12): fp32 state with fp64 phi / phi_bar; single 2-D contexts only (the subclasses refuse it)
        prob.precision = {"fp32": 4, "fp64": 8, "mixed": 12, 4: 4, 8: 8, 12: 12}[precision]
        prob.rho_alp_iters = int(rho_alp_iters)
        prob.dx, prob.dy, prob.dt = float(dx), float(dy if ndim == 2 else 0.0), float(dt)
        prob.epsl, prob.c_on_rho = float(epsl), float(c_on_rho)
        prob.C, prob.pow_, prob.Ct = float(C), float(pow), float(Ct)
        prob.xs = N.dptr(self._xs)
        prob.ys = N.dptr(self._ys) if self._ys is not None else None
        self.rho_alp_iters = int(rho_alp_iters)
        self._prob = prob
        if prob.precision == 12 and type(self)._create is not PDHGContext._create:
            raise ValueError("precision 'mixed' is implemented for the single context (PDHGContext) only")
        self._h = self._create(prob, int(device))
        self._version = 0         # bumped by every call that changes the device state
        self._resident = None     # (version, rho, alp): host arrays known to equal the device's rho / alp

    def _create(self, prob, device):
        h = ctypes.c_void_p()
        N.check(self._lib.pdhg_create(ctypes.byref(prob), device, ctypes.byref(h)))
        return h

    # ---- shapes ----
    @property
    def _space(self):
        return (self.nx,) if self.ndim == 1 else (self.nx, self.ny)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pdhg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----
    def alp_block(self, alp):
        """The contiguous [n_alp, T, ...space, n_ctrl] block a tuple of control arrays views (get_state returns such
        views), or None: lets set_state / the marching driver skip a stacking copy."""
        b = getattr(alp[0], "base", None) if len(alp) else None
        shape = (self.n_alp, self.T) + self._space + (self.n_ctrl,)
        if not (isinstance(b, np.ndarray) and b.dtype == np.float64 and b.flags.c_contiguous and b.shape == shape
                and len(alp) == self.n_alp):
            return None
        p0 = b.__array_interface__["data"][0]
        for i, a in enumerate(alp):
            if a.base is not b or a.shape != shape[1:] or a.__array_interface__["data"][0] != p0 + i * b.strides[0]:
                return None
        return b

    def set_state(self, phi=None, rho=None, alp=None):
        """Upload the given parts of the state (reference layouts); a part passed as None keeps the device's values."""
        phi = None if phi is None else np.ascontiguousarray(phi, dtype=np.float64).reshape((self.T + 1,) + self._space)
        rho = None if rho is None else np.ascontiguousarray(rho, dtype=np.float64).reshape((self.T,) + self._space)
        if alp is not None:
            blk = self.alp_block(alp)
            if blk is None:
                blk = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float64) for a in alp], axis=0))
            alp = blk.reshape((self.n_alp, self.T) + self._space + (self.n_ctrl,))
        self._version += 1
        N.check(self._lib.pdhg_set_state(self._h, N.dptr(phi), N.dptr(rho), N.dptr(alp)))

    def mark_resident(self, rho, alp):
        """rho / alp (host arrays the caller will not modify) equal the device's state now."""
        self._resident = (self._version, rho, tuple(alp))

    def is_resident(self, rho, alp):
        """True if rho / alp are the very arrays mark_resident recorded and the device state has not changed since."""
        r = self._resident
        return (r is not None and r[0] == self._version and rho is r[1] and alp is not None and
                len(alp) == len(r[2]) and all(a is b for a, b in zip(alp, r[2])))

    def get_state(self, phi=True, rho=True, alp=True):
        """(phi, rho, alp) from the device; a part passed as False is not copied and comes back as None."""
        phi = np.empty((self.T + 1,) + self._space) if phi else None
        rho = np.empty((self.T,) + self._space) if rho else None
        alp = np.empty((self.n_alp, self.T) + self._space + (self.n_ctrl,)) if alp else None
        N.check(self._lib.pdhg_get_state(self._h, N.dptr(phi), N.dptr(rho), N.dptr(alp)))
        return phi, rho, (None if alp is None else tuple(alp[i] for i in range(self.n_alp)))

    def get_rows(self, row0, nrows, phi=True, phi_bar=False, rho=True, alp=True):
        """Rows [row0, row0 + nrows) of (phi, phi_bar, rho, alp) in the reference layouts (pdhg_get_rows): for
        windows too large for a host copy of the whole state.  A part passed as False comes back as None."""
        sp = self._space
        f = lambda on: np.empty((nrows,) + sp) if on else None  # noqa: E731
        a = np.empty((self.n_alp, nrows) + sp + (self.n_ctrl,)) if alp else None
        ph, pb, rh = f(phi), f(phi_bar), f(rho)
        N.check(self._lib.pdhg_get_rows(self._h, int(row0), int(nrows), N.dptr(ph), N.dptr(pb), N.dptr(rh),
                                        N.dptr(a)))
        return ph, pb, rh, (None if a is None else tuple(a[i] for i in range(self.n_alp)))

    def get_phi_bar(self):
        pb = np.empty((self.T + 1,) + self._space)
        N.check(self._lib.pdhg_get_phi_bar(self._h, N.dptr(pb)))
        return pb

    def get_work(self, count):
        """The first `count` elements of the spectral work buffer (after update_primal: the preconditioner's output,
        blocked layout [T][nb][nx][B])."""
        out = np.empty(int(count))
        N.check(self._lib.pdhg_get_work(self._h, N.dptr(out), int(count)))
        return out

    def set_phi_bar(self, phi_bar):
        self._version += 1
        pb = np.ascontiguousarray(phi_bar, dtype=np.float64).reshape((self.T + 1,) + self._space)
        N.check(self._lib.pdhg_set_phi_bar(self._h, N.dptr(pb)))

    def init_state(self, g):
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self._space)
        self._version += 1
        N.check(self._lib.pdhg_init_state(self._h, N.dptr(g)))

    # ---- consumers of the controls ----
    def trajectories(self, x_init, method, x_period, y_period=None, center=(False, False), noise=None, seed=0,
                     record=("x", "alp"), sample_offset=0):
        """Closed-loop paths through this window's rows on the device (pdhg_trajectories; run_example.py:18-155):
        (traj_alp [T, n, n_ctrl], traj_x [T+1, n(, 2)], x_final [n(, 2)]) as compute_traj_1d / _2d, from the alp the
        device holds -- no host copy of it.  A record left out of `record` is neither allocated nor copied and comes
        back as None.  noise: standard normals [T, n, ndim] (the reference's per-step draws); None with epsl > 0 uses
        the device's counter-based generator keyed by `seed`, sample i of this call being stream sample
        sample_offset + i."""
        o, x0, noise, rec_x, rec_a = traj_arguments(self.ndim, self.T, x_init, method, x_period, y_period, center,
                                                    noise, record, seed, sample_offset)
        n = x0.shape[0]
        tail = () if self.ndim == 1 else (2,)
        x_final = np.empty((n,) + tail)
        traj_x = np.empty((self.T + 1, n) + tail) if rec_x else None
        traj_alp = np.empty((self.T, n, self.n_ctrl)) if rec_a else None
        N.check(self._lib.pdhg_trajectories(self._h, ctypes.byref(o), N.dptr(x0), N.dptr(noise), N.dptr(x_final),
                                            N.dptr(traj_x), N.dptr(traj_alp)))
        return traj_alp, traj_x, x_final

    def policy_eval(self, x_init=None, stride=None, method="linear", x_period=2.0, y_period=None,
                    center=(False, False), noise=None, seed=0, sample_offset=0, terminal="phi0",
                    outputs=("running", "terminal", "value")):
        """The policy check (pdhg_policy_eval): the closed-loop cost of the resident controls against phi.  Per sample
        value = phi row T at the start, running = sum dt L(alp) along trajectories()' own path, terminal = phi row 0
        at its end (terminal="none": 0.0, for chaining windows); gap = running + terminal - value.  Starts: x_init
        [n(, 2)], or stride (an int, or a pair in 2-D) for every stride-th grid node, sample index
        i * ceil(ny / stride_y) + j, with nothing uploaded.  phi is interpolated linearly whatever `method` the
        controls use.  Returns a dict: pdhg_policy_report's fields, the per-sample arrays named in `outputs` ([n]) and
        x_final [n(, 2)] when "x_final" is among them.  One read-only device pass."""
        po, x0, noise, n, outputs = policy_arguments(self.ndim, self.T, self.nx, self.ny, x_init, stride, method,
                                                     x_period, y_period, center, noise, seed, sample_offset,
                                                     terminal, outputs)
        arr = {k: np.empty((n,) + ((2,) if k == "x_final" and self.ndim == 2 else ())) for k in outputs}
        r = N.pdhg_policy_report()
        N.check(self._lib.pdhg_policy_eval(self._h, ctypes.byref(po), N.dptr(x0), N.dptr(noise), ctypes.byref(r),
                                           N.dptr(arr.get("running")), N.dptr(arr.get("terminal")),
                                           N.dptr(arr.get("value")), N.dptr(arr.get("x_final"))))
        d = {f: getattr(r, f) for f in N.POLICY_FIELDS}
        d.update(arr)
        return d

    # ---- how good is the state the context holds ----
    def report(self):
        """The KKT residual norms of the resident (phi, rho, alp) and the rho / phi ranges (pdhg_report_state): a dict
        of pdhg_report's fields.  One read-only device pass; the iteration's state and bookkeeping are untouched."""
        r = N.pdhg_report()
        N.check(self._lib.pdhg_report_state(self._h, ctypes.byref(r)))
        return {f: getattr(r, f) for f in N.REPORT_FIELDS}

    def residual_rows(self, row0, nrows, hj=True, cont=True):
        """Rows [row0, row0 + nrows) of the HJ residual and of the continuity residual (its rows 1.. of the
        reference's [T+1] array), float64 [nrows, nx(, ny)]: the values report() reduces.  A field passed as False is
        not computed into a host array and comes back as None."""
        f = lambda on: np.empty((int(nrows),) + self._space) if on and nrows >= 1 else None  # noqa: E731
        h, c = f(hj), f(cont)
        N.check(self._lib.pdhg_report_rows(self._h, int(row0), int(nrows), N.dptr(h), N.dptr(c)))
        return h, c

    # ---- updates ----
    def update_primal(self, tau):
        self._version += 1
        N.check(self._lib.pdhg_update_primal(self._h, float(tau)))

    def update_dual(self, sigma, eps, rho_alp_iters):
        used = ctypes.c_int(0)
        self._version += 1
        N.check(self._lib.pdhg_update_dual(self._h, float(sigma), float(eps), int(rho_alp_iters), ctypes.byref(used)))
        return used.value

    def errors(self):
        e1, e2 = ctypes.c_double(), ctypes.c_double()
        N.check(self._lib.pdhg_errors(self._h, ctypes.byref(e1), ctypes.byref(e2)))
        return e1.value, e2.value

    def inner_error(self):
        e = ctypes.c_double()
        N.check(self._lib.pdhg_inner_error(self._h, ctypes.byref(e)))
        return e.value

    def iterate(self, n_iters, tau, sigma, eps, rho_alp_iters):
        st = N.pdhg_stats()
        self._version += 1
        N.check(self._lib.pdhg_iterate(self._h, int(n_iters), float(tau), float(sigma), float(eps),
                                       int(rho_alp_iters), ctypes.byref(st)))
        return {"iters_run": st.iters_run, "status": st.status, "inner_last": st.inner_last,
                "inner_total": st.inner_total, "err1": st.err1, "err2": st.err2, "err_inner": st.err_inner,
                "nan_seen": st.nan_seen, "first_nan_iter": st.first_nan_iter}

    def set_stop_rules(self, converge=True, nan=True):
        N.check(self._lib.pdhg_set_stop_rules(self._h, 1 if converge else 0, 1 if nan else 0))

    def synchronize(self):
        N.check(self._lib.pdhg_synchronize(self._h))

    # ---- measurement ----
    def device_bytes(self):
        b = ctypes.c_ulonglong()
        N.check(self._lib.pdhg_device_bytes(self._h, ctypes.byref(b)))
        return b.value

    def path_info(self, key):
        """Kernel variant selected for this context (pdhg_path_info): "fused_residual", "fast_rows",
        "fast_dual", "fast_xt"."""
        v = ctypes.c_int()
        N.check(self._lib.pdhg_path_info(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def profile_enable(self, on=True):
        N.check(self._lib.pdhg_profile_enable(self._h, 1 if on else 0))

    def profile_query(self, cls):
        ms, n = ctypes.c_double(), ctypes.c_int()
        N.check(self._lib.pdhg_profile_query(self._h, cls.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def algorithmic_bytes(self, k, cls="iteration"):
        b = ctypes.c_double()
        N.check(self._lib.pdhg_algorithmic_bytes(self._h, int(k), cls.encode(), ctypes.byref(b)))
        return b.value
