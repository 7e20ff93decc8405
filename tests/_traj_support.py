"""Shared pieces of the trajectory tests: a restatement of the device noise stream (include/pdhg.h,
pdhg_trajectories) in NumPy integers, and the problems / margins of the rollout parity cases."""
import math

import numpy as np

import pdhg_oracle as O
import traj_oracle as TO

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC'11).  ctr: four
    and key: two uint32 values or equal-shape uint64 arrays holding them; returns the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in ctr]
    k = [int(v) & MASK for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & np.uint64(MASK)]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def device_normals(seed, samples, step, pair=0):
    """The two standard normals per sample of (seed, sample, step, axis pair) as the header documents them."""
    s = np.asarray(samples, dtype=np.uint64)
    r = philox4x32_10([s & np.uint64(MASK), s >> np.uint64(32), np.full(s.shape, step, np.uint64),
                       np.full(s.shape, pair, np.uint64)], [seed & MASK, (seed >> 32) & MASK])
    a = (r[0] << np.uint64(32)) | r[1]
    b = (r[2] << np.uint64(32)) | r[3]
    u1 = ((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (b >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    return rad * np.cos(ang), rad * np.sin(ang)


# ---- rollout parity cases ----
P_SPACE = 2.0
DT = 0.1
SEED = 7

CASES_1D = [(1, "linear"), (2, "nearest")]
CASES_2D = [(1, "linear"), (2, "nearest"), (3, "linear")]
# off-grid starts, some outside [0, P) on both sides; 1.985 lies in the last half cell of the 32-point grid (last
# node 1.9375, midpoint 1.96875): nearest keeps the last node there, it does not wrap to node 0
X0_1D = np.array([-0.37, 0.013, 0.53, 1.117, 1.69, 1.985, 2.41, -1.93, 3.26])
X0_2D = np.array([[0.013, -0.021], [-0.37, 1.117], [1.69, 2.41], [2.41, -1.93], [-2.23, 0.53], [3.26, 3.71],
                  [1.985, 1.93], [0.53, -0.31]])
# egno 3: the grid is centred on [-1, 1); x is the Neumann axis, so starts beyond both x edges
X0_E3 = np.array([[0.47, -0.83], [-1.37, 0.21], [1.29, 0.67], [-0.93, 1.41], [0.07, -1.63], [0.97, 2.77],
                  [-0.41, 0.013], [1.83, -0.53]])


def problem(egno, ndim, T=4):
    nx, ny = (32, 1) if ndim == 1 else (16, 12)
    x_arr = O.make_grid(ndim, nx, ny, egno, P_SPACE, P_SPACE)
    if ndim == 1:
        xs, ys = x_arr[0, :, 0], None
    else:
        xs, ys = x_arr[0, :, 0, 0], x_arr[0, 0, :, 1]
    n_ctrl = 1 if (ndim == 1 or egno == 3) else 2
    n_alp = 2 if ndim == 1 else 4
    bc = O.default_bc(egno, ndim)
    return dict(egno=egno, ndim=ndim, nx=nx, ny=ny, T=T, dt=DT, dx=P_SPACE / nx, dy=P_SPACE / ny, xs=xs, ys=ys,
                n_ctrl=n_ctrl, n_alp=n_alp, bc=bc, x_arr=x_arr, f_fn=O.set_up_example_fns(egno, ndim, 0).f_fn,
                center=(egno == 3, egno == 3), x0=X0_1D if ndim == 1 else (X0_E3 if egno == 3 else X0_2D))


def random_alp(P, seed=SEED, T=None):
    """Random controls with the dead components zero (include/pdhg.h: only live components are stored)."""
    T = P["T"] if T is None else T
    sp = (P["nx"],) if P["ndim"] == 1 else (P["nx"], P["ny"])
    rng = np.random.default_rng(seed)
    alp = np.zeros((P["n_alp"], T) + sp + (P["n_ctrl"],))
    for a in range(P["n_alp"]):
        if P["ndim"] == 1 or P["egno"] == 3:
            comp = 0 if a < 2 else None
        else:
            comp = 0 if a < 2 else 1
        if comp is not None:
            alp[a, ..., comp] = 0.5 * rng.standard_normal(alp.shape[1:-1])
    return alp


def make_ctx(P, precision, epsl, rho_alp_iters=1, T=None):
    from pdhg_amd.context import PDHGContext
    return PDHGContext(P["egno"], P["ndim"], P["nx"], P["ny"], P["T"] if T is None else T, P["dx"], P["dy"], P["dt"],
                       P["xs"], P["ys"], epsl=epsl, bc=P["bc"], precision=precision, rho_alp_iters=rho_alp_iters)


def load_alp(ctx, alp):
    """phi = 0, rho = 1 and the given controls: nothing but the rollout runs."""
    sp = alp.shape[2:-1]
    T = alp.shape[1]
    ctx.set_state(np.zeros((T + 1,) + sp), np.ones((T,) + sp), tuple(alp))


def oracle_traj(P, alp, x0, epsl, method, noise):
    """traj_oracle on alp in PDE time order (reversed here as run_example.py:347 does); the noise array is replayed
    through the rng argument in the oracle's own per-step order."""
    alp = np.asarray(alp)
    T = alp.shape[1]
    t_arr = np.arange(T + 1) * P["dt"]
    alp_c = alp[:, ::-1]

    class Replay:
        def __init__(self):
            self.i = 0

        def normal(self, size):
            z = noise[self.i].reshape(size) if noise is not None else np.zeros(size)
            self.i += 1
            return z
    if P["ndim"] == 1:
        return TO.compute_traj_1d(x0, alp_c[..., 0], P["f_fn"], T + 1, P["xs"], t_arr, P_SPACE, T * P["dt"], epsl,
                                  method, rng=Replay())
    return TO.compute_traj_2d(x0, alp_c, P["f_fn"], T + 1, P["xs"], P["ys"], t_arr, P_SPACE, P_SPACE, T * P["dt"],
                              P["bc"], P["center"], epsl, method, rng=Replay())


def assert_margins(P, alp, traj_x, method, check_f=True):
    """Discrete choices flip under rounding (the nearest node, the cell, the sign split of f), so on the oracle's own
    trajectory: no interpolated position within 1e-6 of a cell width of a cell edge or a nearest-node midpoint,
    and no |f| below 1e-9 (exact zeros take the same branch on both sides and are left out)."""
    alp = np.asarray(alp)
    T = alp.shape[1]
    alp_c = alp[:, ::-1]
    pos = np.asarray(traj_x)[:T].reshape(T, -1, P["ndim"])
    for d, (g, h) in enumerate([(P["xs"], P["dx"]), (P["ys"], P["dy"])][:P["ndim"]]):
        frac = ((pos[..., d] - g[0]) % P_SPACE) / h
        edge = np.abs(frac - np.round(frac))
        mid = np.abs(frac - np.floor(frac) - 0.5)
        assert edge.min() > 1e-6 and mid.min() > 1e-6, (d, edge.min(), mid.min())
    if not check_f:
        return
    fmin = np.inf
    for ind in range(T):
        for s in range(pos.shape[1]):
            if P["ndim"] == 1:
                x = pos[ind, s, 0]
                if method == "linear":
                    a = [TO.interp_periodic(x, P["xs"], alp_c[k, ind, :, 0], P_SPACE) for k in range(2)]
                else:
                    j = TO.nearest_index(x, P["xs"], P_SPACE)
                    a = [alp_c[k, ind, j, 0] for k in range(2)]
                xm = np.array([[x % P_SPACE]])
                f = [float(P["f_fn"](np.array([[v]]), xm, 0.0)[0, 0]) for v in a]
            else:
                x, y = pos[ind, s]
                lo, hi = pos[ind].min(axis=0), pos[ind].max(axis=0)
                e1 = TO.VirtualExtension(P["xs"], lo[0], hi[0], P_SPACE, P["bc"][0], P["center"][0])
                e2 = TO.VirtualExtension(P["ys"], lo[1], hi[1], P_SPACE, P["bc"][1], P["center"][1])
                c = [TO.interp2(alp_c[k, ind], e1, e2, x, y, method) for k in range(4)]
                xin = np.array([[x % P_SPACE if P["bc"][0] == 0 else x, y % P_SPACE]])
                f = [float(P["f_fn"](c[k][None, :], xin, 0.0)[0, 0 if k < 2 else 1]) for k in range(4)]
            for v in f:
                if v != 0.0:
                    fmin = min(fmin, abs(v))
    assert fmin >= 1e-9, fmin


def rounded(alp, precision):
    """The controls as a context of this precision stores them (fp32 and mixed: float; get_state returns these)."""
    return alp if precision == "fp64" else alp.astype(np.float32).astype(np.float64)


def noise_for(P, n, seed=11, T=None):
    T = P["T"] if T is None else T
    return np.random.default_rng(seed).standard_normal((T, n, P["ndim"]))


# the project's bound for the NumPy trajectory module against this oracle (tests/test_trajectories.py)
RTOL, ATOL = 1e-11, 1e-12


def deviation(got, ref):
    """max of |got - ref| / (ATOL + RTOL |ref|): <= 1 is np.allclose(got, ref, RTOL, ATOL)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return float(np.max(np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))))


def kat():
    """Known answers of Philox4x32-10 from the Random123 distribution's kat_vectors."""
    return [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def sqrt2epsdt(epsl, dt):
    return math.sqrt(2 * epsl * dt)
