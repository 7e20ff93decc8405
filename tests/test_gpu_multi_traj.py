"""Closed-loop trajectories on decomposed windows: pdhg_multi_trajectories (MultiContext.trajectories) and the slab
primitive beneath it (pdhg_slab_trajectories: TrajP::step0, csrc/kernels_traj.hpp).

Yardstick: the single context on the same controls.  A slab marches its own rows with the single context's kernel;
the global step offset only selects the Philox step word, the noise row and the record rows, and the positions are
handed from slab to slab as the fp64 values the kernel wrote.  So x_final, traj_x and traj_alp are bit for bit the
single context's (positions are fp64, alp is read as stored).  The single context itself is pinned to the oracle by
test_gpu_traj.py and, across the step0 change, to values recorded before it (tests/golden/make_traj_step_fixture.py).

Grid 16 x 256 (the smallest ny an fp32 t-slab takes); T = 7 over 3 slabs (3 / 2 / 2) and T = 4 over 3 (2 / 1 / 1:
one-row slabs)."""
import ctypes
import os

import numpy as np
import pytest

import pdhg_oracle as O
import _traj_support as S

pytestmark = pytest.mark.gpu

NX, NY = 16, 256
SPLITS = {"T7x3": (7, [0, 0, 0]), "T4x3": (4, [0, 0, 0])}
PHYS = {"e2": (2, 0.1), "e3": (3, 0.0)}


def _problem(egno, T):
    P = S.problem(egno, 2, T)
    x_arr = O.make_grid(2, NX, NY, egno, S.P_SPACE, S.P_SPACE)
    P.update(nx=NX, ny=NY, dx=S.P_SPACE / NX, dy=S.P_SPACE / NY, x_arr=x_arr, xs=x_arr[0, :, 0, 0],
             ys=x_arr[0, 0, :, 1])
    return P


def _multi(P, prec, epsl, devices, k=1):
    from pdhg_amd.multi import MultiContext
    return MultiContext(P["egno"], P["nx"], P["ny"], P["T"], P["dx"], P["dy"], P["dt"], P["xs"], P["ys"],
                        devices=devices, epsl=epsl, precision=prec, rho_alp_iters=k)


def _starts(P, n, seed=2):
    """Off-grid starts, some outside the period cell on both sides (egno 3: centred grid, Neumann x edges)."""
    lo = -2.0 if P["egno"] == 3 else -1.0
    return np.random.default_rng(seed).uniform(lo, lo + 4.0, (n, 2))


def _same(got, want):
    for name, g, w in zip(("traj_alp", "traj_x", "x_final"), got, want):
        assert g.shape == w.shape, name
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("{} differs at {} entries, first {} (row = global step for the records)".format(
                name, len(bad), bad[0]))


CASES = [(ph, sp, pr, me) for ph in PHYS for sp in SPLITS for pr in ("fp32", "fp64") for me in ("linear", "nearest")]


@pytest.mark.parametrize("phys, split, prec, method", CASES)
def test_paths_equal_single_context(native, phys, split, prec, method):
    """(9): 300 samples (a ragged last workgroup), device noise with a sample offset and a supplied noise array."""
    egno, epsl = PHYS[phys]
    T, devs = SPLITS[split]
    P = _problem(egno, T)
    alp = S.random_alp(P)
    x0 = _starts(P, 300)
    ctx, m = S.make_ctx(P, prec, epsl), _multi(P, prec, epsl, devs)
    try:
        S.load_alp(ctx, alp)
        S.load_alp(m, alp)
        kw = dict(center=P["center"])
        runs = [dict(seed=(5 << 32) | 9, sample_offset=1000)]
        if epsl > 0:
            runs.append(dict(noise=S.noise_for(P, len(x0))))
        for extra in runs:
            want = ctx.trajectories(x0, method, S.P_SPACE, S.P_SPACE, **kw, **extra)
            got = m.trajectories(x0, method, S.P_SPACE, S.P_SPACE, **kw, **extra)
            assert np.isfinite(want[2]).all() and np.array_equal(want[1][0], x0)
            _same(got, want)
        if epsl > 0:   # the two noise sources give different paths: the comparison above is not vacuous
            assert not np.array_equal(want[2], ctx.trajectories(x0, method, S.P_SPACE, S.P_SPACE, **kw, **runs[0])[2])
        na, nx_, nf = m.trajectories(x0, method, S.P_SPACE, S.P_SPACE, record=(), **kw, **runs[-1])
        assert na is None and nx_ is None and np.array_equal(nf, want[2])
    finally:
        ctx.close()
        m.close()


def _chunk_samples(T, n_ctrl):
    """Samples one staging chunk holds with both records on and device noise: kTrajBudget (64 MiB, ctx_impl.hpp) over
    the bytes per sample -- positions in / out, traj_x rows [T + 1], traj_alp rows [T] -- in whole workgroups."""
    per = 8 * (2 * 2 + (T + 1) * 2 + T * n_ctrl)
    return max((64 << 20) // per, 256) // 256 * 256


def test_chunks_hand_positions_through_the_slabs(native):
    """(10): more samples than one chunk holds, so at least two chunks march through the slab chain and reuse its
    buffers; bit for bit the one-chunk calls on the two halves with their sample offsets."""
    egno, epsl = PHYS["e2"]
    T, devs = SPLITS["T4x3"]
    P = _problem(egno, T)
    m_chunk = _chunk_samples(T, P["n_ctrl"])
    n = m_chunk + 300
    assert n // 2 < m_chunk < n
    x0 = _starts(P, n)
    m = _multi(P, "fp32", epsl, devs)
    try:
        S.load_alp(m, S.random_alp(P))
        whole = m.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, seed=9, sample_offset=17)
        h = n // 2
        parts = [m.trajectories(x0[a:b], "linear", S.P_SPACE, S.P_SPACE, seed=9, sample_offset=17 + a)
                 for a, b in ((0, h), (h, n))]
    finally:
        m.close()
    assert np.array_equal(np.concatenate([parts[0][0], parts[1][0]], axis=1), whole[0])
    assert np.array_equal(np.concatenate([parts[0][1], parts[1][1]], axis=1), whole[1])
    assert np.array_equal(np.concatenate([parts[0][2], parts[1][2]], axis=0), whole[2])
    assert np.array_equal(whole[1][-1], whole[2])


def test_windows_chain_through_x_final(native):
    """(11): x_final of one multi-device window is x_init of the next window's call; equal to the single-context
    chain (windows are chained in control time: the context holding the later PDE rows first)."""
    egno, epsl = PHYS["e2"]
    late, early = _problem(egno, 7), _problem(egno, 4)
    a_late, a_early = S.random_alp(late, seed=3), S.random_alp(early, seed=4)
    x0 = _starts(late, 300)
    n_late, n_early = S.noise_for(late, 300, seed=5), S.noise_for(early, 300, seed=6)
    ctxs = [S.make_ctx(late, "fp64", epsl), S.make_ctx(early, "fp64", epsl),
            _multi(late, "fp64", epsl, [0, 0, 0]), _multi(early, "fp64", epsl, [0, 0])]
    try:
        for c, a in zip(ctxs, (a_late, a_early, a_late, a_early)):
            S.load_alp(c, a)
        out = []
        for first, second in (ctxs[:2], ctxs[2:]):
            _, _, xf1 = first.trajectories(x0, "linear", S.P_SPACE, S.P_SPACE, noise=n_late)
            out.append((xf1,) + tuple(second.trajectories(xf1, "linear", S.P_SPACE, S.P_SPACE, noise=n_early)))
    finally:
        for c in ctxs:
            c.close()
    assert all(np.array_equal(u, v) for u, v in zip(out[0], out[1]))
    assert np.array_equal(out[1][2][0], out[1][0])      # the second window's traj_x row 0 is the first's x_final


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("method", ["linear", "nearest"])
def test_single_context_reproduces_recorded_paths(native, prec, method):
    """(12): the single context (step0 = 0) reproduces, bit for bit, what the kernels returned before they took a step
    offset (tests/golden/make_traj_step_fixture.py, recorded on the GPU at the previous commit)."""
    import make_traj_step_fixture as F
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", os.path.basename(F.OUT)))
    assert (int(d["seed_hi"]) << 32) | int(d["seed_lo"]) == F.SEED and int(d["offset"]) == F.OFFSET
    P = S.problem(1, 2)
    assert np.array_equal(d["x0"], P["x0"]) and np.array_equal(d["alp"], S.random_alp(P))
    ta, tx, xf = F.run(prec, method)
    key = "{}/{}".format(prec, method)
    assert np.array_equal(xf, d["x_final/" + key])
    assert np.array_equal(tx, d["traj_x/" + key]) and np.array_equal(ta, d["traj_alp/" + key])


def test_argument_checks(native):
    N = native
    P = _problem(2, 4)
    m = _multi(P, "fp32", 0.1, [0, 0])
    ctx = S.make_ctx(P, "fp32", 0.1)
    try:
        S.load_alp(m, S.random_alp(P))
        x0 = np.zeros((4, 2))
        xf = np.empty_like(x0)

        def raw(h, n_sample=4, method=0, xp=S.P_SPACE, yp=S.P_SPACE, offset=0, opts=True, x=x0):
            o = N.pdhg_traj_opts()
            o.n_sample, o.method, o.x_period, o.y_period, o.sample_offset = n_sample, method, xp, yp, offset
            return m._lib.pdhg_multi_trajectories(h, ctypes.byref(o) if opts else None, N.dptr(x) if x is not None
                                                  else None, None, N.dptr(xf), None, None)
        assert raw(m._h) == N.PDHG_OK
        for kw in (dict(n_sample=0), dict(method=2), dict(method=-1), dict(xp=0.0), dict(yp=-1.0), dict(offset=-1),
                   dict(opts=False), dict(x=None)):
            assert raw(m._h, **kw) == N.PDHG_ERR_ARG and m._lib.pdhg_last_error(), kw
        assert raw(ctx._h) == N.PDHG_ERR_ARG                  # a pdhg_ctx handle is not a multi-device one
        # the slab primitive refuses a context that is no t-slab, and the whole-window entry points stay refused
        o = N.pdhg_traj_opts()
        o.n_sample, o.x_period, o.y_period = 4, S.P_SPACE, S.P_SPACE
        assert ctx._lib.pdhg_slab_trajectories(ctx._h, ctypes.byref(o), 0, 4, None, None, None, None, None) == \
            N.PDHG_ERR_ARG
        assert m._lib.pdhg_trajectories(m._h, ctypes.byref(o), N.dptr(x0), None, N.dptr(xf), None, None) == \
            N.PDHG_ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            m.trajectories(np.zeros((4, 3)), "linear", S.P_SPACE, S.P_SPACE)
        with pytest.raises(ValueError):
            m.trajectories(x0, "cubic", S.P_SPACE, S.P_SPACE)
    finally:
        m.close()
        ctx.close()
