"""The dual step from a state where every clamp fires, point by point, on every dual kernel (pytest -m gpu).

Every dual kernel holds three non-smooth operations -- rho' = max(rho + sigma vec, 0), egno 2's clip of the control
to [-1, 1] (nclamp, alp_prox) and the sign masks of the controls -- and from make_problem's seeded state only the masks
fire.  Here one dual step (set_state, set_phi_bar, update_dual(sigma, -inf, 1), get_state) runs from
_dual_support.clamp_state, where the float64 oracle projects 12-50 % of rho, leaves 28-38 % of egno 2's controls at
+-1 and masks about half of them (the shares are asserted per case, here and without a device by
test_dual_clamps_host.py, which also pins the oracle's dual step to a long-double restatement).

Checks (tests/_dual_support.py), none of which excludes a point:
  |d - o64| <= K r u S at every point of rho' and of every live control; u = 2^-24 (fp32, mixed) or 2^-53 (fp64), S the
  output's formula over absolute values, r the float32 oracle's own largest |o32 - o64| / (2^-24 S) on the case, K = 4.
  Where the oracle decides by more than m = K r u S: rho' == 0, control == +-1, control == 0 exactly.
  The dead control components equal the oracle's; inner_error() against the oracle's err (fp64 1e-9, fp32 1e-4).
  The fused-residual kernels: update_primal(tau) after the step consumes the rows the sweep formed from a state with
  rho' == 0 and masked controls; phi' against the oracle's primal at the oracle's (rho', alp') (fp64 1e-9; fp32
  max(1e-6, K e32), e32 the float32 oracle's own distance).
  NaN: one NaN in phi_bar (interior point, tile corner, last time row), in rho, in a live control -- the NaN sets of
  rho' and of every control equal the oracle's (a plain fmax would turn the NaN into 0), the finite points keep the
  bound.
  The chunked dual loop (rho_alp_iters = 10): the oracle's sub-iteration count, the state's relative L2 norm, and the
  exact checks on the last sub-iteration's decisions.

KERNELS lists every dual kernel at the smallest shapes that select it; the selection is asserted through
pdhg_path_info.  Default tier: per kernel row egno 2 (the most branches) and one egno 3 where the kernel handles the
Neumann edge, the fused-residual, NaN and chunked-loop cases; the rest of the shape x egno x T grid is extended.
Every case logs r, the largest |d - o| / (u S) per array over the seam points (first / last row of a row tile, first
/ last column of a strip, time rows 0 and T - 1) and over the interior, the bound, the branch and margin shares.
"""
import collections
import contextlib

import numpy as np
import pytest

import _dual_support as D
import pdhg_oracle as O
from _problems import device_ctx, make_problem, rel

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PDHG_DUAL_RX", "PDHG_DUAL_ONE", "PDHG_DUAL_YPL", "PDHG_DUAL_NBSYNC", "PDHG_SHORT_T", "PDHG_FUSE_RES",
            "PDHG_FUSE_RES1D", "PDHG_FR1D_CHUNKS", "PDHG_DUAL_MULTI", "PDHG_DUAL_HEAD", "PDHG_DUAL64", "PDHG_DUAL_ORDER",
            "PDHG_FS16", "PDHG_FOURSTEP")

# name, precision, (egno, ndim, nx, ny, T, epsl), environment, expected path_info, (row tile, strip) of the seam
# points, fused residual?, default tier?
Case = collections.namedtuple("Case", "name prec problem env expect tile fr default")
CASES = []


def _add(kernel, prec, problem, env, expect, tile, default, fr=False, tag=""):
    egno, ndim, nx, ny, T, epsl = problem
    name = "{}-{}-e{}_{}x{}_T{}{}".format(kernel, prec, egno, nx, ny, T, ("-" + tag) if tag else "")
    CASES.append(Case(name, prec, problem, dict(env), dict(expect), tile, fr, default))


def _epsl(T):
    return 0.0 if T == 1 else 0.1   # both sides of the kernels' epsl != 0 branch


# ---- k_dual_1d (kernels_1d.hpp): one thread per x, 256-thread blocks
for _prec in ("fp64", "fp32"):
    for _egno in (1, 2):
        for _nx in (16, 17, 160):
            for _T in (1, 4):
                _add("dual_1d", _prec, (_egno, 1, _nx, 1, _T, _epsl(_T)), {}, {"fused_residual": 0, "fourstep": 0},
                     (256, 1), _egno == 2 and _nx == 17 and _T == 4)
# ---- k_dual_1d_fr (kernels_fs16.hpp): nx = 65536 only; the time chunks of the sweep forced to 1 and left at min(8, T)
for _prec in ("fp64", "fp32"):
    for _egno in (1, 2):
        for _T in (1, 3):
            for _chunks in ("1", None):
                if _T == 1 and _chunks is None:
                    continue   # one row: one chunk either way
                _add("dual_1d_fr", _prec, (_egno, 1, 65536, 1, _T, _epsl(_T)),
                     {} if _chunks is None else {"PDHG_FR1D_CHUNKS": _chunks}, {"fused_residual": 1, "fs16": 1},
                     (64, 1), _egno == 2 and _T == 3, fr=True, tag="chunks" + (_chunks or "T"))
# ---- k_dual_2d (kernels_2d.hpp): the per-point kernel (ny not a multiple of 256); egno 3: bc (1, 0)
for _prec in ("fp64", "fp32"):
    for _egno in (1, 2, 3):
        for _nx, _ny in ((16, 12), (15, 17), (20, 18)):
            for _T in (1, 3):
                _add("dual_2d", _prec, (_egno, 2, _nx, _ny, _T, _epsl(_T)), {}, {"fast_dual": -1, "mixed": 0},
                     (_nx, _ny), _T == 3 and ((_egno == 2 and _nx == 15) or (_egno == 3 and _nx == 16)))
# ---- k_dual_mixed_2d / k_dual_fast_mixed_2d<ONE = 0, 1>
for _egno in (1, 2, 3):
    for _T in (1, 3):
        _d = _T == 3 and _egno == 2
        _add("dual_mixed_2d", "mixed", (_egno, 2, 16, 12, _T, _epsl(_T)), {}, {"fast_dual": -1, "mixed": 1}, (16, 12),
             _T == 3 and _egno != 1)
        for _one in ("1", "0"):
            _add("dual_fast_mixed_2d", "mixed", (_egno, 2, 16, 256, _T, _epsl(_T)), {"PDHG_DUAL_ONE": _one},
                 {"fast_dual": 0, "mixed": 1, "dual_one": int(_one)}, (16, 256),
                 _d or (_T == 3 and _egno == 3 and _one == "1"), tag="one" + _one)
# ---- k_dual_fast_2d<ONE = 0, 1, 2> (kernels_2d_fast.hpp): row per thread; 16 x 512: two column blocks
for _prec in ("fp64", "fp32"):
    for _egno in (1, 2, 3):
        for _nx, _ny in ((8, 256), (16, 512)):
            for _T in (1, 3):
                for _one in ("0", "1", "2"):
                    if _one == "2" and _prec == "fp32":
                        continue   # the 4-waves-per-SIMD form is fp64
                    _d = _T == 3 and ((_egno == 2 and _nx == 16) or (_egno == 3 and _nx == 8 and _one != "2"))
                    _add("dual_fast_2d", _prec, (_egno, 2, _nx, _ny, _T, _epsl(_T)),
                         {"PDHG_DUAL_RX": "0", "PDHG_DUAL_ONE": _one},
                         {"fast_dual": 0, "dual_one": int(_one != "0"), "mixed": 0}, (_nx, 256), _d, tag="one" + _one)
# ---- k_dual_lds_2d without the fused residual (kernels_dual_lds.hpp): RX x rows per workgroup through LDS
for _prec, _rx, _ypl in (("fp32", 4, 4), ("fp32", 8, 4), ("fp32", 16, 4), ("fp64", 8, 4), ("fp64", 8, 2)):
    for _egno in (1, 2, 3):
        for _nx, _ny in ((16, 256), (32, 512)):
            for _T in (1, 3):
                for _nb in ("0", "1"):
                    _env = {"PDHG_DUAL_RX": str(_rx), "PDHG_SHORT_T": "0", "PDHG_FUSE_RES": "0", "PDHG_DUAL_NBSYNC": _nb}
                    if _prec == "fp64":
                        _env["PDHG_DUAL_YPL"] = str(_ypl)
                    # default tier: every (precision, RX, YPL) once on the two-tile shape, the neighbour-flag sync on
                    # fp32 RX 8 and fp64 YPL 2; egno 3 (the Neumann ghost rows) on RX 8 / YPL 4
                    _nb_dflt = "1" if (_prec, _rx, _ypl) in (("fp32", 8, 4), ("fp64", 8, 2)) else "0"
                    _d = _T == 3 and ((_egno == 2 and _nx == 32 and _nb == _nb_dflt)
                                      or (_egno == 3 and _nx == 16 and _rx == 8 and _ypl == 4 and _nb == "0"))
                    _add("dual_lds_2d", _prec, (_egno, 2, _nx, _ny, _T, _epsl(_T)), _env,
                         {"fast_dual": _rx, "dual_ypl": _ypl, "fused_residual": 0}, (_rx, 64 * _ypl), _d,
                         tag="rx{}_ypl{}_nb{}".format(_rx, _ypl, _nb))
# ---- k_dual_lds_2d<.., FR>: the sweep also forms the next primal's residual rows (egno 1 / 2, periodic)
for _prec, _shape, _T, _ypl in (("fp32", (64, 256), 1, 4), ("fp32", (256, 512), 3, 4), ("fp64", (16, 2048), 3, 2)):
    for _egno in (2, 1):
        for _nb in ("0", "1"):
            _add("dual_lds_2d_fr", _prec, (_egno, 2) + _shape + (_T, _epsl(_T)),
                 {"PDHG_FUSE_RES": "1", "PDHG_SHORT_T": "0", "PDHG_DUAL_NBSYNC": _nb},
                 {"fast_dual": 8, "dual_ypl": _ypl, "fused_residual": 1}, (8, 64 * _ypl), _egno == 2 and _nb == "0",
                 fr=True, tag="nb" + _nb)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the chunked dual loop (kernels_dual_multi.hpp): k_dual_multi_2d / k_dual_multi_mixed_2d, all chunks or the head form
MULTI_SHAPE = (16, 256, 3, 0.1)
MULTI = [(prec, egno, form) for prec in ("fp64", "mixed") for egno in (2, 3, 1) for form in ("multi", "head")]
# NaN propagation: one case per kernel family (per-point, row-per-thread, LDS-tiled, 1-D), egno 2
NAN_FAMILIES = {
    "per_point": ((2, 2, 16, 12, 3, 0.1), {}, {"fast_dual": -1}),
    "row_per_thread": ((2, 2, 16, 256, 3, 0.1), {"PDHG_DUAL_RX": "0"}, {"fast_dual": 0}),
    "lds_tiled": ((2, 2, 16, 256, 3, 0.1), {"PDHG_DUAL_RX": "8", "PDHG_SHORT_T": "0", "PDHG_FUSE_RES": "0"},
                  {"fast_dual": 8, "fused_residual": 0}),
    "1d": ((2, 1, 17, 1, 3, 0.1), {}, {"fused_residual": 0}),
}


def all_problem_cases():
    """Every (egno, ndim, nx, ny, T, epsl) this file runs: test_dual_clamps_host.py asserts their conditions."""
    out = [c.problem for c in CASES] + [v[0] for v in NAN_FAMILIES.values()]
    return out + [(egno, 2) + MULTI_SHAPE for _, egno, _ in MULTI]


def _params():
    cs = sorted(CASES, key=lambda c: (c.problem, c.prec != "fp64", c.name))   # one shape's cases share the reference
    return [pytest.param(c.name, id=c.name, marks=() if c.default else (pytest.mark.extended,)) for c in cs]


_REF = collections.OrderedDict()   # (problem, reference inputs' rounding) -> the case's reference, the last few


def _reference(problem, prec):
    """P, the clamp state, r and the float64 oracle's step on the state as the device of `prec` holds it: computed
    once per (problem, rounding) and left unchanged."""
    key = (problem, prec)
    if key not in _REF:
        P = make_problem(*problem)
        state = D.clamp_state(P)
        r = D.calibrate(P, *state)
        ref = D.reference(P, *D.round_inputs(prec, *state))
        shares, mshare = D.assert_conditions(P, ref, r, D.U32 if prec != "fp64" else D.U64)
        _REF[key] = (P, state, r, ref, shares, mshare)
        while len(_REF) > 4:
            _REF.popitem(last=False)
    return _REF[key]


@contextlib.contextmanager
def _device():
    """A native error (not a failed check) leaves the process's device state unknown: end the session instead of
    launching the remaining cases on it."""
    try:
        yield
    except Exception as e:   # pytest.fail and failed assertions of the checks are raised outside these blocks
        pytest.exit("device error in test_gpu_dual_clamps: {!r}".format(e), returncode=3)


def _ctx(P, prec, env, expect, monkeypatch, **kw):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with _device():
        ctx = device_ctx(P, prec, **kw)
        got = {k: ctx.path_info(k) for k in expect}
    if got != expect:
        ctx.close()
        pytest.fail("kernel not selected: path_info {} != {}".format(got, expect))
    return ctx


def _oracle_primal(P, phi, rho, alp, dtype=np.float64):
    f = dtype
    up = O.update_primal_1d if P["ndim"] == 1 else O.update_primal_2d
    out = up(phi.astype(f), rho.astype(f), 70.0, tuple(a.astype(f) for a in alp), D.TAU, P["dt"], P["dsp"], P["fns"],
             P["fv"], P["epsl"], P["x_arr"].astype(f), None, P["bc"])
    assert out.dtype == f
    return out


def _u(prec):
    return D.U64 if prec == "fp64" else D.U32


def _finish(parity_log, test, name, measured, bounds, fails, **extra):
    """Log, print every figure, then assert."""
    parity_log(test, name, measured, bounds, **extra)
    print(name, "measured", measured, "bounds", bounds, extra)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", _params())
def test_dual_clamps(native, monkeypatch, parity_log, name):
    c = BY_NAME[name]
    P, (rho, alp, phi_bar), r, ref, shares, mshare = _reference(c.problem, c.prec)
    u = _u(c.prec)
    ctx = _ctx(P, c.prec, c.env, c.expect, monkeypatch)
    try:
        with _device():
            ctx.set_state(P["phi"], rho, alp)
            ctx.set_phi_bar(phi_bar)
            ctx.update_dual(D.SIGMA, -np.inf, 1)
            err_d = ctx.inner_error()
            _, rho_d, alp_d = ctx.get_state(phi=False)
            if c.fr:
                ctx.update_primal(D.TAU)
                phi_d = ctx.get_state(rho=False, alp=False)[0]
    finally:
        ctx.close()
    seam = D.seam_mask(rho.shape, *c.tile)
    measured, fails = D.check_device(P, ref, r, u, rho_d, alp_d, seam)
    bounds = {"K_r": D.K * r}
    err_o = ref["err"]
    if np.isnan(err_o):      # egno 3: 0/0 over the dead y-controls (update_fns_in_pdhg.py:162-164)
        if not np.isnan(err_d):
            fails.append("inner_error {} where the oracle's is NaN".format(err_d))
    else:
        measured["inner_error_rel"] = abs(err_d - err_o) / abs(err_o)
        bounds["inner_error_rel"] = 1e-9 if c.prec == "fp64" else 1e-4
        if not measured["inner_error_rel"] <= bounds["inner_error_rel"]:
            fails.append("inner_error {!r} against the oracle's {!r}".format(err_d, err_o))
    if c.fr:
        # the fused rows: phi' from the residual the sweep formed, against the oracle's primal at its own (rho', alp')
        phi0 = P["phi"] if c.prec == "fp64" else P["phi"].astype(np.float32).astype(np.float64)
        phi_o = _oracle_primal(P, phi0, ref["rho"], ref["alp_full"])
        measured["phi_fused"] = rel(phi_d, phi_o)
        if c.prec == "fp64":
            bounds["phi_fused"] = 1e-9
        else:
            e32 = rel(_oracle_primal(P, phi0, ref["rho"], ref["alp_full"], np.float32), phi_o)
            measured["e32_phi"] = e32
            bounds["phi_fused"] = max(1e-6, D.K * e32)
        if not measured["phi_fused"] <= bounds["phi_fused"]:
            fails.append("phi' of the fused rows: {:.3g} > {:.3g}".format(measured["phi_fused"], bounds["phi_fused"]))
    _finish(parity_log, "test_dual_clamps", name, measured, bounds, fails, r=r, unit_roundoff=u, shares=shares,
            margin_share=mshare)


def _nan_states(P, state):
    """(label, rho, alp, phi_bar) with one kind of NaN each: phi_bar at an interior point, a tile corner and in the
    last time row; rho; a live control."""
    rho, alp, pb = state
    nd = P["ndim"]
    mid = (3,) if nd == 1 else (3, 5)
    corner = (8,) if nd == 1 else (8, 0)      # first row of the second 8-row tile, first column of a strip
    late = (5,) if nd == 1 else (5, 7)
    p1 = pb.copy()
    p1[(1,) + mid] = p1[(1,) + corner] = p1[(P["T"],) + late] = np.nan
    r1 = rho.copy()
    r1[(1,) + mid] = np.nan
    a1 = [a.copy() for a in alp]
    a1[1][(2,) + late + (0,)] = np.nan
    return [("phi_bar", rho, alp, p1), ("rho", r1, alp, pb), ("alp", rho, tuple(a1), pb)]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("family", list(NAN_FAMILIES))
def test_nan_propagates_like_the_oracle(native, monkeypatch, parity_log, family, prec):
    problem, env, expect = NAN_FAMILIES[family]
    P, state, r, _, _, _ = _reference(problem, prec)
    runs = []
    for label, rho, alp, pb in _nan_states(P, state):
        ref = D.reference(P, *D.round_inputs(prec, rho, alp, pb))
        n_nan = int(np.isnan(ref["rho"]).sum()) + sum(int(np.isnan(a).sum()) for a in ref["alp"])
        assert 0 < n_nan < ref["rho"].size, "the NaN case has no NaN, or nothing else, in the oracle"
        runs.append((label, rho, alp, pb, ref, n_nan))
    ctx = _ctx(P, prec, env, expect, monkeypatch)
    out = []
    try:
        with _device():
            for label, rho, alp, pb, ref, n_nan in runs:
                ctx.set_state(P["phi"], rho, alp)
                ctx.set_phi_bar(pb)
                ctx.update_dual(D.SIGMA, -np.inf, 1)
                out.append(ctx.get_state(phi=False))
    finally:
        ctx.close()
    measured, fails = {}, []
    for (label, _, _, _, ref, n_nan), (_, rho_d, alp_d) in zip(runs, out):
        m, f = D.check_device(P, ref, r, _u(prec), rho_d, alp_d)
        measured.update({"{}_{}".format(label, k): v for k, v in m.items()})
        measured[label + "_nan_points"] = n_nan
        fails += ["NaN in {}: {}".format(label, x) for x in f]
    _finish(parity_log, "test_nan_propagates_like_the_oracle", "{}-{}".format(family, prec), measured, {"K_r": D.K * r},
            fails, r=r)


def _loop(P, rho, alp, pb, k, eps, dtype=np.float64):
    """update_dual_alternative (update_fns_in_pdhg.py:167-180) in dtype: (rho', alp', sub-iterations, the state the
    last sub-iteration started from, err of every sub-iteration)."""
    f = dtype
    rho, alp = rho.astype(f), tuple(a.astype(f) for a in alp)
    errs = []
    for j in range(k):
        rho_n, alp_n, err = D.oracle_step(P, rho, alp, pb, D.SIGMA, f)
        errs.append(float(err))
        if err < eps or j == k - 1:
            return rho_n, alp_n, j + 1, (rho, alp), errs
        rho, alp = rho_n, alp_n


@pytest.mark.parametrize("eps", [1e-6, 0.04], ids=["eps1e-6", "eps0.04"])
@pytest.mark.parametrize("prec,egno,form", [pytest.param(p, e, f, marks=() if e != 1 else (pytest.mark.extended,),
                                                         id="{}-e{}-{}".format(p, e, f)) for p, e, f in MULTI])
def test_chunked_loop_from_clamp_state(native, monkeypatch, parity_log, prec, egno, form, eps):
    """update_dual(sigma, eps, 10) through the chunk passes against update_dual_alternative: eps = 1e-6 runs all 10
    sub-iterations, 0.04 exits inside the loop (egno 1 / 2; egno 3's err is a NaN, which never exits).
    fp64: the state to 1e-10 (test_multi_pass_vs_oracle's bar); mixed: K x the float32 loop's own distance from the
    float64 loop.  The exact checks on the decisions of the last sub-iteration, from the oracle's state before it."""
    P, state, _, _, _, _ = _reference((egno, 2) + MULTI_SHAPE, prec)
    rho, alp, pb = D.round_inputs(prec, *state)
    rho_o, alp_o, used_o, (rho_l, alp_l), errs = _loop(P, rho, alp, pb, 10, eps)
    stats = []
    rho_a, _ = O.update_dual_alternative(pb, rho, 70.0, alp, D.SIGMA, P["dt"], P["dsp"], P["epsl"], P["fns"],
                                         P["x_arr"], None, 2, P["bc"], rho_alp_iters=10, eps=eps, stats=stats)
    assert stats == [used_o] and np.array_equal(rho_a, rho_o)
    # a test condition: the exit is decided by a margin (no err within 5 % of eps), inside the loop for eps = 0.04
    assert all(np.isnan(e) or abs(e - eps) > 0.05 * eps for e in errs), errs
    assert used_o == 10 if (eps < 1e-3 or egno == 3) else 1 < used_o < 10, errs
    ref = D.reference(P, rho_l, alp_l, pb)          # the last sub-iteration
    assert np.array_equal(ref["rho"], rho_o)
    r = D.calibrate(P, rho_l, alp_l, pb)
    env = {"PDHG_DUAL_MULTI": "1" if form == "multi" else "0", "PDHG_DUAL_HEAD": "1" if form == "head" else "0"}
    expect = {"dual_multi": int(form == "multi"), "dual_head": int(form == "head"), "mixed": int(prec == "mixed")}
    ctx = _ctx(P, prec, env, expect, monkeypatch, rho_alp_iters=10)
    try:
        with _device():
            ctx.set_state(P["phi"], state[0], state[1])
            ctx.set_phi_bar(state[2])
            used = ctx.update_dual(D.SIGMA, eps, 10)
            _, rho_d, alp_d = ctx.get_state(phi=False)
    finally:
        ctx.close()
    measured = {"rho": rel(rho_d, rho_o)}
    for i, (a_d, a_o) in enumerate(zip(alp_d, alp_o)):
        measured["alp{}".format(i)] = rel(a_d, a_o)
    if prec == "fp64":
        bounds = {k: 1e-10 for k in measured}
    else:
        rho_32, alp_32, used_32, _, _ = _loop(P, *D.round_inputs("fp32", *state), 10, eps, np.float32)
        assert used_32 == used_o
        bounds = {"rho": D.K * rel(rho_32, rho_o)}
        for i, (a_32, a_o) in enumerate(zip(alp_32, alp_o)):
            bounds["alp{}".format(i)] = D.K * rel(a_32, a_o)
    fails = ["{}: rel L2 {:.3g} > {:.3g}".format(k, measured[k], bounds[k]) for k in bounds if not measured[k] <= bounds[k]]
    if used != used_o:
        fails.append("{} sub-iterations, the oracle {}".format(used, used_o))
    # exact values only: the point-wise bound belongs to one step from the same input, this state made several
    m_last, f_exact = D.check_device(P, ref, r, _u(prec), rho_d, alp_d, pointwise=False)
    measured.update({"last_step_" + k: v for k, v in m_last.items()})
    _finish(parity_log, "test_chunked_loop_from_clamp_state", "{}-e{}-{}-eps{:g}".format(prec, egno, form, eps),
            measured, bounds, fails + f_exact, r=r, sub_iterations=used)


