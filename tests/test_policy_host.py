"""The policy check (pdhg_policy_eval), the parts that need no device: the NumPy form of the definition
(pdhg_amd.policy.policy_from_arrays) against a per-sample restatement on the trajectory oracle, the symbol in the
header, the binding and the library, the two structs' sizes, and the Python argument refusals."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import _policy_support as PS
import _traj_support as S

CASES = [(1, e, m) for e, m in S.CASES_1D] + [(2, e, m) for e, m in S.CASES_2D]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


def _host(P, phi, alp, epsl, method, noise, terminal):
    from pdhg_amd.policy import policy_from_arrays
    from pdhg_amd.set_fns import set_up_example_fns
    fns = set_up_example_fns(P["egno"], P["ndim"], 0)
    return policy_from_arrays(phi, tuple(alp), fns, P["x0"], P["x_arr"], P["dt"], S.P_SPACE, S.P_SPACE, P["bc"],
                              P["center"], epsl, method, noise, terminal)


@pytest.mark.parametrize("epsl", [0.0, 0.1])
@pytest.mark.parametrize("ndim,egno,method", CASES, ids=["{}d_e{}_{}".format(*c) for c in CASES])
def test_numpy_policy_matches_oracle(ndim, egno, method, epsl):
    P = S.problem(egno, ndim)
    phi, alp = PS.random_phi(P), S.random_alp(P)
    noise = S.noise_for(P, len(P["x0"])) if epsl > 0 else None
    for terminal in ("phi0", "none"):
        ref = PS.oracle_policy(P, phi, alp, P["x0"], epsl, method, noise, terminal)
        S.assert_margins(P, alp, ref["traj_x"], method)
        got = _host(P, phi, alp, epsl, method, noise, terminal)
        for k in ("running", "terminal", "value", "x_final"):
            dev = S.deviation(got[k], ref[k])
            print("{} {}: max |got - ref| / (atol + rtol |ref|) = {:.3e}".format(terminal, k, dev))
            assert got[k].shape == ref[k].shape
            assert np.allclose(got[k], ref[k], rtol=S.RTOL, atol=S.ATOL), (terminal, k, dev)
        if terminal == "none":
            assert not got["terminal"].any()
    assert egno == 2 or np.abs(ref["running"]).max() > 1e-3      # the cost is live (egno 2: L = 0 a^2)
    assert egno != 2 or not ref["running"].any()


@pytest.mark.parametrize("ndim,egno,method", CASES, ids=["{}d_e{}_{}".format(*c) for c in CASES])
def test_running_does_not_rest_on_summation_order(ndim, egno, method):
    """The T step costs added forward (the definition) and pairwise differ by at most a tenth of the parity bound."""
    P = S.problem(egno, ndim)
    phi, alp = PS.random_phi(P), S.random_alp(P)
    noise = S.noise_for(P, len(P["x0"]))
    whole = PS.oracle_policy(P, phi, alp, P["x0"], 0.1, method, noise, "phi0")
    fwd = whole["running"]
    steps = []
    for j in range(P["T"]):          # step j alone: the oracle on alp row T-1-j from the position the path has there
        pos = whole["traj_x"][j]
        Pj = dict(P, T=1)
        row = P["T"] - 1 - j
        one = PS.oracle_policy(Pj, phi[row:row + 2], alp[:, row:row + 1], pos, 0.1, method, noise[j:j + 1], "none")
        steps.append(one["running"])
    assert P["T"] == 4
    pair = (steps[0] + steps[1]) + (steps[2] + steps[3])
    chain = ((steps[0] + steps[1]) + steps[2]) + steps[3]
    assert np.array_equal(chain, fwd)
    gap = np.abs(pair - fwd)
    print("forward against pairwise: max {:.3e}".format(gap.max()))
    assert np.all(gap <= 0.1 * (S.ATOL + S.RTOL * np.abs(fwd)))


def test_symbol_is_declared_bound_and_exported(lib):
    import test_abi
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pdhg_\w+)", out))
    L = lib.load()
    f = "pdhg_policy_eval"
    assert f in test_abi.header_functions() and f in lib.EXPORTS and f in exported
    assert getattr(L, f).restype is ctypes.c_int and len(getattr(L, f).argtypes) == 9
    assert L.pdhg_abi_version() == 1


def test_struct_sizes_match_the_header(lib):
    assert ctypes.sizeof(lib.pdhg_policy_opts) == ctypes.sizeof(lib.pdhg_traj_opts) + 4 * 4
    assert ctypes.sizeof(lib.pdhg_policy_report) == 2 * 8 + 10 * 8
    assert [f for f, _ in lib.pdhg_policy_opts._fields_] == ["traj", "terminal", "stride_x", "stride_y", "reserved0"]
    assert lib.POLICY_FIELDS == ("n_sample", "n_nonfinite", "cost_mean", "value_mean", "running_mean",
                                 "terminal_mean", "gap_mean", "gap_abs_mean", "gap_rms", "gap_abs_max", "gap_lo",
                                 "gap_hi")


def test_null_handle_and_opts_are_refused_before_any_device(lib):
    L = lib.load()
    po, rep = lib.pdhg_policy_opts(), lib.pdhg_policy_report()
    assert L.pdhg_policy_eval(None, ctypes.byref(po), None, None, ctypes.byref(rep), None, None, None, None) == \
        lib.PDHG_ERR_ARG
    assert L.pdhg_last_error().decode()


class _NoNative:
    """Stands where a context keeps its library and handle: any native call is a test failure."""

    def __getattr__(self, name):
        raise AssertionError("native call {} before the argument check".format(name))


def _ctx(ndim):
    from pdhg_amd.context import PDHGContext
    c = object.__new__(PDHGContext)
    c.ndim, c.T, c.nx, c.ny, c.n_ctrl = ndim, 4, 16, (12 if ndim == 2 else 1), ndim
    c._lib, c._h = _NoNative(), None
    return c


BAD_2D = [
    dict(),                                                       # neither x_init nor stride
    dict(x_init=np.zeros((4, 2)), stride=2),                      # both
    dict(x_init=np.zeros(4)), dict(x_init=np.zeros((4, 3))), dict(x_init=np.zeros((0, 2))),
    dict(stride=0), dict(stride=(2, 0)), dict(stride=(2, 2, 2)), dict(stride=1.5),
    dict(stride=2, method="cubic"), dict(stride=2, terminal="g"), dict(stride=2, outputs=("cost",)),
    dict(stride=2, x_period=0.0), dict(stride=2, y_period=None), dict(stride=2, y_period=-1.0),
    dict(stride=2, center=(True,)), dict(stride=2, seed=-1), dict(stride=2, sample_offset=-1),
    dict(stride=(4, 3), noise=np.zeros((4, 15, 2))),              # 4 * 4 = 16 grid starts, not 15
    dict(x_init=np.zeros((5, 2)), noise=np.zeros((3, 5, 2))),
]


@pytest.mark.parametrize("kw", BAD_2D, ids=[str(i) for i in range(len(BAD_2D))])
def test_python_refusals_come_before_any_native_call_2d(kw):
    kw = dict(dict(x_period=2.0, y_period=2.0), **kw)
    with pytest.raises(ValueError) as e:
        _ctx(2).policy_eval(**kw)
    assert str(e.value)


@pytest.mark.parametrize("kw", [dict(x_init=np.zeros((4, 2))), dict(stride=(2, 2)), dict(stride=-1),
                                dict(stride=8, noise=np.zeros((4, 5)))])
def test_python_refusals_come_before_any_native_call_1d(kw):
    with pytest.raises(ValueError):
        _ctx(1).policy_eval(x_period=2.0, **kw)


def test_python_surface():
    import inspect
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.multi import MultiContext
    from pdhg_amd.slab import SlabContext
    from pdhg_amd.xslab import XSlabContext
    want = inspect.signature(PDHGContext.policy_eval)
    assert list(want.parameters)[1:] == ["x_init", "stride", "method", "x_period", "y_period", "center", "noise",
                                         "seed", "sample_offset", "terminal", "outputs"]
    assert inspect.signature(MultiContext.policy_eval) == want
    # the decomposed single-device contexts keep the (refused) call: nothing of that name is defined on them
    assert "policy_eval" not in vars(SlabContext) and "policy_eval" not in vars(XSlabContext)


def test_policy_check_flag(tmp_path):
    from pdhg_amd import run_example as R
    ap = R.build_parser()
    assert ap.parse_args([]).policy_check == 0
    assert ap.parse_args(["--policy_check"]).policy_check == -1          # N = --plot_traj_num_1d
    assert ap.parse_args(["--policy_check", "4"]).policy_check == 4
    with pytest.raises(SystemExit):                                      # ... which defaults to 0: no starts
        R.main(["--policy_check", "--save", "0", "--out", str(tmp_path)])


def test_report_from_samples_and_format():
    from pdhg_amd.policy import format_policy, policy_report_from_samples
    r, t, v = np.array([1.0, 2.0, np.nan, 4.0]), np.array([0.5, 0.5, 0.5, np.inf]), np.array([1.0, 3.0, 1.0, 1.0])
    d = policy_report_from_samples(r, t, v)
    assert (d["n_sample"], d["n_nonfinite"]) == (4, 2)
    assert d["cost_mean"] == 2.0 and d["value_mean"] == 2.0 and d["running_mean"] == 1.5 and d["terminal_mean"] == 0.5
    assert d["gap_mean"] == 0.0 and d["gap_abs_mean"] == 0.5 and d["gap_rms"] == 0.5
    assert (d["gap_lo"], d["gap_hi"], d["gap_abs_max"]) == (-0.5, 0.5, 0.5)
    line = format_policy(d)
    assert "\n" not in line and "2 of 4" in line
    none = policy_report_from_samples([np.nan], [0.0], [0.0])
    assert none["n_nonfinite"] == 1 and all(np.isnan(x) for k, x in none.items() if not k.startswith("n_"))
    assert "\n" not in format_policy(none)
