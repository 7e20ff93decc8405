"""The rollout and the policy check reproduce, bit for bit, what their kernels returned when each carried its own
copy of the time step (tests/golden/make_rollout_fixture.py, recorded on the GPU at the commit before
traj_step_1d / traj_step_2d of csrc/kernels_traj.hpp): positions, records, per-sample costs and phi reads as arrays,
the report's fields as exact floats and ints."""
import os

import numpy as np
import pytest

import _policy_support as PS
import _traj_support as S
import make_rollout_fixture as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", os.path.basename(F.OUT)))
    return {k: d[k] for k in d.files}


def test_fixture_inputs_are_the_suites(recorded):
    d = recorded
    assert (int(d["seed_hi"]) << 32) | int(d["seed_lo"]) == F.SEED and int(d["offset"]) == F.OFFSET
    assert int(d["seed_hi"]) != 0 and int(d["seed_lo"]) != 0 and F.OFFSET > 1 << 32
    assert np.array_equal(d["in/wide_x0"], F.wide_x0()) and len(F.wide_x0()) % 256 != 0 and len(F.wide_x0()) > 256
    seen = set()
    for case in F.CASES:
        if case[0] == "wide" or (case[1], case[2]) in seen:
            continue
        seen.add((case[1], case[2]))
        P = S.problem(case[2], case[1])
        tag = "in/{}d_e{}/".format(case[1], case[2])
        assert np.array_equal(d[tag + "x0"], P["x0"]) and np.array_equal(d[tag + "alp"], S.random_alp(P))
        assert np.array_equal(d[tag + "phi"], PS.random_phi(P))
        assert np.array_equal(d[tag + "noise"], S.noise_for(P, len(P["x0"])))
    # every case of the policy parity list, three noise settings each; the grid starts; the two-workgroup call
    assert len(F.PARITY) == 2 * (len(S.CASES_1D) + len(S.CASES_2D)) + 1 == 11
    assert len(F.CASES) == 3 * len(F.PARITY) + len(F.GRID) + 1


@pytest.mark.parametrize("case", F.CASES, ids=[F.case_id(c) for c in F.CASES])
def test_outputs_are_the_recorded_bits(native, recorded, case):
    got = F.run(case)
    want = {k[len(F.case_id(case)) + 1:]: v for k, v in recorded.items() if k.startswith(F.case_id(case) + "/")}
    assert sorted(got) == sorted(want) and len(got) >= 2
    bad = []
    for k in sorted(got):
        g, w = np.asarray(got[k]), want[k]
        same = g.shape == w.shape and g.dtype.kind == w.dtype.kind and np.array_equal(g, w, equal_nan=True)
        if not same:
            print("{} {}: got {!r}, recorded {!r}".format(F.case_id(case), k, got[k], w))
            bad.append(k)
    assert not bad, bad
