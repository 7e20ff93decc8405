"""--policy_check of the run_example-style driver, end to end on the C0 problem (egno 1, 1-D, nx = 160, nt = 41, windows
of time_step_per_PDHG = 2, capped iterations): the command line prints the worst and the last window's policy line,
and the solution it saves is bit for bit the one a run without the flag computes."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--egno", "1", "--ndim", "1", "--nx", "160", "--nt", "41", "--N_maxiter", "300", "--print_freq", "100",
        "--precision", "fp64"]


def test_policy_check_flag_prints_and_changes_nothing(native, tmp_path, capsys):
    from pdhg_amd import run_example as R, solver
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "pdhg-optimal-control_amd")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    out = subprocess.run([sys.executable, "-m", "pdhg_amd.run_example"] + ARGS +
                         ["--policy_check", "4", "--out", str(tmp_path / "a")], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=300).stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("policy check, ")]
    print("\n".join(lines))
    assert len(lines) == 2, out[-2000:]
    assert lines[0].startswith("policy check, worst window (solve ") and "policy gap (cost - value)" in lines[0]
    assert lines[1].startswith("policy check, last window (solve 39): ") and "0 of 4 samples non-finite" in lines[1]
    saved = glob.glob(str(tmp_path / "a" / "check_points" / "*" / "eg1_1d"))
    assert len(saved) == 1
    res_a, errs_a = solver.load_solution(saved[0], "nt41_nx160")
    capsys.readouterr()      # drop the lines printed above
    res_b, errs_b = R.main(ARGS + ["--out", str(tmp_path / "b")])
    assert "policy check" not in capsys.readouterr().out
    assert len(res_a) == len(res_b) == 1
    assert res_a[0][0] == res_b[0][0]
    for a, b in zip(res_a[0][1:], res_b[0][1:]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert len(errs_a) == len(errs_b) and all(np.array_equal(a, b) for a, b in zip(errs_a, errs_b))
