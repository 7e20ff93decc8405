"""The plan's choice of the fp64 update on 8-row task pairs ("upd64_pair", path_plan.hpp) without a device
(pdhg_plan_info): the expectations tests/test_gpu_upd64_pair.py asserts on its contexts, plus the shapes that must keep
today's kernels.  No GPU needed."""
import pytest

from test_plan_info import _plan, _problem


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


ENV = ("PDHG_UPD_PAIR", "PDHG_UPD_GRID", "PDHG_UPD_T1", "PDHG_RES64")
# (environment, (egno, ndim, nx, ny, T), precision, expected)
CASES = [
    # tests/test_gpu_upd64_pair.py
    *[({"PDHG_UPD_PAIR": f}, (2, 2, nx, ny, T), 8, {"res64": 1, "upd64_pair": int(f)})
      for f in ("1", "0") for nx, ny, T in ((8, 4096, 1), (16, 4096, 3), (40, 4096, 2), (8, 2048, 2), (24, 2048, 3),
                                          (2048, 2048, 2))],
    ({"PDHG_UPD_PAIR": "1", "PDHG_UPD_GRID": "3"}, (2, 2, 40, 4096, 2), 8, {"upd64_pair": 1, "upd_grid": 3}),
    ({"PDHG_UPD_PAIR": "0", "PDHG_UPD_GRID": "3"}, (2, 2, 40, 4096, 2), 8, {"upd64_pair": 0, "upd_grid": 3}),
    *[(env, (2, 2, 12, 4096, 2), 8, {"res64": 1, "upd64_pair": 0}) for env in ({"PDHG_UPD_PAIR": "1"}, {})],
    # the default: windows of >= 100 rows; the workgroups launched: one per pair / per 4-row task, 2048 at the most
    ({}, (2, 2, 40, 4096, 2), 8, {"upd64_pair": 0, "upd_grid": 20}),
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 40, 4096, 2), 8, {"upd64_pair": 1, "upd_grid": 10}),
    ({}, (2, 2, 4096, 4096, 200), 8, {"upd64_pair": 1, "upd_grid": 2048, "res64": 1}),
    ({"PDHG_UPD_PAIR": "0"}, (2, 2, 4096, 4096, 200), 8, {"upd64_pair": 0, "upd_grid": 2048}),
    ({}, (2, 2, 4096, 4096, 100), 8, {"upd64_pair": 1}),
    ({}, (2, 2, 4096, 4096, 99), 8, {"upd64_pair": 0}),
    ({}, (2, 2, 4096, 4096, 25), 8, {"upd64_pair": 0}),
    ({}, (2, 2, 2048, 2048, 100), 8, {"upd64_pair": 1, "upd_grid": 2048}),
    ({}, (2, 2, 8, 4096, 100), 8, {"upd64_pair": 1, "upd_grid": 100}),
    ({}, (2, 2, 12, 4096, 100), 8, {"upd64_pair": 0, "upd_grid": 300}),
    # ny = 2048 one-row windows keep the 256-thread forms unless those are switched off
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 2048, 2048, 1), 8, {"upd64_pair": 0, "upd_t1": 2}),
    ({"PDHG_UPD_PAIR": "1"}, (1, 2, 8, 2048, 1), 8, {"upd64_pair": 0, "upd_t1": 2}),
    ({"PDHG_UPD_PAIR": "1", "PDHG_UPD_T1": "0"}, (1, 2, 8, 2048, 1), 8, {"upd64_pair": 1, "upd_t1": 0}),
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 4096, 4096, 1), 8, {"upd64_pair": 1}),
    # not the fp64 4-row kernels: ny = 8192 (half-real form), other row lengths, the generic rows, fp32, mixed
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 8192, 8192, 3), 8, {"upd64_pair": 0, "upd8192": 1}),
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 16, 1024, 3), 8, {"upd64_pair": 0, "res64": 0}),
    ({"PDHG_UPD_PAIR": "1", "PDHG_RES64": "0"}, (2, 2, 16, 4096, 3), 8, {"upd64_pair": 0, "res64": 0}),
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 16, 4096, 3), 4, {"upd64_pair": 0}),
    ({"PDHG_UPD_PAIR": "1"}, (2, 2, 16, 4096, 3), 12, {"upd64_pair": 0, "mixed": 1}),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_upd64_pair_plan(lib, monkeypatch, i):
    env, shape, precision, expect = CASES[i]
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        assert name in ENV, name
        monkeypatch.setenv(name, v)
    p, keep = _problem(lib, *shape, precision=precision)
    got = {key: _plan(lib, p, key) for key in expect}
    assert got == expect, (env, shape, precision)
