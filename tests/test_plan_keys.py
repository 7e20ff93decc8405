"""The plan's keys over the grid recorded from the parent of the KernelChoice refactor (tests/golden/
plan_keys_parent.json, made by tests/golden/record_plan_keys.py): every key that existed then answers as it did, and
every "as launched" key equals what the stage's kernel choice ("<stage>_kernel" / "<stage>_shape") says.  Also: every
PDHG_* variable a test sets is one Tuning::from_env reads.  No GPU needed."""
import glob
import json
import os
import re

import pytest

import _choice_cases as cc
import record_plan_keys as rec

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pdhg-optimal-control_amd", "csrc")
GOLD = json.load(open(os.path.join(HERE, "golden", "plan_keys_parent.json")))
STAGES = ("xt", "xt_one_row", "res", "res_fused", "upd", "dual", "dual_fused")
NEW_KEYS = tuple(s + suffix for suffix in ("_kernel", "_shape", "_n", "_a", "_b", "_c") for s in STAGES)
# family codes (include/pdhg.h)
XT_FAST, XT_DMA_HR, XT_F64, XT1_F64, XT1_F64_G16 = 1, 5, 6, 9, 10
RES_FAST, RES_FAST64, RES_FUSED, RES_FUSED64 = 2, 3, 4, 5
UPD_FAST, UPD_FAST_MIXED, UPD_T1_G16, UPD_PAIR64, UPD_8192 = 3, 4, 6, 7, 8
DUAL_POINT, DUAL_POINT_MIXED, DUAL_ROW, DUAL_ROW_MIXED, DUAL_LDS = 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pdhg_amd import _native
    return _native


@pytest.fixture(scope="module")
def now(lib):
    """Every recorded case replayed against the current library: the old keys and the new ones."""
    keys = tuple(GOLD["keys"]) + NEW_KEYS
    return [rec.plan_values(lib, tuple(p), env, keys) for p, env, _ in GOLD["cases"]]


def test_grid_is_the_recorders():
    assert tuple(GOLD["keys"]) == rec.KEYS
    assert [(tuple(p), env) for p, env, _ in GOLD["cases"]] == rec.cases()


def test_existing_keys_keep_their_values(now):
    """Exactly the parent's table, except "res64_nt" where PDHG_RES64_NT=1024 applies: the fp64 fused residual at
    ny = 4096 runs 1024 threads there and the key now says so (the parent answered 512)."""
    i_nt, i_fr = GOLD["keys"].index("res64_nt"), GOLD["keys"].index("fused_residual")
    n_drift = 0
    for (p, env, want), got in zip(GOLD["cases"], now):
        if isinstance(want, int):
            assert got == want, (p, env)
            continue
        got = got[:len(want)]
        if env == "PDHG_RES64_NT=1024" and p[0] == 8 and p[4] == 4096 and want[i_fr] == 1:
            assert want[i_nt] == 512 and got[i_nt] == 1024, (p, env)
            want = want[:i_nt] + [1024] + want[i_nt + 1:]
            n_drift += 1
        assert got == want, (p, env, [k for k, a, b in zip(GOLD["keys"], got, want) if a != b])
    assert n_drift >= 1


def test_as_launched_keys_follow_the_choices(now):
    """Each legacy "as launched" key equals the value derived from the stage's choice: its family, threads and template
    integers (n, a, b, c as documented in include/pdhg.h)."""
    n = 0
    for (p, env, want), got in zip(GOLD["cases"], now):
        if isinstance(got, int):
            continue
        v = dict(zip(tuple(GOLD["keys"]) + NEW_KEYS, got))
        ctx = (p, env, v)
        xt, xt1, res, resf, upd, dual, dualf = (v[s + "_kernel"] for s in STAGES)
        if p[1] == 1:   # 1-D: no 2-D stage
            assert [v[k] for k in NEW_KEYS] == [0] * len(NEW_KEYS), ctx
            continue
        n += 1
        assert v["fast_xt"] == (xt if XT_FAST <= xt <= XT_DMA_HR else 0), ctx
        assert v["t1_xt64"] == int(xt1 in (XT1_F64, XT1_F64_G16)) and v["t1_g16"] == int(xt1 == XT1_F64_G16), ctx
        col_pair_4096 = xt == XT_F64 and v["xt_n"] == 4096 and v["xt_b"] == 0   # not the half-real form
        assert v["xt64_bpr"] == int(col_pair_4096 and v["xt_c"] & 1 != 0), ctx
        assert v["xt64_dma"] == int(col_pair_4096 and v["xt_c"] & 4 != 0), ctx
        assert v["tc_spec"] == int(xt == XT_F64 and v["xt_c"] & 2 != 0), ctx
        assert v["rows_rw"] == (v["res_a"] if res == RES_FAST else 0), ctx
        assert v["res_threads"] == (0 if res != RES_FAST else v["res_fused_shape"] if resf else v["res_shape"]), ctx
        assert resf in ((0, RES_FUSED) if res == RES_FAST else (0, RES_FUSED64)) and (resf != 0) == v["fused_residual"], ctx
        assert (dualf != 0) == v["fused_residual"], ctx
        assert v["res64_nt"] == (0 if res != RES_FAST64 else 1024 if v["res_fused_shape"] == 1024 else v["res_shape"]), ctx
        assert v["upd_threads"] == (v["upd_shape"] if upd in (UPD_FAST, UPD_FAST_MIXED) else 0), ctx
        assert v["upd_t1"] == (0 if upd != UPD_T1_G16 else 2 if v["upd_c"] == 2 else 1), ctx
        assert v["upd64_pair"] == int(upd == UPD_PAIR64), ctx
        assert v["upd8192"] == int(upd == UPD_8192), ctx
        assert v["fast_dual"] == (-1 if dual in (DUAL_POINT, DUAL_POINT_MIXED) else v["dual_a"] if dual == DUAL_LDS else 0), ctx
        assert v["dual_ypl"] == (v["dual_b"] if dual == DUAL_LDS else 0), ctx
        assert dual != DUAL_LDS or v["dual_shape"] == 64 * v["dual_a"], ctx   # RX waves per workgroup
        assert v["dual_one"] == int(dual in (DUAL_ROW, DUAL_ROW_MIXED) and v["dual_a"] != 0), ctx
    assert n > 1000


def test_every_planned_choice_has_a_case(now):
    """Over the grid: the (family, n, a, b, c) each stage plans is a `case` label of that stage's launcher (parsed from
    csrc/ctx_impl.hpp), so no planned context can end in the launchers' "no kernel" error."""
    cases, fam = cc.switch_cases(), cc.families()
    no_case = {s: {fam[n] for n in names} for s, names in cc.NO_CASE.items()}
    n = 0
    for (p, env, _), got in zip(GOLD["cases"], now):
        if isinstance(got, int) or p[1] == 1:
            continue
        v = dict(zip(tuple(GOLD["keys"]) + NEW_KEYS, got))
        for s in STAGES:
            c = tuple(v[s + x] for x in ("_kernel", "_n", "_a", "_b", "_c"))
            if c[0] and c[0] not in no_case.get(s, ()):
                assert c in cases[cc.LAUNCHER[s]], (p, env, s, c)
                n += 1
    assert n > 3000


def test_every_case_is_reached_by_a_gpu_test(lib):
    """Every `case` of the five switches is planned by a context of a GPU test's own table (profiles/
    plan_choice_cases.txt is this map, printed by tests/_choice_cases.py)."""
    hit = cc.reached(lib)
    missing = sorted((fn, c) for fn, cs in cc.switch_cases().items() for c in cs if (fn, c) not in hit)
    assert not missing, missing


def _env_names_read():
    """The PDHG_* names the three from_env() functions of tuning.hpp read."""
    src = open(os.path.join(CSRC, "tuning.hpp")).read()
    bodies = re.findall(r"static \w+ from_env\(\) \{(.*?)\n  \}", src, re.S)
    assert len(bodies) == 3
    return set(re.findall(r'"(PDHG_[A-Z0-9_]+)"', "".join(bodies)))


def test_tests_set_only_variables_the_library_reads():
    """A PDHG_* variable a test puts into the environment (a string literal in tests/*.py) that no from_env() reads
    would be a switch that silently does nothing."""
    not_the_librarys = {"PDHG_TESTS", "PDHG_PARITY_LOG", "PDHG_DIST_BACKEND", "PDHG_RECORD_COMMIT"}   # tests' / bench.py's own
    # (PDHG_RECORD_COMMIT: test_gpu_one_text_bitwise.py, when it records its fixture)
    read = _env_names_read()
    assert set(rec.ENVS) <= read
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        used = set(re.findall(r'["\'](PDHG_[A-Z0-9_]+)["\']', open(path).read()))
        stray = {n for n in used - read - not_the_librarys if not n.startswith("PDHG_ERR_") and n != "PDHG_OK"}
        assert not stray, (os.path.basename(path), sorted(stray))
