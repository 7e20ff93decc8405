"""The `case` labels of the five launchers' switches (parsed from csrc/ctx_impl.hpp) and the GPU test contexts that reach
them, from pdhg_plan_info on each GPU test table's problems and environments (no GPU needed).
python tests/_choice_cases.py prints profiles/plan_choice_cases.txt."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pdhg-optimal-control_amd", "csrc")
STAGES = ("xt", "xt_one_row", "res", "res_fused", "upd", "dual", "dual_fused")
PREC = {"fp32": 4, "fp64": 8, "mixed": 12}
# families launched through a line-FFT lift or with their own arguments, not through a case of the switch
NO_CASE = {"xt": ("XT_GENERIC",), "res": ("RES_GENERIC",), "upd": ("UPD_GENERIC", "UPD_GENERIC_MIXED"),
           "dual": ("DUAL_POINT", "DUAL_POINT_MIXED")}


def families():
    """{enumerator: code} of the stage enums of path_plan.hpp."""
    src = open(os.path.join(CSRC, "path_plan.hpp")).read()
    out = {}
    for body in re.findall(r"enum (?:Xt|Res|Upd|Dual)Kernel \{(.*?)\}", src, re.S):
        for i, name in enumerate(n.strip() for n in body.split(",")):
            out[name] = i
    return out


def switch_cases():
    """{launcher: {(family code, n, a, b, c)}} for every `case ck(...)` label of ctx_impl.hpp."""
    src = open(os.path.join(CSRC, "ctx_impl.hpp")).read()
    names = dict(families(), kMixedUpdPF=4)
    out = {}
    for fn, body in re.findall(r"\n  int (launch_\w+)\((.*?)\n  \}\n", src, re.S):
        for args in re.findall(r"case ck\(([^)]*)\):", body):
            v = [eval(a, {}, names) for a in args.split(",")]
            out.setdefault(fn, set()).add(tuple(v + [0] * (5 - len(v))))
    return out


LAUNCHER = {"xt": "launch_precond", "xt_one_row": "launch_precond", "res": "launch_residual",
            "res_fused": "launch_fused_residual", "upd": "launch_update_2d", "dual": "launch_dual_fast",
            "dual_fused": "launch_dual_fast"}


def planned(native, prec, egno, nx, ny, T, env, k=1):
    """{stage: (family, n, a, b, c)} of the 2-D context the problem and environment plan (None: refused)."""
    import record_plan_keys as rec
    keys = [s + suffix for s in STAGES for suffix in ("_kernel", "_n", "_a", "_b", "_c")]
    v = rec.plan_values(native, (PREC[prec], 2, egno, nx, ny, T, k), env, keys)
    return None if isinstance(v, int) else {s: tuple(v[5 * i:5 * i + 5]) for i, s in enumerate(STAGES)}


def gpu_contexts():
    """(test id, precision, egno, nx, ny, T, environment, rho_alp_iters, stages the test launches) for the contexts the
    GPU tests' own tables create; every one of these tests asserts its plan through path_info before it compares."""
    import test_gpu_configs as cfg
    import test_gpu_dual_clamps as dc
    import test_gpu_fused as fu
    import test_gpu_mixed as mx
    import test_gpu_one_text_bitwise as ot
    import test_gpu_precond2d as pc
    import test_plan_info as tpi
    ALL, FR = STAGES, {"PDHG_SHORT_T": "0"}
    for name in sorted(cfg.CASES):
        yield ("test_gpu_configs.py[{}]".format(name), "fp32") + tpi._meta(name)[:1] + tpi._meta(name)[2:] + (cfg.CASES[name][0], 1, ALL)
    for name in sorted(cfg.FP64_CASES):
        m = tpi._meta(name)
        yield ("test_gpu_configs.py[{}@fp64]".format(name), "fp64", m[0]) + m[2:] + (cfg.FP64_ENV.get(name.partition("+")[2], {}), 1, ALL)
    for name in sorted(cfg.ONE_STEP):
        egno, nx, ny, T, env, _ = cfg.ONE_STEP[name]
        yield ("test_gpu_configs.py::one step[{}]".format(name), "fp32", egno, nx, ny, T, env, 1, ALL)
    for name in sorted(mx.MIXED_CASES):
        egno, nx, ny, T, env, _ = mx.MIXED_CASES[name]
        yield ("test_gpu_mixed.py::test_mixed_instantiation[{}]".format(name), "mixed", egno, nx, ny, T, env, 1, ALL)
    for name, kern in pc.KERNELS.items():
        for env, _ in kern.variants:
            for T in kern.Ts:
                yield ("test_gpu_precond2d.py::test_primal_parameters[{}-*-T{}]".format(name, T), kern.prec, kern.egno,
                       kern.nx, kern.ny, T, env, 1, ("xt", "xt_one_row", "res", "upd"))
    for c in dc.CASES:
        egno, ndim, nx, ny, T, _ = c.problem
        if ndim == 2:
            yield ("test_gpu_dual_clamps.py::test_dual_clamps[{}]".format(c.name), c.prec, egno, nx, ny, T, c.env, 1,
                   ("dual_fused",) if c.fr else ("dual",))
    for c in ot.CASES:
        yield ("test_gpu_one_text_bitwise.py::test_state_hash_matches_recorded[{}]".format(c["id"]), c["prec"], c["egno"],
               c["nx"], c["ny"], c["T"], c["env"], c["rai"], ALL)
    import test_gpu_upd64_pair as up
    for c, cid in zip(up.PAIRED, up.IDS):
        yield ("test_gpu_upd64_pair.py::test_pair_form_bitwise[{}]".format(cid), "fp64", up.EGNO, c[0], c[1], c[2],
               dict({"PDHG_UPD_PAIR": "1"}, **({"PDHG_UPD_GRID": str(c[3])} if c[3] else {})), 1, ALL)
    for ny in (2048, 4096):
        for pf in (2, 3):
            yield ("test_gpu_upd64_pair.py::test_pair_prefetch_depths_bitwise[{}-{}]".format(pf, ny), "fp64", up.EGNO, 16, ny,
                   3, {"PDHG_UPD_PAIR": "1", "PDHG_UPD_PAIR_PF": str(pf)}, 1, ALL)
    for form, env in (("lds", {"PDHG_XT64_DMA": "0"}), ("bpr", {"PDHG_XT64_DMA": "0", "PDHG_XT64_BPR": "1"})):
        for flag in ("1", "0"):
            yield ("test_gpu_xt64.py::test_fp64_task_order_spectrum_x_forms[{}]".format(form), "fp64", 2, 4096, 4096, 3,
                   dict(env, PDHG_FUSE_RES="1", PDHG_SHORT_T="0", PDHG_TC_SPEC=flag), 1, ALL)
    for nx, T in ((4096, 37), (2048, 9), (1024, 4), (512, 3)):
        for batch in ("0", "1"):
            yield ("test_gpu_configs.py::test_batched_x_transform_matches_ws[{}-{}]".format(nx, T), "fp32", 2, nx, 256, T,
                   {"PDHG_XT_BATCH": batch, "PDHG_XT_DMA": "0"}, 1, ALL)
    for fuse in ("1", "0"):
        for flag in ("1", "0"):
            yield ("test_gpu_xt64.py::test_fp64_task_order_spectrum[{}]".format("fused" if fuse == "1" else "unfused"),
                   "fp64", 2, 4096, 4096, 6, {"PDHG_FUSE_RES": fuse, "PDHG_TC_SPEC": flag}, 1, ALL)
    for case, cid in list(zip(fu.FUSED, fu.IDS)) + list(zip(fu.FUSED64, fu.IDS64)):
        prec, test = ("fp32", "test_fused_matches_unfused") if case in fu.FUSED else ("fp64", "test_fused_fp64_vs_oracle_and_unfused")
        yield ("test_gpu_fused.py::{}[{}]".format(test, cid), prec, case[0], case[2], case[3], case[4],
               dict(FR, PDHG_FUSE_RES="1"), 1, ALL)


def reached(native):
    """{(launcher, case tuple): first test id}; a test's `dual` / `res` also run next to its fused forms (the first
    iteration's residual is unfused), so a fused context counts for both."""
    out = {}
    for tid, prec, egno, nx, ny, T, env, k, stages in gpu_contexts():
        plan = planned(native, prec, egno, nx, ny, T, env, k)
        if plan is None:
            continue
        for s in stages:
            if s == "xt" and plan["xt_one_row"][0]:
                continue   # the one-row kernel runs instead
            if s == "dual" and plan["dual_fused"][0] and k == 1 and "dual_fused" in stages:
                continue   # every in-place whole-window sweep is the fused one
            if plan[s][0]:
                out.setdefault((LAUNCHER[s], plan[s]), tid)
    return out


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(HERE, "golden"), os.path.join(ROOT, "pdhg-optimal-control_amd")):
        sys.path.insert(0, p)
    from pdhg_amd import _native
    prefix = {"launch_precond": "XT", "launch_residual": "RES", "launch_fused_residual": "RES", "launch_update_2d": "UPD",
              "launch_dual_fast": "DUAL"}
    code = {(k.split("_")[0].rstrip("1"), v): k for k, v in families().items()}
    hit = reached(_native)
    print("# One row per `case` of the five launchers' switches (csrc/ctx_impl.hpp): the first GPU test whose context plans it,\n"
          "# from pdhg_plan_info on the GPU tests' own tables (tests/_choice_cases.py; tests/test_plan_keys.py asserts that no\n"
          "# row is empty).  Each of these tests asserts its plan through path_info before it compares results.")
    for fn, cases in sorted(switch_cases().items()):
        for c in sorted(cases):
            print("{:22s} {:16s} ({:4d}, {:4d}, {:4d}, {:2d})   {}".format(fn, code[(prefix[fn], c[0])], *c[1:], hit.get((fn, c), "-- none --")))
