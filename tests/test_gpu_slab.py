"""t-slab decomposition on the GPU: P slab contexts on one device, exchanging planes
through LocalComm, must reproduce the single-context iteration (pdhg_iterate) of the same window --
same state after n outer iterations within fp32 rounding, same error history and stop decisions, for
both carry exchanges (neighbour planes + long-range modes, or the full allgather) and with the halos
overlapped or serial.
The single-context path is itself pinned to the oracle by test_gpu_parity.py."""
import numpy as np
import pytest

from _problems import make_problem, rel

pytestmark = pytest.mark.gpu

CASES = [
    # (egno, nx, ny, T, P, k)   the x kernel follows the SLAB's row count (path asserted in the test):
    # nx = 512: k_precond_xt_fast_2d; nx = 4096: k_precond_xt_dma_2d for slabs of >= 4 rows, else the
    # single-role k_precond_xt_fast_2d (k_precond_xt_ws_2d: test_ws_slabs below)
    (1, 512, 256, 6, 2, 1),
    (2, 512, 256, 7, 3, 1),
    (1, 512, 256, 5, 5, 3),
    (2, 4096, 256, 6, 2, 1),     # 3-row slabs: single-role
    (1, 4096, 256, 4, 3, 2),
    (2, 4096, 256, 50, 2, 1),    # 25-row slabs (C3's slab length on 8 GPUs): LDS-DMA x transform
    (2, 4096, 256, 11, 2, 1),    # 6 + 5 rows: LDS-DMA x transform with partial last batches
    (2, 8192, 256, 5, 2, 1),    # half-real x blocks (C4's nx): warp-specialised (slabs < 4 rows)
    (2, 8192, 256, 16, 2, 1),   # half-real LDS-DMA x transform's slab phases (8-row slabs)
    (1, 512, 256, 3, 3, 1),     # one-row slabs: the halo row is the whole slab
    (2, 512, 256, 19, 2, 1),    # residual tiles of 8 rows + untiled remainder rows
    (2, 512, 256, 40, 4, 1),    # 10-row slabs: short-range modes take the neighbour-only carries
    # egno 3 (bc (1, 0): DCT-II along x, utils_precond.py:159-174): the generic x kernel's slab phases
    (3, 512, 256, 9, 3, 1),
    (3, 384, 256, 12, 2, 2),    # non-power-of-two nx (runtime-radix plan), dual sub-iterations
    (3, 4096, 256, 8, 2, 1),    # C3's x extent (B = 2 column blocks)
]


def _slabs(P, nranks, k, **kw):
    from pdhg_amd.slab import SlabContext
    return [SlabContext(r, nranks, P["T"], P["egno"], P["nx"], P["ny"], P["dx"], P["dy"], P["dt"], P["xs"], P["ys"],
                        epsl=P["epsl"], rho_alp_iters=k, **kw) for r in range(nranks)]


MODES = [(True, "neighbour", "overlap-nb"), (False, "neighbour", "serial-nb"), (True, "allgather", "overlap-ag")]
# every case in the bench's schedule (overlapped halos, neighbour carries); the serial and allgather schedules on
# the first case only by default, on every case in the extended tier (PDHG_TESTS=full)
PARAMS, PARAM_IDS = [], []
for ci, c in enumerate(CASES):
    for ov, ex, mid in MODES:
        marks = () if (mid == "overlap-nb" or ci == 0) else (pytest.mark.extended,)
        PARAMS.append(pytest.param(*c, ov, ex, marks=marks))
        PARAM_IDS.append(f"e{c[0]}_{c[1]}x{c[2]}_T{c[3]}_P{c[4]}_k{c[5]}-{mid}")


@pytest.mark.parametrize("egno,nx,ny,T,nr,k,overlap,exchange", PARAMS, ids=PARAM_IDS)
def test_slabs_match_single_context(native, egno, nx, ny, T, nr, k, overlap, exchange):
    import torch
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.slab import LocalComm, SlabRunner, join_state, slab_bounds, split_state
    P = make_problem(egno, 2, nx, ny, T, 0.0)
    # egno 3 at dx = 2/4096 from the seeded state diverges in the single context as well (NaN at iteration 5,
    # scripts/diag_slab.py; err2 is inf from iteration 4): 3 iterations there
    tau, sigma, n = 0.1 / 1.5, 0.1 * 1.5, (3 if (egno == 3 and nx >= 4096) else 6)
    ref = PDHGContext(egno, 2, nx, ny, T, P["dx"], P["dy"], P["dt"], P["xs"], P["ys"], epsl=0.0,
                      precision="fp32", rho_alp_iters=k)
    ref.set_state(P["phi"], P["rho"], P["alp"])
    st_ref = ref.iterate(n, tau, sigma, -1.0, k)
    phi_r, rho_r, alp_r = ref.get_state()

    slabs = _slabs(P, nr, k)
    for s in slabs:   # the x kernel the slab runs (see CASES)
        if egno == 3:
            assert s.path_info("fast_xt") == 0   # the generic runtime-radix DCT kernel
        elif nx == 4096:
            assert s.path_info("fast_xt") == (4 if s.T >= 4 else 1), (s.T, s.path_info("fast_xt"))
    for s, part in zip(slabs, split_state(P["phi"], P["rho"], P["alp"], slab_bounds(T, nr))):
        s.set_state(*part)
    runner = SlabRunner(slabs, LocalComm(nr), overlap=overlap, exchange=exchange)
    if exchange == "neighbour":
        assert 0 <= runner.n_long <= nx * ny
        if T // nr >= 8:        # long slabs: most modes exchange with the neighbours only
            assert runner.n_long < nx * ny // 4
    st = runner.iterate(n, tau, sigma, -1.0, k)
    torch.cuda.synchronize()
    phi_s, rho_s, alp_s = join_state([s.get_state() for s in slabs])
    assert st["iters"] == st_ref["iters_run"] == n
    assert rel(phi_s, phi_r) < 2e-5
    assert rel(rho_s, rho_r) < 2e-4
    assert rel(np.stack(alp_s), np.stack(alp_r)) < 2e-4
    assert abs(st["err1"] - st_ref["err1"]) <= 1e-3 * st_ref["err1"]
    assert abs(st["err2"] - st_ref["err2"]) <= 1e-3 * st_ref["err2"]
    for s in slabs:
        s.close()
    ref.close()


@pytest.mark.extended
@pytest.mark.parametrize("env,path", [({"PDHG_XT_BATCH": "0"}, 2), ({"PDHG_XT_BATCH": "1", "PDHG_XT_DMA": "0"}, 3)],
                         ids=["ws", "batched"])
def test_ws_slabs(native, monkeypatch, env, path):
    """The warp-specialised (PDHG_XT_BATCH=0, slabs of >= 16 rows) and the register-staged batched x transforms
    through the slab phases (forward sweep, carry fix-up, backward sweep from the right carry) against the
    single context (the default LDS-DMA kernel runs the CASES above)."""
    import torch
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.slab import LocalComm, SlabRunner, join_state, slab_bounds, split_state
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    P = make_problem(2, 2, 4096, 256, 40, 0.0)
    tau, sigma, n = 0.1 / 1.5, 0.1 * 1.5, 4
    ref = PDHGContext(2, 2, 4096, 256, 40, P["dx"], P["dy"], P["dt"], P["xs"], P["ys"], precision="fp32")
    assert ref.path_info("fast_xt") == path
    ref.set_state(P["phi"], P["rho"], P["alp"])
    ref.iterate(n, tau, sigma, -1.0, 1)
    phi_r, rho_r, _ = ref.get_state()
    slabs = _slabs(P, 2, 1)
    assert all(s.path_info("fast_xt") == path for s in slabs)
    for s, part in zip(slabs, split_state(P["phi"], P["rho"], P["alp"], slab_bounds(40, 2))):
        s.set_state(*part)
    SlabRunner(slabs, LocalComm(2)).iterate(n, tau, sigma, -1.0, 1)
    torch.cuda.synchronize()
    phi_s, rho_s, _ = join_state([s.get_state() for s in slabs])
    assert rel(phi_s, phi_r) < 2e-5 and rel(rho_s, rho_r) < 2e-4
    for s in slabs:
        s.close()
    ref.close()


def test_slab_rejects_unsupported(native):
    from pdhg_amd import _native as N
    from pdhg_amd.slab import SlabContext
    P = make_problem(1, 2, 48, 40, 4, 0.0)
    with pytest.raises(N.PDHGError):      # ny = 40: no fast row kernel (the halo row split of the residual)
        SlabContext(0, 2, 4, 1, 48, 40, P["dx"], P["dy"], P["dt"], P["xs"], P["ys"])


FUSED_CASES = [
    # (egno, nx, ny, T, P): the fused residual (k_dual_lds_2d FR + k_res_fwdy_fused_2d) inside t-slabs
    (1, 512, 256, 6, 2),
    (2, 512, 256, 7, 3),
    (2, 4096, 256, 6, 2),      # 3-row slabs: single-role x transform
    (2, 4096, 256, 16, 2),     # 8-row slabs: batched x transform
    (1, 512, 256, 3, 3),       # one-row slabs: the halo launch is the whole slab
    (2, 512, 256, 19, 2),      # residual tiles of 8 rows + remainder rows
    (2, 64, 8192, 8, 2),       # ny = 8192 (C4): 4-row half-tile tasks, XCD-ordered
]


@pytest.mark.parametrize("egno,nx,ny,T,nr", FUSED_CASES,
                         ids=[f"e{c[0]}_{c[1]}x{c[2]}_T{c[3]}_P{c[4]}" for c in FUSED_CASES])
def test_slabs_fused_residual(native, egno, nx, ny, T, nr, monkeypatch):
    """The dual sweep forms the next residual inside every slab (two launches: the rows without the phi_bar
    halo, then row 0 with rho'_1 read back); the slab's last row gets the next slab's rho/dt from the halo
    in k_res_fwdy_fused_2d.  Must match the fused single context."""
    import torch
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.slab import LocalComm, SlabRunner, join_state, slab_bounds, split_state
    monkeypatch.setenv("PDHG_FUSE_RES", "1")
    monkeypatch.setenv("PDHG_SHORT_T", "0")
    P = make_problem(egno, 2, nx, ny, T, 0.0)
    tau, sigma, n = 0.1 / 1.5, 0.1 * 1.5, 6
    ref = PDHGContext(egno, 2, nx, ny, T, P["dx"], P["dy"], P["dt"], P["xs"], P["ys"], precision="fp32")
    assert ref.path_info("fused_residual") == 1
    ref.set_state(P["phi"], P["rho"], P["alp"])
    st_ref = ref.iterate(n, tau, sigma, -1.0, 1)
    phi_r, rho_r, alp_r = ref.get_state()
    slabs = _slabs(P, nr, 1)
    for s in slabs:
        assert s.path_info("fused_residual") == 1
    for s, part in zip(slabs, split_state(P["phi"], P["rho"], P["alp"], slab_bounds(T, nr))):
        s.set_state(*part)
    st = SlabRunner(slabs, LocalComm(nr)).iterate(n, tau, sigma, -1.0, 1)
    torch.cuda.synchronize()
    phi_s, rho_s, alp_s = join_state([s.get_state() for s in slabs])
    assert st["iters"] == st_ref["iters_run"] == n
    assert rel(phi_s, phi_r) < 2e-5
    assert rel(rho_s, rho_r) < 2e-4
    assert rel(np.stack(alp_s), np.stack(alp_r)) < 2e-4
    assert abs(st["err1"] - st_ref["err1"]) <= 1e-3 * st_ref["err1"]
    for s in slabs:
        s.close()
    ref.close()


@pytest.mark.parametrize("C,dt", [(0.0, 1 / 400), (100.0, 1 / 40)], ids=["C0_dt1/400", "C100_dt1/40"])
def test_slabs_fused_solve_parameter(native, parity_log, monkeypatch, C, dt):
    """The fp32 slab phases at nx = 4096 (8-row slabs: the LDS-DMA x transform; fused residual) with the solve
    parameter away from C = 1: at C = 0 the zero mode's carry gain stops decaying, so the long-range set cannot shrink
    (K(C = 0) >= K(C = 1), both logged).  Against the fused single context with the same (C, dt), the bounds of
    test_slabs_fused_residual."""
    import torch
    from pdhg_amd.context import PDHGContext
    from pdhg_amd.slab import LocalComm, SlabRunner, join_state, slab_bounds, split_state
    monkeypatch.setenv("PDHG_FUSE_RES", "1")
    monkeypatch.setenv("PDHG_SHORT_T", "0")
    egno, nx, ny, T, nr = 2, 4096, 256, 16, 2
    P = make_problem(egno, 2, nx, ny, T, 0.0, dt=dt)
    tau, sigma, n = 0.1 / 1.5, 0.1 * 1.5, 6
    ref = PDHGContext(egno, 2, nx, ny, T, P["dx"], P["dy"], dt, P["xs"], P["ys"], precision="fp32", C=C)
    slabs = []
    try:
        assert ref.path_info("fused_residual") == 1 and ref.path_info("fast_xt") == 4
        ref.set_state(P["phi"], P["rho"], P["alp"])
        st_ref = ref.iterate(n, tau, sigma, -1.0, 1)
        phi_r, rho_r, alp_r = ref.get_state()
        Ks = {}
        for Ck in (1.0, C):   # the long-range mode count at C = 1 and at this C
            slabs = _slabs(P, nr, 1, C=Ck)
            runner = SlabRunner(slabs, LocalComm(nr))
            Ks[Ck] = runner.n_long
            if Ck != C:
                for s in slabs:
                    s.close()
        for s in slabs:
            assert s.path_info("fused_residual") == 1 and s.path_info("fast_xt") == 4
        for s, part in zip(slabs, split_state(P["phi"], P["rho"], P["alp"], slab_bounds(T, nr))):
            s.set_state(*part)
        st = runner.iterate(n, tau, sigma, -1.0, 1)
        torch.cuda.synchronize()
        phi_s, rho_s, alp_s = join_state([s.get_state() for s in slabs])
    finally:
        for s in slabs:
            s.close()
        ref.close()
    m = {"phi": rel(phi_s, phi_r), "rho": rel(rho_s, rho_r), "alp": rel(np.stack(alp_s), np.stack(alp_r)),
         "err1": abs(st["err1"] - st_ref["err1"]) / st_ref["err1"]}
    b = {"phi": 2e-5, "rho": 2e-4, "alp": 2e-4, "err1": 1e-3}
    parity_log("test_slabs_fused_solve_parameter", "e2_4096x256_T16_P2_C{:g}_dt{:g}".format(C, dt), m, b, K=Ks[C],
               K_C1=Ks[1.0])
    assert st["iters"] == st_ref["iters_run"] == n
    assert all(0 <= K <= nx * ny for K in Ks.values())
    if C == 0.0:
        assert Ks[C] >= Ks[1.0], Ks
    assert all(m[q] < b[q] for q in m), (m, b)
