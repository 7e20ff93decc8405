"""Static check of the counted wait of the fp64 LDS-DMA x transform (CPU, no GPU needed).

k_precond_xt_f64_2d<4096, 512, false, true, TC, true> (csrc/kernels_xt_f64.hpp) stages the next forward row
HBM -> LDS with global_load_lds_dwordx4 and retires it one step later with ``s_waitcnt vmcnt(8)``: the 8 row stores
of the step are the only vector-memory operations issued after the DMA, so at most 8 outstanding means the (older)
DMA has landed.  The staged row is read by inline-asm ds_reads the compiler cannot see as depending on the DMA, so
the wait is only right if the generated code really has >= N vector-memory operations between the last DMA and
every ``vmcnt(N)`` (N > 0), in program order.  This test disassembles the built library and checks that for both
instantiations (blocked and task-order input), as tests/test_isa_dma.py does for the fp32 kernel; it looks at vmcnt
and the load / store mnemonics only.  Counted waits the compiler emits for its own loads before the first DMA of the
program (the set-up's table loads) have no DMA to retire and are not counted.
"""
import os
import re
import shutil

import pytest

from test_isa_dma import LIB, TOOLS, VMEM, _disassemble, _kernel_bodies

SYMBOL = "k_precond_xt_f64_2dILi4096ELi512ELb0ELb1ELb{}ELb1E"   # <4096, 512, HR = 0, BPR = 1, TC, DMA = 1>


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    return _disassemble(tmp_path_factory.mktemp("isa_xt64"))


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpdhg.so not built (run __graft_entry__.build())")
@pytest.mark.skipif(not all(os.path.exists(t) or shutil.which(os.path.basename(t)) for t in TOOLS),
                    reason="ROCm LLVM tools absent")
@pytest.mark.parametrize("tc", [0, 1], ids=["blocked", "task_order"])
def test_counted_waits_cover_the_dma(disassembly, tc):
    bodies = _kernel_bodies(disassembly, SYMBOL.format(tc))
    assert len(bodies) == 1, "expected one k_precond_xt_f64_2d<4096, 512, 0, 1, {}, 1> in libpdhg.so: {}".format(
        tc, list(bodies))
    body = next(iter(bodies.values()))
    dmas = [i for i, ln in enumerate(body) if "global_load_lds_dwordx4" in ln]
    assert len(dmas) >= 8, "8 DMA instructions per staged row expected, found {}".format(len(dmas))
    counted = []
    for i, ln in enumerate(body):
        m = re.search(r"s_waitcnt\s+vmcnt\((\d+)\)", ln)
        if not m or int(m.group(1)) == 0 or i < dmas[0]:
            continue
        need, after = int(m.group(1)), 0   # vector-memory ops between the nearest preceding DMA and this wait
        for prev in reversed(body[:i]):
            if "global_load_lds" in prev:
                break
            if VMEM.match(prev.split("//")[0]):
                after += 1
        assert after >= need, ("vmcnt({}) with only {} vector-memory ops after the last DMA: the staged row could "
                               "be read before it lands ({})".format(need, after, ln.strip()))
        counted.append(need)
    # the schedule this test pins: the forward loop's vmcnt(8) behind its 8 row stores
    assert 8 in counted, "no vmcnt(8) after the DMA left in the kernel (schedule changed: re-check it): {}".format(counted)
