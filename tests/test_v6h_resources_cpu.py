"""Register budget of the hybrid-layer-1 headline kernel (nplda_fwd_v6h_kernel): one 512-thread block per CU is two waves per
SIMD, so at most 256 registers, and no scratch — it holds v6's split layer 2 (all ten output blocks beside the accumulators of
layer 1) plus the bf16 pieces of x and of the split blocks' weights in layer 1.  The set of instances is exactly what the
dispatch can launch: S1 in {2, 3, 4} (NPLDA_FWD_V6_L1S) x fp32 / bf16 rows.  nplda_fwd_v6_kernel keeps its four.  hipcc
cross-compiles for gfx950 without a GPU, so this runs in the CPU suite."""
import re

from tests.test_kernel_resources_cpu import _resources


def test_register_budget_of_the_hybrid_kernel():
    res = _resources("nplda_forward.hip")
    v6h = {k: v for k, v in res.items() if "nplda_fwd_v6h_kernel" in k}
    # <NB = 10, WAVES = 8, S1, G1, XM>(FwdArgs, int)
    inst = set()
    for k in v6h:
        m = re.search(r"nplda_fwd_v6h_kernelILi10ELi8ELi(\d+)ELi(\d+)ELi(\d+)EEEvNS_7FwdArgsEi$", k)
        assert m, k
        inst.add((int(m.group(1)), int(m.group(3))))
    assert inst == {(s1, xm) for s1 in (2, 3, 4) for xm in (0, 2)} and len(v6h) == 6, sorted(v6h)
    for k, v in v6h.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
    assert sum("nplda_fwd_v6_kernel" in k for k in res) == 4, sorted(k for k in res if "nplda_fwd_v6" in k)
