"""Register budget of the headline kernel (nplda_fwd_v6_kernel, both layer-2 forms, fp32 and bf16 rows): one 512-thread
block per CU is two waves per SIMD, so at most 256 registers — and NO scratch: the split form holds all ten output blocks of
layer 2 beside the accumulators of layer 1, and a spill there is paid on every tile.  hipcc cross-compiles for gfx950 without
a GPU, so this runs in the CPU suite."""
from tests.test_kernel_resources_cpu import _resources


def test_register_budget_of_the_headline_kernel():
    res = _resources("nplda_forward.hip")
    v6 = {k: v for k, v in res.items() if "nplda_fwd_v6_kernel" in k}
    # <10, 6, 8, 2, 5, 3, XM, 0, 2, L2S> for XM in {0, 2} (fp32 / bf16 rows) and L2S in {0, 1} (fp32 / split layer 2)
    assert len(v6) == 4, sorted(v6)
    assert sum(k.endswith("ELi2ELi1EEEvNS_7FwdArgsEi") for k in v6) == 2, sorted(v6)
    for k, v in v6.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
