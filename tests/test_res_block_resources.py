"""Compile-time resources of the one-launch Residual block on split operands (csrc/res_small_x3.hip; hipcc cross-compiles without a GPU).  The fp16 form
(NP = 2) is built to hold two workgroups on a CU: twice its LDS within the CU's 160 KB, registers for two waves per SIMD, nothing in scratch.  The
bf16x3 form (NP = 3) keeps one workgroup per CU, whose LDS must fit."""
from tests.test_kernel_resources import _usage


def test_res_block_fp16_form_fits_two_workgroups_per_cu(tmp_path):
    k = {n: v for n, v in _usage("res_small_x3.hip", tmp_path).items() if "res_block_x3_kernel" in n}
    two, three = {n: v for n, v in k.items() if "ELi2EE" in n}, {n: v for n, v in k.items() if "ELi3EE" in n}
    assert len(two) == 4 and len(three) == 4, list(k)          # <POOL_IN, UP> x NP
    for name, v in k.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
    for name, v in two.items():
        assert v["Occupancy"] >= 2 and 2 * v["LDS Size"] <= 160 * 1024, (name, v)
        assert v["LDS Size"] + 61568 <= 160 * 1024, (name, v)   # and one beside a Winograd workgroup (csrc/conv_wino_x3.hip: 61 568 B)
    for name, v in three.items():
        assert v["LDS Size"] <= 160 * 1024, (name, v)
