"""Compile-time contract of the one-pass form of the fused Winograd tail (csrc/conv_wino_x3_one_pass.hip): exactly the one kernel its launcher uses (the tail
with the next block's conv1), and for every kernel in the object no spill and no scratch, two waves per SIMD, and two workgroups' LDS inside a CU."""
from tests.test_kernel_resources import _usage


def test_one_pass_form_does_not_spill_and_fits_two_per_cu(tmp_path):
    k = _usage("conv_wino_x3_one_pass.hip", tmp_path)
    assert list(k) == ["_ZN3suo26wino3x3_x3_one_pass_kernelILb1ELb0ELb1ELi4ELi2ELb1ELb0ELb0ELb1EEEvNS_8ConvArgsE"], list(k)      # <FUSE, UP = false, TX3, 4, 2, NEXT, SKD = false, W8 = false, DMA>
    for name, v in k.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
        assert v["Occupancy"] >= 2, (name, v)
        assert 2 * v["LDS Size"] <= 160 * 1024, (name, v)
        assert v["LDS Size"] == 2 * 8 * (128 * 32 + 32) + 4 * 16 * 36 * 4, (name, v)        # the operand planes of the whole tile and four half patches: 75 264 B
