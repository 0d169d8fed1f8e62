"""Compile-time contract of the skip-rows-by-LDS-DMA form of the fused Winograd tail (csrc/conv_wino_x3_skip_dma.hip): the one instantiation its launcher
uses, no spill and no scratch, two waves per SIMD, two workgroups' LDS inside a CU (at most 80 KiB each), and no more registers than the register-load form
of the same tail in csrc/conv_wino_x3_dma.hip."""
from tests.test_kernel_resources import _usage


def test_skip_dma_form_does_not_spill_and_stays_inside_its_parent(tmp_path):
    k = _usage("conv_wino_x3_skip_dma.hip", tmp_path)
    assert list(k) == ["_ZN3suo17wino3x3_x3_kernelILb1ELb1ELb1ELi4ELi2ELb0ELb1ELb0ELb1EEEvNS_8ConvArgsE"], list(k)      # <FUSE, UP, TX3, 4, 2, NEXT = false, SKD, W8 = false, DMA>
    v = next(iter(k.values()))
    assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, v
    assert v["Occupancy"] >= 2 and v["LDS Size"] <= 80 * 1024, v
    parent = _usage("conv_wino_x3_dma.hip", tmp_path)["_ZN3suo17wino3x3_x3_kernelILb1ELb1ELb1ELi4ELi2ELb0ELb0ELb0ELb1EEEvNS_8ConvArgsE"]
    assert v["VGPRs"] <= parent["VGPRs"], (v, parent)
