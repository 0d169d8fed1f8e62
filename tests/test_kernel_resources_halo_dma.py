"""Compile-time contract of the LDS-DMA forms of the four-wave fp16 Winograd kernels (csrc/conv_wino_x3_dma.hip = csrc/conv_wino_x3.hip compiled for
wino3x3_x3_kernel<..., DMA = true> alone): the five instantiations the launchers use and no other, no spill and no scratch anywhere, two waves per SIMD,
two workgroups' LDS inside a CU -- what tests/test_kernel_resources.py holds the register-staged forms to."""
from tests.test_kernel_resources import _usage


def test_dma_forms_do_not_spill(tmp_path):
    k = _usage("conv_wino_x3_dma.hip", tmp_path)
    assert len(k) == 5 and all("wino3x3_x3_kernel" in n and n.endswith("Lb0ELb1EEEvNS_8ConvArgsE") for n in k), list(k)      # <..., W8 = false, DMA = true>
    assert sum("wino3x3_x3_kernelILb1E" in n for n in k) == 3                       # the fused tails: plain, with the up-sampled addend, with the next block's conv1
    for name, v in k.items():
        # (nothing in memory.  Scalar registers parked in VGPR lanes are not: the form with the next block's conv1 parks three, in both staging paths)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
        assert v["Occupancy"] >= 2, (name, v)
        assert 2 * v["LDS Size"] <= 160 * 1024, (name, v)
