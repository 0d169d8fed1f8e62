"""The launch schedule of the keypoint CNN is pinned: suo_net_schedule_bytes (a dry run of csrc/net.hip's schedule, nothing runs) per crop count, with and
without priors, on every matrix pipe, against the table recorded in tests/golden/net_schedule.json.  Every term of the sums is an integer-valued double far
below 2^53, so the comparison is for equality.  A schedule change -- another route for some Residual block (Net::plan_block), another form, one launch more or
less -- moves at least one of the seven numbers of some entry: it is then a deliberate edit of that file.

The crop counts straddle the dispatch thresholds at the network's map sizes (128x128 for r1, 64x64 down to 4x4).  Which count reaches which route (product
build; per crop a 64x64 map has 32 tiles T of 8 x 16 pixels, a 32x32 map 8 and 32 tiles t of 4 x 8 pixels, 16x16 T = 2 / t = 8, 8x8 t = 2, 4x4 t = 1):
  one launch, fp32 kernel      maps of 16 and 32 pixels a side with t < 33 on the fp16 pipe (1 crop at 32x32, 1 ... 4 at 16x16), t < 129 on the others (1 ... 4 crops at
                               32x32; 1 ... 16 at 16x16)
  one launch, fp16 kernel      33 <= t <= 768 on the fp16 pipe (2 ... 24 crops at 32x32, 5 ... 96 at 16x16, 17 ... 384 at 8x8, 33 ... 768 at 4x4)
  one launch, bf16x3 kernel    129 <= t <= 768 on the bf16x3 pipe (5 ... 24 crops at 32x32, 17 ... 96 at 16x16, 65 ... 384 at 8x8, 129 ... 768 at 4x4)
  Winograd + fused tail        256 -> 256 blocks no one-launch kernel takes, T >= 32 on the fp16 pipe (64x64 from 1 crop, 32x32 from 25, 16x16 from 97) / >= 256 on the
                               others (64x64 from 8 crops, 32x32 from 32, 16x16 from 128), on each pipe's form; with the up-sampled addend (the last up1 block) and, on the
                               fp16 pipe beyond the eight-wave form's 256 tiles (64x64 from 9 crops, 32x32 from 33, 16x16 from 129), the next block's conv1
  per layer, Winograd conv2    r1 / r4 / r5 (no 256 <- 128 conv3 without conv4: no fused tail) from the same tile counts (fp16 pipe: every count; the others: r1 from 2
                               crops, r4 / r5 from 8)
  per layer, direct conv2      everything else: 8x8 and 4x4 maps below the one-launch counts, 64x64 at 1 ... 7 crops and r1 at 1 crop on the bf16x3 / fp32 pipes,
                               and there the maps between the one-launch and the fused-tail ranges (bf16x3: 32x32 at 25 ... 31 crops, 16x16 at 97 ... 127; fp32:
                               32x32 at 5 ... 31, 16x16 at 17 ... 127)
(The ranges are those the scan of tests/net_boundary_cases.py finds over every crop count up to 130; the CROPS below sample them, and
tests/test_gpu_net_boundaries.py RUNS the network on both sides of each change.)
The direct 3x3 with fused tail needs 1024 tiles of 128 pixels on a map the Winograd kernel does not take; no shape of this network has that in the product
build (tuning builds reach it with SUO_CONV_WINO=0)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

CROPS = (1, 2, 5, 7, 8, 9, 16, 33, 34, 64, 128, 256)
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_schedule.json")


def schedule_table(state_dict, setenv, delenv):
    """[{pipe, crops, with_priors, bytes: [per kind, PkpNet.SCHEDULE_KINDS order], launches}, ...]: pipes 2 and 1 of a default network, pipe 0 of one built with
    SUO_WINO_BF16X3=0 (read when the network is built)."""
    from suo_slam_amd.pkpnet import PkpNet
    rows = []
    for fp32_build in (False, True):
        if fp32_build:
            setenv("SUO_WINO_BF16X3", "0")
        else:
            delenv("SUO_WINO_BF16X3")
        delenv("SUO_F16X2")
        net = PkpNet(state_dict=state_dict, max_crops=max(CROPS))
        for pipe in ((0,) if fp32_build else (2, 1)):
            net.set_pipe(pipe)
            assert net.pipe() == pipe
            for L in CROPS:
                for wp in (False, True):
                    b = net.schedule_bytes(L, with_priors=wp)
                    by = [b[k] for k in PkpNet.SCHEDULE_KINDS]
                    assert all(v == int(v) and 0 <= v < 2.0 ** 53 for v in by)
                    rows.append({"pipe": pipe, "crops": L, "with_priors": wp, "bytes": [int(v) for v in by], "launches": b["launches"]})
        del net
    return rows


def test_the_launch_schedule_is_the_recorded_one(state_dict, monkeypatch):
    with open(TABLE) as f:
        want = json.load(f)
    got = schedule_table(state_dict, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert len(want) == 3 * len(CROPS) * 2 and len(got) == len(want)
    wrong = [(w, g) for w, g in zip(want, got) if w != g]
    assert not wrong, "%d of %d schedule entries differ; the first (recorded, now): %r" % (len(wrong), len(want), wrong[0])
