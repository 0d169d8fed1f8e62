"""The whole keypoint CNN RUN at every crop count where its launch schedule changes (tests/net_boundary_cases.py: CROPS, found by scanning the dry run), on each
matrix pipe and through both staging layouts.  tests/test_gpu_net_schedule.py pins WHICH launches a call makes; every kernel is tested alone at ragged shapes; here
their composition is held to the reference and to the oracle on both sides of each threshold -- a conv1 computed by the producer that the consumer's plan does not pick
up, an up-sampled addend handed to a route that cannot add it, a pooled tensor only one side of a threshold writes, workspace addresses in the graph captured for that
count, GEMM and tile tails at the odd row counts these L give (17 crops at 4x4 = 272 rows).

  check 1  CROPS covers every count the scan reports, with and without priors, and holds nothing else but the documented counts the scan cannot see
  check 2  with-priors layout (44-channel stem inside the captured graph, suo_net_backbone): the crops of tests/golden/cnn_inputs.py cycled to L, every copy
           within 1e-5 of its crop's range of the REFERENCE's logits (tests/golden/cnn_golden_wide.npz), copies of one crop bit-identical
           (at an odd L the last tile of a launch is partial), replay of the captured graph == direct launches, bit for bit
  check 3  prior-less layout (forward_frames: RoIAlign + stem ahead of the graph, on the fp16 form with r1's conv1; roi_align_concat + the 3-channel stem on the fp32
           build): eight boxes on one frame cycled to L against oracle/cnn_oracle.py: logits 1e-5 of the range, uv / cov / kp_mask 1e-5 absolute, copies bit-identical

One network per pipe for the module, sized for the scan (130 crops; the largest count run is 129).  Worst error over all L observed on an MI355X (relative to the
crop's range; printed when the module ends):
             vs the reference (check 2)   vs the oracle (check 3)
  f16x2      1.062e-06                    1.016e-06
  bf16x3     1.150e-06                    1.179e-06
  f32        1.150e-06                    1.183e-06
No case failed: no schedule bug was found at these counts."""
import os

import numpy as np
import pytest
import torch

from tests import net_boundary_cases as B
from tests.golden import cnn_inputs as I

pytestmark = pytest.mark.gpu
PIPE_NAMES = ("f16x2", "bf16x3", "f32")
CASES = [(p, L) for p in PIPE_NAMES for L in B.CROPS[p]]
WORST = {}


@pytest.fixture(scope="module")
def nets(state_dict):
    """name -> the module's network on that pipe, built on first use the way tests/test_gpu_golden_wide.py::_net builds it (the switches are read at creation)."""
    from suo_slam_amd import _lib
    from suo_slam_amd.pkpnet import PkpNet
    _lib.require_gpu()
    made = {}

    def get(pipe):
        if pipe not in made:
            with pytest.MonkeyPatch().context() as mp:
                mp.delenv("SUO_WINO_BF16X3", raising=False)
                mp.delenv("SUO_F16X2", raising=False)
                if pipe == "bf16x3":
                    mp.setenv("SUO_F16X2", "0")
                if pipe == "f32":
                    mp.setenv("SUO_WINO_BF16X3", "0")
                made[pipe] = PkpNet(state_dict=state_dict, max_crops=max(B.SCAN_L_MAX, max(B.CROPS[pipe])))
            assert made[pipe].pipe() == B.PIPES[pipe]
        net = made[pipe]
        net.range_exceeded()                                        # (a case that left the fp16 range has failed; the next one starts on its own pipe, flag down)
        net.set_pipe(B.PIPES[pipe])
        net.set_graph(True)
        return net

    yield get
    for net in made.values():
        net.close()
    for (what, pipe), v in sorted(WORST.items()):
        print("worst relative error over all crop counts, %s, %s: %.3e" % (what, pipe, v))


@pytest.fixture(scope="module")
def staged_ref():
    """(device [5,256,256,48] staged crops, device [5,41,64,64] reference logits, device [5] their ranges), CROP_KINDS order; computed once, never written."""
    from tests.conftest import GOLDEN
    ref = torch.from_numpy(np.load(os.path.join(GOLDEN, "cnn_golden_wide.npz"))["logits"]).cuda()
    assert tuple(ref.shape) == (len(I.CROP_KINDS), 41, 64, 64)
    return torch.from_numpy(I.staged(I.CROP_KINDS)).cuda(), ref, ref.abs().amax(dim=(1, 2, 3))


@pytest.fixture(scope="module")
def frame_oracle(state_dict):
    """(uint8 frame, float32 boxes [8,4], the oracle's outputs on them as device tensors), computed once on the CPU."""
    from oracle import cnn_oracle as O
    img = (np.random.default_rng(B.FRAME_SEED).uniform(0, 1, (480, 640, 3)) * 255).astype(np.uint8)
    boxes = np.array(B.BOXES, np.float32)
    ref = O.pkpnet_forward(img, boxes, None, state_dict)
    return img, boxes, {k: ref[k].cuda() for k in ("prob_logits", "uv", "cov", "kp_mask")}


def _first_copy(sel):
    """i -> the first position in the call that holds the same input as position i."""
    return torch.as_tensor([sel.index(s) for s in sel], dtype=torch.long, device="cuda")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rel_err(got, ref, ranges, sel_t):
    """Per position of the call: max |got - its reference| / that reference's range, on the device."""
    return (got - ref.index_select(0, sel_t)).abs().amax(dim=(1, 2, 3)) / ranges.index_select(0, sel_t)


def _hold(err, what, pipe, L, tol=1e-5):
    err = err.cpu()
    worst, at = float(err.max()), int(err.argmax())
    print("%s %s L=%d: worst relative error %.3e (copy %d)" % (what, pipe, L, worst, at))
    assert bool(torch.isfinite(err).all()), (pipe, L, "non-finite", [i for i in range(L) if not np.isfinite(float(err[i]))][:8])
    WORST[(what, pipe)] = max(WORST.get((what, pipe), 0.0), worst)
    assert worst < tol, (pipe, L, at, worst)


@pytest.mark.parametrize("with_priors", [False, True])
@pytest.mark.parametrize("pipe", PIPE_NAMES)
def test_crop_lists_cover_every_schedule_change(nets, pipe, with_priors):
    """CROPS was not guessed: every count the scan reports is run, and what is run beyond the scan's counts is the documented remainder."""
    found = set(B.schedule_breaks(nets(pipe), B.PIPES[pipe], with_priors))
    print(pipe, with_priors, sorted(found))
    if pipe == "f16x2":
        assert {8, 9} <= found and {16, 17} <= found, sorted(found)         # 64x64 tails carry the next conv1 from 9 crops; 8x8 blocks in one launch from 17
    if pipe == "bf16x3":
        assert {7, 8} <= found, sorted(found)                               # 64x64 on Winograd + fused tail from 8 crops
    assert B.DOCUMENTED[pipe] <= found, (pipe, sorted(B.DOCUMENTED[pipe] - found))
    assert found <= set(B.CROPS[pipe]), (pipe, "schedule changes no test runs: add to CROPS", sorted(found - set(B.CROPS[pipe])))
    assert set(B.CROPS[pipe]) - found == B.UNSEEN[pipe], (pipe, sorted(set(B.CROPS[pipe]) - found))


@pytest.mark.parametrize("pipe,L", CASES)
def test_staged_backbone_against_the_reference(nets, staged_ref, pipe, L):
    """Check 2 (module docstring): every copy to the reference, copies to each other, graph replay to direct launches."""
    from tests.gpu_backbone import run_backbone_from_device_crops
    net = nets(pipe)
    base, ref, ranges = staged_ref
    # the fp16 form's own results: without the heavy-tailed crop its range flag stays down (tests/test_gpu_golden_wide.py); the other forms take all five
    kinds = [k for k in range(len(I.CROP_KINDS)) if pipe != "f16x2" or I.CROP_KINDS[k] != "heavy_tailed"]
    sel = [kinds[i % len(kinds)] for i in range(L)]
    sel_t = torch.as_tensor(sel, dtype=torch.long, device="cuda")
    out = run_backbone_from_device_crops(net, base, sel)
    assert not net.range_exceeded() and net.pipe() == B.PIPES[pipe], (pipe, L, "left the fp16 range")
    _hold(_rel_err(out, ref, ranges, sel_t), "reference", pipe, L)
    assert _same_bits(out, out.index_select(0, _first_copy(sel))), (pipe, L, "copies of one crop differ within the call")
    try:
        net.set_graph(False)
        direct = run_backbone_from_device_crops(net, base, sel)
    finally:
        net.set_graph(True)
    assert not net.range_exceeded() and net.pipe() == B.PIPES[pipe]
    assert _same_bits(direct, out), (pipe, L, "graph replay and direct launches differ")


@pytest.mark.parametrize("pipe,L", CASES)
def test_prior_less_frames_route_against_the_oracle(nets, frame_oracle, pipe, L):
    """Check 3 (module docstring): one forward_frames call of L crops, every copy to the oracle's outputs for its box, copies to each other."""
    net = nets(pipe)
    img, boxes, ref = frame_oracle
    sel = [i % len(boxes) for i in range(L)]
    sel_t = torch.as_tensor(sel, dtype=torch.long, device="cuda")
    out = net.forward_frames(img[None], [boxes[sel]])
    torch.cuda.synchronize()
    assert not net.range_exceeded() and net.pipe() == B.PIPES[pipe], (pipe, L, "left the fp16 range")
    lr = ref["prob_logits"]
    _hold(_rel_err(out["prob_logits"], lr, lr.abs().amax(dim=(1, 2, 3)), sel_t), "oracle", pipe, L)
    for key in ("uv", "cov", "kp_mask"):
        d = (out[key] - ref[key].index_select(0, sel_t)).abs().reshape(L, -1).amax(dim=1).cpu()
        assert float(d.max()) < 1e-5, (pipe, L, key, int(d.argmax()), float(d.max()))
    first = _first_copy(sel)
    for key in ("prob_logits", "uv", "cov", "kp_mask"):
        assert _same_bits(out[key], out[key].index_select(0, first)), (pipe, L, key, "copies of one box differ within the call")
