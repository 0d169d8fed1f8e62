"""Ways to push the network out of the fp16 form's range (include/suo_hip.h: SUO_PIPE_F16X2), all from the seeded random weights, and the host-side measure of
how far a frame takes them: shared by tests/test_fp16_recipes.py (the calibration, on the host) and tests/test_gpu_fp16_fallback.py (the fallback on every route).
`python -m tests.fp16_recipes {synthetic|bop_tree} DIR` prints the calibration of (c) as one JSON line (tests/test_fp16_recipes.py runs it as a child process).

  (a) recipe_stem:        conv1_ times 3e4 -- every call leaves the range
  (b) recipe_priors:      the prior channels of conv1_ times 2^16 -- a pass with rendered priors leaves it, a pass without (all-zero priors) cannot
  (c) recipe_bright_dim:  the image channels of conv1_ times 2^BRIGHT_DIM_GAIN_LOG2 -- normal frames leave it, the same frames divided by 16 do not
"""
import contextlib
import json
import sys
from unittest import mock

import numpy as np

# (c): frames 16x apart in brightness are ~16.5x apart in every activation (the network is close to linear in the stem's gain at this scale), so a power-of-two
# gain can put the limit at best ~4x from both: 2^13 puts the dim frames 3x below it and the normal ones 5x above (tests/test_fp16_recipes.py holds >= 2.5)
BRIGHT_DIM_GAIN_LOG2 = 13
PRIOR_GAIN = np.float32(2.0 ** 16)
LIMIT_1X1, LIMIT_3X3 = 4094.0, 1023.5          # csrc/f16x2.h: S2_LIMIT / S2_XSCALE, and a quarter of it for the Winograd 3x3 operands


def base_state_dict():
    from suo_slam_amd import weights
    return weights.make_random_state_dict(seed=0, logit_gain=8.0)


def confident(sd):
    """tests/test_gpu_slam_chain.py::_confident: the validity head says yes, so network keypoints pass the masks."""
    sd = dict(sd)
    sd["classifier.2.bias"] = (np.asarray(sd["classifier.2.bias"]) + 4.0).astype(np.float32)
    return sd


def recipe_stem(sd=None):
    sd = dict(sd if sd is not None else base_state_dict())
    sd["backbone.conv1_.weight"] = sd["backbone.conv1_.weight"] * np.float32(3e4)
    return sd


def recipe_priors(sd=None):
    sd = dict(sd if sd is not None else base_state_dict())
    w = np.array(sd["backbone.conv1_.weight"], np.float32)
    w[:, 3:] *= PRIOR_GAIN
    sd["backbone.conv1_.weight"] = w
    return sd


def recipe_bright_dim(gain=2.0 ** BRIGHT_DIM_GAIN_LOG2, sd=None):
    sd = dict(sd if sd is not None else base_state_dict())
    w = np.array(sd["backbone.conv1_.weight"], np.float32)
    w[:, :3] *= np.float32(gain)
    sd["backbone.conv1_.weight"] = w
    return sd


def dim(img):
    """The same frame, 16x darker (uint8)."""
    return np.asarray(img) // 16


def frame_and_boxes():
    """One synthetic 480x640 frame and two boxes on it (the network-level tests)."""
    from suo_slam_amd import synthetic as S
    fr = S.make_frame(np.random.default_rng(2), 2, with_image=True)
    return np.ascontiguousarray(fr["image"]), np.ascontiguousarray(fr["boxes"], dtype=np.float32)


def guard_ratio(img, boxes, sd):
    """The largest |operand| / limit over every 1x1 (4094) and 3x3 (1023.5) convolution of the network on these crops, on the host (oracle/cnn_oracle.py, no
    priors): >= 1 means the fp16 form cannot compute the call.  (Not just the first 1x1 after the stem: on these weights the 3x3 operands of the second stack's
    Residual blocks reach ~5x its ratio, and they run on the fp16 form at every crop count.)"""
    import torch
    from oracle import cnn_oracle as O
    rec = [0.0]
    conv = O._conv

    def recording(x, P, p, stride=1, padding=0):
        k = P[p + ".weight"].shape[-1]
        if k in (1, 3):
            rec[0] = max(rec[0], float(x.abs().max()) / (LIMIT_1X1 if k == 1 else LIMIT_3X3))
        return conv(x, P, p, stride, padding)
    with mock.patch.object(O, "_conv", recording), torch.no_grad():
        O.pkpnet_forward(np.asarray(img), np.asarray(boxes, np.float32), None, sd)
    return rec[0]


@contextlib.contextmanager
def late_reader():
    """Every validity query of a PkpNet first waits for EVERYTHING enqueued on the device: the check then runs when every later call has already finished --
    the worst case of a reader racing the calls behind the one it asks about, without timing luck."""
    import torch
    from suo_slam_amd.pkpnet import PkpNet
    patches = []
    for name in ("range_exceeded", "call_range_exceeded"):
        orig = getattr(PkpNet, name, None)
        if orig is None:
            continue

        def wrapped(self, *a, _orig=orig, **k):
            torch.cuda.synchronize()
            return _orig(self, *a, **k)
        patches.append(mock.patch.object(PkpNet, name, wrapped))
    with contextlib.ExitStack() as st:
        for p in patches:
            st.enter_context(p)
        yield


def bop_views(root):
    """The first two views of a one-scene YCB-V tree (tests/bop_tree.py) with their ground-truth boxes."""
    from suo_slam_amd import bop
    from tests import bop_tree
    desc = bop_tree.build(root, dset="ycbv", seed=41, n_scenes=1, n_views=6)
    ds = bop.BopDataset(desc["data_root"], desc["split"], bop_dset="ycbv", ignore_symmetry=True)
    out = []
    for s in ds.scene_ids():
        for v in ds.view_ids(s)[:2]:
            sample = ds.get_raw(s, v, ds.obj_ids(s, v))
            out.append(((255 * sample["img"].numpy().transpose((1, 2, 0))).astype(np.uint8), sample["bboxes"].numpy().astype(np.float32)))
    return out


def calibration(frames, root):
    """(c) on these frames: guard_ratio of every normal frame and of the same frame / 16, and of the first frame on the unscaled weights."""
    sd = recipe_bright_dim()
    cases = [frame_and_boxes()] if frames == "synthetic" else bop_views(root)
    img, boxes = cases[0]
    return {"cases": [(guard_ratio(i, b, sd), guard_ratio(dim(i), b, sd)) for i, b in cases], "unscaled": guard_ratio(img, boxes, base_state_dict())}


if __name__ == "__main__":
    print("CALIBRATION " + json.dumps(calibration(sys.argv[1], sys.argv[2])))
