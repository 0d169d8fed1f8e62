"""Child process of tests/test_gpu_fp16_fallback.py::test_per_call_validity_with_and_without_graph_replay: two network calls in flight on one stream, one of
them out of fp16's range, with graph replay on or off (argv[1]); prints one JSON line: what each call's own query said, the pipe in between, and digests of
the in-range call's outputs and of the same call alone on a fresh f16x2 network."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tests.fp16_recipes import BRIGHT_DIM_GAIN_LOG2, dim, frame_and_boxes, recipe_bright_dim  # noqa: E402
from suo_slam_amd.pkpnet import PkpNet  # noqa: E402

graph = bool(int(sys.argv[1]))
sd = recipe_bright_dim(2.0 ** BRIGHT_DIM_GAIN_LOG2)
img, boxes = frame_and_boxes()


def digest(out):
    h = hashlib.sha256()
    for k in ("uv", "cov", "kp_mask", "kp_mask_logits", "prob_logits"):
        h.update(np.ascontiguousarray(out[k].cpu().numpy()).tobytes())
    return h.hexdigest()


def net():
    n = PkpNet(state_dict=sd, max_crops=len(boxes))
    n.set_graph(graph)
    return n


res = {}
torch.cuda.set_stream(torch.cuda.Stream())        # (the legacy default stream takes the blocking C entries, which re-issue by themselves)
alone = net()
res["alone"] = digest(alone(dim(img), [torch.from_numpy(boxes)], None))
res["alone_pipe"] = alone.pipe()
for order in ("clean_first", "bright_first"):
    n = net()
    frames = [dim(img), img] if order == "clean_first" else [img, dim(img)]
    outs = [n(f, [torch.from_numpy(boxes)], None, check=False) for f in frames]
    torch.cuda.synchronize()
    clean = outs[0] if order == "clean_first" else outs[1]
    bright = outs[1] if order == "clean_first" else outs[0]
    r = {"calls": [o.call for o in outs]}
    if order == "clean_first":
        r["clean_invalid"] = n.call_range_exceeded(clean.call)
        r["pipe_between"] = n.pipe()
        r["bright_invalid"] = n.call_range_exceeded(bright.call)
    else:
        r["bright_invalid"] = n.call_range_exceeded(bright.call)
        r["pipe_between"] = n.pipe()
        r["clean_invalid"] = n.call_range_exceeded(clean.call)
    r["pipe_end"] = n.pipe()
    r["clean"] = digest(clean)
    res[order] = r
print("RESULT " + json.dumps(res))
