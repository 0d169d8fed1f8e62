"""Time one global bundle adjustment (first camera fixed, everything else free) through suo_optimize (one C call: since round 6 the phase kernels under the
device-resident schedule, driven from C) and through suo_slam_amd/ba_dist.py on one rank (the same kernels, Python between the launches):
python tools/bench_global_ba.py [n_cam] [n_obj]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suo_slam_amd import ba as BA  # noqa: E402
from tests.test_gpu_geometry import _multi_view_scene  # noqa: E402

n_cam = int(sys.argv[1]) if len(sys.argv) > 1 else 60
n_obj = int(sys.argv[2]) if len(sys.argv) > 2 else 8
P, _ = _multi_view_scene(np.random.default_rng(1), n_cam, n_obj)
args = [P[k] for k in ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")]
ts = []
for rep in range(4):
    a = [x.copy() for x in args]
    t0 = time.perf_counter()
    out = BA.optimize(*a)
    ts.append(time.perf_counter() - t0)
print(f"suo_optimize: {n_cam} cams x {n_obj} objs, "
      f"{len(P['edge_cam'])} edges: {1e3 * min(ts):.2f} ms, {1e6 * min(ts) / max(int(out[4][2]), 1):.1f} us per LM trial (rounds/its/trials/good = {[int(v) for v in out[4]]})")

# the multi-GPU phase kernels (csrc/lm_dist.hip) under the host schedule, one rank (no exchange)
from suo_slam_amd import ba_dist  # noqa: E402
ts = []
for rep in range(4):
    prob = BA.Problem(*[x.copy() for x in args])
    t0 = time.perf_counter()
    ba_dist.optimize_distributed(prob)
    ts.append(time.perf_counter() - t0)
print(f"ba_dist.py, one rank (Python-driven): {1e3 * min(ts):.2f} ms, {1e6 * min(ts) / max(int(prob.stats[2]), 1):.1f} us per LM trial (rounds/its/trials/good = {[int(v) for v in prob.stats]})")
