"""Child process of tests/test_gpu_ba_dist_c.py, shaped like tests/rccl_one_rank.py (same scenes): a one-rank "nccl" process group on the box's MI355X;
suo_slam_amd.ba_dist.optimize_distributed with SUO_FORCE_COLLECTIVES=1 (Python + torch.distributed between the launches) against
optimize_distributed_c -- suo_optimize_dist behind the C ABI with an RCCL communicator of world 1 made from that group: the same launches and the same
collectives, enqueued from C.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import ba as BA  # noqa: E402
from suo_slam_amd import ba_dist  # noqa: E402
from tests.test_gpu_geometry import _multi_view_scene  # noqa: E402

KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")


def main():
    n_cam, n_obj = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (12, 6)
    port = int(sys.argv[3]) if len(sys.argv) > 3 else 29578
    torch.cuda.set_device(0)
    P, _ = _multi_view_scene(np.random.default_rng(7), n_cam, n_obj)
    args = [P[k] for k in KEYS]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    os.environ["SUO_FORCE_COLLECTIVES"] = "1"
    py = ba_dist.optimize_distributed(BA.Problem(*[x.copy() for x in args]))
    comm = ba_dist.group_comm()                             # rank 0's unique id through dist.broadcast, suo_ba_comm_create_rccl on the current device
    before = comm.calls
    c = ba_dist.optimize_distributed_c(BA.Problem(*[x.copy() for x in args]))
    calls = comm.calls - before
    again = ba_dist.optimize_distributed_c(BA.Problem(*[x.copy() for x in args]))          # the cached communicator, the recycled contexts
    out = {
        "backend": dist.get_backend(), "rank": comm.rank, "world": comm.world, "calls": calls,
        "rounds": int(c.stats[0]), "iterations": int(c.stats[1]), "trials": int(c.stats[2]), "good": int(c.stats[3]), "py_stats": [int(v) for v in py.stats],
        "same_comm": ba_dist.group_comm() is comm,
    }
    for name, other in (("identical", py), ("repeatable", again)):
        out[name] = {k: bool(np.array_equal(getattr(c, k), getattr(other, k))) for k in ("cam_T", "obj_T", "inlier", "chi2", "stats")}
    torch.cuda.synchronize()
    ba_dist.close_comms()
    dist.destroy_process_group()
    print("RCCL_ONE_RANK_C " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
