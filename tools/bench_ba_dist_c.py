"""What the C driver of the partitioned bundle adjustment buys: one process, one run, the 32 cameras x 16 objects graph of bench.py's `global_ba` leg.
  (a) ba_dist.optimize_distributed, one "nccl" rank, SUO_FORCE_COLLECTIVES=1   Python + torch.distributed between the launches, every collective issued
  (b) suo_optimize_dist, RCCL communicator of world 1                           the same launches and collectives, enqueued from C
  (c) suo_optimize                                                              one rank, no collective, control steps folded: the floor
  (d) suo_optimize_partitioned at 2 and 4 local ranks                           the N-rank schedule on one GPU: world x the launches on one stream -- SLOWER by construction
Medians over `--reps` alternating repetitions after warm-up; host clock around calls that end in a device synchronise (each call returns the result to the host).
Per-solve time follows the LM trial count, which differs between the routes' summation orders: compare per LM trial.  Boxes differ by 2-3 %: compare within one run.
    python tools/bench_ba_dist_c.py [--reps 30] [--out profiles/ba_dist_c.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from suo_slam_amd import _lib, ba, ba_dist  # noqa: E402
from suo_slam_amd import synthetic as S  # noqa: E402

KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--port", type=int, default=29733)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit("--reps: at least 30 repetitions")
    _lib.require_gpu()
    torch.cuda.set_device(0)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=0, world_size=1)
    P = S.make_pose_graph(np.random.default_rng(5), 32, 16)
    comm = ba_dist.group_comm()
    local = {w: ba_dist.LocalRanks(w) for w in (2, 4)}

    def fresh():
        return ba.Problem(*[P[k].copy() for k in KEYS])

    def py_forced():
        os.environ["SUO_FORCE_COLLECTIVES"] = "1"
        try:
            return ba_dist.optimize_distributed(fresh())
        finally:
            os.environ["SUO_FORCE_COLLECTIVES"] = "0"

    def floor():
        q = fresh()
        ba.optimize_batch([q])
        return q
    routes = [("a", "optimize_distributed, one nccl rank, collectives forced (Python-driven)", py_forced),
              ("b", "suo_optimize_dist, RCCL world 1 (C-driven)", lambda: ba_dist.optimize_distributed_c(fresh(), comm)),
              ("c", "suo_optimize (one rank, no collectives: the floor)", floor),
              ("d2", "suo_optimize_partitioned, 2 local ranks", lambda: ba_dist.optimize_distributed_c(fresh(), local[2])),
              ("d4", "suo_optimize_partitioned, 4 local ranks", lambda: ba_dist.optimize_distributed_c(fresh(), local[4]))]
    times = {k: [] for k, _, _ in routes}
    stats = {}
    for rep in range(a.warmup + a.reps):
        for key, _, fn in routes:                           # alternating: every route sees the same drift of the box
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q = fn()
            dt = time.perf_counter() - t0
            stats[key] = [int(v) for v in q.stats]
            if rep >= a.warmup:
                times[key].append(dt)
    lines = [f"tools/bench_ba_dist_c.py: {len(P['cam_T'])} cameras x {len(P['obj_T'])} objects, {len(P['edge_cam'])} edges; medians of {a.reps} alternating repetitions after "
             f"{a.warmup} warm-up rounds, one process, device {torch.cuda.get_device_name(0)}",
             f"{'':4s}{'route':78s}{'ms':>9s}{'min ms':>9s}{'trials':>8s}{'us/trial':>10s}   rounds/its/trials/good"]
    per = {}
    for key, name, _ in routes:
        med, trials = statistics.median(times[key]), max(stats[key][2], 1)
        per[key] = 1e6 * med / trials
        lines.append(f"({key:2s}) {name:77s}{1e3 * med:9.3f}{1e3 * min(times[key]):9.3f}{trials:8d}{per[key]:10.1f}   {stats[key]}")
    gap = per["a"] - per["c"]
    lines.append(f"per LM trial: (a) {per['a']:.1f} us, (b) {per['b']:.1f} us, (c) {per['c']:.1f} us: the C driver closes {100 * (per['a'] - per['b']) / gap if gap > 0 else float('nan'):.0f} % "
                 f"of the gap between (a) and (c); (b) <= (a): {per['b'] <= per['a']}")
    lines.append(f"local ranks per LM trial: 2 ranks {per['d2'] / per['c']:.2f} x, 4 ranks {per['d4'] / per['c']:.2f} x the floor (expected above 1: world x the launches on one stream)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    torch.cuda.synchronize()
    for c in local.values():
        c.close()
    ba_dist.close_comms()
    dist.destroy_process_group()
    if not per["b"] <= per["a"]:
        raise SystemExit("the C-driven schedule is slower per LM trial than the Python-driven one: something is wrong")


if __name__ == "__main__":
    main()
