"""Times suo_pose_covariances_graph's device-memory form (csrc/pose_cov_graph.hip) in one run on one GPU.  Medians of 30 repetitions, host wall clock around the
blocking C calls (staging and read-back included), at the state suo_optimize leaves.

  Table 1  the one-workgroup LDS form against the grid-spread form on the SAME graph: suo_pose_covariances_pairs with one (camera, object) pair, and
           suo_pose_covariances_graph forced onto the new form by one (camera, camera) pair, on 32 x 16 and 60 x 8.
  Table 2  the new form alone, with all consecutive (camera, camera) pairs, on 32 x 17, 32 x 33 and 60 x 20, beside the whole suo_optimize call and one of its LM
           trials (the call divided by the trials its `stats` report), as tools/bench_pose_cov.py does.

Writes nothing: redirect into profiles/pose_cov_graph.txt.

    python tools/bench_pose_cov_graph.py [--reps 30]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suo_slam_amd import ba  # noqa: E402
from suo_slam_amd import synthetic as S  # noqa: E402

KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")


def _median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def _optimized(g, reps):
    """(the problem at the refined state, median ms of suo_optimize, median trials)"""
    args = [g[k] for k in KEYS]
    trials = []

    def opt():
        p = ba.Problem(*args)
        ba.optimize_batch([p])
        trials.append(int(p.stats[2]))
        return p
    t_opt = _median_ms(opt, reps)
    return opt(), t_opt, max(int(np.median(trials)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    print(f"{'graph':10s} {'edges':>6s} {'pairs entry (LDS form) ms':>26s} {'graph entry (device-memory form) ms':>36s} {'new / old':>10s}")
    for C, O in ((32, 16), (60, 8)):
        g = S.make_pose_graph(rng, C, O)
        p, _, _ = _optimized(g, 3)
        t_old = _median_ms(lambda: ba.pose_covariances_pairs_batch([p], [np.array([(1, C)], np.int32)]), a.reps)
        t_new = _median_ms(lambda: ba.pose_covariances_graph_batch([p], [np.array([(0, 1)], np.int32)]), a.reps)
        print(f"{f'{C} x {O}':10s} {len(g['edge_cam']):6d} {t_old:26.3f} {t_new:36.3f} {t_new / t_old:10.2f}")
    print()
    print(f"{'graph':10s} {'edges':>6s} {'optimize ms':>12s} {'trials':>7s} {'LM trial us':>12s} {'camera pairs':>13s} {'graph entry ms':>15s} {'= LM trials':>12s}")
    for C, O in ((32, 17), (32, 33), (60, 20)):
        g = S.make_pose_graph(rng, C, O)
        p, t_opt, n_tr = _optimized(g, a.reps)
        pairs = np.array([(c, c + 1) for c in range(C - 1)], np.int32)
        t_new = _median_ms(lambda: ba.pose_covariances_graph_batch([p], [pairs]), a.reps)
        us = 1e3 * t_opt / n_tr
        print(f"{f'{C} x {O}':10s} {len(g['edge_cam']):6d} {t_opt:12.3f} {n_tr:7d} {us:12.1f} {len(pairs):13d} {t_new:15.3f} {1e3 * t_new / us:12.1f}")


if __name__ == "__main__":
    main()
