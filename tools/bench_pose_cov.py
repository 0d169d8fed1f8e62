"""Times suo_pose_covariances beside one LM trial of suo_optimize on the same graph: 1 x 8 (a single-view frame), 32 x 16 and 60 x 8 (global adjustments).
Medians of 30 repetitions, host wall clock around the blocking C calls (staging and read-back included on both sides); the LM trial is the whole suo_optimize
call divided by the trials its `stats` report.  Expectation: the coupled form costs about one linearisation + one Schur complement + 16 solves; more than
roughly ten LM trials would point at a serial column loop.  The last two columns time suo_pose_covariances_pairs with every (camera, object) pair of the graph
(C x O cross blocks and relative covariances) in the same run, and its ratio to suo_pose_covariances.  Writes nothing: redirect into profiles/pose_cov.txt.

    python tools/bench_pose_cov.py [--reps 30]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    fr = S.make_frame(rng, 8, noise=0.004, with_image=False)
    graphs = [("1 x 8 (frame)", S.frame_to_ba_problem(fr, fr["T_OtoC"])), ("32 x 16 (global)", S.make_pose_graph(rng, 32, 16)),
              ("60 x 8 (global)", S.make_pose_graph(rng, 60, 8))]
    print(f"{'graph':18s} {'edges':>6s} {'optimize ms':>12s} {'trials':>7s} {'LM trial us':>12s} {'covariances ms':>15s} {'= LM trials':>12s} {'pairs':>6s} {'with pairs ms':>14s} {'/ covariances':>14s}")
    for name, g in graphs:
        args = [g[k] for k in KEYS]
        trials = []

        def opt():
            p = ba.Problem(*args)
            ba.optimize_batch([p])
            trials.append(int(p.stats[2]))
            return p
        t_opt = _median_ms(opt, a.reps)
        p = opt()                                            # the state the covariances are taken at
        t_cov = _median_ms(lambda: ba.pose_covariances_batch([p]), a.reps)
        C, O = len(p.cam_T), len(p.obj_T)
        pairs = np.array([(c, C + o) for c in range(C) for o in range(O)], np.int32)
        t_pairs = _median_ms(lambda: ba.pose_covariances_pairs_batch([p], [pairs]), a.reps)
        n_tr = max(int(np.median(trials)), 1)
        us = 1e3 * t_opt / n_tr
        print(f"{name:18s} {len(g['edge_cam']):6d} {t_opt:12.3f} {n_tr:7d} {us:12.1f} {t_cov:15.3f} {1e3 * t_cov / us:12.1f} {len(pairs):6d} {t_pairs:14.3f} {t_pairs / t_cov:14.2f}")


if __name__ == "__main__":
    main()
