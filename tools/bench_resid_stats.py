"""Times suo_residual_statistics (csrc/resid_stats.hip behind the pose-covariance kernels) in one run on one GPU, on the 60 x 8 and 32 x 16 synthetic graphs the
global-BA numbers use, at the state suo_optimize leaves.  Host wall clock around the blocking C calls (staging and read-back included):

  residual statistics   suo_residual_statistics, per call
  baseline              suo_pose_covariances_graph asked for the same (camera, object) pairs -- every pair that carries an edge -- on the same graph: the part of
                        the call that existed before

The two calls ALTERNATE inside one loop, so that whatever else the host and the GPU are doing falls on both; medians, with the 10th and 90th percentile as the
spread, and the ratio of the medians.  Which share of the added time is the edge kernel and which the reduction is not visible from the host: run the tool's
--loop mode (the entry alone, nothing timed) under a kernel trace, e.g.
    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_resid_stats.py --loop 50 --graph 60x8
and read rs_edge_kernel / rs_reduce_kernel from the kernel statistics.

Writes nothing: redirect into profiles/resid_stats.txt.

    python tools/bench_resid_stats.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suo_slam_amd import ba  # noqa: E402
from suo_slam_amd import synthetic as S  # noqa: E402

KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")
GRAPHS = {"60x8": (60, 8), "32x16": (32, 16)}


def _problem(rng, C, O):
    """(the problem at the refined state, its (camera, object) pairs that carry an edge as vertex codes)"""
    g = S.make_pose_graph(rng, C, O)
    p = ba.Problem(*[g[k] for k in KEYS])
    ba.optimize_batch([p])
    seen = sorted(set(zip(g["edge_cam"].tolist(), g["edge_obj"].tolist())))
    return p, np.array([(c, C + o) for c, o in seen], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loop", type=int, default=0, help="only call the entry this many times on --graph (for a kernel trace)")
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="60x8")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    if a.loop:
        p, _ = _problem(rng, *GRAPHS[a.graph])
        for _ in range(a.loop):
            ba.residual_statistics_batch([p])
        return
    print(f"{'graph':8s} {'edges':>6s} {'pairs':>6s} {'dof':>6s} {'s0^2':>7s} {'residual statistics ms (p10 .. p90)':>38s} {'baseline ms (p10 .. p90)':>30s} {'ratio':>6s} {'added ms':>9s}")
    for name, (C, O) in GRAPHS.items():
        p, pairs = _problem(rng, C, O)
        new = lambda: ba.residual_statistics_batch([p])
        old = lambda: ba.pose_covariances_graph_batch([p], [pairs])
        for _ in range(3):
            r = new()[0]
            old()
        t_new, t_old = [], []
        for _ in range(a.reps):
            for fn, t in ((new, t_new), (old, t_old)):
                t0 = time.perf_counter()
                fn()
                t.append(1e3 * (time.perf_counter() - t0))
        q = lambda t: (float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90)))
        (mn, ln, hn), (mo, lo, ho) = q(t_new), q(t_old)
        s = r["summary"]
        print(f"{name:8s} {len(p.edge_cam):6d} {len(pairs):6d} {int(s[4]):6d} {s[5]:7.3f} {f'{mn:.3f} ({ln:.3f} .. {hn:.3f})':>38s} {f'{mo:.3f} ({lo:.3f} .. {ho:.3f})':>30s} "
              f"{mn / mo:6.2f} {mn - mo:9.3f}")


if __name__ == "__main__":
    main()
