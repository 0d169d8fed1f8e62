"""Times ObjectSLAM.tracking_covariance with a cached map covariance -- the covariance of the current view with the map's uncertainty carried in,
suo_tracking_covariances (csrc/track_cov.hip) on the view's curr_only graph -- in one run on one GPU, beside the only route to that figure there was before:
ObjectSLAM.pose_covariances() of the whole global graph, rebuilt and inverted for every view.  The state is a map of 60 views x 8, 16 and 64 objects, made from
synthetic.make_pose_graph at the poses suo_optimize leaves and installed in an ObjectSLAM without a network.  Host wall clock around the blocking Python calls
(graph assembly, staging and read-back included), per view:

  tracking              ObjectSLAM.tracking_covariance(view, map_cov=cached) of the last view
  of which the entry    ba.tracking_covariances_batch on the same problem and map covariance (the C call alone)
  whole graph           ObjectSLAM.pose_covariances() on the same state
  map, once             ObjectSLAM.map_covariance(): paid once per global adjustment, not per view

The calls ALTERNATE inside one loop, so that whatever else the host and the GPU are doing falls on all of them; medians, with the 10th and 90th percentile as the
spread.  Also prints trace(cam) / trace(cam_fixed_map): by how much Hcc^-1 alone understates the camera's covariance on that map.

Writes nothing: redirect into profiles/track_cov.txt.

    python tools/bench_track_cov.py [--reps 30]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suo_slam_amd import ba  # noqa: E402
from suo_slam_amd import synthetic as S  # noqa: E402
from suo_slam_amd.object_slam import ObjectSLAM  # noqa: E402

KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")
GRAPHS = {"60x8": (60, 8), "60x16": (60, 16), "60x64": (60, 64)}


def _slam_state(rng, C, O):
    """an ObjectSLAM (no network) holding the refined graph: one detection per (view, object) that carries edges"""
    g = S.make_pose_graph(rng, C, O)
    p = ba.Problem(*[g[k] for k in KEYS])
    ba.optimize_batch([p])
    cam_T, obj_T, inl = p.cam_T.reshape(-1, 3, 4), p.obj_T.reshape(-1, 3, 4), np.asarray(p.inlier).astype(bool)
    slam = ObjectSLAM(None, None, debug_gt_kp=True)
    k = g["edge_camk"][0]
    K = np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]])
    info = g["edge_info"][0]
    cov = np.linalg.inv(np.array([[info[0], info[1]], [info[1], info[2]]]))
    for c in range(C):
        slam.view_ids.append(c)
        slam.cam_poses[c] = cam_T[c].copy()
        slam.detections[c] = {}
    for o in range(O):
        slam.obj_poses[o] = obj_T[o].copy()
    pair = g["edge_cam"].astype(np.int64) * O + g["edge_obj"]
    for q in np.unique(pair):
        e = np.flatnonzero(pair == q)
        slam.detections[int(q // O)][int(q % O)] = {"inliers": inl[e].copy(), "uv_pred": g["edge_uv"][e].copy(), "cov_pred": np.tile(cov, (len(e), 1, 1)),
                                                   "model_kp": g["edge_p"][e].copy(), "K": K}
    return slam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    q = lambda t: f"{np.median(t):.3f} ({np.percentile(t, 10):.3f} .. {np.percentile(t, 90):.3f})"
    print(f"{'map':7s} {'view edges':>10s} {'graph edges':>11s} {'tracking ms (p10 .. p90)':>28s} {'of which the entry':>26s} {'whole graph ms':>28s} {'ratio':>7s} "
          f"{'map, once ms':>26s} {'tr(cam)/tr(fixed map)':>22s}")
    for name, (C, O) in GRAPHS.items():
        slam = _slam_state(rng, C, O)
        view = slam.view_ids[-1]
        cached = slam.map_covariance(exclude_views=(view,))          # the map without the tracked view: what tracking_covariance assumes
        prob, (_, obj_index, _, _, _) = slam.build_problem(True, view=view)
        at = np.concatenate([np.arange(6 * o, 6 * o + 6) for o in obj_index])
        sub = np.ascontiguousarray(cached[1][np.ix_(at, at)])
        calls = {"track": lambda: slam.tracking_covariance(view, map_cov=cached), "entry": lambda: ba.tracking_covariances_batch([prob], [sub]),
                 "whole": lambda: slam.pose_covariances(), "map": lambda: slam.map_covariance()}
        times = {k: [] for k in calls}
        for _ in range(3):
            for fn in calls.values():
                r = fn()
        for _ in range(a.reps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(1e3 * (time.perf_counter() - t0))
        r = calls["track"]()
        n_graph = len(slam.build_problem(False)[0].edge_cam)
        print(f"{name:7s} {len(prob.edge_cam):10d} {n_graph:11d} {q(times['track']):>28s} {q(times['entry']):>26s} {q(times['whole']):>28s} "
              f"{np.median(times['whole']) / np.median(times['track']):7.1f} {q(times['map']):>26s} {np.trace(r['cam']) / np.trace(r['cam_fixed_map']):22.2f}")


if __name__ == "__main__":
    main()
