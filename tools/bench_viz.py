#!/usr/bin/env python3
"""Time a view's three-panel visualisation on the device (suo_viz_view, csrc/viz.hip) against tests/viz_ref.py on the CPU:

    python tools/bench_viz.py [--out profiles/viz.txt] [--calls 200]

The view is synthetic: 640 x 480, 8 objects, each with a box, 14 keypoints, 14 prior stamps and a mesh of 30 000 points at its pose (240 000 points a view),
with and without covariance ellipses (viz_cov).  Device time is taken with HIP events around ``calls`` back-to-back suo_viz_view calls on one stream (the call
does not wait for the device); host time is the wall time of those calls' enqueueing, descriptor packing included.  A record, not a gate."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import viz_ref  # noqa: E402


def synthetic_view(H=480, W=640, n_obj=8, n_kp=14, n_pts=30000, seed=0, with_cov=True):
    from suo_slam_amd import viz
    rng = np.random.default_rng(seed)
    kp_cols, box_cols = viz.colour_tables()
    K = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])
    box, stamp, kp, ang, overlay, points = [], [], [], [], [], {}
    for i in range(n_obj):
        o = i + 1
        cx, cy = rng.uniform(100, W - 100), rng.uniform(80, H - 80)
        x1, y1, x2, y2 = int(cx - 70), int(cy - 60), int(cx + 70), int(cy + 60)
        box.append([x1, y1, x2, y2, viz.pack(box_cols[o - 1])])
        wx0, wx1, _ = slice(x1, x2).indices(W)
        wy0, wy1, _ = slice(y1, y2).indices(H)
        for k in rng.choice(41, n_kp, replace=False):
            x, y = int(rng.uniform(x1, x2)), int(rng.uniform(y1, y2))
            A, B = int(rng.integers(2, 30)), int(rng.integers(2, 30))
            kp.append([x, y, 10, 8, viz.pack(kp_cols[k]), int(with_cov), A if with_cov else 0, B if with_cov else 0])
            ang.append(float(rng.uniform(-180, 180)) if with_cov else 0.0)
            stamp.append([int(k), x - 45 + int(rng.integers(-6, 7)), y - 45 + int(rng.integers(-6, 7)), wx0, max(wx1, wx0), wy0, max(wy1, wy0), o])
        z = rng.uniform(600, 1100)
        T = np.eye(4)[:3]
        T[:, 3] = [(cx - K[0, 2]) * z / K[0, 0], (cy - K[1, 2]) * z / K[1, 1], z]
        overlay.append((o, viz.pack(box_cols[o - 1]), T, K))
        d = rng.normal(size=(n_pts, 3))
        points[o] = (60.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)          # a sphere of 60 mm
    overlay.sort(key=lambda e: -e[2][2, 3])
    prims = {"box": np.array(box, np.int64), "stamp": np.array(stamp, np.int64), "kp": np.array(kp, np.int64), "kp_angle": np.array(ang), "overlay": overlay}
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return frame, prims, points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    import torch
    from suo_slam_amd import viz
    lines = ["A view's three-panel visualisation on the device (csrc/viz.hip: viz_splat_kernel + viz_compose_kernel), MI355X.  A record, not a gate.",
             f"device: {torch.cuda.get_device_name(0)}   python tools/bench_viz.py --calls {args.calls}",
             "view: 640 x 480, 8 objects: 8 boxes, 112 keypoints, 112 prior stamps, 8 meshes of 30 000 points (240 000 points); out uint8 [480][1920][3] = 2.76 MB", ""]
    for with_cov in (False, True):
        frame, prims, points = synthetic_view(with_cov=with_cov)
        vz = viz.Visualizer({o: {"points": p} for o, p in points.items()}, *frame.shape[:2])
        frame_dev = torch.from_numpy(frame).cuda()
        t0 = time.perf_counter()
        want = viz_ref.render(frame, prims, points, viz.colour_tables()[0])
        cpu_ms = 1e3 * (time.perf_counter() - t0)
        got = vz.render(frame_dev, prims)
        equal = bool(np.array_equal(got, want))
        for _ in range(10):
            vz.render_device(frame_dev, prims)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dev_ms = []
        for _rep in range(5):
            t0 = time.perf_counter()
            ev0.record()
            for _ in range(args.calls):
                out = vz.render_device(frame_dev, prims)
                if (_ + 1) % 4 == 0:                      # (the staging ring takes 8 views in flight: keep well inside it)
                    torch.cuda.current_stream().synchronize()
            ev1.record()
            host_ms = 1e3 * (time.perf_counter() - t0) / args.calls
            torch.cuda.synchronize()
            dev_ms.append(ev0.elapsed_time(ev1) / args.calls)
        t0 = time.perf_counter()
        for _ in range(20):
            vz.render(frame_dev, prims)
        sync_ms = 1e3 * (time.perf_counter() - t0) / 20
        del out
        vz.close()
        lines.append(f"viz_cov={with_cov!s:5}  suo_viz_view {np.median(dev_ms):.4f} ms a view between events (median of 5 x {args.calls}; a stream wait every 4th call included), "
                     f"{host_ms:.4f} ms wall a call;  with the 2.76 MB read-back to numpy {sync_ms:.3f} ms;  tests/viz_ref.py on the CPU {cpu_ms:.1f} ms;  equal: {equal}")
    lines += ["", "beside it: the tracking time of a view is 4.5-4.8 ms (profiles/r06_slam_run.txt); the reference's authors put their visualisation at '200ms or so per image'",
              "(lib/args.py:122-123), which is why they time with --no_viz."]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
