"""Times suo_model_info (csrc/model_info.hip, row N8) at 8 192, 65 536 and 262 144 points a model, for one model and for 21 (a YCB-V-sized database),
beside the same O(N^2) scan in numpy on the same box's CPU, one pass per point as the toolkit's misc.calc_pts_diameter makes it (host_diameter below: a
broadcast difference where the toolkit copies the point with np.tile, otherwise the same work per row).  The CPU loop is run only up to the size expected -- by N^2 from the size before -- to finish in about a minute; larger rows are marked
"extrapolated by N^2".  Device times are medians after warm-up, one process, host wall clock around the blocking call (staging and read-back included).
Also the pairs/s reached and their share of the fp64 vector rate at 9 operations a pair.  A record, not a gate.

    python tools/bench_model_info.py [--reps 5] [--cpu-budget 75] [--out profiles/model_info.txt]"""
import argparse
import datetime
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop_model_info  # noqa: E402

SIZES = (8192, 65536, 262144)
MODELS = 21
# MI355X: 256 CUs x 4 SIMDs x 16 fp64 lanes a clock x 2.4 GHz.  The 78.6 TFLOP/s of the data sheet count an fma as two; + - x max are one operation each.
FP64_OPS = 256 * 4 * 16 * 2.4e9


def host_diameter(p):
    """The host baseline: the O(N^2) scan as the toolkit's misc.calc_pts_diameter does it -- one numpy pass per point over the points from it onward
    (differences, squares, a 3-term row sum, a maximum, a square root) -- written here; the toolkit is not part of this repository.  Broadcasting stands
    in for the toolkit's np.tile copy of the point: one temporary less per row, the same arithmetic and the same bits."""
    best = 0.0
    for i in range(len(p)):
        d = p[i] - p[i:]
        best = max(best, math.sqrt((d * d).sum(axis=1).max()))
    return best


def _median_ms(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def _box():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{torch.cuda.device_count()} x {p.name} ({getattr(p, 'gcnArchName', '').split(':')[0]}, {p.multi_processor_count} CUs), one used"
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-budget", type=float, default=75.0, help="seconds the CPU loop may be expected to take at a size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_info.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    tile, itile = bop_model_info.tiles()
    rows, cpu_s, cpu_n = [], None, None
    for n in SIZES:
        clouds = [(rng.normal(size=(n, 3)) * (60.0, 45.0, 30.0)).astype(np.float32) for _ in range(MODELS)]
        with bop_model_info.PointDb(clouds) as db:
            one = _median_ms(lambda: db.run([0], pairs=False), a.reps)
            one_pair = _median_ms(lambda: db.run([0], pairs=True), a.reps)
            many = _median_ms(lambda: db.run(list(range(MODELS)), pairs=False), a.reps)
            info, _, _ = db.run([0], pairs=False)
        expect = None if cpu_s is None else cpu_s * (n / cpu_n) ** 2
        if expect is None or expect <= a.cpu_budget:
            t0 = time.perf_counter()
            d = host_diameter(clouds[0].astype(np.float64))
            cpu_s, cpu_n, how = time.perf_counter() - t0, n, "measured"
            assert d == info[0, 6], (d, info[0, 6])                            # the same bits on both paths
            cpu = cpu_s
        else:
            cpu, how = expect, f"extrapolated by N^2 from {cpu_n}"
        pairs = n * (n + 1) / 2
        rows.append((n, one, one_pair, many, cpu, how, pairs))
    lines = [
        "models_info (3-D box and diameter) on the device (csrc/model_info.hip, row N8), MI355X.  A record, not a gate.",
        f"box: {_box()}   date: {datetime.date.today().isoformat()}",
        "",
        f"== Time: python tools/bench_model_info.py (device: medians of {a.reps} after 2 warm-up calls, one process, blocking calls, staging and read-back included;",
        "   CPU: host_diameter of the tool -- the toolkit's per-point numpy scan with a broadcast difference in place of its np.tile copy -- one run, one model, this box's CPU;",
        "   the measured rows gave the device's bits) ==",
        f"tiles: {itile} i-points in registers x {tile} j-points in LDS a work item; pairs = N (N + 1) / 2, 9 fp64 operations each; "
        f"fp64 vector rate taken as {FP64_OPS / 1e12:.1f}e12 operations/s (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz; an fma would count twice)",
        "",
        f"{'points':>8s} {'1 model':>11s} {'with pair':>11s} {str(MODELS) + ' models':>11s} {'pairs/s (1)':>12s} {'share':>6s} {'pairs/s (' + str(MODELS) + ')':>13s} {'share':>6s} {'CPU, 1 model':>13s}   {'CPU / device':>12s}",
    ]
    for n, one, one_pair, many, cpu, how, pairs in rows:
        r1, rm = pairs / (one * 1e-3), MODELS * pairs / (many * 1e-3)
        lines.append(f"{n:8d} {one:8.3f} ms {one_pair:8.3f} ms {many:8.3f} ms {r1:12.3e} {100 * 9 * r1 / FP64_OPS:5.1f}% {rm:13.3e} {100 * 9 * rm / FP64_OPS:5.1f}% {cpu:11.2f} s   "
                     f"{cpu / (one * 1e-3):10.0f}x   ({how})")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
