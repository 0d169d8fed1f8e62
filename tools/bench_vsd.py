"""Times suo_pose_errors_vsd (csrc/raster.hip + csrc/eval_vsd.hip) at a T-LESS shape -- 64 (estimate, ground truth) pairs at 640 x 480 against one test depth
image each, an evaluation mesh of 20 480 faces (an icosphere) about 200 px across, ten taus -- beside suo_render_depth alone and the numpy restatement
(tests/vsd_ref.py) of one pair on the same box.  Medians, host wall clock around the blocking C calls (staging, the upload of the test images and the
read-back included).  The account printed with the times: triangle records written and scanned, samples tested, image bytes.  A record, not a gate.

    python tools/bench_vsd.py [--reps 10] [--pairs 64] [--out profiles/vsd.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop_eval  # noqa: E402
from tests import vsd_ref as VR  # noqa: E402
from tests.golden import bop19_cases as BC  # noqa: E402

W, H, TILE, RECORD = 640, 480, 64, 88


def _median_ms(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsd.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n = a.pairs
    pts, faces = VR.icosphere(radius=80.0, subdivisions=5)
    pts = (pts * np.array([1.0, 0.8, 0.6], np.float32)).astype(np.float32)
    F = len(faces)
    K = np.array([[1075.65, 0, 320.0], [0, 1073.9, 240.0], [0, 0, 1]])
    be = bop_eval.BopErrors({1: {"points": pts, "faces": faces}}, {1: {"diameter": 160.0}})
    Tg = np.stack([np.hstack((BC.random_rotation(rng), [[rng.uniform(-120, 120)], [rng.uniform(-80, 80)], [rng.uniform(650, 750)]])) for _ in range(n)])
    Te = np.stack([BC.compose(T, np.hstack((BC.rotvec(rng.standard_normal(3) * 0.05), rng.standard_normal((3, 1)) * 4))) for T in Tg])
    ids = [1] * n
    gt = be.render_depth(ids, Tg, K, (H, W))
    tests = [np.where(g > 0, g, np.float32(1200.0)).astype(np.float32) for g in gt]
    for t in tests:
        t[200:260, 280:380] = 400.0
        t[100:140, 100:160] = 0.0
    covered = float(np.mean([(g > 0).sum() for g in gt]))
    across = float(np.mean([np.ptp(np.nonzero((g > 0).any(0))[0]) + 1 for g in gt]))
    old = bop_eval.VSD_PAIRS_PER_CALL
    bop_eval.VSD_PAIRS_PER_CALL = n                                            # one device call for the whole batch
    t_vsd = _median_ms(lambda: be.vsd(ids, Te, Tg, K, tests, list(range(n))), a.reps)
    t_ren = _median_ms(lambda: be.render_depth(ids + ids, np.concatenate((Te, Tg)), K, (H, W)), a.reps)
    errs, counts = be.vsd(ids, Te, Tg, K, tests, list(range(n)), return_counts=True)
    bop_eval.VSD_PAIRS_PER_CALL = old
    t0 = time.perf_counter()
    de, dg = VR.render_depth(pts, faces, Te[0], K, W, H), VR.render_depth(pts, faces, Tg[0], K, W, H)
    e_np, c_np = VR.vsd_from_depth(de, dg, tests[0], K, 15, bop_eval.VSD_TAUS, True, 160.0)
    t_np = 1e3 * (time.perf_counter() - t0)
    be.close()
    tiles = -(-W // TILE) * -(-H // TILE)
    hit_tiles = float(np.mean([len({(y // TILE, x // TILE) for y, x in zip(*np.nonzero(g > 0))}) for g in gt[:8]]))
    lines = [
        "BOP-19 VSD on the device (csrc/raster.hip, csrc/eval_vsd.hip, row N6), MI355X.  A record, not a gate.",
        "",
        f"== Time: python tools/bench_vsd.py (medians of {a.reps}, blocking C calls, staging, upload of the test images and read-back included) ==",
        f"{n} pairs at {W} x {H}, mesh of {F} faces / {len(pts)} vertices, {across:.0f} px across, {covered:.0f} covered pixels a render, 10 taus",
        f"suo_pose_errors_vsd   {t_vsd:9.3f} ms a call   {t_vsd / n:8.4f} ms a pair   (2 renders a pair on the device + the error kernel + {n} test images up)",
        f"suo_render_depth      {t_ren:9.3f} ms a call   {t_ren / (2 * n):8.4f} ms a render (the same {2 * n} renders, their {2 * n * W * H * 4 / 1e6:.0f} MB of images copied to the host)",
        f"numpy (tests/vsd_ref.py), one pair on this box's CPU: {t_np:.0f} ms   -> {t_np * n / t_vsd:.0f}x",
        f"pair 0: device counts {counts[0].tolist()}  numpy counts {c_np}  equal errors: {errs[0].tolist() == list(e_np)}",
        "",
        "== Account for one call ==",
        f"setup kernel    {2 * n * F} triangle records of {RECORD} B written: {2 * n * F * RECORD / 1e6:.0f} MB; {2 * n * F * 3} vertex transforms and projections in fp64",
        f"raster kernel   {2 * n * tiles} workgroups, about {hit_tiles:.0f} of a render's {tiles} tiles meet its box; each of those scans the render's {F} boxes "
        f"(16 B each: {F * 16 / 1e3:.0f} kB a tile, {2 * n * hit_tiles * F * 16 / 1e6:.0f} MB a call, from L2) and reads 72 B more for a triangle that meets the tile;",
        f"                samples tested ~ 2-4 per covered pixel (boxes of ~1 px^2 triangles): about {2 * n * covered * 3 / 1e6:.0f} M edge-function triples "
        "(9 fp64 multiplies, 12 adds) and, for a covered one, 2 fp64 divisions and an LDS atomicMin;",
        f"                images written {2 * n * W * H * 4 / 1e6:.0f} MB (every tile stores its 64 x 64 floats, zeros included)",
        f"error kernel    {n * tiles} workgroups, those outside the union of the two boxes leave at once; a pixel with a model depth costs 3 fp64 square roots, "
        f"2 divisions; reads 3 images over the union box: about {n * hit_tiles * TILE * TILE * 12 / 1e6:.0f} MB; {n * H * W * 4 / 1e6:.0f} MB of test images uploaded from the host",
    ]
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
