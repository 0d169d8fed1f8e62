"""Times suo_gt_info (csrc/gt_info.hip, row N7) on a T-LESS-shaped load -- 720 x 540 test images, a call of 32 images with 8 instances each (a scene of
504 images goes through in 16 such calls), random poses over a mesh database of six evaluation meshes of 20 480 faces -- beside what the library could do
for the same numbers before this row: suo_render_depth at 2160 x 1620, the canvas copied to the host, and numpy (tests/gt_info_ref.py's arithmetic on the
device's render).  Medians after warm-up, one process, host wall clock around the blocking calls (staging, upload of the test images and read-back
included).  A record, not a gate.

    python tools/bench_gt_info.py [--reps 10] [--images 32] [--per-image 8] [--old 8] [--out profiles/gt_info.txt]"""
import argparse
import datetime
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop_eval  # noqa: E402
from tests import gt_info_ref as GR  # noqa: E402
from tests import vsd_ref as VR  # noqa: E402
from tests.golden import bop19_cases as BC  # noqa: E402

W, H, TILE, RECORD = 720, 540, 64, 88


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


def old_path(be, obj_ids, T, K, tests, ii, delta):
    """The same six entries with the entries the library had before: the 3x canvas rendered on the device, copied out, reduced with numpy."""
    Kc = GR.canvas_K(K, W, H)
    out = []
    for b in range(0, len(obj_ids), 4):                                        # 14 MB a canvas: four a call
        large = be.render_depth(obj_ids[b:b + 4], T[b:b + 4], Kc, (3 * H, 3 * W))
        for k, lg in enumerate(large):
            dist_gt, dist_test = GR.dist_im(lg[H:2 * H, W:2 * W], K), GR.dist_im(tests[ii[b + k]], K)
            visib = GR.visib_mask(dist_test, dist_gt, delta)
            cov = lg > 0
            n_all, n_visib = int(cov.sum()), int(visib.sum())
            e = {"px_count_all": n_all, "px_count_valid": int(((dist_gt > 0) & (dist_test > 0)).sum()), "px_count_visib": n_visib,
                 "visib_fract": n_visib / float(n_all) if n_all else 0.0, "bbox_obj": [-1] * 4, "bbox_visib": [-1] * 4}
            if n_visib:
                ys, xs = cov.nonzero()
                e["bbox_obj"] = [int(xs.min()) - W, int(ys.min()) - H, int(xs.max() - xs.min()), int(ys.max() - ys.min())]
                ys, xs = visib.nonzero()
                e["bbox_visib"] = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]
            out.append(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--per-image", type=int, default=8)
    ap.add_argument("--old", type=int, default=8, help="instances timed on the old path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_info.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    pts, faces = VR.icosphere(radius=80.0, subdivisions=5)
    F = len(faces)
    mesh_db = {o: {"points": (pts * rng.uniform(0.4, 1.0, 3).astype(np.float32)).astype(np.float32), "faces": faces} for o in range(1, 7)}
    be = bop_eval.BopErrors(mesh_db, {o: {"diameter": 160.0} for o in mesh_db})
    K = np.array([[1075.65, 0, 360.0], [0, 1073.9, 270.0], [0, 0, 1]])
    n = a.images * a.per_image
    obj_ids = [int(rng.integers(1, 7)) for _ in range(n)]
    ii = [i // a.per_image for i in range(n)]
    # objects over and somewhat beyond the image: some truncated by its border
    T = np.stack([np.hstack((BC.random_rotation(rng), [[rng.uniform(-260, 260)], [rng.uniform(-200, 200)], [rng.uniform(650, 800)]])) for _ in range(n)])
    tests = []
    for k in range(a.images):
        sl = slice(k * a.per_image, (k + 1) * a.per_image)
        d = be.render_depth(obj_ids[sl], T[sl], K, (H, W))
        d = np.where(d > 0, d, np.inf).min(0)
        t = np.where(np.isfinite(d), d, 1200.0).astype(np.float32)
        t[200:300, 280:420] = 400.0
        t[100:160, 100:180] = 0.0
        tests.append(t)
    t_new = _median_ms(lambda: be.gt_info(obj_ids, T, K, tests, ii), a.reps)
    new = be.gt_info(obj_ids, T, K, tests, ii)
    m = min(a.old, n)
    t_old = _median_ms(lambda: old_path(be, obj_ids[:m], T[:m], K, tests, ii, 15), max(3, a.reps // 3))
    old = old_path(be, obj_ids[:m], T[:m], K, tests, ii, 15)
    be.close()
    tiles = -(-3 * W // TILE) * -(-3 * H // TILE)
    covered = float(np.mean([e["px_count_all"] for e in new]))
    fract = float(np.mean([e["visib_fract"] for e in new]))
    in_bytes = 96 + 72 + 4 + 4 + 32 + 4 + 16                                     # pose, K, model, record offset, image K, image index, staged box
    out_bytes = 11 * 4
    lines = [
        "scene_gt_info on the device (csrc/gt_info.hip, row N7), MI355X.  A record, not a gate.",
        f"box: {_box()}   date: {datetime.date.today().isoformat()}",
        "",
        f"== Time: python tools/bench_gt_info.py (medians of {a.reps} after 2 warm-up calls, one process, blocking calls, staging, upload and read-back included) ==",
        f"{n} instances = {a.images} images of {W} x {H} with {a.per_image} each, meshes of {F} faces, {covered:.0f} covered samples an instance, mean visib_fract {fract:.3f}",
        f"suo_gt_info                         {t_new:9.3f} ms a call   {t_new / n:8.4f} ms an instance   {1e3 * n / t_new:9.0f} instances/s",
        f"suo_render_depth 2160 x 1620 + D2H + numpy, {m} instances   {t_old:9.3f} ms   {t_old / m:8.4f} ms an instance   {1e3 * m / t_old:9.0f} instances/s   -> {t_old / m / (t_new / n):.0f}x",
        f"the first {m} instances equal on both paths: {new[:m] == old}",
        "",
        "== Bytes an instance moves on the new path ==",
        f"host <-> device   {in_bytes} B of arguments up, {out_bytes} B of record down, and its share of the test images: {W * H * 4 / a.per_image / 1e3:.0f} kB "
        f"({W * H * 4 / 1e6:.2f} MB an image, uploaded once a call) -- against {9 * W * H * 4 / 1e6:.1f} MB of canvas down on the old path",
        f"device memory     {F * RECORD / 1e6:.2f} MB of triangle records written by the setup kernel ({RECORD} B each) and scanned by each of the tiles that meet the "
        f"render's box (of {tiles}; the others read 16 B and leave); test depth at covered window pixels only: at most {covered * 4 / 1e3:.0f} kB; no canvas: 0 B of "
        f"the {9 * W * H * 4 / 1e6:.1f} MB the canvas would take; {out_bytes} B of record by at most 11 integer atomics a workgroup",
    ]
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
