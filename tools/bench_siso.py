"""Times the in-process SISO evaluation (row N4): suo_pose_errors_points' ADI (csrc/eval_points.hip) per 1000 (estimate, ground truth) pairs at the point
counts of the synthetic models and at 10 000 points, suo_pose_errors_masks (csrc/eval_masks.hip: cus / cou_bb_proj) per 1000 pairs at 720 x 540, and the SISO
VSD evaluation of the synthetic T-LESS tree end to end (bop_eval.LocalizationMeter over the device) next to the numpy meter of
tests/test_gpu_siso_evaluator.py.  Medians after warm-up, one process, host wall clock around the blocking calls (staging, upload and read-back included: call
times, not kernel times).  The parent commit has no in-process SISO evaluation to time against.  A record, not a gate.

    python tools/bench_siso.py [--reps 10] [--pairs 1000] [--out profiles/siso.txt]"""
import argparse
import datetime
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop, bop_eval  # noqa: E402
from tests import bop_tree  # noqa: E402
from tests import points_errors_ref as PR  # noqa: E402
from tests import vsd_ref as VR  # noqa: E402
from tests.golden import bop19_cases as BC  # noqa: E402

PEAK_FP64_VECTOR = 78.6e12                       # flop/s with every instruction a fused multiply-add (the vendor's peak); 39.3e12 instructions/s
OPS_PER_PAIR = 9                                 # 3 sub, 3 mul, 2 add, 1 min: -ffp-contract=off, none of them fused


def _median_ms(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def _box():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{torch.cuda.device_count()} x {p.name} ({getattr(p, 'gcnArchName', '').split(':')[0]}, {p.multi_processor_count} CUs), one used"
    except Exception:
        return "unknown"


def _poses(rng, n, spread=(260.0, 200.0), z=(650.0, 800.0), rot=0.1, trans=5.0):
    Tg = np.stack([np.hstack((BC.random_rotation(rng), [[rng.uniform(-spread[0], spread[0])], [rng.uniform(-spread[1], spread[1])], [rng.uniform(*z)]])) for _ in range(n)])
    Te = np.stack([BC.compose(T, np.hstack((BC.rotvec(rng.standard_normal(3) * rot), rng.standard_normal((3, 1)) * trans))) for T in Tg])
    return Te, Tg


def bench_adi(a, lines):
    rng = np.random.default_rng(0)
    counts = (60, 200, 1000, 10000)              # tests/bop_tree.py draws 60 .. 200 vertices a model; T-LESS's evaluation models hold a few thousand
    clouds = {k + 1: {"points": (rng.uniform(-1, 1, (P, 3)) * rng.uniform(30, 90, 3)).astype(np.float32)} for k, P in enumerate(counts)}
    be = bop_eval.BopErrors(clouds, {o: {"diameter": 1.0} for o in clouds})
    Te, Tg = _poses(rng, a.pairs)
    lines += [f"== ADI: suo_pose_errors_points(which = ADI), {a.pairs} pairs a call, medians of {a.reps} (min .. max) ==",
              f"{'points':>7s} {'ms a call':>24s} {'ms / 1000 pairs':>16s} {'G point pairs/s':>16s} {'fp64 instr/s':>13s} {'of 39.3 T instr/s':>18s} {'as flop/s of 78.6 T':>20s}   ADD alone"]
    for k, P in enumerate(counts):
        objs = [k + 1] * a.pairs
        med, lo, hi = _median_ms(lambda: be.point_errors(objs, Te, Tg, which=("adi",)), a.reps)
        add_ms = _median_ms(lambda: be.point_errors(objs, Te, Tg, which=("add",)), a.reps)[0]
        rate = a.pairs * P * P / (med * 1e-3)
        lines.append(f"{P:7d} {med:10.3f} ({lo:.3f} .. {hi:.3f}) {med * 1000 / a.pairs:16.3f} {rate / 1e9:16.2f} {OPS_PER_PAIR * rate / 1e12:12.2f}T {100 * OPS_PER_PAIR * rate / (PEAK_FP64_VECTOR / 2):17.1f}% "
                     f"{100 * OPS_PER_PAIR * rate / PEAK_FP64_VECTOR:19.1f}%   {add_ms:.3f} ms")
    ref = PR.adi(clouds[2]["points"], Te[0], Tg[0])
    dev = be.point_errors([2], Te[:1], Tg[:1], which=("adi",))["adi"][0]
    lines += [f"pair 0 at 200 points: device {dev!r}, numpy restatement {ref!r}",
              "What bounds it: the pair loop is fp64 VALU issue -- 9 instructions a point pair, none fused under -ffp-contract=off (the kernels must round like",
              "the toolkit's numpy), so its ceiling is the instruction rate, half the quoted 78.6 TF/s, and the column beside it is the share of that; one",
              "broadcast LDS read of 24 bytes feeds 36 of them.  A call's fixed cost -- staging, one upload, two launches, one read-back, a synchronise -- is",
              "the ADD-alone column, and is what a call at a few hundred points measures.", ""]
    be.close()


def bench_cus(a, lines):
    rng = np.random.default_rng(1)
    W, H = 720, 540
    pts, faces = VR.icosphere(radius=80.0, subdivisions=5)
    mesh_db = {o: {"points": (pts * rng.uniform(0.4, 1.0, 3).astype(np.float32)).astype(np.float32), "faces": faces} for o in range(1, 7)}
    be = bop_eval.BopErrors(mesh_db, {o: {"diameter": 160.0} for o in mesh_db})
    K = np.array([[1075.65, 0, 360.0], [0, 1073.9, 270.0], [0, 0, 1]])
    Te, Tg = _poses(rng, a.pairs)
    objs = [int(rng.integers(1, 7)) for _ in range(a.pairs)]
    med, lo, hi = _median_ms(lambda: be.mask_errors(objs, Te, Tg, K, (H, W)), a.reps)
    out = be.mask_errors(objs, Te, Tg, K, (H, W))
    u, i, be_, bg = PR.mask_counts(mesh_db[objs[0]]["points"], faces, Te[0], Tg[0], K, W, H)
    lines += [f"== CUS / COU_BB_PROJ: suo_pose_errors_masks, {a.pairs} pairs a call at {W} x {H}, meshes of {len(faces)} faces, medians of {a.reps} (min .. max) ==",
              f"{med:10.3f} ms a call ({lo:.3f} .. {hi:.3f})   {med * 1000 / a.pairs:.3f} ms / 1000 pairs   {1e3 * a.pairs / med:.0f} pairs/s   "
              f"mean union {out['union'].mean():.0f} px, mean cus {out['cus'].mean():.4f}",
              f"pair 0: device union {int(out['union'][0])} inter {int(out['inter'][0])} boxes {out['box_est'][0].tolist()} {out['box_gt'][0].tolist()}; "
              f"numpy rasteriser {u} {i} {be_} {bg}",
              f"no depth image leaves the device: {2 * W * H * 4 / 1e6:.1f} MB a pair stay in LDS tile by tile; 40 B of record a pair come back", ""]
    be.close()


def bench_tree(a, lines):
    rng = np.random.default_rng(2)
    with tempfile.TemporaryDirectory() as tmp:
        desc = bop_tree.build(tmp, dset="tless", seed=31, n_scenes=2, n_views=2)
        root, split = desc["data_root"], desc["split"]
        mesh = bop.load_mesh_db(os.path.join(root, "models_eval"), faces=True)
        VR.add_depth(desc, mesh, seed=9)
        ds = bop.BopDataset(root, split, bop_dset="tless", ignore_symmetry=True)
        info = bop_eval.load_models_info(os.path.join(root, "models_eval"))
        with open(os.path.join(root, "all_target_tless.json")) as f:
            targets = json.load(f)
        ests = []
        for t in targets:                                                      # estimates: the ground truths of the targets, perturbed
            gts = json.load(open(os.path.join(root, split, f"{t['scene_id']:06d}", "scene_gt.json")))[str(t["im_id"])]
            cam = json.load(open(os.path.join(root, split, f"{t['scene_id']:06d}", "scene_camera.json")))[str(t["im_id"])]
            g = next(g for g in gts if g["obj_id"] == t["obj_id"])
            T = np.hstack((np.reshape(g["cam_R_m2c"], (3, 3)), np.reshape(g["cam_t_m2c"], (3, 1))))
            T = BC.compose(T, np.hstack((BC.rotvec(rng.standard_normal(3) * 0.05), rng.standard_normal((3, 1)) * 3.0)))
            ests.append((t["scene_id"], t["im_id"], t["obj_id"], float(rng.uniform(0.2, 1.0)), T, np.reshape(cam["cam_K"], (3, 3))))

        def run(errors):
            m = bop_eval.LocalizationMeter.from_dataset_tree(errors, os.path.join(root, split), os.path.join(root, "all_target_tless.json"), depth_loader=ds.read_depth,
                                                             obj_ids=sorted(mesh), symmetric_obj_ids=[o for o, v in mesh.items() if v["is_symmetric"]], **bop_eval.SISO_PARAMS)
            for e in ests:
                m.add(*e)
            return m.result()
        be = bop_eval.BopErrors(mesh, info)
        med, lo, hi = _median_ms(lambda: run(be), a.reps)
        got = run(be)
        be.close()
        t0 = time.perf_counter()
        want = run(PR.RefSisoErrors(mesh, info))
        t_ref = 1e3 * (time.perf_counter() - t0)
    lines += [f"== SISO VSD (tau 20, th 0.3, n_top 1, visib >= 0.1) of the synthetic T-LESS tree: 2 scenes x 3 images of 640 x 480, {len(targets)} targets, {len(ests)} estimates ==",
              f"LocalizationMeter over the device   {med:10.3f} ms ({lo:.3f} .. {hi:.3f}), depth PNGs read and decoded each time",
              f"the same over the numpy rasteriser and numpy VSD (one run)   {t_ref:10.1f} ms   -> {t_ref / med:.0f}x",
              f"recall {got['recall']:.4f} ({got['tp_count']} of {got['targets_count']} targets); equal to the numpy meter: {got == want}", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siso.txt"))
    a = ap.parse_args()
    lines = ["In-process SISO evaluation (csrc/eval_points.hip, csrc/eval_masks.hip, bop_eval.LocalizationMeter; row N4), MI355X.  A record, not a gate.",
             f"box: {_box()}   date: {datetime.date.today().isoformat()}",
             f"python tools/bench_siso.py --reps {a.reps} --pairs {a.pairs}: host wall clock around blocking calls after 2 warm-up calls, one process", ""]
    bench_adi(a, lines)
    bench_cus(a, lines)
    bench_tree(a, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
