"""Times suo_pose_nees at n = 4096 pairs over a 1500-point model with the 314 symmetry transformations of one continuous axis at the default step (ceil(pi / 0.01) - 1), beside
suo_pose_errors_bop (MSSD only) on the same pairs -- the P x S pass the two share -- and suo_keypoint_nees on 4096 x 16 keypoints.  Medians, host wall clock
around the blocking C calls (staging and read-back included).  For the record: the parent has nothing to compare with.  Writes nothing: redirect into
profiles/consistency.txt.

    python tools/bench_consistency.py [--reps 20]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suo_slam_amd import _lib, bop_eval  # noqa: E402


def _median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=4096)
    a = ap.parse_args()
    lib = _lib.lib()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    n, P = a.n, 1500
    cloud = (rng.uniform(-1, 1, (P, 3)) * [50.0, 35.0, 60.0]).astype(np.float32)                 # mm
    syms = np.ascontiguousarray(bop_eval.symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01).reshape(-1, 12))
    h = C.c_void_p()
    _lib.check(lib.suo_mesh_db_create(1, np.array([P], np.int32).ctypes.data, cloud.ctypes.data, C.byref(h)), "suo_mesh_db_create")
    _lib.check(lib.suo_mesh_db_set_symmetries(h, np.array([len(syms)], np.int32).ctypes.data, syms.ctypes.data), "suo_mesh_db_set_symmetries")
    Tg = np.zeros((n, 3, 4))
    for i in range(n):
        Tg[i, :, :3], Tg[i, :, 3] = _rot(rng), [rng.uniform(-100, 100), rng.uniform(-80, 80), rng.uniform(500, 1500)]
    Te = Tg.copy()
    Te[:, :, 3] += rng.normal(0, 2.0, (n, 3))
    idx = np.zeros(n, np.int32)
    cov = np.ascontiguousarray(np.tile(np.diag([1e-4] * 3 + [4.0] * 3).reshape(36), (n, 1)))
    nees, xi, sym, Tr, status, mssd = np.zeros(n), np.zeros((n, 6)), np.zeros(n, np.int32), np.zeros((n, 12)), np.zeros(1, np.int32), np.zeros(n)

    def run_nees():
        _lib.check(lib.suo_pose_nees(h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, cov.ctypes.data, nees.ctypes.data, xi.ctypes.data, sym.ctypes.data,
                                     Tr.ctypes.data, status.ctypes.data), "suo_pose_nees")

    def run_mssd():
        _lib.check(lib.suo_pose_errors_bop(h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, None, mssd.ctypes.data, None), "suo_pose_errors_bop")
    t_nees, t_mssd = _median_ms(run_nees, a.reps), _median_ms(run_mssd, a.reps)
    assert status[0] == 0 and np.isfinite(nees).all()
    k = 16
    n_pts = np.full(n, k, np.int32)
    kp, uv, cv = rng.uniform(-50, 50, (n * k, 3)), rng.uniform(-1, 1, (n * k, 2)), np.ascontiguousarray(np.tile(np.eye(2).reshape(4) * 1e-4, (n * k, 1)))
    K = np.ascontiguousarray(np.tile(np.array([10.0, 0, 0, 0, 10.0, 0, 0, 0, 1.0]), (n, 1)))
    chi2, err = np.zeros(n * k), np.zeros((n * k, 2))
    Tg12 = np.ascontiguousarray(Tg.reshape(n, 12))

    def run_kp():
        _lib.check(lib.suo_keypoint_nees(h, n, n_pts.ctypes.data, kp.ctypes.data, uv.ctypes.data, cv.ctypes.data, K.ctypes.data, Tg12.ctypes.data, chi2.ctypes.data,
                                         err.ctypes.data), "suo_keypoint_nees")
    t_kp = _median_ms(run_kp, a.reps)
    lib.suo_mesh_db_destroy(h)
    print(f"suo_pose_nees        n = {n}, {P} points, {len(syms)} symmetries: {t_nees:9.3f} ms  (median of {a.reps})")
    print(f"suo_pose_errors_bop  the same pairs, MSSD only:                 {t_mssd:9.3f} ms  -> the arg-min, logarithm and NEES add {t_nees - t_mssd:+.3f} ms")
    print(f"suo_keypoint_nees    {n} detections x {k} keypoints:             {t_kp:9.3f} ms")


if __name__ == "__main__":
    main()
