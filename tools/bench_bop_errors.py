"""Times suo_pose_errors_bop (csrc/eval_bop.hip) at a T-LESS shape -- an evaluation mesh of P = 20 000 vertices, S = 628 symmetry transformations (one
continuous and one discrete symmetry at max_sym_disc_step 0.01), n = 8 and 64 (estimate, ground truth) pairs per call -- beside the numpy restatement
(tests/bop_errors_ref.py) on the same box.  Medians, host wall clock around the blocking C call (staging and read-back included).  The device time is set
against the fp64 vector rate: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 3.93e13 fp64 instructions/s (an FMA counting once; the kernel is built without
contraction), at the 84 instructions per (symmetry, point) counted in the kernel's header.  Writes nothing: redirect into profiles/bop_errors.txt.

    python tools/bench_bop_errors.py [--reps 20] [--points 20000]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from suo_slam_amd import _lib, bop_eval  # noqa: E402
from tests import bop_errors_ref as REF  # noqa: E402
from tests.golden import bop19_cases as BC  # noqa: E402

INSTR_PER_SYM_POINT = 84
FP64_INSTR_PER_S = 256 * 4 * 16 * 2.4e9


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    P = a.points
    info = {"diameter": 200.0, "symmetries_discrete": [np.diag([1.0, -1.0, -1.0, 1.0]).ravel().tolist()], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
    pts = (rng.uniform(-1, 1, (P, 3)) * [60, 45, 80]).astype(np.float32)
    be = bop_eval.BopErrors({1: {"points": pts}}, {1: info})
    S = len(be.syms[1])
    K = np.array([[1075.65, 0, 360.0], [0, 1073.9, 270.0], [0, 0, 1]])
    print(f"suo_pose_errors_bop, P = {P}, S = {S}; numpy = tests/bop_errors_ref.py on this box's CPU")
    print(f"{'n':>4s} {'chunk':>6s} {'workgroups':>11s} {'device ms':>10s} {'pairs/s':>10s} {'fp64 bound ms':>14s} {'of bound':>9s} {'numpy ms/pair':>14s} {'numpy pairs/s':>14s} {'speed-up':>9s}")
    for n in (8, 64):
        Tg = np.stack([np.hstack((BC.random_rotation(rng), [[rng.uniform(-200, 200)], [rng.uniform(-150, 150)], [rng.uniform(600, 900)]])) for _ in range(n)])
        Te = np.stack([BC.compose(T, np.hstack((BC.rotvec(rng.standard_normal(3) * 0.05), rng.standard_normal((3, 1)) * 4))) for T in Tg])
        ids = [1] * n
        t_dev = _median_ms(lambda: be.errors(ids, Te, Tg, K), a.reps)
        mssd, mspd = be.errors(ids, Te, Tg, K)
        t0 = time.perf_counter()
        r = [REF.pose_errors(pts, Te[i], Tg[i], K, be.syms[1]) for i in range(2)]
        t_np = 1e3 * (time.perf_counter() - t0) / 2
        err = max(max(abs(mssd[i] - r[i][0]), abs(mspd[i] - r[i][1])) for i in range(2))
        tile, _, chunk = bop_eval.kernel_partition(n, P, S)
        wgs = n * -(-P // tile) * -(-S // chunk)
        bound = 1e3 * n * S * P * INSTR_PER_SYM_POINT / FP64_INSTR_PER_S
        print(f"{n:4d} {chunk:6d} {wgs:11d} {t_dev:10.3f} {1e3 * n / t_dev:10.0f} {bound:14.3f} {100 * bound / t_dev:8.1f}% {t_np:14.1f} {1e3 / t_np:14.2f} {t_np * n / t_dev:8.0f}x"
              f"   (max |device - numpy| on 2 pairs: {err:.2e})")
    be.close()


if __name__ == "__main__":
    main()
