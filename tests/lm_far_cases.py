"""Far starts for every LM route: the smallest graph of tests/ba_route_cases.py per route, its free vertices started 0.05 rad / 0.3 rad (and 30 mm) from the truth, so
that the first updates lie in the Taylor range / the closed forms of pose_oplus (csrc/lm_device.h) -- the near starts of the route table never leave its shortcut.

A case is compared with the C oracle after ONE and TWO LM iterations only (longer trajectories from a far start part legitimately at accept / reject decisions), and
only if the oracle ALONE says the comparison is well posed (admit()):
  1. every edge's chi2 after the run is further than 1e-6 relative from the inlier threshold;
  2. the oracle run on the same graph with its edges in reverse order gives poses within 1e-9, chi2 within 1e-7 relative and the same flags -- 1000 x inside the
     gates of tests/test_gpu_geometry.py: _compare_ba, so no gate is decided by the reference's own summation order;
  3. the first step (the oracle's its=(1,) run, one trial, accepted) turns every free vertex by an angle in (1e-3, 0.3) at the low level, and at least half of
     them by more than 0.3 at the high level.
The seed of each case was chosen on the CPU so that all three hold (SEEDS; tests/test_lm_far_cases.py checks them again on every run, and the GPU test before it
looks at a kernel's result).  REJECT: per family, a start 0.6 rad out from which the oracle rejects a trial after a large step, with conditions 1 and 2 and the
high level's condition 3.

build_recovery(): noise-free graphs (edge_uv overwritten by the exact float64 projection of the truth) started 0.1 / 0.3 rad out; 40 iterations must return the truth."""
from __future__ import annotations

import zlib

import numpy as np

from oracle import geometry as G
from tests import ba_route_cases as RC

CHI2_THR = G.CHI2_THR
LEVELS = {"low": (0.05, 30.0), "high": (0.3, 30.0)}
ITS = ((1,), (2,))


def _mixed16(r, p):
    return [RC.frame(r, [20] * 12, perturb=p), RC.frame(r, [300, 20, 20, 20, 20], perturb=p)]


BUILDERS = {
    "FRAME2": lambda r, p: [RC.frame(r, [20] * 6, perturb=p)],
    "FRAME8": lambda r, p: [RC.frame(r, [257, 60, 40], perturb=p)],
    "FRAME16": _mixed16,
    "CAM2": lambda r, p: [RC.tracking(r, [12] * 5, perturb=p)],
    "CAM": lambda r, p: [RC.tracking(r, [12] * 5, n_fixed_cams=1, perturb=p)],
    "LM": lambda r, p: [RC.global_graph(r, 40, 3, 2, miss=0.0, perturb=p)],
    "LM_BIG": lambda r, p: [RC.frame(r, [129] + [50] * 8, perturb=p)],                    # 529 edges: the largest graph here
    "PHASES": lambda r, p: [RC.global_graph(r, 512, 8, 6, perturb=p)],
    "PHASEWISE": lambda r, p: [RC.global_graph(r, 300, 5, 17, perturb=p)],
}
ROUTES = list(BUILDERS)

# (route, level) -> seed offset, chosen on the CPU: the first of 0, 1, 2, ... at which admit() holds for its=(1,) and its=(2,)
SEEDS = {(route, level): 0 for route in BUILDERS for level in LEVELS}          # (offset 0 is admitted on every route at both levels)

# family -> (seed offset, its): the first of 200 offsets at which the oracle rejects a trial from 0.6 rad out (stats[2] > stats[1]) and the case is admitted.  With no
# free object (one free camera) none of the 200 is: wherever the oracle rejects a trial there, the step it accepts first is below 0.08 rad.
REJECT_PERTURB = (0.6, 30.0)
REJECT_BUILDERS = {
    "no_free_camera": lambda r, p: [RC.frame(r, [20] * 6, perturb=p)],
    "no_free_object": lambda r, p: [RC.tracking(r, [12] * 5, perturb=p)],
    "both_free": lambda r, p: [RC.global_graph(r, 200, 5, 4, miss=0.0, perturb=p)],
}
REJECT = {"no_free_camera": (32, (2,)), "both_free": (36, (2,))}


def build(route, level, seed=None):
    seed = SEEDS[(route, level)] if seed is None else seed
    rng = np.random.default_rng(zlib.crc32(f"far/{route}/{level}".encode()) + seed)
    return BUILDERS[route](rng, LEVELS[level])


def build_reject(family, seed=None):
    seed = REJECT[family][0] if seed is None else seed
    rng = np.random.default_rng(zlib.crc32(f"reject/{family}".encode()) + seed)
    return REJECT_BUILDERS[family](rng, REJECT_PERTURB)


def args(P):
    return [P[k] for k in RC.KEYS]


def reversed_edges(P):
    Q = dict(P)
    for k in ("edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier"):
        Q[k] = np.ascontiguousarray(P[k][::-1])
    return Q


def turn_angles(T0, T1):
    """Angle of R1 R0^T per pose."""
    R = np.einsum("nij,nkj->nik", np.asarray(T1)[:, :, :3], np.asarray(T0)[:, :, :3])
    c = (np.trace(R, axis1=1, axis2=2) - 1) / 2
    s = 0.5 * np.sqrt((R[:, 2, 1] - R[:, 1, 2]) ** 2 + (R[:, 0, 2] - R[:, 2, 0]) ** 2 + (R[:, 1, 0] - R[:, 0, 1]) ** 2)
    return np.arctan2(s, c)


def first_step_angles(P, ref1):
    """The turn of every free vertex between the start and the oracle's result `ref1`."""
    cf, of = ~P["cam_fixed"].astype(bool), ~P["obj_fixed"].astype(bool)
    return np.r_[turn_angles(P["cam_T"][cf], ref1[0][cf]), turn_angles(P["obj_T"][of], ref1[1][of])]


def admit(P, its, level, need_single_trial=True):
    """(ok, why, info) from the oracle alone; info carries its result `ref` and the first-step angles."""
    kw = dict(its=its, init_with_outliers=True)
    ref = G.optimize(*args(P), **kw)
    info = {"ref": ref}
    if not all(np.isfinite(a).all() for a in (ref[0], ref[1], ref[3])) or ref[4][0] < 1 or ref[4][1] < 1:
        return False, f"the oracle did not run: stats {ref[4]}", info
    margin = np.abs(ref[3] - CHI2_THR).min() / CHI2_THR
    info["margin"] = float(margin)
    if not margin > 1e-6:
        return False, f"an edge's chi2 lies {margin:.1e} relative from the threshold", info
    rev = G.optimize(*args(reversed_edges(P)), **kw)
    dpose = max(np.abs(rev[0] - ref[0]).max(), np.abs(rev[1] - ref[1]).max())
    dchi = (np.abs(rev[3][::-1] - ref[3]) / (np.abs(ref[3]) + 1e-3)).max()             # (_compare_ba: rtol 1e-4 + atol 1e-7; here 1e-7 of |chi2| + 1e-3)
    info["reorder"] = (float(dpose), float(dchi))
    if not (dpose <= 1e-9 and dchi <= 1e-7 and np.array_equal(rev[2][::-1], ref[2])):
        return False, f"unstable under edge reordering: poses {dpose:.1e}, chi2 {dchi:.1e}", info
    one = ref if tuple(its) == (1,) else G.optimize(*args(P), its=(1,), init_with_outliers=True)
    if need_single_trial and one[4][2] != 1:
        return False, f"the first trial was rejected: stats {one[4]}", info
    ang = first_step_angles(P, one)
    info["angles"] = ang
    if level == "low" and not ((ang > 1e-3) & (ang < 0.3)).all():
        return False, f"first-step angles {np.round(ang, 3).tolist()} leave (1e-3, 0.3)", info
    if level == "high" and not (ang > 0.3).sum() * 2 >= len(ang):
        return False, f"first-step angles {np.round(ang, 3).tolist()}: fewer than half above 0.3", info
    return True, "", info


# ---- recovery of the truth ----------------------------------------------------------------------------------------------------------------------------------

RECOVERY_BUILDERS = {
    "FRAME2": lambda r, p: RC.frame(r, [20] * 6, perturb=p),
    "CAM2": lambda r, p: RC.tracking(r, [12] * 5, perturb=p),
    "LM": lambda r, p: RC.global_graph(r, 200, 5, 4, miss=0.0, perturb=p),
    "PHASES": lambda r, p: RC.global_graph(r, 512, 8, 6, miss=0.0, perturb=p),
}
RECOVERY_ROT = (0.1, 0.3)
RECOVERY_KW = dict(its=(40,), init_with_outliers=True)
RECOVERY_SEEDS = {(route, rot): 0 for route in RECOVERY_BUILDERS for rot in RECOVERY_ROT}
RECOVERY_SEEDS[("PHASES", 0.3)] = 1            # (from offset 0 the oracle itself ends in a local minimum, 25 edges gated out)


def exact_projection(P):
    """edge_uv of the truth's poses, float64."""
    Tc, To = P["cam_gt"][P["edge_cam"]], P["obj_gt"][P["edge_obj"]]
    pw = np.einsum("eij,ej->ei", To[:, :, :3], P["edge_p"]) + To[:, :, 3]
    pc = np.einsum("eij,ej->ei", Tc[:, :, :3], pw) + Tc[:, :, 3]
    k = P["edge_camk"]
    return np.stack([k[:, 0] * pc[:, 0] / pc[:, 2] + k[:, 2], k[:, 1] * pc[:, 1] / pc[:, 2] + k[:, 3]], -1)


def build_recovery(route, rot, seed=None):
    seed = RECOVERY_SEEDS[(route, rot)] if seed is None else seed
    rng = np.random.default_rng(zlib.crc32(f"recover/{route}/{rot}".encode()) + seed)
    P = RECOVERY_BUILDERS[route](rng, (rot, 30.0))
    P["edge_uv"] = exact_projection(P)                                 # noise and outliers gone: every measurement is the truth's
    return P


def truth_distance(P, res):
    """(max |dR|_F, max |dt| / max(1, |t|)) of a result's poses from the truth."""
    dR = dt = 0.0
    for got, gt in ((res[0], P["cam_gt"]), (res[1], P["obj_gt"])):
        for a, b in zip(got, gt):
            dR = max(dR, float(np.linalg.norm(a[:, :3] - b[:, :3])))
            dt = max(dt, float(np.linalg.norm(a[:, 3] - b[:, 3]) / max(1.0, np.linalg.norm(b[:, 3]))))
    return dR, dt


def admit_recovery(P):
    ref = G.optimize(*args(P), **RECOVERY_KW)
    dR, dt = truth_distance(P, ref)
    ok = dR <= 1e-9 and dt <= 1e-9 and bool(ref[2].all())
    return ok, f"the oracle ends {dR:.1e} / {dt:.1e} from the truth, {int((ref[2] == 0).sum())} outliers, stats {ref[4]}", ref
