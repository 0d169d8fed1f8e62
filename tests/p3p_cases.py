"""The P3P / P4P case table with its two yardsticks, and the comparison the device and the oracle are held to.

table        tests/golden/p3p_edge_cases.py (families B .. F, inputs) and the 400 generic problems of tests/golden/pnp_golden.npz (family A)
yardstick a  what the reference's own solver answered: tests/golden/p3p_edge_golden.npz, pnp_golden.npz
yardstick b  the mp solution set of tests/p3p_ref.py, computed once per process

analysis(family)   per case, from the inputs, the recorded answers and mp alone:
    on_edge        edge margin < 1e-9
    match[k]       the all-positive mp solution recorded candidate k lies within 1e-6 of (error rule below), or -1: `unexplained`
    err_ref[k]     its error against that solution
    missed         all-positive mp solutions no recorded candidate lies within 1e-6 of
    fourth         per all-positive mp solution: (error of point 3, z > 0); adm: those p4p may choose; gap: relative gap between the two smallest admissible errors
    ref_choice     the recorded candidate the recorded p4p pose is (nearest as rotation and translation), -1: identity
    decided        the choice among the candidates is a stable property of the input: not on an edge, every recorded candidate explained, none missed, one admissible
                   solution or gap > 1e-6, every solution's z of point 3 at least 1e-6 |t| from zero
    branch         the branches of the matrix-to-quaternion conversion the chosen pose can enter, from its mp rotation
error rule   err = max(|R - R_mp|_max, |t - t_mp|_inf / max(|t_mp|_inf, |x|_max))
gate         err_got <= 8 err_ref + 64 2^-53 for every explained candidate and for the chosen pose: the recorded answer's own error carries the conditioning of the
             case; both sides run the same fp64 operations with contraction off, so a factor 8 is slack and a wrong sign or index is orders of magnitude away."""
from __future__ import annotations

import functools
import os

import numpy as np

from oracle import geometry as G
from tests import p3p_ref as PR
from tests.golden import p3p_edge_cases as EC

HERE = os.path.dirname(os.path.abspath(__file__))
EXPLAINED = 1e-6
GAP = 1e-6
FACTOR = 8.0
FLOOR = 64 * 2.0 ** -53
FAMILIES = "ABCDEF"


def _rt_dist(R, t, R2, t2):
    d = max(np.abs(R.reshape(-1) - R2.reshape(-1)).max(), np.abs(t - t2).max() / max(np.abs(t2).max(), 1e-300))
    return np.inf if np.isnan(d) else d


def _analyse(x, y, valid, Rr, tr, T):
    s = PR.solve(x, y)
    pos = [q for q in s["sols"] if q["positive"]]
    xmax = float(np.abs(x).max())
    a = {"sol": s, "pos": pos, "margin": s["margin"], "on_edge": s["margin"] < PR.EDGE, "xmax": xmax, "valid": int(valid)}
    a["match"], a["err_ref"] = [], []
    for k in range(valid):
        errs = [PR.pose_err(Rr[k], tr[k], q, xmax) for q in pos]
        j = int(np.argmin(errs)) if errs else -1
        ok = j >= 0 and errs[j] <= EXPLAINED
        a["match"].append(j if ok else -1)
        a["err_ref"].append(errs[j] if ok else np.inf)
    a["missed"] = [j for j in range(len(pos)) if s["framed"] and j not in a["match"]]
    a["fourth"] = [PR.fourth_point(q, x[3], y[3]) for q in pos]
    adm = sorted((e, j) for j, (e, front) in enumerate(a["fourth"]) if front and e is not None)
    a["adm"] = [j for _, j in adm]
    a["gap"] = float((adm[1][0] - adm[0][0]) / adm[1][0]) if len(adm) > 1 and adm[1][0] > 0 else (1.0 if len(adm) == 1 else 0.0)
    a["ref_identity"] = bool(np.array_equal(T, np.eye(4)))
    a["ref_choice"] = -1
    if not a["ref_identity"] and valid > 0:
        a["ref_choice"] = int(np.argmin([_rt_dist(Rr[k], tr[k], T[:3, :3], T[:3, 3]) for k in range(valid)]))
    zs_ok = True
    for q in pos:
        if q["R"] is not None:
            z = sum(q["R"][2, c] * float(x[3][c]) for c in range(3)) + q["t"][2]
            zs_ok = zs_ok and abs(z) > 1e-6 * max(abs(v) for v in q["t"])
    a["decided"] = bool(not a["on_edge"] and s["framed"] and all(m >= 0 for m in a["match"]) and not a["missed"] and zs_ok
                        and np.isfinite(y[3]).all() and (len(adm) == 1 or (len(adm) > 1 and a["gap"] > GAP) or (len(adm) == 0 and a["ref_identity"])))
    a["pose_sol"] = a["match"][a["ref_choice"]] if a["ref_choice"] >= 0 else -1
    a["pose_err_ref"] = PR.pose_err(T[:3, :3], T[:3, 3], pos[a["pose_sol"]], xmax) if a["pose_sol"] >= 0 else np.inf
    a["branch"] = PR.quat_branch(pos[a["pose_sol"]]["R"]) if a["pose_sol"] >= 0 else set()
    return a


@functools.lru_cache(maxsize=None)
def designed():
    """The designed cases: table, xs [n,4,3], ys [n,4,2], the recorded answers and the analysis of every case."""
    table = EC.cases()
    xs, ys = EC.arrays(table)
    g = np.load(os.path.join(HERE, "golden", "p3p_edge_golden.npz"))
    gold = {"valid": g["valid"], "R": g["R"], "t": g["t"], "T": g["T"]}
    assert len(gold["valid"]) == len(table), "tests/golden/p3p_edge_golden.npz is not of this table: run tests/golden/make_p3p_edge_golden.py"
    info = [_analyse(xs[i], ys[i], gold["valid"][i], gold["R"][i], gold["t"][i], gold["T"][i]) for i in range(len(table))]
    fam = np.array([c["family"] for c in table])
    return {"table": table, "family": fam, "xs": xs, "ys": ys, "gold": gold, "info": info}


@functools.lru_cache(maxsize=None)
def generic():
    """Family A in the same form."""
    g = np.load(os.path.join(HERE, "golden", "pnp_golden.npz"))
    xs, ys = g["xs"], g["ys"]
    gold = {"valid": g["p3p_valid"], "R": g["p3p_R"], "t": g["p3p_t"], "T": g["p4p_T"]}
    info = [_analyse(xs[i], ys[i], gold["valid"][i], gold["R"][i], gold["t"][i], gold["T"][i]) for i in range(len(xs))]
    table = [{"family": "A", "name": f"generic {i}"} for i in range(len(xs))]
    return {"table": table, "family": np.array(["A"] * len(xs)), "xs": xs, "ys": ys, "gold": gold, "info": info}


def run_oracle(xs, ys, L=None):
    """The C oracle (or another library with its orc_p3p / orc_p4p) in the layout of suo_debug_p3p: valid, R, t, qt, status."""
    L = G.lib() if L is None else L
    n = len(xs)
    valid, R, t, qt, status = np.zeros(n, np.int32), np.zeros((n, 4, 9)), np.zeros((n, 4, 3)), np.zeros((n, 7)), np.zeros(n, np.int32)
    idx = np.arange(4, dtype=np.int32)
    for i in range(n):
        x, y = np.ascontiguousarray(xs[i]), np.ascontiguousarray(ys[i])
        yh = np.ascontiguousarray(np.c_[y[:3], np.ones(3)])
        r, tt = np.zeros(36), np.zeros(12)
        v = L.orc_p3p(yh[0].copy(), yh[1].copy(), yh[2].copy(), x[0].copy(), x[1].copy(), x[2].copy(), r, tt)
        valid[i] = v
        R[i, :v], t[i, :v] = r.reshape(4, 9)[:v], tt.reshape(4, 3)[:v]
        q, tq = np.zeros(4), np.zeros(3)
        L.orc_p4p(x, y, idx, q, tq)
        qt[i] = np.r_[q, tq]
        status[i] = int(np.array_equal(qt[i], [1, 0, 0, 0, 0, 0, 0]))
    return valid, R, t, qt, status


def pose_of(qt):
    return G.quat_to_rot(qt[:4]), qt[4:7]          # (the kernel's quat_to_rot, operation for operation)


def compare(D, valid, R, t, qt, status, ties=()):
    """Hold one implementation's answers on the cases of D (designed() or generic()) to the count, candidate and chosen-pose rules of tests/test_gpu_p3p.py.
    ties: case indices whose choice is asserted although the mp gap is zero (an exact tie of the fp64 errors: the first candidate wins).
    Returns (failures: list of strings, stats: dict)."""
    fails = []
    ratios, n_cand, n_ident_cases, n_pose, n_choice = [], 0, 0, 0, 0
    for i, (c, a) in enumerate(zip(D["table"], D["info"])):
        who = f"case {i} [{c['family']}] {c['name']}"
        gv, gR, gt, gT = D["gold"]["valid"][i], D["gold"]["R"][i], D["gold"]["t"][i], D["gold"]["T"][i]
        v = int(valid[i])
        if not 0 <= v <= 4:
            fails.append(f"{who}: valid = {v}")
            continue
        if not a["on_edge"] and v != gv:
            fails.append(f"{who}: valid = {v}, the reference has {gv}")
            continue
        if np.any(R[i, v:] != 0) or np.any(t[i, v:] != 0):
            fails.append(f"{who}: candidates beyond valid are not zero")
        n_ident_cases += int(v == gv and np.array_equal(R[i], gR, equal_nan=True) and np.array_equal(t[i], gt, equal_nan=True))
        if v == gv:
            for k in range(v):
                if a["match"][k] < 0:
                    if not np.array_equal(np.isfinite(np.r_[R[i, k], t[i, k]]), np.isfinite(np.r_[gR[k], gt[k]])):
                        fails.append(f"{who}: unexplained candidate {k}: finiteness pattern differs from the reference's")
                    continue
                e = PR.pose_err(R[i, k], t[i, k], a["pos"][a["match"][k]], a["xmax"])
                n_cand += 1
                ratios.append(e / max(a["err_ref"][k], 2.0 ** -53))
                if not e <= FACTOR * a["err_ref"][k] + FLOOR:
                    fails.append(f"{who}: candidate {k}: err {e:.3e}, the reference's {a['err_ref'][k]:.3e}")
        # the chosen pose
        if not np.isfinite(qt[i]).all():
            fails.append(f"{who}: qt is not finite")
            continue
        ident = bool(np.array_equal(qt[i], [1, 0, 0, 0, 0, 0, 0]))
        if ident != bool(status[i]):
            fails.append(f"{who}: status {status[i]} but qt {'is' if ident else 'is not'} the identity")
        if a["on_edge"] and v != gv:
            continue
        if ident != a["ref_identity"]:
            fails.append(f"{who}: identity {ident}, the reference {a['ref_identity']}")
            continue
        if ident:
            continue
        Rq, tq = pose_of(qt[i])
        choice = int(np.argmin([_rt_dist(R[i, k], t[i, k], Rq, tq) for k in range(v)]))
        if a["decided"] or i in ties:
            n_choice += 1
            if choice != a["ref_choice"]:
                fails.append(f"{who}: p4p chose candidate {choice}, the reference candidate {a['ref_choice']}")
                continue
        if choice == a["ref_choice"] and a["pose_sol"] >= 0:
            e = PR.pose_err(Rq, tq, a["pos"][a["pose_sol"]], a["xmax"])
            n_pose += 1
            ratios.append(e / max(a["pose_err_ref"], 2.0 ** -53))
            if not e <= FACTOR * a["pose_err_ref"] + FLOOR:
                fails.append(f"{who}: chosen pose: err {e:.3e}, the reference's {a['pose_err_ref']:.3e}")
    stats = {"max_ratio": max(ratios) if ratios else 0.0, "candidates": n_cand, "poses": n_pose, "choices": n_choice, "bit_identical_cases": n_ident_cases,
             "cases": len(D["table"])}
    return fails, stats


def tie_cases(D):
    """The designed tie cases whose fourth-point errors, evaluated in doubles on the RECORDED candidates, are all equal: there the choice is the first-wins rule's."""
    out = []
    for i, c in enumerate(D["table"]):
        if c["name"].startswith("exact tie"):
            v = D["gold"]["valid"][i]
            e = p4p_errors(D["gold"]["R"][i][:v], D["gold"]["t"][i][:v], D["xs"][i][3], D["ys"][i][3])
            if v >= 2 and None not in e and len(set(e)) == 1:
                out.append(i)
    return tuple(out)


def p4p_errors(Rs, ts, x3, y3):
    """The fourth-point errors p4p computes for candidates (Rs [v][9], ts [v][3]) in doubles, step by step as p4p.cpp:25-56 states them: matrix -> unit quaternion
    -> matrix, project point 3, squared distance; None where the candidate is skipped (z < 0).  Used to establish that a tie case ties in doubles."""
    out = []
    for Rm, tv in zip(Rs, ts):
        Rm = Rm.reshape(3, 3)
        tr = Rm[0, 0] + Rm[1, 1] + Rm[2, 2] + 1.0
        assert tr > 1e-7, "p4p_errors covers the trace branch only"
        S = 0.5 / np.sqrt(tr)
        q = np.array([0.25 / S, (Rm[2, 1] - Rm[1, 2]) * S, (Rm[0, 2] - Rm[2, 0]) * S, (Rm[1, 0] - Rm[0, 1]) * S])
        q = q * (1.0 / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
        Rq = G.quat_to_rot(q)
        xr = np.array([Rq[r, 0] * x3[0] + Rq[r, 1] * x3[1] + Rq[r, 2] * x3[2] + tv[r] for r in range(3)])
        if xr[2] < 0:
            out.append(None)
            continue
        iz = 1.0 / xr[2]
        ex, ey = xr[0] * iz - y3[0], xr[1] * iz - y3[1]
        out.append(ex * ex + ey * ey)
    return out
