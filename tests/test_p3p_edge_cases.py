"""The P3P / P4P case table (tests/golden/p3p_edge_cases.py, tests/p3p_cases.py) judged WITHOUT a GPU: the oracle is pinned to the recorded reference on it bit for
bit, the table reaches the branches it was designed for, and the conditions under which tests/test_gpu_p3p.py may leave something out hold on the reference alone.

What a GPU case may leave out, and the cap on it:
    on an edge      edge margin < 1e-9 (tests/p3p_ref.py): the count is compared loosely.  At most 5 % of the designed cases, from families C and D only, none in A.
    unexplained     a recorded candidate within 1e-6 of no all-positive mp solution (the reference's own not-quite-rotations: Lambda-Twist clamps a negative
                    discriminant to zero and refines what comes out): only its finiteness pattern is compared.  At most 2 % of all recorded candidates.
    missed          off the edges, with a model frame that exists, the reference misses no all-positive mp solution.
Each fourth-point rule of family F is shown to fire from the recorded answers and the mp data."""
import collections

import numpy as np
import pytest

from oracle import geometry as G
from tests import p3p_cases as PC
from tests import p3p_ref as PR


@pytest.fixture(scope="module")
def designed():
    return PC.designed()


@pytest.fixture(scope="module")
def generic():
    return PC.generic()


def _chosen_trace(a):
    R = a["pos"][a["pose_sol"]]["R"]
    return float(R[0, 0] + R[1, 1] + R[2, 2] + 1)


def test_oracle_reproduces_the_recorded_reference_bit_for_bit(designed):
    D, g = designed, designed["gold"]
    valid, R, t, qt, status = PC.run_oracle(D["xs"], D["ys"])
    live = G.ref() is not None
    for i, c in enumerate(D["table"]):
        who = (i, c["family"], c["name"])
        assert valid[i] == g["valid"][i], who
        assert np.array_equal(R[i], g["R"][i], equal_nan=True) and np.array_equal(t[i], g["t"][i], equal_nan=True), who
        T = G.p4p(D["xs"][i], D["ys"][i], [0, 1, 2, 3])
        assert np.array_equal(T, g["T"][i]), who
        assert np.array_equal(T[:3, :3], PC.pose_of(qt[i])[0]) and np.array_equal(T[:3, 3], qt[i, 4:]) and status[i] == int(np.array_equal(T, np.eye(4))), who
        if live:
            assert np.array_equal(T, G.ref_p4p(D["xs"][i], D["ys"][i], [0, 1, 2, 3])), who


def test_table_and_caps_summary(designed, generic, capsys):
    """Prints, per family, the cases, the counts by `valid`, the branch tallies, the on-edge and the unexplained share; asserts the caps."""
    rows = []
    n_edge_designed = n_unexpl = n_cand = 0
    for D in (generic, designed):
        for f in sorted(set(D["family"])):
            idx = np.flatnonzero(D["family"] == f)
            info = [D["info"][i] for i in idx]
            counts = np.bincount(D["gold"]["valid"][idx], minlength=5)
            br = collections.Counter("trace" if a["branch"] == {0} else "".join(str(b) for b in sorted(a["branch"])) for a in info if a["branch"])
            edge = sum(a["on_edge"] for a in info)
            un = sum(m < 0 for a in info for m in a["match"])
            cand = sum(len(a["match"]) for a in info)
            missed = sum(bool(a["missed"]) and not a["on_edge"] for a in info)
            rows.append(f"family {f}: {len(idx)} cases, valid 0..4 = {counts.tolist()}, on an edge {edge}, unexplained {un} of {cand} candidates, missed {missed}, "
                        f"decided {sum(a['decided'] for a in info)}, branch of the chosen pose {dict(sorted(br.items()))}")
            n_unexpl += un
            n_cand += cand
            if f == "A":
                assert edge == 0, "a generic problem is on an edge"
            else:
                n_edge_designed += edge
                assert edge == 0 or f in "CD", f
            assert missed == 0, f
    n_designed = len(designed["table"])
    rows.append(f"on an edge: {n_edge_designed} of {n_designed} designed cases = {100 * n_edge_designed / n_designed:.2f} % (cap 5 %); unexplained: {n_unexpl} of {n_cand} "
                f"recorded candidates = {100 * n_unexpl / n_cand:.2f} % (cap 2 %)")
    with capsys.disabled():
        print("\n" + "\n".join(rows))
    assert 200 <= n_designed <= 400
    assert n_edge_designed <= 0.05 * n_designed
    assert n_unexpl <= 0.02 * n_cand


def test_reference_chooses_the_mp_best_where_the_choice_is_decided(designed, generic):
    """The second yardstick agrees with the first on which candidate wins, wherever the test will insist on it."""
    for D in (designed, generic):
        n = 0
        for i, a in enumerate(D["info"]):
            if a["decided"]:
                n += 1
                if a["adm"]:
                    assert not a["ref_identity"] and a["match"][a["ref_choice"]] == a["adm"][0], (i, D["table"][i]["name"])
                else:
                    assert a["ref_identity"], (i, D["table"][i]["name"])
        assert n >= 0.85 * len(D["info"])


def test_table_reaches_every_candidate_count(designed):
    counts = np.bincount(designed["gold"]["valid"], minlength=5)
    for v in (0, 1, 2, 4):
        assert counts[v] >= 5, (v, counts)
    stable = [a["valid"] for a in designed["info"] if not a["on_edge"] and a["sol"]["framed"] and all(m >= 0 for m in a["match"])]
    assert {1, 2, 3, 4} <= set(stable)                   # counts that are stable properties of their input, three among them


def test_table_enters_every_quaternion_branch_and_both_sides_of_the_switch(designed):
    D = designed
    certain = collections.Counter()
    ties = collections.Counter()
    for a in D["info"]:
        if a["pose_sol"] < 0:
            continue
        if len(a["branch"]) == 1:
            certain[next(iter(a["branch"]))] += 1
        else:
            ties[tuple(sorted(a["branch"]))] += 1
    for b in (0, 1, 2, 3):
        assert certain[b] >= 5, (b, certain)
    for pair in ((1, 2), (1, 3), (2, 3), (1, 2, 3)):      # the tied diagonals: either order of the strict comparisons
        assert ties[pair] >= 5, (pair, ties)
    tr = np.array([_chosen_trace(a) for a, f in zip(D["info"], D["family"]) if f == "B" and a["pose_sol"] >= 0])
    assert ((tr > 1e-8) & (tr < 1e-7)).sum() >= 5 and ((tr > 1e-7) & (tr < 1e-6)).sum() >= 5          # delta 2e-4 and 4e-4: 4e-8 and 1.6e-7
    assert (np.abs(tr) < 1e-11).sum() >= 5 and (tr > 1e-5).sum() >= 5
    # a slip in a non-trace branch shows only where the entries it reads are not zero: the axes with one dominant component, at a delta the bound resolves
    for b in (1, 2, 3):
        n = 0
        for a, f in zip(D["info"], D["family"]):
            if f == "B" and a["pose_sol"] >= 0 and a["branch"] == {b}:
                R = np.array([[float(a["pos"][a["pose_sol"]]["R"][r, c]) for c in range(3)] for r in range(3)])
                off = [abs(R[r, c] + R[c, r]) for r in range(3) for c in range(r)]
                skew = [abs(R[r, c] - R[c, r]) for r in range(3) for c in range(r)]
                n += int(min(off) > 0.1 and min(skew) > 1e-7)
        assert n >= 2, (b, n)


def test_table_takes_every_entry_branch_of_the_cubic(designed, generic):
    for D in (designed, generic):
        got = collections.Counter(PR.cubic_branch(a["sol"]["coeffs"]) for a in D["info"] if a["sol"]["coeffs"] is not None)
        for b in ("monotone", "two-extrema-left", "two-extrema-right"):
            assert got[b] >= 5, (b, got)


def test_every_fourth_point_rule_fires(designed):
    D = designed
    fired = collections.Counter()
    for i, (c, a) in enumerate(zip(D["table"], D["info"])):
        errs = [e for e, _ in a["fourth"]]
        if c["family"] == "F" and a["decided"] and not a["ref_identity"]:
            chosen = a["match"][a["ref_choice"]]
            if any((not front) and e is not None and e < errs[chosen] for e, front in a["fourth"]):
                fired["a better candidate skipped for z < 0"] += 1
            if min(e for e in errs if e is not None) > 1:
                fired["a grossly wrong point still chooses"] += 1
            if 1e-6 < a["gap"] < 1e-2:
                fired["close errors decided by strict <"] += 1
        if c["family"] == "F" and a["ref_identity"] and a["valid"] > 0 and a["fourth"] and not any(front for _, front in a["fourth"]):
            fired["every candidate behind: identity"] += 1
        if a["ref_identity"] and a["valid"] > 0 and np.isnan(D["ys"][i][3]).any():
            fired["NaN error: identity"] += 1
        if i in PC.tie_cases(D) and a["ref_choice"] == 0:
            fired["exact tie: the first wins"] += 1
    print(dict(fired))
    for rule in ("a better candidate skipped for z < 0", "a grossly wrong point still chooses", "close errors decided by strict <", "every candidate behind: identity",
                 "NaN error: identity", "exact tie: the first wins"):
        assert fired[rule] >= 2, (rule, fired)


def test_oracle_passes_the_gates_the_device_is_held_to(designed, generic):
    """tests/test_gpu_p3p.py's comparison, run on the oracle: the gates are satisfiable and the comparison code itself runs without a GPU."""
    for D in (designed, generic):
        fails, stats = PC.compare(D, *PC.run_oracle(D["xs"], D["ys"]), ties=PC.tie_cases(D))
        print(stats)
        assert not fails, fails[:5]
        assert stats["bit_identical_cases"] == stats["cases"] and stats["max_ratio"] <= 1.0


def test_comparison_catches_planted_slips(designed):
    """The comparison is not vacuous: a sign flipped in one candidate entry, the second-best candidate returned, a count off by one -- each is reported."""
    D = designed
    base = PC.run_oracle(D["xs"], D["ys"])
    i = next(k for k, (c, a) in enumerate(zip(D["table"], D["info"])) if "about X, delta 0.0002" in c["name"] and a["decided"] and a["valid"] == 2 and a["branch"] == {1})
    valid, R, t, qt, status = [v.copy() for v in base]
    R[i, 0, 1] = -R[i, 0, 1]
    assert any(f.startswith(f"case {i} ") and "candidate 0" in f for f in PC.compare(D, valid, R, t, qt, status)[0])
    valid, R, t, qt, status = [v.copy() for v in base]
    other = 1 - D["info"][i]["ref_choice"]
    Rq = R[i, other].reshape(3, 3)
    w = 0.5 * np.sqrt(max(1 + Rq[0, 0] + Rq[1, 1] + Rq[2, 2], 0))
    x = 0.5 * np.sqrt(max(1 + Rq[0, 0] - Rq[1, 1] - Rq[2, 2], 0))
    q = np.array([w, x, (Rq[0, 1] + Rq[1, 0]) / (4 * x), (Rq[0, 2] + Rq[2, 0]) / (4 * x)]) if x > 0.1 else np.array([w, (Rq[2, 1] - Rq[1, 2]) / (4 * w),
                                                                                                                (Rq[0, 2] - Rq[2, 0]) / (4 * w), (Rq[1, 0] - Rq[0, 1]) / (4 * w)])
    qt[i] = np.r_[q / np.linalg.norm(q), t[i, other]]
    assert any(f.startswith(f"case {i} ") and "chose candidate" in f for f in PC.compare(D, valid, R, t, qt, status)[0])
    valid, R, t, qt, status = [v.copy() for v in base]
    valid[i] = 1
    R[i, 1:] = 0
    t[i, 1:] = 0
    assert any(f.startswith(f"case {i} ") and "valid = 1" in f for f in PC.compare(D, valid, R, t, qt, status)[0])
    for k in PC.tie_cases(D):                                  # `<=` for `<`: the last of the tied candidates
        valid, R, t, qt, status = [v.copy() for v in base]
        Rq = R[k, 1].reshape(3, 3)
        w = 0.5 * np.sqrt(1 + Rq[0, 0] + Rq[1, 1] + Rq[2, 2])
        qt[k] = np.r_[w, (Rq[2, 1] - Rq[1, 2]) / (4 * w), (Rq[0, 2] - Rq[2, 0]) / (4 * w), (Rq[1, 0] - Rq[0, 1]) / (4 * w), t[k, 1]]
        assert any(f.startswith(f"case {k} ") and "chose candidate" in f for f in PC.compare(D, valid, R, t, qt, status, ties=PC.tie_cases(D))[0])


def _quat_branches(text):
    """The three non-trace branches of rot_to_quat as they stand in a source text, white space squeezed."""
    import re
    m = re.search(r"\} else if \(R\[0\] > R\[4\] && R\[0\] > R\[8\]\) \{.*?q\[3\] = 0\.25 \* S;\n    \}", text, re.S)
    assert m, "rot_to_quat's non-trace branches not found"
    return re.sub(r"\s+", " ", m.group(0))


def test_mutants_of_the_choice_and_conversion_code_fail_the_comparison(designed, tmp_path):
    """The kernel's rot_to_quat and the oracle's are the same text in the three non-trace branches, and their outputs are bit-identical on this table
    (tests/test_gpu_p3p.py), so what the comparison says of a mutated ORACLE it says of the kernel mutated the same way -- no mutated kernel needs a GPU.  Mutants:
    every sign of the nine off-diagonal quaternion terms of those branches, one index per branch, `xr[2] < 0` reversed, `e < e0` -> `e <= e0`.  Each must fail."""
    import ctypes
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "oracle", "pnp_oracle.c")).read()
    hip = open(os.path.join(root, "suo_slam_amd", "csrc", "pnp.hip")).read()
    assert _quat_branches(src) == _quat_branches(hip)
    for text in ("if (xr[2] < 0) continue;", "if (e < e0) {"):
        assert src.count(text) == 1 and hip.count(text) == 1, text
    block = re.search(r"\} else if \(R\[0\] > R\[4\] && R\[0\] > R\[8\]\) \{.*?q\[3\] = 0\.25 \* S;\n    \}", src, re.S)
    mutants = []
    for m in re.finditer(r"\(R\[\d\] ([+-]) R\[\d\]\) / S", block.group(0)):
        at = block.start() + m.start(1)
        mutants.append((f"sign at {m.group(0)!r}", src[:at] + ("-" if m.group(1) == "+" else "+") + src[at + 1:]))
    assert len(mutants) == 9
    for m in list(re.finditer(r"q\[0\] = \(R\[(\d)\]", block.group(0))):
        at = block.start() + m.start(1)
        mutants.append((f"index at {m.group(0)!r}", src[:at] + str((int(m.group(1)) + 1) % 9) + src[at + 1:]))
    mutants.append(("xr[2] < 0 reversed", src.replace("if (xr[2] < 0) continue;", "if (xr[2] > 0) continue;")))
    mutants.append(("e <= e0", src.replace("if (e < e0) {", "if (e <= e0) {")))
    keep = [i for i, f in enumerate(designed["family"]) if f in "BF"]
    sub = {"table": [designed["table"][i] for i in keep], "info": [designed["info"][i] for i in keep], "gold": {k: v[keep] for k, v in designed["gold"].items()},
           "xs": designed["xs"][keep], "ys": designed["ys"][keep], "family": designed["family"][keep]}
    dp, ip = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    caught = {}
    for k, (name, text) in enumerate([("unchanged", src)] + mutants):
        c, so = tmp_path / f"m{k}.c", tmp_path / f"m{k}.so"
        c.write_text(text)
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=c99", "-ffp-contract=off", "-w", "-shared", "-o", str(so), str(c), "-lm"])
        L = ctypes.CDLL(str(so))
        L.orc_p3p.restype, L.orc_p3p.argtypes = ctypes.c_int, [dp] * 8
        L.orc_p4p.restype, L.orc_p4p.argtypes = None, [dp, dp, ip, dp, dp]
        fails, _ = PC.compare(sub, *PC.run_oracle(sub["xs"], sub["ys"], L), ties=PC.tie_cases(sub))
        caught[f"{k} {name}"] = len(fails)
    print(caught)
    assert caught.pop("0 unchanged") == 0 and len(caught) == 14
    assert all(n >= 2 for n in caught.values()), caught
