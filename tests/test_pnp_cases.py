"""The designed PnP cases (tests/pnp_cases.py) held against the C oracle before a GPU sees them: the oracle's sequential RANSAC over a case's draw table
must return exactly the (best, winner, iterations) the case states -- itself already checked against pnp_cases.sequential_accept at import -- and the
scene must be what the script assumes: a group's quadruple has the group's consensus and nothing more, an outlier or degenerate row at most 4 inliers,
a ZERO row none.  No GPU."""
import numpy as np
import pytest

from oracle import geometry as G
from tests import pnp_cases as PC


def _count(T, xs, ys, thr=PC.THRESHOLD):
    X = xs @ T[:3, :3].T + T[:3, 3]
    with np.errstate(all="ignore"):
        e = X[:, :2] / X[:, 2:3] - ys
        return int(((1.0 / X[:, 2] >= 0) & ((e ** 2).sum(1) < thr * thr)).sum())


def test_every_family_is_present_for_both_round_sizes():
    names = [c.name for c in PC.CASES]
    assert len(set(names)) == len(names)
    for stem in ("winner_at_0", "winner_at_255", "winner_at_256", "winner_at_999", "beyond_cap_only_over_outliers", "beyond_cap_only_over_zeros",
                 "shrink_B_at_last_admitted_W256", "shrink_B_at_last_admitted_W1024", "shrink_C_at_tB_ignored_W256", "shrink_C_at_tB_ignored_W1024",
                 "shrink_C_at_tB_minus_1_accepted_W256", "shrink_C_at_tB_minus_1_accepted_W1024", "tie_same_round", "tie_next_round_W256",
                 "low_outliers_only", "low_best_4_runs_the_refinement", "low_all_zero", "degenerate_rows_before_the_winner", "behind_never_counts"):
        assert stem in names, stem
    for bound in (255, 256, 257, 511, 512, 513, 768):
        assert sum(n.startswith(f"bound_{bound}_better_at_bound_ignored") for n in names) >= 1
        assert sum(n.startswith(f"bound_{bound}_better_at_bound_minus_1_accepted") for n in names) >= 1
    for W, bound in ((256, 767), (1024, 767), (1024, 769)):
        assert sum(n.startswith(f"lane_{bound}_W{W}_winner_at_e") for n in names) == W // 64
    assert sum(n.startswith("lane_") and "_higher_past_J_" in n for n in names) >= 8


def test_sequential_accept_is_the_loop():
    tab = [1000, 1000, 1000, 10, 5, 3]
    assert PC.sequential_accept([0] * 1000, tab) == (0, -1, 1000)
    assert PC.sequential_accept([0, 3, 3, 4] + [5] * 996, tab) == (5, 4, 5)            # the tie at 2 is not accepted; 4 at index 3 sets the bound 5, index 4 is still reached
    assert PC.sequential_accept([0, 3, 3, 4, 0, 5], tab) == (4, 3, 5)                  # index 5 == the bound: never drawn
    assert PC.sequential_accept([0, 3, 3, 3, 3, 3, 3, 3, 3, 3, 5], tab) == (3, 1, 10)  # index 10 == tab[3]


@pytest.mark.parametrize("case", PC.CASES, ids=repr)
def test_oracle_agrees_with_the_case(case):
    scene, table = case.make()
    xs, ys = scene["xs"], scene["ys"]
    assert len(xs) == case.n and table.shape == (case.n_draws, 4) and (np.diff(table, axis=1) >= 0).all()
    _, best, its, win = G.pnp_with_draws(xs, ys, table, PC.THRESHOLD, refine=False)
    if case.expect is not None:
        assert (best, win, its) == tuple(case.expect)
    else:                                                          # outlier rows decide: the oracle says which, within what such rows can give
        assert best in (3, 4) and its == PC.CAP and 0 <= win < PC.CAP
        assert not isinstance(case.script.get(win, PC.OUTLIER), int) or (best == 4 and case.sizes == (4,))
    # the scene is what the script assumes, row by row (all scripted rows, a sample of the outlier rows)
    rows = sorted(case.script) + [i for i in range(0, case.n_draws, 37) if i not in case.script]
    for i in rows:
        what = case.script.get(i, PC.OUTLIER)
        c = _count(G.p4p(xs, ys, table[i]), xs, ys)
        if isinstance(what, int):
            assert c == scene["consensus"][what], (i, what, c)
        elif what == PC.ZERO:
            assert c == 0, (i, c)
        else:
            assert c <= 4, (i, what, c)
