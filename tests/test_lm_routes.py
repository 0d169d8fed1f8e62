"""Which kernel suo_optimize_batch runs each bundle-adjustment graph on, at every threshold of its dispatcher, on both sides of each threshold
(suo_debug_lm_routes: the dispatcher's own decision, evaluated on the host; no GPU needed).  The cases live in tests/ba_route_cases.py, where
tests/test_gpu_lm_routes.py runs each of them on its route against the C oracle."""
import numpy as np
import pytest

from tests import ba_route_cases as RC


@pytest.fixture(scope="module")
def built():
    from suo_slam_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def table(built):
    out = {}
    for case in RC.CASES:
        out[case.name] = RC.routes_of(case.problems(), its=case.its)
    return out


@pytest.mark.parametrize("name", RC.CASE_IDS)
def test_route_of_each_case(table, name):
    routes, need = table[name]
    assert routes == RC.BY_NAME[name].routes, (name, routes, need)
    for r, n in zip(routes, need):
        assert (n > 0) if r in ("LM", "LM_BIG") else (n == -1), (r, n)


def test_frame2_per_object_cap_and_edge_budget_are_exact(built):
    """The cap is 32 edges per lane (the lane's outlier flags live in a 32-bit mask, csrc/lm_frame2.hip): 8 lanes (256 edges) per object up to 8 objects,
    4 lanes (128) with 9-16; the frame's edges fit LF2_MAX_EDGES = 656.  One edge more on either side leaves lm_frame2_kernel."""
    rng = np.random.default_rng(5)
    for n_obj, cap in ((1, 256), (8, 256), (9, 128), (16, 128)):
        rest = max(0, min(20, (656 - cap - 1) // max(n_obj - 1, 1)))
        at = RC.frame(rng, [cap] + [rest] * (n_obj - 1))
        over = RC.frame(rng, [cap + 1] + [rest] * (n_obj - 1))
        assert RC.routes_of([at])[0] == ["FRAME2"], (n_obj, cap)
        r_over = RC.routes_of([over])[0][0]
        assert r_over != "FRAME2", (n_obj, cap)
        assert r_over == ("FRAME8" if n_obj <= 8 else ("LM" if len(over["edge_cam"]) < 512 else "LM_BIG")), (n_obj, r_over)


def test_big_graph_members_of_a_batch_run_alone_on_their_own_routes(built):
    """A batch holding a > 16-free-object graph runs its other problems one by one: each gets the route it takes alone, PHASES included."""
    rng = np.random.default_rng(6)
    big = RC.global_graph(rng, 300, 4, 18)
    g600 = RC.global_graph(rng, 600, 10, 6)
    small = RC.global_graph(rng, 200, 5, 4)
    routes, need = RC.routes_of([g600, big, small])
    assert routes == ["PHASES", "PHASEWISE", "LM"], routes
    assert need[0] == -1 and need[1] == -1 and need[2] > 0


def test_lds_sweep_covers_resident_partial_and_staged_layouts(table):
    """lm_kernel moves arrays into LDS while they fit (150 KiB) and stages the Jacobians above 384 edges: the LM-route graphs of the table ask for
    less and more than the cap, sit on both sides of the stage threshold, and two LM_BIG batches ask for several times the cap."""
    lm = [(name, sum(len(P["edge_cam"]) for P in RC.BY_NAME[name].problems()), need[0])
          for name, (routes, need) in table.items() if routes[0] == "LM" and name.startswith(("lds_", "global_", "degenerate_"))]
    needs = [n for _, _, n in lm]
    assert min(needs) < RC.LM_LDS_CAP < max(needs), lm
    assert any(n > RC.LM_LDS_CAP for _, e, n in lm if e < RC.LM_STAGE_EDGES), lm          # partially resident without the stage
    edges = {e for _, e, _ in lm}
    assert {RC.LM_STAGE_EDGES, RC.LM_STAGE_EDGES + 1, 511} <= edges and min(edges) <= 40, sorted(edges)
    big = [max(table[name][1]) for name in ("lds_big_two_global", "lds_big_free_cameras_fixed_objects")]
    assert all(n > 3 * RC.LM_LDS_CAP for n in big), big


def test_every_default_route_is_reached(table):
    """If a route becomes unreachable or a new one appears, the table must follow -- coverage does not shrink silently."""
    default = set(RC.route_codes()) - RC.TUNING_ONLY_ROUTES
    assert default == {"LM", "LM_BIG", "FRAME2", "FRAME8", "FRAME16", "CAM2", "CAM", "PHASES", "PHASEWISE"}, default
    expected = {r for c in RC.CASES for r in c.routes}
    assert expected == default, (default - expected, expected - default)
    reported = {r for routes, _ in table.values() for r in routes}
    assert reported == default, reported ^ default


def test_route_entry_rejects_a_dangling_edge(built):
    from suo_slam_amd import _lib
    P = RC.frame(np.random.default_rng(7), [10, 10])
    P["edge_obj"] = P["edge_obj"].copy()
    P["edge_obj"][3] = 2
    with pytest.raises(_lib.SuoError):
        RC.routes_of([P])
