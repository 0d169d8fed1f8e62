"""Designed inputs for the PnP RANSAC accept rule (csrc/pnp.hip: pnp_batch_kernel; oracle/pnp_oracle.c: orc_pnp_ransac_draws).  Host only.

A SCENE is a set of 2D-3D correspondences made of disjoint groups, each exactly consistent with a pose of its own, plus outliers consistent with
nothing.  A draw TABLE dictates every hypothesis's 4-point sample, so a SCRIPT {hypothesis index: group} turns into a known sequence of inlier counts:
a quadruple of group g has exactly consensus[g] inliers, an outlier quadruple at most 4.  What the RANSAC loop makes of that sequence,
    for i: if i >= iters: break;  if cnt[i] > best: best, winner, iters = cnt[i], i, tab[best]
is sequential_accept() below -- ten lines that share nothing with the oracle's C or the kernel's scan -- and every case states its expected
(best, winner, iterations) from the reasoning in its template; _case() holds that statement against sequential_accept() at import, with every
outlier row counted as 0 and again as 4 (the result may not hang on which).

tab[b] = get_iterations(b / n) falls below its cap of 1000 only for b / n > 0.37, and to 256 only for b / n > 0.53: two DISJOINT groups cannot both
be that large.  shared = s therefore relates the groups' poses by rotations about one model-space line and puts s points ON that line: they are
consistent with every group's pose, consensus[g] = sizes[g] + s, and groups of consensus b and b + 1 fit any n >= b + 13.

W is the kernel's round size (64 * PNP_WAVES: 256 for launches of more than 32 objects, 1024 up to 32), E = W / 64 the entries per lane of its scan
(entry j of a round sits in lane j // E at e = j % E).  Every case runs at both widths; the templates place their events per W.

Two statements of the issue that listed these cases do not survive the sequential loop and are stated here as the loop has them: a hypothesis accepted
at index i >= tab[new best] - 1 ends the loop with iterations == i + 1 (not tab[new best]); so "B at tA - 1" ends at tA, "C at tB - 1" at tB."""
import numpy as np

from oracle import geometry as G

THRESHOLD = 1e-3
CAP = 1000                                     # get_iterations' cap: the loop never runs further, whatever the table holds
OUTLIER, ZERO, COLLINEAR, COINCIDENT, REPEAT = "outlier", "zero", "collinear", "coincident", "repeat"


def iter_table(n):
    """tab[b] = get_iterations(b / n), b = 0..n (the oracle's restatement of PnpParams::get_iterations)."""
    f = G.lib().orc_get_iterations
    return [f(b / n) for b in range(n + 1)]


def sequential_accept(counts, tab):
    """The loop of PNP::compute over a given sequence of inlier counts: (best, winner, iterations)."""
    best, winner, iters, i = 0, -1, tab[0], 0
    while i < iters and i < len(counts):
        if counts[i] > best:
            best, winner = counts[i], i
            iters = tab[best]
        i += 1
    return best, winner, i


def _rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _random_pose(rng):
    R = _rotation(rng.normal(size=3), rng.uniform(0.3, 2.8))
    return R, np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(4, 7)])


def _project(R, t, X):
    P = X @ R.T + t
    return P[:, :2] / P[:, 2:3]


def grouped_scene(rng, sizes, n_outliers, behind=0, shared=0, degenerate=False):
    """Model points in [-1, 1]^3, depth 4-7, noise-free.  Points are laid out group after group, then the shared points, the outliers and the `behind` points.
    behind = m: m further points of group 0 that reproject perfectly from BEHIND the camera (z < 0): they must never count.
    degenerate: the first 7 outliers are 3 collinear and 4 coincident model points (with unrelated image points).
    Returns a dict: xs [n,3], ys [n,2], group_of_point [n] (group label; -1 outlier, -2 shared), behind [n] bool, poses [(R, t)], consensus [per group]."""
    R0, t0 = _random_pose(rng)
    poses = [(R0, t0)]
    p_line, d_line = rng.uniform(-0.3, 0.3, 3), rng.normal(size=3)
    d_line /= np.linalg.norm(d_line)
    for g in range(1, len(sizes)):
        if shared:                              # x -> R0 (p + Q (x - p)) + t0 with Q about the line through p: points on the line go where pose 0 sends them
            Q = _rotation(d_line, rng.uniform(0.5, 2.5) * (1 if g % 2 else -1) + 0.2 * g)
            poses.append((R0 @ Q, R0 @ (p_line - Q @ p_line) + t0))
        else:
            poses.append(_random_pose(rng))
    xs, ys, label = [], [], []
    for g, m in enumerate(sizes):
        X = rng.uniform(-1, 1, (m, 3))
        xs.append(X); ys.append(_project(*poses[g], X)); label += [g] * m
    if shared:
        X = p_line + np.linspace(-0.6, 0.6, shared)[:, None] * d_line
        xs.append(X); ys.append(_project(R0, t0, X)); label += [-2] * shared
    X = rng.uniform(-1, 1, (n_outliers, 3))
    if degenerate:
        assert n_outliers >= 12
        X[1] = 0.5 * (X[0] + X[2])                                            # 0, 1, 2 collinear
        X[3:7] = X[3]                                                         # 3..6 coincident
    xs.append(X); ys.append(rng.uniform(-0.25, 0.25, (n_outliers, 2))); label += [-1] * n_outliers
    n_front = len(label)
    if behind:
        Xf = rng.uniform(-1, 1, (behind, 3))
        Pf = Xf @ R0.T + t0
        xs.append((-Pf - t0) @ R0)                                            # R0 x + t0 = -Pf: the mirror image, same x / z and y / z, z < 0
        ys.append(Pf[:, :2] / Pf[:, 2:3]); label += [0] * behind
    label = np.array(label)
    is_behind = np.arange(len(label)) >= n_front
    return {"xs": np.ascontiguousarray(np.concatenate(xs)), "ys": np.ascontiguousarray(np.concatenate(ys)), "group_of_point": label, "behind": is_behind,
            "poses": poses, "consensus": [m + shared for m in sizes], "degenerate": degenerate}


def table_from_script(scene, script, n_draws, rng):
    """int32 [n_draws, 4], rows ascending, all indices in [0, n).  script[i] = a group label (a quadruple of that group's own points, none of them shared or
    behind), OUTLIER (four outliers; also every unlisted i), ZERO / REPEAT (one index four times / a row with a repeated index), COLLINEAR (three collinear
    model points first), COINCIDENT (four coincident model points)."""
    assert n_draws in (1000, 1024)
    lab, beh = scene["group_of_point"], scene["behind"]
    out = np.flatnonzero(lab == -1)
    plain = out[7:] if scene["degenerate"] else out
    tab = np.zeros((n_draws, 4), np.int32)
    for i in range(n_draws):
        what = script.get(i, OUTLIER)
        if what == OUTLIER:
            row = rng.choice(plain, 4, replace=False)
        elif what == ZERO:
            row = np.repeat(rng.integers(0, len(lab)), 4)
        elif what == REPEAT:
            a = rng.choice(plain, 3, replace=False)
            row = np.r_[a, a[0]]
        elif what == COLLINEAR:
            row = np.r_[out[:3], rng.choice(plain, 1)]
        elif what == COINCIDENT:
            row = out[3:7]
        else:
            row = rng.choice(np.flatnonzero((lab == what) & ~beh), 4, replace=False)
        tab[i] = np.sort(row)
    assert tab.min() >= 0 and tab.max() < len(lab)
    return tab


class Case:
    def __init__(self, name, sizes, n_outliers, script, expect, n_draws, scene_kw, seed, pose_group):
        self.name, self.sizes, self.n_outliers, self.script, self.expect, self.n_draws = name, sizes, n_outliers, script, expect, n_draws
        self.scene_kw, self.seed, self.pose_group = scene_kw, seed, pose_group
        self._made = None

    def make(self):
        """(scene, table), built once from the case's own seed."""
        if self._made is None:
            rng = np.random.default_rng(self.seed)
            scene = grouped_scene(rng, self.sizes, self.n_outliers, **self.scene_kw)
            self._made = (scene, table_from_script(scene, self.script, self.n_draws, rng))
        return self._made

    @property
    def n(self):
        return sum(self.sizes) + self.n_outliers + self.scene_kw.get("shared", 0) + self.scene_kw.get("behind", 0)

    def __repr__(self):
        return self.name


CASES = []


def _case(name, sizes, n_outliers, script, expect, n_draws=1000, bounds=None, pose_group=None, **scene_kw):
    """expect = (best, winner, iterations), or None where only the oracle can say (tables of outlier rows alone: best is 3 or 4).
    bounds = {consensus: tab[consensus]} the case's reasoning relies on: asserted, never assumed."""
    if any(c.name == name for c in CASES):
        return
    c = Case(name, tuple(sizes), n_outliers, dict(script), expect, n_draws, scene_kw, 1000 + len(CASES), pose_group)
    tab = iter_table(c.n)
    assert tab[0] == CAP and tab[4] == CAP, name                            # outlier rows (<= 4 inliers) never shorten the loop
    for b, it in (bounds or {}).items():
        assert tab[b] == it, (name, b, tab[b], it)
    cons = [m + scene_kw.get("shared", 0) for m in sizes]
    assert not cons or min(cons) > 4 or expect is None or expect[0] <= 4, name
    if expect is not None and expect[0] > 4:
        for filler in (0, 4):
            counts = [cons[script[i]] if isinstance(script.get(i), int) else (0 if script.get(i) == ZERO else filler) for i in range(n_draws)]
            assert sequential_accept(counts, tab) == tuple(expect), (name, filler, sequential_accept(counts, tab), expect)
    CASES.append(c)


ROUNDS = (256, 1024)          # W
#            bound: (n, b) with tab_n[b] == bound
BOUND_AT = {255: (67, 36), 256: (41, 22), 257: (69, 37), 511: (84, 37), 512: (134, 59), 513: (25, 11), 767: (38, 15), 768: (223, 88), 769: (109, 43),
            999: (239, 88), 101: (51, 38)}


def _shared_groups(n, b, own=(8, 9)):
    """groups of consensus b, b + 1, ... in a scene of n points: own[g] points of their own and b - own[0] shared ones; the rest are outliers"""
    s = b - own[0]
    n_out = n - s - sum(own)
    assert s >= 0 and n_out >= 5, (n, b)
    return dict(sizes=own, n_outliers=n_out, shared=s)


# ---- 1. winner positions ---------------------------------------------------------------------------------------------------------------------------
# one group of 9 among 49 points: tab[9] = 1000, nothing ever shortens the loop, so any index below 1000 is reached
for _i in (0, 255, 256, 999):                  # 0, W - 1 and W of the 256-round; 999 is the last hypothesis of all (W - 1 = 1023 and W = 1024 lie beyond the cap: below)
    _case(f"winner_at_{_i}", (9,), 40, {_i: 0}, (9, _i, 1000), bounds={9: 1000}, pose_group=0)
# n_draws = 1024: rows 1000..1023 exist, the 1024-round evaluates them, the loop never reaches them
_case("beyond_cap_only_over_outliers", (9,), 40, {i: 0 for i in range(1000, 1024)}, None, n_draws=1024)
_case("beyond_cap_only_over_zeros", (9,), 40, {**{i: ZERO for i in range(1000)}, **{i: 0 for i in range(1000, 1024)}}, (0, -1, 1000), n_draws=1024)

# ---- 2. the bound shrinks inside a round --------------------------------------------------------------------------------------------------------
# consensus A = 56 < B = 59 < C = 60 of n = 134: tA = 620, tB = 512, tC = 481
_ABC = dict(sizes=(5, 8, 9), n_outliers=61, shared=51, bounds={56: 620, 59: 512, 60: 481})
for _W in ROUNDS:
    _b0 = 619 // _W * _W                       # the round that holds tA - 1
    # B at tA - 1, the last index A's bound admits: accepted, and the loop ends there (tB <= tA - 1)
    _case(f"shrink_B_at_last_admitted_W{_W}", script={_b0 + 3: 0, 619: 1}, expect=(59, 619, 620), **_ABC)
    _case(f"shrink_B_at_first_excluded_W{_W}", script={_b0 + 3: 0, 620: 1}, expect=(56, _b0 + 3, 620), **_ABC)
    # A, then B, then C at tB -- the first index B's bound excludes -- all in one round: ignored; at tB - 1: accepted.  n = 84: tA = 698, tB = 511, tC = 464
    _b0 = 510 // _W * _W
    _kw = dict(sizes=(5, 8, 9), n_outliers=33, shared=29, bounds={34: 698, 37: 511, 38: 464})
    _case(f"shrink_C_at_tB_ignored_W{_W}", script={_b0 + 2: 0, _b0 + 9: 1, 511: 2}, expect=(37, _b0 + 9, 511), **_kw)
    _case(f"shrink_C_at_tB_minus_1_accepted_W{_W}", script={_b0 + 2: 0, _b0 + 9: 1, 510: 2}, expect=(38, 510, 511), **_kw)
    # the same with a C lying beyond BOTH later bounds but inside the first (A's): only the prefix maximum at its index decides
    _case(f"shrink_C_between_tB_and_tA_W{_W}", script={_b0 + 2: 0, _b0 + 9: 1, 600: 2}, expect=(37, _b0 + 9, 511), **_kw)

# ---- 3. the bound on a round boundary -----------------------------------------------------------------------------------------------------------
for _bound in (255, 256, 257, 511, 512, 513, 768):
    _n, _b = BOUND_AT[_bound]
    for _W in ROUNDS:
        _b0 = (_bound - 1) // _W * _W          # the round that holds the last admitted index
        _jB = _b0 + 1 if _b0 + 1 < _bound - 1 else _bound - 2
        _kw = dict(bounds={_b: _bound}, **_shared_groups(_n, _b))
        # (at 256, 512 and 768 the 256-round ends exactly at the bound: no further round may start)
        _case(f"bound_{_bound}_better_at_bound_ignored_jB{_jB}", script={_jB: 0, _bound: 1}, expect=(_b, _jB, _bound), pose_group=0, **_kw)
        _case(f"bound_{_bound}_better_at_bound_minus_1_accepted_jB{_jB}", script={_jB: 0, _bound - 1: 1}, expect=(_b + 1, _bound - 1, _bound), pose_group=1, **_kw)

# ---- 4. J (the first entry the loop does not reach) inside a lane ---------------------------------------------------------------------------
# bounds that are no multiple of E: 257 and 769 (e = 1 for both E), 767 (e = 3 of 4, 15 of 16), 999 (e = 3 of 4, 7 of 16)
for _bound in (257, 767, 769, 999):
    _n, _b = BOUND_AT[_bound]
    _kw = dict(bounds={_b: _bound}, **_shared_groups(_n, _b))
    for _W in ROUNDS:
        _E = _W // 64
        _b0 = (_bound - 1) // _W * _W
        _jB = _b0 + 1 if _b0 + 1 < _bound - 1 else _bound - 2
        assert _bound % _E != 0
        # a higher count in J's own lane, at J and after it: ignored
        for _j in range(_bound, min(_b0 + ((_bound - _b0) // _E + 1) * _E, 1000)):
            _case(f"lane_{_bound}_higher_past_J_at_{_j}_jB{_jB}", script={_jB: 0, _j: 1}, expect=(_b, _jB, _bound), **_kw)
        _case(f"lane_{_bound}_higher_at_bound_minus_1_jB{_jB}", script={_jB: 0, _bound - 1: 1}, expect=(_b + 1, _bound - 1, _bound), **_kw)
# the true winner at every e of the last full lane before J, and a still higher count right behind it -- past the J that winner makes: ignored
for _bound, _W in ((767, 256), (767, 1024), (769, 1024)):
    _n, _b = BOUND_AT[_bound]
    _E = _W // 64
    _b0 = (_bound - 1) // _W * _W
    _lane = (_bound - _b0) // _E - 1
    _kw = dict(bounds={_b: _bound}, **_shared_groups(_n, _b, own=(5, 6, 7)))
    for _e in range(_E):
        _j = _b0 + _lane * _E + _e
        assert iter_table(_n)[_b + 1] <= _j
        _case(f"lane_{_bound}_W{_W}_winner_at_e{_e}", script={_b0 + 1: 0, _j: 1, _j + 1: 2}, expect=(_b + 1, _j, _j + 1), **_kw)

# ---- 5. ties ------------------------------------------------------------------------------------------------------------------------------------
# two groups of equal consensus and different poses: the first one met wins, and the pose is its quadruple's
_case("tie_same_round", (8, 8), 48, {5: 0, 8: 1}, (8, 5, 1000), pose_group=0)
_case("tie_same_lane", (8, 8), 48, {520: 1, 521: 0}, (8, 520, 1000), pose_group=1)
_case("tie_next_round_W256", (8, 8), 48, {250: 0, 256: 1}, (8, 250, 1000), pose_group=0)
_case("tie_under_a_bound_same_round", bounds={59: 512}, script={3: 0, 200: 1}, expect=(59, 3, 512), pose_group=0, **_shared_groups(134, 59, own=(8, 8)))
_case("tie_under_a_bound_next_round_W256", bounds={59: 512}, script={255: 1, 256: 0}, expect=(59, 255, 512), pose_group=1, **_shared_groups(134, 59, own=(8, 8)))
_case("tie_at_the_last_admitted_index", bounds={59: 512}, script={300: 0, 511: 1}, expect=(59, 300, 512), pose_group=0, **_shared_groups(134, 59, own=(8, 8)))

# ---- 6. low consensus ---------------------------------------------------------------------------------------------------------------------------
# outlier rows alone: three points of a sample always reproject, the fourth only by chance: best is 3 (no refinement) or, when one of the thousand rows is
# lucky, 4 (refinement on four points) -- the oracle says which, test_pnp_cases holds it to one of the two.  low_best_4_* make sure of a 4: a "group" of four.
# Then a table of samples that yield no pose at all.
_case("low_outliers_only", (), 40, {}, None)
_case("low_best_4_runs_the_refinement", (4,), 40, {0: 0}, (4, 0, 1000), pose_group=0)
_case("low_best_4_late", (4,), 40, {777: 0}, None)
_case("low_all_zero", (9,), 40, {i: ZERO for i in range(1000)}, (0, -1, 1000))

# ---- 7. degenerate samples before the real winner -------------------------------------------------------------------------------------------------
_case("degenerate_rows_before_the_winner", (9,), 40, {0: REPEAT, 1: COLLINEAR, 2: COINCIDENT, 3: ZERO, 4: REPEAT, 6: 0}, (9, 6, 1000), degenerate=True, pose_group=0)
_case("degenerate_rows_inside_a_shrunk_loop", script={0: COINCIDENT, 1: 0, 2: COLLINEAR, 3: REPEAT, 510: COINCIDENT, 511: 1}, expect=(60, 511, 512), degenerate=True,
      bounds={59: 512}, **_shared_groups(134, 59))

# ---- 8. behind the camera -----------------------------------------------------------------------------------------------------------------------
# group 0: 9 points in front and 5 perfect reprojections from behind.  Were they counted, its 14 would block group 1's 12
_case("behind_never_counts", (9, 12), 30, {2: 0, 7: 1}, (12, 7, 1000), behind=5, pose_group=1)
_case("behind_group_alone", (9,), 40, {2: 0}, (9, 2, 1000), behind=5, pose_group=0)

BY_NAME = {c.name: c for c in CASES}
