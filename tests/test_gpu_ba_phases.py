"""Every phase kernel of the global bundle adjustment (csrc/lm_dist.hip) against the mp reference of tests/ba_phases_ref.py, number for number, on the graphs of
tests/ba_phase_cases.py (placed on the kernels' lane-group shapes), driven through suo_ba_ctx_create and the host-array entries; then the failure paths, pop(), the
classification's thresholds, the exact properties (repeatability, the _dev entries, the per-rank maximum slots), the three-rank partition and the device control block.

Tolerances: |kernel - mp| <= K eps M per entry, M the reference's error scale of that entry (condition numbers of Hcc + lambda I and of the reduced system folded in
for the Schur, solve and update outputs; tests/ba_phases_ref.py says how).  K = max(8, 4 K_ref) with K_ref = max |NumpyPhases - mp| / (eps M) measured on the CPU
over every case, state and lambda by tests/test_ba_phases_ref.py -- reference against reference, no GPU in it:

    buffer                                   K_ref (CPU)    K
    chi2    per-edge chi2 of classify           0.426        8
    lin     [chi2 | Hoo 21 + bo 6 | max]        3.96        16
    sch     [S_g | r_g]                         1.43         8
    red     [chi2 after | scale | . | scale]    0.268        8
    poses   the downloaded 3x4 poses            0.996        8

For the record, the worst |kernel - mp| / (eps M) observed on an MI355X (printed by every run; NOT used for K):  see the table test_each_phase_alone prints; the
figures of the run this module was written against are in OBSERVED below (chi2 0.43, lin 1.8, sch 1.5, red 0.077, poses 2.8).
An entry whose M is 0 (a block no edge reaches, the ok flags) must be met exactly."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import ba_phase_cases as PC  # noqa: E402
from tests import ba_phases_ref as R  # noqa: E402

EPS = R.EPS
# worst |kernel - mp| / (eps M) per buffer over every case, state and lambda, as one MI355X run printed them (for the record only)
OBSERVED = {"chi2": 0.426, "lin": 1.81, "sch": 1.52, "red": 0.0765, "poses": 2.8}
_seen = {b: 0.0 for b in R.K}


class Ctx:
    """A suo_ba_ctx over one ba.Problem through the HOST-array entries (ba_dist.HipPhases drives the _dev entries of the same context type)."""

    def __init__(self, prob):
        from suo_slam_amd import _lib
        self._lib, self.lib, self.prob = _lib, _lib.lib(), prob
        _lib.require_gpu()
        self.s = _lib.BaProblem()
        prob._fill(self.s)
        self.h = C.c_void_p()
        _lib.check(self.lib.suo_ba_ctx_create(C.byref(self.s), C.byref(self.h)), "suo_ba_ctx_create")
        self.O, self.E = len(prob.obj_T), len(prob.edge_cam)
        self.ns = int(self.lib.suo_ba_ctx_ns(self.h))

    def classify(self, keep_all):
        good = np.zeros(1)
        self._lib.check(self.lib.suo_ba_classify(self.h, int(keep_all), good.ctypes.data), "suo_ba_classify")
        return float(good[0])

    def linearize(self, robust_on):
        out = np.full(2 + 27 * self.O, np.nan)
        self._lib.check(self.lib.suo_ba_linearize(self.h, int(robust_on), out.ctypes.data), "suo_ba_linearize")
        return out

    def schur(self, lam):
        out = np.full(self.ns * self.ns + self.ns + 1, np.nan)
        self._lib.check(self.lib.suo_ba_schur(self.h, float(lam), out.ctypes.data), "suo_ba_schur")
        return out

    def solve_update(self, lam, robust_on, totals):
        """red in the DEVICE order [chi2 | scale over cameras | ok | scale over objects]."""
        t = np.ascontiguousarray(totals, np.float64)
        assert len(t) == 27 * self.O + self.ns * self.ns + self.ns
        out = np.full(4, np.nan)
        self._lib.check(self.lib.suo_ba_solve_update(self.h, float(lam), int(robust_on), t.ctypes.data, out.ctypes.data), "suo_ba_solve_update")
        return out[[0, 1, 3, 2]]

    def restore(self):
        self._lib.check(self.lib.suo_ba_restore(self.h), "suo_ba_restore")

    def download(self):
        """(cam_T [C,3,4], obj_T [O,3,4], chi2 [E], inlier [E]) as the context holds them now."""
        self._lib.check(self.lib.suo_ba_ctx_download(self.h, C.byref(self.s)), "suo_ba_ctx_download")
        p = self.prob
        return p.cam_T.reshape(-1, 3, 4).copy(), p.obj_T.reshape(-1, 3, 4).copy(), p.chi2[:self.E].copy(), p.inlier.copy()

    def totals(self, lin, sch):
        return np.concatenate([lin[1:1 + 27 * self.O], sch[:-1]])

    def close(self):
        if self.h is not None:
            self.lib.suo_ba_ctx_destroy(self.h)
            self.h = None


@pytest.fixture
def ctx_of():
    made = []

    def make(prob):
        made.append(Ctx(prob))
        return made[-1]
    yield make
    for c in made:
        c.close()


@pytest.fixture
def phases_of():
    from suo_slam_amd import ba_dist
    made = []

    def make(prob, world=1):
        made.append(ba_dist.HipPhases(prob, world))
        return made[-1]
    yield make
    for p in made:
        p.close()


def _host(t):
    """A device tensor of any length on the host (HipPhases.read is sized for the schedule's few scalars)."""
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check(buf, what, got, ref, M, bad):
    """Holds got to ref within K eps M; returns the worst |got - ref| / (eps M) and notes a miss in `bad`."""
    got, ref, M = (np.asarray(a, np.float64).ravel() for a in (got, ref, M))
    d = np.abs(got - ref)
    exact = M == 0
    worst = float((d[~exact] / (EPS * M[~exact])).max()) if (~exact).any() else 0.0
    _seen[buf] = max(_seen[buf], worst)
    if not np.isfinite(got).all() or (d[exact] != 0).any() or worst > R.K[buf]:
        i = int(np.argmax(np.where(exact, np.where(d != 0, np.inf, 0), d / (EPS * np.maximum(M, 1e-300)))))
        bad.append(f"{what}: entry {i} got {got[i]!r} ref {ref[i]!r}, |d| / (eps M) = {worst:.3g} > K = {R.K[buf]}")
    return worst


def _check_poses(what, poses, U, bad):
    return max(_check("poses", what + " cameras", poses[0], U.cam_T, U.MCcam, bad), _check("poses", what + " objects", poses[1], U.obj_T, U.MCobj, bad))


# ---- each phase alone ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_each_phase_alone(name, ctx_of):
    """linearize, schur(lambda) and solve_update of one context per case, Huber kernel off and on, before and after the chi2 classification, lambda in {1e-5 maxdiag, 1,
    1e6 maxdiag}: every output entry against mp.  solve_update once on the reference's totals rounded to fp64 (no earlier phase's error reaches it) and once on the
    kernels' own lin and sch, to the same tolerances; every phase twice for the same bits."""
    cr, ctx, bad = R.case(name), ctx_of(PC.problem(name)), []
    worst = {b: 0.0 for b in R.K}
    for classified in (0, 1):
        good = ctx.classify(keep_all=not classified)
        start = ctx.download()
        worst["chi2"] = max(worst["chi2"], _check("chi2", f"classify({classified}) chi2", start[2], cr.chi2, cr.Mchi2, bad))
        if classified:
            assert np.array_equal(start[3], cr.inlier) and good == cr.inlier.sum()
        else:
            assert good == cr.ref.E
        for robust_on in (0, 1):
            tag = f"{name} robust {robust_on} classified {classified}"
            L = cr.lin(robust_on, classified)
            lin = ctx.linearize(robust_on)
            assert _same_bits(lin, ctx.linearize(robust_on)), tag + ": linearize twice"
            worst["lin"] = max(worst["lin"], _check("lin", tag + " lin", lin, L.lin, L.M, bad))
            for which in R.LAMBDAS:
                lam, Sc, U = cr.lam(robust_on, classified, which), cr.sch(robust_on, classified, which), cr.upd(robust_on, classified, which)
                assert Sc.ok == 1.0 and U.ok == 1.0
                sch = ctx.schur(lam)
                assert _same_bits(sch, ctx.schur(lam)), f"{tag} lambda {which}: schur twice"
                worst["sch"] = max(worst["sch"], _check("sch", f"{tag} lambda {which} sch", sch, Sc.sch, Sc.MC, bad))
                assert sch[-1] == 1.0
                for feed, totals in (("reference totals", cr.ref.totals(L, Sc)), ("own lin and sch", ctx.totals(lin, sch))):
                    if feed != "reference totals":
                        ctx.schur(lam)                      # push() again: the first step was popped
                    red = ctx.solve_update(lam, robust_on, totals)
                    assert red[2] == 1.0, f"{tag} lambda {which} ({feed}): the step was refused"
                    worst["red"] = max(worst["red"], _check("red", f"{tag} lambda {which} red ({feed})", red, U.red, U.Mred, bad))
                    worst["poses"] = max(worst["poses"], _check_poses(f"{tag} lambda {which} ({feed})", ctx.download(), U, bad))
                    ctx.restore()
        after = ctx.download()
        assert _same_bits(after[0], start[0]) and _same_bits(after[1], start[1]), "restore did not bring the poses back"
    print(f"observed {name:7s} " + "  ".join(f"{b} {v:.3g}" for b, v in worst.items()))
    assert not bad, "\n".join(bad)


def test_ns96_and_ns102_agree_on_the_shared_objects(ctx_of):
    """ns96 is ns102 without its last object: the Hoo and bo of the sixteen shared objects are the same sums over the same edges, and agree within the two tolerances
    (bits are not required: another grid, another tree).  S_g and r_g do NOT agree and are not compared: the seventeenth object's edges are part of every camera's
    Hcc, so (Hcc + lambda I)^-1 -- and with it every block of S_g -- is another matrix in ns102; each is held to its own reference by test_each_phase_alone."""
    a, b = ctx_of(PC.problem("ns96")), ctx_of(PC.problem("ns102"))
    ra, rb = R.case("ns96"), R.case("ns102")
    n = 1 + 27 * 16
    for robust_on in (0, 1):
        out = []
        for c in (a, b):
            c.classify(1)
            out.append(c.linearize(robust_on))
        Ma, Mb = ra.lin(robust_on, 0).M[1:n], rb.lin(robust_on, 0).M[1:n]
        assert np.array_equal(ra.lin(robust_on, 0).lin[1:n], rb.lin(robust_on, 0).lin[1:n]) and (Ma > 0).all()
        assert (np.abs(out[0][1:n] - out[1][1:n]) <= R.tol("lin", Ma) + R.tol("lin", Mb)).all()


# ---- failure paths ------------------------------------------------------------------------------------------------------------------------------------------------
def _with_camera_fixed(name, cam):
    prob = PC.problem(name)
    prob.cam_fixed[cam] = 1
    return prob


@pytest.mark.parametrize("name,classified", [("weak", 0), ("slots", 1)])
def test_singular_camera_block_at_lambda_zero(name, classified, ctx_of):
    """The camera seen through one keypoint (Hcc of rank 2) and the camera whose every edge was cast out (Hcc = 0) at lambda = 0: the reference's Cholesky of that
    block meets a non-positive pivot, and of that block alone.  The kernels must say ok = 0, add exactly nothing of that camera to S_g and r_g -- the bits of a context
    in which the camera is FIXED, whose S_g and r_g pass it over --, refuse the step ([chi2 at the unchanged poses, 0, 0, 0]) and leave every pose's bits."""
    cam = PC.weak_camera() if name == "weak" else PC.SLOTS_CAST_OUT_CAMERA
    cr = R.case(name)
    L, Sc = cr.lin(1, classified), cr.sch(1, classified, "zero")
    assert Sc.failed == [cam] and Sc.ok == 0.0
    U = cr.ref.solve_update(L, Sc, 0.0, 1)
    assert U.ok == 0.0 and (U.red[1:] == 0).all()
    ctx, twin, bad = ctx_of(PC.problem(name)), ctx_of(_with_camera_fixed(name, cam)), []
    for c in (ctx, twin):
        c.classify(keep_all=not classified)
        c.linearize(1)
    before = ctx.download()
    sch, sch_twin = ctx.schur(0.0), twin.schur(0.0)
    assert sch[-1] == 0.0 and sch_twin[-1] == 1.0
    assert _same_bits(sch[:-1] + 0.0, sch_twin[:-1] + 0.0)           # (+ 0.0: a sum of signed zeros may be -0)
    _check("sch", "sch without the failed camera", sch, Sc.sch, Sc.MC, bad)
    red = ctx.solve_update(0.0, 1, cr.ref.totals(L, Sc))
    assert (red[1:] == 0).all(), red
    _check("red", "chi2 at the unchanged poses", red[:1], U.red[:1], U.Mred[:1], bad)
    after = ctx.download()
    assert _same_bits(after[0], before[0]) and _same_bits(after[1], before[1])
    assert not bad, "\n".join(bad)


def test_edgeless_free_object_does_not_move(ctx_of):
    """The free object of `slots` that no edge reaches: its block of the reduced system is lambda I and its right-hand side 0, so x_o = 0 exactly at any lambda > 0.  Seen
    from outside: exp(0) T keeps the translation's bits (t' = V 0 + I t) and the rotation up to the renormalisation of the unit quaternion."""
    cr, ctx = R.case("slots"), ctx_of(PC.problem("slots"))
    o = PC.SLOTS_EDGELESS_OBJECT
    ctx.classify(0)
    before = ctx.download()
    lin = ctx.linearize(1)
    assert (lin[1 + 27 * o:28 + 27 * o] == 0).all()
    for which in R.LAMBDAS:
        lam = cr.lam(1, 1, which)
        U = cr.upd(1, 1, which)
        assert (U.xo[o] == 0).all()
        sch = ctx.schur(lam)
        red = ctx.solve_update(lam, 1, ctx.totals(lin, sch))
        assert red[2] == 1.0
        after = ctx.download()
        assert _same_bits(after[1][o][:, 3], before[1][o][:, 3])
        assert np.abs(after[1][o][:, :3] - before[1][o][:, :3]).max() <= 4 * EPS
        assert not _same_bits(after[1][0], before[1][0])                       # (the others did move)
        ctx.restore()


@pytest.mark.parametrize("name", ["ns96", "ns102"])
def test_indefinite_reduced_system_is_refused(name, ctx_of):
    """S_total = 2 (Hoo + lambda I) on one diagonal block leaves -(Hoo + lambda I) there: the reference's Cholesky stops at its first pivot, and so must ba_solve_kernel
    (ns = 96, LDS) and ba_solve_big_kernel (ns = 102): [chi2 at the unchanged poses, 0, 0, 0], every pose's bits as they were."""
    cr, ctx, bad = R.case(name), ctx_of(PC.problem(name)), []
    L, lam, Sc = cr.lin(1, 0), cr.lam(1, 0, "lo"), cr.sch(1, 0, "lo")
    totals = cr.ref.totals(L, Sc)
    O, ns, blk = cr.ref.O, cr.ref.ns, 7
    S = totals[27 * O:27 * O + ns * ns].reshape(ns, ns)
    H = np.zeros((6, 6))
    H[R.IU] = totals[27 * blk:27 * blk + 21]
    H = H + H.T - np.diag(np.diag(H))
    S[6 * blk:6 * blk + 6, 6 * blk:6 * blk + 6] = 2 * (H + lam * np.eye(6))
    U = cr.ref.solve_update(L, Sc, lam, 1, totals=totals)
    assert U.ok == 0.0
    ctx.classify(1)
    ctx.linearize(1)
    before = ctx.download()
    assert ctx.schur(lam)[-1] == 1.0
    red = ctx.solve_update(lam, 1, totals)
    assert (red[1:] == 0).all(), red
    _check("red", "chi2 at the unchanged poses", red[:1], U.red[:1], U.Mred[:1], bad)
    after = ctx.download()
    assert _same_bits(after[0], before[0]) and _same_bits(after[1], before[1])
    assert not bad, "\n".join(bad)


# ---- pop() ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_restore_brings_back_the_bits(ctx_of):
    cr, ctx = R.case("small"), ctx_of(PC.problem("small"))
    lam = cr.lam(1, 0, "lo")
    ctx.classify(1)
    lin = ctx.linearize(1)
    before = ctx.download()
    first = []
    for _ in range(2):
        sch = ctx.schur(lam)
        red = ctx.solve_update(lam, 1, ctx.totals(lin, sch))
        assert red[2] == 1.0
        moved = ctx.download()
        assert not _same_bits(moved[0][1:], before[0][1:]) and not _same_bits(moved[1], before[1])
        ctx.restore()
        back = ctx.download()
        assert _same_bits(back[0], before[0]) and _same_bits(back[1], before[1])
        first.append((sch, red, moved))
    assert _same_bits(first[0][0], first[1][0]) and _same_bits(first[0][1], first[1][1])
    assert _same_bits(first[0][2][0], first[1][2][0]) and _same_bits(first[0][2][1], first[1][2][1])


# ---- classify: the threshold rule ------------------------------------------------------------------------------------------------------------------------------------
def test_classify_thresholds(ctx_of):
    """chi2 > chi2_thr casts an edge out: with the threshold ON an edge's own chi2 (as the device reported it) the edge stays, one ulp below it goes; nothing else
    changes sides, since the reference places every other edge 1e-6 relative away.  num_good is the count of the flags; keep_all changes none and counts every edge."""
    cr = R.case("small")
    ctx = ctx_of(PC.problem("small"))
    ctx.classify(1)
    chi2 = ctx.download()[2]
    for e in R.threshold_edges(cr):
        others = np.delete(cr.chi2, e)
        assert (np.abs(others - cr.chi2[e]) > 1e-6 * cr.chi2[e]).all()
        expected = (cr.chi2 <= cr.chi2[e]).astype(np.uint8)
        for thr, own in ((chi2[e], 1), (np.nextafter(chi2[e], 0.0), 0)):
            c = ctx_of(PC.problem("small", chi2_thr=float(thr)))
            good = c.classify(0)
            flags = c.download()[3]
            expected[e] = own
            assert np.array_equal(flags, expected), (e, thr)
            assert good == flags.sum()
            assert c.classify(1) == len(flags) and np.array_equal(c.download()[3], flags)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------------------------
def test_dev_entries_give_the_host_entries_bits(ctx_of, phases_of):
    cr, ctx, ph = R.case("small"), ctx_of(PC.problem("small")), phases_of(PC.problem("small"))
    lam = cr.lam(1, 1, "lo")
    good = ctx.classify(0)
    ph.classify(0)
    assert _host(ph.good)[0] == good
    lin = ctx.linearize(1)
    ph.linearize(1, 0, 1)
    assert _same_bits(_host(ph.lin), lin)
    sch = ctx.schur(lam)
    ph.schur(lam)
    assert _same_bits(_host(ph.sch), sch)
    red = ctx.solve_update(lam, 1, ctx.totals(lin, sch))
    ph.solve_update(lam, 1, 1)
    assert _same_bits(_host(ph.red), red)
    host, dev = ctx.download(), ph.download()
    assert _same_bits(dev.cam_T.reshape(-1, 3, 4), host[0]) and _same_bits(dev.obj_T.reshape(-1, 3, 4), host[1])
    ctx.restore()
    ph.restore()
    host, dev = ctx.download(), ph.download()
    assert _same_bits(dev.cam_T.reshape(-1, 3, 4), host[0]) and _same_bits(dev.obj_T.reshape(-1, 3, 4), host[1])


@pytest.mark.parametrize("rank,world", [(0, 1), (2, 3), (0, 3)])
def test_linearize_dev_puts_the_maximum_in_its_ranks_slot(rank, world, ctx_of, phases_of):
    import torch
    ctx, ph = ctx_of(PC.problem("small")), phases_of(PC.problem("small"), world)
    ctx.classify(1)
    ph.classify(1)
    lin = ctx.linearize(1)
    ph.lin.fill_(float("nan"))
    torch.cuda.synchronize()
    ph.linearize(1, rank, world)
    got = _host(ph.lin)
    n = 1 + 27 * ctx.O
    assert _same_bits(got[:n], lin[:n])
    assert got[n + rank] == lin[n] and lin[n] > 0
    assert _same_bits(np.delete(got[n:], rank), np.zeros(world - 1))


# ---- the partition -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_three_ranks_sum_to_the_whole_graph(phases_of):
    """`ranks` dealt to three contexts (ba_dist.split_problem): their lin and sch summed equal the reference of the WHOLE graph, the sum of the maximum slots carries
    every rank's own maximum, solve_update_dev(world = 3) on the summed buffers moves the objects to the same bits on every rank (and every vertex to the reference's
    pose), and an ok count of 2 makes every rank refuse."""
    import torch
    from suo_slam_amd import ba_dist
    world, bad = 3, []
    cr = R.case("ranks")
    full = PC.problem("ranks")
    shares = [ba_dist.split_problem(full, r, world) for r in range(world)]
    ph = [phases_of(local, world) for local, _, _ in shares]
    L, lam, Sc, U = cr.lin(1, 0), cr.lam(1, 0, "lo"), cr.sch(1, 0, "lo"), cr.upd(1, 0, "lo")
    O, ns = cr.ref.O, cr.ref.ns
    for r, p in enumerate(ph):
        p.classify(1)
        p.linearize(1, r, world)
        p.schur(lam)
    lin = sum(p.lin for p in ph[1:]) + ph[0].lin
    sch = sum(p.sch for p in ph[1:]) + ph[0].sch
    torch.cuda.synchronize()
    hl, hs = lin.cpu().numpy(), sch.cpu().numpy()
    n = 1 + 27 * O
    _check("lin", "summed lin", hl[:n], L.lin[:n], L.M[:n], bad)
    for r, (_, cams, _) in enumerate(shares):
        free = [c for c in cams if not cr.ref.cam_fixed[c]]
        top = max(abs(float(L.Hcc[c][d, d])) for c in free for d in range(6))
        _check("lin", f"maximum slot of rank {r}", hl[n + r:n + r + 1], [top], [max(L.MHcc[c][d, d] for c in free for d in range(6))], bad)
    assert hs[-1] == 3.0
    _check("sch", "summed sch", hs[:-1], Sc.sch[:-1], Sc.MC[:-1], bad)
    before = [p.download() for p in ph]
    before = [(b.cam_T.copy(), b.obj_T.copy()) for b in before]
    # an ok count of 2: every rank refuses
    refused = sch.clone()
    refused[-1] = 2.0
    for p in ph:
        p.lin.copy_(lin)
        p.sch.copy_(refused)
        p.solve_update(lam, 1, world)
        red = _host(p.red)
        assert (red[1:] == 0).all(), red
        d = p.download()
        assert _same_bits(d.obj_T, before[0][1]) and _same_bits(d.cam_T, before[ph.index(p)][0])
    chi = sc_cams = 0.0
    objs = []
    for r, p in enumerate(ph):
        p.schur(lam)                                        # push() and this rank's camera blocks again; its S_g is then replaced by the total
        p.sch.copy_(sch)
        p.solve_update(lam, 1, world)
        red = _host(p.red)
        assert red[2] == 1.0
        chi, sc_cams = chi + red[0], sc_cams + red[1]
        d = p.download()
        objs.append(d.obj_T.copy())
        cams = shares[r][1]
        _check("poses", f"rank {r} cameras", d.cam_T.reshape(-1, 3, 4), U.cam_T[cams], U.MCcam[cams], bad)
        _check("poses", f"rank {r} objects", d.obj_T.reshape(-1, 3, 4), U.obj_T, U.MCobj, bad)
        _check("red", f"rank {r} scale over objects", red[3:], U.red[3:], U.Mred[3:], bad)
    assert _same_bits(objs[0], objs[1]) and _same_bits(objs[0], objs[2])
    _check("red", "chi2 after and the scale over cameras, summed over ranks", [chi, sc_cams], U.red[:2], U.Mred[:2], bad)
    assert not bad, "\n".join(bad)


# ---- the device control block --------------------------------------------------------------------------------------------------------------------------------------------
DBL_MAX = float(np.finfo(np.float64).max)


def _host_decision(prev, lin, red, O, free_obj, its):
    """g2o's accept / reject arithmetic as suo_slam_amd/ba_dist.py: optimize_distributed runs it on the host (the lambda init, rho, alpha, lambda max(1/3, alpha),
    lambda ni, ni 2, the counters), applied to the control block before the unit and the lin / red the unit left: the entries [0,1,2,3,4,6,7,8,9,10] after it."""
    import math
    lam, ni, cur, state, it, qmax, lm_its, trials = prev[0], prev[1], prev[2], int(prev[3]), int(prev[4]), int(prev[6]), prev[7], prev[8]
    if state == 0:
        cur = float(lin[0])
        if it == 0:
            maxd = float(lin[1 + 27 * O:].max())
            for o in free_obj:
                maxd = max(maxd, max(abs(float(lin[1 + 27 * o + d])) for d in (0, 6, 11, 15, 18, 20)))
            lam, ni = 1e-5 * maxd, 2.0
        qmax = 0
    temp, scale = DBL_MAX, 0.0
    if int(round(red[2])) == 1:
        temp, scale = float(red[0]), float(red[1]) + float(red[3])
    rho = (cur - temp) / (scale + 1e-3)
    restore, finite = 0.0, True
    if rho > 0 and math.isfinite(temp):
        r21 = 2 * rho - 1
        alpha = min(1.0 - r21 * r21 * r21, 2.0 / 3.0)
        lam *= max(1.0 / 3.0, alpha)
        ni = 2.0
        cur = temp
    else:
        lam *= ni
        ni *= 2
        restore = 1.0
        finite = math.isfinite(lam)
    if finite:
        qmax += 1
        trials += 1
    if finite and rho < 0 and qmax < 10:
        state = 1
    else:
        lm_its += 1
        it += 1
        state = 2 if (qmax == 10 or rho == 0 or not finite or it >= its) else 0
    return {0: lam, 1: ni, 2: cur, 3: float(state), 4: float(it), 6: float(qmax), 7: lm_its, 8: trials, 9: rho, 10: restore}


def _control_cases():
    from tests import lm_far_cases as F
    from tests import ba_route_cases as RC
    from suo_slam_amd import ba
    far = F.build_reject("both_free")[0]
    return {"small": (lambda: PC.problem("small"), 6, False), "far": (lambda: ba.Problem(*[far[k] for k in RC.KEYS]), 2, True)}


@pytest.mark.parametrize("which", ["small", "far"])
def test_control_block_follows_the_host_arithmetic(which, phases_of):
    """suo_ba_lm_begin_dev, then one unit at a time (suo_ba_lm_unit_one_rank_dev), the control block read after each: bit for bit the host schedule's arithmetic on the
    lin and red the unit left; a rejected unit leaves the pre-trial poses.  The far start (tests/lm_far_cases.py: REJECT both_free) must show an accepted trial, a
    rejected one and the end of the round.  The four separate _lm_*_dev calls then give the folded call's control blocks on the same sequence."""
    import torch
    make, its, need_reject = _control_cases()[which]
    ph, four = phases_of(make()), phases_of(make())
    from suo_slam_amd import _lib
    lib, check = ph.lib, _lib.check
    O = ph.n_obj
    free_obj = [o for o in range(O) if not ph.local.obj_fixed[o]]
    seq, accepted, rejected = [], 0, 0
    for p in (ph, four):
        p.classify(1)
        p.ctl.zero_()
        torch.cuda.synchronize()
        p.begin_round(its, 1)
    prev = _host(ph.ctl)
    assert prev[3] == 0 and prev[5] == its and prev[11] == 1
    for _ in range(its * 11 + 1):
        if int(prev[3]) == 2:
            break
        d = ph.download()
        poses = (d.cam_T.copy(), d.obj_T.copy())
        s = ph._stream()
        check(lib.suo_ba_lm_unit_one_rank_dev(ph._h, 1, ph._p(ph.ctl), ph._p(ph.lin_loc), ph._p(ph.lin), ph._p(ph.sch), ph._p(ph.red), s), "unit")
        ctl, lin, red = _host(ph.ctl), _host(ph.lin), _host(ph.red)
        want = _host_decision(prev, lin, red, O, free_obj, its)
        for i, v in want.items():
            assert _same_bits(ctl[i], v), f"unit {len(seq)}: ctl[{i}] = {ctl[i]!r}, the host arithmetic gives {v!r}"
        if want[10]:
            rejected += 1
            d = ph.download()
            assert _same_bits(d.cam_T, poses[0]) and _same_bits(d.obj_T, poses[1]), "a rejected unit left other poses than it found"
        else:
            accepted += 1
        seq.append(ctl)
        prev = ctl
    assert int(prev[3]) == 2, "the round did not end"
    assert accepted >= 1 and (rejected >= 1 or not need_reject), (accepted, rejected)
    for k, want in enumerate(seq):
        s = four._stream()
        check(lib.suo_ba_lm_linearize_dev(four._h, 1, 0, 1, four._p(four.ctl), four._p(four.lin_loc), four._p(four.lin), s), "lm_linearize")
        check(lib.suo_ba_lm_schur_dev(four._h, four._p(four.ctl), four._p(four.lin), four._p(four.sch), s), "lm_schur")
        check(lib.suo_ba_lm_solve_update_dev(four._h, 1, 1, four._p(four.ctl), four._p(four.lin), four._p(four.sch), four._p(four.red), s), "lm_solve_update")
        check(lib.suo_ba_lm_decide_dev(four._h, four._p(four.ctl), four._p(four.red), s), "lm_decide")
        assert _same_bits(_host(four.ctl), want), f"unit {k}: the four calls and the folded call part"


def test_zz_observed_ratios():
    """Prints the worst |kernel - mp| / (eps M) per buffer this run has seen (the record of the module docstring); holds nothing the tests above do not."""
    print("observed (all tests) " + "  ".join(f"{b} {v:.3g} (K {R.K[b]:g})" for b, v in _seen.items()))
