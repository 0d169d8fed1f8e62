"""tests/se3_ref.py (the SE(3) update in mpmath at 50 digits) held against exponentials computed other ways, and the project's two transcriptions of se3quat.h --
orc_pose_oplus (oracle/lm_oracle.c) and tests/ba_numpy_phases._exp -- measured against it over the case table of tests/se3_cases.py.  No GPU."""
import numpy as np
import scipy.linalg
from scipy.spatial.transform import Rotation

from tests import se3_cases as SC
from tests import se3_ref as SR
from tests.ba_numpy_phases import _exp

EPS = 2.0 ** -52


def _twist(u):
    X = np.zeros((4, 4))
    w = u[:3]
    X[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    X[:3, 3] = u[3:]
    return X


def test_table_covers_what_it_claims():
    th = SC.ANGLE
    assert 300 <= len(SC.ROWS) <= 1000
    assert not ((th >= SC.BAND[0]) & (th <= SC.BAND[1])).any()                       # nothing inside the band around 1e-5
    assert np.array_equal(SC.SHORTCUT, th < 1e-5)                                    # so th^2 < 1e-10 and th < 1e-5 are the same rows
    wmax = np.abs(SC.U[:, :3]).max(1)
    assert (wmax == 0).any() and ((wmax > 0) & (SC.TH2 == 0)).any() and ((SC.TH2 > 0) & (SC.TH2 < 2.3e-308)).any()       # 0; th^2 underflows to 0, to a denormal
    assert ((th > 1e-5) & (th < 1.1e-5)).any() and ((th < 1e-5) & (th > 0.9e-5)).any()
    for lo, hi in ((0.3 * (1 - 2e-9), 0.3), (0.3, 0.3 * (1 + 2e-9)), (SC.TWO_PI_3 - 2e-9, SC.TWO_PI_3), (SC.TWO_PI_3, SC.TWO_PI_3 + 2e-9),
                   (np.pi - 2e-6, np.pi), (np.pi, np.pi + 2e-6), (2 * np.pi - 2e-6, 2 * np.pi), (6.9, 7.1)):
        assert ((th > lo) & (th < hi)).any() or (th == lo).any() or (th == hi).any(), (lo, hi)
    assert SC.SHORTCUT.sum() >= 50 and SC.TAYLOR.sum() >= 100 and SC.CLOSED.sum() >= 100
    assert ((SC.TH2 < 0.09) & (SC.TH2 > 0.09 * (1 - 1e-8))).any() and ((SC.TH2 >= 0.09) & (SC.TH2 < 0.09 * (1 + 1e-8))).any()
    R = SC.T_IN[:, :, :3]
    tr = np.trace(R, axis1=1, axis2=2)
    assert np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max() < 8 * EPS         # the inputs are rotations to rounding
    for i in range(3):                                                               # trace <= 0 with each diagonal entry the largest, exact half turns among them
        m = (tr <= 0) & (np.diagonal(R, axis1=1, axis2=2).argmax(1) == i)
        assert m.sum() >= 10, i
    for H in (np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])):
        assert (np.abs(R - H).max((1, 2)) == 0).any()
    assert (np.abs(R - np.eye(3)).max((1, 2)) == 0).any()
    tn = np.linalg.norm(SC.T_IN[:, :, 3], axis=1)
    for v in (0.0, 1.0, 1e3, 1e4):
        assert (np.abs(tn - v) <= 1e-9 * v).sum() >= 10
    # the product quaternion before the sign flip: w < 0 on some rows, |w| < 1e-15 on others
    q_in = np.array([Rotation.from_matrix(r).as_quat() for r in R])                 # (x, y, z, w)
    q_in *= np.where(q_in[:, 3] < 0, -1.0, 1.0)[:, None]                            # w >= 0, as R_to_q leaves it
    q_e = np.array([Rotation.from_rotvec(u[:3]).as_quat() for u in SC.U])
    q_e *= np.where(q_e[:, 3] < 0, -1.0, 1.0)[:, None]
    w_prod = q_e[:, 3] * q_in[:, 3] - (q_e[:, :3] * q_in[:, :3]).sum(1)
    assert (w_prod < -0.05).sum() >= 10 and (np.abs(w_prod) < 1e-15).sum() >= 10


def test_rodrigues_in_mp_is_mpmaths_own_expm():
    ex, _ = SC.references()
    xm = np.stack([SR.oplus_expm(T, u) for T, u in zip(SC.T_IN, SC.U)])
    dR, dt = SC.errors(xm, ex)
    print(f"Rodrigues in mp against mpmath.expm over {len(ex)} rows: dR {dR.max():.2e}  dt {dt.max():.2e}")
    assert dR.max() <= EPS and dt.max() <= EPS                                      # both are 50-digit values rounded once: the same float64 but for a tie


def test_against_scipy():
    """Rotation.from_rotvec on every row's omega, and scipy.linalg.expm of the 4x4 twist, to 1e-15.  scipy's Pade expm carries an error proportional to the norm
    of its argument (measured: 1.5e-14 at 7 rad, 4.8e-15 at 5 rad), so it is given the table's twists with |omega| <= 1 and |upsilon| <= 2; from_rotvec sees every angle."""
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
    worst_R = worst_X = 0.0
    n_x = 0
    for u in SC.U:
        mine = SR.oplus(I34, u)
        worst_R = max(worst_R, np.abs(Rotation.from_rotvec(u[:3]).as_matrix() - mine[:, :3]).max())
        if np.abs(u[3:]).max() <= 2.0 and np.linalg.norm(u[:3]) <= 1.0:
            X = scipy.linalg.expm(_twist(u))
            worst_X = max(worst_X, np.abs(X[:3] - mine).max())
            n_x += 1
    print(f"se3_ref against scipy: from_rotvec {worst_R:.2e} over {len(SC.U)} rows, linalg.expm {worst_X:.2e} over {n_x} rows")
    assert n_x >= 200
    assert worst_R < 1e-15 and worst_X < 1e-15


def test_shortcut_is_within_th2_of_the_exponential():
    """g2o's shortcut against the true exponential on the rows below the band: the rotation within th^2 (the normalised quaternion of I + Om + Om^2 is a rotation about omega by th to second order).
    Its V = R however is I + Om where the exponential has I + Om / 2: the translation is off by |omega x upsilon| / 2 to first order, which is no th^2 -- it is held
    within th |upsilon| + th^2 (|upsilon| + |t|)."""
    ex, target = SC.references()
    m = np.flatnonzero(SC.SHORTCUT)
    assert len(m) >= 50
    for i in m:
        th, ups, t = SC.ANGLE[i], np.linalg.norm(SC.U[i, 3:]), np.linalg.norm(SC.T_IN[i, :, 3])
        assert np.abs(target[i, :, :3] - ex[i, :, :3]).max() <= th * th + EPS, SC.WHY[i]
        assert np.abs(target[i, :, 3] - ex[i, :, 3]).max() <= th * ups + th * th * (ups + t) + EPS * max(1.0, t, ups), SC.WHY[i]
    # and it is NOT the exponential: on some row the translation is off by a good part of th |upsilon|
    rel = [np.abs(target[i, :, 3] - ex[i, :, 3]).max() / (SC.ANGLE[i] * np.linalg.norm(SC.U[i, 3:])) for i in m if SC.ANGLE[i] > 1e-7 and np.linalg.norm(SC.U[i, 3:]) > 0]
    assert max(rel) > 0.2


def test_transcriptions_measured_against_the_mp_reference():
    """orc_pose_oplus and ba_numpy_phases._exp over the table, worst values per angle class (printed).  Held: on the rows with |omega| >= 0.3 -- where the GPU test
    takes its bound from -- the oracle is within 8 ulp of one; the growth of dt below that is cancellation in the closed-form b and c, a property of the oracle."""
    _, target = SC.references()
    orc = SC.oracle_oplus(SC.T_IN, SC.U)
    dR, dt = SC.errors(orc, target)
    print(SC.report("orc_pose_oplus against the mp reference", dR, dt))
    num = np.stack([(_exp(u) @ np.vstack([T, [0, 0, 0, 1]]))[:3] for T, u in zip(SC.T_IN, SC.U)])
    nR, nt = SC.errors(num[~SC.SHORTCUT], target[~SC.SHORTCUT])
    full_R, full_t = np.zeros(len(dR)), np.zeros(len(dR))
    full_R[~SC.SHORTCUT], full_t[~SC.SHORTCUT] = nR, nt
    print(SC.report("ba_numpy_phases._exp (times T, no quaternion) against the mp reference, rows above the band", full_R, full_t, ~SC.SHORTCUT))
    b = SC.bound_rows()
    print(f"bound of tests/test_gpu_se3_update.py: dR {4 * dR[b].max():.3e}  dt {4 * dt[b].max():.3e}")
    assert np.isfinite(orc).all()
    assert dR[b].max() < 8 * EPS and dt[b].max() < 8 * EPS
    assert dR.max() < 8 * EPS                                                        # the rotation everywhere, the shortcut rows (against the shortcut in mp) included
    assert nR[SC.ANGLE[~SC.SHORTCUT] >= 0.3].max() < 8 * EPS and nt[SC.ANGLE[~SC.SHORTCUT] >= 0.3].max() < 8 * EPS
