"""The SE(3) update of the LM kernels -- pose_from_T, pose_oplus (all three coefficient branches), R_to_q (all four forms, both sign canonicalisations) and
pose_to_T of csrc/lm_device.h, reached through suo_debug_pose_oplus -- against the mpmath reference of tests/se3_ref.py over the designed table of
tests/se3_cases.py, in ONE launch.

The bound is not a literal: 4 x the worst error of orc_pose_oplus (oracle/lm_oracle.c) against the same reference over the rows with |omega| >= 0.3, computed here on
the same inputs (about 3.6e-15 for dR and 4.4e-15 for dt relative to max(1, |t_ref|_inf)).  The factor 4 pays for rsqrt_nr (1-2 ulp at each of its three sites, where
the oracle divides by a correctly rounded root), the explicit fma of the Taylor series and the hand-expanded Om^2.  It is applied to EVERY row: in the Taylor range
the kernel must not show the cancellation the oracle's closed forms have there (dt 1.5e-12 at 1e-5 rad).  Below the band around 1e-5 rad the target is g2o's shortcut
restated in mp, which is what that branch is meant to compute.

Measured on an MI355X, worst dR / dt per class of |omega|, kernel | oracle (bound: dR 3.55e-15, dt 4.37e-15):
    < 1e-5 (shortcut)   8.9e-16 / 2.2e-16 | 6.7e-16 / 2.2e-16        1e-5 .. 1e-3    6.7e-16 / 2.3e-16 | 4.4e-16 / 1.5e-12
    1e-3 .. 0.1         6.7e-16 / 2.1e-16 | 6.7e-16 / 8.0e-15        0.1 .. 0.3      8.9e-16 / 2.7e-16 | 6.7e-16 / 6.4e-16
    0.3 .. 2pi/3        8.9e-16 / 8.8e-16 | 8.9e-16 / 6.6e-16        2pi/3 .. pi     6.7e-16 / 6.0e-16 | 8.9e-16 / 6.5e-16
    >= pi               8.9e-16 / 8.2e-16 | 8.3e-16 / 1.1e-15
R R^T - I and det - 1 1.1e-15, |q| - 1 1.1e-16, R(q) - R 0, u = 0: 7.8e-16 / 0, round trip 8.9e-16 / 9.8e-16.  With the th^2 coefficient of c's series set to
-1/121 the test fails by dt 6.3e-7 (row |omega| = 0.3 (1 - 1e-9)); with the sign of v[k] flipped in R_to_q's trace <= 0 form by dR 2.0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import se3_cases as SC  # noqa: E402
from tests import se3_ref as SR  # noqa: E402


def _oplus(T, u, want_q=True):
    from suo_slam_amd import _lib
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1, 12))
    u = np.ascontiguousarray(np.asarray(u, np.float64).reshape(-1, 6))
    n = len(T)
    out = np.full((n, 12), np.nan)
    q = np.full((n, 4), np.nan)
    _lib.check(_lib.lib().suo_debug_pose_oplus(T.ctypes.data, u.ctypes.data, n, out.ctypes.data, q.ctypes.data if want_q else None), "suo_debug_pose_oplus")
    return out.reshape(n, 3, 4), q


@pytest.fixture(scope="module")
def run():
    """The one launch over the table, the references and the bound."""
    from suo_slam_amd import _lib
    _lib.require_gpu()
    T_out, q = _oplus(SC.T_IN, SC.U)
    ex, target = SC.references()
    oR, ot = SC.errors(SC.oracle_oplus(SC.T_IN, SC.U), target)
    b = SC.bound_rows()
    assert b.sum() >= 200
    bound_R, bound_t = 4 * oR[b].max(), 4 * ot[b].max()
    assert 0 < bound_R < 1e-14 and 0 < bound_t < 1e-14           # (tests/test_se3_ref.py holds the oracle within 8 ulp there: the bound cannot drift wide)
    return {"T": T_out, "q": q, "target": target, "oR": oR, "ot": ot, "bR": bound_R, "bt": bound_t}


def _worst(v, why=SC.WHY):
    i = int(np.argmax(v))
    return f"row {i} ({why[i]}): {v[i]:.3e}"


def test_bad_arguments_launch_nothing():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    lib = _lib.lib()
    T, u, out = np.zeros(12), np.zeros(6), np.full(12, 7.0)
    assert lib.suo_debug_pose_oplus(T.ctypes.data, u.ctypes.data, 0, out.ctypes.data, None) != 0
    assert lib.suo_debug_pose_oplus(T.ctypes.data, u.ctypes.data, -3, out.ctypes.data, None) != 0
    assert lib.suo_debug_pose_oplus(None, u.ctypes.data, 1, out.ctypes.data, None) != 0
    assert lib.suo_debug_pose_oplus(T.ctypes.data, None, 1, out.ctypes.data, None) != 0
    assert lib.suo_debug_pose_oplus(T.ctypes.data, u.ctypes.data, 1, None, None) != 0
    assert (out == 7.0).all()
    a, _ = _oplus(SC.T_IN[:70], SC.U[:70], want_q=False)                           # q_out may be NULL; more than one block
    b, _ = _oplus(SC.T_IN[:70], SC.U[:70])
    assert np.array_equal(a, b)


def test_update_matches_the_mp_reference(run):
    dR, dt = SC.errors(run["T"], run["target"])
    print(SC.report("kernel (pose_from_T, pose_oplus, pose_to_T) against the mp reference", dR, dt))
    print(SC.report("orc_pose_oplus against the mp reference", run["oR"], run["ot"]))
    print(f"bound (4 x the oracle's worst over |omega| >= 0.3): dR {run['bR']:.3e}  dt {run['bt']:.3e}")
    for name, m in (("shortcut", SC.SHORTCUT), ("Taylor", SC.TAYLOR), ("closed forms", SC.CLOSED)):
        print(f"  branch {name:12s} rows {int(m.sum()):4d}  dR {dR[m].max():.2e}  dt {dt[m].max():.2e}")
    assert np.isfinite(run["T"]).all() and np.isfinite(run["q"]).all()
    assert dR.max() <= run["bR"], _worst(dR)
    assert dt.max() <= run["bt"], _worst(dt)


def test_output_is_a_rotation_and_its_quaternion(run):
    T, q, bR = run["T"], run["q"], run["bR"]
    R = T[:, :, :3]
    orth = np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max((1, 2))
    det = np.abs(np.linalg.det(R) - 1.0)
    qn = np.abs(np.sqrt((q * q).sum(1)) - 1.0)
    rebuilt = np.abs(np.stack([SR.quat_to_R(x) for x in q]) - R).max((1, 2))
    print(f"R R^T - I {orth.max():.2e}  det - 1 {det.max():.2e}  |q| - 1 {qn.max():.2e}  R(q) - R {rebuilt.max():.2e}  min w {q[:, 0].min():.3e}  (bound {bR:.3e})")
    assert orth.max() <= bR, _worst(orth)
    assert det.max() <= bR, _worst(det)
    assert qn.max() <= bR, _worst(qn)
    assert (q[:, 0] >= 0).all(), _worst(-q[:, 0])
    assert rebuilt.max() <= bR, _worst(rebuilt)


def test_zero_update_returns_the_pose(run):
    T, _ = _oplus(SC.T_IN, np.zeros_like(SC.U))
    dR, dt = SC.errors(T, SC.T_IN)
    print(f"u = 0: dR {dR.max():.2e}  dt {dt.max():.2e}")
    assert dR.max() <= run["bR"], _worst(dR)
    assert dt.max() <= run["bt"], _worst(dt)


def test_update_and_its_inverse_return_the_pose(run):
    """oplus(oplus(T, u), -u) = T to 4 x the bound, for 1e-5 < |omega| < pi and for omega = 0.  (Below 1e-5 rad the shortcut's V = I + Om + Om^2 is no
    homomorphism: V(-w) (-ups) + R(-w) V(w) ups = Om ups + O(th^2), off by th |upsilon| by g2o's own definition; that branch is held to the mp restatement above.)
    Each of the two updates errs relative to the larger of 1 and ITS result's translation, so dt is taken relative to max(1, |t|_inf, |t_mid|_inf)."""
    m = ((SC.ANGLE > 1e-5) & (SC.ANGLE < np.pi)) | (np.abs(SC.U[:, :3]).max(1) == 0)
    assert m.sum() >= 300
    mid = run["T"][m]
    back, _ = _oplus(mid, -SC.U[m])
    T0 = SC.T_IN[m]
    dR = np.abs(back[:, :, :3] - T0[:, :, :3]).max((1, 2))
    scale = np.maximum(1.0, np.maximum(np.abs(T0[:, :, 3]).max(1), np.abs(mid[:, :, 3]).max(1)))
    dt = np.abs(back[:, :, 3] - T0[:, :, 3]).max(1) / scale
    why = [SC.WHY[i] for i in np.flatnonzero(m)]
    print(f"round trip over {int(m.sum())} rows: dR {dR.max():.2e}  dt {dt.max():.2e}  (bounds {4 * run['bR']:.3e}, {4 * run['bt']:.3e})")
    assert dR.max() <= 4 * run["bR"], _worst(dR, why)
    assert dt.max() <= 4 * run["bt"], _worst(dt, why)
