"""suo_pose_nees and suo_keypoint_nees are declared in include/suo_hip.h, exported by libsuo_hip.so and typed in suo_slam_amd/_lib.py, and refuse what the
header says they refuse before anything touches a device (no GPU needed).  The one rule that needs a live database -- a model index at or past n_models -- is in
tests/test_gpu_nees.py; a negative index is outside every database and is refused here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
EXPECTED = {
    "suo_pose_nees": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, VP, VP, VP, VP]),
    "suo_keypoint_nees": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, VP, VP, VP]),
}
SUO_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from suo_slam_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_symbol_is_exported_and_typed(lib, name):
    from suo_slam_amd import _lib
    assert name in _lib.SIGNATURES, f"{name} is not declared in suo_slam_amd/_lib.py"
    assert _lib.SIGNATURES[name] == EXPECTED[name]
    fn = getattr(lib, name)
    assert fn.restype == EXPECTED[name][0] and list(fn.argtypes) == EXPECTED[name][1]


def test_header_declares_the_entries_and_states_the_rules():
    hdr = open(os.path.join(ROOT, "include", "suo_hip.h")).read()
    assert re.search(r"int suo_pose_nees\(void\* mesh_db, int n, const int\* model_index, const double\* T_est[^;]*const double\* T_gt[^;]*const double\* cov[^;]*"
                     r"double\* nees[^;]*double\* xi[^;]*int\* sym_index[^;]*double\* T_ref[^;]*int\* status[^;]*\);", hdr)
    assert re.search(r"int suo_keypoint_nees\(void\* mesh_db[^;]*int n_det, const int\* n_pts, const double\* model_kp[^;]*const double\* uv[^;]*const double\* cov[^;]*"
                     r"const double\* K[^;]*const double\* T_ref[^;]*double\* chi2[^;]*double\* err[^;]*\);", hdr)
    doc = hdr[hdr.index("pose NEES and keypoint chi2"):hdr.index("int suo_pose_nees(")]
    for phrase in ("LOWEST index", "3.0 rad", "NOT applied", "ONE length unit", "non-finite entry", "pivot that is not positive", "sym_index -1", "det C <= 0"):
        assert phrase in doc, phrase


def _pose_args(n, model=0):
    return (np.full(max(n, 1), model, np.int32), np.tile(np.eye(4)[:3].reshape(12), (max(n, 1), 1)), np.tile(np.eye(4)[:3].reshape(12), (max(n, 1), 1)),
            np.tile(np.eye(6).reshape(36), (max(n, 1), 1)), np.zeros(max(n, 1)))


def test_pose_nees_refuses_bad_arguments_without_a_device(lib):
    idx, Te, Tg, cov, out = _pose_args(2)
    p = lambda a: a.ctypes.data
    assert lib.suo_pose_nees(None, 2, p(idx), p(Te), p(Tg), p(cov), p(out), None, None, None, None) == SUO_ERR_ARG
    assert b"null mesh database" in lib.suo_last_error()
    assert lib.suo_pose_nees(None, 0, None, None, None, None, None, None, None, None, None) == SUO_ERR_ARG
    assert b"null mesh database" in lib.suo_last_error()
    assert lib.suo_pose_nees(None, -1, p(idx), p(Te), p(Tg), p(cov), p(out), None, None, None, None) == SUO_ERR_ARG
    assert b"negative" in lib.suo_last_error()
    for hole in range(5):
        a = [p(idx), p(Te), p(Tg), p(cov), p(out)]
        a[hole] = None
        assert lib.suo_pose_nees(None, 2, *a, None, None, None, None) == SUO_ERR_ARG
        assert b"null model_index, T_est, T_gt, cov or nees" in lib.suo_last_error()
    idx[1] = -1
    assert lib.suo_pose_nees(None, 2, p(idx), p(Te), p(Tg), p(cov), p(out), None, None, None, None) == SUO_ERR_ARG
    assert b"model_index[1]=-1 out of range" in lib.suo_last_error()
    assert np.all(out == 0)


def test_keypoint_nees_refuses_bad_arguments_without_a_device(lib):
    n_pts = np.array([2, 1], np.int32)
    kp, uv, cov, K, T, out = np.zeros((3, 3)), np.zeros((3, 2)), np.tile(np.eye(2).reshape(4), (3, 1)), np.tile(np.eye(3).reshape(9), (2, 1)), \
        np.tile(np.eye(4)[:3].reshape(12), (2, 1)), np.zeros(3)
    p = lambda a: a.ctypes.data
    assert lib.suo_keypoint_nees(None, 2, p(n_pts), p(kp), p(uv), p(cov), p(K), p(T), p(out), None) == SUO_ERR_ARG
    assert b"null mesh database" in lib.suo_last_error()
    assert lib.suo_keypoint_nees(None, 0, None, None, None, None, None, None, None, None) == SUO_ERR_ARG
    assert b"null mesh database" in lib.suo_last_error()
    assert lib.suo_keypoint_nees(None, -3, p(n_pts), p(kp), p(uv), p(cov), p(K), p(T), p(out), None) == SUO_ERR_ARG
    assert b"negative" in lib.suo_last_error()
    assert lib.suo_keypoint_nees(None, 2, None, p(kp), p(uv), p(cov), p(K), p(T), p(out), None) == SUO_ERR_ARG
    assert b"null n_pts" in lib.suo_last_error()
    for hole in range(6):
        a = [p(kp), p(uv), p(cov), p(K), p(T), p(out)]
        a[hole] = None
        assert lib.suo_keypoint_nees(None, 2, p(n_pts), *a, None) == SUO_ERR_ARG
        assert b"null model_kp, uv, cov, K, T_ref or chi2" in lib.suo_last_error()
    n_pts[1] = -1
    assert lib.suo_keypoint_nees(None, 2, p(n_pts), p(kp), p(uv), p(cov), p(K), p(T), p(out), None) == SUO_ERR_ARG
    assert b"n_pts[1]=-1 is negative" in lib.suo_last_error()
    assert np.all(out == 0)
