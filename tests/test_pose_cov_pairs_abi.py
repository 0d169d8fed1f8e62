"""The pair entries of the pose covariances are declared in include/suo_hip.h, exported, typed in suo_slam_amd/_lib.py, and refuse bad pairs before anything touches
a device (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
EXPECTED = {
    "suo_pose_covariances_pairs": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, VP, VP]),
    "suo_pose_covariances_pairs_batch": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, VP, VP, VP]),
}


@pytest.fixture(scope="module")
def lib():
    from suo_slam_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_symbol_is_exported_and_typed(lib, name):
    from suo_slam_amd import _lib
    assert _lib.SIGNATURES[name] == EXPECTED[name]
    fn = getattr(lib, name)
    assert fn.restype == EXPECTED[name][0] and list(fn.argtypes) == EXPECTED[name][1]


def test_header_declares_the_entries_and_the_conventions():
    hdr = open(os.path.join(ROOT, "include", "suo_hip.h")).read()
    assert re.search(r"int suo_pose_covariances_pairs\(const suo_ba_problem\* problem, int n_pair, const int32_t\* pair_a, const int32_t\* pair_b, double\* cam_cov[^;]*"
                     r"double\* obj_cov[^;]*double\* cross[^;]*double\* rel[^;]*int\* status[^;]*\);", hdr)
    assert re.search(r"int suo_pose_covariances_pairs_batch\(const suo_ba_problem\* problems, int n, const int\* n_pair,[^;]*int\* status[^;]*\);", hdr)
    for text in ("camera c is c, object o is n_cam + o", "Ad(T) = [[R, 0], [[t]x R, R]]", "T_OtoC = T_c * T_o", "T_AtoB = T_b^-1 * T_a", "(camera, camera): SUO_ERR_ARG"):
        assert text in hdr, text


def test_bad_arguments_are_refused_without_a_device(lib):
    from suo_slam_amd import _lib, ba
    from tests import pose_cov_cases as K
    assert lib.suo_pose_covariances_pairs(None, 0, None, None, None, None, None, None, None) == 1 and b"null" in lib.suo_last_error()
    assert lib.suo_pose_covariances_pairs_batch(None, 0, None, None, None, None, None, None, None, None) == 0
    g = K.CASES["3x2"]()                                   # 3 cameras, 2 objects: vertices 0..4
    s = _lib.BaProblem()
    p = ba.Problem(*K.args(g))
    p._fill(s)
    for a, b, n, text in (([0], [5], 1, b"outside"), ([-1], [3], 1, b"outside"), ([0, 1], [3, 2], 2, b"camera, camera"), ([0], [3], -1, b"n_pair"), ([0], [3], 1, None)):
        pa, pb = np.array(a, np.int32), np.array(b, np.int32)
        if text is None:
            pa = pb = None                                 # a count without the lists
            text = b"null pair lists"
        rc = lib.suo_pose_covariances_pairs(C.byref(s), n, None if pa is None else pa.ctypes.data, None if pb is None else pb.ctypes.data, None, None, None, None, None)
        assert rc == 1 and text in lib.suo_last_error(), (a, b, n, lib.suo_last_error())
    g17 = K.CASES["2x17"]()
    p17 = ba.Problem(*K.args(g17))
    p17._fill(s)
    one = np.array([1], np.int32), np.array([2], np.int32)
    assert lib.suo_pose_covariances_pairs(C.byref(s), 1, one[0].ctypes.data, one[1].ctypes.data, None, None, None, None, None) == 1
    assert b"17 free objects" in lib.suo_last_error()
