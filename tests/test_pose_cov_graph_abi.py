"""The graph entries of the pose covariances are declared in include/suo_hip.h, exported, typed in suo_slam_amd/_lib.py, and refuse bad arguments and maps over
the cap before anything touches a device (no GPU needed).  The old entries keep their two refusals in the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
EXPECTED = {
    "suo_pose_covariances_graph": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, VP, VP]),
    "suo_pose_covariances_graph_batch": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, VP, VP, VP, VP]),
}
CAP = 64


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


def test_header_declares_the_entries_the_camera_pair_formulas_and_the_cap():
    hdr = open(os.path.join(ROOT, "include", "suo_hip.h")).read()
    assert re.search(r"int suo_pose_covariances_graph\(const suo_ba_problem\* problem, int n_pair, const int32_t\* pair_a, const int32_t\* pair_b, double\* cam_cov[^;]*"
                     r"double\* obj_cov[^;]*double\* cross[^;]*double\* rel[^;]*int\* status[^;]*\);", hdr)
    assert re.search(r"int suo_pose_covariances_graph_batch\(const suo_ba_problem\* problems, int n, const int\* n_pair,[^;]*int\* status[^;]*\);", hdr)
    for text in ("T_AtoB = T_b * T_a^-1", "delta_rel = delta_b - A delta_a", "A = Ad(T_b T_a^-1)", "rel = Sigma_bb + A Sigma_aa A^T - A Sigma_ab - Sigma_ba A^T",
                 "cross = Sigma_ab: rows are vertex a, columns are vertex b", f"#define SUO_POSE_COV_GRAPH_MAX_OBJ {CAP}", "rel is 36 zeros exactly",
                 "(a, b) is the transpose of (b, a) to the bit"):
        assert text in hdr, text
    # the old entries still refuse, in the words their tests match
    assert "(camera, camera): SUO_ERR_ARG" in hdr and "free cameras next to more than 16 free objects                SUO_ERR_ARG" in hdr


def test_bad_arguments_and_a_map_over_the_cap_are_refused_without_a_device(lib):
    from suo_slam_amd import _lib, ba
    from tests import pose_cov_cases as K
    assert lib.suo_pose_covariances_graph(None, 0, None, None, None, None, None, None, None) == 1 and b"null" in lib.suo_last_error()
    assert lib.suo_pose_covariances_graph_batch(None, 0, None, None, None, None, None, None, None, None) == 0
    assert lib.suo_pose_covariances_graph_batch(None, 1, None, None, None, None, None, None, None, None) == 1 and b"null" in lib.suo_last_error()
    g = K.CASES["3x2"]()                                   # 3 cameras, 2 objects: vertices 0..4
    s = _lib.BaProblem()
    p = ba.Problem(*K.args(g))
    p._fill(s)
    for a, b, n, text in (([0], [5], 1, b"outside"), ([-1], [3], 1, b"outside"), ([0, 1], [1, 7], 2, b"outside"), ([0], [3], -1, b"n_pair"), ([0], [3], 1, None)):
        pa, pb = np.array(a, np.int32), np.array(b, np.int32)
        if text is None:
            pa = pb = None                                 # a count without the lists
            text = b"null pair lists"
        rc = lib.suo_pose_covariances_graph(C.byref(s), n, None if pa is None else pa.ctypes.data, None if pb is None else pb.ctypes.data, None, None, None, None, None)
        assert rc == 1 and text in lib.suo_last_error() and b"suo_pose_covariances_graph" in lib.suo_last_error(), (a, b, n, lib.suo_last_error())
    over = K.coupled(40, 2, CAP + 1, kp=(4, 4))
    p_over = ba.Problem(*K.args(over))
    p_over._fill(s)
    one = np.array([0], np.int32), np.array([1], np.int32)
    assert lib.suo_pose_covariances_graph(C.byref(s), 1, one[0].ctypes.data, one[1].ctypes.data, None, None, None, None, None) == 1
    err = lib.suo_last_error()
    assert f"{CAP + 1} free objects".encode() in err and f"at most {CAP}".encode() in err, err
