"""suo_residual_statistics and its batch form are declared in include/suo_hip.h with the definitions they implement, exported, typed in suo_slam_amd/_lib.py, and
refuse what suo_pose_covariances_graph refuses before anything touches a device (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
EXPECTED = {
    "suo_residual_statistics": (C.c_int, [VP] * 11),
    "suo_residual_statistics_batch": (C.c_int, [VP, C.c_int] + [VP] * 10),
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


def test_header_declares_the_entries_and_states_the_definitions():
    hdr = open(os.path.join(ROOT, "include", "suo_hip.h")).read()
    assert re.search(r"int suo_residual_statistics\(const suo_ba_problem\* problem, double\* cam_cov[^;]*double\* obj_cov[^;]*double\* edge_chi2[^;]*double\* edge_pcov[^;]*"
                     r"double\* edge_lev[^;]*double\* edge_t[^;]*double\* cam_stat[^;]*double\* obj_stat[^;]*double\* summary[^;]*int\* status[^;]*\);", hdr)
    assert re.search(r"int suo_residual_statistics_batch\(const suo_ba_problem\* problems, int n, double\* const\* cam_cov,[^;]*double\* summary[^;]*int\* status[^;]*\);", hdr)
    for text in ("chi2_e       = v_e^T Omega_e v_e", "P_e          = J_e Sigma_e J_e^T", "lev_e        = tr(P_e Omega_e)", "sum lev_e = n exactly",
                 "t_e          = v_e^T (Omega_e^-1 + s P_e)^-1 v_e, s = -1 for a counted edge and s = +1 otherwise", "R_e = I + s P_e Omega_e", "det R_e <= 1e-9",
                 "The threshold is part of the rule, not a tolerance", "counted in status[2]", "counted in status[3]", "dof = 2 m - n", "s0^2 = sum chi2_e / dof",
                 "summary = {0, 0, 0, 0, 0, NaN}", "status [4] = NaN camera blocks, NaN object blocks, NaN edges, edges without redundancy",
                 "in ascending edge index"):
        assert text in hdr, text


def test_bad_arguments_and_a_map_over_the_cap_are_refused_without_a_device(lib):
    from suo_slam_amd import _lib, ba
    from tests import pose_cov_cases as K
    none = [None] * 10
    assert lib.suo_residual_statistics(None, *none) == 1 and b"null" in lib.suo_last_error()
    assert lib.suo_residual_statistics_batch(None, 0, *none) == 0
    assert lib.suo_residual_statistics_batch(None, 1, *none) == 1 and b"null" in lib.suo_last_error()
    g = K.CASES["3x2"]()
    s = _lib.BaProblem()
    p = ba.Problem(*K.args(g))
    # 65 free objects next to a free camera
    over = K.coupled(40, 2, CAP + 1, kp=(4, 4))
    p_over = ba.Problem(*K.args(over))
    p_over._fill(s)
    assert lib.suo_residual_statistics(C.byref(s), *none) == 1
    err = lib.suo_last_error()
    assert f"{CAP + 1} free objects".encode() in err and f"at most {CAP}".encode() in err and b"problem 0" in err, err
    # null flags, negative sizes: named by problem, in a batch by its position
    arr = (_lib.BaProblem * 2)()
    for field, value in (("cam_fixed", None), ("obj_fixed", None), ("n_cam", -1), ("n_obj", -1), ("n_edge", -1)):
        p._fill(arr[0])
        p._fill(arr[1])
        setattr(arr[1], field, value)
        assert lib.suo_residual_statistics_batch(C.cast(arr, VP), 2, *none) == 1, field
        err = lib.suo_last_error()
        assert b"problem 1" in err and (b"null flags" in err or b"bad sizes" in err), (field, err)
    # an edge that names a missing vertex, in the coupled form that needs the pair list first
    bad = ba.Problem(*K.args(g))
    bad.edge_obj[3] = 2
    bad._fill(s)
    assert lib.suo_residual_statistics(C.byref(s), *none) == 1 and b"edge 3 of problem 0 references a missing vertex" in lib.suo_last_error()
