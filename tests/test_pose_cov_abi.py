"""The pose-covariance entry points are declared in include/suo_hip.h, exported by libsuo_hip.so and typed in suo_slam_amd/_lib.py (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
EXPECTED = {
    "suo_pose_covariances": (C.c_int, [VP, VP, VP, VP]),
    "suo_pose_covariances_batch": (C.c_int, [VP, C.c_int, VP, VP, VP]),
    "suo_frame_geom_covariances": (C.c_int, [VP, VP]),
}


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


def test_header_declares_the_entries_and_the_result_field():
    hdr = open(os.path.join(ROOT, "include", "suo_hip.h")).read()
    assert re.search(r"int suo_pose_covariances\(const suo_ba_problem\* problem, double\* cam_cov[^;]*double\* obj_cov[^;]*int\* status[^;]*\);", hdr)
    assert re.search(r"int suo_pose_covariances_batch\(const suo_ba_problem\* problems, int n, double\* const\* cam_cov, double\* const\* obj_cov, int\* status[^;]*\);", hdr)
    assert "int suo_frame_geom_covariances(suo_frame_geom* g, void* stream);" in hdr
    res = hdr[hdr.index("typedef struct suo_frame_geom_result"):hdr.index("} suo_frame_geom_result;")]
    assert "const double* obj_cov;" in res


def test_result_mirror_ends_with_obj_cov():
    from suo_slam_amd import _lib
    assert _lib.FrameGeomResult._fields_[-1] == ("obj_cov", VP)


def test_null_and_empty_arguments_are_refused_without_a_device(lib):
    from suo_slam_amd import _lib
    assert lib.suo_pose_covariances(None, None, None, None) == 1
    assert lib.suo_pose_covariances_batch(None, 0, None, None, None) == 0
    assert lib.suo_frame_geom_covariances(None, None) == 1
    assert b"null" in lib.suo_last_error()
