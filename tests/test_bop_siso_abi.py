"""suo_pose_errors_points and suo_pose_errors_masks (row N4) are declared in include/suo_hip.h with their definitions written out, exported by libsuo_hip.so and
typed in suo_slam_amd/_lib.py, and refuse a call without a database before anything touches a device (no GPU needed).  The rules that need a live database
-- a model index out of range, a model without faces -- are in tests/test_gpu_points_errors.py and tests/test_gpu_masks_errors.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
EXPECTED = {
    "suo_pose_errors_points": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, C.c_int, VP, VP, VP]),
    "suo_pose_errors_masks": (C.c_int, [VP, C.c_int, VP, VP, VP, VP, C.c_int, C.c_int, VP, VP, VP]),
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
    assert re.search(r"int suo_pose_errors_points\(void\* mesh_db, int n, const int\* model_index, const double\* T_est, const double\* T_gt, const double\* K, "
                     r"int which,\s*double\* add_out, double\* adi_out, double\* proj_out\);", hdr)
    assert re.search(r"int suo_pose_errors_masks\(void\* mesh_db, int n, const int\* model_index, const double\* T_est, const double\* T_gt, const double\* K, "
                     r"int width, int height,\s*long long\* counts_out[^;]*int\* box_est[^;]*int\* box_gt[^;]*\);", hdr)
    doc = hdr[hdr.index("point-set pose errors: ADD, ADI, PROJ"):hdr.index("int suo_pose_errors_points(")]
    for phrase in ("GROUND-TRUTH point the nearest ESTIMATED-pose point", "not this", "M = K [R|t] formed first", "depends on P alone", "the bits it has alone",
                   "= 0 exactly", "+inf for ADD and ADI", "z exactly 0", "does not pay for it", "No input makes the call fault"):
        assert phrase in doc, phrase
    for name, bit in (("SUO_POINTS_ADD", 1), ("SUO_POINTS_ADI", 2), ("SUO_POINTS_PROJ", 4)):
        assert re.search(rf"#define {name} {bit}\b", hdr), name
    doc = hdr[hdr.index("mask pose errors from two renders"):hdr.index("int suo_pose_errors_masks(")]
    for phrase in ("union", "intersection", "[xmin, ymin, xmax - xmin, ymax - ymin]", "[-1, -1, -1, -1]", "1.0 when union is 0", "raises on an empty mask",
                   "neither depth image is written to memory", "integers only", "do not depend on the batch"):
        assert phrase in doc, phrase


def test_the_bits_of_which_are_the_python_side_s():
    from suo_slam_amd import bop_eval
    assert bop_eval.POINT_ERROR_BITS == {"add": 1, "adi": 2, "proj": 4}


def test_both_refuse_a_call_without_a_database(lib):
    idx, T, K, out = np.zeros(2, np.int32), np.tile(np.eye(4)[:3].reshape(12), (2, 1)), np.tile(np.eye(3).reshape(9), (2, 1)), np.zeros(2)
    p = lambda a: a.ctypes.data
    assert lib.suo_pose_errors_points(None, 2, p(idx), p(T), p(T), p(K), 7, p(out), p(out), p(out)) == SUO_ERR_ARG
    assert b"suo_pose_errors_points: bad argument" in lib.suo_last_error()
    assert lib.suo_pose_errors_points(None, 0, None, None, None, None, 0, None, None, None) == SUO_ERR_ARG
    counts, box = np.zeros((2, 2), np.int64), np.zeros((2, 4), np.int32)
    assert lib.suo_pose_errors_masks(None, 2, p(idx), p(T), p(T), p(K), 160, 96, p(counts), p(box), p(box)) == SUO_ERR_ARG
    assert b"suo_pose_errors_masks: null mesh database" in lib.suo_last_error()
    assert np.all(out == 0) and np.all(counts == 0)
