"""The partition the C driver of the multi-rank bundle adjustment makes (csrc/ba_drive.hip: suo_ba_split, behind suo_optimize_dist) is the one
suo_slam_amd/ba_dist.py: split_problem makes: camera c to rank c % world, local camera indices in ascending global order, the edges of the rank's cameras in
the caller's order.  Host only: no GPU."""
import ctypes as C

import numpy as np
import pytest

from suo_slam_amd import _lib, ba, ba_dist
from tests.ba_route_cases import KEYS, global_graph

GRAPHS = {"7x5": (11, 300, 7, 5, 0.3), "32x16": (12, 2000, 32, 16, 0.15), "5x3": (13, 90, 5, 3, 0.4)}      # seed, edges, cameras, objects, unseen pairs


def _c_split(full, rank, world):
    lib = _lib.lib()
    s = _lib.BaProblem()
    full._fill(s)
    cams = np.full(len(full.cam_T) + 1, -7, np.int32)
    edges = np.full(len(full.edge_cam) + 1, -7, np.int32)
    n_cams, n_edges = C.c_int(-1), C.c_int(-1)
    _lib.check(lib.suo_ba_split(C.byref(s), rank, world, cams.ctypes.data, C.byref(n_cams), edges.ctypes.data, C.byref(n_edges)), "suo_ba_split")
    assert cams[n_cams.value:].tolist() == [-7] * (len(cams) - n_cams.value) and edges[n_edges.value:].tolist() == [-7] * (len(edges) - n_edges.value)
    return cams[:n_cams.value].tolist(), edges[:n_edges.value].tolist()


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_c_split_equals_split_problem(name, world):
    seed, total, n_cam, n_obj, miss = GRAPHS[name]
    P = global_graph(np.random.default_rng(seed), total, n_cam, n_obj, miss=miss)
    # the builder emits edges camera by camera: shuffle them, so that "the caller's order" is not "sorted by camera"
    perm = np.random.default_rng(seed + 100).permutation(len(P["edge_cam"]))
    for k in KEYS:
        if k.startswith("edge_"):
            P[k] = P[k][perm]
    full = ba.Problem(*[P[k] for k in KEYS])
    assert (np.bincount(full.edge_cam * n_obj + full.edge_obj, minlength=n_cam * n_obj) == 0).any()          # a graph with missing (camera, object) pairs
    seen_cams, seen_edges = [], []
    for rank in range(world):
        local, cams, sel = ba_dist.split_problem(full, rank, world)
        c_cams, c_edges = _c_split(full, rank, world)
        assert c_cams == list(cams)
        assert c_edges == sel.tolist()
        # local camera index = position in the ascending camera list
        assert [c_cams.index(int(full.edge_cam[e])) for e in c_edges] == local.edge_cam.tolist()
        seen_cams += c_cams
        seen_edges += c_edges
    assert sorted(seen_cams) == list(range(n_cam)) and sorted(seen_edges) == list(range(len(full.edge_cam)))
    if world > n_cam:
        assert _c_split(full, world - 1, world) == ([], [])                                                 # a rank that owns no camera


def test_split_rejects_bad_arguments():
    P = global_graph(np.random.default_rng(3), 60, 3, 2, miss=0.0)
    full = ba.Problem(*[P[k] for k in KEYS])
    for rank, world in [(0, 0), (2, 2), (-1, 2)]:
        with pytest.raises(_lib.SuoError, match="rank"):
            _c_split(full, rank, world)
    full.edge_cam[5] = 3
    with pytest.raises(_lib.SuoError, match="missing camera"):
        _c_split(full, 0, 2)


def test_units_per_look_constant_lives_in_the_library():
    lib = _lib.lib()
    assert lib.suo_ba_units_per_look(1) == 12 and [lib.suo_ba_units_per_look(w) for w in (2, 4, 8)] == [6, 6, 6]


def test_communicator_errors_need_no_gpu_and_no_rccl():
    """The library loads where no RCCL is on the loader path (it is resolved with dlopen at first use); the local backend's limits and a missing RCCL are error
    codes with a message.  (The child is a process without torch, so that no RCCL copy is mapped when SUO_RCCL_LIB is looked at.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = _lib.lib()
    for world in (0, 17):
        h = C.c_void_p()
        with pytest.raises(_lib.SuoError, match="ranks"):
            _lib.check(lib.suo_ba_comm_create_local(world, C.byref(h)), "suo_ba_comm_create_local")
    h = C.c_void_p()
    _lib.check(lib.suo_ba_comm_create_local(3, C.byref(h)), "suo_ba_comm_create_local")
    assert (lib.suo_ba_comm_rank(h), lib.suo_ba_comm_world(h), lib.suo_ba_comm_calls(h)) == (0, 3, 0)
    lib.suo_ba_comm_destroy(h)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "ba_dist_c_child.py"), "bad_rccl_path"], cwd=root, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, SUO_RCCL_LIB="/nonexistent/librccl.so.1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("BA_DIST_C ")][-1].split(" ", 1)[1])
    assert out["unique_id_rc"] == 3 and "/nonexistent/librccl.so.1" in out["unique_id_msg"] and out["handle_null"], out
