"""Child processes of tests/test_gpu_ba_dist_c.py (each a fresh process under the parent's `timeout`).  Prints one JSON line.
  bad_rccl_path            no torch in the process (so no RCCL is mapped yet), SUO_RCCL_LIB names a file that does not exist: the RCCL entry points must
                           return an error code with a message
  rocm_rccl N_CAM N_OBJ    no torch in the process: RCCL comes from the loader path (ROCm's own copy, not PyTorch's); suo_optimize_dist with an RCCL
                           communicator of world 1 against suo_optimize
  two_ranks RANK PORT OUT  one of two real RCCL ranks (device = rank): optimize_distributed_c on 32 x 16, the result saved to OUT"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")


def _without_torch():
    sys.modules["torch"] = None                 # `import torch` raises ImportError: suo_slam_amd._lib then loads the library on the system's HIP runtime
    from suo_slam_amd import _lib, ba
    return _lib, ba


def bad_rccl_path():
    _lib, _ = _without_torch()
    lib = _lib.lib()
    ident = np.zeros(128, np.uint8)
    out = {"lib": os.environ.get("SUO_RCCL_LIB")}
    out["unique_id_rc"] = int(lib.suo_ba_comm_rccl_unique_id(ident.ctypes.data))
    out["unique_id_msg"] = lib.suo_last_error().decode()
    h = C.c_void_p()
    try:
        _lib.check(lib.suo_ba_comm_create_rccl(ident.ctypes.data, 0, 1, C.byref(h)), "suo_ba_comm_create_rccl")
        out["create"] = "no error"
    except _lib.SuoError as exc:
        out["create"] = str(exc)
    out["handle_null"] = not h.value
    print("BA_DIST_C " + json.dumps(out), flush=True)


def rocm_rccl(n_cam, n_obj):
    _lib, ba = _without_torch()
    from tests.ba_route_cases import global_graph
    lib = _lib.lib()
    _lib.require_gpu()
    P = global_graph(np.random.default_rng(7), 60 * n_cam, n_cam, n_obj)
    one = ba.Problem(*[P[k] for k in KEYS])
    ba.optimize_batch([one])
    ident = np.zeros(128, np.uint8)
    _lib.check(lib.suo_ba_comm_rccl_unique_id(ident.ctypes.data), "suo_ba_comm_rccl_unique_id")
    h = C.c_void_p()
    _lib.check(lib.suo_ba_comm_create_rccl(ident.ctypes.data, 0, 1, C.byref(h)), "suo_ba_comm_create_rccl")
    full = ba.Problem(*[P[k] for k in KEYS])
    s = _lib.BaProblem()
    full._fill(s)
    _lib.check(lib.suo_optimize_dist(C.byref(s), h), "suo_optimize_dist")
    full.stats[:] = list(s.stats)
    calls = int(lib.suo_ba_comm_calls(h))
    lib.suo_ba_comm_destroy(h)
    maps = open("/proc/self/maps").read()
    out = {"calls": calls, "stats": [int(v) for v in full.stats], "torch_loaded": "torch" in maps,
           "rccl": sorted({ln.split()[-1] for ln in maps.splitlines() if "librccl" in ln}),
           "identical": {k: bool(np.array_equal(getattr(full, k)[:len(getattr(one, k))], getattr(one, k))) for k in ("cam_T", "obj_T", "inlier", "chi2", "stats")}}
    print("BA_DIST_C " + json.dumps(out), flush=True)


def two_ranks(rank, port, path):
    import torch
    import torch.distributed as dist
    from suo_slam_amd import ba, ba_dist
    from tests.test_gpu_geometry import _multi_view_scene
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    P, _ = _multi_view_scene(np.random.default_rng(7), 32, 16)
    full = ba_dist.optimize_distributed_c(ba.Problem(*[P[k] for k in KEYS]))
    calls = ba_dist.group_comm().calls
    np.savez(path, cam_T=full.cam_T, obj_T=full.obj_T, inlier=full.inlier, chi2=full.chi2, stats=full.stats)
    torch.cuda.synchronize()
    ba_dist.close_comms()
    dist.destroy_process_group()
    print("BA_DIST_C " + json.dumps({"rank": rank, "calls": calls, "stats": [int(v) for v in full.stats]}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "bad_rccl_path":
        bad_rccl_path()
    elif mode == "rocm_rccl":
        rocm_rccl(int(sys.argv[2]), int(sys.argv[3]))
    elif mode == "two_ranks":
        two_ranks(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        raise SystemExit(f"unknown mode {mode}")
