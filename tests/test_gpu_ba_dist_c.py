"""The multi-rank global bundle adjustment driven from C (include/suo_hip.h: suo_ba_comm, suo_optimize_dist, suo_optimize_partitioned).

  * the local backend's all-reduce kernel against the rank-ordered numpy sum, bit for bit;
  * one real RCCL rank with every collective issued: the C driver against the Python driver (tests/rccl_one_rank_c.py), bit for bit -- with PyTorch's RCCL copy,
    and ROCm's own in a process without torch against suo_optimize;
  * the N-rank schedule itself on ONE GPU through the local backend: worlds 1 (bit-identical to suo_optimize), 2, 3, 4 and 8 (a rank without a camera) against
    the C oracle on the full graph, with the tolerances tests/test_ba_dist_gloo.py uses for this comparison;
  * errors; two real RCCL ranks where the box has two GPUs.
Trial counts are not compared with the oracle's (not a parity property).  Every child is a fresh process under its own `timeout`."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import geometry as G
from suo_slam_amd import _lib
from suo_slam_amd import ba as BA
from tests.ba_route_cases import BY_NAME, KEYS, global_graph, routes_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_GATE = 5.991


def _child(args, env=None, seconds=420):
    """A fresh process under `timeout` (SIGKILL 10 s after the limit): its exit status and its last tagged JSON line."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable] + [str(a) for a in args], cwd=ROOT, env=env or dict(os.environ),
                       capture_output=True, text=True)
    assert r.returncode == 0, f"exit status {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("RCCL_ONE_RANK_C ", "BA_DIST_C "))]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1].split(" ", 1)[1])


# ---- the local all-reduce kernel ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 433, 9313, 100003])            # 9313 = 96^2 + 96 + 1: [S | r | ok] at 16 objects
@pytest.mark.parametrize("world", [1, 2, 3, 4, 16])
def test_local_allreduce_is_the_rank_ordered_sum_bit_for_bit(world, n):
    import torch
    lib = _lib.lib()
    _lib.require_gpu()
    rng = np.random.default_rng(1000 * world + n % 997)
    even = n + (n & 1)
    # (stride, offset of the block in doubles): 16-byte aligned with an even stride = the 16-byte path; an odd stride, and a block 8 bytes off, = the scalar path
    for stride, off in [(even + 6, 0), (even + 7, 0), (even + 6, 1), (n, 0)]:
        size = off + world * stride + 9
        host = rng.standard_normal(size) * 10.0 ** rng.uniform(-8, 8, size)              # mixed magnitude and sign: the order of the additions shows
        bufs = [host[off + r * stride: off + r * stride + n].copy() for r in range(world)]
        want = functools.reduce(np.add, bufs)                                               # ((b0 + b1) + b2) + ...
        expect = host.copy()
        for r in range(world):
            expect[off + r * stride: off + r * stride + n] = want
        dev = torch.from_numpy(host).cuda()
        assert dev.data_ptr() % 16 == 0
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.suo_debug_ba_local_allreduce(C.c_void_p(dev.data_ptr() + 8 * off), world, stride, n, C.c_void_p(stream)), "suo_debug_ba_local_allreduce")
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        # every slot the sum, the doubles between n and stride (and around the block) untouched -- as bit patterns
        bad = np.flatnonzero(got.view(np.uint64) != expect.view(np.uint64))
        assert bad.size == 0, (world, n, stride, off, bad[:8].tolist(), got[bad[:4]].tolist(), expect[bad[:4]].tolist())


def test_local_allreduce_rejects_bad_arguments():
    import torch
    lib = _lib.lib()
    dev = torch.zeros(64, dtype=torch.float64, device="cuda")
    for world, stride, n in [(0, 8, 4), (17, 2, 2), (2, 3, 4)]:
        with pytest.raises(_lib.SuoError, match="local all-reduce"):
            _lib.check(lib.suo_debug_ba_local_allreduce(C.c_void_p(dev.data_ptr()), world, stride, n, None), "suo_debug_ba_local_allreduce")
    with pytest.raises(_lib.SuoError, match="local all-reduce"):
        _lib.check(lib.suo_debug_ba_local_allreduce(None, 2, 8, 4, None), "suo_debug_ba_local_allreduce")


# ---- one real RCCL rank -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cam,n_obj", [(12, 6), (32, 16)])
def test_one_rccl_rank_c_driver_is_bit_identical_to_the_python_driver(n_cam, n_obj):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    port = 29900 + (os.getpid() % 400) + n_cam
    out = _child([os.path.join(ROOT, "tests", "rccl_one_rank_c.py"), n_cam, n_obj, port], env)
    assert out["backend"] == "nccl" and (out["rank"], out["world"]) == (0, 1) and out["same_comm"]
    # a one-rank SUM is the identity and the launches are the same: poses, inlier flags, chi2 and all four stats
    assert all(out["identical"].values()), out
    assert all(out["repeatable"].values()), out
    assert out["trials"] > 0 and out["rounds"] == 4
    # per LM trial three collectives (a unit holds all three), one per classification (one before the rounds, one after each), one for the result assembly
    assert out["calls"] >= 3 * out["trials"] + out["rounds"] + 2, out


def test_rocm_rccl_copy_in_a_process_without_torch():
    """The other RCCL of the image: no torch in the process, so nothing is mapped and the library comes from the loader path."""
    env = {k: v for k, v in os.environ.items() if k != "SUO_RCCL_LIB"}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    out = _child([os.path.join(ROOT, "tests", "ba_dist_c_child.py"), "rocm_rccl", 12, 6], env)
    assert not out["torch_loaded"] and len(out["rccl"]) == 1, out
    assert all(out["identical"].values()), out
    assert out["calls"] >= 3 * out["stats"][2] + out["stats"][0] + 2, out


# ---- the N-rank schedule on one GPU -----------------------------------------------------------------------------------------------------------------------

def _problem(P, **kw):
    return BA.Problem(*[P[k] for k in KEYS], **kw)


def _partitioned(P, n_parts):
    lib = _lib.lib()
    _lib.require_gpu()
    q = _problem(P)
    s = _lib.BaProblem()
    q._fill(s)
    _lib.check(lib.suo_optimize_partitioned(C.byref(s), n_parts), "suo_optimize_partitioned")
    q.stats[:] = list(s.stats)
    q.chi2 = q.chi2[:len(q.edge_cam)]
    return q


@pytest.mark.parametrize("name", ["global_512", "mv_12x6"])
def test_local_world_one_is_bit_identical_to_suo_optimize(name):
    if name == "mv_12x6":
        from tests.test_gpu_geometry import _multi_view_scene
        P, _ = _multi_view_scene(np.random.default_rng(7), 12, 6)
    else:
        P = BY_NAME[name].problems()[0]
    assert routes_of([P])[0] == ["PHASES"]
    one = _problem(P)
    BA.optimize_batch([one])
    got = _partitioned(P, 1)
    for k in ("cam_T", "obj_T", "inlier", "chi2", "stats"):
        assert np.array_equal(getattr(got, k), getattr(one, k)), k
    assert one.stats[2] > 0


def _graph(name):
    if name == "7x5":
        return global_graph(np.random.default_rng(7), 315, 7, 5)
    if name == "7x5_fixed_cameras":                      # nothing to eliminate on any rank: the objects alone are adjusted
        P = global_graph(np.random.default_rng(7), 315, 7, 5)
        P["cam_fixed"] = np.ones(7, np.uint8)
        return P
    from tests.test_gpu_geometry import _multi_view_scene
    n_cam, n_obj = {"32x16": (32, 16), "60x8": (60, 8)}[name]
    return _multi_view_scene(np.random.default_rng(7), n_cam, n_obj)[0]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    P = _graph(name)
    ref = G.optimize(*[P[k] for k in KEYS])
    # the oracle's own inlier decisions must be away from the gate, or a last-bit difference may flip one (another seed then; no edge is left out)
    assert np.abs(ref[3] - CHI2_GATE).min() > 1e-6, name
    return ref


def _check_against_oracle(got, ref):
    """tests/test_ba_dist_gloo.py: _check_against_oracle -- inlier flags, round count and final inlier count equal; rotation blocks within 1e-6 (Frobenius),
    translations within 1e-5 relative."""
    assert np.array_equal(got.inlier, ref[2]) and got.stats[0] == ref[4][0] and got.stats[3] == ref[4][3]
    for a, b in zip(got.cam_T.reshape(-1, 3, 4), ref[0]):
        assert np.linalg.norm(a[:, :3] - b[:, :3]) < 1e-6 and np.linalg.norm(a[:, 3] - b[:, 3]) < 1e-5 * max(1, np.linalg.norm(b[:, 3]))
    for a, b in zip(got.obj_T.reshape(-1, 3, 4), ref[1]):
        assert np.linalg.norm(a[:, :3] - b[:, :3]) < 1e-6 and np.linalg.norm(a[:, 3] - b[:, 3]) < 1e-5 * np.linalg.norm(b[:, 3])


@pytest.mark.parametrize("name,world", [(g, w) for g in ("32x16", "60x8", "7x5") for w in (2, 3, 4)] + [("7x5", 8), ("7x5_fixed_cameras", 2)])
def test_local_ranks_run_the_partitioned_schedule_and_match_the_oracle(name, world):
    from suo_slam_amd import ba_dist
    P, ref = _graph(name), _oracle(name)
    comm = ba_dist.LocalRanks(world)
    try:
        assert (comm.rank, comm.world, comm.calls) == (0, world, 0)
        got = ba_dist.optimize_distributed_c(_problem(P), comm)
        calls = comm.calls
        again = ba_dist.optimize_distributed_c(_problem(P), comm)
    finally:
        comm.close()
    _check_against_oracle(got, ref)
    if world > len(P["cam_T"]):
        assert not any(c % world == world - 1 for c in range(len(P["cam_T"])))            # the last rank owns no camera and took part with zeros
    # the schedule: three collectives per LM trial, one per classification, one for the assembly
    assert got.stats[2] > 0 and calls >= 3 * got.stats[2] + got.stats[0] + 2
    # fixed summation order everywhere: the same call gives the same bits
    for k in ("cam_T", "obj_T", "inlier", "chi2", "stats"):
        assert np.array_equal(getattr(got, k), getattr(again, k)), k
    # the same result through the convenience entry
    conv = _partitioned(P, world)
    for k in ("cam_T", "obj_T", "inlier", "chi2", "stats"):
        assert np.array_equal(getattr(got, k), getattr(conv, k)), k


# ---- errors -------------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_fail_loudly():
    from suo_slam_amd import ba_dist
    lib = _lib.lib()
    P = _graph("7x5")
    q = _problem(P)
    s = _lib.BaProblem()
    q._fill(s)
    with pytest.raises(_lib.SuoError, match="null communicator"):
        _lib.check(lib.suo_optimize_dist(C.byref(s), None), "suo_optimize_dist")
    for world in (0, 17, -3):
        with pytest.raises(_lib.SuoError, match="ranks"):
            ba_dist.LocalRanks(world)
        with pytest.raises(_lib.SuoError, match="ranks"):
            _partitioned(P, world)
    with pytest.raises(_lib.SuoError, match="no communicator"):
        ba_dist.optimize_distributed_c(q)                                                # no process group and no communicator
    assert np.array_equal(q.cam_T, _problem(P).cam_T)                                    # nothing was touched


def test_rccl_path_that_does_not_exist_is_an_error_with_a_message():
    env = dict(os.environ, SUO_RCCL_LIB="/nonexistent/librccl.so.1")
    out = _child([os.path.join(ROOT, "tests", "ba_dist_c_child.py"), "bad_rccl_path"], env, seconds=120)
    assert out["unique_id_rc"] == 3 and "/nonexistent/librccl.so.1" in out["unique_id_msg"], out          # SUO_ERR_MISSING
    assert "suo_ba_comm_create_rccl failed" in out["create"] and "/nonexistent/librccl.so.1" in out["create"] and out["handle_null"], out


# ---- two real RCCL ranks ------------------------------------------------------------------------------------------------------------------------------------

def test_two_real_rccl_ranks(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("two real RCCL ranks need two GPUs: two ranks cannot share one device under RCCL")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    port = 29300 + (os.getpid() % 400)
    paths = [str(tmp_path / f"rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tests", "ba_dist_c_child.py"), "two_ranks", str(r), str(port), paths[r]],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-3000:] for o in outs)
    res = [np.load(p) for p in paths]
    for k in ("cam_T", "obj_T", "inlier", "chi2", "stats"):
        assert np.array_equal(res[0][k], res[1][k]), k

    class Got:
        pass
    got = Got()
    got.cam_T, got.obj_T, got.inlier, got.stats = res[0]["cam_T"], res[0]["obj_T"], res[0]["inlier"], res[0]["stats"]
    _check_against_oracle(got, _oracle("32x16"))
