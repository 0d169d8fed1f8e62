"""The fp16 form's range contract where it decides what the user gets (include/suo_hip.h: SUO_PIPE_F16X2): a forward's outputs are invalid if and only if ITS OWN
activations left the range, and the network moves to bf16x3 when the host learns of such a call -- at the network (two calls in flight, graph replay on / off, the
blocking C entry) and on each of ObjectSLAM's five routes that re-issue calls:
  R1 single-view device chain, R2 batched single views (two batches in flight), R3 host route, R4 one SLAM pass on the device, R5 both SLAM passes as one chain.
Each route runs against a reference that takes no race: the same views one call at a time, or another route that the existing suites hold equal, or a network
built on bf16x3.  tests/fp16_recipes.py: the three ways out of the range, and the late reader (every validity query first waits for the whole device)."""
import copy
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import fp16_recipes as R
from tests.test_gpu_slam_chain import _run, _states_equal

pytestmark = pytest.mark.gpu

TLESS = dict(kp_var_thresh=0.5, bbox_thresh=1.0, manual_kp_std=0.1)      # network keypoints: _confident weights, T-LESS thresholds
# ... of a network driven far beyond its normal range: its heat-maps saturate, and their covariances are singular (the graph's information matrices could not be
# formed) -- the keypoints stay the network's, their weights come from a fixed std, which the vote then accepts hypotheses with (the chained views project priors)
SATURATED = dict(TLESS, manual_kp_std=1.0, no_network_cov=True)


def _fresh_net(sd, max_crops, monkeypatch, f16x2=True):
    from suo_slam_amd.pkpnet import PkpNet
    monkeypatch.delenv("SUO_WINO_BF16X3", raising=False)
    if f16x2:
        monkeypatch.delenv("SUO_F16X2", raising=False)
    else:
        monkeypatch.setenv("SUO_F16X2", "0")
    net = PkpNet(state_dict=sd, max_crops=max_crops)
    if not f16x2:
        monkeypatch.delenv("SUO_F16X2", raising=False)
    assert net.pipe() == (2 if f16x2 else 1)
    return net


def _np(out):
    return {k: out[k].cpu().numpy() for k in ("uv", "cov", "kp_mask", "kp_mask_logits", "prob_logits")}


def _equal(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _on_a_stream():
    """A stream of its own: PkpNet calls on the legacy default stream are the BLOCKING C entries, which check and re-issue by themselves."""
    return torch.cuda.stream(torch.cuda.Stream())


def _invalid(net, out):
    torch.cuda.synchronize()
    return net.call_range_exceeded(out.call)


def _prior_inputs(L, seed=5):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-0.6, 0.6, (L, 41, 2)).astype(np.float32)
    return uv, np.ones((L, 41), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# preconditions: which calls of a fresh f16x2 network leave the range under each recipe (asserted, not assumed)

def test_recipe_preconditions(monkeypatch):
    with _on_a_stream():
        _recipe_preconditions(monkeypatch)


def _recipe_preconditions(monkeypatch):
    img, boxes = R.frame_and_boxes()
    bx = [torch.from_numpy(boxes)]
    net = _fresh_net(R.recipe_stem(), 2, monkeypatch)                          # (a) every call
    assert _invalid(net, net(img, bx, None, check=False)) and net.pipe() == 1
    net = _fresh_net(R.recipe_priors(), 2, monkeypatch)                        # (b) the pass with rendered priors, not the one without
    assert not _invalid(net, net(img, bx, None, check=False))
    puv, pmk = _prior_inputs(2)
    assert _invalid(net, net(img, bx, None, prior_uv=puv, prior_mask=pmk, check=False))
    net = _fresh_net(R.recipe_bright_dim(), 2, monkeypatch)                    # (c) normal frames, not the same frames / 16
    assert not _invalid(net, net(R.dim(img), bx, None, check=False)) and net.pipe() == 2
    assert _invalid(net, net(img, bx, None, check=False)) and net.pipe() == 1
    base = _fresh_net(R.base_state_dict(), 2, monkeypatch)                     # the unscaled weights: neither
    assert not _invalid(base, base(img, bx, None, check=False))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# network level

@pytest.mark.parametrize("entry", ["forward", "forward_frames"])
@pytest.mark.parametrize("order", ["clean_first", "out_of_range_first"])
def test_two_calls_in_flight_report_their_own_validity(monkeypatch, entry, order):
    """(c) on one stream, two calls enqueued before either is asked about.  The in-range call is valid -- bit for bit what the same call returns alone on a fresh
    f16x2 network -- whatever the other did; the network stays on f16x2 until the out-of-range call is asked about.  Under the late reader as well."""
    with _on_a_stream():
        _two_calls_in_flight(monkeypatch, entry, order)


def _two_calls_in_flight(monkeypatch, entry, order):
    img, boxes = R.frame_and_boxes()
    sd = R.recipe_bright_dim()

    def call(net, frame):
        if entry == "forward":
            return net(frame, [torch.from_numpy(boxes)], None, check=False)
        return net.forward_frames([frame, frame], [boxes, boxes[::-1].copy()], check=False)
    alone_net = _fresh_net(sd, 4, monkeypatch)
    alone = call(alone_net, R.dim(img))
    assert not _invalid(alone_net, alone)
    alone = _np(alone)
    for late in (False, True):
        net = _fresh_net(sd, 4, monkeypatch)
        frames = [R.dim(img), img] if order == "clean_first" else [img, R.dim(img)]
        outs = [call(net, f) for f in frames]
        assert outs[1].call == outs[0].call + 1 == net.last_call()
        clean, bright = (outs[0], outs[1]) if order == "clean_first" else (outs[1], outs[0])
        torch.cuda.synchronize()
        with (R.late_reader() if late else _nothing()):
            if order == "clean_first":
                assert not net.call_range_exceeded(clean.call)
                assert net.pipe() == 2                                    # (the host has not learnt of the invalid call yet)
                assert net.call_range_exceeded(bright.call) and net.pipe() == 1
            else:
                assert net.call_range_exceeded(bright.call) and net.pipe() == 1
                assert not net.call_range_exceeded(clean.call)            # (it ran on fp16, before the host learnt anything: valid)
        _equal(_np(clean), alone)
        # the record for suo_net_range_exceeded's readers: a forward since its last call left the range -- once
        assert net.range_exceeded() and not net.range_exceeded()


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_call_query_refuses_calls_it_cannot_answer(monkeypatch):
    from suo_slam_amd import _lib
    img, boxes = R.frame_and_boxes()
    net = _fresh_net(R.base_state_dict(), 2, monkeypatch)
    with pytest.raises(_lib.SuoError):
        net.call_range_exceeded(1)                                        # (no call issued yet)
    out = net(img, [torch.from_numpy(boxes)], None, check=False)
    with pytest.raises(_lib.SuoError):
        net.call_range_exceeded(out.call + 1)
    torch.cuda.synchronize()
    assert not net.call_range_exceeded(out.call)
    for _ in range(64):
        net(img, [torch.from_numpy(boxes)], None, check=False)
    torch.cuda.synchronize()
    with pytest.raises(_lib.SuoError):
        net.call_range_exceeded(out.call)                                 # (older than the last 64 calls)
    assert not net.call_range_exceeded(net.last_call())


def test_blocking_entry_reissues_its_own_call(monkeypatch):
    """suo_net_forward on the NULL stream with (a): the entry notices, re-issues on bf16x3 and returns, bit for bit, what a network built with SUO_F16X2=0 returns."""
    import ctypes as C
    from suo_slam_amd import _lib
    img, boxes = R.frame_and_boxes()
    sd = R.recipe_stem()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def blocking(net):
        L = len(boxes)
        d_img, d_bx = torch.from_numpy(img).cuda(), torch.from_numpy(boxes).cuda()
        outs = [torch.empty(s, dtype=torch.float32, device="cuda") for s in ((L, 41, 2), (L, 41, 2, 2), (L, 41), (L, 41), (L, 41, 64, 64))]
        torch.cuda.synchronize()
        _lib.check(_lib.lib().suo_net_forward(net._h, P(d_img), 0, img.shape[0], img.shape[1], P(d_bx), L, None, *[P(t) for t in outs], None), "suo_net_forward")
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]
    n16 = _fresh_net(sd, 2, monkeypatch)
    got = blocking(n16)
    assert n16.pipe() == 1 and not n16.call_range_exceeded(n16.last_call()) and not n16.range_exceeded()
    want = blocking(_fresh_net(sd, 2, monkeypatch, f16x2=False))
    for g, w in zip(got, want):
        assert np.isfinite(w).all() and np.array_equal(g, w)


def test_per_call_validity_with_and_without_graph_replay():
    """The per-call record is written behind the captured graph's replay as well as behind the per-layer launches: one child process each."""
    here = os.path.dirname(os.path.abspath(__file__))
    res = []
    for graph in (0, 1):
        env = {k: v for k, v in os.environ.items() if k not in ("SUO_F16X2", "SUO_WINO_BF16X3")}
        out = subprocess.run([sys.executable, os.path.join(here, "gpu_fp16_fallback_child.py"), str(graph)], env=env, capture_output=True, text=True, timeout=400)
        assert out.returncode == 0, out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res.append(json.loads(line[len("RESULT "):]))
    for r in res:
        assert r["alone_pipe"] == 2
        for order in ("clean_first", "bright_first"):
            o = r[order]
            assert o["bright_invalid"] and not o["clean_invalid"] and o["pipe_end"] == 1, (order, o)
            assert o["pipe_between"] == (2 if order == "clean_first" else 1), (order, o)
            assert o["clean"] == r["alone"], order
    assert res[0]["alone"] == res[1]["alone"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# ObjectSLAM routes

def _snapshot(slam):
    return types.SimpleNamespace(detections=copy.deepcopy(slam.detections), obj_poses=copy.deepcopy(slam.obj_poses), cam_poses=copy.deepcopy(slam.cam_poses),
                                 view_ids=list(slam.view_ids), _pnp_seed=slam._pnp_seed, obj_num_dets=dict(slam.obj_num_dets),
                                 obj_num_det_kps=dict(slam.obj_num_det_kps))


def _env(monkeypatch, f16x2=True, vote_chain=None):
    monkeypatch.delenv("SUO_WINO_BF16X3", raising=False)
    if f16x2:
        monkeypatch.delenv("SUO_F16X2", raising=False)
    else:
        monkeypatch.setenv("SUO_F16X2", "0")
    if vote_chain is not None:
        monkeypatch.setenv("SUO_SLAM_VOTE_CHAIN", "1" if vote_chain else "0")


def _slam_run(monkeypatch, seq, sd, n, f16x2=True, vote_chain=None, **kw):
    _env(monkeypatch, f16x2, vote_chain)
    return _run(seq, sd, n, **kw)


def _end_state(s, pipe, reissues):
    assert s.model.pipe() == pipe and s.fp16_range_reissues == reissues, (s.model.pipe(), s.fp16_range_reissues)


def _single_views(monkeypatch, seq, sd, n, f16x2=True):
    from suo_slam_amd.object_slam import ObjectSLAM
    _env(monkeypatch, f16x2)
    slam = ObjectSLAM(None, seq["mesh_db"], state_dict=sd, max_crops=16, single_view_mode=True, **TLESS)
    snaps = []
    for vw in seq["views"][:n]:
        slam.reset()
        slam.process_view(vw["view_id"], vw["image"], vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy(), vw["model_kps"], vw["model_kps_masks"], vw["kp_masks"])
        snaps.append(_snapshot(slam))
    return slam, snaps


def test_r1_single_view_chain_out_of_range_equals_a_bf16x3_network(monkeypatch):
    """R1, (a): the first view's call is invalid, re-issued once; every view's state equals a network built on bf16x3.  Exactly one re-issue: the first call
    moves the network to bf16x3, every later call is in range there."""
    from suo_slam_amd import synthetic as S
    seq = S.make_slam_sequence(np.random.default_rng(11), 4, 6)
    sd = R.confident(R.recipe_stem())
    got, gs = _single_views(monkeypatch, seq, sd, 4)
    want, ws = _single_views(monkeypatch, seq, sd, 4, f16x2=False)
    for a, b in zip(gs, ws):
        _states_equal(a, b, 0.0, 1e-9)
    _end_state(got, 1, 1)
    _end_state(want, 1, 0)


def test_r3_host_route_out_of_range_equals_a_bf16x3_network(monkeypatch):
    """R3 (device_chain=False), (a): a short SLAM sequence; the state equals a SUO_F16X2=0 run's; one re-issue (the first call), the pipe ends on bf16x3."""
    from suo_slam_amd import synthetic as S
    seq = S.make_slam_sequence(np.random.default_rng(11), 5, 6)
    sd = R.confident(R.recipe_stem())
    got = _slam_run(monkeypatch, seq, sd, 5, device_chain=False, **SATURATED)
    want = _slam_run(monkeypatch, seq, sd, 5, f16x2=False, device_chain=False, **SATURATED)
    _states_equal(got, want, 0.0, 1e-9)
    assert got._rng.bit_generator.state == want._rng.bit_generator.state
    _end_state(got, 1, 1)
    _end_state(want, 1, 0)


@pytest.mark.parametrize("recipe", ["stem", "priors"])
def test_r4_slam_pass_on_the_device_equals_the_host_route(monkeypatch, recipe):
    """R4 (SUO_SLAM_VOTE_CHAIN=0, device_chain=True) against R3 on the same views: (a) the first pass is invalid; (b) the first pass WITH PRIORS is invalid, every
    prior-less pass before it valid on fp16.  Both routes re-issue exactly that one call; (a) also equals a SUO_F16X2=0 run."""
    from suo_slam_amd import synthetic as S
    seq = S.make_slam_sequence(np.random.default_rng(11), 8, 6)
    sd = R.confident(R.recipe_stem() if recipe == "stem" else R.recipe_priors())
    chain = _slam_run(monkeypatch, seq, sd, 8, vote_chain=False, device_chain=True, **SATURATED)
    host = _slam_run(monkeypatch, seq, sd, 8, vote_chain=False, device_chain=False, **SATURATED)
    _states_equal(chain, host, 0.0, 1e-9)
    _end_state(chain, 1, 1)
    _end_state(host, 1, 1)
    if recipe == "stem":
        ref = _slam_run(monkeypatch, seq, sd, 8, f16x2=False, vote_chain=False, device_chain=True, **SATURATED)
        _states_equal(chain, ref, 0.0, 1e-9)
        _end_state(ref, 1, 0)


def _spy_chain(monkeypatch):
    """Records, per chained view: its return value, the re-issues it counted, the pipe before / after, and what each of its validity queries answered."""
    from suo_slam_amd.object_slam import ObjectSLAM
    from suo_slam_amd.pkpnet import PkpNet
    calls, answers = [], []
    orig_chain, orig_q = ObjectSLAM._process_view_slam_chain, PkpNet.call_range_exceeded

    def query(self, call):
        r = orig_q(self, call)
        answers.append(r)
        return r

    def chain(self, *a, **k):
        n0, p0 = self.fp16_range_reissues, self.model.pipe()
        del answers[:]
        r = orig_chain(self, *a, **k)
        calls.append({"ret": r, "reissues": self.fp16_range_reissues - n0, "pipe": (p0, self.model.pipe()), "answers": list(answers)})
        return r
    monkeypatch.setattr(PkpNet, "call_range_exceeded", query)
    monkeypatch.setattr(ObjectSLAM, "_process_view_slam_chain", chain)
    return calls


@pytest.mark.parametrize("late", [False, True])
def test_r5_both_passes_as_one_chain_keep_a_valid_pass_a(monkeypatch, late):
    """R5, (b), network keypoints: pass A (no priors) is in range, pass B (priors rendered from the vote) is not -- and B is still running when A is asked about.
    A's fp16 results stand, B alone is issued again (on bf16x3, through the per-pass route), exactly what SUO_SLAM_VOTE_CHAIN=0 does with the same views.
    The late reader asks about A only once B has finished: the answer must not change.  (no_network_cov with a wide keypoint std: the vote accepts hypotheses
    from the random network's poses, so the chained views do project priors and their pass B does leave the range.)"""
    from suo_slam_amd import synthetic as S
    seq = S.make_slam_sequence(np.random.default_rng(11), 10, 6)
    sd = R.confident(R.recipe_priors())
    with (R.late_reader() if late else _nothing()):
        calls = _spy_chain(monkeypatch)
        chain = _slam_run(monkeypatch, seq, sd, 10, vote_chain=True, **SATURATED)
        monkeypatch.undo()                                    # (the spies go before the late reader does)
    host = _slam_run(monkeypatch, seq, sd, 10, vote_chain=False, **SATURATED)
    _states_equal(chain, host, 0.0, 1e-9)
    _end_state(chain, 1, 1)           # (B of that view, once; everything after runs on bf16x3)
    _end_state(host, 1, 1)            # (the first pass with priors, once)
    assert calls, "the tracking views take the chain"
    c = next(c for c in calls if c["pipe"][1] == 1)
    # the first fallback: inside a chained view, pass B handed back to the caller (ret False), only B counted, A asked about first and valid, B invalid
    assert c["pipe"] == (2, 1) and c["reissues"] == 1 and c["ret"] is False and c["answers"] == [False, True], c


def test_r5_restores_the_noise_draws_of_a_reissued_pass_b(monkeypatch):
    """R5, (b), ground-truth keypoints injected on the device: a pass B handed back to the caller draws its keypoint noise again from where pass A left the
    generator (rng_after_a) -- the generator's state after the sequence equals the one of the per-pass route."""
    from suo_slam_amd import synthetic as S
    seq = S.make_slam_sequence(np.random.default_rng(3), 12, 8)
    sd = R.recipe_priors()
    kw = dict(debug_gt_kp=True, manual_kp_std=0.01, run_network_in_debug=True, debug_gt_on_device=True)
    calls = _spy_chain(monkeypatch)
    chain = _slam_run(monkeypatch, seq, sd, 12, vote_chain=True, **kw)
    assert any(c["answers"][-1:] == [True] and c["ret"] is False for c in calls), calls
    monkeypatch.undo()
    host = _slam_run(monkeypatch, seq, sd, 12, vote_chain=False, **kw)
    _states_equal(chain, host, 0.0, 1e-9)
    assert chain._rng.bit_generator.state == host._rng.bit_generator.state
    _end_state(chain, 1, 1)
    _end_state(host, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# R2: batched single views, two batches in flight

def _bop(tmp_path, n_views=6):
    from suo_slam_amd import bop
    from tests import bop_tree
    desc = bop_tree.build(str(tmp_path), dset="ycbv", seed=41, n_scenes=1, n_views=n_views)
    reader = bop.BopDataset(desc["data_root"], desc["split"], bop_dset="ycbv", ignore_symmetry=True)
    bop_tree.write_saved_detections(str(tmp_path), desc, reader, seed=5, trans_noise_mm=4.0, drop_every=1000)
    return desc, reader


def _evaluator(desc, tmp_path, sd, tag, fpc=2):
    from suo_slam_amd import evaluator
    ev = evaluator.Evaluator("ycbv", desc["data_root"], None, nviews=1, detection_type="saved", out_dir=str(tmp_path / tag), state_dict=sd, frames_per_call=fpc)
    ev.object_slam.bbox_thresh, ev.object_slam.kp_var_thresh = 10.0, 1e6         # random weights: let the masks pass, so that PnP / LM run on what the network emitted
    return ev


def _drive(slam, batches, pipelined):
    """pipelined: as Evaluator.run -- batch i+1 submitted before batch i is collected; else one batch at a time."""
    out, uv = [], []

    def collect():
        out.extend(slam.collect_views_single())
        last = slam.view_ids[-1]
        uv.append({o: (d["uv_pred"].copy(), d["kp_mask"].copy()) for o, d in slam.detections[last].items()})
    if pipelined:
        slam.submit_views_single(batches[0])
        for b in batches[1:]:
            slam.submit_views_single(b)
            collect()
        collect()
    else:
        for b in batches:
            slam.submit_views_single(b)
            collect()
    return out, uv


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("pattern", [("dim", "bright", "dim"), ("bright", "dim", "dim")])
def test_r2_batches_in_flight_keep_valid_batches(tmp_path, monkeypatch, pattern, late):
    """R2, (c): three batches of two views, dim (in range) or bright (out of range).  Submitted as Evaluator.run does (batch i+1 before batch i is collected)
    against one batch at a time: the same poses, scores, keypoints and sampler keys.  A valid batch collected before the invalid one keeps its fp16 results; the
    invalid one is re-issued with the batch behind it (its sampler keys continued from the invalid counts)."""
    _env(monkeypatch)
    desc, reader = _bop(tmp_path)
    sd = R.recipe_bright_dim()
    s = reader.scene_ids()[0]
    ev0 = _evaluator(desc, tmp_path, sd, "views")
    views = [ev0._view_args(s, v, v)[0] for v in reader.view_ids(s)]
    assert len(views) == 6 and all(v is not None for v in views)
    batches = []
    for i, kind in enumerate(pattern):
        b = [tuple(v[:1]) + ((R.dim(v[1]) if kind == "dim" else v[1]),) + tuple(v[2:]) for v in views[2 * i:2 * i + 2]]
        batches.append(b)
    # precondition on a fresh f16x2 network: the bright batches' calls leave the range, the dim ones' do not
    with _on_a_stream():
        for b, kind in zip(batches, pattern):
            fresh = _fresh_net(sd, 32, monkeypatch)
            out = fresh.forward_frames([v[1] for v in b], [np.asarray(v[4], np.float32) for v in b], check=False)
            assert _invalid(fresh, out) == (kind == "bright"), kind
    ev0.object_slam.model.close()
    with (R.late_reader() if late else _nothing()):
        piped = _evaluator(desc, tmp_path, sd, "piped").object_slam
        got, got_uv = _drive(piped, batches, True)
    serial = _evaluator(desc, tmp_path, sd, "serial").object_slam
    want, want_uv = _drive(serial, batches, False)
    assert len(got) == len(want) == 6
    n_pose = 0
    for g, w in zip(got, want):
        assert list(g.keys()) == list(w.keys())
        for vid in g:
            assert set(g[vid]["poses"]) == set(w[vid]["poses"])
            for o, r in g[vid]["poses"].items():
                assert r["score"] == w[vid]["poses"][o]["score"]
                assert (r["T_OtoC"] is None) == (w[vid]["poses"][o]["T_OtoC"] is None)
                if r["T_OtoC"] is not None:
                    assert np.array_equal(r["T_OtoC"], w[vid]["poses"][o]["T_OtoC"]), (vid, o)
                    n_pose += 1
    assert n_pose > 0
    for g, w in zip(got_uv, want_uv):
        assert g.keys() == w.keys()
        for o in g:
            assert np.array_equal(g[o][0], w[o][0]) and np.array_equal(g[o][1], w[o][1])
    assert piped._pnp_seed == serial._pnp_seed
    # one batch at a time: the bright batch alone is re-issued.  Pipelined: the bright batch and the one submitted behind it while it was in flight
    _end_state(serial, 1, 1)
    _end_state(piped, 1, 2)


def test_r2_evaluator_reports_the_fallback(tmp_path, monkeypatch):
    """Evaluator.run(frames_per_call=2) over a tree whose second batch of views is bright: two calls re-issued (that batch, and the one in flight behind it), and
    the run says it ended on bf16x3."""
    from PIL import Image
    _env(monkeypatch)
    desc, reader = _bop(tmp_path)
    s = reader.scene_ids()[0]
    rgb = os.path.join(desc["data_root"], desc["split"], "%06d" % s, "rgb")
    for k, v in enumerate(reader.view_ids(s)):
        if k // 2 != 1:
            p = os.path.join(rgb, "%06d.png" % v)
            Image.fromarray(R.dim(np.asarray(Image.open(p).convert("RGB")))).save(p)
    out = _evaluator(desc, tmp_path, R.recipe_bright_dim(), "run").run()
    assert out["num_views"] == 6
    assert out["fp16_range_reissues"] == 2 and out["matrix_pipe_at_end"] == "bf16x3", out
