"""Call trace and outputs of the two BOP meters of suo_slam_amd/bop_eval.py over a logging stand-in: tests/golden/meter_trace_golden.json.  No device.

The golden pins what a rearrangement of the meters must not move: which ``errors`` calls are made, in which order, with which pairs, which depth images are
loaded and when, the re-indexed ``image_index`` of every VSD run, and every output down to the key order JSON keeps.  It is a characterisation of the code
as it stood, not a restatement of the toolkit (tests/test_siso_host.py and tests/test_bop_eval_host.py hold the meters to the toolkit).

WRITTEN ONCE, from the code of commit 420aac61538619d9285017be334e7e985048d22d (the parent of the commit that introduced one pair walk for both meters),
and NOT regenerated afterwards: a golden rewritten from the code under test pins nothing.  Run as ``python -m tests.golden.make_meter_trace_golden`` only to
add configurations, from a checkout of that commit.

Tree and estimates are those of tests/golden/siso_cases.py.  ``Logged`` appends every call to one shared log and serves values derived from a hash of
(method, object, T_est bytes, T_gt bytes), scaled to straddle the thresholds of the error type so that matching is not trivial; the depth loader appends
``["load", scene, im]`` to the same log, so loads and device calls are recorded interleaved.  tests/test_meter_trace.py replays ``record`` per configuration.
"""
import hashlib
import json
import os

import numpy as np

from suo_slam_amd import bop_eval
from tests.golden import siso_cases as SC

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "meter_trace_golden.json")
PAIRS_PER_CALL = (32, 2)
N_TOPS = (1, -1, 0)
VISIB_GT_MINS = (-1, 0.1)


def sha(x, dtype=np.float64):
    return None if x is None else hashlib.sha256(np.ascontiguousarray(np.asarray(x, dtype)).tobytes()).hexdigest()


def _unit(name, obj_id, Te, Tg, k=0):
    """A value in [0, 1) from sha-256 of (name, object, pose bytes): 8 bytes at offset 8 k."""
    h = hashlib.sha256(name.encode() + int(obj_id).to_bytes(4, "little") + np.asarray(Te, np.float64).tobytes() + np.asarray(Tg, np.float64).tobytes()).digest()
    return int.from_bytes(h[8 * k:8 * k + 8], "little") / 2.0 ** 64


class Logged:
    """The stand-in ``errors`` object.  Served ranges: MSSD 0 .. 0.6 diameters (thresholds 0.05 .. 0.5), MSPD 0 .. 15 px (x 640 / 160: 0 .. 60 against
    5 .. 50), VSD 0 .. 0.6 per tau (thresholds 0.05 .. 0.5), ADD / ADI 0 .. 0.2 diameters (threshold 0.1), PROJ 0 .. 10 px (5), CUS 0 .. 1 (0.5)."""

    def __init__(self, log):
        self.log, self.models_info, self.max_sym_disc_step = log, SC.models_info(), 0.01

    def _entry(self, name, obj_ids, T_est, T_gt, K, **kw):
        self.log.append(dict({"call": name, "obj_ids": [int(o) for o in obj_ids], "T_est": sha(T_est), "T_gt": sha(T_gt), "K": sha(K)}, **kw))

    def _diam(self, o):
        return float(self.models_info[int(o)]["diameter"])

    def errors(self, obj_ids, T_est, T_gt, K):
        self._entry("errors", obj_ids, T_est, T_gt, K)
        return (np.array([0.6 * self._diam(o) * _unit("mssd", o, e, g) for o, e, g in zip(obj_ids, T_est, T_gt)], np.float64),
                np.array([15.0 * _unit("mspd", o, e, g) for o, e, g in zip(obj_ids, T_est, T_gt)], np.float64))

    def vsd(self, obj_ids, T_est, T_gt, K, depth_images, image_index, delta=15, taus=bop_eval.VSD_TAUS, normalized=True):
        self._entry("vsd", obj_ids, T_est, T_gt, K, delta=delta, taus=[float(t) for t in taus], normalized=bool(normalized),
                    image_index=[int(i) for i in image_index], depth=[[list(np.asarray(d).shape), sha(d, np.float32)] for d in depth_images])
        return np.array([[0.6 * _unit("vsd", o, e, g, t % 4) for t in range(len(taus))] for o, e, g in zip(obj_ids, T_est, T_gt)], np.float64).reshape(-1, len(taus))

    def point_errors(self, obj_ids, T_est, T_gt, K=None, which=("add", "adi", "proj")):
        self._entry("point_errors", obj_ids, T_est, T_gt, K, which=list(which))
        return {w: np.array([(10.0 if w == "proj" else 0.2 * self._diam(o)) * _unit(w, o, e, g) for o, e, g in zip(obj_ids, T_est, T_gt)], np.float64) for w in which}

    def mask_errors(self, obj_ids, T_est, T_gt, K, hw):
        self._entry("mask_errors", obj_ids, T_est, T_gt, K, hw=[int(v) for v in hw])
        return {"cus": np.array([_unit("cus", o, e, g) for o, e, g in zip(obj_ids, T_est, T_gt)], np.float64)}


def configurations():
    """``[(name, pairs per call, kind, parameters)]``: both meters' recorded configurations at both run lengths."""
    out = []
    for ppc in PAIRS_PER_CALL:
        out.append((f"bop19-noloader-ppc{ppc}", ppc, "bop19", {"loader": False}))
        out.append((f"bop19-loader-ppc{ppc}", ppc, "bop19", {"loader": True}))
        for et in bop_eval.ERROR_TYPES:
            for n_top in N_TOPS:
                for vmin in VISIB_GT_MINS:
                    out.append((f"{et}-ntop{n_top}-visib{vmin}-ppc{ppc}", ppc, "loc", {"error_type": et, "n_top": n_top, "visib_gt_min": vmin}))
    return out


_TREE = {}


def _fixtures():
    if not _TREE:
        t = SC.tree()
        _TREE.update(tree=t, gt=SC.scene_gt(t), info=SC.scene_gt_info(t))
    return _TREE["tree"], _TREE["gt"], _TREE["info"]


def record(ppc, kind, params):
    """Runs one configuration with bop_eval.VSD_PAIRS_PER_CALL = ``ppc`` and returns ``{"log": [...], "out": {...}}``, JSON-ready."""
    tree, gt, info = _fixtures()
    log = []
    errors = Logged(log)

    def loader(s, im):
        log.append(["load", int(s), int(im)])
        return SC.read_raw(tree["scenes"][s][im]["raw"])

    saved, bop_eval.VSD_PAIRS_PER_CALL = bop_eval.VSD_PAIRS_PER_CALL, ppc
    try:
        if kind == "bop19":
            meter = bop_eval.Bop19Meter(errors, tree["targets"], gt, info, SC.W, depth_loader=loader if params["loader"] else None, vsd_delta=SC.DELTA)
        else:
            meter = bop_eval.LocalizationMeter(errors, tree["targets"], gt, info, symmetric_obj_ids=SC.SYMMETRIC_OBJ_IDS, im_width=SC.W, im_hw=(SC.H, SC.W),
                                               scene_ids=SC.SCENE_IDS, obj_ids=SC.OBJ_IDS, depth_loader=loader, **params, **SC.VSD)
        for e in tree["ests"]:
            meter.add(e["scene_id"], e["im_id"], e["obj_id"], e["score"], e["T"], tree["scenes"][e["scene_id"]][e["im_id"]]["K"])
        out = {}

        def take(name, fn):
            log.append(["output", name])                                                 # the log is cut by the output that caused its calls
            out[name] = fn()

        if kind == "bop19":
            take("result", meter.result)
            take("error_table", meter.error_table)
            out["normalised"] = meter.normalised(out["error_table"])
            if params["loader"]:
                take("vsd_table", lambda: meter.vsd_table(bop_eval.VSD_TAUS))
        else:
            take("result", meter.result)
            take("matches", meter.matches)
            take("errors_json", lambda: {s: meter.errors_json(s) for s in SC.SCENE_IDS})
            out["error_sign"], out["score_sign"], out["parameters"], out["n_estimates"] = meter.error_sign(), meter.score_sign(), meter.parameters(), meter.n_estimates
    finally:
        bop_eval.VSD_PAIRS_PER_CALL = saved
    return json.loads(json.dumps({"log": log, "out": out}))


def segment(log, name):
    """The entries of ``log`` between the marker of output ``name`` and the next marker."""
    at = log.index(["output", name]) + 1
    end = next((i for i in range(at, len(log)) if isinstance(log[i], list) and log[i][0] == "output"), len(log))
    return log[at:end]


def _check(records):
    """The conditions that keep the trace from being vacuous."""
    seg = segment(records["bop19-loader-ppc2"]["log"], "result")
    calls = [e for e in seg if isinstance(e, dict)]
    assert [c["call"] for c in calls] == ["errors", "vsd", "vsd", "vsd"] and len(calls[0]["obj_ids"]) == 9, [c["call"] for c in calls]
    loads = [tuple(e[1:]) for e in seg if isinstance(e, list)]
    assert loads.count((1, 0)) == 2 and loads.count((5, 2)) == 2, loads
    for ppc in PAIRS_PER_CALL:
        for n_top in N_TOPS:
            for vmin in VISIB_GT_MINS:
                ad = [e["which"] for e in records[f"ad-ntop{n_top}-visib{vmin}-ppc{ppc}"]["log"] if isinstance(e, dict)]
                assert ad == [["adi"], ["add"]], ad
                for et in ("re", "te", "rete"):
                    assert all(e[0] == "output" for e in records[f"{et}-ntop{n_top}-visib{vmin}-ppc{ppc}"]["log"])
    assert len(set(records["bop19-loader-ppc2"]["out"]["result"]["mssd"]["recalls"])) > 1
    assert any(0.0 < r["out"]["result"]["recall"] < 1.0 for k, r in records.items() if not k.startswith("bop19"))


def main():
    records = {name: record(ppc, kind, params) for name, ppc, kind, params in configurations()}
    _check(records)
    # a configuration whose record does not depend on the run length is stored once: the name of its twin stands for it
    for name, ppc, _, _ in configurations():
        twin = name.replace(f"-ppc{ppc}", f"-ppc{PAIRS_PER_CALL[0]}")
        if ppc != PAIRS_PER_CALL[0] and records[name] == records[twin]:
            records[name] = twin
    with open(PATH, "w") as f:
        json.dump(records, f, separators=(",", ":"))
    print(PATH, os.path.getsize(PATH), "bytes,", len(records), "configurations")


if __name__ == "__main__":
    main()
