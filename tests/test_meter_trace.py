"""Characterisation of the two BOP meters (suo_slam_amd/bop_eval.py) against a recorded trace.  No GPU.

tests/golden/meter_trace_golden.json was written once by tests/golden/make_meter_trace_golden.py, from the code as it stood before the meters came to share
one pair walk.  Every configuration -- Bop19Meter with and without a depth loader, LocalizationMeter for every error type x n_top x visib_gt_min, each at 32
and at 2 VSD pairs per call -- is replayed over the same logging stand-in, and the log and the outputs must equal the golden exactly: call order and count,
the pairs of each call, the re-indexed image_index, which images are loaded and when, and the key order of every dictionary JSON keeps."""
import json

import pytest

from tests.golden import make_meter_trace_golden as MT

with open(MT.PATH, "r") as f:
    GOLD = json.load(f)
CONFIGS = MT.configurations()


def _golden(name):
    rec = GOLD[name]
    return GOLD[rec] if isinstance(rec, str) else rec            # a record that does not depend on the run length is stored under its twin's name


def test_golden_holds_every_configuration():
    assert list(GOLD) == [c[0] for c in CONFIGS] and len(CONFIGS) == 2 * (2 + 11 * 3 * 2)
    MT._check({name: _golden(name) for name in GOLD})
    assert not isinstance(GOLD["bop19-loader-ppc2"], str) and not isinstance(GOLD["vsd-ntop0-visib-1-ppc2"], str)      # the run length shows where VSD runs


@pytest.mark.parametrize("name,ppc,kind,params", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_meter_replays_the_recorded_trace(name, ppc, kind, params):
    got, want = MT.record(ppc, kind, params), _golden(name)
    assert len(got["log"]) == len(want["log"]), [e["call"] if isinstance(e, dict) else e for e in got["log"]]
    for i, (a, b) in enumerate(zip(got["log"], want["log"])):
        assert a == b and (not isinstance(a, dict) or list(a) == list(b)), (i, a, b)
    assert list(got["out"]) == list(want["out"])
    for key in want["out"]:
        assert json.dumps(got["out"][key]) == json.dumps(want["out"][key]), key      # as text: dictionary key order included
