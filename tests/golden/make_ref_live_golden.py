#!/usr/bin/env python3
"""What the REFERENCE's compiled P4P (oracle/_ref/libp4p_ref.so) and RANSAC sampler (oracle/_ref/librandom_ref.so) return on the inputs of
tests/golden/ref_live_cases.py, both built from where the reference lies by `make -C oracle ref`.  Data only.
Run in the build container:  python tests/golden/make_ref_live_golden.py"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all", "ref"])
from oracle import geometry as G  # noqa: E402
from tests.golden import ref_live_cases as cases  # noqa: E402

assert G.ref() is not None and G.ref_random() is not None
out = {"p4p_T": np.stack([G.ref_p4p(x, y, idx) for x, y, idx in cases.p4p_cases()])}
R = G.ref_random()
R.ref_rng_reset()
draws = []
for kind, n, k in cases.sampler_ops():
    a = np.zeros(k if kind == "randui" else 4 * k, np.int32)
    (R.ref_randui if kind == "randui" else R.ref_get4)(n, k, a)
    draws.append(a)
out["sampler_draws"] = np.concatenate(draws)
out["sampler_offsets"] = np.cumsum([0] + [len(a) for a in draws]).astype(np.int64)
np.savez_compressed(os.path.join(HERE, "ref_live_golden.npz"), **out)
print("wrote ref_live_golden.npz:", {k: v.shape for k, v in out.items()})
