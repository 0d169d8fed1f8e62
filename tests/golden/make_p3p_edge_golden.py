#!/usr/bin/env python3
"""What the REFERENCE's own solver answers on the designed P3P / P4P cases of tests/golden/p3p_edge_cases.py: thirdparty/lambdatwist/p4p.cpp and
lambdatwist/lambdatwist.p3p.h compiled from where they lie by `make -C oracle ref` (oracle/_ref/libp4p_ref.so).  Recorded results only:
    valid [n], R [n][4][9], t [n][4][3] from ref_p3p on points 0, 1, 2 (zero beyond valid), T [n][4][4] from ref_p4p(xs, ys, {0, 1, 2, 3}).
Run in the build container:  python tests/golden/make_p3p_edge_golden.py
    --search N   instead: print the indices k < N of p3p_edge_cases.stream(k) that the reference answers with 0, 1, 3 and 4 candidates (COUNT*_KEYS there)"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all", "ref"])
from oracle import geometry as G  # noqa: E402
from tests.golden import p3p_edge_cases as EC  # noqa: E402

R = G.ref()


def ref_p3p(x, y):
    yh = np.ascontiguousarray(np.c_[y[:3], np.ones(3)])
    r, tt = np.zeros(36), np.zeros(12)
    v = R.ref_p3p(yh[0].copy(), yh[1].copy(), yh[2].copy(), x[0].copy(), x[1].copy(), x[2].copy(), r, tt)
    r, tt = r.reshape(4, 9), tt.reshape(4, 3)
    r[v:] = 0
    tt[v:] = 0
    return v, r, tt


if "--search" in sys.argv:
    found = {0: [], 1: [], 3: [], 4: []}
    for k in range(int(sys.argv[sys.argv.index("--search") + 1])):
        x, y, _, _ = EC.stream(k)
        v = ref_p3p(x, y)[0]
        if v in found:
            found[v].append(k)
    for v, ks in found.items():
        print(v, "candidates:", len(ks), tuple(ks[:12]))
    sys.exit(0)

table = EC.cases()
n = len(table)
valid, Rs, Ts, T4 = np.zeros(n, np.int32), np.zeros((n, 4, 9)), np.zeros((n, 4, 3)), np.zeros((n, 4, 4))
for i, c in enumerate(table):
    valid[i], Rs[i], Ts[i] = ref_p3p(c["xs"], c["ys"])
    T4[i] = G.ref_p4p(c["xs"], c["ys"], [0, 1, 2, 3])
np.savez_compressed(os.path.join(HERE, "p3p_edge_golden.npz"), valid=valid, R=Rs, t=Ts, T=T4)
print("wrote p3p_edge_golden.npz", n, "cases; valid counts", np.bincount(valid, minlength=5))
for f in sorted({c["family"] for c in table}):
    m = np.array([c["family"] == f for c in table])
    print(" family", f, int(m.sum()), "cases, valid counts", np.bincount(valid[m], minlength=5))
