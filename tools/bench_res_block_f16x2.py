"""The one-launch Residual block on two fp16 terms (csrc/res_small_x3.hip, NP = 2) alone, under HIP events, at the shapes the network launches it at:
the batched call's (256 crops at 8x8 = 512 workgroups and at 4x4 = 256, each plain / pool_in / up) and the one-frame call's (8 crops at 32x32 = 256
workgroups and at 16x16 = 64: fewer workgroups than CUs).  Every shape is timed REPS times over; the spread of those repeats is what a difference
between two builds of the library (SUO_HIP_LIB) has to clear.   python tools/bench_res_block_f16x2.py [reps] [launches per repeat]"""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from bench_legs.common import _timed
from suo_slam_amd import _lib
from tests import hipops as ops
from tests.test_gpu_res_block import _block_weights
lib = _lib.lib()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rng = np.random.default_rng(1)
B = _block_weights(rng)
h1, h2, h3 = np.empty(2 * 128 * 256, np.uint16), np.empty(2 * 128 * 128 * 9, np.uint16), np.empty(2 * 256 * 128, np.uint16)
o1, o2, o3 = np.empty(128, np.float32), np.empty(128, np.float32), np.empty(256, np.float32)
_lib.check(lib.suo_pack_res_block_f16x2(B["w1"].ctypes.data, B["w2"].ctypes.data, None, B["w3"].ctypes.data, h1.ctypes.data, h2.ctypes.data, h3.ctypes.data, o1.ctypes.data, o2.ctypes.data, o3.ctypes.data))
dh = [torch.from_numpy(t.view(np.int16)).cuda() for t in (h1, h2, h3)]
do = [ops.dev(t) for t in (o1, o2, o3)]
d = [ops.dev(t) for t in (B["pro"][0], B["pro"][1], B["b1"], B["b2"], B["b3"])]
flag = torch.zeros(1, dtype=torch.int32, device="cuda")
st = torch.cuda.current_stream(); s = C.c_void_p(st.cuda_stream)
P = ops.P
print(f"library {_lib.LIB_PATH}; {torch.cuda.get_device_name(0)}; {REPS} repeats of {ITERS} launches, us per launch")
for L, H in ((256, 8), (256, 4), (8, 32), (8, 16)):
    tiles = L * ((H + 3) // 4) * ((H + 7) // 8)
    x = torch.rand((L, H, H, 256), device="cuda") - 0.5
    xp = torch.rand((L, 2 * H, 2 * H, 256), device="cuda") - 0.5
    up = torch.rand((L, H // 2, H // 2, 256), device="cuda") - 0.5
    out = torch.empty_like(x)
    def run(xin, pool, low):
        return lambda: _lib.check(lib.suo_res_block_f16x2(P(xin), L, H, H, pool, P(d[0]), P(d[1]), P(dh[0]), P(do[0]), P(d[2]), P(dh[1]), P(do[1]), P(d[3]), P(dh[2]), P(do[2]), P(d[4]),
                                                          P(low), P(out), P(flag), s))
    for name, f in (("plain", run(x, 0, None)), ("pool_in", run(xp, 1, None)), ("up", run(x, 0, up))):
        t = [_timed(f, st, ITERS) for _ in range(REPS)]
        print(f"{L:4d} crops {H:2d}x{H:<2d} {tiles:4d} workgroups {name:8s} median {float(np.median(t)):6.2f}  min {min(t):6.2f}  max {max(t):6.2f}   " + " ".join(f"{v:6.2f}" for v in t), flush=True)
assert int(flag.item()) == 0
