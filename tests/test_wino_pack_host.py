"""Host half of the Winograd 3x3 kernels: the three weight packers (fp32 pipe, three bf16 terms, two fp16 terms) lay out and split ONE transform,
U = G g G^T in float64, rounded once to float32, row xi = 3 negated (suo_slam_amd/csrc/conv_wino.hip: wino_weight_transform).  No GPU needed: the packers
are host code.  Each layout is undone in numpy as the comment above its packer documents it; w[64, 32, 3, 3] is two n-tiles and two 16-channel chunks, the
smallest shape that exercises every index of the three layouts."""
import numpy as np
import pytest

from suo_slam_amd import _lib

N, C = 64, 32
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


@pytest.fixture(scope="module")
def w():
    return (np.random.default_rng(7).standard_normal((N, C, 3, 3)) / 17).astype(np.float32)


@pytest.fixture(scope="module")
def u_ref(w):
    """[n][c][xi][nu] in float32, row xi = 3 NOT yet negated"""
    u = np.einsum("ik,nckl,jl->ncij", G, w.astype(np.float64), G)
    return u.astype(np.float32)


def _stored(u_ref):
    s = u_ref.copy()
    s[:, :, 3, :] = -s[:, :, 3, :]
    return s.reshape(N, C, 16)                                             # comp = 4 xi + nu


def _unpack_split(buf, planes, dtype):
    # Up[chunk][comp][nb][plane][lane][e]: n = nb*32 + (lane & 31), c = chunk*16 + 8*(lane >> 5) + e
    p = buf.view(dtype).reshape(C // 16, 16, N // 32, planes, 2, 32, 8)    # [chunk][comp][nb][plane][lane >> 5][lane & 31][e]
    return p.transpose(3, 2, 5, 0, 4, 6, 1).reshape(planes, N, C, 16)      # [plane][n][c][comp]


def test_fp32_packer_stores_the_transform_rounded_once(w, u_ref):
    out = np.empty(16 * N * C, np.float32)
    _lib.check(_lib.lib().suo_pack_wino_weight(w.ctypes.data, N, C, N, C, out.ctypes.data))
    # Up[chunk][comp][s][nb][lane][t]: n = nb*32 + (lane & 31), c = chunk*16 + s*8 + (lane >> 5)*4 + t
    p = out.reshape(C // 16, 16, 2, N // 32, 2, 32, 4)                      # [chunk][comp][s][nb][lane >> 5][lane & 31][t]
    u = p.transpose(3, 5, 0, 2, 4, 6, 1).reshape(N, C, 16)
    assert np.array_equal(u, _stored(u_ref))
    assert np.array_equal(u.reshape(N, C, 4, 4)[:, :, 3], -u_ref[:, :, 3]) and np.any(u_ref[:, :, 3] != 0)      # row xi = 3 negated


def test_bf16x3_packer_terms_sum_exactly_to_the_fp32_transform(w, u_ref):
    out = np.empty(3 * 16 * N * C, np.uint16)
    _lib.check(_lib.lib().suo_pack_wino_weight_bf16x3(w.ctypes.data, N, C, out.ctypes.data))
    terms = (_unpack_split(out, 3, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    total = terms.sum(0)                                                   # (three bf16 numbers in float64: exact)
    assert np.array_equal(total, _stored(u_ref).astype(np.float64))
    assert np.array_equal(total.reshape(N, C, 4, 4)[:, :, 3], -u_ref[:, :, 3].astype(np.float64))
    # round-to-nearest terms: each is the bf16 nearest to what the terms before it left
    assert np.all(np.abs(terms[1]) <= np.abs(terms[0]) * 2.0 ** -8) and np.all(np.abs(terms[2]) <= np.abs(terms[0]) * 2.0 ** -16)


def test_f16x2_packer_scales_each_channel_and_splits_in_two(w, u_ref):
    out = np.empty(2 * 16 * N * C, np.uint16)
    osc = np.empty(N, np.float32)
    _lib.check(_lib.lib().suo_pack_wino_weight_f16x2(w.ctypes.data, N, C, out.ctypes.data, osc.ctypes.data))
    planes = _unpack_split(out, 2, np.float16).astype(np.float64)
    stored = _stored(u_ref).astype(np.float64)
    # t_n: the channel's largest |U| times 2^t_n lies in [2^12, 2^13); oscale = 2^-(t_n + 4)
    t = 13 - np.frexp(np.abs(stored).reshape(N, -1).max(1))[1]
    assert np.array_equal(osc.astype(np.float64), np.exp2(-(t + 4.0)))
    scaled = stored * np.exp2(t)[:, None, None]
    mx = np.abs(scaled).reshape(N, -1).max(1)
    assert np.all((mx >= 2.0 ** 12) & (mx < 2.0 ** 13))
    err = np.abs(planes[0] + planes[1] - scaled)
    rel = err / np.abs(scaled)
    print("f16x2 packer: max |hi + lo - U 2^t| / |U 2^t| = 2^%.2f, smallest |U 2^t| = 2^%.2f" % (np.log2(rel.max()), np.log2(np.abs(scaled).min())))
    assert np.all(err <= 2.0 ** -22 * np.abs(scaled))                      # the split's bound (csrc/f16x2.h)
    row3 = -u_ref[:, :, 3].astype(np.float64) * np.exp2(t)[:, None, None]                                   # row xi = 3 negated
    assert np.all(np.abs((planes[0] + planes[1]).reshape(N, C, 4, 4)[:, :, 3] - row3) <= 2.0 ** -22 * np.abs(row3)) and np.any(row3 != 0)
