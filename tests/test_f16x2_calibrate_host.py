"""Host half of the fp16 form's per-site calibration (include/suo_hip.h: suo_net_calibrate): the rule suo_f16x2_shift_for -- the largest s with
2^s k max|x| <= 65504 / 16, k = 4 for a 3x3 (Winograd) input and 1 for a 1x1 input, clamped to [-26, 26], 4 for an all-zero operand -- and the new entries'
presence in the header and the library.  No GPU needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from suo_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 65504.0 / 16                                   # 4094: 16x of headroom below the fp16 guard
NEW = ["suo_net_calibrate", "suo_net_f16x2_sites", "suo_net_f16x2_site_name", "suo_net_get_f16x2_shifts", "suo_net_set_f16x2_shifts", "suo_f16x2_shift_for"]


@pytest.fixture(scope="module")
def lib():
    from suo_slam_amd import build
    build.build(verbose=False)
    return _lib.lib()


def shift_for(lib, amax, ksize):
    out = C.c_int(-999)
    rc = lib.suo_f16x2_shift_for(C.c_float(amax), ksize, C.byref(out))
    return rc, out.value


def reference(amax, ksize):
    """The rule by brute force over every admissible s, in float64 (k max is exact there)."""
    if amax == 0:
        return 4
    v = (4.0 if ksize == 3 else 1.0) * float(np.float32(amax))
    ok = [s for s in range(-200, 200) if math.ldexp(v, s) <= BOUND]
    return min(max(max(ok), -26), 26)


def below(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


def above(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


@pytest.mark.parametrize("ksize,k", [(1, 1.0), (3, 4.0)])
def test_default_shift_is_exactly_the_window_of_the_old_constant(lib, ksize, k):
    """s = 4 exactly when 4094/32 < k max <= 4094/16; one float past either end moves it."""
    lo, hi = BOUND / 32 / k, BOUND / 16 / k
    assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi       # (exact binary fractions)
    assert shift_for(lib, hi, ksize) == (0, 4)
    assert shift_for(lib, above(hi), ksize) == (0, 3)
    assert shift_for(lib, above(lo), ksize) == (0, 4)
    assert shift_for(lib, lo, ksize) == (0, 5)
    assert shift_for(lib, below(lo), ksize) == (0, 5)


@pytest.mark.parametrize("ksize", [1, 3])
def test_rule_matches_brute_force_around_every_power_of_two_boundary(lib, ksize):
    k = 4.0 if ksize == 3 else 1.0
    vals = []
    for s in range(-24, 25):
        b = math.ldexp(BOUND, -s) / k                                        # the largest max that still takes s
        vals += [below(b), b, above(b)]
    rng = np.random.default_rng(3)
    vals += list(np.exp(rng.uniform(np.log(1e-6), np.log(1e9), 200)).astype(np.float32).astype(float))
    for v in vals:
        rc, s = shift_for(lib, v, ksize)
        assert rc == 0 and s == reference(v, ksize), (v, ksize, s)
        assert math.ldexp(k * v, s) <= BOUND or s == -26


def test_seeded_scale_maxima_calibrate_to_larger_shifts(lib):
    """Weights far below the old limit (the seeded test weights: >= 195x of headroom) get more of fp16's precision, never less: 195x of headroom at 2^4
    is more than 16 x 2^3, so s = 7 keeps the 16x margin."""
    for ksize, limit in ((1, 4094.0), (3, 4094.0 / 4)):
        rc, s = shift_for(lib, limit / 195, ksize)
        assert rc == 0 and s == 7


def test_clamps(lib):
    for ksize in (1, 3):
        assert shift_for(lib, 1e-30, ksize) == (0, 26)                       # tiny operands: 2^26, not 2^100
        assert shift_for(lib, float(np.finfo(np.float32).tiny) / 8, ksize) == (0, 26)    # a subnormal max
        assert shift_for(lib, 3e38, ksize) == (0, -26)                       # huge ones: the guard decides, the factors stay normal
        assert shift_for(lib, float(np.finfo(np.float32).max), ksize) == (0, -26)
    # at the clamps every 2^-(t + s) with |t| <= 100 is a normal fp32 number
    for s in (-26, 26):
        for t in (-100, 100):
            f = np.float32(2.0 ** -(t + s))
            assert f >= np.finfo(np.float32).tiny and np.isfinite(f)


def test_zero_keeps_the_default(lib):
    assert shift_for(lib, 0.0, 1) == (0, 4)
    assert shift_for(lib, 0.0, 3) == (0, 4)


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), -1.0, -0.5e-3])
def test_non_finite_or_negative_max_is_rejected(lib, bad):
    rc, s = shift_for(lib, bad, 1)
    assert rc != 0 and s == -999
    assert "suo_f16x2_shift_for" in lib.suo_last_error().decode()


@pytest.mark.parametrize("ksize", [0, 2, 5, 7])
def test_other_kernel_sizes_are_rejected(lib, ksize):
    assert shift_for(lib, 1.0, ksize)[0] != 0


def test_new_entries_declared_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "suo_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_null_network_is_an_error_not_a_crash(lib):
    assert lib.suo_net_f16x2_sites(None) == -1
    assert lib.suo_net_f16x2_site_name(None, 0) is None
    out = (C.c_int * 4)()
    assert lib.suo_net_get_f16x2_shifts(None, out, 4) != 0
    assert lib.suo_net_set_f16x2_shifts(None, out, 4) != 0
    assert lib.suo_net_calibrate(None, None, 0, 480, 640, None, None, 1, None) != 0
