"""suo_model_info (csrc/model_info.hip, row N8) on the device, through the C ABI and suo_slam_amd.bop_model_info.

Yardsticks: what the toolkit's own functions wrote on the clouds of tests/golden/model_info_cases.py (tests/golden/model_info_golden.npz, made by
tests/golden/make_model_info_golden.py) and, at the sizes built around the kernel's tiles, the numpy restatement tests/model_info_ref.py, which
tests/test_model_info_ref.py ties to the toolkit with ``==``.

Tolerance: none.  The arithmetic is pinned -- fp64 + - x in a fixed association on float32 inputs, exact minima and maxima, one correctly rounded sqrt -- so
every one of the seven numbers is compared on its fp64 bits and every pair on its indices.  TILE and ITILE are probed from the library."""
import json
import os

import numpy as np
import pytest

from suo_slam_amd import bop, bop_eval, bop_model_info, eval_meter
from tests import model_info_ref as MR
from tests.golden import model_info_cases as MC

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_info_golden.npz"))
TEXT = GOLD["text"].tobytes().decode()
SUO_ERR_ARG = 1


Db = bop_model_info.PointDb                       # a mesh database of float32 clouds and the raw entry over it: .clouds, .h, .lib, .run(index, pairs)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(info, ref):
    """fp64 bits equal, NaN by position (the bit pattern of a NaN is not pinned)."""
    info, ref = np.asarray(info, np.float64), np.asarray(ref, np.float64)
    return np.array_equal(np.isnan(info), np.isnan(ref)) and np.array_equal(bits(np.nan_to_num(info, nan=0.0)), bits(np.nan_to_num(ref, nan=0.0)))


def check_against_ref(db, index, got, refs=None):
    info, pair, flags = got
    for k, m in enumerate(index):
        r_info, r_pair, r_flag = MR.model_info(db.clouds[m], pair=True) if refs is None else refs[m]
        assert same(info[k], r_info), (k, m, info[k], r_info)
        assert flags[k] == r_flag
        if pair is not None:
            assert tuple(pair[k]) == r_pair, (k, m, tuple(pair[k]), r_pair)


@pytest.fixture(scope="module")
def tiles():
    tile, itile = bop_model_info.tiles()
    assert 1 < tile <= itile
    return tile, itile


def compact(rng, n):
    return rng.normal(size=(n, 3)).astype(np.float32)


def test_point_counts_around_the_tiles(tiles):
    T, I = tiles
    rng = np.random.default_rng(1)
    sizes = [1, 2, 3, T - 1, T, T + 1, I - 1, I, I + 1, 2 * I + 1]
    with Db([compact(rng, n) * 40 + (5.0, -3.0, 9.0) for n in sizes]) as db:
        for m in range(len(sizes)):                               # each alone
            got = db.run([m])
            check_against_ref(db, [m], got)
        info, pair, _ = db.run([0])
        assert info[0, 6] == 0.0 and (info[0, 3:6] == 0.0).all() and tuple(pair[0]) == (0, 0)          # one point: the pair (i, i) counts


def test_designed_diametral_pairs(tiles):
    T, I = tiles
    rng = np.random.default_rng(2)
    n = 2 * I + 37 if (2 * I + 37) % T else 2 * I + 38          # a ragged last j-tile
    last = (n - 1) // T * T                                      # first point of the last tile
    assert n - last >= 3
    planted = [(0, n - 1), (last + 1, n - 2), (I + 5, I + T - 3), (T - 1, T), (I - 1, I), (2 * T - 1, 5 * T + 1), (2 * T + 1, 5 * T - 1), (T, T + 1)]
    clouds = []
    for i, j in planted:
        c = compact(rng, n)
        c[i] = (500.25, -3.0, 7.5)
        c[j] = (-480.0, 11.0, -2.125)
        clouds.append(c)
    with Db(clouds) as db:
        index = list(range(len(planted)))
        got = db.run(index)
        check_against_ref(db, index, got)
        for k, want in enumerate(planted):
            assert tuple(got[1][k]) == want
            p = clouds[k].astype(np.float64)
            d = p[want[0]] - p[want[1]]
            assert got[0][k, 6] == np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            assert same(got[0][k, :3], p.min(0)) and same(got[0][k, 3:6], p.max(0) - p.min(0))


def test_ties_report_the_lowest_pair(tiles):
    T, I = tiles
    rng = np.random.default_rng(3)
    n = 2 * I + 1
    A, B, Cc, D = (100.0, 0.0, 0.0), (-100.0, 0.0, 0.0), (0.0, 100.0, 0.0), (0.0, -100.0, 0.0)          # |A - B|^2 = |C - D|^2 = 40000 exactly, |A - C|^2 = 20000

    def cloud(places):
        c = rng.integers(-10, 11, (n, 3)).astype(np.float32)
        for i, p in places:
            c[i] = p
        return c

    cases = [
        (cloud([(5, A), (2 * I - 1, B), (3, Cc), (I + 7, D)]), (3, I + 7)),                 # two pairs: the lower i wins although its tile comes later in no order
        (cloud([(3, A), (T + 9, B), (2 * I, B)]), (3, T + 9)),                              # one i, two j: the lower j
        (cloud([(I + 2, A), (I + 3, B), (4, Cc), (2 * I, D)]), (4, 2 * I)),                 # the lower i lies with a far j, the other pair in one diagonal tile
        (cloud([(T - 1, A), (T, B), (T - 2, Cc), (3 * T, D), (0, Cc), (n - 1, D)]), (0, 3 * T)),          # duplicates of both ends
    ]
    with Db([c for c, _ in cases]) as db:
        index = list(range(len(cases)))
        got = db.run(index)
        check_against_ref(db, index, got)
        for k, (_, want) in enumerate(cases):
            assert tuple(got[1][k]) == want and got[0][k, 6] == 200.0
        again = db.run(index[::-1])                               # the order of the batch changes nothing
        assert same(again[0][::-1], got[0]) and np.array_equal(again[1][::-1], got[1])


def test_identical_and_duplicated_points(tiles):
    T, I = tiles
    rng = np.random.default_rng(4)
    ident = np.tile(np.array([[12.5, -7.25, 3.0]], np.float32), (T + 3, 1))
    base = compact(rng, I + 11) * 30
    dup = np.concatenate((base, base[::2], base[:7], base))          # every point at least twice
    with Db([ident, dup]) as db:
        got = db.run([0, 1])
        check_against_ref(db, [0, 1], got)
        assert got[0][0, 6] == 0.0 and tuple(got[1][0]) == (0, 0) and (got[0][0, 3:6] == 0.0).all()
        i, j = got[1][1]
        assert i < j < len(base)                                  # the first copies of both ends


def test_signed_zero_extremes(tiles):
    """The stated rule of the box where a zero is an axis's minimum: -0 orders below +0, so with both present the minimum is -0.0, wherever they stand (in
    one tile, tiles apart, either order); one kind of zero alone is reported as it is.  A zero maximum shows in size only, the same number with either zero.
    tests/model_info_ref.py holds the same rule."""
    T, I = tiles
    rng = np.random.default_rng(9)
    nz, pz = np.float32(-0.0), np.float32(0.0)
    clouds = []
    for first, second in ((nz, pz), (pz, nz)):
        for at in ((0, 1), (3, I + 5)):
            lo = np.abs(compact(rng, I + T + 1)) + 1                # x > 0 but for the zeros: zero is the minimum
            lo[at[0], 0], lo[at[1], 0] = first, second
            hi = -lo                                                # x < 0 but for the zeros: zero is the maximum
            hi[at[0], 0], hi[at[1], 0] = first, second
            clouds += [lo, hi]
    for z in (nz, pz):
        only = np.abs(compact(rng, 40)) + 1
        only[7, 0] = only[9, 0] = z
        clouds += [only, -only]
        clouds[-1][7, 0] = clouds[-1][9, 0] = z
    with Db(clouds) as db:
        index = list(range(len(clouds)))
        info, pair, flags = db.run(index)
        check_against_ref(db, index, (info, pair, flags))
        for k in range(0, 8, 2):
            assert info[k, 0] == 0.0 and np.signbit(info[k, 0])                                  # minimum -0.0
            assert info[k + 1, 0] + info[k + 1, 3] == 0.0 and info[k + 1, 3] == -info[k + 1, 0]   # a zero maximum: size = 0.0 - min
        for k, z in ((8, nz), (10, pz)):
            assert info[k, 0] == 0.0 and np.signbit(info[k, 0]) == np.signbit(z)


def test_scale_cancellation_and_signs_on_the_golden_clouds():
    """Coordinates of order 1e-3 and 1e4, a cloud of extent 1 at 1e6 (the differences round), negative-only and mixed-sign boxes: the toolkit's numbers."""
    cases = MC.models()
    with Db([c[1] for c in cases]) as db:
        index = list(range(len(cases)))
        info, pair, flags = db.run(index)
        assert np.array_equal(bits(info), bits(GOLD["info"])), (info, GOLD["info"])
        assert not flags.any()
        check_against_ref(db, index, (info, pair, flags))


def test_batching_and_no_pair(tiles):
    T, I = tiles
    rng = np.random.default_rng(5)
    sizes = [1, T + 1, 3, 2 * I + 1]
    with Db([compact(rng, n) * 100 for n in sizes]) as db:
        alone = [db.run([m]) for m in range(len(sizes))]
        index = [0, 1, 2, 3, 1, 3, 0, 2, 2, 3]                    # repeated models, more items than models
        info, pair, flags = db.run(index)
        for k, m in enumerate(index):
            assert np.array_equal(bits(info[k]), bits(alone[m][0][0])) and np.array_equal(pair[k], alone[m][1][0]) and flags[k] == 0
        check_against_ref(db, index, (info, pair, flags))
        info2, pair2, flags2 = db.run(index, pairs=False)         # pair_out = NULL
        assert pair2 is None and np.array_equal(bits(info2), bits(info)) and not flags2.any()
        lib = db.lib                                              # flags_out = NULL as well
        idx = np.array(index, np.int32)
        info3 = np.zeros((len(index), 7))
        assert lib.suo_model_info(db.h, len(index), idx.ctypes.data, info3.ctypes.data, None, None) == 0
        assert np.array_equal(bits(info3), bits(info))
        assert lib.suo_model_info(db.h, 0, None, None, None, None) == 0                                 # n = 0: nothing to do


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinates(tiles, value):
    T, I = tiles
    rng = np.random.default_rng(6)
    n = 2 * I + 1
    a, b, c = compact(rng, 300) * 20, compact(rng, n) * 50, compact(rng, 5)
    clouds = [a, c]
    for at, axis in ((0, 0), (n // 2 + 1, 1), (n - 1, 2)):
        bad = b.copy()
        bad[at, axis] = value
        clouds.append(bad)
    with Db(clouds) as db:
        clean = db.run([0, 1])
        check_against_ref(db, [0, 1], clean)
        for m in (2, 3, 4):
            info, pair, flags = db.run([0, m, 1])
            assert flags.tolist() == [0, 1, 0]
            assert np.isnan(info[1]).all() and tuple(pair[1]) == (-1, -1)
            assert np.array_equal(bits(info[[0, 2]]), bits(clean[0])) and np.array_equal(pair[[0, 2]], clean[1])
            info, pair, flags = db.run([m, m], pairs=False)
            assert flags.tolist() == [1, 1] and np.isnan(info).all()
            check_against_ref(db, [m], db.run([m]))


@pytest.fixture(scope="module")
def large():
    rng = np.random.default_rng(7)
    big = (rng.normal(size=(12000, 3)) * (60.0, 45.0, 30.0) + (10.0, 200.0, -50.0)).astype(np.float32)
    small = compact(rng, 5)
    return big, small, MR.model_info(big, pair=True), MR.model_info(small, pair=True)


def test_one_larger_cloud(large):
    """12 000 points, 7.2e7 pairs: many workgroups on one atomic target, and (four times in one call) more work items than the grid holds workgroups."""
    big, small, r_big, r_small = large
    with Db([small, big]) as db:
        refs = {0: r_small, 1: r_big}
        first = db.run([1])
        check_against_ref(db, [1], first, refs)
        second = db.run([1])
        assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(first[1], second[1])
        check_against_ref(db, [0, 1], db.run([0, 1]), refs)
        index = [1, 0, 1, 1, 1]
        check_against_ref(db, index, db.run(index), refs)
        check_against_ref(db, index, db.run(index, pairs=False), refs)


def test_golden_file_through_calc_models_info(tmp_path):
    d = str(tmp_path)
    ids = MC.write_models(d)
    out = bop_model_info.calc_models_info(d)
    with open(os.path.join(d, "models_info.json"), "r") as f:
        assert f.read() == TEXT
    assert sorted(out) == ids and bop_model_info.format_models_info(out) == TEXT
    assert all(type(v) is float for e in out.values() for v in e.values())
    # a second run over the file it wrote, keep on: the same text; an annotation survives it
    with open(os.path.join(d, "models_info.json"), "r") as f:
        info = json.load(f)
    info["4"]["symmetries_continuous"] = [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]
    with open(os.path.join(d, "models_info.json"), "w") as f:
        json.dump(info, f)
    kept = bop_model_info.calc_models_info(d)
    assert kept[4]["symmetries_continuous"] == info["4"]["symmetries_continuous"] and {k: kept[4][k] for k in bop_model_info.KEYS} == out[4]
    bop_model_info.calc_models_info(d, keep=False)
    with open(os.path.join(d, "models_info.json"), "r") as f:
        assert f.read() == TEXT


def test_load_mesh_db_compute_info(tmp_path):
    d = str(tmp_path)
    ids = MC.write_models(d)
    with pytest.raises(FileNotFoundError):
        bop.load_mesh_db(d)                                       # the default: as before
    db = bop.load_mesh_db(d, compute_info=True)
    assert sorted(db) == ids and not os.path.exists(os.path.join(d, "models_info.json"))
    for o in ids:
        assert db[o]["diameter"] == GOLD["info"][o - 1, 6] and type(db[o]["diameter"]) is float
        assert db[o]["is_symmetric"] is False and db[o]["continuous_sym"] == []
        assert np.array_equal(db[o]["points"], MC.models()[o - 1][1])
    # a file that lacks the diameter of some objects: those are filled in, the others are read
    part = {str(o): ({"diameter": 123.0} if o % 2 else {"symmetries_discrete": [[1.0] * 16]}) for o in ids}
    with open(os.path.join(d, "models_info.json"), "w") as f:
        json.dump(part, f)
    text = open(os.path.join(d, "models_info.json")).read()
    db = bop.load_mesh_db(d, compute_info=True)
    for o in ids:
        assert db[o]["diameter"] == (123.0 if o % 2 else GOLD["info"][o - 1, 6])
        assert db[o]["is_symmetric"] is (o % 2 == 0)
    assert open(os.path.join(d, "models_info.json")).read() == text
    with pytest.raises(KeyError):
        bop.load_mesh_db(d)                                       # the default: as before


def test_model_info_over_the_meters_and_a_dictionary():
    cases = MC.models()
    mesh_db = {10 * (k + 1): {"points": c[1], "is_symmetric": False} for k, c in enumerate(cases[:6])}
    want = {10 * (k + 1): {name: float(v) for name, v in zip(bop_model_info.KEYS, GOLD["info"][k])} for k in range(6)}
    assert bop_model_info.model_info(mesh_db) == want
    assert bop_model_info.model_info(mesh_db, [40, 20]) == {40: want[40], 20: want[20]}
    got = bop_model_info.model_info(mesh_db, [50], pairs=True)[50]
    assert got["pair"] == MR.model_info(cases[4][1], pair=True)[1] and {k: got[k] for k in bop_model_info.KEYS} == want[50]
    be = bop_eval.BopErrors(mesh_db, {o: {"diameter": 1.0} for o in mesh_db})
    assert bop_model_info.model_info(be) == want and bop_model_info.model_info(be, [60]) == {60: want[60]}
    be.close()
    em = eval_meter.EvalMeter(mesh_db)
    assert bop_model_info.model_info(em, [30, 10]) == {30: want[30], 10: want[10]}
    em.close()


def test_refusals_on_a_live_database(tiles):
    rng = np.random.default_rng(8)
    with Db([compact(rng, 9), compact(rng, 4)]) as db:
        lib = db.lib
        info = np.full((3, 7), 7.5)
        pair = np.full((3, 2), 9, np.int32)
        flags = np.full(3, 9, np.int32)

        def refused(why, n, idx, info_ptr):
            rc = lib.suo_model_info(db.h, n, None if idx is None else idx.ctypes.data, info_ptr, pair.ctypes.data, flags.ctypes.data)
            msg = lib.suo_last_error().decode()
            assert rc == SUO_ERR_ARG and why in msg and "suo_model_info" in msg, (why, rc, msg)
            assert (info == 7.5).all() and (pair == 9).all() and (flags == 9).all()

        refused("model_index[1]=2 out of range", 3, np.array([0, 2, 1], np.int32), info.ctypes.data)
        refused("model_index[2]=-1 out of range", 3, np.array([0, 1, -1], np.int32), info.ctypes.data)
        refused("negative", -1, np.array([0, 1, 1], np.int32), info.ctypes.data)
        refused("null model_index or info_out", 3, np.array([0, 1, 1], np.int32), None)
        refused("null model_index or info_out", 3, None, info.ctypes.data)
        check_against_ref(db, [0, 1, 1], db.run([0, 1, 1]))       # the database is still good
