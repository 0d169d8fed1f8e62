"""Host side of the model-statistics row (N8).  No GPU.

The toolkit's own inout.load_ply, misc.calc_pts_diameter and inout.save_json wrote tests/golden/model_info_golden.npz (tests/golden/make_model_info_golden.py,
following scripts/calc_model_info.py line by line); the numpy restatement tests/model_info_ref.py -- the yardstick of the GPU tests at sizes the toolkit was
not run on -- must reproduce its numbers exactly, the formatter must write its text byte for byte, and the file handling of calc_models_info (``keep``) is
checked with that restatement in the device's place.  Tolerance: none anywhere; every comparison is ``==`` on fp64 values or on text."""
import json
import os

import numpy as np
import pytest

from suo_slam_amd import bop, bop_model_info
from tests import model_info_ref as MR
from tests.golden import model_info_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "model_info_golden.npz"))
TEXT = GOLD["text"].tobytes().decode()


@pytest.fixture(scope="module")
def cases():
    return MC.models()


def test_numpy_rule_equals_the_toolkit_exactly(cases):
    assert GOLD["info"].shape == (len(cases), 7)
    for k, (label, pts, _) in enumerate(cases):
        info, _, flag = MR.model_info(pts)
        assert flag == 0 and np.array_equal(info.view(np.uint64), GOLD["info"][k].view(np.uint64)), (label, info, GOLD["info"][k])
    # what the cases were designed to hold
    by = {c[0]: GOLD["info"][k] for k, c in enumerate(cases)}
    assert by["one"][6] == 0.0 and by["identical"][6] == 0.0 and (by["identical"][3:6] == 0.0).all()
    assert (by["negative_box"][:3] < 0).all() and (by["negative_box"][:3] + by["negative_box"][3:6] < 0).all()
    assert (by["offset_1e4"][:3] < 0).all() and (by["offset_1e4"][:3] + by["offset_1e4"][3:6] > 0).all()          # mixed signs
    assert by["small_1e-3"][6] < 1e-2 and by["offset_1e4"][6] > 1e4 and (by["extent_1_at_1e6"][:3] >= 1e6).all()


def test_pair_rule_of_the_restatement(cases):
    """The pair is a diametral one, and the lowest: checked against a plain double loop on the small cases."""
    for label, pts, _ in cases:
        if len(pts) > 300:
            continue
        info, pair, _ = MR.model_info(pts, pair=True)
        p = pts.astype(np.float64)
        d = p[:, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        want = min((i, j) for i in range(len(p)) for j in range(i, len(p)) if d2[i, j] == d2.max())
        assert pair == want and np.sqrt(d2[pair]) == info[6], (label, pair, want)
    assert MR.model_info(cases[7][1], pair=True)[1] == (0, 0)                       # all points identical
    bad = cases[3][1].copy()
    bad[100, 1] = np.inf
    info, pair, flag = MR.model_info(bad, pair=True)
    assert flag == 1 and np.isnan(info).all() and pair == (-1, -1)


def test_signed_zero_extremes_of_the_restatement():
    """-0 orders below +0: with both zeros as an axis's minimum it is -0.0, whatever their order in the cloud; with one kind of zero alone the rule is
    numpy's (and so the toolkit's) own.  A zero maximum shows in size only, which is the same number with either zero."""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    for order in ((nz, pz), (pz, nz)):
        lo_case = np.array([[order[0], 1, 1], [order[1], 2, 2], [3, 3, 3]], np.float32)          # x: zero is the minimum
        hi_case = np.array([[order[0], 1, 1], [order[1], 2, 2], [-3, 3, 3]], np.float32)         # x: zero is the maximum
        info = MR.model_info(lo_case)[0]
        assert info[0] == 0.0 and np.signbit(info[0]) and info[3] == 3.0
        info = MR.model_info(hi_case)[0]
        assert info[0] == -3.0 and info[3] == 3.0                                                 # a zero maximum: 0.0 - (-3.0) with either zero
        flat = np.array([[order[0], 1, 1], [order[1], 2, 2]], np.float32)                        # x: both extremes are zeros
        info = MR.model_info(flat)[0]
        assert np.signbit(info[0]) and info[3] == 0.0 and not np.signbit(info[3])
    for z in (nz, pz):
        one = np.array([[z, 1, 1], [z, 2, 2], [3, 3, 3]], np.float32)
        info = MR.model_info(one)[0]
        assert np.signbit(info[0]) == np.signbit(z) and np.signbit(one.astype(np.float64).min(axis=0)[0]) == np.signbit(z)


def test_format_equals_the_recorded_text_byte_for_byte(cases):
    info = {k + 1: {name: float(v) for name, v in zip(bop_model_info.KEYS, GOLD["info"][k])} for k in range(len(cases))}
    assert bop_model_info.format_models_info(info) == TEXT
    assert bop_model_info.format_models_info(dict(reversed(list(info.items())))) == TEXT            # ordered by the integer keys, whatever the dictionary's order
    assert not TEXT.endswith("\n") and TEXT.count("\n") == len(info) + 1
    assert {int(k): v for k, v in json.loads(TEXT).items()} == info                                 # every float round-trips
    assert bop_model_info.format_models_info({10: {"b": 1.5, "a": 2.0}, 9: {}}) == '{\n  "9": {},\n  "10": {"a": 2.0, "b": 1.5}\n}'
    assert bop_model_info.format_models_info({}) == "{\n}"
    assert bop_model_info.KEYS == MR.KEYS


def test_files_through_calc_models_info_and_keep(tmp_path, cases):
    """The whole file path (bop_model_info._calc_models_info, the body of calc_models_info) with the numpy rule in the device's place: the PLY files of the cases parsed by load_ply_points, the entries, the text.  keep=True
    carries symmetries_* (and any other key) of an existing file over; keep=False writes exactly the toolkit's file."""
    d = str(tmp_path)
    ids = MC.write_models(d)
    assert bop_model_info.model_ids(d) == ids == list(range(1, len(cases) + 1))
    out = bop_model_info._calc_models_info(d, None, False, True, MR.models_info)
    path = os.path.join(d, "models_info.json")
    with open(path, "r") as f:
        assert f.read() == TEXT
    assert bop_model_info.format_models_info(out) == TEXT
    # an annotated file
    sym = {"symmetries_discrete": [[-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
    old = {int(k): v for k, v in json.loads(TEXT).items()}
    old[2].update(sym)
    old[2]["diameter"] = 1.0                                                       # a stale number is recomputed, not kept
    old[5]["note"] = "hand"
    old[77] = {"diameter": 5.0}                                                    # an object without a PLY file here
    with open(path, "w") as f:
        f.write(bop_model_info.format_models_info(old))
    kept = bop_model_info._calc_models_info(d, None, True, True, MR.models_info)
    with open(path, "r") as f:
        on_disk = {int(k): v for k, v in json.load(f).items()}
    assert on_disk == kept
    assert kept[2]["symmetries_discrete"] == sym["symmetries_discrete"] and kept[2]["symmetries_continuous"] == sym["symmetries_continuous"]
    assert kept[2]["diameter"] == out[2]["diameter"] and kept[5]["note"] == "hand" and kept[77] == {"diameter": 5.0}
    assert all({k: kept[o][k] for k in bop_model_info.KEYS} == out[o] for o in ids)
    # a subset, nothing written
    before = open(path, "r").read()
    part = bop_model_info._calc_models_info(d, [3, 1], False, False, MR.models_info)
    assert part == {3: out[3], 1: out[1]} and open(path, "r").read() == before
    dropped = bop_model_info._calc_models_info(d, None, False, True, MR.models_info)
    with open(path, "r") as f:
        assert f.read() == TEXT
    assert "symmetries_discrete" not in dropped[2] and 77 not in dropped


def test_ascii_exact_file_gives_the_bits_of_its_binary_twin(tmp_path, cases):
    labels = [c[0] for c in cases]
    b, a = labels.index("eighths"), labels.index("eighths_ascii")
    assert cases[a][2] == "ascii" and cases[b][2] == "binary"
    assert np.array_equal(GOLD["info"][a].view(np.uint64), GOLD["info"][b].view(np.uint64))
    MC.write_models(str(tmp_path), which=(a + 1, b + 1))
    pa = bop.load_ply_points(os.path.join(str(tmp_path), f"obj_{a + 1:06d}.ply"))
    pb = bop.load_ply_points(os.path.join(str(tmp_path), f"obj_{b + 1:06d}.ply"))
    assert pa.dtype == np.float64 and np.array_equal(pa, pb) and np.array_equal(pa.astype(np.float32), cases[a][1])
    ia, ib = MR.model_info(pa.astype(np.float32))[0], MR.model_info(pb.astype(np.float32))[0]
    assert np.array_equal(ia.view(np.uint64), ib.view(np.uint64)) and np.array_equal(ia.view(np.uint64), GOLD["info"][a].view(np.uint64))


def test_load_mesh_db_default_still_needs_the_file(tmp_path):
    MC.write_models(str(tmp_path), which=(1,))
    with pytest.raises(FileNotFoundError):
        bop.load_mesh_db(str(tmp_path))


def test_calc_models_info_has_the_specified_signature():
    import inspect
    assert list(inspect.signature(bop_model_info.calc_models_info).parameters) == ["model_dir", "obj_ids", "keep", "write"]
    p = inspect.signature(bop_model_info.calc_models_info).parameters
    assert p["obj_ids"].default is None and p["keep"].default is True and p["write"].default is True
