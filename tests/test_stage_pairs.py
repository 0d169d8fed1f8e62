"""bop_eval.stage_pairs / pack_poses / stage_images: what every BopErrors method and consistency.py hand to the C entries.  No GPU."""
import numpy as np
import pytest
import torch

from suo_slam_amd import bop_eval

INDEX = {7: 0, 3: 1, 11: 2}


def _poses(n, rows, seed=0):
    T = np.random.default_rng(seed).standard_normal((n, rows, 4))
    if rows == 4:
        T[:, 3] = [0.0, 0.0, 0.0, 1.0]
    return T


def _c(a, dtype, shape):
    return isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("rows", [3, 4])
def test_poses_of_three_and_four_rows_pack_to_their_first_twelve(rows):
    Te, Tg = _poses(5, rows, 1), _poses(5, rows, 2)
    n, idx, K, te, tg = bop_eval.stage_pairs(INDEX, [3, 7, 7, 11, 3], None, Te, Tg)
    assert n == 5 and K is None and idx.tolist() == [1, 0, 0, 2, 1] and _c(idx, np.int32, (5,))
    assert _c(te, np.float64, (5, 12)) and _c(tg, np.float64, (5, 12))
    assert np.array_equal(te, Te[:, :3, :].reshape(5, 12)) and np.array_equal(tg, Tg[:, :3, :].reshape(5, 12))
    assert np.array_equal(bop_eval.stage_pairs(INDEX, [3, 7, 7, 11, 3], None, Te[:, :3, :].reshape(5, 12))[3], te)      # already packed: unchanged


def test_one_camera_matrix_is_repeated_and_n_are_kept():
    T = _poses(3, 3)
    K1 = np.array([[500.0, 0.0, 80.0], [0.0, 510.0, 48.0], [0.0, 0.0, 1.0]])
    Kn = np.stack([K1, 2 * K1, 3 * K1])
    _, _, one, _ = bop_eval.stage_pairs(INDEX, [7, 7, 3], K1, T)
    _, _, per, _ = bop_eval.stage_pairs(INDEX, [7, 7, 3], Kn, T)
    assert _c(one, np.float64, (3, 9)) and _c(per, np.float64, (3, 9))
    assert np.array_equal(one, np.tile(K1.reshape(1, 9), (3, 1))) and np.array_equal(per, Kn.reshape(3, 9))
    assert bop_eval.stage_pairs(INDEX, [7, 7, 3], Kn.reshape(3, 9).astype(np.float32), T)[2].dtype == np.float64


def test_torch_inputs_non_contiguous_inputs_and_other_dtypes():
    T = _poses(4, 4, 5)
    K = np.arange(9.0).reshape(3, 3)
    want = bop_eval.stage_pairs(INDEX, [3, 3, 11, 7], K, T)
    got = bop_eval.stage_pairs(INDEX, np.array([3, 3, 11, 7]), torch.from_numpy(K), torch.from_numpy(T).requires_grad_(True))
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(want[1:], got[1:]))
    f32 = bop_eval.stage_pairs(INDEX, [3, 3, 11, 7], None, torch.from_numpy(T).float())[3]
    assert _c(f32, np.float64, (4, 12)) and np.array_equal(f32, T.astype(np.float32)[:, :3].reshape(4, 12).astype(np.float64))
    strided = np.asfortranarray(T)
    assert np.array_equal(bop_eval.stage_pairs(INDEX, [3, 3, 11, 7], None, strided)[3], want[3])


def test_no_items():
    n, idx, K, te, tg = bop_eval.stage_pairs(INDEX, [], np.eye(3), np.zeros((0, 3, 4)), [])
    assert n == 0 and _c(idx, np.int32, (0,)) and _c(K, np.float64, (0, 9)) and _c(te, np.float64, (0, 12)) and _c(tg, np.float64, (0, 12))
    assert bop_eval.stage_pairs(INDEX, [], None)[2] is None and len(bop_eval.stage_pairs(INDEX, [], None)) == 3


def test_unknown_object_is_a_key_error():
    with pytest.raises(KeyError):
        bop_eval.stage_pairs(INDEX, [7, 8], None, _poses(2, 3))
    with pytest.raises(KeyError):
        bop_eval.stage_pairs({}, [7], None)


def test_images_a_call_names_are_stacked_in_ascending_order_and_re_indexed():
    images = [np.full((2, 3), float(i), np.float64) for i in range(6)]
    test, ii = bop_eval.stage_images(images, [4, 1, 4, 5, 1])
    assert _c(test, np.float32, (3, 2, 3)) and test[:, 0, 0].tolist() == [1.0, 4.0, 5.0]
    assert _c(ii, np.int32, (5,)) and ii.tolist() == [1, 0, 1, 2, 0]
    test, ii = bop_eval.stage_images({(0): images[0], 9: images[3]}, np.array([9, 9]))       # anything indexable by the integers named
    assert test.shape == (1, 2, 3) and test[0, 0, 0] == 3.0 and ii.tolist() == [0, 0]
    with pytest.raises(ValueError):
        bop_eval.stage_images([np.zeros((2, 3)), np.zeros((3, 3))], [0, 1])                    # one size a call
