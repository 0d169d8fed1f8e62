"""Numpy yardstick of the scene_gt_info / ground-truth mask row (N7); a helper, not a test.

A fp64 restatement of the definition in include/suo_hip.h (suo_gt_info, suo_gt_masks) over the numpy rasteriser of tests/vsd_ref.py, written from that
definition.  tests/test_gt_info_host.py ties it to the toolkit: on the cases of tests/golden/gt_info_cases.py it reproduces what the toolkit's own scripts
wrote (tests/golden/gt_info_golden.npz) exactly."""
import numpy as np

from tests import vsd_ref as VR


def dist_im(depth, K):
    """misc.depth_im_to_dist_im: Xs = ((x - cx) d) (1 / fx), Ys likewise, sqrt((Xs^2 + Ys^2) + d^2) in fp64 on the float32 depth."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    depth = np.asarray(depth, np.float32)
    xs, ys = np.meshgrid(np.arange(depth.shape[1]), np.arange(depth.shape[0]))
    with np.errstate(all="ignore"):
        Xs = ((xs - K[0, 2]) * depth.astype(np.float64)) * (1.0 / K[0, 0])
        Ys = ((ys - K[1, 2]) * depth.astype(np.float64)) * (1.0 / K[1, 1])
        return np.sqrt((Xs * Xs + Ys * Ys) + depth.astype(np.float64) * depth.astype(np.float64))


def visib_mask(dist_test, dist_gt, delta):
    with np.errstate(all="ignore"):
        diff = dist_gt.astype(np.float32) - dist_test.astype(np.float32)
        return ((diff <= np.float32(delta)) | (dist_test == 0)) & (dist_gt > 0)


def _bbox(mask, off_x=0, off_y=0):
    ys, xs = mask.nonzero()
    xs, ys = xs - off_x, ys - off_y
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def canvas_K(K, width, height):
    """The camera of the 3 width x 3 height canvas: the principal point moved by (width, height), summed in fp64."""
    Kc = np.array(K, np.float64).reshape(3, 3)
    Kc[0, 2] = Kc[0, 2] + width
    Kc[1, 2] = Kc[1, 2] + height
    return Kc


def gt_info(points, faces, T, K, depth_test, delta=15, details=False):
    """The six entries of scene_gt_info.json for one instance.  ``details``: also ``(depth_gt_large, near_large, min |float32 difference - delta|)`` for the
    conditions the fixtures must meet."""
    depth_test = np.asarray(depth_test, np.float32)
    H, W = depth_test.shape
    K = np.asarray(K, np.float64).reshape(3, 3)
    large, near = VR.render_depth(points, faces, T, canvas_K(K, W, H), 3 * W, 3 * H, with_near=True)
    depth_gt = large[H:2 * H, W:2 * W]
    dist_gt, dist_test = dist_im(depth_gt, K), dist_im(depth_test, K)
    visib = visib_mask(dist_test, dist_gt, delta)
    n_all, n_valid, n_visib = int((large > 0).sum()), int(((dist_gt > 0) & (dist_test > 0)).sum()), int(visib.sum())
    info = {"px_count_all": n_all, "px_count_valid": n_valid, "px_count_visib": n_visib, "visib_fract": n_visib / float(n_all) if n_all > 0 else 0.0,
            "bbox_obj": _bbox(large > 0, W, H) if n_visib > 0 else [-1, -1, -1, -1], "bbox_visib": _bbox(visib) if n_visib > 0 else [-1, -1, -1, -1]}
    if not details:
        return info
    return info, large, near, delta_margin(dist_gt, dist_test, delta)


def delta_margin(dist_gt, dist_test, delta):
    """min |float32 difference - delta| in mm over the pixels where the comparison decides (a model distance, a measurement)."""
    sel = (dist_gt > 0) & (dist_test != 0)
    if not sel.any():
        return np.inf
    diff = (dist_gt.astype(np.float32) - dist_test.astype(np.float32))[sel].astype(np.float64)
    return float(np.abs(diff - delta).min())


def gt_masks(points, faces, T, K, depth_test, delta=15, details=False):
    """``(mask, mask_visib)`` uint8 [H,W] of one instance, rendered on the plain canvas as calc_gt_masks.py does."""
    depth_test = np.asarray(depth_test, np.float32)
    H, W = depth_test.shape
    K = np.asarray(K, np.float64).reshape(3, 3)
    depth_gt, near = VR.render_depth(points, faces, T, K, W, H, with_near=True)
    dist_gt, dist_test = dist_im(depth_gt, K), dist_im(depth_test, K)
    out = 255 * (dist_gt > 0).astype(np.uint8), 255 * visib_mask(dist_test, dist_gt, delta).astype(np.uint8)
    return out + (depth_gt, near) if details else out
