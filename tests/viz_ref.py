"""The rules of a view's three-panel visualisation (include/suo_hip.h, "A view's three-panel visualisation"), restated in numpy: integers, fp64 and fp32, written
from the rules and not from the kernels.  Two users:

  tests/golden/make_viz_golden.py   its cv2 stand-in rasterises the reference's own draw calls through disc / ellipse / box / dilate3 / gray
  tests/test_viz_ref.py, tests/test_gpu_viz.py, tools/bench_viz.py     render(frame, prims, points) is what suo_viz_view must equal, byte for byte

``prims`` is what suo_slam_amd.viz.build_primitives returns: "box" int [n,5] (x1, y1, x2, y2, colour), "stamp" int [n,8] (channel, ulx, uly, x0, x1, y0, y1,
object), "kp" int [n,8] (x, y, r_outer, r_inner, colour, has_ellipse, A, B), "kp_angle" float64 [n] (degrees, as handed to cv2.ellipse), "overlay" a list of
(obj_id, colour, T [3,4], K [3,3]) in paint order.  A colour is packed b | g << 8 | r << 16.  ``points``: {obj_id: float32 [P,3]}."""
import math

import numpy as np

NUM_KP = 41
HALF = 45


def unpack(colour):
    return [int(colour) & 255, (int(colour) >> 8) & 255, (int(colour) >> 16) & 255]


def pack(bgr):
    return int(bgr[0]) | int(bgr[1]) << 8 | int(bgr[2]) << 16


def stamp_weights():
    """w[i] = exp(-(i - 45)^2 / (2 sigma^2)), sigma = 0.3 ((91 - 1) 0.5 - 1) + 0.8 = 14, doubled at the two ends (BORDER_REFLECT_101): through math.exp, the C
    library's exp that the product's table is made with."""
    sigma = 0.3 * ((2 * HALF + 1 - 1) * 0.5 - 1) + 0.8
    w = np.zeros(2 * HALF + 1)
    for i in range(2 * HALF + 1):
        d = float(i) - (2 * HALF) // 2
        w[i] = math.exp(-(d * d) / (2 * sigma * sigma)) * (2.0 if i in (0, 2 * HALF) else 1.0)
    return w


def _window(lo, hi, n):
    return max(int(lo), 0), min(int(hi), n)


def disc(img, x, y, r, bgr):
    """Pixels with dx^2 + dy^2 <= r^2, in integers."""
    H, W = img.shape[:2]
    x0, x1 = _window(x - r, x + r + 1, W)
    y0, y1 = _window(y - r, y + r + 1, H)
    if x0 >= x1 or y0 >= y1:
        return img
    dx = np.arange(x0, x1, dtype=np.int64)[None, :] - int(x)
    dy = np.arange(y0, y1, dtype=np.int64)[:, None] - int(y)
    img[y0:y1, x0:x1][dx * dx + dy * dy <= int(r) * int(r)] = bgr
    return img


def cos_sin(angle_deg):
    phi = float(angle_deg) * math.pi / 180
    return math.cos(phi), math.sin(phi)


def _inside(xr, yr, a, b):
    ab = float(a) * float(b)
    t1, t2 = xr * float(b), yr * float(a)
    return t1 * t1 + t2 * t2 <= ab * ab


def ellipse(img, x, y, A, B, angle_deg, bgr):
    """The outline of thickness 2: inside(A + 1, B + 1) and not (A >= 2 and B >= 2 and inside(A - 1, B - 1)), in fp64."""
    H, W = img.shape[:2]
    A, B = int(A), int(B)
    R = max(A, B) + 1
    x0, x1 = _window(x - R, x + R + 1, W)
    y0, y1 = _window(y - R, y + R + 1, H)
    if x0 >= x1 or y0 >= y1:
        return img
    c, s = cos_sin(angle_deg)
    dx = (np.arange(x0, x1, dtype=np.int64)[None, :] - int(x)).astype(np.float64)
    dy = (np.arange(y0, y1, dtype=np.int64)[:, None] - int(y)).astype(np.float64)
    xr = dx * c + dy * s
    yr = -dx * s + dy * c
    hit = _inside(xr, yr, A + 1, B + 1)
    if A >= 2 and B >= 2:
        hit &= ~_inside(xr, yr, A - 1, B - 1)
    img[y0:y1, x0:x1][hit] = bgr
    return img


def box(img, x1, y1, x2, y2, bgr):
    """Thickness 3: inside [x1 - 1, x2 + 1] x [y1 - 1, y2 + 1] and not inside [x1 + 2, x2 - 2] x [y1 + 2, y2 - 2]."""
    H, W = img.shape[:2]
    xs = np.arange(W, dtype=np.int64)[None, :]
    ys = np.arange(H, dtype=np.int64)[:, None]
    x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
    outer = (xs >= x1 - 1) & (xs <= x2 + 1) & (ys >= y1 - 1) & (ys <= y2 + 1)
    inner = (xs >= x1 + 2) & (xs <= x2 - 2) & (ys >= y1 + 2) & (ys <= y2 - 2)
    img[outer & ~inner] = bgr
    return img


def dilate3(mask):
    """3 x 3 square; nothing enters from outside the canvas."""
    m = np.asarray(mask)
    out = m.copy()
    H, W = m.shape
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] = np.maximum(out[yd, xd], m[ys, xs])
    return out


def gray(bgr):
    """OpenCV's documented 8-bit BGR2GRAY."""
    v = bgr.astype(np.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).astype(np.uint8)


def prior_image(H, W, stamps, kp_colours):
    """uint8 [H,W,3]: per channel the float32 sum of its stamps in list order, clipped to [0, 1], times the channel's colour, summed in fp64, clipped, truncated."""
    w = stamp_weights()
    acc = np.zeros((H, W, 3), np.float64)
    stamps = np.asarray(stamps, np.int64).reshape(-1, 8)
    for k in range(NUM_KP):
        sk = np.zeros((H, W), np.float32)
        for ch, ulx, uly, x0, x1, y0, y1, _ in stamps:
            if ch != k:
                continue
            lx, hx = _window(max(ulx, x0), min(ulx + 2 * HALF, x1), W)
            ly, hy = _window(max(uly, y0), min(uly + 2 * HALF, y1), H)
            if lx >= hx or ly >= hy:
                continue
            sk[ly:hy, lx:hx] += (w[np.arange(ly, hy) - uly][:, None] * w[np.arange(lx, hx) - ulx][None, :]).astype(np.float32)
        sk = np.clip(sk, np.float32(0), np.float32(1))
        acc += sk.astype(np.float64)[..., None] * np.asarray(kp_colours[k], np.float64)[None, None, :]
    return np.trunc(np.clip(acc, 0, 255)).astype(np.uint8)


def blend(img, prior):
    """p = float32(gray) / 255, out = uint8(trunc((1 - p) img + p prior)) in fp32."""
    p = gray(prior).astype(np.float32)[..., None] / np.float32(255)
    return ((np.float32(1) - p) * img.astype(np.float32) + p * prior.astype(np.float32)).astype(np.uint8)


def project(points, T, K):
    """(u + 0.5, v + 0.5) of every point in fp64, in the rule's order of operations; non-finite where the rule skips."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64)
    K = np.asarray(K, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        X = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
        Y = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
        Z = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
        a = (K[0, 0] * X + K[0, 1] * Y) + K[0, 2] * Z
        b = (K[1, 0] * X + K[1, 1] * Y) + K[1, 2] * Z
        c = (K[2, 0] * X + K[2, 1] * Y) + K[2, 2] * Z
        u, v = a / c, b / c
        ok = np.isfinite(u) & np.isfinite(v)
        uh, vh = u + 0.5, v + 0.5
        ok &= (np.abs(uh) < 2.0 ** 31) & (np.abs(vh) < 2.0 ** 31)
    return np.where(ok, uh, np.nan), np.where(ok, vh, np.nan)


def boundary_margin(points, T, K, H, W):
    """The smallest distance of a projected u + 0.5 or v + 0.5 to an integer, over the points within two pixels of the canvas (farther ones miss it under any
    rounding): the float32 projection of the reference and the fp64 rule pick the same pixel when this is well above float32's error."""
    uh, vh = project(points, T, K)
    near = np.isfinite(uh) & (uh > -2) & (uh < W + 2) & (vh > -2) & (vh < H + 2)
    if not near.any():
        return np.inf
    d = np.concatenate((uh[near], vh[near]))
    return float(np.abs(d - np.rint(d)).min())


def splat_mask(points, T, K, H, W):
    uh, vh = project(points, T, K)
    ok = np.isfinite(uh)
    px, py = np.trunc(uh[ok]).astype(np.int64), np.trunc(vh[ok]).astype(np.int64)
    keep = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    mask = np.zeros((H, W), bool)
    mask[py[keep], px[keep]] = True
    return mask


def render(frame, prims, points, kp_colours):
    """uint8 [H,3W,3]: left | centre | right."""
    frame = np.ascontiguousarray(frame, np.uint8)
    H, W = frame.shape[:2]
    left, centre, right = frame.copy(), frame.copy(), frame.copy()
    for x1, y1, x2, y2, col in np.asarray(prims["box"], np.int64).reshape(-1, 5):
        box(left, x1, y1, x2, y2, unpack(col))
    left = blend(left, prior_image(H, W, prims["stamp"], kp_colours))
    for (x, y, ro, ri, col, has, A, B), ang in zip(np.asarray(prims["kp"], np.int64).reshape(-1, 8), prims["kp_angle"]):
        disc(centre, x, y, ro, [0, 0, 0])
        disc(centre, x, y, ri, unpack(col))
        if has:
            ellipse(centre, x, y, A, B, ang, unpack(col))
    for obj_id, col, T, K in prims["overlay"]:
        m = dilate3(splat_mask(points[obj_id], T, K, H, W))
        right[m] = unpack(col)
    return np.concatenate((left, centre, right), axis=1)
