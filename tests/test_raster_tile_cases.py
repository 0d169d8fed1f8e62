"""The inputs of tests/raster_tile_cases.py reach what they were designed to reach -- on the numpy rasteriser and the route census alone, no GPU, so that
tests/test_gpu_raster_tile_edges.py cannot pass without having asked the device the question."""
import numpy as np

from tests import gt_info_ref as GR
from tests import raster_tile_cases as RC
from tests import vsd_ref as VR

NEAR_CAP = 1e-3                 # the share of samples within the NEAR band an image may hold: the cap of tests/test_gpu_vsd.py


def test_sizes_hold_every_store_and_tile_edge():
    assert RC.SIZES == [(1, 1), (3, 2), (5, 64), (63, 65), (64, 64), (65, 63), (67, 70), (97, 130), (131, 67), (161, 99)]
    widths = {w % 4 for w, _ in RC.SIZES + RC.CHUNK_SIZES + RC.RECT_SIZES}
    assert widths == {0, 1, 2, 3}
    assert any(w % 64 == 1 for w, _ in RC.SIZES) and any(h % 64 == 1 for _, h in RC.SIZES)                 # a last tile column / row of one pixel
    assert any(w < 64 and h < 64 for w, h in RC.SIZES) and (1, 1) in RC.SIZES                               # smaller than a tile
    assert sum(w % 4 != 0 for w, _ in RC.CHUNK_SIZES) == 2 and (160, 96) in RC.CHUNK_SIZES
    assert RC.ODD[0] % 4 != 0 and RC.ODD in RC.CHUNK_SIZES
    m = RC.meshes()
    assert len(m["ico3"][1]) == 1280 and len(m["shingles"][1]) == 700 and len(m["full_list"][1]) >= 300 and len(m["box"][1]) == 12
    assert all(len(f) <= 1400 for _, f in m.values())


def test_every_render_case_is_clear_of_triangle_edges_and_draws():
    for lab, (mesh, T, K, w, h) in RC.render_cases().items():
        depth, near = RC.reference(lab)
        assert depth.shape == (h, w) and near.mean() <= NEAR_CAP, (lab, near.mean())
        assert (depth > 0).any(), lab
        if (w, h) in ((1, 1), (3, 2)):
            assert (depth > 0).all(), lab                                       # the pixel(s) of the smallest images are covered
    labels = list(RC.render_cases())
    for w, h in RC.SIZES:
        assert f"sizes/box@{w}x{h}" in labels and f"sizes/ico3@{w}x{h}" in labels
    for w, h in RC.CHUNK_SIZES:
        assert all(f"chunks/{name}@{w}x{h}" in labels for name in ("ico3_near", "ico3_far", "shingles", "full_list"))


def test_close_ups_cross_every_tile_boundary_present():
    """A triangle of the box on the list of every tile of the image, at every size that has more than 32 samples in each tile."""
    for w, h in RC.SIZES:
        c = RC.case_census(f"sizes/box@{w}x{h}")
        tx, ty = (w + 63) // 64, (h + 63) // 64
        assert c["list"].shape == (tx * ty, 1)
        big_tiles = [t for t in range(tx * ty) if (min(64, w - 64 * (t % tx)) * min(64, h - 64 * (t // tx))) > 4 * RC.SMALL]
        assert all(c["list"][t, 0] > 0 for t in big_tiles), (w, h, c["list"].ravel())
        assert ((c["samples"] > 0).sum(1) == tx * ty).any() or tx * ty == 1, (w, h)      # one triangle meets every tile


def test_chunk_and_list_coverage():
    cens = {lab: RC.case_census(lab) for lab in RC.render_cases() if lab.startswith("chunks/")}
    # a tile whose list is non-empty in at least 3 different chunks
    for name in ("ico3_near", "shingles"):
        for w, h in RC.CHUNK_SIZES:
            c = cens[f"chunks/{name}@{w}x{h}"]
            assert ((c["list"] > 0).sum(1) >= 3).any(), (name, w, h)
    # full_list: 256 entries in a chunk of its tile and a non-empty list in the next -- here 256, 256, then the rest
    for w, h in RC.CHUNK_SIZES + [(64, 64)]:
        c = cens[f"chunks/full_list@{w}x{h}"]
        assert c["list"][0].tolist() == [256, 256, RC.N_FULL - 512] and c["lane"].sum() == 0 and c["list"][1:].sum() == 0, (w, h, c["list"])
        assert c["samples"][:, 0].min() > RC.SMALL
    # both routes for one triangle, in neighbouring tiles
    assert all(cens[f"chunks/shingles@{w}x{h}"]["both"] >= 50 for w, h in RC.CHUNK_SIZES)
    # many lanes walking their own triangle, in at least 4 chunks
    for w, h in RC.CHUNK_SIZES:
        c = cens[f"chunks/ico3_far@{w}x{h}"]
        assert c["lane"].sum() >= 500 and (c["lane"].sum(0) > 0).sum() >= 4, (w, h)
    # lists and lanes in the same (tile, chunk), and a list that is long but not full
    c = cens["chunks/shingles@%dx%d" % RC.ODD]
    assert ((c["list"] > 0) & (c["lane"] > 0)).any() and 100 <= c["list"].max() < 256


def test_threshold_rectangles_sit_on_the_threshold():
    P, F = RC.meshes()["threshold_rects"]
    u, v, Z = VR.project(P, RC.RECT_T, RC.RECT_K)
    assert np.array_equal(u, np.round(u)) and np.array_equal(v, np.round(v)) and set(Z.tolist()) <= {2.0, 4.0, 8.0}      # integers throughout
    for w, h in RC.RECT_SIZES:
        c = RC.census(P, F, RC.RECT_T, RC.RECT_K, w, h)
        seen = set(c["samples"].ravel().tolist())
        assert RC.SMALL in seen and RC.SMALL + 1 in seen, (w, h, sorted(seen))
        s = c["samples"][6]                                                     # the rectangle across x = 64
        assert s[0] == 32 and s[1] == 40 and c["both"] >= 2
    c = RC.census(P, F, RC.RECT_T, RC.RECT_K, 130, 66)
    assert sorted(c["samples"][8][c["samples"][8] > 0].tolist()) == [4, 12, 16, 48]      # four tiles, the last column and row two pixels wide


def test_mask_and_gt_cases_are_exact_on_the_reference():
    """The integer comparisons allow no sample in the NEAR band at all, and the visibility decision must stay clear of delta."""
    for lab, mesh, Te, Tg, K, w, h, e, g in RC.mask_pairs():
        assert not RC.reference(e)[1].any() and not RC.reference(g)[1].any(), lab
        me, mg = RC.reference(e)[0] > 0, RC.reference(g)[0] > 0
        assert (me & mg).any() and (me ^ mg).any(), lab
    for lab, mesh, T, K, test in RC.gt_cases():
        P, F = RC.meshes()[mesh]
        info, large, near_l, margin = GR.gt_info(P, F, T, K, test, RC.DELTA, details=True)
        _, mask_visib, _, near_p = GR.gt_masks(P, F, T, K, test, RC.DELTA, details=True)
        assert not near_l.any() and not near_p.any() and margin > 1e-3, (lab, margin)
        assert large.shape == (210, 201)
        assert 0 < info["px_count_visib"] < info["px_count_valid"] < info["px_count_all"], (lab, info)      # occluded in part, and past the image
        assert info["bbox_obj"][0] < 0 and info["bbox_obj"][1] < 0
