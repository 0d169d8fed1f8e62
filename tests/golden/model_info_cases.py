"""The seeded point clouds of the model-statistics row (N8) and their PLY files.  tests/golden/make_model_info_golden.py runs the toolkit on them and
records tests/golden/model_info_golden.npz; the tests regenerate them from the seeds.  Object ids are 1-based in the order of ``models()``.

Sizes stay small: the toolkit's scan is a Python loop over points.  They still cross the device's tiles (256 and 1024 points) once each; the GPU tests
build the sizes around the tiles themselves against tests/model_info_ref.py, which tests/test_model_info_ref.py ties to the toolkit here."""
import os

import numpy as np

SEED = 20261021


def _cloud(rng, n, scale, offset=(0.0, 0.0, 0.0)):
    return (rng.normal(size=(n, 3)) * scale + np.asarray(offset, np.float64)).astype(np.float32)


def models():
    """``[(label, float32 [n,3], format)]``; format "binary" or "ascii".  The ascii file is the twin of ``eighths``, whose coordinates are multiples of 1/8
    below 2^17: %.9g prints such a number exactly, so the toolkit's float64 parse of the text is the float32 value itself."""
    rng = np.random.default_rng(SEED)
    out = [("one", _cloud(rng, 1, 50.0), "binary"),
           ("two", _cloud(rng, 2, 50.0), "binary"),
           ("three", _cloud(rng, 3, 50.0), "binary"),
           ("small_1e-3", _cloud(rng, 257, 1e-3), "binary"),
           ("offset_1e4", _cloud(rng, 700, 1e4, (3e4, -2e4, 5e3)), "binary"),
           ("extent_1_at_1e6", (rng.uniform(0.0, 1.0, (1025, 3)) + 1e6).astype(np.float32), "binary"),
           ("negative_box", (-rng.uniform(1.0, 200.0, (2049, 3))).astype(np.float32), "binary"),
           ("identical", np.tile(_cloud(rng, 1, 80.0), (40, 1)), "binary")]
    dup = _cloud(rng, 600, 60.0)
    out.append(("duplicated", np.concatenate((dup, dup[::3], dup[:5])), "binary"))
    eighths = (np.round(_cloud(rng, 300, 2e4, (1e4, -3e4, 0.0)).astype(np.float64) * 8.0) / 8.0).astype(np.float32)
    assert np.abs(eighths).max() < 2 ** 17
    out.append(("eighths", eighths, "binary"))
    out.append(("eighths_ascii", eighths.copy(), "ascii"))
    return out


def write_ply(path, pts, fmt):
    """A vertex-only PLY file of float x, y, z: binary little endian, or ascii printed with %.9g -- asserted to be the float32 value exactly (nine digits
    identify a float32, but a reader that parses to float64, as the toolkit does, sees the float32 value only where the digits are all of it)."""
    pts = np.ascontiguousarray(pts, np.float32)
    head = ["ply", "format {} 1.0".format("binary_little_endian" if fmt == "binary" else "ascii"), f"element vertex {len(pts)}",
            "property float x", "property float y", "property float z", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "binary":
            f.write(pts.astype("<f4").tobytes())
        else:
            for p in pts:
                line = "%.9g %.9g %.9g" % (p[0], p[1], p[2])
                assert [float(t) for t in line.split()] == [float(v) for v in p], line
                f.write((line + "\n").encode("ascii"))


def write_models(model_dir, which=None):
    """obj_%06d.ply for every model (``which``: 1-based ids); returns the ids written."""
    ids = []
    for k, (_, pts, fmt) in enumerate(models()):
        if which is None or k + 1 in which:
            write_ply(os.path.join(model_dir, f"obj_{k + 1:06d}.ply"), pts, fmt)
            ids.append(k + 1)
    return ids
