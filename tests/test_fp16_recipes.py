"""Host-side calibration of the bright / dim recipe (tests/fp16_recipes.py, (c)) that tests/test_gpu_fp16_fallback.py drives through the batched single-view
route: with the image channels of the stem scaled by 2^BRIGHT_DIM_GAIN_LOG2, normal frames take some activation beyond the fp16 form's limit and the same frames
divided by 16 stay inside it, each by a margin -- measured on the oracle, so the GPU tests' preconditions are not luck of the kernels.
The oracle runs in a child process (tests/fp16_recipes.py, __main__): CPU convolution libraries may round differently once a run of whole-network forwards has
reshaped this process's heap (alignment-dependent kernels), and tests/test_oracle_cnn.py holds the same oracle to stored logits at 2e-5 in this process."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("frames", ["synthetic", "bop_tree"])
def test_bright_frames_leave_the_fp16_range_and_dim_ones_do_not(frames, tmp_path):
    out = subprocess.run([sys.executable, "-m", "tests.fp16_recipes", frames, str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CALIBRATION ")][-1][len("CALIBRATION "):])
    assert len(res["cases"]) == (1 if frames == "synthetic" else 2)
    for bright, dark in res["cases"]:
        # (frames 16x apart are ~16.5x apart in every activation: no power-of-two gain can leave more than ~4x on both sides; 2^13 leaves 5x / 3x)
        assert bright >= 2.5 and dark <= 1.0 / 2.5, (bright, dark)
    # and the unscaled network stays far inside the range on the same frames (the recipe, not the frames, takes it out)
    assert res["unscaled"] < 0.01
