"""The tiled rate-distortion probe's prediction, stated in numpy (tests/rd_nd_cases.py) and held against the oracle's own decode:
the reference alone stays inside the tolerances tests/test_gpu_rd_probe_nd.py and tests/test_gpu_psnr_target_nd.py hold the
GPU to.  The statement leans on dctzhip_rd_probe_nd's documented contract (include/dctz_hip.h): the padded places' share is
taken out with the inverse transform of the coefficient errors."""
import os

import numpy as np
import pytest

from tests import rd_nd_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_contract_is_documented():
    with open(os.path.join(ROOT, "include", "dctz_hip.h")) as f:
        hdr = " ".join(f.read().split())
    assert "int dctzhip_rd_probe_nd(" in hdr and "int dctzhip_compress_psnr_nd(" in hdr
    assert "The edge padding of the streams enters no field" in hdr


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", R.SMALL, ids=lambda s: "x".join(map(str, s)))
def test_prediction_matches_the_oracles_decode(shape, dtype):
    x = R.array(shape, dtype)
    worst = 0.0
    for eb in R.EBS:
        ref = R.reference(shape, dtype, eb)
        if not R.sse_checked(shape, dtype, eb):
            continue
        assert R.sse_ok(ref["pred"], ref["meas"], x), (shape, eb, ref["pred"], ref["meas"], abs(ref["pred"] - ref["meas"]) / ref["meas"])
        if ref["meas"] > 0:
            worst = max(worst, abs(ref["pred"] - ref["meas"]) / ref["meas"])
    print(f"worst relative SSE miss of the numpy prediction, {shape} {np.dtype(dtype).name}: {worst:.3e}")


@pytest.mark.parametrize("shape", [(9, 4099), (5, 6, 7)], ids=lambda s: "x".join(map(str, s)))
def test_the_padded_share_is_a_real_part_of_the_layouts_error(shape):
    """What the GPU file's padding test leans on: at 1e-3 the array's own SSE is well under the padded layout's."""
    ref = R.reference(shape, np.float64, 1e-3)
    assert abs(ref["pred_padded_layout"] - ref["meas_padded_layout"]) <= R.SSE_RTOL_F64 * ref["meas_padded_layout"]
    ratio = ref["meas"] / ref["meas_padded_layout"]
    print(f"{shape}: SSE over the array / over the padded layout = {ratio:.3f}")
    assert ratio < 0.97


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", R.TARGET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_search_on_the_predictions_lands_on_the_right_point(shape, dtype):
    g = R.grid()
    assert len(g) == 61 and g == sorted(g) and g[0] == 1e-6 and g[-1] == 1.0
    for target in R.TARGETS:
        at = R.search(shape, dtype, target)
        assert at is not None, (shape, target)
        got = R.measured_psnr(shape, dtype, g[at])
        assert got >= target, (shape, target, g[at], got)
        if at + 1 < len(g):
            nxt = R.measured_psnr(shape, dtype, g[at + 1])
            assert nxt < target, (shape, target, g[at + 1], nxt)
