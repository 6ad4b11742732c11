"""-m gpu: the fused "moment" window (moment_refine_kernel, csrc/misc.hip) at its edges, with peaks steered there on purpose
(tests/steered_peaks.py): rows and columns 16 (the window's origin at an odd pixel) and 240 (its last row or column reads
low-resolution row or column 128, the zero padding), 15 and 241 (not refined at all), the corners, every parity, and each of
those on the 64 full rows of conv11's tile, on its 16-row strip and - 84 landmarks - on its 4-row strip; peaks in the image's
corners for the simple selection.  test_gpu_round4.py::test_fused_moment_equals_the_materialised_heatmaps asserts the same
equalities on whatever peaks seeded networks produce, which for 84 landmarks never met row 16, row 240 or column 240."""
import numpy as np
import pytest
import torch

import steered_peaks as sp

pytestmark = pytest.mark.gpu


def _three_passes(pred, imgs, out):
    """launch by launch, capture, replay: the three must agree, and the third must really be a replay"""
    before = pred.execution_stats()
    got = [pred.predict_device(imgs, out=out).clone() for _ in range(3)]
    after = pred.execution_stats()
    assert after["graph_replays"] > before["graph_replays"] and after["graph_failures"] == before["graph_failures"]
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    return got[2].cpu().numpy()


# (the 73-landmark network in device batches of 4 views out of 5: a second batch with a view offset)
@pytest.mark.parametrize("nl,mode,device_batch", [(73, "RGB", 4), (84, "RGB+depth", None)])
def test_steered_peaks_through_the_fused_window(monkeypatch, nl, mode, device_batch):
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor
    from oracle import cnn as ocnn

    sd, images, plan = sp.steered_scene(nl, mode)
    n_views = images.shape[0]
    assert device_batch is None or device_batch < n_views
    cls = BU3DFEPredictor if nl == 84 else DTU3DPredictor
    pred = cls(image_mode=mode, weights=sd, selection_method="moment", verbose=False, device_batch=device_batch)
    imgs = torch.from_numpy(images).cuda()
    out = torch.empty((nl, n_views, 3), dtype=torch.float32, device="cuda")
    fused = _three_passes(pred, imgs, out)
    monkeypatch.setenv("MVLM_MOMENT_MATERIALISED", "1")
    materialised = pred.predict_device(imgs).cpu().numpy()
    monkeypatch.delenv("MVLM_MOMENT_MATERIALISED")
    np.testing.assert_array_equal(fused, materialised)
    heat = pred.heatmaps_device(imgs).cpu().numpy()
    np.testing.assert_array_equal(fused, ocnn.maxima_from_heatmaps(heat, "moment"))
    want_simple = ocnn.maxima_from_heatmaps(heat, "simple")
    assert sp.check_targets(want_simple, plan) == []            # every steered plane of the HIP heatmaps peaks on its target
    for k, v, y, x in plan:
        was_refined = not np.array_equal(fused[k, v, :2], want_simple[k, v, :2])
        assert was_refined == sp.refined(y, x), (k, v, y, x, fused[k, v], want_simple[k, v])
        assert fused[k, v, 2] == want_simple[k, v, 2] == heat[v, k, y, x]
    pred.selection_method = "simple"
    simple = _three_passes(pred, imgs, out)                     # (the same buffers: the moment passes' graphs must not be replayed)
    np.testing.assert_array_equal(simple, want_simple)
    assert sp.check_targets(simple, plan) == []
    print(f"\nsteered peaks {nl} {mode}: {len(plan)} targets in {n_views} views (device batch {device_batch}), "
          f"{sum(sp.refined(y, x) for _, _, y, x in plan)} refined by the fused window, all on target")
