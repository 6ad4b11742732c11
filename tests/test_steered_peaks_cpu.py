"""The steered peaks of tests/steered_peaks.py on the CPU oracle: every steered plane peaks at its target with the runner-up at
least 1 % below, and the reference's moment rule refines exactly the targets more than 15 pixels inside.  The same scenes go
through the fused window kernel in tests/test_gpu_steered_peaks.py."""
import numpy as np
import pytest

import steered_peaks as sp
from mvlm_amd import arch
from oracle import cnn as ocnn


def test_the_targets_cover_every_threshold_in_every_row_group():
    for nl in (73, 84):
        tg = sp.targets(nl)
        groups = [range(0, 64), range(64, 80)] + ([range(80, 84)] if nl == 84 else [])
        for g in groups:
            rows = {y for k, y, _ in tg if k in g}
            cols = {x for k, _, x in tg if k in g}
            assert {15, 16, 240, 241} <= rows and {15, 16, 240, 241} <= cols, (nl, g)
        first = {(y, x) for k, y, x in tg if k < 64}
        assert set(sp.CORNERS + sp.IMAGE_CORNERS) <= first
        assert {(y % 2, x % 2) for y, x in sp.INTERIOR} == {(0, 0), (0, 1), (1, 0), (1, 1)} and all(sp.refined(*p) for p in sp.INTERIOR)
        plan = sp.assign_views(tg)
        for v in {v for _, v, _, _ in plan}:
            blocks = [(2 * (y // 2), 2 * (x // 2)) for _, w, y, x in plan if w == v]
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= sp.MIN_DISTANCE for n, a in enumerate(blocks) for b in blocks[:n])


@pytest.mark.parametrize("nl,mode", [(73, "RGB"), (84, "RGB+depth")])
def test_steered_peaks_land_on_their_targets_on_the_oracle(nl, mode):
    sd, images, plan = sp.steered_scene(nl, mode)
    assert 2 <= images.shape[0] <= sp.MAX_VIEWS
    assert np.count_nonzero(sd["conv11.weight"]) == sd["conv11.weight"].size
    _, _, heat = ocnn.predict_landmarks_from_images(sd, images, arch.CHANNEL_SELECT[mode], return_heatmaps=True)
    heat = heat.numpy()
    simple = ocnn.maxima_from_heatmaps(heat, "simple")
    moment = ocnn.maxima_from_heatmaps(heat, "moment")
    assert sp.check_targets(simple, plan) == []
    worst = 0.0
    for k, v, y, x in plan:
        plane = heat[v, k]
        peak = plane[y, x]
        second = np.partition(plane.ravel(), -2)[-2]
        worst = max(worst, second / peak)
        assert peak > 0 and second <= 0.99 * peak, (k, v, y, x, peak, second)
        was_refined = not np.array_equal(moment[k, v, :2], simple[k, v, :2])
        assert was_refined == sp.refined(y, x), (k, v, y, x)
        assert moment[k, v, 2] == simple[k, v, 2] == peak
    print(f"\nsteered peaks {nl} {mode}: {len(plan)} targets in {images.shape[0]} views, every peak on its target, largest runner-up {worst:.4f} of its peak")
