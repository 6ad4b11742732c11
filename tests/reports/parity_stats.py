#!/usr/bin/env python3
"""Report how far the HIP network is from the CPU oracle (torch fp32, oneDNN): heatmap
deviation and argmax differences.  Test infrastructure (imports oracle/); run on the GPU box.
usage: tests/reports/parity_stats.py [n_views]   (the exact path, then the two opt-in precisions against the same oracle; each
with its class table against a float64 forward pass, tests/net_reference.py)"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))  # tests/ (conftest helpers)
import net_reference as nr  # noqa: E402
from conftest import seeded_images  # noqa: E402
from mvlm_amd import arch, weights  # noqa: E402
from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor  # noqa: E402
from oracle import cnn as ocnn  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
for nl, mode, c, seed in ((73, "RGB", 3, 1), (84, "RGB+depth", 4, 2)):
    imgs = seeded_images(500 + seed, n)
    cls = BU3DFEPredictor if nl == 84 else DTU3DPredictor
    pred = cls(image_mode=mode, weights=f"synthetic:{seed}", verbose=False)
    sd = weights.synthetic_state_dict(nl, c, seed=seed)
    lms, _, oheat = ocnn.predict_landmarks_from_images(sd, imgs, arch.CHANNEL_SELECT[mode], return_heatmaps=True)
    oheat = oheat.numpy()
    scale = np.abs(oheat).max()
    top2 = np.sort(oheat.reshape(n, nl, -1), axis=2)[:, :, -2:]
    gap = (top2[..., 1] - top2[..., 0]) / scale
    ref64 = nr.heatmaps_f64(sd, imgs, arch.CHANNEL_SELECT[mode])
    table_ref = nr.error_table(oheat, ref64)
    for precision in ("exact", "fast", "fast16"):
        pred.set_precision(precision)
        heat = pred.heatmaps_device(torch.from_numpy(imgs).cuda()).cpu().numpy()
        mine = ocnn.maxima_fast(torch.from_numpy(heat))
        d = np.abs(heat - oheat)
        flips = int((~np.all(mine[:, :, :2] == lms[:, :, :2], axis=2)).sum())
        print(f"{nl}_{mode} {precision:6s}: max|d|/max|h| = {d.max() / scale:.3e}  mean|d|/max|h| = {d.mean() / scale:.3e}  "
              f"argmax differences {flips}/{n * nl}  (oracle top-2 gap: min {gap.min():.2e}, median {np.median(gap):.2e})")
        print(nr.format_table(f"{nl}_{mode} {precision}: HIP against float64, S = {np.abs(ref64).max():.4g}", nr.error_table(heat, ref64), table_ref, 8))
