#!/usr/bin/env python3
"""The bench's configs[2] step (bench.py's default workload: BU_3DFE-RGB+depth, 96 views of the 224-grid face, synthetic
weights) with the renderer at 0 and at 4 samples per pixel (Pipeline(render_multisamples=...)): views/s of each, alternating.
usage: tools/msaa_step_bench.py [steps]  -> profiles/<tag>_msaa_step.txt"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd import config
from mvlm_amd.utils.synthetic import face_like_mesh


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    mesh = face_like_mesh(224, 2048, seed=0)
    cfg = config.load_config(config.default_config("BU_3DFE", "RGB+depth", n_views=96))
    pipe = cfg.build_pipeline(weights="synthetic:0", verbose=False)
    np.random.seed(0)
    poses = pipe.renderer_3d.generate_3d_transformations()
    rates = {0: [], 4: []}
    for rnd in range(3):
        for samples in (0, 4):
            pipe.renderer_3d.multisamples = samples
            for _ in range(3):
                np.random.seed(1)
                pipe.predict_mesh_device(mesh, poses)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                np.random.seed(1)
                pipe.predict_mesh_device(mesh, poses)
            torch.cuda.synchronize()
            rates[samples].append(96 * steps / (time.perf_counter() - t))
    for samples, r in rates.items():
        print(f"configs[2] step, {samples} samples: {np.median(r):.1f} views/s (rounds {', '.join(f'{v:.1f}' for v in r)})")


if __name__ == "__main__":
    main()
