#!/usr/bin/env python3
"""What the opt-in landmark report costs a step: the bench's configs[2] step (bench.py's default workload: BU_3DFE-RGB+depth,
96 views of the 224-grid face, 84 landmarks, synthetic weights) and its 478 x 128 fusion stress (configs[4]: render + dense
fusion around synthetic 2-D landmarks) with ``Pipeline.landmark_report`` off and on, alternating: ms per step of each.
usage: tools/report_step_bench.py [steps] > profiles/report_step.txt   (it prints; the committed file is that output)"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

import bench
from mvlm_amd import config, pipeline
from mvlm_amd.utils.synthetic import face_like_mesh


def measure(label, pipe, mesh, poses, steps):
    ms = {False: [], True: []}
    for rnd in range(3):
        for on in (False, True):
            pipe.landmark_report = on
            pipe._buffers.pop("result", None)       # (the result buffer only grows: without the report it is the small one again)
            pipe._buffers.pop("result_host", None)
            for _ in range(3):
                np.random.seed(1)
                pipe.predict_mesh_device(mesh, poses)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                np.random.seed(1)
                pipe.predict_mesh_device(mesh, poses)
            torch.cuda.synchronize()
            ms[on].append(1e3 * (time.perf_counter() - t) / steps)
    off, on = np.median(ms[False]), np.median(ms[True])
    for flag, r in ms.items():
        print(f"{label}, landmark_report={flag}: {np.median(r):.3f} ms per step (rounds {', '.join(f'{v:.3f}' for v in r)})")
    print(f"{label}: the report adds {on - off:+.3f} ms per step ({100 * (on - off) / off:+.1f} %)")


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    mesh = face_like_mesh(224, 2048, seed=0)
    pipe = config.load_config(config.default_config("BU_3DFE", "RGB+depth", n_views=96)).build_pipeline(weights="synthetic:0", verbose=False)
    np.random.seed(0)
    measure("configs[2] step (96 views, 84 landmarks)", pipe, mesh, pipe.renderer_3d.generate_3d_transformations(), steps)
    del pipe
    pipe = pipeline.Pipeline(n_views=128, verbose=False)
    np.random.seed(0)
    poses = pipe.renderer_3d.generate_3d_transformations()
    pipe.predictor_2d, _, _ = bench.synthetic_landmark_predictor(mesh, poses, 478, torch.device("cuda", 0))
    measure("fusion stress (128 views, 478 landmarks)", pipe, mesh, poses, steps)


if __name__ == "__main__":
    main()
