#!/usr/bin/env python3
"""Stage times of the surface heat at the bench size (MI355X; the figures of DESIGN.md 5.1, "Surface heat", and section 8 - they gate
nothing): the 99 458-triangle mesh face_like_mesh(224, 256, seed=0), 96 views, the 84-landmark network's own heatmaps of those
views.  Peak, back-projection and paint from mvlm_surface_heat_stage_ms; beside them, from the same run, the heat sheet's three
stages on the same heatmaps and the second network pass (heatmaps_device) that either picture costs; and what the back-projection
moves: the (vertex, view) pairs that are seen, the 4-byte gathers they make, and those over the kernel's time.

    tools/surface_heat_bench.py [--out FILE]     print the table (and write it to FILE: profiles/surface_heat_time.txt)
"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mvlm_amd import config  # noqa: E402
from mvlm_amd.utils.render3d import view_rotations  # noqa: E402
from mvlm_amd.utils.synthetic import face_like_mesh  # noqa: E402

N_VIEWS, WARMUP, RUNS = 96, 3, 20
out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def events(fn, runs=RUNS, warmup=WARMUP):
    ms = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        keep = fn()
        e1.record()
        torch.cuda.synchronize()
        del keep
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


mesh = face_like_mesh(224, 256, seed=0)
pipe = config.load_config(config.default_config("BU_3DFE", "RGB+depth", n_views=N_VIEWS)).build_pipeline(weights="synthetic:0", verbose=False)
r3, p2 = pipe.renderer_3d, pipe.predictor_2d
ctx = r3.ctx
np.random.seed(0)
poses = r3.generate_3d_transformations()
rot = view_rotations(poses)
images = r3.render_device(mesh, poses).clone()
heat = p2.heatmaps_device(images)
r3.check()
n_lm = int(heat.shape[1])
say(f"surface heat, MI355X, {mesh.n_verts} vertices ({mesh.n_tris} triangles), {N_VIEWS} views x {n_lm} landmarks, the network's heatmaps "
    f"(synthetic weights): {heat.numel() * 4 / 1e9:.2f} GB; depth_tol 2")

ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 1))
try:
    rows, sheet = [], []
    for k in range(WARMUP + RUNS):
        res = r3.surface_heat(mesh, images, heat, rot)
        ms = r3.surface_heat_stage_ms()
        r3.render_heat_sheet_device(images, heat)
        hs = r3.heat_sheet_stage_ms()
        if k >= WARMUP:
            rows.append(ms.tolist())
            sheet.append(hs.tolist())
finally:
    ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 0))
n_vis = res["n_visible"].cpu().numpy().astype(np.int64)
peaks = torch.amax(torch.where(torch.isfinite(heat), heat, torch.full_like(heat, -float("inf"))), dim=(2, 3))
counting = int((torch.isfinite(peaks) & (peaks > 0)).sum())
pairs = int(n_vis.sum())
gathers = pairs * n_lm * counting / (N_VIEWS * n_lm)   # (a plane whose peak does not count costs no load)
med = [statistics.median(r[k] for r in rows) for k in range(3)]
low = [min(r[k] for r in rows) for k in range(3)]
say(f"  seen (vertex, view) pairs: {pairs} of {mesh.n_verts * N_VIEWS} ({100 * pairs / (mesh.n_verts * N_VIEWS):.1f} %), "
    f"{counting} of {N_VIEWS * n_lm} planes count: {gathers / 1e6:.1f} M gathers of 4 bytes")
for k, name in enumerate(("peak", "back-projection", "paint")):
    extra = ""
    if k == 0:
        extra = f", {heat.numel() * 4 / (med[k] * 1e-3) / 1e12:.2f} TB/s of heatmaps read"
    if k == 1:
        extra = (f", {gathers / (med[k] * 1e-3) / 1e9:.1f} G gathers/s = {4 * gathers / (med[k] * 1e-3) / 1e12:.3f} TB/s of values used, "
                 f"{64 * gathers / (med[k] * 1e-3) / 1e12:.2f} TB/s if every gather moved a 64-byte line of its own")
    say(f"  {name}: device events median of {RUNS} {med[k]:.3f} ms (min {low[k]:.3f}){extra}")
say(f"  surface heat, the three stages: {sum(med):.3f} ms")
hmed = [statistics.median(r[k] for r in sheet) for k in range(3)]
for k, name in enumerate(("background", "peak", "compose")):
    say(f"  heat sheet {name}, same heatmaps, same run: device events median of {RUNS} {hmed[k]:.3f} ms")
net = events(lambda: p2.heatmaps_device(images), runs=5, warmup=2)
say(f"  the second network pass (heatmaps_device, {N_VIEWS} views): device events median of 5 {net[0]:.3f} ms (min {net[1]:.3f}); "
    f"the back-projection is {100 * med[1] / net[0]:.1f} % of it")
if out is not None:
    out.close()
