#!/usr/bin/env python3
"""Stage times of the heat sheet at 96 views x 84 landmarks, scale 1 (MI355X; the figures of DESIGN.md 5.1, "Heat sheet" - they
gate nothing): background, peak and compose from mvlm_heat_sheet_stage_ms, torch.amax over the same tensor as the yardstick of the
peak kernel, and the bytes each kernel has to read over its time.

    tools/heat_sheet_bench.py [--out FILE]     print the table (and write it to FILE: profiles/heat_sheet_time.txt)
"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mvlm_amd.utils.render3d import HipRenderer3D  # noqa: E402

N_VIEWS, N_LM, WARMUP, RUNS = 96, 84, 3, 20
out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


r3 = HipRenderer3D(n_views=N_VIEWS, verbose=False)
ctx = r3.ctx
dev = torch.device("cuda", ctx.device)
gen = torch.Generator(device=dev).manual_seed(1)
images = torch.rand((N_VIEWS, 256, 256, 4), device=dev, generator=gen)
# every value counts and nearly every pixel is drawn: no plane is skipped, the composition's longest path
heat = torch.rand((N_VIEWS, N_LM, 256, 256), device=dev, generator=gen)
heat_bytes = heat.numel() * 4
say(f"heat sheet, MI355X, {N_VIEWS} views x {N_LM} landmarks of uniform noise, scale 1, gap 2: sheet",
    r3.view_sheet_layout(N_VIEWS)[2:], f"pixels; the heatmaps are {heat_bytes / 1e9:.2f} GB")

ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 1))
try:
    rows = []
    for k in range(WARMUP + RUNS):
        r3.render_heat_sheet_device(images, heat)
        ms = r3.heat_sheet_stage_ms()
        if k >= WARMUP:
            rows.append(ms.tolist())
finally:
    ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 0))
med = [statistics.median(r[k] for r in rows) for k in range(3)]
low = [min(r[k] for r in rows) for k in range(3)]
for k, name in enumerate(("background", "peak", "compose")):
    rate = f", {heat_bytes / (med[k] * 1e-3) / 1e12:.2f} TB/s of heatmaps read" if k else ""
    say(f"  {name}: device events median of {RUNS} {med[k]:.3f} ms (min {low[k]:.3f}){rate}")

amax = []
for k in range(WARMUP + RUNS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    peaks = torch.amax(heat, dim=(2, 3))
    e1.record()
    torch.cuda.synchronize()
    if k >= WARMUP:
        amax.append(e0.elapsed_time(e1))
say(f"  torch.amax(heat, dim=(2, 3)) on the same tensor: device events median of {RUNS} {statistics.median(amax):.3f} ms "
    f"(min {min(amax):.3f}), {heat_bytes / (statistics.median(amax) * 1e-3) / 1e12:.2f} TB/s")
if out is not None:
    out.close()
