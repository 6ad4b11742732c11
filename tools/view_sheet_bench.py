#!/usr/bin/env python3
"""Draw time and file time of the view sheet at 96 views, scale 1, under both PNG encoders (MI355X; the figures of DESIGN.md 4.2,
"View sheet" - they gate nothing).

    tools/view_sheet_bench.py [--out FILE]     print the table (and write it to FILE: profiles/view_sheet_time.txt)
"""
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mvlm_amd import pipeline  # noqa: E402
from mvlm_amd.utils.render3d import view_rotations  # noqa: E402
from mvlm_amd.utils.synthetic import write_face_like_obj  # noqa: E402
from mvlm_amd.utils.viewer import write_view_png  # noqa: E402

out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def med(xs):
    return statistics.median(xs)


with tempfile.TemporaryDirectory() as td:
    import os

    os.chdir(td)
    obj = write_face_like_obj(Path(td) / "face.obj", seed=3)
    pipe = pipeline.create_pipeline("dtu3d", n_views=96, weights="synthetic:7", verbose=False)
    r3 = pipe.renderer_3d
    np.random.seed(1)
    mesh = r3.load_mesh(obj)
    poses = r3.generate_3d_transformations()
    images = r3.render_device(mesh, poses)
    maxima = pipe.predictor_2d.predict_device(images).clone()
    np.random.seed(1)
    landmarks, _ = pipe.predict_mesh_device(mesh, poses)
    rot = view_rotations(poses)
    torch.cuda.synchronize()
    say(f"view sheet, MI355X, bench mesh, 96 views x {maxima.shape[0]} landmarks, scale 1, gap 2: sheet",
        r3.view_sheet_layout(96)[2:], "pixels")
    for what, kw in (("views alone", {}), ("markers", dict(maxima=maxima)),
                     ("markers + residuals", dict(maxima=maxima, rot=rot, landmarks=landmarks))):
        for _ in range(5):
            r3.render_view_sheet_device(images, **kw)
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(40):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            sheet = r3.render_view_sheet_device(images, **kw)
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        say(f"  draw ({what}): device events median of 40 {med(ev) * 1e3:.0f} us (min {min(ev) * 1e3:.0f}), host call to synchronise "
            f"{med(wall) * 1e3:.0f} us")
    kw = dict(maxima=maxima, rot=rot, landmarks=landmarks)
    for encoder in ("host", "device"):
        enc, whole = [], []
        for k in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if encoder == "device":
                sheet = r3.render_view_sheet_device(images, **kw)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                p = write_view_png(sheet, Path(td) / f"s_{encoder}.png", encoder="device", renderer=r3)
            else:
                sheet = r3.render_view_sheet(images, **kw)
                t1 = time.perf_counter()
                p = write_view_png(sheet, Path(td) / f"s_{encoder}.png")
            t2 = time.perf_counter()
            if k >= 2:
                enc.append((t2 - t1) * 1e3)
                whole.append((t2 - t0) * 1e3)
        say(f"  file, {encoder} encoder: draw to file on disk median of 5 {med(whole):.1f} ms, of which encode + write {med(enc):.1f} ms, "
            f"{Path(p).stat().st_size} bytes")
    for encoder in ("host", "device"):
        p2 = pipeline.create_pipeline("dtu3d", n_views=96, weights="synthetic:7", verbose=False, visualize_sheet=True,
                                      view_png_encoder=encoder)
        ts, tot = [], []
        for k in range(5):
            np.random.seed(1)
            p2.predict_one_file(obj)
            if k >= 2:
                ts.append(p2.timings["visualize_sheet"] * 1e3)
                tot.append(p2.timings["total"] * 1e3)
        say(f"  Pipeline(visualize_sheet=True, view_png_encoder={encoder!r}): stage 'visualize_sheet' median of 3 {med(ts):.1f} ms of "
            f"{med(tot):.1f} ms per scan")
if out is not None:
    out.close()
