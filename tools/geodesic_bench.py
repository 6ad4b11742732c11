#!/usr/bin/env python
"""Time the surface distances between landmarks (mvlm_landmark_geodesics) on the bench mesh.

    tools/geodesic_bench.py [--out FILE]      the table (profiles/geodesic_time.txt; FILE receives what is printed)

The bench mesh, face_like_mesh(224): 50 176 vertices, 99 458 triangles; 84 landmarks put into triangles drawn with a fixed seed and
lifted a little off the surface.  Per configuration the four stage times (adjacency with the attachment, init, sweeps with the
host's reads of the settled flags, targets: mvlm_geodesic_stage_ms, device events), median and minimum of RUNS calls after a warm-up;
the sweeps per source; triangle updates per second - an update is one (vertex, incident triangle, source) evaluation of the rule,
counted for every sweep a source ran; and the float64 operations those updates are as written in csrc/geodesic_math.h (11 adds and
multiplies, 2 divisions, 1 square root per update; an incidence's frame - 31 adds and multiplies, 1 division, 4 square roots - is
shared by the 4 sources of a thread) over the sweeps' time, beside the vector float64 peak."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np

from mvlm_amd.utils import HipRenderer3D, Mesh
from mvlm_amd.utils.synthetic import face_like_mesh

RUNS = 20
N_LANDMARKS = 84
PEAK_F64_VECTOR = 78.6e12  # half the FP32 vector peak of 157.3 TFLOPS
_out = None


def say(text=""):
    print(text, flush=True)
    if _out is not None:
        _out.write(text + "\n")


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return f"{np.median(ms):8.3f} ms median, {ms.min():8.3f} min"


def landmarks(face, n, seed=0):
    rs = np.random.RandomState(seed)
    ids = rs.randint(0, face.n_tris, n)
    w = rs.uniform(0.2, 1.0, (n, 3))
    w /= w.sum(axis=1, keepdims=True)
    corners = face.verts.astype(np.float64)[face.tris[ids]]
    return (corners * w[:, :, None]).sum(axis=1) + np.array([0.0, 0.0, 0.5])


def measure(r, mesh, pts, name, **kw):
    lib, handle = r.ctx.lib, r.ctx.handle
    res = r.landmark_geodesics(mesh, pts, **kw)  # (warm-up: the scratch is allocated)
    r.ctx.check(lib.mvlm_render_set_profiling(handle, 1))
    try:
        ms = []
        for _ in range(RUNS):
            res = r.landmark_geodesics(mesh, pts, **kw)
            ms.append(r.geodesic_stage_ms().copy())
    finally:
        r.ctx.check(lib.mvlm_render_set_profiling(handle, 0))
    ms = np.array(ms)
    ran = res.sweeps[res.sweeps >= 0].astype(np.int64) + 1  # (the sweep that changed nothing ran too)
    incidences = 3 * mesh.n_tris
    updates = float(ran.sum()) * incidences
    sweep_s = float(np.median(ms[:, 2])) * 1e-3
    flops = updates * 14 + float(ran.max()) * incidences * 36 * ((len(ran) + 3) // 4)
    say(f"{name}: {len(ran)} sources, {mesh.n_verts} vertices, {mesh.n_tris} triangles")
    for k, stage in enumerate(("adjacency", "init", "sweeps", "targets")):
        say(f"    {stage:10s} {stats(ms[:, k])}")
    say(f"    all four   {stats(ms.sum(axis=1))}")
    say(f"    sweeps per source: least {ran.min() - 1}, median {int(np.median(ran)) - 1}, most {ran.max() - 1}")
    say(f"    {updates / sweep_s / 1e9:.2f} G triangle updates per second ({updates / 1e9:.3f} G updates in the sweeps' time)")
    say(f"    {flops / sweep_s / 1e12:.3f} T float64 operations per second as written, {100 * flops / sweep_s / PEAK_F64_VECTOR:.2f} % of the "
        f"{PEAK_F64_VECTOR / 1e12:.1f} T vector peak")
    far = res.euclidean > 60
    geo, asym = res.geodesic, res.asymmetry
    say(f"    pairs more than 60 units apart: surface / straight {np.nanmedian(geo[far] / res.euclidean[far]):.4f} median, asymmetry "
        f"{np.nanmedian(asym[far] / geo[far]):.5f} median, {np.nanmax(asym[far] / geo[far]):.5f} worst")
    return ms


def main():
    global _out
    if "--out" in sys.argv:
        _out = open(sys.argv[sys.argv.index("--out") + 1], "w")
    face = face_like_mesh(224, 16, seed=0)
    mesh = Mesh(face.verts, face.tris)
    pts = landmarks(face, N_LANDMARKS)
    r = HipRenderer3D(n_views=1, verbose=False)
    say(f"mvlm_landmark_geodesics, MI355X, median and minimum of {RUNS} calls (device events)")
    measure(r, mesh, pts, "bench mesh, every pair, init_rings 2")
    measure(r, mesh, pts, "bench mesh, 3 pairs (6 sources)", pairs=[(0, 16), (8, 27), (40, 83)])
    measure(r, mesh, pts[:4], "bench mesh, 4 landmarks (one thread's sources)")
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()
