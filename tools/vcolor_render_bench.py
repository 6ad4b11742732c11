#!/usr/bin/env python3
"""Time one render of the bench mesh (face_like_mesh(224, 256, seed=0), 96 views) textured, with per-vertex colours and white,
at 0 and 4 samples per pixel: median and minimum of 40 renders by the library's own events, and a digest of the images.

    tools/vcolor_render_bench.py
    MVLM_HIP_LIB=<older build of the library> tools/vcolor_render_bench.py    textured only: a build from before
                                                                             mvlm_mesh_upload_colors has nothing else to time
Two builds that print the same digest render the same bytes (profiles/vcolor_render_time.txt)."""
import ctypes as C
import hashlib
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd import _lib

older = bool(os.environ.get("MVLM_HIP_LIB"))   # a build without the colour entry points: do not ask it for them
if older:
    for k in ("mvlm_obj_has_colors", "mvlm_obj_copy_colors", "mvlm_mesh_upload_colors"):
        _lib.SIGNATURES.pop(k)
from mvlm_amd.utils import HipRenderer3D, Mesh
from mvlm_amd.utils.synthetic import face_like_mesh

base = face_like_mesh(224, 256, seed=0, **({} if older else {"vertex_colors": True}))
forms = {"textured": Mesh(base.verts, base.tris, base.uvs, base.texture)}
if not older:
    forms["coloured"] = Mesh(base.verts, base.tris, colors=base.colors)
    forms["white"] = Mesh(base.verts, base.tris)
for samples in (0, 4):
    for name, mesh in forms.items():
        r = HipRenderer3D(n_views=96, verbose=False, multisamples=samples)
        np.random.seed(0)
        poses = r.generate_3d_transformations()
        out = torch.empty((96, 256, 256, 4), dtype=torch.float32, device="cuda")
        for _ in range(3):
            r.render_device(mesh, poses, out=out)
        r.check()
        lib, h = r.ctx.lib, r.ctx.handle
        lib.mvlm_render_set_profiling(h, 1)
        for _ in range(40):
            r.render_device(mesh, poses, out=out)
        r.check()
        nv, nve, nt, ms = (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_float * 64)()
        k = lib.mvlm_render_get_profile(h, nv, nve, nt, ms, 64)
        lib.mvlm_render_set_profiling(h, 0)
        t = sorted(ms[i] for i in range(k))
        print(f"{'older' if older else 'this '} {name:9s} {samples} samples: median {1e3 * t[k // 2]:7.1f} us  min {1e3 * t[0]:7.1f} us  "
              f"sha256 {hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}", flush=True)
