"""ctypes loader of tests/native/landmark_view.c, the CPU model of the landmark view (test infrastructure), and the small
scenes the landmark-view tests share.

`load(directory)` compiles the model with the flags oracle/Makefile uses (gcc -O2 -ffp-contract=off) into the given directory -
a pytest temporary directory, once per session - and `render` takes mvlm_render_landmark_view's arguments (poses in degrees
instead of matrices) and returns the image, the per-landmark pixel counts and the per-pixel winner."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "native" / "landmark_view.c"
NETWORK_FRAME = (0.0, 0.0, 150.0)
_lib = None


def load(directory: Path):
    global _lib
    if _lib is None:
        so = Path(directory) / "liblandmark_view.so"
        r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", str(SRC), "-o", str(so), "-lm"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building the landmark-view model failed:\n{r.stderr}")
        _lib = C.CDLL(str(so))
        _lib.landmark_view.restype = C.c_int
    return _lib


def rotations(poses) -> np.ndarray:
    from oracle.estimator import view_rotation

    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    return np.ascontiguousarray(np.stack([view_rotation(*p).ravel() for p in poses]), np.float64)


def frames_for(n: int, frame) -> np.ndarray:
    f = np.asarray(frame, np.float32)
    return np.ascontiguousarray(np.broadcast_to(f, (n, 3)) if f.ndim == 1 else f.reshape(n, 3), np.float32)


def render(verts, tris, uvs, texture, poses, size, frame=NETWORK_FRAME, landmarks=None, radius=0.0, lm_rgb=None,
           colors=None, shading: str = "texture", subpixel_bits: int = 8):
    """-> (image u8 [N,S,S,4], counts i32 [N,NL], winner i32 [N,S,S]); image rows (row 0 = top).  winner: the triangle's id,
    -1 = background, -2 - l = landmark l's sphere."""
    assert _lib is not None, "view_model.load(directory) first"
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    rot = rotations(poses)
    n = rot.shape[0]
    fr = frames_for(n, frame)
    use_tex = uvs is not None and texture is not None
    uv = np.ascontiguousarray(uvs, np.float32) if uvs is not None else None
    tex = np.ascontiguousarray(texture, np.uint8) if use_tex else None
    col = np.ascontiguousarray(colors, np.uint8) if colors is not None else None
    lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3) if landmarks is not None else np.zeros((0, 3))
    nl = lm.shape[0]
    rgb = np.ascontiguousarray(lm_rgb, np.uint8).reshape(nl, 3) if lm_rgb is not None else None
    out = np.empty((n, size, size, 4), np.uint8)
    counts = np.zeros((n, nl), np.int32)
    winner = np.empty((n, size, size), np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None and a.size else None
    rc = _lib.landmark_view(p(verts, C.c_float), p(uv, C.c_float), C.c_int(verts.shape[0]), p(tris, C.c_int32),
                            C.c_int(tris.shape[0]), p(tex, C.c_uint8), C.c_int(tex.shape[0] if use_tex else 0),
                            C.c_int(tex.shape[1] if use_tex else 0), p(col, C.c_uint8), p(rot, C.c_double), C.c_int(n),
                            C.c_int(size), p(fr, C.c_float), p(lm, C.c_double), C.c_int(nl), C.c_float(radius),
                            p(rgb, C.c_uint8), C.c_int(1 if shading == "geometry" else 0), C.c_int(subpixel_bits),
                            p(out, C.c_uint8), p(counts, C.c_int32), p(winner, C.c_int32))
    if rc != 0:
        raise ValueError(f"landmark_view failed ({rc})")
    return out, counts, winner


# ---- shared scenes ---------------------------------------------------------------------------------------------------------
def quad(z: float = 0.0, half: float = 100.0):
    """A screen-parallel square [-half, half]^2 at depth z: two counter-clockwise triangles that share no vertex, so that each
    can carry a colour of its own (QUAD_COLOURS) and the mesh's winner shows in the image."""
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, -half, z], [half, half, z], [-half, half, z]], np.float32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.int32)


QUAD_COLOURS = np.array([[200, 40, 40]] * 3 + [[40, 160, 60]] * 3, np.uint8)  # per vertex: triangle 0 red, triangle 1 green


def far_triangle():
    """A mesh that covers no pixel of any window used here (the entry refuses an empty mesh): the 'empty mesh' scenes."""
    v = np.array([[9000, 9000, 0], [9001, 9000, 0], [9000, 9001, 0]], np.float32)
    return v, np.array([[0, 1, 2]], np.int32)


def surface_landmarks(verts, n: int, seed: int = 0) -> np.ndarray:
    """n distinct vertices of the mesh, as float64 landmarks on its surface."""
    rs = np.random.RandomState(seed)
    idx = rs.permutation(len(verts))[:n]
    return np.asarray(verts, np.float64)[idx]


def fit_frame(verts, landmarks, pose) -> tuple:
    """HipRenderer3D.render_landmark_view's frame="fit", restated: the view-space centre of the 3-D bounding box of vertices and
    landmarks, half = its half diagonal / 1.4."""
    pts = np.asarray(verts, np.float64).reshape(-1, 3)
    if landmarks is not None and len(landmarks):
        pts = np.concatenate([pts, np.asarray(landmarks, np.float64).reshape(-1, 3)])
    lo, hi = pts.min(0), pts.max(0)
    centre = rotations([pose])[0].reshape(3, 3) @ ((lo + hi) / 2)
    return float(centre[0]), float(centre[1]), float(np.linalg.norm(hi - lo) / 2 / 1.4)
