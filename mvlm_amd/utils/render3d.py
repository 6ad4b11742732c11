"""Multi-view renderer slot: all camera poses of a mesh rasterised on the MI355X.

Drop-in for the reference's ``ObjVTKRenderer3D`` (src/mvlm/utils/render3d.py):
same constructor arguments, same pose generation (global numpy RNG, same draw
order), same ``multiview_render(path) -> (image_stack, transform_stack, mesh)``
contract, with the per-pose VTK offscreen loop (:139-170) replaced by one
batched HIP launch set (mvlm_amd/csrc/raster.hip) through ``mvlm_render``.
"""
from __future__ import annotations

import ctypes as C
import operator
import time
from pathlib import Path

import numpy as np

from .. import _lib
from .mesh_io import Mesh, load_obj

__all__ = ["HipRenderer3D", "view_rotations", "upload_mesh"]


def _view_rotation_scalar(rx, ry, rz) -> np.ndarray:
    """One view, evaluated exactly like the reference's estimator (estimator3d.py:8-15, :57)."""
    rx, ry, rz = (np.deg2rad(v) for v in (rx, ry, rz))
    mx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    my = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    mz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    return (my @ mx) @ mz


def view_rotations(transform_stack: np.ndarray) -> np.ndarray:
    """[N,>=3] (rx, ry, rz) degrees -> [N,9] float64 row-major M = Ry @ Rx @ Rz.

    The order is VTK's RotateY / RotateX / RotateZ pre-multiplication
    (render3d.py:140-144), which the estimator inverts (estimator3d.py:57).
    Evaluated for all views at once; the first and last view are re-evaluated with the
    reference's scalar formulation and, should numpy's array kernels ever round differently
    from its scalar ones on this machine, the whole table falls back to the scalar path.
    """
    t = np.asarray(transform_stack)
    n = t.shape[0]
    if n == 0:
        return np.zeros((0, 9))
    # the fixed 8-view table (render3d.py:94-111) is the same for every scan, and a caller that repeats a pose table gets the
    # same answer: the last few tables are kept (read-only), keyed by the angles' bytes
    key = (t.dtype.str, n, t[:, :3].tobytes())
    hit = _ROTATION_MEMO.get(key)
    if hit is not None:
        return hit
    out = _view_rotations_uncached(t, n)
    out.setflags(write=False)
    if len(_ROTATION_MEMO) >= 8:
        _ROTATION_MEMO.pop(next(iter(_ROTATION_MEMO)))
    _ROTATION_MEMO[key] = out
    return out


_ROTATION_MEMO: dict = {}


def _view_rotations_uncached(t: np.ndarray, n: int) -> np.ndarray:
    r = np.deg2rad(t[:, :3].astype(np.float64))
    c, s = np.cos(r), np.sin(r)
    mx, my, mz = np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    mx[:, 0, 0] = 1; mx[:, 1, 1] = c[:, 0]; mx[:, 1, 2] = -s[:, 0]; mx[:, 2, 1] = s[:, 0]; mx[:, 2, 2] = c[:, 0]
    my[:, 0, 0] = c[:, 1]; my[:, 0, 2] = s[:, 1]; my[:, 1, 1] = 1; my[:, 2, 0] = -s[:, 1]; my[:, 2, 2] = c[:, 1]
    mz[:, 0, 0] = c[:, 2]; mz[:, 0, 1] = -s[:, 2]; mz[:, 1, 0] = s[:, 2]; mz[:, 1, 1] = c[:, 2]; mz[:, 2, 2] = 1
    out = np.matmul(np.matmul(my, mx), mz).reshape(n, 9)
    for i in {0, n - 1}:
        if not np.array_equal(out[i], _view_rotation_scalar(*t[i, :3]).ravel()):
            return np.stack([_view_rotation_scalar(*t[k, :3]).ravel() for k in range(n)])
    return out


POINT_NORMALS = ("file", "estimate")
POINT_SURFACES = ("splats", "mesh")


def check_point_surface(value) -> str:
    """``point_surface`` of a renderer or a pipeline: "splats" or "mesh"."""
    if value not in POINT_SURFACES:
        raise ValueError(f"point_surface must be 'splats' or 'mesh', not {value!r}")
    return value


def upload_mesh(ctx: "_lib.Context", mesh: Mesh, normals: str | None = None) -> C.c_void_p:
    """Copy a host mesh to the context's device once; cached on the Mesh object.  ``normals``: what a renderer that shades
    geometry asks for a point cloud's device copy - "file": ``mesh.normals`` follow the points where the mesh has them;
    "estimate": likewise, and a cloud without gets them estimated on the device (mvlm_mesh_estimate_normals, on the context's
    launch stream); None (every other caller): normals are left alone.  Done once per device copy."""
    key = id(ctx)
    ent = mesh._device.get(key)
    if ent is not None:
        if mesh.n_tris == 0 and ent[3] != mesh.point_radius:  # the cloud's radius was changed after the upload
            _set_point_radius(ctx, ent[0], mesh)
            ent = mesh._device[key] = ent[:3] + (mesh.point_radius,) + ent[4:]
        if normals is not None and mesh.n_tris == 0 and ent[4] is None:
            mesh._device[key] = ent[:4] + (_send_point_normals(ctx, ent[0], mesh, normals),)
        return ent[0]
    cloud = mesh.n_tris == 0  # a point cloud: the points (and their colours) alone; uvs and texture are ignored
    verts = np.ascontiguousarray(mesh.verts, dtype=np.float32)
    tris = np.ascontiguousarray(mesh.tris, dtype=np.int32)
    uvs = None if mesh.uvs is None or cloud else np.ascontiguousarray(mesh.uvs, dtype=np.float32)
    handle = C.c_void_p()
    uploaded = False
    ahead = None if cloud else getattr(mesh, "_texture_ahead", None)
    if cloud:
        ctx.check(ctx.lib.mvlm_mesh_upload(ctx.handle, _lib.as_ptr(verts, C.c_float), None, mesh.n_verts, None, 0, None, 0, 0,
                                           C.byref(handle)), ValueError)
        uploaded = True
    elif ahead is not None and ahead.ctx is ctx and ahead.handle:
        # the texture was decoded on the device while the geometry was parsed (HipRenderer3D.load_mesh): its buffer
        # becomes the mesh's
        consumed = C.c_int(0)
        ctx.check(ctx.lib.mvlm_mesh_upload_texture(
            ctx.handle, _lib.as_ptr(verts, C.c_float), None if uvs is None else _lib.as_ptr(uvs, C.c_float), mesh.n_verts,
            _lib.as_ptr(tris, C.c_int32), mesh.n_tris, ahead.handle, C.byref(consumed), C.byref(handle)), ValueError)
        if consumed.value:
            ahead.handle = None
        mesh._texture_ahead = None  # (an unused handle is freed with its owner)
        uploaded = True
    elif uvs is not None and mesh.texture_jpeg is not None and getattr(mesh, "_texture", None) is None:
        # the texture is still the JPEG file's bytes: entropy decoding, inverse DCT, upsampling and colour conversion on
        # the device (csrc/jpeg.hip).  2 = a kind of JPEG that decoder does not take: libjpeg on the host below
        raw = np.frombuffer(mesh.texture_jpeg, dtype=np.uint8)
        rc = ctx.lib.mvlm_mesh_upload_jpeg(
            ctx.handle, _lib.as_ptr(verts, C.c_float), _lib.as_ptr(uvs, C.c_float), mesh.n_verts, _lib.as_ptr(tris, C.c_int32),
            mesh.n_tris, _lib.as_ptr(raw, C.c_uint8), raw.size, C.byref(handle))
        if rc == 0:
            uploaded = True
        elif rc != 2:
            ctx.check(rc, ValueError)
    if not uploaded:
        tex = None if mesh.texture is None else np.ascontiguousarray(mesh.texture, dtype=np.uint8)
        ctx.check(ctx.lib.mvlm_mesh_upload(
            ctx.handle, _lib.as_ptr(verts, C.c_float), None if uvs is None else _lib.as_ptr(uvs, C.c_float), mesh.n_verts,
            _lib.as_ptr(tris, C.c_int32), mesh.n_tris, None if tex is None else _lib.as_ptr(tex, C.c_uint8),
            0 if tex is None else tex.shape[0], 0 if tex is None else tex.shape[1], C.byref(handle)), ValueError)

    class _Owner:  # frees the device copy with the Mesh
        def __init__(self, ctx, h):
            self.ctx, self.h = ctx, h

        def __del__(self):
            try:
                self.ctx.lib.mvlm_mesh_free(self.ctx.handle, self.h)
            except Exception:  # noqa: BLE001
                pass

    owner = _Owner(ctx, handle)
    # Per-point colours follow when the render can use them: the mesh has no usable texture (with one it renders with the
    # texture alone) and the consumer reads an RGB plane (_colors_wanted: HipRenderer3D.load_mesh(load_texture=False)).
    textured = uvs is not None and (mesh.texture_jpeg is not None or getattr(mesh, "_texture", None) is not None
                                    or ahead is not None)
    send_colors = mesh.colors is not None and not textured and getattr(mesh, "_colors_wanted", True)
    if send_colors:
        colors = np.ascontiguousarray(mesh.colors, dtype=np.uint8)
        if colors.shape != (mesh.n_verts, 3):
            raise ValueError(f"mesh colours must be uint8 [V,3] with V = {mesh.n_verts}, not {colors.shape}")
        ctx.check(ctx.lib.mvlm_mesh_upload_colors(ctx.handle, handle, _lib.as_ptr(colors, C.c_uint8), mesh.n_verts), ValueError)
    if cloud and mesh.point_radius is not None:
        _set_point_radius(ctx, handle, mesh)
    # (the third entry: were colours uploaded with it?  the fourth: the point radius the device copy has, None = automatic; the
    # fifth: the normals the device copy has - None, "file" or "estimated")
    mesh._device[key] = (handle, owner, send_colors, mesh.point_radius if cloud else None, None)
    if cloud and normals is not None:
        mesh._device[key] = mesh._device[key][:4] + (_send_point_normals(ctx, handle, mesh, normals),)
    return handle


def _send_point_normals(ctx: "_lib.Context", handle, mesh: Mesh, mode: str):
    """Normals for a cloud's device copy: the mesh's own where it has them, else - under "estimate" - the device's estimate.
    -> what the copy has now: "file", "estimated" or None."""
    if mode not in POINT_NORMALS:
        raise ValueError(f"point_normals must be 'file' or 'estimate', not {mode!r}")
    if mesh.normals is not None:
        nrm = np.ascontiguousarray(mesh.normals, dtype=np.float32)
        if nrm.shape != (mesh.n_verts, 3):
            raise ValueError(f"mesh normals must be float32 [V,3] with V = {mesh.n_verts}, not {nrm.shape}")
        ctx.check(ctx.lib.mvlm_mesh_upload_normals(ctx.handle, handle, _lib.as_ptr(nrm, C.c_float), mesh.n_verts), ValueError)
        return "file"
    if mode == "estimate":
        ctx.check(ctx.lib.mvlm_mesh_estimate_normals(ctx.handle, handle, None), ValueError)
        return "estimated"
    return None


def _set_point_radius(ctx: "_lib.Context", handle, mesh: Mesh) -> None:
    """Give a cloud's device copy the radius its Mesh names (None: the automatic one of its points)."""
    r = mesh.point_radius
    if r is None:
        verts = np.ascontiguousarray(mesh.verts, dtype=np.float32)
        auto = C.c_double()
        ctx.lib.mvlm_points_auto_radius(_lib.as_ptr(verts, C.c_float), mesh.n_verts, C.byref(auto))
        r = auto.value
    ctx.check(ctx.lib.mvlm_mesh_set_point_radius(ctx.handle, handle, C.c_double(float(r))), ValueError)


class _DevicePointer:
    """A borrowed device address with the one method the C-ABI wrappers ask of a tensor."""

    def __init__(self, ptr: int):
        self._ptr = int(ptr)

    def data_ptr(self) -> int:
        return self._ptr


class _TextureAhead:
    """A texture decoded on the device ahead of its mesh (mvlm_texture_from_jpeg); gives the buffer back unless a mesh
    upload has taken it over."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def __del__(self):
        try:
            if self.handle:
                self.ctx.lib.mvlm_texture_free(self.ctx.handle, self.handle)
                self.handle = None
        except Exception:  # noqa: BLE001
            pass


def decode_texture_ahead(ctx: "_lib.Context", jpeg_bytes: bytes):
    """JPEG bytes -> _TextureAhead on the context's device, or None when the device decoder does not take the file."""
    raw = np.frombuffer(jpeg_bytes, dtype=np.uint8)
    handle = C.c_void_p()
    rc = ctx.lib.mvlm_texture_from_jpeg(ctx.handle, _lib.as_ptr(raw, C.c_uint8), raw.size, C.byref(handle))
    if rc == 0:
        return _TextureAhead(ctx, handle)
    if rc != 2:
        ctx.check(rc, ValueError)
    return None


class HipRenderer3D:
    def __init__(self, n_views: int = 8, image_size: tuple = (256, 256), offscreen: bool = True,
                 min_x_angle: int = -40, max_x_angle: int = 40, min_y_angle: int = -80, max_y_angle: int = 80,
                 min_z_angle: int = -20, max_z_angle: int = 20, min_scale: float = 1.4, max_scale: float = 1.9,
                 min_tx: int = -20, max_tx: int = 20, min_ty: int = -20, max_ty: int = 20, device: int = 0,
                 verbose: bool = True, shading: str = "texture", subpixel_bits: int = 8, multisamples: int = 0,
                 point_radius: float | None = None, point_normals: str = "file", point_surface: str = "splats"):
        if tuple(image_size) != (256, 256):
            raise ValueError("the HIP renderer is built for 256x256 views (general_pipeline.py:57)")
        self.n_views = n_views
        self.image_size = tuple(image_size)
        self.offscreen = offscreen  # accepted for signature compatibility; there is no window
        self.min_x_angle, self.max_x_angle = min_x_angle, max_x_angle
        self.min_y_angle, self.max_y_angle = min_y_angle, max_y_angle
        self.min_z_angle, self.max_z_angle = min_z_angle, max_z_angle
        self.min_scale, self.max_scale = min_scale, max_scale
        self.min_tx, self.max_tx = min_tx, max_tx
        self.min_ty, self.max_ty = min_ty, max_ty
        self.slack = 5
        self.side_length = max([150 - (-150), 150 - (-150)]) * 1.0 / 2  # render3d.py:50
        self.verbose = verbose
        if shading not in ("texture", "geometry"):
            raise ValueError("shading must be 'texture' (the reference's unlit render) or 'geometry'")
        # "geometry": build-defined shaded plane for models trained on geometry renderings
        self.shading = shading
        # vertex snap of the rasteriser, 2^-bits pixel: GL_SUBPIXEL_BITS of the OpenGL whose images are to be matched (the
        # reference's pixels depend on it; 8 = GPUs, 4 = the software GL behind tests/golden/gl_raster.npz)
        if subpixel_bits not in (4, 5, 6, 7, 8):
            raise ValueError("subpixel_bits must be 4..8")
        self.subpixel_bits = int(subpixel_bits)
        # samples per pixel (vtkRenderWindow.MultiSamples, which the reference leaves to VTK's default): 0 = one at the pixel
        # centre (the default contract), 4 = four, resolved like the OpenGL behind tests/golden/gl_raster_msaa4.npz
        self.multisamples = multisamples
        # splat radius (model units) of the point clouds - scans without faces - that load_mesh reads: None = automatic, from
        # the spacing of the points (Mesh.point_radius, which a Mesh handed to render_device carries itself)
        self.point_radius = None if point_radius is None else float(point_radius)
        # where a point cloud's normals come from when this renderer shades geometry: "file" - the cloud's own (Mesh.normals: a
        # .ply's nx ny nz, a .vtk's NORMALS), a cloud without is refused; "estimate" - a cloud without gets them estimated on the
        # device, once per device copy (a file's normals still win).  DESIGN.md 5.1, "Point clouds".
        if point_normals not in POINT_NORMALS:
            raise ValueError(f"point_normals must be 'file' or 'estimate', not {point_normals!r}")
        self.point_normals = point_normals
        # what the file entries (multiview_render, multiview_render_device) make of a point cloud: "splats" - the cloud as it is;
        # "mesh" - its triangulation (triangulate_point_cloud), an ordinary mesh.  render_device draws the Mesh it is handed.
        self.point_surface = check_point_surface(point_surface)
        # "pre-align" block of a Deep-MVLM config (utils/prealign.py; utils3d.py:465-503): applied to every mesh this
        # renderer loads, the mesh handle it returns carries the matrix (Mesh.to_original)
        self.pre_align: dict | None = None
        # where load_mesh's JPEG texture is decoded: "device" (the upload decodes the file's bytes on the GPU, csrc/jpeg.hip)
        # or "host" (libjpeg through Pillow at load time); the pixels are the same bytes either way
        self.texture_decode = "device"
        self.ctx = _lib.get_context(device)

    @property
    def multisamples(self) -> int:
        return self._multisamples

    @multisamples.setter
    def multisamples(self, samples: int) -> None:
        if isinstance(samples, bool) or samples not in (0, 4):
            raise ValueError(f"multisamples must be 0 (one sample at the pixel centre) or 4, not {samples!r}")
        self._multisamples = int(samples)

    # ---- pose table (render3d.py:79-112) ----------------------------------------------
    def random_transform(self, size=1):
        rx = np.random.randint(self.min_x_angle, self.max_x_angle, size=size)
        ry = np.random.randint(self.min_y_angle, self.max_y_angle, size=size)
        rz = np.random.randint(self.min_z_angle, self.max_z_angle, size=size)
        # drawn but unused, kept so the global RNG advances exactly as in the reference
        scale = np.random.uniform(self.min_scale, self.max_scale, size=size)
        tx = np.random.randint(self.min_tx, self.max_tx, size=size)
        ty = np.random.randint(self.min_ty, self.max_ty, size=size)
        return np.stack((rx, ry, rz, scale, tx, ty), axis=1)

    def generate_3d_transformations(self):
        if self.n_views == 8:
            table = [[rx, ry, 0, 0, 0, 0] for rx in (30, -30) for ry in (15, -15, 45, -45)]
            return np.array(table, dtype=np.float32)
        return self.random_transform(size=self.n_views)

    # ---- rendering --------------------------------------------------------------------
    def _push_render_mode(self) -> None:
        """Shading, sub-pixel bits and samples of THIS renderer into the context, when they are not the ones it holds (renderers
        of one GPU share the context)."""
        mode = (1 if self.shading == "geometry" else 0, self.subpixel_bits, self.multisamples)
        if getattr(self.ctx, "_render_mode", None) != mode:
            self.ctx.check(self.ctx.lib.mvlm_set_render_shading(self.ctx.handle, mode[0]))
            self.ctx.check(self.ctx.lib.mvlm_set_render_subpixel_bits(self.ctx.handle, mode[1]))
            self.ctx.check(self.ctx.lib.mvlm_set_render_multisamples(self.ctx.handle, mode[2]))
            self.ctx._render_mode = mode

    @staticmethod
    def _view_colours_and_size(colors, nl: int, size) -> tuple:
        """The landmark and ray views' checks of ``colors`` (None or uint8 [NL,3]) and ``size`` -> (colour table or None, size)."""
        rgb = None
        if colors is not None:
            rgb = np.ascontiguousarray(colors, dtype=np.uint8)
            if rgb.shape != (nl, 3):
                raise ValueError(f"colors must be uint8 [{nl},3], not {rgb.shape}")
        size = int(size)
        if size < 64 or size > 2048 or size % 16:
            raise ValueError(f"size must be a multiple of 16 in 64..2048, not {size}")
        return rgb, size

    def render_device(self, mesh: Mesh, transform_stack: np.ndarray, rot: np.ndarray | None = None, out=None):
        """Poses -> torch.float32 [N,256,256,4] on the device (RGB + depth, /255, flipped).
        Only enqueues work; ``check()`` reports a deferred failure after the caller's sync.
        ``out``: an existing stack of that shape to render into (the pipeline reuses one buffer per view count)."""
        import torch

        n = int(transform_stack.shape[0])
        dev = torch.device("cuda", self.ctx.device)
        if out is None:
            out = torch.empty((n, 256, 256, 4), dtype=torch.float32, device=dev)
        elif tuple(out.shape) != (n, 256, 256, 4) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("render_device: out must be a contiguous float32 [N,256,256,4] tensor on the renderer's GPU")
        rot = np.ascontiguousarray(view_rotations(transform_stack) if rot is None else rot, dtype=np.float64)
        self.ctx.bind_current_stream(torch, dev)  # (before the upload: a cloud's normals may be estimated on this stream)
        handle = upload_mesh(self.ctx, mesh, normals=self.point_normals if self.shading == "geometry" else None)
        self._push_render_mode()
        # (a cloud's refusals - geometry shading without normals, multisampling - are argument errors, said before anything is launched)
        self.ctx.check(self.ctx.lib.mvlm_render(self.ctx.handle, handle, _lib.as_ptr(rot, C.c_double), n,
                                                C.c_void_p(out.data_ptr())), ValueError if mesh.n_tris == 0 else _lib.MvlmHipError)
        return out

    # ---- landmark view (utils/viewer.py's offscreen window) ----------------------------------
    def landmark_view_arguments(self, mesh: Mesh, landmarks, poses=None, frame="fit", radius=None):
        """The host half of ``render_landmark_view``: (poses [n,3], frames f32 [n,3], landmarks f64 [NL,3], radius), computed from
        the arrays the ``Mesh`` object holds.

        ``frame="fit"`` is the orthographic reading of viewer.py:74-78 (``ResetCamera`` then ``Zoom(1.4)``): the window's centre is
        the view-space centre of the 3-D bounding box of the mesh's vertices and the landmarks, ``half`` that box's half diagonal
        divided by 1.4.  ``frame="network"`` is (0, 0, 150), the window the network saw; a tuple ``(cx, cy, half)`` (or one row per
        pose) is taken as given.  ``radius=None`` is 0.008 x the diagonal of the landmarks' bounding box (viewer.py:119-128); with
        ONE landmark that diagonal is 0 and the radius falls back to 0.008 x the mesh's diagonal; with none nothing is drawn."""
        poses = np.zeros((1, 3)) if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        n = poses.shape[0]
        lm = np.zeros((0, 3)) if landmarks is None else np.ascontiguousarray(landmarks, dtype=np.float64).reshape(-1, 3)
        verts = np.asarray(mesh.verts, dtype=np.float64).reshape(-1, 3)
        v_lo, v_hi = verts.min(axis=0), verts.max(axis=0)
        if isinstance(frame, str):
            if frame == "network":
                frames = np.tile(np.array([0.0, 0.0, self.side_length], np.float32), (n, 1))
            elif frame == "fit":
                lo = np.minimum(v_lo, lm.min(axis=0)) if len(lm) else v_lo
                hi = np.maximum(v_hi, lm.max(axis=0)) if len(lm) else v_hi
                centre = view_rotations(poses).reshape(n, 3, 3) @ ((lo + hi) / 2)
                half = float(np.linalg.norm(hi - lo)) / 2 / 1.4
                frames = np.column_stack([centre[:, 0], centre[:, 1], np.full(n, half)]).astype(np.float32)
            else:
                raise ValueError('frame must be "fit", "network" or (cx, cy, half)')
        else:
            f = np.asarray(frame, dtype=np.float32)
            frames = np.tile(f, (n, 1)) if f.shape == (3,) else f.reshape(n, 3)
        if radius is None:
            if len(lm) == 0:
                radius = 0.0
            else:
                diag = float(np.linalg.norm(lm.max(axis=0) - lm.min(axis=0)))
                radius = 0.008 * (diag if diag > 0.0 else float(np.linalg.norm(v_hi - v_lo)))
        return poses, np.ascontiguousarray(frames, dtype=np.float32), lm, float(radius)

    def render_landmark_view_device(self, mesh: Mesh, landmarks, poses=None, size: int = 1024, frame="fit", radius=None,
                                    colors=None, return_pixels: bool = False, vertex_colors=None):
        """``render_landmark_view`` with the results left on the device: uint8 [n,S,S,4] RGBA (and int32 [n,NL] with
        ``return_pixels``).  Only enqueues work; ``check()`` reports a deferred failure."""
        import torch

        poses, frames, lm, radius = self.landmark_view_arguments(mesh, landmarks, poses, frame, radius)
        n, nl = poses.shape[0], lm.shape[0]
        rgb, size = self._view_colours_and_size(colors, nl, size)
        dev = torch.device("cuda", self.ctx.device)
        if vertex_colors is not None:
            vertex_colors = self._vertex_colours(vertex_colors, mesh, dev)
        out = torch.empty((n, size, size, 4), dtype=torch.uint8, device=dev)
        pixels = torch.empty((n, nl), dtype=torch.int32, device=dev) if return_pixels else None
        rot = np.ascontiguousarray(view_rotations(poses), dtype=np.float64)
        handle = upload_mesh(self.ctx, mesh)
        self.ctx.bind_current_stream(torch, dev)
        self._push_render_mode()  # (the view reads the shading and the sub-pixel bits)
        args = (self.ctx.handle, handle, _lib.as_ptr(rot, C.c_double), n, size, _lib.as_ptr(frames, C.c_float),
                _lib.as_ptr(lm, C.c_double) if nl else None, nl, C.c_float(radius), None if rgb is None or nl == 0 else _lib.as_ptr(rgb, C.c_uint8),
                C.c_void_p(out.data_ptr()), C.c_void_p(pixels.data_ptr()) if pixels is not None and nl else None)
        if vertex_colors is None:
            self.ctx.check(self.ctx.lib.mvlm_render_landmark_view(*args), ValueError)
        else:
            self.ctx.check(self.ctx.lib.mvlm_render_landmark_view_colored(*args, C.c_void_p(vertex_colors.data_ptr())), ValueError)
            self._view_keepalive = vertex_colors  # (read by the enqueued kernels)
        return (out, pixels) if return_pixels else out

    @staticmethod
    def _vertex_colours(vertex_colors, mesh: Mesh, dev):
        """``vertex_colors`` of the landmark view on the renderer's device: uint8 [V,4] (r g b and a byte that is not read, the layout
        ``surface_heat`` leaves) or [V,3]; a numpy array is uploaded."""
        import torch

        if not hasattr(vertex_colors, "data_ptr"):
            try:
                vertex_colors = torch.from_numpy(np.ascontiguousarray(vertex_colors, dtype=np.uint8))
            except (TypeError, ValueError) as e:
                raise ValueError(f"landmark view: vertex_colors is not a numeric array ({e})") from None
        t = vertex_colors
        if t.dtype != torch.uint8 or t.dim() != 2 or int(t.shape[0]) != mesh.n_verts or int(t.shape[1]) not in (3, 4):
            raise ValueError(f"landmark view: vertex_colors must be uint8 [{mesh.n_verts},4] (or [{mesh.n_verts},3]), not "
                             f"{t.dtype} {tuple(t.shape)}")
        if t.is_cuda and t.device != dev:
            raise ValueError(f"landmark view: vertex_colors live on {t.device}, the renderer on {dev}")
        t = t.to(dev)
        if int(t.shape[1]) == 3:
            t = torch.cat([t, torch.full((mesh.n_verts, 1), 255, dtype=torch.uint8, device=dev)], dim=1)
        return t.contiguous()

    def render_landmark_view(self, mesh: Mesh, landmarks, poses=None, size: int = 1024, frame="fit", radius=None, colors=None,
                             return_pixels: bool = False, vertex_colors=None):
        """The mesh with a shaded sphere at every landmark, as the reference's offscreen viewer draws it (utils/viewer.py with
        ``save=True``): uint8 [n,S,S,3], and with ``return_pixels`` also int32 [n,NL], the pixels each landmark's sphere won in
        each view (0: hidden there).  ``poses`` [n,3] degrees (rx, ry, rz), default one front view (viewer.py:45-55);
        ``landmarks`` [NL,3] in the mesh's coordinates; ``colors`` uint8 [NL,3], default blue; ``frame`` / ``radius``: see
        ``landmark_view_arguments``.  One sample per pixel, whatever ``multisamples`` is ("Landmark view").
        ``vertex_colors`` uint8 [V,4] or [V,3] (a device tensor, e.g. ``surface_heat(...)["colors"]``, or a numpy array): the mesh is
        drawn with these colours instead of its own colours or texture, unlit - byte for byte the view of a ``Mesh`` of the same
        vertices and triangles with these colours and no texture."""
        res = self.render_landmark_view_device(mesh, landmarks, poses, size, frame, radius, colors, return_pixels, vertex_colors)
        out, pixels = res if return_pixels else (res, None)
        image = out.cpu().numpy()[..., :3].copy()
        counts = pixels.cpu().numpy() if pixels is not None else None
        self.check()
        return (image, counts) if return_pixels else image

    # ---- ray view (visualization/ray_visualizer.py's offscreen window) -------------------------
    @staticmethod
    def _ray_array(x, what):
        """starts / ends as given: a device tensor stays on the device (float64, contiguous, [n,3]); anything else becomes a numpy
        float64 [n,3]."""
        if hasattr(x, "data_ptr"):
            import torch

            if x.shape[-1] != 3:
                raise ValueError(f"{what} must have shape [..., 3], not {tuple(x.shape)}")
            return x.to(torch.float64).reshape(-1, 3).contiguous()
        a = np.asarray(x, dtype=np.float64)
        if a.ndim == 0 or a.shape[-1] != 3:
            raise ValueError(f"{what} must have shape [..., 3], not {a.shape}")
        return np.ascontiguousarray(a.reshape(-1, 3))

    @classmethod
    def ray_view_arguments(cls, starts, ends, ray_radius=0.5, ray_colors=None):
        """The host checks of ``render_ray_view`` that need no device: (starts [n,3], ends [n,3], ray_radius, ray_colors u8 [n,3] or
        None).  ``starts`` / ``ends`` [..., 3], numpy or device tensors, are flattened to [n,3] float64."""
        a, b = cls._ray_array(starts, "starts"), cls._ray_array(ends, "ends")
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"starts and ends must hold the same rays, not {tuple(a.shape)} and {tuple(b.shape)}")
        n = int(a.shape[0])
        if n > 65536:
            raise ValueError(f"at most 65536 rays per call, not {n}")
        ray_radius = float(ray_radius)
        if not np.isfinite(ray_radius) or ray_radius < 0.0:
            raise ValueError(f"ray_radius must be finite and >= 0, not {ray_radius}")
        rgb = None
        if ray_colors is not None:
            rgb = np.ascontiguousarray(ray_colors, dtype=np.uint8)
            if rgb.shape != (n, 3):
                raise ValueError(f"ray_colors must be uint8 [{n},3], not {rgb.shape}")
        return a, b, ray_radius, rgb

    def render_ray_view_device(self, mesh: Mesh, landmarks, starts, ends, poses=None, size: int = 1024, frame="fit", radius=None,
                               ray_radius: float = 0.5, colors=None, ray_colors=None, return_pixels: bool = False):
        """``render_ray_view`` with the results left on the device: uint8 [n,S,S,4] RGBA (and int32 [n,NL], int32 [n,NR] with
        ``return_pixels``).  Device tensors of rays are read where they are.  Only enqueues work."""
        import torch

        a, b, ray_radius, rrgb = self.ray_view_arguments(starts, ends, ray_radius, ray_colors)
        poses, frames, lm, radius = self.landmark_view_arguments(mesh, landmarks, poses, frame, radius)
        n, nl, nr = poses.shape[0], lm.shape[0], int(a.shape[0])
        rgb, size = self._view_colours_and_size(colors, nl, size)
        dev = torch.device("cuda", self.ctx.device)
        a_dev = a.to(dev) if hasattr(a, "data_ptr") else torch.from_numpy(a).to(dev)
        b_dev = b.to(dev) if hasattr(b, "data_ptr") else torch.from_numpy(b).to(dev)
        out = torch.empty((n, size, size, 4), dtype=torch.uint8, device=dev)
        pixels = torch.empty((n, nl), dtype=torch.int32, device=dev) if return_pixels else None
        ray_pixels = torch.empty((n, nr), dtype=torch.int32, device=dev) if return_pixels else None
        rot = np.ascontiguousarray(view_rotations(poses), dtype=np.float64)
        handle = upload_mesh(self.ctx, mesh)
        self.ctx.bind_current_stream(torch, dev)
        self._push_render_mode()  # (the view reads the shading and the sub-pixel bits)
        self.ctx.check(self.ctx.lib.mvlm_render_ray_view(
            self.ctx.handle, handle, _lib.as_ptr(rot, C.c_double), n, size, _lib.as_ptr(frames, C.c_float),
            _lib.as_ptr(lm, C.c_double) if nl else None, nl, C.c_float(radius), None if rgb is None or nl == 0 else _lib.as_ptr(rgb, C.c_uint8),
            C.c_void_p(a_dev.data_ptr()) if nr else None, C.c_void_p(b_dev.data_ptr()) if nr else None, nr, C.c_float(ray_radius),
            None if rrgb is None or nr == 0 else _lib.as_ptr(rrgb, C.c_uint8), C.c_void_p(out.data_ptr()),
            C.c_void_p(pixels.data_ptr()) if pixels is not None and nl else None,
            C.c_void_p(ray_pixels.data_ptr()) if ray_pixels is not None and nr else None), ValueError)
        self._ray_view_keepalive = (a_dev, b_dev)  # (read by the enqueued kernels)
        return (out, pixels, ray_pixels) if return_pixels else out

    def render_ray_view(self, mesh: Mesh, landmarks, starts, ends, poses=None, size: int = 1024, frame="fit", radius=None,
                        ray_radius: float = 0.5, colors=None, ray_colors=None, return_pixels: bool = False):
        """The landmark view with every ray ``starts[r] -> ends[r]`` drawn between the mesh and the spheres, as the reference's
        ``RayVisualizer`` shows them (visualization/ray_visualizer.py): an opaque, head-lit tube of ``ray_radius`` model units,
        green unless ``ray_colors`` (uint8 [NR,3]) says otherwise, depth-tested against the mesh and the spheres.  uint8 [n,S,S,3];
        with ``return_pixels`` also int32 [n,NL] and int32 [n,NR], the pixels each sphere and each ray won in each view.
        ``starts`` / ``ends`` [..., 3]: numpy arrays or device tensors (``HipEstimator3D.lines_device``'s, clipped or not), in
        the mesh's coordinates; a ray with a non-finite coordinate is left out.  ``frame="fit"`` fits the mesh and the landmarks,
        not the rays, which reach 500 units out.  The other arguments: ``render_landmark_view`` ("Ray view")."""
        res = self.render_ray_view_device(mesh, landmarks, starts, ends, poses, size, frame, radius, ray_radius, colors, ray_colors,
                                          return_pixels)
        out, pixels, ray_pixels = res if return_pixels else (res, None, None)
        image = out.cpu().numpy()[..., :3].copy()
        counts = pixels.cpu().numpy() if pixels is not None else None
        ray_counts = ray_pixels.cpu().numpy() if ray_pixels is not None else None
        self.check()
        return (image, counts, ray_counts) if return_pixels else image

    # ---- view sheet (prediction/predictor2d.py's draw_image_with_landmarks, all views in one picture) ----------
    @staticmethod
    def view_sheet_layout(n_views: int, cols=None, scale: int = 1, gap: int = 2) -> tuple:
        """(cols, rows, width, height) of a sheet of ``n_views`` views (mvlm_view_sheet_layout; no GPU): ``cols`` columns, default
        ceil(sqrt(n_views)), cells of 256 * scale pixels, ``gap`` pixels between them and around the sheet.  ValueError with the
        library's reason for what does not fit (a side above 4096: the message names the largest scale that does)."""
        return HipRenderer3D._sheet_layout("view sheet", n_views, cols, scale, gap)

    @staticmethod
    def _sheet_layout(label: str, n_views, cols, scale, gap) -> tuple:
        """``view_sheet_layout`` for the picture ``label`` names in its refusals (the view sheet, the heat sheet)."""
        for name, value in (("n_views", n_views), ("scale", scale), ("gap", gap)) + ((("cols", cols),) if cols is not None else ()):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError(f"{label}: {name} must be an integer, not {value!r}")
        if cols is not None and cols < 1:
            raise ValueError(f"{label}: cols must be at least 1 ({cols} given)")
        out = [C.c_int() for _ in range(4)]
        why = C.create_string_buffer(512)
        rc = _lib.load().mvlm_view_sheet_layout(int(n_views), 0 if cols is None else int(cols), int(scale), int(gap),
                                                *[C.byref(o) for o in out], why, len(why))
        if rc != 0:
            raise ValueError(f"{label}: {why.value.decode()}")
        return tuple(int(o.value) for o in out)

    def _sheet_tensor(self, x, what, dtype, dev, shape_ok, shape_words, label="view sheet"):
        """A view-sheet (or, with its ``label``, heat-sheet) input on the renderer's device: a tensor is taken where it lies (dtype,
        device and shape checked), anything else is made a numpy array of that dtype and uploaded."""
        import torch

        if hasattr(x, "data_ptr"):
            if x.dtype != dtype:
                raise ValueError(f"{label}: {what} must be {dtype}, not {x.dtype}")
            if x.device != dev:
                raise ValueError(f"{label}: {what} lives on {x.device}, the renderer on {dev}")
            t = x
        else:
            try:
                a = np.ascontiguousarray(x, dtype={torch.float32: np.float32}[dtype])
            except (TypeError, ValueError) as e:
                raise ValueError(f"{label}: {what} is not a numeric array ({e})") from None
            t = None if not shape_ok(a.shape) else torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        if t is None or not shape_ok(tuple(t.shape)):
            raise ValueError(f"{label}: {what} must be {shape_words}, not {tuple(np.shape(x) if t is None else t.shape)}")
        return t.contiguous()

    def render_view_sheet_device(self, images, maxima=None, rot=None, landmarks=None, colors=None, used=None, background="rgb",
                                 cols=None, scale: int = 1, gap: int = 2, marker_radius: float = 2.0, chan_sel=None):
        """``render_view_sheet`` with the picture left on the device: uint8 [H,W,4] RGBA, the layout ``encode_png`` takes.  Only
        enqueues work."""
        import torch

        dev = torch.device("cuda", self.ctx.device)
        images = self._sheet_tensor(images, "images", torch.float32, dev, lambda s: len(s) == 4 and s[0] >= 1 and tuple(s[1:]) == (256, 256, 4),
                                    "float32 [N,256,256,4]")
        n = int(images.shape[0])
        _, _, width, height = self.view_sheet_layout(n, cols, scale, gap)
        nl = 0
        if maxima is not None:
            maxima = self._sheet_tensor(maxima, "maxima", torch.float32, dev, lambda s: len(s) == 3 and s[1] == n and s[2] == 3,
                                        f"float32 [NL,{n},3]")
            nl = int(maxima.shape[0])
            if nl > 65536:
                raise ValueError(f"view sheet: at most 65536 landmarks, not {nl}")

        def host(x, what, dtype, shape, words):
            if x is None:
                return None
            if hasattr(x, "data_ptr"):
                x = x.detach().cpu().numpy()
            try:
                a = np.ascontiguousarray(x, dtype=dtype)
            except (TypeError, ValueError) as e:
                raise ValueError(f"view sheet: {what} is not a numeric array ({e})") from None
            if a.size != int(np.prod(shape)) or a.ndim < 1 or (a.ndim > 1 and a.shape[0] != shape[0]):
                raise ValueError(f"view sheet: {what} must be {words}, not {a.shape}")
            return np.ascontiguousarray(a.reshape(shape))

        rot = host(rot, "rot", np.float64, (n, 9), f"float64 [{n},3,3]")
        landmarks = host(landmarks, "landmarks", np.float64, (nl, 3), f"float64 [{nl},3]")
        colors = host(colors, "colors", np.uint8, (nl, 3), f"uint8 [{nl},3]")
        used = host(used, "used", np.uint8, (nl, n), f"uint8 [{nl},{n}]")
        if rot is not None and not np.isfinite(rot).all():
            raise ValueError("view sheet: non-finite rotation")
        if background == "auto":  # the planes the predictor read (Pipeline passes its chan_sel); unknown: the RGB planes
            background = "rgb" if chan_sel is None or any(int(c) < 3 for c in chan_sel) else "depth"
        if background not in ("rgb", "depth"):
            raise ValueError(f'view sheet: background must be "rgb", "depth" or "auto", not {background!r}')
        try:
            marker_radius = float(marker_radius)
        except (TypeError, ValueError):
            raise ValueError(f"view sheet: marker_radius must be a number, not {marker_radius!r}") from None
        if not np.isfinite(marker_radius) or not 0.5 <= marker_radius <= 16.0:
            raise ValueError(f"view sheet: marker_radius must be finite and in 0.5..16, not {marker_radius}")
        out = torch.empty((height, width, 4), dtype=torch.uint8, device=dev)
        residuals = nl > 0 and rot is not None and landmarks is not None
        self.ctx.bind_current_stream(torch, dev)
        self.ctx.check(self.ctx.lib.mvlm_render_view_sheet(
            self.ctx.handle, C.c_void_p(images.data_ptr()), n, C.c_void_p(maxima.data_ptr()) if nl else None, nl,
            _lib.as_ptr(rot, C.c_double) if residuals else None, _lib.as_ptr(landmarks, C.c_double) if residuals else None,
            _lib.as_ptr(colors, C.c_uint8) if nl and colors is not None else None,
            _lib.as_ptr(used, C.c_uint8) if nl and used is not None else None, 1 if background == "depth" else 0,
            0 if cols is None else int(cols), int(scale), int(gap), C.c_double(marker_radius), C.c_void_p(out.data_ptr())), ValueError)
        self._sheet_keepalive = (images, maxima)  # (read by the enqueued kernels)
        return out

    def render_view_sheet(self, images, maxima=None, rot=None, landmarks=None, colors=None, used=None, background="rgb", cols=None,
                          scale: int = 1, gap: int = 2, marker_radius: float = 2.0, chan_sel=None):
        """Every rendered view in one picture with the network's 2-D predictions on it - the reference's
        ``Predictor2D.draw_image_with_landmarks`` for all views at once: uint8 [H,W,3].  ``images`` float32 [N,256,256,4]
        (``render_device``'s stack), ``maxima`` float32 [NL,N,3] (``predict_device``'s) - tensors on the renderer's device, or numpy
        arrays, which are uploaded.  A marker of ``marker_radius`` view pixels stands where each prediction's ray pierces its view
        (a ring where ``used`` uint8 [NL,N] is 0), in ``colors`` uint8 [NL,3] (default blue); with ``rot`` float64 [N,3,3] (``view_rotations``)
        and ``landmarks`` float64 [NL,3] (the space the mesh was uploaded in) a red residual runs from each marker to where its landmark
        projects in that view.  ``background``: "rgb", "depth", or "auto" (depth when ``chan_sel`` names no plane below 3).  Views sit
        in ``cols`` columns (default ceil(sqrt(N))), ``scale`` 1..4 sheet pixels per view pixel, ``gap`` 0..16 grey pixels between
        them ("View sheet")."""
        out = self.render_view_sheet_device(images, maxima, rot, landmarks, colors, used, background, cols, scale, gap, marker_radius,
                                            chan_sel)
        image = out.cpu().numpy()[..., :3].copy()
        self.check()
        return image

    # ---- heat sheet (the view sheet's cells with the network's heatmaps laid over them) ---------------------------
    def render_heat_sheet_device(self, images, heat, landmarks=None, colors=None, background="rgb", cols=None, scale: int = 1,
                                 gap: int = 2, floor: float = 0.25, opacity: float = 0.75, chan_sel=None):
        """``render_heat_sheet`` with the picture left on the device: uint8 [H,W,4] RGBA, the layout ``encode_png`` takes.  Only
        enqueues work; every bad argument is a ValueError that starts with "heat sheet:", raised before any launch."""
        import torch

        label = "heat sheet"
        # what needs no tensor first: a bad scalar is refused before anything is uploaded
        picked = None
        if landmarks is not None:
            try:
                picked = [operator.index(k) for k in landmarks]
            except TypeError:
                raise ValueError(f"{label}: landmarks must be None or a sequence of integers, not {landmarks!r}") from None
            if any(isinstance(k, (bool, np.bool_)) for k in landmarks):
                raise ValueError(f"{label}: landmarks must be None or a sequence of integers, not {landmarks!r}")
            if len(set(picked)) != len(picked):
                raise ValueError(f"{label}: landmarks must be distinct, not {picked!r}")
        if background == "auto":  # the planes the predictor read (Pipeline passes its chan_sel); unknown: the RGB planes
            background = "rgb" if chan_sel is None or any(int(c) < 3 for c in chan_sel) else "depth"
        if background not in ("rgb", "depth"):
            raise ValueError(f'{label}: background must be "rgb", "depth" or "auto", not {background!r}')
        try:
            floor, opacity = float(floor), float(opacity)
        except (TypeError, ValueError):
            raise ValueError(f"{label}: floor and opacity must be numbers, not {floor!r} and {opacity!r}") from None
        if not (np.isfinite(floor) and 0.0 <= floor < 1.0):
            raise ValueError(f"{label}: floor must be finite and in [0, 1), not {floor}")
        if not (np.isfinite(opacity) and 0.0 < opacity <= 1.0):
            raise ValueError(f"{label}: opacity must be finite and in (0, 1], not {opacity}")
        try:
            shape = tuple(np.shape(images))
        except ValueError:
            shape = ()
        if len(shape) == 4 and shape[0] >= 1:  # (any other shape: refused below, in _sheet_tensor's words)
            _, _, width, height = self._sheet_layout(label, int(shape[0]), cols, scale, gap)
        dev = torch.device("cuda", self.ctx.device)
        images = self._sheet_tensor(images, "images", torch.float32, dev, lambda s: len(s) == 4 and s[0] >= 1 and tuple(s[1:]) == (256, 256, 4),
                                    "float32 [N,256,256,4]", label)
        n = int(images.shape[0])
        heat = self._sheet_tensor(heat, "heat", torch.float32, dev,
                                  lambda s: len(s) == 4 and s[0] == n and s[1] >= 1 and tuple(s[2:]) == (256, 256),
                                  f"float32 [{n},NL,256,256]", label)
        nl = int(heat.shape[1])
        if nl > 65536 or n * nl > 32768:
            raise ValueError(f"{label}: at most 65536 landmarks and 32768 planes (views x landmarks) per call, not {n} x {nl}")
        if heat.data_ptr() % 16:
            raise ValueError(f"{label}: heat must be 16-byte aligned on the device")
        sel = None
        if picked is not None:
            if any(not 0 <= k < nl for k in picked):
                raise ValueError(f"{label}: landmarks must lie in 0..{nl - 1}, not {picked!r}")
            sel = np.zeros(nl, np.uint8)
            sel[picked] = 1
        if colors is not None:
            if hasattr(colors, "data_ptr"):
                colors = colors.detach().cpu().numpy()
            try:
                colors = np.ascontiguousarray(colors, dtype=np.uint8)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{label}: colors is not a numeric array ({e})") from None
            if colors.shape != (nl, 3):
                raise ValueError(f"{label}: colors must be uint8 [{nl},3], not {colors.shape}")
        out = torch.empty((height, width, 4), dtype=torch.uint8, device=dev)
        self.ctx.bind_current_stream(torch, dev)
        self.ctx.check(self.ctx.lib.mvlm_render_heat_sheet(
            self.ctx.handle, C.c_void_p(images.data_ptr()), C.c_void_p(heat.data_ptr()), n, nl,
            _lib.as_ptr(sel, C.c_uint8) if sel is not None else None, _lib.as_ptr(colors, C.c_uint8) if colors is not None else None,
            1 if background == "depth" else 0, 0 if cols is None else int(cols), int(scale), int(gap), C.c_double(floor),
            C.c_double(opacity), C.c_void_p(out.data_ptr())), ValueError)
        self._sheet_keepalive = (images, heat)  # (read by the enqueued kernels)
        return out

    def render_heat_sheet(self, images, heat, landmarks=None, colors=None, background="rgb", cols=None, scale: int = 1, gap: int = 2,
                          floor: float = 0.25, opacity: float = 0.75, chan_sel=None):
        """Every rendered view in one picture - the cells of ``render_view_sheet(images)`` - with the network's heatmaps laid over
        it: uint8 [H,W,3].  ``images`` float32 [N,256,256,4] (``render_device``'s stack), ``heat`` float32 [N,NL,256,256]
        (``HipPaulsenModel.heatmaps_device``'s) - tensors on the renderer's device, or numpy arrays, which are uploaded.  Per view
        pixel the landmark of ``landmarks`` (None: all; else distinct ints in 0..NL-1) whose value is the largest share t of its
        plane's largest finite value wins, the lowest index on a tie, and is laid over the background in its colour of ``colors`` uint8
        [NL,3] (default red) with opacity ``opacity`` * (t - ``floor``) / (1 - ``floor``); t <= ``floor`` draws nothing.  Heat pixel
        [row, col] lies over image pixel [row, col]; no markers are drawn.  ``background``, ``cols``, ``scale``, ``gap``:
        ``render_view_sheet`` ("Heat sheet")."""
        out = self.render_heat_sheet_device(images, heat, landmarks, colors, background, cols, scale, gap, floor, opacity, chan_sel)
        image = out.cpu().numpy()[..., :3].copy()
        self.check()
        return image

    def _stage_ms(self, entry: str, n: int) -> np.ndarray:
        """The ``n`` stage times, float32 milliseconds, that the library's reader ``entry`` gives for its feature's last call."""
        ms = np.zeros(n, np.float32)
        self.ctx.check(getattr(self.ctx.lib, entry)(self.ctx.handle, _lib.as_ptr(ms, C.c_float)))
        return ms

    def heat_sheet_stage_ms(self) -> np.ndarray:
        """Milliseconds of the last heat sheet's stages under render profiling: background, peak, compose."""
        return self._stage_ms("mvlm_heat_sheet_stage_ms", 3)

    # ---- surface heat (all views' heatmaps laid on the scan) ---------------------------------------------------
    def surface_heat(self, mesh: Mesh, images, heat, rot, landmarks=None, colors=None, floor: float = 0.25, opacity: float = 0.75,
                     depth_tol: int = 2, return_scores: bool = False) -> dict:
        """All views' heatmaps laid on the scan (mvlm_surface_heat; DESIGN.md 5.1, "Surface heat").  ``images`` float32
        [N,256,256,4] (``render_device``'s stack of ``mesh``), ``heat`` float32 [N,NL,256,256] (``HipPaulsenModel.heatmaps_device``'s)
        - tensors on the renderer's device, or numpy arrays, which are uploaded; ``rot`` the views' rotations: float64 [N,3,3] /
        [N,9] as a tensor or an array (``view_rotations``), or ``rotations_device()``'s handle.  Every vertex is carried into every
        view as the render carried it; a view sees it when it lies at most ``depth_tol`` depth steps (0..255; one is 5.9 model units)
        behind the view's depth plane, and then adds the share its heatmap value there has of its plane's peak.  A vertex's score
        for a landmark is the mean of those shares over the views that see it.  Returns a dict of device tensors: ``colors`` uint8
        [V,4] - per vertex the landmark of ``landmarks`` (None: all; else distinct ints in 0..NL-1) with the largest score, the
        lowest index on a tie, laid over the vertex's own colour (its colour, else its texel, else grey 200) in its colour of
        ``colors`` uint8 [NL,3] (default red) with opacity ``opacity`` * (score - ``floor``) / (1 - ``floor``), nothing at a score
        <= ``floor``: what ``render_landmark_view(vertex_colors=)`` takes -, ``peak_vertex`` int32 [NL] (per landmark the vertex
        of the largest score above 0, -1: none), ``peak_score`` float32 [NL], ``n_visible`` int32 [V], and with ``return_scores``
        ``scores`` float32 [V,NL].  Only enqueues work; every bad argument is a ValueError that starts with "surface heat:",
        raised before any launch."""
        import torch

        label = "surface heat"
        picked = None
        if landmarks is not None:
            try:
                picked = [operator.index(k) for k in landmarks]
            except TypeError:
                raise ValueError(f"{label}: landmarks must be None or a sequence of integers, not {landmarks!r}") from None
            if any(isinstance(k, (bool, np.bool_)) for k in landmarks):
                raise ValueError(f"{label}: landmarks must be None or a sequence of integers, not {landmarks!r}")
            if len(set(picked)) != len(picked):
                raise ValueError(f"{label}: landmarks must be distinct, not {picked!r}")
        try:
            floor, opacity = float(floor), float(opacity)
        except (TypeError, ValueError):
            raise ValueError(f"{label}: floor and opacity must be numbers, not {floor!r} and {opacity!r}") from None
        if not (np.isfinite(floor) and 0.0 <= floor < 1.0):
            raise ValueError(f"{label}: floor must be finite and in [0, 1), not {floor}")
        if not (np.isfinite(opacity) and 0.0 < opacity <= 1.0):
            raise ValueError(f"{label}: opacity must be finite and in (0, 1], not {opacity}")
        if isinstance(depth_tol, (bool, np.bool_)) or not isinstance(depth_tol, (int, np.integer)) or not 0 <= depth_tol <= 255:
            raise ValueError(f"{label}: depth_tol must be an integer in 0..255, not {depth_tol!r}")
        if not isinstance(mesh, Mesh):
            raise ValueError(f"{label}: mesh must be a Mesh, not {type(mesh).__name__}")
        if mesh.n_tris == 0:
            raise ValueError(f"{label}: a point cloud is not supported here (the mesh has no triangles)")
        dev = torch.device("cuda", self.ctx.device)
        images = self._sheet_tensor(images, "images", torch.float32, dev, lambda s: len(s) == 4 and s[0] >= 1 and tuple(s[1:]) == (256, 256, 4),
                                    "float32 [N,256,256,4]", label)
        n = int(images.shape[0])
        heat = self._sheet_tensor(heat, "heat", torch.float32, dev,
                                  lambda s: len(s) == 4 and s[0] == n and s[1] >= 1 and tuple(s[2:]) == (256, 256),
                                  f"float32 [{n},NL,256,256]", label)
        nl, nv = int(heat.shape[1]), int(mesh.n_verts)
        if nl > 65536 or n * nl > 32768:
            raise ValueError(f"{label}: at most 65536 landmarks and 32768 planes (views x landmarks) per call, not {n} x {nl}")
        if nv * nl > 1 << 28:
            raise ValueError(f"{label}: at most 268435456 scores (vertices x landmarks) per call, not {nv} x {nl}")
        if heat.data_ptr() % 16 or images.data_ptr() % 16:
            raise ValueError(f"{label}: images and heat must be 16-byte aligned on the device")
        if isinstance(rot, _DevicePointer):
            rot_keep = rot
        else:
            if hasattr(rot, "data_ptr"):
                if rot.dtype != torch.float64 or rot.numel() != n * 9:
                    raise ValueError(f"{label}: rot must be float64 [{n},3,3], not {rot.dtype} {tuple(rot.shape)}")
                rot_host = rot.detach().cpu().numpy()
            else:
                try:
                    rot_host = np.ascontiguousarray(rot, dtype=np.float64)
                except (TypeError, ValueError) as e:
                    raise ValueError(f"{label}: rot is not a numeric array ({e})") from None
                if rot_host.size != n * 9:
                    raise ValueError(f"{label}: rot must be float64 [{n},3,3], not {rot_host.shape}")
            if not np.isfinite(rot_host).all():
                raise ValueError(f"{label}: non-finite rotation")
            rot_keep = rot.to(dev).contiguous() if hasattr(rot, "data_ptr") else torch.from_numpy(rot_host.reshape(n, 9).copy()).to(dev)
        sel = None
        if picked is not None:
            if any(not 0 <= k < nl for k in picked):
                raise ValueError(f"{label}: landmarks must lie in 0..{nl - 1}, not {picked!r}")
            sel = np.zeros(nl, np.uint8)
            sel[picked] = 1
        if colors is not None:
            if hasattr(colors, "data_ptr"):
                colors = colors.detach().cpu().numpy()
            try:
                colors = np.ascontiguousarray(colors, dtype=np.uint8)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{label}: colors is not a numeric array ({e})") from None
            if colors.shape != (nl, 3):
                raise ValueError(f"{label}: colors must be uint8 [{nl},3], not {colors.shape}")
        out = {"colors": torch.empty((nv, 4), dtype=torch.uint8, device=dev),
               "peak_vertex": torch.empty((nl,), dtype=torch.int32, device=dev),
               "peak_score": torch.empty((nl,), dtype=torch.float32, device=dev),
               "n_visible": torch.empty((nv,), dtype=torch.int32, device=dev)}
        if return_scores:
            out["scores"] = torch.empty((nv, nl), dtype=torch.float32, device=dev)
        self.ctx.bind_current_stream(torch, dev)
        handle = upload_mesh(self.ctx, mesh)
        self._push_render_mode()  # (the positions are the render's: its sub-pixel bits)
        self.ctx.check(self.ctx.lib.mvlm_surface_heat(
            self.ctx.handle, handle, C.c_void_p(rot_keep.data_ptr()), C.c_void_p(images.data_ptr()), C.c_void_p(heat.data_ptr()), n, nl,
            _lib.as_ptr(sel, C.c_uint8) if sel is not None else None, _lib.as_ptr(colors, C.c_uint8) if colors is not None else None,
            C.c_double(floor), C.c_double(opacity), int(depth_tol), C.c_void_p(out["colors"].data_ptr()),
            C.c_void_p(out["scores"].data_ptr()) if return_scores else None, C.c_void_p(out["n_visible"].data_ptr()),
            C.c_void_p(out["peak_vertex"].data_ptr()), C.c_void_p(out["peak_score"].data_ptr())), ValueError)
        self._surface_keepalive = (images, heat, rot_keep)  # (read by the enqueued kernels)
        return out

    def surface_heat_stage_ms(self) -> np.ndarray:
        """Milliseconds of the last surface heat's stages under render profiling: peak, back-projection, paint."""
        return self._stage_ms("mvlm_surface_heat_stage_ms", 3)

    def release_surface_heat(self) -> None:
        """Free the scratch ``surface_heat`` keeps in the context (its score table above all: 4 bytes per vertex and landmark);
        waits for the stream.  The next call allocates again."""
        self.ctx.check(self.ctx.lib.mvlm_surface_heat_release(self.ctx.handle))

    def scratch_bytes(self, prefix: str = "") -> int:
        """Bytes of the context's internal scratch whose names start with ``prefix`` ("backproject": the surface heat's)."""
        n = C.c_size_t()
        self.ctx.check(self.ctx.lib.mvlm_scratch_bytes(self.ctx.handle, prefix.encode(), C.byref(n)))
        return int(n.value)

    # ---- surface distances between landmarks ----------------------------------------------------
    def landmark_geodesics(self, mesh: Mesh, points, *, init_rings: int = 2, pairs=None, return_fields: bool = False,
                           max_sweeps: int = 4096, max_scratch_bytes: int = 0):
        """The distances between landmarks, straight and along the scan's triangles (mvlm_landmark_geodesics; DESIGN.md 5.1,
        "Surface distances").  ``points`` float64 [n,3], host or device, in the space of ``mesh``; each is attached to the surface as
        the landmark report attaches it.  ``pairs``: None for every pair, else a sequence of (i, j) - only the landmarks named get a
        distance field and only those entries are computed.  ``init_rings`` 0..8: rings of triangles round the source triangle that
        start at their straight distance.  Returns a ``LandmarkDistances`` (utils/distances.py); with ``return_fields`` its
        ``fields`` is the float64 [n,V] device tensor of the distance fields.  The surface distance is the first-order fast-marching
        discretisation, an overestimate of a few per cent, not an exact geodesic.  Waits for the stream.  ValueError for a point
        cloud, bad values, or a source that does not settle within ``max_sweeps`` sweeps."""
        import torch

        from .distances import LandmarkDistances, check_pairs

        label = "landmark_geodesics"
        if not isinstance(mesh, Mesh):
            raise ValueError(f"{label}: mesh must be a Mesh, not {type(mesh).__name__}")
        if mesh.n_tris == 0:
            raise ValueError(f"{label}: a point cloud is not supported here (the mesh has no triangles; triangulate_point_cloud gives it some)")
        for name, value, lo, hi in (("init_rings", init_rings, 0, 8), ("max_sweeps", max_sweeps, 1, 1 << 20),
                                    ("max_scratch_bytes", max_scratch_bytes, 0, 1 << 62)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
                raise ValueError(f"{label}: {name} must be an integer in {lo}..{hi}, not {value!r}")
        dev = torch.device("cuda", self.ctx.device)
        if hasattr(points, "data_ptr"):
            pts = points.detach().to(device=dev, dtype=torch.float64).contiguous()
        else:
            try:
                pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).to(dev)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{label}: points is not a numeric array ({e})") from None
        if pts.dim() != 2 or pts.shape[1] != 3 or not 1 <= pts.shape[0] <= 65536:
            raise ValueError(f"{label}: points must be float64 [n,3] with n in 1..65536, not {tuple(pts.shape)}")
        n, nv = int(pts.shape[0]), int(mesh.n_verts)
        pairs = check_pairs(pairs, n, f"{label}: pairs")
        snapped = torch.empty((n, 3), dtype=torch.float64, device=dev)
        tri = torch.empty((n,), dtype=torch.int32, device=dev)
        directed = torch.empty((n, n), dtype=torch.float64, device=dev)
        euclid = torch.empty((n, n), dtype=torch.float64, device=dev)
        sweeps = torch.empty((n,), dtype=torch.int32, device=dev)
        fields = torch.empty((n, nv), dtype=torch.float64, device=dev) if return_fields else None
        self.ctx.bind_current_stream(torch, dev)
        handle = upload_mesh(self.ctx, mesh)
        self.ctx.check(self.ctx.lib.mvlm_landmark_geodesics(
            self.ctx.handle, handle, C.c_void_p(pts.data_ptr()), n, int(init_rings), int(max_sweeps), C.c_longlong(int(max_scratch_bytes)),
            _lib.as_ptr(pairs, C.c_int32) if pairs is not None else None, 0 if pairs is None else int(pairs.shape[0]),
            C.c_void_p(snapped.data_ptr()), C.c_void_p(tri.data_ptr()), C.c_void_p(directed.data_ptr()), C.c_void_p(euclid.data_ptr()),
            C.c_void_p(sweeps.data_ptr()), C.c_void_p(fields.data_ptr()) if return_fields else None), ValueError)
        return LandmarkDistances(snapped.cpu().numpy(), tri.cpu().numpy(), euclid.cpu().numpy(), directed.cpu().numpy(),
                                 sweeps.cpu().numpy(), pairs, fields)

    def geodesic_stage_ms(self) -> np.ndarray:
        """Milliseconds of the last ``landmark_geodesics``'s stages under render profiling: adjacency, init, sweeps, targets."""
        return self._stage_ms("mvlm_geodesic_stage_ms", 4)

    def release_geodesics(self) -> None:
        """Free the scratch ``landmark_geodesics`` keeps in the context (adjacency, field buffers); waits for the stream."""
        self.ctx.check(self.ctx.lib.mvlm_geodesic_release(self.ctx.handle))

    # ---- PNG on the device -------------------------------------------------------------------
    @staticmethod
    def png_bound(height: int, width: int) -> int:
        """Bytes that hold any file ``encode_png`` writes for a picture of this size (mvlm_png_bound; no GPU)."""
        n = C.c_size_t()
        if _lib.load().mvlm_png_bound(int(height), int(width), C.byref(n)) != 0:
            raise ValueError(f"png: height and width must be 1..4096, not {height} x {width}")
        return int(n.value)

    def encode_png(self, rgba, filter_mode: int = -1) -> list:
        """The pictures of a uint8 device tensor [H,W,4] or [n,H,W,4] (RGBA as ``render_landmark_view_device`` and
        ``render_ray_view_device`` leave them; alpha is dropped) as complete 8-bit RGB PNG files, one ``bytes`` per picture,
        filtered and compressed on the device: only the compressed bytes cross to the host (mvlm_png_encode).
        ``filter_mode`` -1 picks a filter type per row, 0..4 forces one."""
        import torch

        if not hasattr(rgba, "data_ptr") or not rgba.is_cuda or rgba.dtype != torch.uint8:
            raise ValueError("png: encode_png takes a uint8 tensor on the device")
        if rgba.device.index != self.ctx.device:
            raise ValueError(f"png: the tensor lives on {rgba.device}, the renderer on cuda:{self.ctx.device}")
        if rgba.dim() == 3:
            rgba = rgba[None]
        if rgba.dim() != 4 or rgba.shape[-1] != 4:
            raise ValueError(f"png: the pictures must be [H,W,4] or [n,H,W,4], not {tuple(rgba.shape)}")
        rgba = rgba.contiguous()
        n, h, w = int(rgba.shape[0]), int(rgba.shape[1]), int(rgba.shape[2])
        if n < 1 or not (1 <= h <= 4096 and 1 <= w <= 4096):
            raise ValueError(f"png: n >= 1 pictures of 1..4096 pixels a side, not {tuple(rgba.shape)}")
        stride = self.png_bound(h, w)
        host = np.empty((n, stride), dtype=np.uint8)
        sizes = (C.c_size_t * n)()
        self.ctx.bind_current_stream(torch, rgba.device)
        self.ctx.check(self.ctx.lib.mvlm_png_encode(self.ctx.handle, C.c_void_p(rgba.data_ptr()), n, h, w, int(filter_mode),
                                                    C.c_void_p(host.ctypes.data), C.c_size_t(stride), sizes), ValueError)
        return [host[i, :int(sizes[i])].tobytes() for i in range(n)]

    def png_stage_ms(self) -> np.ndarray:
        """Milliseconds of the last ``encode_png``'s stages under render profiling: filter, deflate, gather, copy to host."""
        return self._stage_ms("mvlm_png_stage_ms", 4)

    # ---- normals of a point cloud ---------------------------------------------------------------
    def estimate_point_normals(self, mesh: Mesh, return_neighbors: bool = False):
        """Normals of a point cloud estimated on the device (mvlm_mesh_estimate_normals; DESIGN.md 5.1, "Point clouds"): per point
        the least-variance direction of its 16 nearest neighbours, itself included - float32 [V,3], unit length, the sign
        unspecified, (0,0,0) for a non-finite point, fewer than 3 neighbours or coincident ones.  They become ``mesh.normals`` and
        the device copy's normals.  With ``return_neighbors`` also int32 [V,16]: per point the ids of those neighbours in ascending
        (squared distance, id), unused slots -1.  ValueError for a mesh with triangles."""
        import torch

        dev = torch.device("cuda", self.ctx.device)
        handle = upload_mesh(self.ctx, mesh)
        self.ctx.bind_current_stream(torch, dev)
        table = torch.empty((mesh.n_verts, 16), dtype=torch.int32, device=dev) if return_neighbors else None
        self.ctx.check(self.ctx.lib.mvlm_mesh_estimate_normals(self.ctx.handle, handle, None if table is None else C.c_void_p(table.data_ptr())),
                       ValueError)
        normals = np.empty((mesh.n_verts, 3), np.float32)
        self.ctx.check(self.ctx.lib.mvlm_mesh_copy_normals(self.ctx.handle, handle, _lib.as_ptr(normals, C.c_float)))
        mesh.normals = normals
        key = id(self.ctx)
        mesh._device[key] = mesh._device[key][:4] + ("estimated",)
        return (normals, table.cpu().numpy()) if return_neighbors else normals

    def normals_stage_ms(self) -> np.ndarray:
        """Milliseconds of the last normal estimate's stages under render profiling: grid build, search, solve."""
        return self._stage_ms("mvlm_normals_stage_ms", 3)

    # ---- a triangle surface for a point cloud ---------------------------------------------------
    def triangulate_point_cloud(self, mesh: Mesh) -> Mesh:
        """A point cloud -> a new ``Mesh`` with triangles over its points (mvlm_mesh_triangulate_points; DESIGN.md 5.1, "Point
        clouds"): every point votes for the Delaunay triangles of its 16 nearest neighbours in its tangent plane, a triangle is
        kept where its three corners agree and it is no sliver.  The neighbour table is the device's (mvlm_mesh_estimate_normals);
        the normals are ``mesh.normals`` where the cloud has them, else that estimate's.  The result holds the cloud's finite points
        in their order (triangle indices renumbered), their colours, the cloud's ``path`` and ``to_original``, and ``point_ids``,
        int32: the cloud's point behind every vertex.  It has no ``point_radius`` and no ``normals`` - a mesh with triangles takes
        neither.  Made once per cloud object and kept on it.  Meant for scanner-like sampling, not a general reconstruction.
        ValueError for a mesh with triangles."""
        import torch

        if mesh.n_tris != 0:
            raise ValueError("triangulate_point_cloud: the mesh has triangles (a surface is built for a point cloud)")
        kept = getattr(mesh, "_triangulation", None)
        if kept is not None:
            return kept
        dev = torch.device("cuda", self.ctx.device)
        ctx = self.ctx
        handle = upload_mesh(ctx, mesh)
        ctx.bind_current_stream(torch, dev)
        n_points = mesh.n_verts
        table = torch.empty((n_points, 16), dtype=torch.int32, device=dev)
        ctx.check(ctx.lib.mvlm_mesh_estimate_normals(ctx.handle, handle, C.c_void_p(table.data_ptr())), ValueError)
        key = id(ctx)
        mesh._device[key] = mesh._device[key][:4] + ("estimated",)
        if mesh.normals is not None:  # the cloud's own normals replace the estimate (the table stays)
            mesh._device[key] = mesh._device[key][:4] + (_send_point_normals(ctx, handle, mesh, "file"),)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        cap = 3 * n_points + 1024
        tris = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        for _ in range(2):
            ctx.check(ctx.lib.mvlm_mesh_triangulate_points(ctx.handle, handle, C.c_void_p(table.data_ptr()), C.c_void_p(tris.data_ptr()),
                                                           C.c_longlong(cap), C.c_void_p(count.data_ptr())), ValueError)
            n_tris = int(count.item())
            if n_tris <= cap:
                break
            cap = n_tris  # (more than three triangles a point: once more, with room for all of them)
            tris = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        tris = tris[:n_tris].cpu().numpy()
        verts = np.ascontiguousarray(mesh.verts, dtype=np.float32).reshape(-1, 3)
        finite = np.isfinite(verts).all(axis=1)
        point_ids = np.nonzero(finite)[0].astype(np.int32)
        renumber = (np.cumsum(finite) - 1).astype(np.int32)  # (no triangle touches a non-finite point)
        out = Mesh(np.ascontiguousarray(verts[finite]), np.ascontiguousarray(renumber[tris].reshape(-1, 3), dtype=np.int32), path=mesh.path,
                   to_original=mesh.to_original,
                   colors=None if mesh.colors is None else np.ascontiguousarray(np.asarray(mesh.colors)[finite]), point_ids=point_ids)
        if hasattr(mesh, "_colors_wanted"):
            out._colors_wanted = mesh._colors_wanted
        mesh._triangulation = out
        return out

    def surface_of(self, mesh: Mesh) -> Mesh:
        """``mesh`` itself, or - for a point cloud under ``point_surface="mesh"`` - its triangulation."""
        if self.point_surface == "mesh" and mesh is not None and getattr(mesh, "n_tris", 1) == 0:
            return self.triangulate_point_cloud(mesh)
        return mesh

    def cloud_mesh_stage_ms(self) -> np.ndarray:
        """Milliseconds of the last triangulation's stages under render profiling: star (with the shift), count + scan, emit."""
        return self._stage_ms("mvlm_cloud_mesh_stage_ms", 3)

    def rotations_device(self):
        """The last render's rotation table where the rasteriser keeps it on the device (f64[N,9]; valid until this context's
        next render): an object with ``data_ptr()`` that ``HipEstimator3D.lines_device(rot_dev=...)`` takes - the rays of the
        same views need the same matrices (estimator3d.py:57), so the table crosses PCIe once per mesh."""
        p = C.c_void_p()
        self.ctx.check(self.ctx.lib.mvlm_render_rotations_dev(self.ctx.handle, C.byref(p)))
        return _DevicePointer(p.value)

    def check(self):
        """Wait for the stream and raise if an enqueued render failed."""
        self.ctx.check(self.ctx.lib.mvlm_render_check(self.ctx.handle))

    def render_3d_multi_rgb_geometry_depth(self, transform_stack, file_name):
        """Signature of render3d.py:114; returns the *unscaled* 0..255 stack like the reference."""
        tt = time.time()
        mesh = file_name if isinstance(file_name, Mesh) else load_obj(file_name)
        if self.verbose:
            print("Render [1] - Setup time: ", f"{time.time() - tt:08.6f} s")
        tt = time.time()
        stack = self.render_device(mesh, np.asarray(transform_stack))
        image_stack = (stack * 255.0).round().cpu().numpy()
        self.check()
        if self.verbose:
            print("Render [2] - Render", f"{time.time() - tt:08.6f} s")
        return image_stack, mesh

    def _check_file(self, file_name: Path):
        file_name = Path(file_name)
        if not file_name.exists():
            raise FileNotFoundError(f"File {file_name} does not exist")
        if not file_name.is_file():
            raise FileNotFoundError(f"File {file_name} is not a file")
        if not file_name.suffix == ".obj":
            raise ValueError(f"File {file_name} is not an .obj file. Only .obj files are supported.")
        return file_name

    def multiview_render(self, file_name: Path, load_texture: bool = True):
        """render3d.py:179-193 - numpy results, as the slot contract requires.  ``load_texture``: see ``load_mesh``."""
        t = time.time()
        file_name = self._check_file(file_name)
        if self.verbose:
            print("Render [0] - Prepare", f"{time.time() - t:08.6f} s")
        transformation_stack = self.generate_3d_transformations()
        mesh = self.surface_of(self.load_mesh(file_name, load_texture=load_texture))
        image_stack = self.render_device(mesh, transformation_stack).cpu().numpy()
        self.check()
        return image_stack, transformation_stack, mesh

    def load_mesh(self, file_name: Path, load_texture: bool = True) -> Mesh:
        """OBJ (+ texture) from disk, through the ``pre_align`` block when one is set.
        ``load_texture=False`` leaves the JPEG alone (not even read) and keeps per-point colours off the device, and the
        consumer of a depth / geometry model's views reads no texture-shaded plane.  It is
        an argument of the call, decided by the caller that knows the consumer (``Pipeline._texture_needed``) - the
        renderer keeps no such state, so its public entry points load the texture like the reference (utils3d.py:26-36)."""
        from .prealign import aligned

        jpg = Path(file_name).with_suffix(".jpg")
        if not (load_texture and self.texture_decode == "device" and jpg.exists()):
            mesh = load_obj(file_name, load_texture=load_texture, decode=self.texture_decode)
            if not load_texture:
                mesh._colors_wanted = False  # nobody reads an RGB plane: per-point colours are not uploaded either
            return aligned(self._with_point_radius(mesh), self.pre_align)
        # The texture is decoded on the device by a second thread (read the .jpg, unstuff, GPU decode: 1.8 ms at 2048^2)
        # while this one parses the geometry (2.7 ms): the scan is ready when the slower of the two is.
        import threading

        box: list = [None, None, None, None]  # bytes, device texture, exception, host-decoded pixels (device refused)

        def texture_job():
            try:
                box[0] = jpg.read_bytes()
                box[1] = decode_texture_ahead(self.ctx, box[0])
                if box[1] is None:
                    # not a JPEG the device takes (progressive ones are common among exported textures): libjpeg on the host,
                    # HERE, beside the geometry parse - not afterwards on the caller's thread inside upload_mesh
                    from .mesh_io import decode_texture_bytes

                    box[3] = decode_texture_bytes(box[0])
            except Exception as e:  # noqa: BLE001 - "if we cannot load the texture, we just ignore it" (utils3d.py:35-36) ...
                box[2] = e        # ... but a failing GPU call is not a texture problem: raised below

        job = threading.Thread(target=texture_job, daemon=True)
        job.start()
        try:
            mesh = load_obj(file_name, load_texture=False)
        finally:
            job.join()
        if isinstance(box[2], ValueError):
            raise box[2]
        if mesh.uvs is not None and box[0] is not None:  # utils3d.py:26: only with tcoords
            mesh.texture_jpeg = box[0]
            mesh._texture_ahead = box[1]
            if box[1] is None:
                # decoded on the host by the texture thread (or not decodable at all: ignored, utils3d.py:35-36): the upload
                # goes straight to mvlm_mesh_upload, without a second look at the header
                mesh._texture = box[3]
                if box[3] is None:
                    mesh.texture_jpeg = None
        return aligned(self._with_point_radius(mesh), self.pre_align)

    def _with_point_radius(self, mesh: Mesh) -> Mesh:
        """A cloud read from a file gets the renderer's radius (None leaves the automatic one)."""
        if mesh.n_tris == 0 and self.point_radius is not None:
            mesh.point_radius = self.point_radius
        return mesh

    def multiview_render_device(self, file_or_mesh, transformation_stack=None):
        """Same, but the image stack stays in HBM (used by the fused pipeline path)."""
        mesh = file_or_mesh if isinstance(file_or_mesh, Mesh) else self.surface_of(self.load_mesh(self._check_file(file_or_mesh)))
        if transformation_stack is None:
            transformation_stack = self.generate_3d_transformations()
        return self.render_device(mesh, transformation_stack), transformation_stack, mesh
