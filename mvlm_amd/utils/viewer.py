"""Offscreen landmark view: the reference's ``VTKViewer(filename, landmarks, pname, save=True)`` (utils/viewer.py, main.py:66-67)
drawn by the HIP rasteriser (mvlm_render_landmark_view) instead of a VTK window.

``LandmarkViewer`` keeps ``VTKViewer``'s signature for the offscreen case: it loads the file, draws the front view with a blue
sphere at every landmark and writes ``visualization/<stem>[_<pname>].png`` relative to the working directory.  The interactive
window (``save=False``, ``--visualize-iter``) is out of scope.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np

__all__ = ["LandmarkViewer", "RayVisualizer", "RayVisualizerConfig", "view_path", "view_sheet_path", "heat_sheet_path", "surface_path", "HEAT_PALETTE",
           "heat_colours", "write_view_png"]


def _picture_path(filename, pname: str | None, kind: str) -> Path:
    suffix = f"_{pname}" if pname else ""
    return Path("visualization") / f"{Path(filename).stem}{suffix}{kind}.png"


def view_path(filename, pname: str | None = None) -> Path:
    """``visualization/<stem>[_<pname>].png`` relative to the working directory (viewer.py:89-92)."""
    return _picture_path(filename, pname, "")


def view_sheet_path(filename, pname: str | None = None) -> Path:
    """``visualization/<stem>[_<pname>]_views.png`` relative to the working directory: the view sheet beside the landmark view."""
    return _picture_path(filename, pname, "_views")


def heat_sheet_path(filename, pname: str | None = None) -> Path:
    """``visualization/<stem>[_<pname>]_heat.png`` relative to the working directory: the heat sheet beside the view sheet."""
    return _picture_path(filename, pname, "_heat")


def surface_path(filename, pname: str | None = None) -> Path:
    """``visualization/<stem>[_<pname>]_surface.png`` relative to the working directory: the surface heat beside the heat sheet."""
    return _picture_path(filename, pname, "_surface")


def select_rays(n_landmarks: int, n_views: int, landmark_indices=None, view_indices=None) -> tuple:
    """The rows (landmarks) and columns (views) of a ray table [NL,N,3] that a caller picked, as two lists: None means all,
    otherwise every index wraps round (``int(i) % n``: -1 is the last), as the reference's ``RayVisualizer`` takes them."""
    lm_idx = list(range(n_landmarks)) if landmark_indices is None else [int(i) % n_landmarks for i in landmark_indices]
    v_idx = list(range(n_views)) if view_indices is None else [int(i) % n_views for i in view_indices]
    return lm_idx, v_idx


# The heat sheet's default colours, cycled over the landmark index: neighbouring landmarks, whose blobs lie side by side, differ.
HEAT_PALETTE = ((255, 0, 0), (0, 200, 0), (0, 90, 255), (255, 200, 0), (255, 0, 255), (0, 220, 220), (255, 120, 0), (150, 60, 255))


def heat_colours(n_landmarks: int) -> np.ndarray:
    """uint8 [n_landmarks,3]: ``HEAT_PALETTE[l % len(HEAT_PALETTE)]`` for landmark l."""
    palette = np.asarray(HEAT_PALETTE, dtype=np.uint8)
    return palette[np.arange(int(n_landmarks)) % len(palette)].copy()


PNG_ENCODERS = ("host", "device")


def check_png_encoder(encoder: str) -> str:
    if encoder not in PNG_ENCODERS:
        raise ValueError(f"the PNG encoder must be 'host' or 'device', not {encoder!r}")
    return encoder


def write_view_png(image, out_path, encoder: str = "host", renderer=None):
    """uint8 [S,S,3] -> PNG through Pillow (as Pipeline.visualize_image_stack); makes the folder (viewer.py:93).

    ``encoder="device"``: ``image`` is the uint8 device tensor [S,S,4] a ``render_*_view_device`` call left (or [n,S,S,4] with
    ``out_path`` a sequence of n paths; the list of paths is returned): filtered and compressed on the device
    (``HipRenderer3D.encode_png``, all pictures in one call), so the pixels never cross to the host.  ``renderer``: the
    ``HipRenderer3D`` to encode with (default: one on the tensor's device)."""
    if check_png_encoder(encoder) == "device":
        if not hasattr(image, "data_ptr"):
            raise ValueError("write_view_png(encoder='device') takes the device tensor of a render_*_view_device call")
        if renderer is None:
            from .render3d import HipRenderer3D

            renderer = HipRenderer3D(n_views=1, device=image.device.index or 0, verbose=False)
        single = image.dim() == 3
        paths = [Path(out_path)] if single else [Path(q) for q in out_path]
        files = renderer.encode_png(image)
        if len(files) != len(paths):
            raise ValueError(f"{len(files)} pictures but {len(paths)} paths")
        for q, data in zip(paths, files):
            q.parent.mkdir(parents=True, exist_ok=True)
            q.write_bytes(data)
        return paths[0] if single else paths
    from PIL import Image

    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8)).save(out_path)
    return out_path


def render_to_png(renderer, kind: str, encoder: str, out, *args, first: bool = False, **kw) -> tuple:
    """``renderer.render_<kind>(*args, **kw)`` into the file ``out`` (a list: one file per picture) by the encoder asked for ->
    (pictures, what ``write_view_png`` returned).  "device": ``render_<kind>_device`` leaves the pictures on the device and one
    encode call makes all the files; ``first``: the call returns a stack of which the first picture is the one meant."""
    device = check_png_encoder(encoder) == "device"
    images = getattr(renderer, f"render_{kind}_device" if device else f"render_{kind}")(*args, **kw)
    if first:
        images = images[0]
    if device:
        written = write_view_png(images, out, encoder="device", renderer=renderer)
        renderer.check()
        return images, written
    return images, [write_view_png(im, q) for im, q in zip(images, out)] if isinstance(out, list) else write_view_png(images, out)


class LandmarkViewer:
    def __init__(self, filename, landmarks: np.ndarray | None = None, pname: str | None = None, save: bool = True,
                 size: int = 1024, device: int = 0, encoder: str = "host") -> None:
        if not save:
            raise NotImplementedError("LandmarkViewer draws offscreen only (save=True): the interactive window of the "
                                      "reference's VTKViewer (--visualize-iter) is out of scope")
        from .mesh_io import load_mesh
        from .render3d import HipRenderer3D

        self.pname = pname
        self.filename = Path(filename)
        self.size = int(size)
        renderer = HipRenderer3D(n_views=1, device=device, verbose=False)
        mesh = load_mesh(self.filename)
        image, self.out_path = render_to_png(renderer, "landmark_view", encoder, view_path(self.filename, pname), mesh, landmarks,
                                             first=True, size=self.size)
        if encoder == "device":  # the picture stays on the device; ``image`` is read back on demand only
            self.image_device, self.image = image, None
        else:
            self.image = image


def colour_byte(c: float) -> int:
    """A colour component in 0..1 as the byte the views carry: round(255 c), clamped."""
    return int(min(255, max(0, int(float(c) * 255.0 + 0.5))))


@dataclass
class RayVisualizerConfig:
    """What the offscreen ray view honours of the reference's ``RayVisualizerConfig`` (ray_visualizer.py) - ``ray_color``,
    ``landmark_color``, ``landmark_radius`` - and three fields of its own: the pictures' side in pixels, the rays' radius in
    model units (the reference draws lines 8 pixels wide, whatever the zoom) and the poses (degrees rx, ry, rz), one picture each;
    ``encoder``: "host" (Pillow) or "device" (the PNG files are made on the device, all pictures in one call).
    Rays are opaque here; the reference's 0.9 opacity and its bounding-box outline are left out."""
    ray_color: tuple = (0.1, 0.9, 0.1)
    landmark_color: tuple = (0.1, 0.1, 0.9)
    landmark_radius: float = 1.5
    size: int = 1024
    ray_radius: float = 0.5
    poses: tuple = ((0, 0, 0), (0, 60, 0), (0, -60, 0))
    encoder: str = "host"


class RayVisualizer:
    """The reference's ``RayVisualizer`` for the offscreen case: ``show`` selects and clips the rays as the reference does, draws
    them with the mesh and the landmarks (HipRenderer3D.render_ray_view) and writes one PNG per pose.  No window is opened."""

    def __init__(self, config: RayVisualizerConfig | None = None, device: int = 0):
        self.config = config or RayVisualizerConfig()
        self.device = device
        self.images = None

    def show(self, mesh, line_starts, line_ends, landmarks=None, screenshot_dir=None, landmark_indices=None, view_indices=None,
             obj_path=None, clip_to_mesh: bool = True):
        """``mesh``: a ``Mesh``; ``line_starts`` / ``line_ends`` [NL,N,3]; ``landmarks`` [NL,3] or None.  ``landmark_indices`` /
        ``view_indices`` pick rows and columns of the rays (default all).  The PNGs go to ``screenshot_dir`` (default
        ``visualization/ray_screenshots`` under the working directory) as ``<stem>_rays_<i>.png``, ``stem`` from ``obj_path``
        or the mesh's own path.  Returns their paths."""
        from .estimator3d import HipEstimator3D
        from .mesh_io import Mesh
        from .render3d import HipRenderer3D

        if not isinstance(mesh, Mesh):
            raise TypeError("RayVisualizer.show expects a Mesh (mvlm_amd.utils.load_mesh)")
        cfg = self.config
        starts, ends = np.asarray(line_starts, dtype=np.float64), np.asarray(line_ends, dtype=np.float64)
        if starts.ndim != 3 or starts.shape[-1] != 3 or starts.shape != ends.shape:
            raise ValueError(f"line_starts and line_ends must both be [NL,N,3], not {starts.shape} and {ends.shape}")
        lm_idx, v_idx = select_rays(starts.shape[0], starts.shape[1], landmark_indices, view_indices)
        fs = np.ascontiguousarray(starts[np.ix_(lm_idx, v_idx)])
        fe = np.ascontiguousarray(ends[np.ix_(lm_idx, v_idx)])
        if clip_to_mesh and fs.size:
            fe, _ = HipEstimator3D(device=self.device).clip_rays_to_mesh(mesh, fs, fe)
        renderer = HipRenderer3D(n_views=1, device=self.device, verbose=False)
        nl = 0 if landmarks is None else len(np.asarray(landmarks).reshape(-1, 3))
        nr = fs.reshape(-1, 3).shape[0]
        folder = Path(screenshot_dir) if screenshot_dir else Path("visualization") / "ray_screenshots"
        stem = Path(obj_path or getattr(mesh, "path", None) or "mesh.obj").stem
        # (``images`` stays the device tensor [n,S,S,4] under the "device" encoder)
        self.images, paths = render_to_png(
            renderer, "ray_view", cfg.encoder, [folder / f"{stem}_rays_{i}.png" for i in range(len(np.reshape(cfg.poses, (-1, 3))))],
            mesh, landmarks, fs, fe, poses=cfg.poses, size=cfg.size, radius=cfg.landmark_radius, ray_radius=cfg.ray_radius,
            colors=np.tile(np.array([colour_byte(c) for c in cfg.landmark_color], np.uint8), (nl, 1)) if nl else None,
            ray_colors=np.tile(np.array([colour_byte(c) for c in cfg.ray_color], np.uint8), (nr, 1)) if nr else None)
        return paths
