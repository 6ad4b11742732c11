"""Offscreen landmark view: the reference's ``VTKViewer(filename, landmarks, pname, save=True)`` (utils/viewer.py, main.py:66-67)
drawn by the HIP rasteriser (mvlm_render_landmark_view) instead of a VTK window.

``LandmarkViewer`` keeps ``VTKViewer``'s signature for the offscreen case: it loads the file, draws the front view with a blue
sphere at every landmark and writes ``visualization/<stem>[_<pname>].png`` relative to the working directory.  The interactive
window (``save=False``, ``--visualize-iter``) is out of scope.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

__all__ = ["LandmarkViewer", "view_path", "write_view_png"]


def view_path(filename, pname: str | None = None) -> Path:
    """``visualization/<stem>[_<pname>].png`` relative to the working directory (viewer.py:89-92)."""
    suffix = f"_{pname}" if pname else ""
    return Path("visualization") / f"{Path(filename).stem}{suffix}.png"


def write_view_png(image: np.ndarray, out_path: Path) -> Path:
    """uint8 [S,S,3] -> PNG through Pillow (as Pipeline.visualize_image_stack); makes the folder (viewer.py:93)."""
    from PIL import Image

    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8)).save(out_path)
    return out_path


class LandmarkViewer:
    def __init__(self, filename, landmarks: np.ndarray | None = None, pname: str | None = None, save: bool = True,
                 size: int = 1024, device: int = 0) -> None:
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
        self.image = renderer.render_landmark_view(mesh, landmarks, size=self.size)[0]
        self.out_path = write_view_png(self.image, view_path(self.filename, pname))
