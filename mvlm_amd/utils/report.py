"""Per-landmark quality report of one prediction (``Pipeline(..., landmark_report=True)`` -> ``pipe.last_report``).

What the consensus (mvlm_amd/csrc/report.hip) and the snap (surface_attach.hip) know about every landmark and the plain
pipeline drops: surviving views, inliers of the one-shot draw, the branch of the reference's RANSAC that produced the point,
the spread of the rays around it, how far the snap moved it and where on the mesh it landed.

COORDINATES.  Every length of the report (``raw``, ``rms``, ``max_dist``, ``sigma``, ``sigma2``, ``cov``, ``view_dist2``,
``snap_dist``) is in the space the network sees: the pre-aligned model space, where the consensus's inlier threshold of
100 (10 units squared, estimator3d.py:97) lives.  Only ``landmarks`` is mapped back to the file's coordinates, as the
pipeline's return value is.  Without a pre-align block the two spaces are the same.

This module is host-side numpy only: the device buffer of a report is ONE byte range (``ReportLayout``), fetched with one
copy and cut into arrays here.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

__all__ = ["LandmarkReport", "ReportLayout", "ResultPack", "CSV_HEADER", "texel"]

N_STATS = 9  # MVLM_REPORT_STATS: rms, max_dist, sigma2, cov xx yy zz xy xz yz
VIEW_KEPT, VIEW_DRAWN, VIEW_INLIER, VIEW_USED = 1, 2, 4, 8  # MVLM_VIEW_* (include/mvlm_hip.h)
# the ray view's colours by what the consensus did with a view's ray (LandmarkReport.ray_colours)
RAY_USED, RAY_KEPT, RAY_FILTERED = (26, 230, 26), (255, 165, 0), (160, 160, 160)
CSV_HEADER = "index,x,y,z,n_kept,n_inliers,n_used,branch,error,rms,sigma,snap_dist,tri,b0,b1,b2,u,v"


def _device_views(fields: dict, buf) -> dict:
    """{name: (offset, bytes, dtype, shape)} over a uint8 device tensor -> {name: typed tensor view} (no copies)."""
    import torch

    kinds = {"f8": torch.float64, "i4": torch.int32, "f4": torch.float32, "u1": torch.uint8}
    views = {}
    for name, (off, nb, dt, shape) in fields.items():
        flat = buf[off: off + nb].view(kinds[dt.str[1:]])
        views[name] = flat if len(shape) == 1 else flat.view(shape)  # (on the hot path: no second view where [NL] is the shape)
    return views


class ReportLayout:
    """Byte offsets of a report's arrays in one buffer for NL landmarks and N views: float64 first, then the 4-byte
    and the 1-byte arrays, so every array is aligned to its element size."""

    FIELDS = (("raw", "f8", (3,), False), ("error", "f8", (), False), ("stats", "f8", (N_STATS,), False),
              ("snapped", "f8", (3,), False), ("bary", "f8", (3,), False), ("uv", "f8", (2,), False),
              ("view_dist2", "f8", (), True), ("counts", "i4", (4,), False), ("tri", "i4", (), False),
              ("scores", "f4", (), True), ("view_flags", "u1", (), True))

    def __init__(self, n_landmarks: int, n_views: int):
        self.nl, self.n = int(n_landmarks), int(n_views)
        self.fields, off = {}, 0
        for name, dt, tail, per_view in self.FIELDS:
            shape = (self.nl,) + ((self.n,) if per_view else ()) + tail
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            self.fields[name] = (off, nbytes, np.dtype(dt), shape)
            off += nbytes
        self.nbytes = (off + 7) // 8 * 8

    def device_views(self, buf) -> dict:
        """uint8 device tensor (8-byte aligned, at least ``nbytes`` long) -> {name: typed tensor view}."""
        return _device_views(self.fields, buf)

    def host_arrays(self, host: np.ndarray) -> dict:
        """The fetched bytes -> {name: array} (copies: the staging buffer is reused by the next call)."""
        return {name: host[off: off + nb].view(dt).reshape(shape).copy() for name, (off, nb, dt, shape) in self.fields.items()}


class ResultPack:
    """Byte offsets of a prediction's result buffer for NL landmarks: ``snapped`` f64 [NL,3] | ``error`` f64 [NL] | ``counts``
    i32 [NL] (the survivors the RANSAC draws were made for), rounded up to 8 bytes: ``nbytes``, which is also a scan's stride
    when several scans share one buffer.  With ``n_views`` a report for that many views rides behind it in the same buffer and
    the same copy: ``report`` (a ``ReportLayout``) starts at ``nbytes``, and ``total`` covers both."""

    FIELDS = (("snapped", np.dtype("f8"), 3), ("error", np.dtype("f8"), 1), ("counts", np.dtype("i4"), 1))

    def __init__(self, n_landmarks: int, n_views: int | None = None):
        self.nl = int(n_landmarks)
        self.fields, off = {}, 0
        for name, dt, width in self.FIELDS:
            nbytes = self.nl * width * dt.itemsize
            self.fields[name] = (off, nbytes, dt, (self.nl, width) if width > 1 else (self.nl,))
            off += nbytes
        self.nbytes = (off + 7) // 8 * 8
        self.report = None if n_views is None else ReportLayout(self.nl, n_views)
        self.total = self.nbytes + (0 if self.report is None else self.report.nbytes)

    def device_views(self, buf) -> dict:
        """uint8 device tensor (8-byte aligned, at least ``nbytes`` long) -> {name: typed tensor view}."""
        return _device_views(self.fields, buf)

    def host_views(self, host: np.ndarray) -> dict:
        """The fetched bytes -> {name: array view}.  Views, not copies: the staging buffer is reused by the next call, so what a
        caller keeps of them it copies."""
        return {name: np.ndarray(shape, dt, host, off) for name, (off, nb, dt, shape) in self.fields.items()}

    def report_bytes(self, buf):
        """The byte range of ``buf`` (device tensor or fetched array) that holds the report."""
        return buf[self.nbytes: self.total]


def texel(u, v, tex_w: int, tex_h: int):
    """The rasteriser's nearest-texel convention (rm_texel, mvlm_amd/csrc/raster_math.h) in numpy: float32 arithmetic,
    GL_REPEAT wrapping, v = 0 at the bottom row of an image stored top row first.  -> (column, row) int arrays, -1 where
    u or v is NaN."""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    bad = np.isnan(u) | np.isnan(v)
    u, v = np.where(bad, np.float32(0), u), np.where(bad, np.float32(0), v)
    uu, vv = u - np.floor(u), v - np.floor(v)
    tx = np.clip((uu * np.float32(tex_w)).astype(np.int64), 0, tex_w - 1)
    ty = np.clip((vv * np.float32(tex_h)).astype(np.int64), 0, tex_h - 1)
    return np.where(bad, -1, tx), np.where(bad, -1, tex_h - 1 - ty)


# The landmark view (Pipeline(visualize_img=True)) colours a landmark's sphere by the branch of its report: refitted on its
# inliers (1) blue, fallback to all lines (2) orange, fewer than three lines (0) red.
BRANCH_COLOURS = {1: (0, 0, 255), 2: (255, 165, 0), 0: (255, 0, 0)}


class LandmarkReport:
    """See the module docstring for the coordinate spaces.  NL landmarks, N views (those that remained after a
    detector's ``valid`` mask: ``view_indices`` names them in the pose table).

    landmarks [NL,3]   as returned by the pipeline (file coordinates)      raw [NL,3]        the consensus point, pre-snap
    n_kept [NL]        views that survived the score filter               n_inliers [NL]    inliers of the 8-draw sample fit
    n_used [NL]        lines of the final fit                             branch [NL]       0 fewer than 3 lines, plain least squares;
                                                                                            1 refit on the inliers; 2 "RANSAC failed",
                                                                                            all lines, error 1e8
    error [NL]         the landmark's term of ``last_error``               rms, max_dist     ray distances of the used lines to raw
    sigma2 [NL]        sum d2 / (2 n_used - 3)                             cov [NL,3,3]      sigma2 pinv(sum (I - n n^T))
    sigma [NL]         sqrt of cov's largest eigenvalue                   snap_dist [NL]    |snapped - raw|
    tri [NL]           triangle the snap chose (-1: none)                 bary [NL,3], uv [NL,2]
    scores [NL,N]      heatmap maxima' values                             view_dist2 [NL,N] squared ray distance to raw, all views
    view_flags [NL,N]  VIEW_KEPT | VIEW_DRAWN | VIEW_INLIER | VIEW_USED    view_indices [N]
    """

    VIEW_KEPT, VIEW_DRAWN, VIEW_INLIER, VIEW_USED = VIEW_KEPT, VIEW_DRAWN, VIEW_INLIER, VIEW_USED

    def branch_colours(self) -> np.ndarray:
        """uint8 [NL,3]: ``BRANCH_COLOURS`` of every landmark's branch (the sphere colours of the landmark view)."""
        table = np.array([BRANCH_COLOURS[b] for b in (0, 1, 2)], np.uint8)
        return table[np.clip(np.asarray(self.branch, np.int64), 0, 2)]

    def ray_colours(self, views=None) -> np.ndarray:
        """uint8 [NL,len(views),3]: a colour per view ray (the ray view, Pipeline(visualize_rays_img=True)) - ``RAY_USED`` green
        for a line of the final fit (``VIEW_USED``), ``RAY_KEPT`` orange for one that survived the score filter but was not
        used, ``RAY_FILTERED`` grey for one filtered out.  ``views``: view numbers as ``view_indices`` lists them (default:
        all of them, in that order); a view the report does not hold raises."""
        cols = np.arange(self.view_flags.shape[1])
        if views is not None:
            where = {int(v): j for j, v in enumerate(np.asarray(self.view_indices))}
            missing = [int(v) for v in np.asarray(views).ravel() if int(v) not in where]
            if missing:
                raise ValueError(f"views {missing} are not among the report's view_indices")
            cols = np.array([where[int(v)] for v in np.asarray(views).ravel()], dtype=np.int64)
        flags = np.asarray(self.view_flags)[:, cols]
        out = np.empty(flags.shape + (3,), np.uint8)
        out[...] = RAY_FILTERED
        out[(flags & VIEW_KEPT) != 0] = RAY_KEPT
        out[(flags & VIEW_USED) != 0] = RAY_USED
        return out

    def __init__(self, arrays: dict, landmarks=None, view_indices=None):
        a = arrays
        self.raw, self.error = a["raw"], a["error"]
        self.snapped = a["snapped"]  # model space; ``landmarks`` is this mapped back to the file's coordinates
        self.landmarks = np.array(self.snapped if landmarks is None else landmarks, dtype=np.float64)
        counts, st = a["counts"], a["stats"]
        self.n_kept, self.n_inliers, self.n_used, self.branch = (np.ascontiguousarray(counts[:, j]) for j in range(4))
        self.rms, self.max_dist, self.sigma2 = (np.ascontiguousarray(st[:, j]) for j in range(3))
        self.cov = st[:, [3, 6, 7, 6, 4, 8, 7, 8, 5]].reshape(-1, 3, 3)
        self.sigma = np.full(len(st), np.nan)
        ok = np.isfinite(self.cov).all(axis=(1, 2))
        if ok.any():
            self.sigma[ok] = np.sqrt(np.maximum(np.linalg.eigvalsh(self.cov[ok])[:, -1], 0.0))
        self.snap_dist = np.sqrt(((self.snapped - self.raw) ** 2).sum(axis=1))
        self.tri, self.bary, self.uv = a["tri"], a["bary"], a["uv"]
        self.scores, self.view_dist2, self.view_flags = a["scores"], a["view_dist2"], a["view_flags"]
        n = self.view_flags.shape[1]
        self.view_indices = np.arange(n) if view_indices is None else np.asarray(view_indices, dtype=np.int64)

    def __len__(self) -> int:
        return len(self.raw)

    def texture_pixel(self, tex_w: int, tex_h: int) -> np.ndarray:
        """[NL,2] int (column, row) of the texel the rasteriser would read at every landmark's ``uv``; -1 where uv is NaN."""
        tx, ty = texel(self.uv[:, 0], self.uv[:, 1], int(tex_w), int(tex_h))
        return np.stack([tx, ty], axis=1)

    def rows(self) -> np.ndarray:
        """[NL,18] float64 in the column order of ``CSV_HEADER``."""
        cols = [np.arange(len(self)), *self.landmarks.T, self.n_kept, self.n_inliers, self.n_used, self.branch, self.error,
                self.rms, self.sigma, self.snap_dist, self.tri, *self.bary.T, *self.uv.T]
        return np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1)

    def to_csv(self, path) -> Path:
        """One row per landmark under ``CSV_HEADER``; floats with 17 significant digits (they read back exactly), NaN as nan."""
        ints = {0, 4, 5, 6, 7, 12}
        lines = [CSV_HEADER]
        for row in self.rows():
            lines.append(",".join(str(int(x)) if j in ints else repr(float(x)) for j, x in enumerate(row)))
        path = Path(path)
        path.write_text("\n".join(lines) + "\n")
        return path
