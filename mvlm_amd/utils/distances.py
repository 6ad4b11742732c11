"""Distances between the landmarks of one prediction (``HipRenderer3D.landmark_geodesics``; ``Pipeline(..., landmark_distances=True)``
-> ``pipe.last_distances``): the straight distance and the distance along the scan's triangles - the "tape-measure" distance of
facial anthropometry.  The surface distance is the first-order fast-marching discretisation iterated to its fixed point
(csrc/geodesic_math.h, DESIGN.md 5.1 "Surface distances"), not an exact polyhedral geodesic: it overestimates by a few per cent.
It is computed in both directions; ``geodesic`` is their mean and ``asymmetry`` their difference, which says how far to trust it."""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np

CSV_COLUMNS = ("i", "j", "euclidean", "geodesic", "geodesic_ij", "geodesic_ji")


def check_pairs(pairs, n: int | None = None, label: str = "distance_pairs"):
    """``pairs`` -> int32 [m,2] or None (all pairs).  ValueError for anything that is not a sequence of (i, j) with integers
    i != j, and - when ``n`` is known - inside 0..n-1."""
    if pairs is None:
        return None
    try:
        arr = np.asarray(pairs)
    except (TypeError, ValueError):
        raise ValueError(f"{label} must be None or a sequence of (i, j) landmark indices, not {pairs!r}") from None
    if arr.size == 0:
        raise ValueError(f"{label} must be None or name at least one pair")
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{label} must be None or a sequence of (i, j) landmark indices, not {pairs!r}")
    if (arr[:, 0] == arr[:, 1]).any():
        raise ValueError(f"{label}: a pair needs two different landmarks, not {pairs!r}")
    if (arr < 0).any() or (n is not None and (arr >= n).any()):
        upper = "" if n is None else f"..{n - 1}"
        raise ValueError(f"{label}: landmark indices must lie in 0{upper}, not {pairs!r}")
    return np.ascontiguousarray(arr, dtype=np.int32)


def parse_pairs(text: str):
    """The command line's ``--distance-pairs 0-16,8-27`` -> [(0, 16), (8, 27)]."""
    out = []
    for item in str(text).split(","):
        parts = item.strip().split("-")
        if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
            raise ValueError(f"--distance-pairs takes pairs like 0-16,8-27, not {text!r}")
        out.append((int(parts[0]), int(parts[1])))
    return out


@dataclass
class LandmarkDistances:
    """``snapped`` f64[n,3] and ``tri`` i32[n]: the landmarks on the surface and their triangles (-1: none); ``euclidean`` f64[n,n];
    ``directed`` f64[n,n]: [i,j] from source i to target j; ``geodesic``: the mean of the two directions; ``asymmetry``: their
    absolute difference; ``sweeps`` i32[n]: per source the first sweep that changed nothing (-1: no field).  NaN: a landmark that is
    not attached, or - with ``pairs`` - an entry that was not asked for; inf: another connected component.  ``fields``: with
    ``return_fields`` the distance fields f64[n,V] as a device tensor, else None.  Lengths are in the space the mesh was uploaded
    in, divided by ``scale`` (a pre-align block's) where one is given."""
    snapped: np.ndarray
    tri: np.ndarray
    euclidean: np.ndarray
    directed: np.ndarray
    sweeps: np.ndarray
    pairs: np.ndarray | None = None
    fields: object = None

    @property
    def geodesic(self) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return 0.5 * (self.directed + self.directed.T)

    @property
    def asymmetry(self) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return np.abs(self.directed - self.directed.T)

    def scaled(self, scale: float) -> "LandmarkDistances":
        """The same with every length divided by ``scale``: a scan that was pre-aligned with a scale, in its own units again.
        (``snapped`` stays in the space of the mesh; ``fields`` are dropped.)"""
        s = float(scale)
        return LandmarkDistances(self.snapped, self.tri, self.euclidean / s, self.directed / s, self.sweeps, self.pairs, None)

    def rows(self):
        """(i, j, euclidean, geodesic, geodesic_ij, geodesic_ji) per pair i < j: the listed pairs (each once, in ascending order),
        else all."""
        n = int(self.directed.shape[0])
        if self.pairs is None:
            todo = [(i, j) for i in range(n) for j in range(i + 1, n)]
        else:
            todo = sorted({(int(min(a, b)), int(max(a, b))) for a, b in np.asarray(self.pairs).reshape(-1, 2)})
        geo = self.geodesic
        return [(i, j, float(self.euclidean[i, j]), float(geo[i, j]), float(self.directed[i, j]), float(self.directed[j, i])) for i, j in todo]

    def to_csv(self, path) -> Path:
        """One row per pair i < j; ``inf`` and ``nan`` are written as such."""
        path = Path(path)
        with open(path, "w") as f:
            f.write(",".join(CSV_COLUMNS) + "\n")
            for i, j, *values in self.rows():
                f.write(f"{i},{j}," + ",".join(_number(v) for v in values) + "\n")
        return path


def _number(v: float) -> str:
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "inf" if v > 0 else "-inf"
    return repr(float(v))
