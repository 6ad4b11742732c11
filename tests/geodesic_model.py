"""The surface distances between landmarks, stated a second time in numpy (test infrastructure): the rule of
mvlm_amd/csrc/geodesic_math.h without including it.  The kernels (tests/test_gpu_geodesics.py) and the header compiled for the host
(tests/native/geodesic_host.cpp, tests/test_geodesic_cpu.py) must equal ``geodesics`` bit for bit.

The rule.  float64 throughout; a vertex is its float32 coordinates widened; a sum of three products is (a + b) + c; numpy's
elementwise + - * / sqrt are IEEE, and nothing here goes through dot, einsum or norm.
  valid triangle   indices in [0, V), nine finite coordinates; every other triangle is ignored everywhere.  A landmark is attached
                   iff its triangle is valid and its point finite; else its row and column of D are NaN and it has no field.
  frame(A, B, C)   c = |B - A|, lac = |C - A|, lbc = |C - B|; with c > 0: px = (C - A).(B - A) / c, py = sqrt(max(|C - A|^2 - px^2, 0))
  u(da, db, frame) min(da + lac, db + lbc) and, iff da, db finite, c > 0, py > 0, |k| < 1 with k = (db - da) / c, and
                   0 < s < c with w = sqrt(1 - k k), s = px - (k py) / w:  (da + k px) + py w
  corner's edge    triangle (i0, i1, i2): i0 reads (i1, i2), i1 reads (i2, i0), i2 reads (i0, i1)
  initial set      the source triangle's corners, widened ``init_rings`` times by every valid triangle that touches the set;
                   d = |V - P| there, +inf elsewhere
  sweep            new[v] = min(old[v], u over v's incidences), all reads of old; until a sweep changes nothing - its index is sweeps[i]
  target           min of u over the three edges of the target's triangle with C = the target's point; |P_i - P_j| too when both
                   lie in one triangle; 0 on the diagonal

Fixture builders: ``grid`` (one diagonal per cell, optionally stretched and jittered), ``strip``, ``folded_sheet``, ``icosphere``,
``two_components``; ``plant`` puts landmarks into triangles by barycentric weights."""
from __future__ import annotations

import numpy as np


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def dist(a, b):
    d = a - b
    return np.sqrt(_dot(d, d))


def frame(A, B, C):
    ab, ac, bc = B - A, C - A, C - B
    ac2 = _dot(ac, ac)
    c = np.sqrt(_dot(ab, ab))
    lac, lbc = np.sqrt(ac2), np.sqrt(_dot(bc, bc))
    with np.errstate(all="ignore"):
        px = np.where(c > 0.0, _dot(ac, ab) / c, 0.0)
        h2 = ac2 - px * px
        py = np.where(c > 0.0, np.sqrt(np.where(h2 > 0.0, h2, 0.0)), 0.0)
    return lac, lbc, c, px, py


def update(da, db, fr):
    lac, lbc, c, px, py = fr
    best = np.minimum(da + lac, db + lbc)
    with np.errstate(all="ignore"):
        k = (db - da) / c
        w = np.sqrt(1.0 - k * k)
        s = px - (k * py) / w
        interior = (da + k * px) + py * w
        counts = np.isfinite(da) & np.isfinite(db) & (c > 0.0) & (py > 0.0) & (np.abs(k) < 1.0) & (s > 0.0) & (s < c)
    return np.where(counts & (interior < best), interior, best)


def valid_triangles(verts, tris):
    V = verts.shape[0]
    inside = ((tris >= 0) & (tris < V)).all(axis=1)
    ok = inside.copy()
    finite = np.isfinite(verts).all(axis=1)
    ok[inside] = finite[tris[inside]].all(axis=1)
    return ok


class NotSettled(RuntimeError):
    def __init__(self, source):
        super().__init__(f"source landmark {source} did not settle")
        self.source = source


def geodesics(verts, tris, snapped, tri, init_rings=2, max_sweeps=4096, pairs=None):
    """-> (D f64[n,n], E f64[n,n], sweeps i32[n], fields f64[n,V]).  ``snapped`` f64[n,3] and ``tri`` i32[n]: the attachment.
    With ``pairs`` only the landmarks named get a field and only D[i,j], D[j,i] of a pair are computed; the rest is NaN / -1."""
    v64 = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    P = np.asarray(snapped, np.float64).reshape(-1, 3)
    tri = np.asarray(tri, np.int32).reshape(-1)
    V, T, n = v64.shape[0], tris.shape[0], P.shape[0]
    valid = valid_triangles(v64, tris)
    vt = tris[valid]
    with np.errstate(invalid="ignore"):
        E = dist(P[:, None, :], P[None, :, :])
    ok = np.array([0 <= tri[i] < T and bool(valid[tri[i]]) and bool(np.isfinite(P[i]).all()) for i in range(n)])
    # incidences: (corner, A, B)
    inc_c = np.concatenate([vt[:, 0], vt[:, 1], vt[:, 2]])
    inc_a = np.concatenate([vt[:, 1], vt[:, 2], vt[:, 0]])
    inc_b = np.concatenate([vt[:, 2], vt[:, 0], vt[:, 1]])
    fr = frame(v64[inc_a], v64[inc_b], v64[inc_c])
    order = np.argsort(inc_c, kind="stable")
    firsts = np.nonzero(np.diff(inc_c[order], prepend=-1))[0]
    owners = inc_c[order][firsts]
    D = np.full((n, n), np.nan)
    sweeps = np.full(n, -1, np.int32)
    fields = np.full((n, V), np.nan)
    if pairs is None:
        sources = list(range(n))
        wanted = None
    else:
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        sources = sorted(set(pairs.ravel().tolist()))
        wanted = {(int(a), int(b)) for a, b in pairs} | {(int(b), int(a)) for a, b in pairs}
    for i in sources:
        if not ok[i]:
            continue
        inside = np.zeros(V, bool)
        inside[tris[tri[i]]] = True
        for _ in range(init_rings):
            touched = inside[vt].any(axis=1)
            inside = inside.copy()
            inside[vt[touched].ravel()] = True
        d = np.where(inside, dist(v64, P[i][None, :]), np.inf)
        k = 0
        while True:
            if k == max_sweeps:
                raise NotSettled(i)
            u = update(d[inc_a], d[inc_b], fr)
            new = d.copy()
            if u.size:
                new[owners] = np.minimum(d[owners], np.minimum.reduceat(u[order], firsts))
            changed = bool((new != d).any())
            d = new
            if not changed:
                break
            k += 1
        sweeps[i] = k
        fields[i] = d
        for j in range(n):
            if not ok[j] or (wanted is not None and (i, j) not in wanted):
                continue
            if i == j:
                D[i, j] = 0.0
                continue
            idx = tris[tri[j]]
            a, b = idx[[1, 2, 0]], idx[[2, 0, 1]]
            out = update(d[a], d[b], frame(v64[a], v64[b], P[j][None, :])).min()
            if tri[i] == tri[j]:
                out = min(out, E[i, j])
            D[i, j] = out
    return D, E, sweeps, fields


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def grid(nx, ny, sx=1.0, sy=1.0, jitter=0.0, seed=0):
    """nx x ny vertices at (x sx, y sy, 0), one diagonal per cell (the same way everywhere); vertex id = y * nx + x.
    ``jitter``: every vertex moved in the plane by up to that share of a cell."""
    y, x = np.mgrid[0:ny, 0:nx]
    verts = np.stack([x.ravel() * sx, y.ravel() * sy, np.zeros(nx * ny)], axis=1)
    if jitter:
        rs = np.random.RandomState(seed)
        verts[:, 0] += rs.uniform(-jitter, jitter, nx * ny) * sx
        verts[:, 1] += rs.uniform(-jitter, jitter, nx * ny) * sy
    v00 = (y[:-1, :-1] * nx + x[:-1, :-1]).ravel()
    tris = np.concatenate([np.stack([v00, v00 + 1, v00 + nx + 1], axis=1), np.stack([v00, v00 + nx + 1, v00 + nx], axis=1)])
    return verts.astype(np.float32), tris.astype(np.int32)


def strip(n):
    """2 x n vertices: a field needs about n sweeps to cross it"""
    return grid(n, 2)


def folded_sheet(nx=17, ny=33, fold=8):
    """(flat, folded): an integer grid and the same folded by 90 degrees along the grid line x = fold - an isometry"""
    verts, tris = grid(nx, ny)
    folded = verts.copy()
    over = verts[:, 0] > fold
    folded[over, 2] = verts[over, 0] - fold
    folded[over, 0] = fold
    return (verts, tris), (folded, tris)


def icosphere(subdivisions, radius=100.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
             (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(v, float) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return (np.array(verts) * radius).astype(np.float32), np.array(faces, np.int32)


def two_components(n=5, gap=50.0):
    """two n x n grids that share nothing"""
    v, t = grid(n, n)
    v2 = v.copy()
    v2[:, 0] += gap
    return np.concatenate([v, v2]), np.concatenate([t, t + v.shape[0]]).astype(np.int32)


def plant(verts, tris, tri_ids, weights):
    """landmarks inside the named triangles: -> (points f64[n,3], tri i32[n])"""
    v64 = np.asarray(verts, np.float32).astype(np.float64)
    tri_ids = np.asarray(tri_ids, np.int32)
    w = np.asarray(weights, np.float64).reshape(-1, 3)
    c = v64[np.asarray(tris)[tri_ids]]  # [n,3,3]
    return (c * w[:, :, None]).sum(axis=1), tri_ids


def spread(verts, tris, n, seed=0):
    """n landmarks in triangles drawn with a fixed seed, well inside them"""
    rs = np.random.RandomState(seed)
    ids = rs.randint(0, len(tris), n)
    w = rs.uniform(0.2, 1.0, (n, 3))
    w /= w.sum(axis=1, keepdims=True)
    return plant(verts, tris, ids, w)
