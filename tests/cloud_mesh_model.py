"""The contract of a point cloud's triangulation ("Point clouds") restated in numpy: the checker of
mvlm_mesh_triangulate_points.  It shares nothing with mvlm_amd/csrc/cloud_mesh_math.h: the star is found by brute force over
whole arrays (every ordered pair against every third entry at once), the triangles by set membership.

Inputs: float32 points v, float32 normals n, the neighbour table N int32 [V,16] (ascending (d2, id), -1 unused; tests/
cloud_normals_model.py supplies brute-force ones).  All arithmetic float64, every sum of three products (a + b) + c.
  perturbed point  s = sqrt(least positive d2 of the row) / 256 (0 without one); x = ((p + 1) * 0x9E3779B1) mod 2^32, three rounds
                   of x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16, after each h = (x >> 8) / 2^23 - 1 and
                   u[c] = v[c] + h s.
  star of p        empty unless L2 = |n|^2 is finite and > 0 and the row has two entries other than p.  n^ = n / sqrt(L2), c the
                   least |n^_c| (lowest index on a tie), e1 = cross(n^, axis_c) / its length, e2 = cross(n^, e1); per entry m != p:
                   d = u_m - u_p, q = (d . e1, d . e2), r2 = qx qx + qy qy, dropped when r2 == 0, w = q / r2.  {a, b} is in the star
                   iff in one order cross2(w_a, w_b) > 0 and (w_b - w_a) x (w_c - w_a) > 0 for every other kept c.
  triangle         i < j < k with {j,k} in S(i), {i,k} in S(j), {i,j} in S(k) and |cross(v_j - v_i, v_k - v_i)|^2 * 1024 > (largest
                   squared edge)^2 on the unperturbed points.  Rows ascending."""
import numpy as np

K = 16
MASK = 0xFFFFFFFF


def _f64(a):
    return np.asarray(a, np.float32).reshape(-1, 3).astype(np.float64)


def _dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2 over the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def hash_units(p: int):
    """the three numbers in [-1, 1) of point p"""
    x = ((p + 1) * 0x9E3779B1) & MASK
    out = []
    for _ in range(3):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & MASK
        x ^= x >> 15
        x = (x * 0x846CA68B) & MASK
        x ^= x >> 16
        out.append(float(x >> 8) / 8388608.0 - 1.0)
    return out


def perturbed(verts, table) -> np.ndarray:
    v = _f64(verts)
    u = v.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(len(v)):
            row = table[p][table[p] >= 0]
            d = v[row] - v[p]
            d2 = _dot3(d, d)
            pos = d2[d2 > 0.0]
            s = float(np.sqrt(pos.min())) * 0.00390625 if len(pos) else 0.0
            u[p] = v[p] + np.array(hash_units(p)) * s
    return u


def star(p: int, u, normals, table) -> set:
    """the pairs (lower id, higher id) of S(p)"""
    n = np.asarray(normals, np.float32).reshape(-1, 3)[p].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        L2 = float(_dot3(n, n))
        if not np.isfinite(L2) or not L2 > 0.0:
            return set()
        ids = np.array([m for m in table[p] if m >= 0 and m != p], np.int64)
        if len(ids) < 2:
            return set()
        nh = n / np.sqrt(L2)
        axis = np.zeros(3)
        axis[int(np.argmin(np.abs(nh)))] = 1.0          # (argmin: the first of equal values)
        e1 = _cross3(nh, axis)
        e1 = e1 / np.sqrt(_dot3(e1, e1))
        e2 = _cross3(nh, e1)
        d = u[ids] - u[p]
        qx, qy = _dot3(d, e1), _dot3(d, e2)
        r2 = qx * qx + qy * qy
        keep = ~(r2 == 0.0)
        ids, wx, wy = ids[keep], (qx / r2)[keep], (qy / r2)[keep]
        m = len(ids)
        turn = wx[:, None] * wy[None, :] - wy[:, None] * wx[None, :] > 0.0                             # [a, b]
        left = ((wx[None, :, None] - wx[:, None, None]) * (wy[None, None, :] - wy[:, None, None])
                - (wy[None, :, None] - wy[:, None, None]) * (wx[None, None, :] - wx[:, None, None])) > 0.0   # [a, b, c]
    idx = np.arange(m)
    third = (idx[None, None, :] != idx[:, None, None]) & (idx[None, None, :] != idx[None, :, None])      # c is neither a nor b
    ok = turn & (left | ~third).all(axis=2) & (idx[:, None] != idx[None, :])
    return {(int(min(ids[a], ids[b])), int(max(ids[a], ids[b]))) for a, b in zip(*np.nonzero(ok))}


def not_sliver(v, i, j, k) -> bool:
    a, b, c = v[j] - v[i], v[k] - v[i], v[k] - v[j]
    x = _cross3(a, b)
    longest = max(float(_dot3(a, a)), float(_dot3(b, b)), float(_dot3(c, c)))
    return bool(float(_dot3(x, x)) * 1024.0 > longest * longest)


def stars(verts, normals, table) -> list:
    u = perturbed(verts, table)
    return [star(p, u, normals, table) for p in range(len(u))]


def triangulate(verts, normals, table) -> np.ndarray:
    """-> int32 [T,3], rows (i, j, k) with i < j < k in ascending order"""
    v = _f64(verts)
    table = np.asarray(table)
    s = stars(verts, normals, table)
    assert all(len(x) <= 16 for x in s)
    rows = []
    for i in range(len(v)):
        for j, k in s[i]:
            if i < j and (i, k) in s[j] and (i, j) in s[k] and not_sliver(v, i, j, k):
                rows.append((i, j, k))
    return np.array(sorted(rows), np.int32).reshape(-1, 3)


# ---- what the tests measure on a triangle list --------------------------------------------------------------------------------
def area(verts, tris) -> float:
    v = _f64(verts)
    t = np.asarray(tris).reshape(-1, 3)
    x = _cross3(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return float(0.5 * np.sqrt(_dot3(x, x)).sum())


def edge_uses(tris) -> np.ndarray:
    """how many triangles every edge of the list is in"""
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]]), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return n


# ---- the clouds the tests share -----------------------------------------------------------------------------------------------
def tilt(points, rx=25.0, ry=-35.0, rz=15.0) -> np.ndarray:
    """a cloud turned out of the axes (float64 rotation, rounded to float32 once)"""
    a, b, c = np.deg2rad([rx, ry, rz])
    mx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    my = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    mz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return (np.asarray(points, np.float64) @ (my @ mx @ mz).T).astype(np.float32)


def exact_tilt(points) -> np.ndarray:
    """a rotation with rational entries, Rx(5-12-13) Rz(3-4-5) = M / 65 with M integer, of points that are whole multiples of
    65/16 (a grid of step 8.125 about its centre): every coordinate is a whole number of sixteenths, a float32 without any rounding"""
    rz5 = np.array([[3, -4, 0], [4, 3, 0], [0, 0, 5]], np.float64)
    rx13 = np.array([[13, 0, 0], [0, 5, -12], [0, 12, 5]], np.float64)
    k = np.rint(np.asarray(points, np.float64) / 4.0625)
    assert np.array_equal(k * 4.0625, np.asarray(points, np.float64)) and np.abs(k).max() < 1e4
    out = (k @ (rx13 @ rz5).T) / 16.0           # whole numbers all the way: exact
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def flat_grid(nx=21, ny=21, step=10.0) -> np.ndarray:
    x, y = np.meshgrid(np.arange(nx) * step - (nx - 1) * step / 2.0, np.arange(ny) * step - (ny - 1) * step / 2.0)
    return np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny)], axis=1).astype(np.float32)


def jittered(verts, amount=2.5, seed=4) -> np.ndarray:
    v = np.asarray(verts, np.float32).copy()
    v[:, :2] += np.random.RandomState(seed).uniform(-amount, amount, size=(len(v), 2)).astype(np.float32)
    return v


def duplicates_and_nan(seed=6) -> np.ndarray:
    """200 points on a bumpy sheet, five of them again, and one NaN point in the middle of the file"""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(-80, 80, size=(200, 2))
    z = 10.0 * np.sin(xy[:, 0] / 40.0) * np.cos(xy[:, 1] / 50.0)
    v = np.column_stack([xy, z]).astype(np.float32)
    v = np.concatenate([v[:100], [[np.nan, 0.0, 0.0]], v[100:], v[[3, 50, 120, 150, 199]]]).astype(np.float32)
    return v
