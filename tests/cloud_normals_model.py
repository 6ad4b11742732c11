"""The contract of a point cloud's normals ("Point clouds") restated in numpy: the checker of the neighbour
search, of the estimated normals and of the geometry shade of the splats.  It shares nothing with
mvlm_amd/csrc/cloud_normals_math.h: the search is brute force, the eigenvector numpy.linalg.eigh's.

Neighbourhood of a finite point p: the 16 finite points of least (d2, id), p included, d2 = (dx dx + dy dy) + dz dz in float64 from
the float32 coordinates; all of them when there are fewer.  A row lists them in ascending (d2, id), unused slots -1; a non-finite
point is in no row and its own row is all -1.  Normal: the unit eigenvector of the least eigenvalue of the neighbourhood's 3 x 3
covariance about its centroid, float64; (0, 0, 0) for a non-finite point, fewer than 3 neighbours, a zero covariance; the sign is
unspecified.  Shade of a splat whose point has the float32 normal n, under the rotation M: (int)(|nz| / len * 255 + 0.5) with
nz = (M[6] n.x + M[7] n.y) + M[8] n.z and len = sqrt((n.x n.x + n.y n.y) + n.z n.z) in float64; 0 when len is 0 or not finite."""
import numpy as np

K = 16


def neighbors(verts) -> np.ndarray:
    """float32 [V,3] -> int32 [V,16], brute force."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    finite = np.isfinite(v).all(axis=1)
    ids = np.nonzero(finite)[0]
    good = v[finite]
    table = np.full((len(v), K), -1, np.int32)
    for p in ids:
        d = good - v[p]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((ids, d2))[:K]              # by d2, then by id
        table[p, :len(order)] = ids[order]
    return table


def covariance(verts, row) -> tuple:
    """(number of neighbours, 3 x 3 covariance about their centroid, float64) of one row of the table."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    q = v[row[row >= 0]]
    if len(q) == 0:
        return 0, np.zeros((3, 3))
    d = q - q.mean(axis=0)
    return len(q), d.T @ d / len(q)


def normals(verts, table=None) -> tuple:
    """-> (float64 [V,3] unit normals or (0,0,0), float64 [V,3] eigenvalues ascending (NaN where the normal is (0,0,0)))."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    table = neighbors(v) if table is None else table
    out, lam = np.zeros((len(v), 3)), np.full((len(v), 3), np.nan)
    for p in range(len(v)):
        n, c = covariance(v, table[p])
        if n < 3 or not c.any():
            continue
        w, vec = np.linalg.eigh(c)
        out[p], lam[p] = vec[:, 0], w
    return out, lam


def shade(normals_f32, m) -> np.ndarray:
    """float32 [V,3] normals, one rotation f64[9] -> int64 [V] shade bytes."""
    n = np.asarray(normals_f32, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nz = (m[6] * x + m[7] * y) + m[8] * z
        length = np.sqrt((x * x + y * y) + z * z)
        ok = np.isfinite(length) & (length > 0.0)
        s = np.where(ok, np.abs(nz) / np.where(ok, length, 1.0) * 255.0 + 0.5, 0.0)
    return np.where(ok, s, 0.0).astype(np.int64)


def render(verts, normals_f32, transform_stack, radius=None, subpixel_bits: int = 8) -> np.ndarray:
    """What render_device gives for the cloud under geometry shading: the splats of tests/points_model.render - the winner of every
    pixel read off a render whose colours spell the point ids - with planes 0..2 the winner's shade / 255."""
    import points_model as pm

    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    assert len(verts) < (1 << 24) - 1
    ids = np.arange(len(verts))
    codes = np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=1).astype(np.uint8)
    base = pm.render(verts, transform_stack, radius, codes, subpixel_bits)
    rot = pm.rotations(transform_stack)
    out = base.copy()
    far = np.float32(1.0) / np.float32(255.0)
    for k in range(len(base)):
        rgb = np.rint(base[k, :, :, :3] * 255.0).astype(np.int64)
        win = rgb[..., 0] | (rgb[..., 1] << 8) | (rgb[..., 2] << 16)
        # a background pixel is white (code 0xFFFFFF: no such id); a covered one carries an id
        covered = win != 0xFFFFFF
        s = shade(normals_f32, rot[k])
        plane = np.where(covered, s[np.where(covered, win, 0)], 255).astype(np.float32) / np.float32(255.0)
        out[k, :, :, 0] = out[k, :, :, 1] = out[k, :, :, 2] = plane
        assert (base[k, :, :, 3][~covered] == far).all()
    return out
