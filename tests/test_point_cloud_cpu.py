"""Point clouds without a GPU: the automatic splat radius of the library (a host function) against the model's rule, the
readers on files that have points and no faces, and what the contract itself promises - a grid cloud under its automatic
radius leaves no hole and its depth stays within the splat's reach of the plane the points lie on (tests/points_model.py
against the oracle's render of that plane as two triangles)."""
import ctypes as C
import math

import numpy as np
import pytest

import points_model as pm


def _lib_auto_radius(verts):
    from mvlm_amd import _lib

    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    r = C.c_double()
    assert _lib.load().mvlm_points_auto_radius(_lib.as_ptr(v, C.c_float), len(v), C.byref(r)) == 0
    return r.value


def _grid(n, spacing, z=0.0):
    lin = (np.arange(n) - (n - 1) / 2) * spacing
    x, y = np.meshgrid(lin, lin)
    return np.stack([x.ravel(), y.ravel(), np.full(n * n, z)], axis=1).astype(np.float32)


FLOOR, CEILING = 0.75 * 300.0 / 256.0, 8.0 * 300.0 / 256.0

AUTO_CASES = {
    "one point": np.array([[1.0, 2.0, 3.0]], np.float32),
    "collinear": np.stack([np.linspace(-50, 50, 30), np.zeros(30), np.zeros(30)], axis=1).astype(np.float32),
    "a NaN point": np.concatenate([_grid(40, 5.0), [[np.nan, 0.0, 0.0]], [[0.0, np.inf, 0.0]]]).astype(np.float32),
    "40 x 40, spacing 5": _grid(40, 5.0),
    "dense": _grid(300, 0.3),
    "sparse": _grid(5, 40.0),
}


@pytest.mark.parametrize("name", sorted(AUTO_CASES))
def test_auto_radius_is_the_models_rule(name):
    verts = AUTO_CASES[name]
    got, want = _lib_auto_radius(verts), pm.auto_radius(verts)
    assert got == want, (got, want)
    assert FLOOR <= got <= CEILING and pm.R_MIN <= pm.radius_steps(got) <= pm.R_MAX
    if name in ("one point", "collinear", "dense"):
        assert got == FLOOR and pm.radius_steps(got) == pm.R_MIN
    if name == "sparse":
        assert got == CEILING and pm.radius_steps(got) == pm.R_MAX
    if name == "40 x 40, spacing 5":
        s = math.sqrt(195.0 * 195.0 / 1600)
        assert got == 1.25 * s * 300.0 / 256.0 and FLOOR < got < CEILING
    if name == "a NaN point":  # the two non-finite points count for nothing: neither in the box nor in n
        assert got == pm.auto_radius(_grid(40, 5.0))


def test_auto_radius_refuses_nothing_to_measure():
    from mvlm_amd import _lib

    r = C.c_double()
    v = np.zeros((1, 3), np.float32)
    assert _lib.load().mvlm_points_auto_radius(_lib.as_ptr(v, C.c_float), 0, C.byref(r)) != 0
    assert _lib.load().mvlm_points_auto_radius(None, 1, C.byref(r)) != 0
    assert _lib_auto_radius(np.full((3, 3), np.nan, np.float32)) == FLOOR   # no finite point: the floor


def _write_ply(path, verts, colors, binary):
    n = len(verts)
    head = f"ply\nformat {'binary_little_endian' if binary else 'ascii'} 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
    if colors is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        if binary:
            fields = [("p", "<f4", 3)] + ([("c", "u1", 3)] if colors is not None else [])
            rec = np.zeros(n, np.dtype(fields))
            rec["p"] = verts
            if colors is not None:
                rec["c"] = colors
            f.write(rec.tobytes())
        else:
            for k in range(n):
                line = " ".join(f"{float(x):.9g}" for x in verts[k])
                if colors is not None:
                    line += " " + " ".join(str(int(c)) for c in colors[k])
                f.write((line + "\n").encode())


@pytest.mark.parametrize("coloured", [False, True])
def test_readers_take_a_file_without_faces(tmp_path, coloured):
    from mvlm_amd.utils import load_mesh
    from mvlm_amd.utils.mesh_io import load_obj

    rs = np.random.RandomState(5)
    verts = rs.uniform(-90, 90, size=(257, 3)).astype(np.float32)
    colors = rs.randint(0, 256, size=(257, 3)).astype(np.uint8) if coloured else None
    obj = tmp_path / "cloud.obj"
    lines = []
    for k in range(len(verts)):
        line = "v " + " ".join(f"{float(x):.9g}" for x in verts[k])
        if coloured:
            line += " " + " ".join(f"{c / 255.0:.6f}" for c in colors[k])
        lines.append(line)
    obj.write_text("\n".join(lines) + "\n")
    _write_ply(tmp_path / "ascii.ply", verts, colors, binary=False)
    _write_ply(tmp_path / "binary.ply", verts, colors, binary=True)
    meshes = {"load_obj native": load_obj(obj), "load_obj python": load_obj(obj, reader="python"), "load_mesh obj": load_mesh(obj),
              "load_mesh ascii ply": load_mesh(tmp_path / "ascii.ply"), "load_mesh binary ply": load_mesh(tmp_path / "binary.ply")}
    for name, m in meshes.items():
        assert m.n_tris == 0 and m.tris.shape == (0, 3) and m.n_verts == 257, name
        assert m.point_radius is None and m.uvs is None, name
        np.testing.assert_array_equal(m.verts, verts, err_msg=name)
        if coloured:
            np.testing.assert_array_equal(m.colors, colors, err_msg=name)
        else:
            assert m.colors is None, name


def test_a_radius_travels_with_the_mesh():
    from mvlm_amd.__main__ import build_parser
    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.prealign import aligned

    cloud = Mesh(_grid(4, 10.0), np.zeros((0, 3), np.int32), point_radius=3.0)
    moved = aligned(cloud, {"align_center_of_mass": True, "rot_x": 10, "rot_y": 0, "rot_z": 0, "scale": 1})
    assert moved is not cloud and moved.n_tris == 0 and moved.point_radius == 3.0
    assert Mesh(_grid(2, 1.0), np.zeros((0, 3), np.int32)).point_radius is None
    assert build_parser().parse_args(["-p", "x"]).point_radius is None
    assert build_parser().parse_args(["-p", "x", "--point-radius", "3.0"]).point_radius == 3.0


@pytest.mark.parametrize("ry", [0.0, 60.0])
def test_a_grid_cloud_has_no_holes_and_stays_near_its_plane(ry):
    """A planar 60 x 60 grid under its automatic radius: every pixel more than ceil(r_px) + 1 pixels inside the outline is
    covered, and its depth byte is within 255 (r tan(theta) + r) / 1500 + 1 of the plane's - in-plane reach r on a plane tilted
    by theta, the paraboloid's rim, truncation."""
    from oracle.raster import multiview_render

    verts = _grid(60, 3.0, z=10.0)
    r = pm.auto_radius(verts)
    r_px = pm.radius_steps(r) / 256.0
    assert 0.75 < r_px < 8.0
    poses = np.array([[0.0, ry, 0.0, 0.0, 0.0, 0.0]], np.float32)
    cloud = pm.render(verts, poses)[0]
    half = 29.5 * 3.0
    quad = np.array([[-half, -half, 10.0], [half, -half, 10.0], [half, half, 10.0], [-half, half, 10.0]], np.float32)
    plane = multiview_render(quad, np.array([[0, 1, 2], [0, 2, 3]], np.int32), None, None, poses)[0]
    X, Y, _ = pm.transform(quad, pm.rotations(poses)[0])
    margin = (math.ceil(r_px) + 1) * 256
    i, j = np.meshgrid(np.arange(256), np.arange(256))
    cx, cy = 256 * i + 128, 256 * j + 128
    inside = (cx > X.min() + margin) & (cx < X.max() - margin) & (cy > Y.min() + margin) & (cy < Y.max() - margin)
    inside = inside[::-1]                                                      # (image rows run top down)
    assert inside.sum() > 5000
    covered = cloud[..., 3] != np.float32(1.0) / np.float32(255.0)
    assert covered[inside].all(), f"{(~covered[inside]).sum()} holes"
    assert (plane[..., 3][inside] != np.float32(1.0) / np.float32(255.0)).all()
    got = np.rint(cloud[..., 3] * 255.0).astype(np.int64)[inside]
    want = np.rint(plane[..., 3] * 255.0).astype(np.int64)[inside]
    bound = 255.0 * (r * math.tan(math.radians(ry)) + r) / 1500.0 + 1.0
    worst = int(np.abs(got - want).max())
    print(f"ry {ry}: r {r:.3f} units = {r_px:.3f} px, worst depth difference {worst} of at most {bound:.2f}")
    assert worst <= bound
