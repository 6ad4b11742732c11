"""Normals of point clouds without a GPU: the readers keep a file's per-point normals (.ply nx ny nz in ASCII and both binary byte
orders, legacy .vtk POINT_DATA NORMALS in ASCII and BINARY) and drop what is no complete set of them, a mesh with faces keeps them
too, the numpy model of the estimate (tests/cloud_normals_model.py) finds the normal of an exact plane, and the option that says
where a cloud's normals come from is parsed and judged by Pipeline._check_cloud as the contract says (a stub renderer: no device)."""
import types

import numpy as np
import pytest

import cloud_normals_model as cm

RS = np.random.RandomState(3)
VERTS = RS.uniform(-90, 90, size=(37, 3)).astype(np.float32)
NORMALS = RS.normal(size=(37, 3)).astype(np.float32)           # any length: the readers do not normalise
NORMALS[5] = 0.0
TRIS = np.array([[0, 1, 2], [2, 3, 4], [10, 20, 30]], np.int32)


def _ply_header(fmt, n, props, faces=0):
    head = f"ply\nformat {fmt} 1.0\nelement vertex {n}\n" + "".join(f"property {t} {name}\n" for t, name in props)
    if faces:
        head += f"element face {faces}\nproperty list uchar int vertex_indices\n"
    return (head + "end_header\n").encode()


def _write_ply(path, fmt, verts, normals, tris=None, ntype="float", names=("nx", "ny", "nz")):
    props = [("float", "x"), ("float", "y"), ("float", "z")] + [(ntype, n) for n in names]
    tris = np.zeros((0, 3), np.int32) if tris is None else tris
    with open(path, "wb") as f:
        f.write(_ply_header(fmt, len(verts), props, len(tris)))
        if fmt == "ascii":
            for v, n in zip(verts, normals):
                vals = [f"{float(x):.9g}" for x in v] + [(f"{float(x):.9g}" if ntype != "int" else str(int(x))) for x in n[:len(names)]]
                f.write((" ".join(vals) + "\n").encode())
            for t in tris:
                f.write(("3 " + " ".join(str(int(i)) for i in t) + "\n").encode())
        else:
            e = "<" if fmt == "binary_little_endian" else ">"
            nt = {"float": "f4", "double": "f8", "int": "i4"}[ntype]
            rec = np.zeros(len(verts), np.dtype([("p", e + "f4", 3), ("n", e + nt, len(names))]))
            rec["p"], rec["n"] = verts, normals[:, :len(names)]
            f.write(rec.tobytes())
            face = np.zeros(len(tris), np.dtype([("c", "u1"), ("i", e + "i4", 3)]))
            face["c"], face["i"] = 3, tris
            f.write(face.tobytes())


def _write_vtk(path, binary, verts, normals, tris=None, ntype="float"):
    with open(path, "wb") as f:
        f.write(f"# vtk DataFile Version 3.0\ncloud\n{'BINARY' if binary else 'ASCII'}\nDATASET POLYDATA\nPOINTS {len(verts)} float\n".encode())
        if binary:
            f.write(verts.astype(">f4").tobytes() + b"\n")
        else:
            f.write(("\n".join(" ".join(f"{float(x):.9g}" for x in v) for v in verts) + "\n").encode())
        if tris is not None and len(tris):
            f.write(f"POLYGONS {len(tris)} {4 * len(tris)}\n".encode())
            cells = np.concatenate([np.full((len(tris), 1), 3, np.int32), tris], axis=1)
            if binary:
                f.write(cells.astype(">i4").tobytes() + b"\n")
            else:
                f.write(("\n".join(" ".join(str(int(i)) for i in c) for c in cells) + "\n").encode())
        f.write(f"POINT_DATA {len(verts)}\nNORMALS Normals {ntype}\n".encode())
        if binary:
            f.write(normals.astype(">f4" if ntype == "float" else ">f8").tobytes() + b"\n")
        else:
            f.write(("\n".join(" ".join(f"{float(x):.9g}" for x in n) for n in normals) + "\n").encode())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("ntype", ["float", "double"])
def test_a_ply_keeps_its_normals(tmp_path, fmt, ntype):
    from mvlm_amd.utils import load_mesh

    _write_ply(tmp_path / "c.ply", fmt, VERTS, NORMALS, ntype=ntype)
    m = load_mesh(tmp_path / "c.ply")
    assert m.n_tris == 0 and m.normals.dtype == np.float32 and m.normals.shape == (37, 3)
    np.testing.assert_array_equal(m.verts, VERTS)
    np.testing.assert_array_equal(m.normals, NORMALS)


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("ntype", ["float", "double"])
def test_a_vtk_keeps_its_normals(tmp_path, binary, ntype):
    from mvlm_amd.utils import load_mesh

    _write_vtk(tmp_path / "c.vtk", binary, VERTS, NORMALS, ntype=ntype)
    m = load_mesh(tmp_path / "c.vtk")
    assert m.n_tris == 0 and m.normals.dtype == np.float32
    np.testing.assert_array_equal(m.verts, VERTS)
    np.testing.assert_array_equal(m.normals, NORMALS)


def test_what_is_no_complete_set_of_normals_is_none(tmp_path):
    from mvlm_amd.utils import load_mesh
    from mvlm_amd.utils.mesh_io import load_obj

    for fmt in ("ascii", "binary_little_endian"):
        _write_ply(tmp_path / "two.ply", fmt, VERTS, NORMALS, names=("nx", "ny"))           # only nx ny
        m = load_mesh(tmp_path / "two.ply")
        assert m.normals is None
        np.testing.assert_array_equal(m.verts, VERTS)
        _write_ply(tmp_path / "int.ply", fmt, VERTS, np.rint(NORMALS * 100), ntype="int")   # an integer type: no agreed scale
        m = load_mesh(tmp_path / "int.ply")
        assert m.normals is None
        np.testing.assert_array_equal(m.verts, VERTS)
    # two vertex elements, the second alone with normals: 3 normals for 5 points
    text = ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            "element vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
            "property float nz\nend_header\n0 0 0\n1 0 0\n2 0 0 0 0 1\n3 0 0 0 0 1\n4 0 0 0 0 1\n")
    (tmp_path / "mismatch.ply").write_text(text)
    m = load_mesh(tmp_path / "mismatch.ply")
    assert m.n_verts == 5 and m.normals is None
    # no normals at all; OBJ "vn" lines are not read
    _write_ply(tmp_path / "bare.ply", "ascii", VERTS, NORMALS, names=())
    assert load_mesh(tmp_path / "bare.ply").normals is None
    (tmp_path / "vn.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvn 0 0 1\nvn 0 0 1\n")
    assert load_mesh(tmp_path / "vn.obj").normals is None and load_obj(tmp_path / "vn.obj").normals is None


def test_a_mesh_with_faces_keeps_its_normals_and_renders_as_before(tmp_path):
    from mvlm_amd.utils import Mesh, load_mesh
    from oracle.raster import multiview_render

    _write_ply(tmp_path / "m.ply", "binary_little_endian", VERTS, NORMALS, TRIS)
    _write_vtk(tmp_path / "m.vtk", True, VERTS, NORMALS, TRIS)
    _write_vtk(tmp_path / "a.vtk", False, VERTS, NORMALS, TRIS)
    poses = np.array([[10.0, -20.0, 5.0, 0, 0, 0]], np.float32)
    want = multiview_render(VERTS, TRIS, None, None, poses)
    for name in ("m.ply", "m.vtk", "a.vtk"):
        m = load_mesh(tmp_path / name)
        assert m.n_tris == 3, name
        np.testing.assert_array_equal(m.tris, TRIS, err_msg=name)
        np.testing.assert_array_equal(m.normals, NORMALS, err_msg=name)
        np.testing.assert_array_equal(multiview_render(m.verts, m.tris, None, None, poses), want, err_msg=name)   # the geometry is the file's
    assert Mesh(VERTS, TRIS).normals is None


def test_normals_turn_with_a_pre_aligned_mesh():
    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.prealign import aligned

    cloud = Mesh(VERTS, np.zeros((0, 3), np.int32), normals=NORMALS)
    moved = aligned(cloud, {"align_center_of_mass": True, "rot_x": 0, "rot_y": 0, "rot_z": 90, "scale": 2})
    want = np.stack([-NORMALS[:, 1], NORMALS[:, 0], NORMALS[:, 2]], axis=1).astype(np.float64) * 2.0
    np.testing.assert_allclose(moved.normals, want, rtol=0, atol=1e-5)
    assert moved.normals.dtype == np.float32 and cloud.normals is NORMALS


def test_the_models_normal_of_an_exact_plane():
    lin = (np.arange(12) - 5.5) * 3.0
    x, y = np.meshgrid(lin, lin)
    verts = np.stack([x.ravel(), y.ravel(), np.full(x.size, 5.0)], axis=1).astype(np.float32)
    table = cm.neighbors(verts)
    assert (table >= 0).all() and (table[:, 0] == np.arange(len(verts))).all()          # itself first: d2 = 0
    n, lam = cm.normals(verts, table)
    np.testing.assert_array_equal(np.abs(n), np.tile([0.0, 0.0, 1.0], (len(verts), 1)))
    assert (lam[:, 0] == 0.0).all() and (lam[:, 1] > 0.0).all()
    front = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
    assert (cm.shade(n.astype(np.float32), front) == 255).all()
    side = np.array([0.0, 0, 1.0, 0, 1.0, 0, -1.0, 0, 0.0])                            # seen edge-on: n.z = 0
    assert (cm.shade(n.astype(np.float32), side) == 0).all()
    planted = np.array([[0, 0, 0], [np.nan, 0, 1], [0, 0, -3.0], [3.0, 0, 4.0], [np.inf, 0, 0]], np.float32)
    np.testing.assert_array_equal(cm.shade(planted, front), [0, 0, 255, 204, 0])


def test_the_models_degenerate_rows():
    verts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [0, 0, np.inf], [1, 0, 0]], np.float32)
    table = cm.neighbors(verts)
    np.testing.assert_array_equal(table[2], np.full(16, -1))
    np.testing.assert_array_equal(table[4], np.full(16, -1))
    np.testing.assert_array_equal(table[0, :5], [0, 1, 5, 3, -1])                       # equal d2: the lower id first
    np.testing.assert_array_equal(table[5, :5], [1, 5, 0, 3, -1])
    n, _ = cm.normals(verts, table)
    np.testing.assert_array_equal(n[[2, 4]], np.zeros((2, 3)))
    np.testing.assert_array_equal(np.abs(n[0]), [0.0, 0.0, 1.0])                        # four points of the plane z = 0
    two, _ = cm.normals(np.array([[0, 0, 0], [1, 1, 1]], np.float32))
    np.testing.assert_array_equal(two, np.zeros((2, 3)))                                # fewer than 3 neighbours
    same, _ = cm.normals(np.tile(np.array([[1.5, -2.0, 3.0]], np.float32), (20, 1)))
    np.testing.assert_array_equal(same, np.zeros((20, 3)))                              # a zero covariance


def test_the_option_is_parsed_and_checked():
    from mvlm_amd.__main__ import build_parser
    from mvlm_amd.utils.render3d import POINT_NORMALS

    assert POINT_NORMALS == ("file", "estimate")
    assert build_parser().parse_args(["-p", "x"]).point_normals == "file"
    assert build_parser().parse_args(["-p", "x", "--point-normals", "estimate"]).point_normals == "estimate"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-p", "x", "--point-normals", "guess"])


def _stub_pipeline(shading, point_normals, multisamples=0):
    r3 = types.SimpleNamespace(shading=shading, point_normals=point_normals, multisamples=multisamples)
    return types.SimpleNamespace(landmark_report=False, visualize_img=False, visualize_rays_img=False, renderer_3d=r3)


def test_check_cloud_lets_a_cloud_through_when_it_has_or_gets_normals():
    from mvlm_amd.pipeline.general_pipeline import Pipeline
    from mvlm_amd.utils import Mesh

    no_tris = np.zeros((0, 3), np.int32)
    bare, with_n, mesh = Mesh(VERTS, no_tris), Mesh(VERTS, no_tris, normals=NORMALS), Mesh(VERTS, TRIS)
    check = Pipeline._check_cloud
    for m in (bare, with_n, mesh):                                                      # texture mode: nothing about normals
        check(_stub_pipeline("texture", "file"), m)
    check(_stub_pipeline("geometry", "file"), mesh)                                     # triangles: not a cloud
    check(_stub_pipeline("geometry", "file"), with_n)
    check(_stub_pipeline("geometry", "estimate"), with_n)
    check(_stub_pipeline("geometry", "estimate"), bare)
    with pytest.raises(ValueError, match="geometry") as e:
        check(_stub_pipeline("geometry", "file"), bare)
    assert "point cloud" in str(e.value) and "point_normals" in str(e.value)
    with pytest.raises(ValueError, match="render_multisamples"):                        # what a cloud still cannot do
        check(_stub_pipeline("geometry", "estimate", multisamples=4), with_n)
