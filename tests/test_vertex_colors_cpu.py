"""Per-vertex colours on the host (CPU only): the readers of .ply / .vtk / .obj, malformed colour blocks under ASan + UBSan,
the Mesh helpers that carry colours along, and the self-checks of the CPU model of the coloured render
(tests/native/vcolor_raster.c) that tests/test_gpu_vertex_colors.py holds the HIP kernels against."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

import msaa_model
import vcolor_model
from conftest import REPO
from mvlm_amd.utils import load_mesh, load_obj
from mvlm_amd.utils.mesh_io import Mesh, write_obj
from mvlm_amd.utils.prealign import aligned


def tiny_mesh():
    """a 2x2-cell grid (9 points, 8 triangles) and a fan of 5 triangles around a tenth point, every point its own colour"""
    lin = np.linspace(-40.0, 0.0, 3)
    x, y = np.meshgrid(lin, lin)
    grid = np.stack([x.ravel(), y.ravel(), 5.0 + 0.25 * x.ravel() * y.ravel() / 40.0], 1)
    idx = np.arange(9).reshape(3, 3)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    tris = [np.stack([a, b, c], 1), np.stack([a, c, d], 1)]
    ang = np.linspace(0.0, 2 * np.pi, 6)[:5]
    fan = np.concatenate([[[30.0, 30.0, 12.0]], np.stack([30 + 20 * np.cos(ang), 30 + 20 * np.sin(ang), 3.0 + ang], 1)])
    tris.append(np.array([[9, 10 + k, 10 + (k + 1) % 5] for k in range(5)]))
    verts = np.concatenate([grid, fan]).astype(np.float32)
    colors = np.random.RandomState(11).randint(0, 256, (len(verts), 3)).astype(np.uint8)
    colors[0], colors[1] = (0, 255, 1), (254, 128, 127)
    return verts, np.concatenate(tris).astype(np.int32), colors


def write_ply(path, verts, tris, colors, fmt="ascii", alpha=False, names=("red", "green", "blue"), ctype="uchar"):
    hdr = ["ply", f"format {fmt} 1.0", f"element vertex {len(verts)}", "property float x", "property float y", "property float z"]
    if colors is not None:
        hdr += [f"property {ctype} {n}" for n in names]
        if alpha:
            hdr += [f"property {ctype} alpha"]
    hdr += [f"element face {len(tris)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(hdr) + "\n").encode())
        e = "<" if fmt == "binary_little_endian" else ">"
        for i, v in enumerate(verts):
            c = [] if colors is None else list(colors[i]) + ([77] if alpha else [])
            if ctype == "float":
                c = [float(k) / 255.0 for k in c]
            if fmt == "ascii":
                f.write((" ".join([repr(float(k)) for k in v] + [repr(k) if ctype == "float" else str(int(k)) for k in c]) + "\n").encode())
            else:
                f.write(struct.pack(e + "3f", *v) + (struct.pack(e + f"{len(c)}f", *c) if ctype == "float" else bytes(int(k) for k in c)))
        for t in tris:
            f.write(f"3 {t[0]} {t[1]} {t[2]}\n".encode() if fmt == "ascii" else struct.pack(e + "B3i", 3, *t))


def write_vtk(path, verts, tris, colors, binary, ncomp=3):
    with open(path, "wb") as f:
        f.write(f"# vtk DataFile Version 3.0\nvtk output\n{'BINARY' if binary else 'ASCII'}\nDATASET POLYDATA\n".encode())
        f.write(f"POINTS {len(verts)} float\n".encode())
        f.write(verts.astype(">f4").tobytes() + b"\n" if binary else
                ("\n".join(" ".join(repr(float(k)) for k in v) for v in verts) + "\n").encode())
        cells = np.concatenate([np.full((len(tris), 1), 3), tris], 1)
        f.write(f"POLYGONS {len(tris)} {cells.size}\n".encode())
        f.write(cells.astype(">i4").tobytes() + b"\n" if binary else ("\n".join(" ".join(str(k) for k in c) for c in cells) + "\n").encode())
        if colors is not None:
            c = np.concatenate([colors, np.full((len(colors), ncomp - 3), 255, np.uint8)], 1)
            f.write(f"POINT_DATA {len(verts)}\nCOLOR_SCALARS scan_colours {ncomp}\n".encode())
            f.write(c.tobytes() + b"\n" if binary else
                    ("\n".join(" ".join(f"{k / 255.0:.6f}" for k in row) for row in c) + "\n").encode())


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("coloured")
    verts, tris, colors = tiny_mesh()
    out = {}
    for fmt in ("ascii", "binary_little_endian", "binary_big_endian"):
        for alpha in (False, True):
            for names in (("red", "green", "blue"), ("diffuse_red", "diffuse_green", "diffuse_blue")):
                p = d / f"{fmt}_{int(alpha)}_{names[0]}.ply"
                write_ply(p, verts, tris, colors, fmt, alpha, names)
                out[p.name] = (p, d / f"plain_{fmt}.ply")
        write_ply(d / f"plain_{fmt}.ply", verts, tris, None, fmt)
    for binary in (False, True):
        for ncomp in (3, 4):
            p = d / f"{'bin' if binary else 'ascii'}_{ncomp}.vtk"
            write_vtk(p, verts, tris, colors, binary, ncomp)
            out[p.name] = (p, d / f"plain_{int(binary)}.vtk")
        write_vtk(d / f"plain_{int(binary)}.vtk", verts, tris, None, binary)
    write_obj(d / "xyzrgb.obj", verts, tris, colors=colors)
    write_obj(d / "plain.obj", verts, tris)
    out["xyzrgb.obj"] = (d / "xyzrgb.obj", d / "plain.obj")
    return d, out, (verts, tris, colors)   # {name: (coloured file, the same mesh without colours)}


def test_every_format_gives_the_same_coloured_mesh(files):
    d, coloured, (verts, tris, colors) = files
    assert len(coloured) == 12 + 4 + 1
    for name, (p, plain_path) in coloured.items():
        m = load_mesh(p)
        plain = load_mesh(plain_path)
        assert plain.colors is None, name
        np.testing.assert_array_equal(m.verts, plain.verts, err_msg=name)
        np.testing.assert_array_equal(m.tris, plain.tris, err_msg=name)
        assert m.uvs is None and m.colors is not None and m.colors.dtype == np.uint8, name
        if p.suffix == ".obj":   # the OBJ reader numbers points in order of first use: the colour has followed its point
            order = [int(np.nonzero((np.abs(verts - v) < 1e-5).all(1))[0][0]) for v in m.verts]
            np.testing.assert_array_equal(np.asarray(order)[m.tris], tris, err_msg=name)
            np.testing.assert_array_equal(m.colors, colors[order], err_msg=name)
        else:
            np.testing.assert_array_equal(m.tris, tris, err_msg=name)
            np.testing.assert_array_equal(m.colors, colors, err_msg=name)


def test_ply_colours_of_another_type_mean_no_colours(tmp_path):
    verts, tris, colors = tiny_mesh()
    for fmt in ("ascii", "binary_little_endian"):
        write_ply(tmp_path / "f.ply", verts, tris, colors, fmt, ctype="float")
        m = load_mesh(tmp_path / "f.ply")
        assert m.colors is None
        np.testing.assert_array_equal(m.verts, verts)
        np.testing.assert_array_equal(m.tris, tris)


def test_obj_colours_follow_a_duplicated_point_and_need_every_v_line(tmp_path):
    text = ("v 0 0 0 1.0 0.0 0.501961\nv 10 0 0 0.2 0.4 0.6\nv 10 10 0 0 0 0\nv 0 10 0 1 1 1\n"
            "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.5 0.5\n"
            "f 1/1 2/2 3/3\nf 1/5 3/3 4/4\n")                       # point 1 under two vt: two corners
    (tmp_path / "dup.obj").write_text(text)
    for reader in ("native", "python"):
        m = load_obj(tmp_path / "dup.obj", reader=reader)
        assert m.n_verts == 5 and m.uvs is not None
        np.testing.assert_array_equal(m.colors, [[255, 0, 128], [51, 102, 153], [0, 0, 0], [255, 0, 128], [255, 255, 255]])
        np.testing.assert_array_equal(m.verts[3], m.verts[0])           # (corners are numbered in order of first use)
    (tmp_path / "partial.obj").write_text(text.replace("v 10 10 0 0 0 0\n", "v 10 10 0\n"))
    (tmp_path / "w.obj").write_text("v 0 0 0 1\nv 10 0 0 1\nv 0 10 0 1\nf 1 2 3\n")   # "v x y z w": four numbers, no colour
    for reader in ("native", "python"):
        assert load_obj(tmp_path / "partial.obj", reader=reader).colors is None
        m = load_obj(tmp_path / "w.obj", reader=reader)
        assert m.colors is None and m.n_verts == 3


def test_the_native_and_the_python_obj_reader_agree_on_colours(files, tmp_path):
    d, coloured, (verts, tris, colors) = files
    a, b = load_obj(coloured["xyzrgb.obj"][0], reader="native"), load_obj(coloured["xyzrgb.obj"][0], reader="python")
    for k in ("verts", "tris", "colors"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    # out-of-range and odd numbers: clamped, rounded to nearest, NaN -> 0 - in both
    (tmp_path / "odd.obj").write_text("v 0 0 0 -0.5 1.5 nan\nv 1 0 0 0.0019 0.00197 0.998\nv 0 1 0 1e-9 0.5 inf\nf 1 2 3\n")
    a, b = load_obj(tmp_path / "odd.obj", reader="native"), load_obj(tmp_path / "odd.obj", reader="python")
    np.testing.assert_array_equal(a.colors, [[0, 255, 0], [0, 1, 254], [0, 128, 255]])
    np.testing.assert_array_equal(a.colors, b.colors)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_malformed_colour_blocks_under_sanitizers(files, tmp_path):
    """truncated binary colour blocks, a COLOR_SCALARS count beyond the file, NaN in an OBJ colour: an error code or a defined
    result, and nothing for ASan / UBSan to report (host build of the readers; the harnesses are the existing ones)"""
    d, coloured, (verts, tris, colors) = files
    flags = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-x", "c++"]
    mesh_exe, obj_exe = tmp_path / "mesh_harness", tmp_path / "obj_harness"
    for exe, srcs in ((mesh_exe, ["mvlm_amd/csrc/mesh_readers.hip", "mvlm_amd/csrc/obj_reader.hip", "tests/native/mesh_reader_harness.cpp"]),
                      (obj_exe, ["mvlm_amd/csrc/obj_reader.hip", "tests/native/obj_reader_harness.cpp"])):
        r = subprocess.run(flags + [str(REPO / s) for s in srcs] + ["-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    bad, expect_error = [], []
    ply = coloured["binary_little_endian_1_red.ply"][0].read_bytes()
    body = ply.index(b"end_header\n") + 11
    for cut in (body + 13, body + 16 * len(verts) - 2, body + 16 * len(verts) + 5):   # inside a colour, the last alpha, a face
        p = tmp_path / f"cut{cut}.ply"
        p.write_bytes(ply[:cut])
        bad.append(p)
        expect_error.append(p.name)
    vtk = coloured["bin_4.vtk"][0].read_bytes()
    at = vtk.index(b"COLOR_SCALARS")
    for k, data in enumerate((vtk[:at + 40], vtk[:-3], vtk.replace(b"COLOR_SCALARS scan_colours 4", b"COLOR_SCALARS scan_colours 4000000"),
                              vtk.replace(f"POINT_DATA {len(verts)}".encode(), b"POINT_DATA 99999"),
                              vtk.replace(b"COLOR_SCALARS scan_colours 4", b"COLOR_SCALARS scan_colours -1"))):
        p = tmp_path / f"bad{k}.vtk"
        p.write_bytes(data)
        bad.append(p)
        if k != 3:                                              # (the count of POINT_DATA is not what sizes the block)
            expect_error.append(p.name)
    asc = coloured["ascii_3.vtk"][0].read_bytes()
    for k, data in enumerate((asc[:asc.index(b"COLOR_SCALARS") + 60], asc.replace(b"0.", b"nan ", 3) + b" 1e999 -inf")):
        p = tmp_path / f"bad_ascii{k}.vtk"
        p.write_bytes(data)
        bad.append(p)
    expect_error.append("bad_ascii0.vtk")
    rs = np.random.RandomState(2)
    for i in range(40):                                         # random damage inside the colour blocks
        src = (ply, vtk, asc)[i % 3]
        b = bytearray(src)
        lo = (body, at, asc.index(b"COLOR_SCALARS"))[i % 3]
        for p_ in rs.randint(lo, len(b), 6):
            b[p_] = rs.randint(256) if i % 3 < 2 else rs.randint(32, 127)
        p = tmp_path / f"noise{i}{'.ply' if i % 3 == 0 else '.vtk'}"
        p.write_bytes(bytes(b))
        bad.append(p)
    env = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(mesh_exe)] + [str(p) for p in bad], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = {ln.split(": ")[0].rsplit("/", 1)[-1]: ln for ln in r.stdout.splitlines()}
    for name in expect_error:
        assert " rc=" in lines[name] and " ok " not in lines[name], lines[name]
    objs = []
    for k, text in enumerate(("v 0 0 0 nan nan nan\nv 1 0 0 inf -inf 1e999\nv 0 1 0 0.5 0.5 0.5\nf 1 2 3\n",
                              "v 0 0 0 0.1 0.2\nv 1 0 0 0.1 0.2 0.3 0.4 0.5\nv 0 1 0 x y z\nf 1 2 3\n",
                              "v 0 0 0 1 1 " + "9" * 300 + "\nv 1 0 0 1 1 1\nv 0 1 0 1 1 1\nf 1 2 3")):
        p = tmp_path / f"c{k}.obj"
        p.write_text(text)
        objs.append(p)
    r = subprocess.run([str(obj_exe)] + [str(p) for p in objs], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert r.stdout.count(" ok verts=3 tris=1") == 3, r.stdout
    np.testing.assert_array_equal(load_obj(objs[0]).colors, [[0, 0, 0], [255, 0, 255], [128, 128, 128]])   # NaN: a defined result
    assert load_obj(objs[1]).colors is None


def test_mesh_helpers_carry_colours_along(tmp_path):
    verts, tris, colors = tiny_mesh()
    m = Mesh(verts, tris, colors=colors)
    assert Mesh(verts, tris, None, None, None).colors is None            # positional construction is what it was
    moved = aligned(m, {"align_center_of_mass": True, "rot_x": 10, "rot_y": 0, "rot_z": -5, "scale": 1.5})
    assert moved is not m and moved.to_original is not None
    np.testing.assert_array_equal(moved.colors, colors)
    every = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256], 1).astype(np.uint8)   # each byte value
    v = np.zeros((256, 3), np.float32)
    v[:, 0] = np.arange(256)
    write_obj(tmp_path / "all.obj", v, np.array([[0, 1, 2]], np.int32), colors=every)
    assert "0.501961" in (tmp_path / "all.obj").read_text()           # 128 / 255 with six decimals
    for reader in ("native", "python"):
        back = load_obj(tmp_path / "all.obj", reader=reader)            # a point cloud but for one triangle
        np.testing.assert_array_equal(back.colors[:3], every[:3])
    from mvlm_amd.utils.mesh_io import _read_obj_native, _read_obj_python

    (tmp_path / "cloud.obj").write_text("\n".join((tmp_path / "all.obj").read_text().splitlines()[:-1]) + "\n")
    for read in (_read_obj_native, _read_obj_python):                    # no face: every point of the file, every byte value
        np.testing.assert_array_equal(read(tmp_path / "cloud.obj")[3], every)
    from mvlm_amd.utils.synthetic import face_like_mesh

    f = face_like_mesh(12, 16, seed=2, vertex_colors=True)
    assert f.colors.shape == (144, 3) and f.colors.dtype == np.uint8 and len(np.unique(f.colors, axis=0)) > 50
    assert face_like_mesh(12, 16, seed=2).colors is None


# ---- the CPU model of the coloured render ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("models")
    vcolor_model.load(d)
    msaa_model.load(d)
    return vcolor_model.render, msaa_model.render


@pytest.fixture(scope="module")
def face40():
    import gl_contract

    return gl_contract.load()[1]["face40"]


def test_model_without_colours_is_the_oracle_and_the_multisampling_model(models, face40):
    from oracle import raster

    model, msaa = models
    sc = face40
    for uvs, tex in ((sc["uvs"], sc["tex"]), (None, None)):
        want1 = raster.multiview_render(sc["verts"], sc["tris"], uvs, tex, sc["poses"])
        want4 = msaa(sc["verts"], sc["tris"], uvs, tex, sc["poses"], samples=4)
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], uvs, tex, sc["poses"], samples=1), want1)
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], uvs, tex, sc["poses"], samples=4), want4)
    # all-255 colours are the white mesh; with a texture, colours change nothing
    white = np.full((len(sc["verts"]), 3), 255, np.uint8)
    some = np.random.RandomState(0).randint(0, 256, white.shape).astype(np.uint8)
    for samples, want in ((1, want1), (4, want4)):
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], None, None, sc["poses"], samples=samples, colors=white), want)
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], sc["uvs"], None, sc["poses"], samples=samples, colors=white), want)
        textured = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], samples=samples)
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], samples=samples, colors=some),
                                      textured)


@pytest.mark.parametrize("samples", [1, 4])
def test_a_constant_colour_stays_constant_bit_for_bit(models, face40, samples):
    model, _ = models
    sc = face40
    const = np.tile(np.array([17, 200, 93], np.uint8), (len(sc["verts"]), 1))
    out, win_tri, win_rgb = model(sc["verts"], sc["tris"], None, None, sc["poses"], samples=samples, colors=const, per_sample=True)
    plain = model(sc["verts"], sc["tris"], None, None, sc["poses"], samples=samples)
    np.testing.assert_array_equal(out[..., 3], plain[..., 3])            # the depth plane never sees a colour
    covered = win_tri >= 0
    assert covered.any() and (~covered).any()
    assert (win_rgb[covered] == (17, 200, 93)).all() and (win_rgb[~covered] == 255).all()
    if samples == 1:
        rgb = np.round(out[..., :3] * 255).astype(np.uint8)[:, ::-1]       # GL rows, like win_tri
        assert (rgb[covered[..., 0]] == (17, 200, 93)).all() and (rgb[~covered[..., 0]] == 255).all()
