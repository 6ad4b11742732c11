"""-m gpu: the device PNG encoder from the pipeline down, on the planted 8-view scan of tests/test_gpu_landmark_view_pipeline.py at
visualize_size 256 - Pipeline(view_png_encoder="device") returns the landmarks of "host" and of the flags off bit for bit, its
landmark view and ray views decode to the host encoder's pixels and are the files the model of the format makes of them
(tests/png_model.py); the CLI flag does the same; the default still writes Pillow's bytes; LandmarkViewer and RayVisualizer take
the encoder too."""
import io
import shutil
from pathlib import Path

import numpy as np
import pytest

import png_model

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def planted_scan(tmp_path_factory):
    """The planted-peak scene of tests/planted.py at 8 views, written as an OBJ + JPEG pair."""
    from mvlm_amd.utils.mesh_io import write_obj
    from test_planted_cpu import planted_scene

    mesh, pts, sd, poses = planted_scene(n_views=8)
    path = tmp_path_factory.mktemp("planted_scan_png") / "scan.obj"
    write_obj(path, mesh.verts, mesh.tris, mesh.uvs, mesh.texture)
    return path, sd


def _pipeline(sd, **kw):
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config

    return pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=8), weights=sd, verbose=False, **kw)


def _pixels(path):
    from PIL import Image

    Image.open(path).verify()
    return np.asarray(Image.open(path))


def _pillow_bytes(image):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(image).save(b, "PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def runs(planted_scan, tmp_path_factory):
    """One prediction with the flags off, one per encoder with both views on; each in a working directory of its own."""
    import os

    path, sd = planted_scan
    out = {}
    here = os.getcwd()
    try:
        for name, kw in (("off", {}), ("host", dict(view_png_encoder="host")), ("device", dict(view_png_encoder="device")),
                         ("default", dict())):
            folder = tmp_path_factory.mktemp(f"png_{name}")
            os.chdir(folder)
            if name != "off":
                kw = dict(kw, visualize_img=True, visualize_rays_img=True, visualize_size=256, visualize_name="planted")
            pipe = _pipeline(sd, **kw)
            np.random.seed(1)
            landmarks = pipe.predict_one_file(path)
            out[name] = (folder, pipe, landmarks, pipe.last_error)
    finally:
        os.chdir(here)
    return out


def test_the_encoder_changes_no_landmark(runs):
    _, off, want, err = runs["off"]
    assert off.view_png_encoder == "host" and not (runs["off"][0] / "visualization").exists()
    for name in ("host", "device", "default"):
        _, pipe, got, e = runs[name]
        np.testing.assert_array_equal(_bits(got), _bits(want))
        assert e == err
    assert runs["device"][1].view_png_encoder == "device" and runs["default"][1].view_png_encoder == "host"


def test_the_device_files_hold_the_host_files_pixels(runs):
    host_dir, host, _, _ = runs["host"]
    dev_dir, dev, _, _ = runs["device"]
    assert dev.last_view_path == host.last_view_path == Path("visualization") / "scan_planted.png"
    assert [p.name for p in dev.last_ray_view_paths] == [p.name for p in host.last_ray_view_paths] == [f"scan_planted_rays_{i}.png" for i in range(3)]
    pairs = [(host_dir / host.last_view_path, dev_dir / dev.last_view_path)] + list(zip(host.last_ray_view_paths, dev.last_ray_view_paths))
    for h, d in pairs:
        want = _pixels(h)
        assert want.shape == (256, 256, 3) and (want != 255).any()
        np.testing.assert_array_equal(_pixels(d), want)
        assert Path(d).read_bytes() == png_model.encode(want)[0]     # the device's file: the contract's bytes
        assert Path(h).read_bytes() == _pillow_bytes(want)           # the host's: Pillow's, as before
    assert len({_pixels(d).tobytes() for _, d in pairs}) == 4        # four different pictures


def test_the_default_writes_pillows_bytes(runs):
    host_dir, host, _, _ = runs["host"]
    folder, pipe, _, _ = runs["default"]
    for a, b in [(host_dir / host.last_view_path, folder / pipe.last_view_path)] + list(zip(host.last_ray_view_paths, pipe.last_ray_view_paths)):
        assert Path(a).read_bytes() == Path(b).read_bytes() == _pillow_bytes(_pixels(a))


def test_an_unknown_encoder_is_refused(planted_scan):
    with pytest.raises(ValueError, match="'host' or 'device'"):
        _pipeline(planted_scan[1], view_png_encoder="gpu")


def test_cli_flag(planted_scan, tmp_path, monkeypatch):
    from mvlm_amd.__main__ import build_parser, main

    assert build_parser().parse_args(["-p", "x"]).png_encoder == "host"
    path, _ = planted_scan
    results = {}
    for enc in ("host", "device"):
        work = tmp_path / enc
        folder = work / "scans"
        folder.mkdir(parents=True)
        for f in path.parent.glob("scan.*"):
            shutil.copy(f, folder / f"one{f.suffix}")
        monkeypatch.chdir(work)
        assert main(["-p", str(folder), "--pipelines", "dtu3d", "--weights", "synthetic:3", "--seed", "2", "--visualize-img",
                     "--visualize-rays", "--visualize-size", "256", "--png-encoder", enc]) == 0
        files = [work / "visualization" / "one_dtu3d.png"] + [work / "visualization" / "ray_screenshots" / f"one_dtu3d_rays_{i}.png"
                                                              for i in range(3)]
        results[enc] = ((folder / "one_dtu3d.txt").read_bytes(), files)
    assert results["host"][0] == results["device"][0]                # the landmarks' text, byte for byte
    for h, d in zip(results["host"][1], results["device"][1]):
        np.testing.assert_array_equal(_pixels(d), _pixels(h))
        assert d.read_bytes() == png_model.encode(_pixels(h))[0] and h.read_bytes() == _pillow_bytes(_pixels(h))


def test_the_viewers_take_the_encoder(planted_scan, tmp_path, monkeypatch):
    from mvlm_amd.utils import LandmarkViewer, RayVisualizer, RayVisualizerConfig
    from mvlm_amd.utils.mesh_io import load_mesh

    path, _ = planted_scan
    mesh = load_mesh(path)
    lm = np.asarray(mesh.verts, np.float64)[::997]
    files = {}
    for enc in ("host", "device"):
        monkeypatch.chdir(tmp_path)
        (tmp_path / enc).mkdir()
        monkeypatch.chdir(tmp_path / enc)
        v = LandmarkViewer(path, lm, pname="demo", size=128, encoder=enc)
        starts = np.repeat(lm[:, None, :], 2, axis=1) + np.array([0.0, 0.0, 40.0])
        ends = np.repeat(lm[:, None, :], 2, axis=1) - np.array([[3.0, 0.0, 40.0], [0.0, 3.0, 40.0]])
        rays = RayVisualizer(RayVisualizerConfig(size=128, encoder=enc)).show(mesh, starts, ends, landmarks=lm, clip_to_mesh=False)
        files[enc] = [tmp_path / enc / v.out_path] + [tmp_path / enc / q for q in rays]
    assert len(files["device"]) == 4
    for h, d in zip(files["host"], files["device"]):
        np.testing.assert_array_equal(_pixels(d), _pixels(h))
        assert d.read_bytes() == png_model.encode(_pixels(h))[0]
    with pytest.raises(ValueError, match="'host' or 'device'"):
        LandmarkViewer(path, lm, size=128, encoder="pillow")
