"""-m gpu: every picture flag in ONE pipeline - landmark view, ray view, view sheet and heat sheet behind the same prediction, with a
report.  The landmarks are those of a pipeline that draws nothing, and every file holds the pixels of the file a pipeline with only
that picture's flag (and the report) writes: the pictures share a pass without seeing each other."""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# flag -> the files it writes, under the working directory
FILES = {"visualize_img": ["visualization/scan_dtu3d.png"],
         "visualize_rays_img": [f"visualization/ray_screenshots/scan_dtu3d_rays_{i}.png" for i in range(3)],
         "visualize_sheet": ["visualization/scan_dtu3d_views.png"],
         "visualize_heat": ["visualization/scan_dtu3d_heat.png"]}


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _decoded(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    from mvlm_amd.utils.synthetic import write_face_like_obj

    return write_face_like_obj(tmp_path_factory.mktemp("pictures_scan") / "scan.obj", grid=40, tex_size=64, seed=3)


def _predict(scan, folder, monkeypatch, **kw):
    from mvlm_amd import pipeline

    folder.mkdir()
    monkeypatch.chdir(folder)
    pipe = pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:3", verbose=False, **kw)
    np.random.seed(1)
    return pipe, pipe.predict_one_file(scan)


@pytest.fixture(scope="module")
def plain(scan, tmp_path_factory):
    """Every flag off: the landmarks, and nothing written."""
    with pytest.MonkeyPatch.context() as mp:
        folder = tmp_path_factory.mktemp("pictures_off") / "off"
        _, landmarks = _predict(scan, folder, mp)
        assert list(folder.iterdir()) == []
    return landmarks


@pytest.mark.parametrize("encoder", ("host", "device"))
def test_all_pictures_of_one_pass_equal_the_pictures_drawn_alone(scan, plain, encoder, tmp_path, monkeypatch):
    look = dict(landmark_report=True, visualize_size=64, sheet_scale=1, view_png_encoder=encoder)
    pipe, got = _predict(scan, tmp_path / "all", monkeypatch, **look, **{flag: True for flag in FILES})
    np.testing.assert_array_equal(_bits(got), _bits(plain))                  # the pictures change nothing: bit for bit
    assert pipe._ray_view is None and pipe.last_report is not None
    written = sorted(str(p.relative_to(tmp_path / "all")) for p in (tmp_path / "all").rglob("*") if p.is_file())
    assert written == sorted(f for files in FILES.values() for f in files)
    assert all(key in pipe.timings for key in ("visualize", "visualize_sheet", "visualize_heat", "visualize_rays"))
    for flag, files in FILES.items():
        alone, again = _predict(scan, tmp_path / flag, monkeypatch, **look, **{flag: True})
        np.testing.assert_array_equal(_bits(again), _bits(plain))
        assert sorted(str(p.relative_to(tmp_path / flag)) for p in (tmp_path / flag).rglob("*") if p.is_file()) == sorted(files)
        for f in files:
            together, single = _decoded(tmp_path / "all" / f), _decoded(tmp_path / flag / f)
            assert together.shape == single.shape and int((together != single).sum()) == 0, (flag, f)
    assert _decoded(tmp_path / "all" / FILES["visualize_img"][0]).shape == (64, 64, 3)
    assert (_decoded(tmp_path / "all" / FILES["visualize_heat"][0]) != _decoded(tmp_path / "all" / FILES["visualize_sheet"][0])).any()
    assert Path(pipe.last_view_path) == Path(FILES["visualize_img"][0]) and len(pipe.last_ray_view_paths) == 3
