"""The CPU model of the landmark view (tests/native/landmark_view.c, tests/view_model.py) - no GPU.

The mesh half: at S = 256 with the network's frame and no landmarks the model must be oracle/raster.c (the contract the OpenGL
golden pins), and tests/native/vcolor_raster.c with per-vertex colours.  The sphere half: closed forms of an analytic sphere
under an orthographic camera, on an empty mesh and on a screen-parallel quad."""
import math

import numpy as np
import pytest

import vcolor_contract
import vcolor_model
import view_model
from gl_contract import load

_, SCENES = load()
_, COLOURED = vcolor_contract.load()
NAMES = ["face40", "coarse", "offscreen", "centres"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    view_model.load(tmp_path_factory.mktemp("view_model"))
    return view_model.render


@pytest.fixture(scope="module")
def vcolor(tmp_path_factory):
    vcolor_model.load(tmp_path_factory.mktemp("vcolor_model_for_view"))
    return vcolor_model.render


def _bytes(stack):
    return np.round(stack[..., :3] * 255.0).astype(np.uint8)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_the_model_is_the_oracle_at_the_network_window(model, name, bits):
    from oracle.raster import multiview_render

    sc = SCENES[name]
    poses = np.asarray(sc["poses"], np.float64)
    for uvs, tex in ((sc["uvs"], sc["tex"]), (None, None)):  # textured, white
        want = _bytes(multiview_render(sc["verts"], sc["tris"], uvs, tex, poses, subpixel_bits=bits))
        got, counts, winner = model(sc["verts"], sc["tris"], uvs, tex, poses, 256, subpixel_bits=bits)
        np.testing.assert_array_equal(got[..., :3], want)
        assert (got[..., 3] == 255).all() and counts.shape == (len(poses), 0)
        assert ((winner >= 0) | (winner == -1)).all()


@pytest.mark.parametrize("name", NAMES)
def test_the_model_is_the_oracle_with_geometry_shading(model, name):
    from oracle.raster import multiview_render

    sc = SCENES[name]
    poses = np.asarray(sc["poses"], np.float64)
    want = _bytes(multiview_render(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], poses, shading="geometry"))
    got, _, _ = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], poses, 256, shading="geometry")
    np.testing.assert_array_equal(got[..., :3], want)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_the_model_is_the_vertex_colour_model(model, vcolor, name, bits):
    sc = SCENES[name]
    col = COLOURED[name]["colors"]
    poses = np.asarray(sc["poses"], np.float64)
    want = _bytes(vcolor(sc["verts"], sc["tris"], None, None, poses, subpixel_bits=bits, colors=col))
    got, _, _ = model(sc["verts"], sc["tris"], None, None, poses, 256, colors=col, subpixel_bits=bits)
    np.testing.assert_array_equal(got[..., :3], want)


# ---- spheres ---------------------------------------------------------------------------------------------------------------
# frame (0, 0, 128) at S = 256: k = 1 exactly, a pixel is a model unit, pixel (i, j) has its centre at (i + 0.5 - 128, j + 0.5 - 128)
UNIT = (0.0, 0.0, 128.0)
FRONT = [[0.0, 0.0, 0.0]]
EMPTY = view_model.far_triangle()
QUAD = view_model.quad(0.0)


def _disc(model, mesh, lm, r, rgb=None, frame=UNIT, size=256):
    return model(mesh[0], mesh[1], None, None, FRONT, size, frame=frame, landmarks=lm, radius=r, lm_rgb=rgb)


def test_the_centre_pixel_has_the_full_colour(model):
    img, counts, winner = _disc(model, EMPTY, [[0.5, 0.5, 0.0]], 7.25, rgb=[[10, 200, 255]])
    assert tuple(img[0, 255 - 128, 128]) == (10, 200, 255, 255)  # pixel (128, 128): dx = dy = 0, hgt = R
    assert winner[0, 255 - 128, 128] == -2
    blue, _, _ = _disc(model, EMPTY, [[0.5, 0.5, 0.0]], 7.25)
    assert tuple(blue[0, 255 - 128, 128]) == (0, 0, 255, 255)  # the default colour (viewer.py:71)
    edge = img[0][winner[0] == -2]
    assert edge[:, 2].min() < 128  # shaded towards the rim


@pytest.mark.parametrize("r", [0.75, 3.1, 20.3, 61.7])
def test_the_pixel_count_is_the_disc_area_within_the_perimeter_bound(model, r):
    _, counts, winner = _disc(model, EMPTY, [[0.21, -0.37, 10.0]], r)
    assert counts[0, 0] == (winner == -2).sum()
    assert abs(counts[0, 0] - math.pi * r * r) <= 2 * math.pi * r + 4


def test_depth_against_the_quad(model):
    free = _disc(model, EMPTY, [[3.3, -2.1, 0.0]], 9.5)[1][0, 0]
    assert free > 0
    assert _disc(model, QUAD, [[3.3, -2.1, -40.0]], 9.5)[1][0, 0] == 0      # wholly behind: hidden
    assert _disc(model, QUAD, [[3.3, -2.1, 0.0]], 9.5)[1][0, 0] == free     # centred ON the quad: the whole disc (ties win)
    assert _disc(model, QUAD, [[3.3, -2.1, 40.0]], 9.5)[1][0, 0] == free    # in front
    part = _disc(model, QUAD, [[3.3, -2.1, -5.0]], 9.5)[1][0, 0]            # the cap that pokes through
    assert 0 < part < free


def test_two_spheres_at_one_point_the_later_wins_every_pixel(model):
    p = [1.5, 2.5, 5.0]
    img, counts, winner = _disc(model, QUAD, [p, p], 6.0, rgb=[[255, 0, 0], [0, 255, 0]])
    assert counts[0, 0] == 0 and counts[0, 1] > 0
    assert ((winner == -3).sum() == counts[0, 1]) and not (winner == -2).any()


def test_radius_zero_and_outside_the_window_win_nothing(model):
    img, counts, _ = _disc(model, QUAD, [[0.5, 0.5, 1.0]], 0.0)
    assert counts[0, 0] == 0
    ref, _, _ = model(QUAD[0], QUAD[1], None, None, FRONT, 256, frame=UNIT)
    np.testing.assert_array_equal(img, ref)
    _, counts, _ = _disc(model, QUAD, [[200.0, 0.0, 1.0], [0.0, -400.0, 1.0], [1e30, 1e30, 0.0]], 20.0)
    assert (counts == 0).all()
    _, counts, _ = _disc(model, QUAD, [[0.0, 0.0, 600.0], [0.0, 0.0, -1100.0]], 5.0)  # beyond the near / the far plane
    assert (counts == 0).all()
