"""The multisampled renderer contract against a real OpenGL drawing into a 4-sample target.

tests/golden/gl_raster_msaa4.npz = the eleven scenes of gl_raster.npz plus three probe scenes, drawn by SwiftShader's OpenGL ES
3.0 with 4 samples and resolved the way VTK resolves (tools/make_gl_msaa_golden.py).  This file holds the CPU model of the
contract (tests/native/msaa_raster.c) against it; tests/test_gpu_msaa.py holds the HIP rasteriser against the model.
tests/msaa_contract.py explains the classes a disagreement may fall into.  The numbers asserted are the measured ones."""
import numpy as np
import pytest

import gl_contract
import msaa_contract
import msaa_model

META, SCENES = msaa_contract.load()
_, SCENES1 = gl_contract.load()
GL_BITS = META["gl"]["subpixel_bits"]

# measured with the model at the GL's own sub-pixel precision: {scene: (clip, texel)} upper bounds
MEASURED = {
    "face40": (0, 12), "face224": (0, 29), "coarse": (0, 22), "centres": (0, 0), "uv_wrap": (51, 0), "last_texel": (0, 0),
    "coplanar": (0, 0), "clip": (0, 0), "offscreen": (44, 0), "third": (0, 0), "depth_ramp": (0, 0),
    "ms_positions_lo": (0, 0), "ms_positions_hi": (0, 0), "ms_resolve": (0, 0), "ms_centre": (0, 0),
}


@pytest.fixture(scope="session")
def model(tmp_path_factory):
    msaa_model.load(tmp_path_factory.mktemp("msaa_model"))
    return msaa_model.render


def _inputs(name):
    sc = SCENES[name]
    return sc if "verts" in sc else SCENES1[name]


def test_the_golden_file_is_what_the_generator_found():
    f = META["findings"]
    assert META["gl"]["renderer"] == "Google SwiftShader" and META["samples"] == 4 and GL_BITS == 4
    assert f["sample_positions_16th"] == [[3, 6], [13, 10], [6, 13], [10, 3]]
    assert f["colour_resolve"].startswith("per byte avg(avg(s0, s1), avg(s2, s3))")
    assert f["colour_evaluated_at"].startswith("pixel centre") and f["tie_rule"].startswith("left / bottom")
    assert f["depth_resolve"].startswith("not readable") and "sample 0 assumed" in f["depth_resolve"]
    assert set(SCENES) == set(MEASURED) and set(SCENES1) <= set(SCENES)
    # no other rounding of the average explains every probe pixel
    assert sorted(v for v in f["colour_resolve_hits"].values())[-2:] == [355, 512]


@pytest.mark.parametrize("name", sorted(SCENES1))
def test_model_at_one_sample_is_the_oracle(model, name):
    from oracle import raster

    sc = SCENES1[name]
    for bits in (GL_BITS, 8):
        want = raster.multiview_render(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=bits)
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=bits,
                                            samples=1), want)


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_model_against_opengl_with_four_samples(model, name):
    sc = _inputs(name)
    out, win_tri, win_rgb = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=GL_BITS, samples=4,
                                  per_sample=True)
    r = msaa_contract.compare(sc, out, win_tri, win_rgb, SCENES[name]["rgb"])
    print(name, r)
    assert r["unexplained"] == 0, r
    clip, texel = MEASURED[name]
    assert r["clip"] <= clip and r["texel"] <= texel, r
    assert r["clip"] + r["texel"] <= 0.001 * r["pixels"]


@pytest.mark.parametrize("name", sorted(n for n in MEASURED if n in SCENES1 and SCENES1[n]["lattice"] or n.startswith("ms_")))
def test_lattice_scenes_do_not_depend_on_the_subpixel_bits_at_four_samples(model, name):
    sc = _inputs(name)
    a = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=4, samples=4)
    for bits in (5, 6, 7, 8):
        np.testing.assert_array_equal(model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=bits, samples=4), a)


def test_multisampling_changes_the_views_where_the_probe_said():
    """what the GL's 4 samples change against its own single-sample drawing: silhouettes and sub-pixel triangles (2-10 % of the
    covered pixels on the faces, profiles/r06_gl_msaa_probe.txt) - the fixture is not the single-sample image"""
    for name in ("face40", "face224", "coarse"):
        one = SCENES1[name]["image_u8"][..., :3]
        four = SCENES[name]["rgb"]
        covered = SCENES1[name]["z"] < 1
        frac = float((one != four).any(-1).sum() / covered.sum())
        print(name, frac)
        assert 0.01 < frac < 0.15
