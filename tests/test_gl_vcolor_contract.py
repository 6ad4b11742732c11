"""The per-vertex-colour contract against a real OpenGL.

tests/golden/gl_raster_vcolor.npz = four scenes of gl_raster.npz with colours of their own, one of them also through a 4-sample
target, and two probes (a 0 -> 255 ramp; strips whose colour rises by one code value, stepping through k + 1/2 in units of
1/3840), drawn by SwiftShader's OpenGL ES 3.0 the way VTK's mapper draws point scalars (tools/make_gl_vcolor_golden.py).  This
file holds the CPU model of the contract (tests/native/vcolor_raster.c), at the GL's sub-pixel bits, against it;
tests/test_gpu_vertex_colors.py holds the HIP rasteriser against the model and against the fixture.  tests/vcolor_contract.py
explains the classes a disagreement may fall into.

The class bounds are the measured ones.  One condition was fixed before anything was measured: `interp` may hold at most 2 % of
a scene's covered pixels - two float evaluations of one plane disagree in a byte only where the exact value lies within their
error of a conversion boundary.  With round-to-nearest as the conversion the shares were 0.63 % (face40, coarse) to 3.47 %
(centres, over the cap), every one of them at an exact value within 1/512 of k + 1/2, rounded down from 128 on and up below:
the rule was wrong, not the cap.  The fine probe shows the GL's rule - 16-bit fixed point, truncated - and with it the shares
are 0 but for ONE pixel of coarse."""
import numpy as np
import pytest

import vcolor_contract
import vcolor_model

META, SCENES = vcolor_contract.load()
GL_BITS = META["gl"]["subpixel_bits"]

# measured with the model at the GL's own sub-pixel precision: {scene: (clip, interp, ztie)} upper bounds
MEASURED = {
    "face40": (0, 0, 0), "coarse": (0, 1, 0), "offscreen": (8, 0, 0), "centres": (0, 0, 0), "ramp": (0, 0, 0), "fine": (0, 0, 0),
    "face40_ms4": (0, 0, 1),
}
INTERP_CAP = 0.02      # of a scene's covered pixels; fixed in advance (see above)


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    vcolor_model.load(tmp_path_factory.mktemp("vcolor_model"))
    return {name: vcolor_model.render(sc["verts"], sc["tris"], None, None, sc["poses"], subpixel_bits=GL_BITS, samples=sc["samples"],
                                      colors=sc["colors"]) for name, sc in SCENES.items()}


def test_the_golden_file_is_what_the_generator_found():
    f = META["findings"]
    assert META["gl"]["renderer"] == "Google SwiftShader" and GL_BITS == 4 and META["samples"] == {"face40_ms4": 4}
    rule = f["colour_to_byte"]
    assert rule == "16-bit fixed point: c16 = trunc(65535 f), (c16 - (c16 >> 8) + 128) >> 8"
    hits, fine = f["colour_to_byte_hits"], f["colour_to_byte_fine_hits"]
    assert hits[rule] == f["colour_to_byte_pixels"] == 3 * 65536                       # every byte of the ramp
    assert fine[rule] == f["colour_to_byte_fine_pixels"] == 184272                     # and of the fine probe
    # no other rule explains both: the ramp cannot tell round-to-nearest from it (no value within 1/512 of a boundary), the
    # fine probe does
    assert hits["round to nearest: (int)(255 f + 0.5)"] == 3 * 65536 and fine["round to nearest: (int)(255 f + 0.5)"] == fine[rule] - 356
    for other in ("truncate: (int)(255 f)", "round up: ceil(255 f)"):
        assert hits[other] < 0.6 * 3 * 65536 and fine[other] < 0.6 * fine[rule]
    assert set(SCENES) == set(MEASURED)
    assert vcolor_contract.GOLDEN.stat().st_size < 1 << 20
    for name, sc in SCENES.items():
        assert sc["colors"].dtype == np.uint8 and sc["colors"].shape == (len(sc["verts"]), 3), name
        assert sc["rgb"].shape == (len(sc["poses"]), 256, 256, 3), name
    tris = SCENES["centres"]
    a, b, c = (tris["verts"][tris["tris"][:, k], :2].astype(np.float64) for k in range(3))
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    assert (area < 0).sum() >= 5 and (area > 0).sum() >= 5                              # the clockwise-wound scene


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_model_against_opengl(renders, name):
    r = vcolor_contract.compare(SCENES[name], renders[name], GL_BITS)
    print(name, r, f"interp share {r['interp'] / r['covered']:.4%}")
    assert r["unexplained"] == 0, r
    clip, interp, ztie = MEASURED[name]
    assert r["clip"] <= clip and r["interp"] <= interp and r["ztie"] <= ztie, r
    # the fixture is not the uncoloured image
    assert r["coloured"] > 0.5 * r["covered"], r


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_interp_stays_under_the_cap_fixed_in_advance(renders, name):
    """measured interp / covered: coarse 1 / 93 688; 0 on every other scene (offscreen's 8 differing pixels are `clip`)"""
    r = vcolor_contract.compare(SCENES[name], renders[name], GL_BITS)
    assert r["interp"] <= INTERP_CAP * r["covered"], (name, r["interp"], r["covered"], r["interp"] / r["covered"])


def test_the_probes_are_reproduced_exactly(renders):
    fine = np.round(renders["fine"] * 255).astype(np.uint8)
    np.testing.assert_array_equal(fine[..., :3], SCENES["fine"]["rgb"])
    got = np.round(renders["ramp"] * 255).astype(np.uint8)
    np.testing.assert_array_equal(got[..., :3], SCENES["ramp"]["rgb"])
    assert len(np.unique(got[0, 0, :, 0])) == 256 and len(np.unique(got[0, :, 0, 1])) == 256   # every byte value, per channel
