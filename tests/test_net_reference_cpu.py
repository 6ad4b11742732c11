"""The every-pixel comparison of tests/net_reference.py on the CPU: what the fp32 oracle itself measures against the float64
forward pass (the figures every bound of tests/test_gpu_net_every_pixel.py is a multiple of), and three subtle faults planted
into the oracle's heatmaps, each of which the class-wise rule names and the older lattice criterion passes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net_reference as nr


@pytest.mark.parametrize("name", list(nr.NETWORKS))
def test_the_oracle_against_float64(name):
    """The reference's own arithmetic, class by class.  Measured (max / mean, in units of max |ref64|): 73 RGB synthetic:1
    3.51e-6 / 4.37e-7, 84 RGB+depth synthetic:2 3.32e-6 / 4.20e-7; the dense planted detector (one view) 1.69e-4 / 1.55e-5 (its
    heatmaps are differences of order-one hinges, S = 0.282) - the class-wise rule scales with it."""
    case = nr.reference_case(name)
    t = case["table_ref"]
    print("\n" + nr.format_table(f"oracle fp32 against float64, {name}, S = {case['scale']:.4g}", t))
    assert list(t) == list(nr.pixel_classes())
    assert all(np.isfinite(e) and np.isfinite(mu) and 0 < mu <= e for e, mu in t.values())
    assert max(e for e, _ in t.values()) == t["all"][0]
    if "seeded" in name:
        assert t["all"][0] < 1e-5
    assert nr.check_against(t, t, 1) == []
    assert nr.lattice_criterion(case["oheat"], case["ref64"])


def test_pixel_classes():
    c = nr.pixel_classes()
    assert all(m.shape == (256, 256) and m.dtype == bool for m in c.values())
    assert c["row255"].sum() == 256 and c["col0"][:, 0].all() and c["all"].all()
    assert sum(c[k].sum() for k in nr.PARITY_CLASSES) == 65536 and c["par10"][1, 0] and c["par01"][0, 1]
    assert c["rowseam8"].sum() == 64 * 256 and c["colseam32"].sum() == 16 * 256
    assert c["seam64"][63, 5] and c["seam64"][5, 64] and not c["seam64"][62, 65]
    assert not (c["interior"] & (c["row1"] | c["col254"] | c["rowseam8"] | c["colseam32"] | c["seam64"])).any()
    assert c["interior"][2, 2] and c["interior"].sum() == (256 - 64 - 2) * (256 - 16 - 2)   # rows 1, 254 and columns 1, 254 besides the seams
    # the lattice of the older criterion: one parity, no border, no first or last row or column of a tile
    lat = np.zeros((256, 256), bool)
    lat[5::16, 3::16] = True
    assert lat.sum() == 256 and (lat & c["par11"]).sum() == 256 and (lat & c["interior"]).sum() == 256


# ---- planted faults ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv11_case():
    """The 73 / RGB network with conv11's input as the fp32 oracle computes it (the upsampled output of conv10)."""
    from oracle import cnn as ocnn

    case = nr.reference_case("73-rgb-seeded")
    seen = {}
    conv = ocnn._conv

    def spy(sd, prefix, x, pad):
        if prefix == "conv11":
            seen.setdefault("x", []).append(x.clone())
        return conv(sd, prefix, x, pad)

    ocnn._conv = spy
    try:
        again = nr.heatmaps_oracle(case["sd"], case["images"], case["sel"])
    finally:
        ocnn._conv = conv
    assert np.array_equal(again, case["oheat"])
    up = torch.cat(seen["x"], 0).contiguous()
    w, b = torch.from_numpy(case["sd"]["conv11.weight"]), torch.from_numpy(case["sd"]["conv11.bias"])
    assert up.shape == (2, 73, 256, 256)
    return case, up, w, b


def _row255_with_replicate_padding(heat, up, w, b):
    """conv11's last output row as if the row below the image repeated row 255 instead of being zero."""
    rows = F.pad(up[:, :, 254:256], (0, 0, 0, 1), mode="replicate")          # rows 254, 255, 255
    heat[:, :, 255] = F.conv2d(rows, w, b, 1, (0, 1))[:, :, 0].numpy()
    return np.s_[:, 255, :]


def _parity00_without_the_last_input_channel(heat, up, w, b):
    part = F.conv2d(up[:, :-1].contiguous(), w[:, :-1].contiguous(), b, 1, 1).numpy()
    heat[:, :, 0::2, 0::2] = part[:, :, 0::2, 0::2]
    return np.s_[:, 0::2, 0::2]


def _column32_of_one_plane_scaled(heat, up, w, b):
    v, k = np.unravel_index(np.abs(heat[:, :, :, 32]).max(axis=2).argmax(), heat.shape[:2])   # the plane whose column 32 is largest
    heat[v, k, :, 32] *= np.float32(1 + 1e-4)
    return np.s_[:, :, 32]


# fault -> (how to plant it, classes that must be flagged, gross: every class holding a faulty pixel must be flagged)
FAULTS = {
    "row255-replicate": (_row255_with_replicate_padding, {"row255"}, True),
    "par00-channel": (_parity00_without_the_last_input_channel, {"par00", "interior", "all"}, True),
    "col32-scaled": (_column32_of_one_plane_scaled, {"colseam32", "seam64"}, False),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_named_and_the_lattice_does_not_see_it(conv11_case, fault):
    """A fault planted into the fp32 oracle's heatmaps.  check_against(m = 3) must flag every class named for the fault and no
    class without a faulty pixel.  The classes overlap - row 255 is also a row seam, of parities (1, *) and holds a pixel of
    every border column - so the two gross faults must be flagged in exactly the classes that hold a faulty pixel; the subtle
    one (1e-4 of one column's values) in its seams at least, and in a border row only where that row's pixel of the column is
    large.  The lattice criterion at 2e-4 passes all three - it reads rows 5 mod 16 and columns 3 mod 16 only, which is the gap
    the every-pixel tests close."""
    case, up, w, b = conv11_case
    plant, named, gross = FAULTS[fault]
    heat = case["oheat"].copy()
    where = plant(heat, up, w, b)
    touched = np.zeros((1, 256, 256), bool)
    touched[where] = True
    changed = (heat != case["oheat"]).any(axis=(0, 1))
    assert changed.any() and not (changed & ~touched[0]).any()
    table = nr.error_table(heat, case["ref64"])
    found = nr.check_against(table, case["table_ref"], 3)
    flagged = {k for k, *_ in found}
    print("\n" + nr.format_table(f"fault {fault}", table, case["table_ref"], 3))
    print(f"flagged: {sorted(flagged)}")
    with_faulty_pixels = {k for k, m in nr.pixel_classes().items() if (m & changed).any()}
    assert named <= flagged, (fault, sorted(flagged))
    assert flagged <= with_faulty_pixels, (fault, sorted(flagged - with_faulty_pixels))
    assert not gross or flagged == with_faulty_pixels, (fault, sorted(with_faulty_pixels - flagged))
    for k, stat, value, bound in found:
        assert value > bound and stat in ("max", "mean")
    # the lattice criterion against float64 and, as the GPU tests state it, against the reference's vectors = the oracle's heatmaps
    assert nr.lattice_criterion(heat, case["ref64"]) and nr.lattice_criterion(heat, case["oheat"])
