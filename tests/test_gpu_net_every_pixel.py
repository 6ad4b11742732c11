"""-m gpu: the network's final heatmaps against a float64 forward pass at every pixel, class by class (tests/net_reference.py).

The per-layer tests hold every tile to torch float64; the assembled network was held to the reference's vectors on a lattice of
one pixel in 256 (rows 5 mod 16, columns 3 mod 16: one of conv11's four parity forms, no border, no tile seam) at 2e-4 of scale,
sixty times the arithmetic's noise.  Here every configuration of the convolution path runs one forward pass of
`heatmaps_device`, and in every class of pixels - the border rows and columns, the four parities, the tile seams, the interior
- its max and mean distance from float64 must stay within `m` times the fp32 oracle's own distance from the same tensor:

  m = 3  two fp32 evaluations of the same sums in different orders.  The recorded HIP-to-oracle distance (at most 5.1e-6 of scale,
         profiles/r02..r06_parity_stats.txt) plus the oracle-to-float64 distance (at most 3.5e-6) is at most 2.5 times the latter by
         the triangle inequality; 3 is the next integer.
  m = 8  3 times the largest per-layer F(4,3)-over-direct error ratio on record (2.48, profiles/r10_wino4_error.txt), rounded up;
         it also covers the split-operand precisions, whose recorded heatmaps sit as far from the oracle as the exact path's.

No margin comes from a run of the code under test.  Each configuration proves from the profile records and the launch counters
of the very pass it compares that the intended kernels ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import net_reference as nr

pytestmark = pytest.mark.gpu

WINO = 40      # conv3x3w_*: the F(2,3) tile
WINO4 = 2048   # MVLM_CONV_VARIANT_WINO4: the F(4,3) tile, both workgroup shapes
CAP = 1024
ALL = list(nr.NETWORKS)
SEEDED = [n for n in ALL if "seeded" in n]


@pytest.fixture(scope="module")
def networks():
    """name -> (reference case with the float64 heatmaps and the oracle's table, predictor, images on the device); each network is
    evaluated in float64 once, a few seconds of CPU per view, and shared by every configuration."""
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    torch.set_num_threads(min(torch.get_num_threads(), 16))
    made = {}

    def get(name):
        if name not in made:
            case = nr.reference_case(name)
            w = nr.NETWORKS[name][2]
            cls = BU3DFEPredictor if case["nl"] == 84 else DTU3DPredictor
            pred = cls(image_mode=case["mode"], weights=case["sd"] if w == "planted-dense" else w, verbose=False)
            made[name] = (case, pred, torch.from_numpy(case["images"]).cuda())
        return made[name]

    return get


def _configure(pred, winograd=1, winograd4=1, wide=1, padded=1, pairing=1, precision="exact"):
    ctx = pred.ctx
    ctx.check(ctx.lib.mvlm_cnn_set_winograd(ctx.handle, winograd))
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4(ctx.handle, winograd4))
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4_wide(ctx.handle, wide))
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4_padded(ctx.handle, padded))
    pred.set_execution(graphs=True, pairing=pairing)
    if pred.precision != precision:
        pred.set_precision(precision)


def _counter(ctx, fn):
    n = C.c_int64()
    ctx.check(fn(ctx.handle, C.byref(n), 1))
    return int(n.value)


def _heatmaps_with_proof(pred, x):
    """One launch-by-launch pass of heatmaps_device: the heatmaps, the variant codes of its launches, and its launches on the wide
    shape and over padded weights."""
    ctx = pred.ctx
    pred.set_execution(graphs=False)
    ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 1))
    try:
        _counter(ctx, ctx.lib.mvlm_conv_wino4_wide_launches)
        _counter(ctx, ctx.lib.mvlm_conv_wino4_padded_launches)
        heat = pred.heatmaps_device(x).cpu().numpy()
        slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
        n = ctx.lib.mvlm_cnn_get_profile(ctx.handle, slot, var, (C.c_double * CAP)(), (C.c_float * CAP)(), CAP)
        assert 0 < n < CAP
        wide = _counter(ctx, ctx.lib.mvlm_conv_wino4_wide_launches)
        padded = _counter(ctx, ctx.lib.mvlm_conv_wino4_padded_launches)
        return heat, [var[i] for i in range(n)], wide, padded
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 0))
        pred.set_execution(graphs=True)


def _name(lib, v):
    return lib.mvlm_conv_variant_name(v).decode() if v >= 0 else ""


def _compare(networks, name, label, m, settings, proof):
    case, pred, x = networks(name)
    try:
        _configure(pred, **settings)
        heat, variants, wide, padded = _heatmaps_with_proof(pred, x)
        assert pred.precision == settings.get("precision", "exact") and pred.fast16_fallbacks == 0
        if pred.precision == "fast16":
            assert not pred.fast16_overflowed()
    finally:
        _configure(pred)
    lib = pred.ctx.lib
    on_f23 = [v for v in variants if v == WINO or _name(lib, v).startswith("conv3x3w_")]
    on_f43 = [v for v in variants if v == WINO4 or _name(lib, v).startswith("conv3x3q_")]
    print(f"\n{label} / {name}: {len(variants)} launches, {len(on_f23)} on the F(2,3) tile, {len(on_f43)} on the F(4,3) tile, "
          f"{wide} on its wide shape, {padded} over padded weights")
    proof(len(on_f23), len(on_f43), wide, padded)
    assert heat.shape == case["ref64"].shape
    table = nr.error_table(heat, case["ref64"])
    print(nr.format_table(f"{label} / {name}: HIP against float64, S = {case['scale']:.4g}, m = {m}", table, case["table_ref"], m))
    assert nr.check_against(table, case["table_ref"], m) == []


# ---- the exact-arithmetic configurations ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("pairing", [0, 1, 2])
def test_direct_path(networks, pairing, name):
    def proof(f23, f43, wide, padded):
        assert (f23, f43, wide, padded) == (0, 0, 0, 0)

    _compare(networks, name, f"direct, pairing {pairing}", 3, dict(winograd=0, pairing=pairing), proof)


@pytest.mark.parametrize("name", SEEDED)
def test_defaults(networks, name):
    _compare(networks, name, "defaults", 3, dict(), lambda *counts: None)


@pytest.mark.parametrize("name", SEEDED)
def test_f23_everywhere(networks, name):
    def proof(f23, f43, wide, padded):
        assert f23 >= 30 and (f43, wide, padded) == (0, 0, 0)

    _compare(networks, name, "F(2,3) everywhere", 8, dict(winograd=2, winograd4=0), proof)


@pytest.mark.parametrize("name", ALL)
def test_f43_everywhere_narrow(networks, name):
    def proof(f23, f43, wide, padded):
        assert f43 >= 30 and (wide, padded) == (0, 0)

    _compare(networks, name, "F(4,3) everywhere, narrow", 8, dict(winograd=1, winograd4=2, wide=0, padded=0), proof)


@pytest.mark.parametrize("name", ALL)
def test_f43_everywhere_wide_and_padded(networks, name):
    def proof(f23, f43, wide, padded):
        assert f43 >= 30 and wide >= 20 and padded >= 1

    _compare(networks, name, "F(4,3) everywhere, wide + padded", 8, dict(winograd=1, winograd4=2, wide=1, padded=2), proof)


# ---- the opt-in precisions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,name", [("fast", n) for n in SEEDED] + [("fast16", n) for n in ALL])
def test_opt_in_precision(networks, precision, name):
    _compare(networks, name, f'precision "{precision}"', 8, dict(precision=precision), lambda *counts: None)
