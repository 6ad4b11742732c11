"""-m gpu: the 84- and 80-row layers (conv6 / conv10: 3x3 + bias, cout_pad no multiple of 32) on the F(4,3) Winograd tile over weights
padded to whole 32-channel columns (conv_mfma.hip: f43_plan, mvlm_cnn_set_winograd4_padded).

The dispatcher still names variant 26 / 16 for them and then runs the launch on the tile (f43_plan).  Single layers against torch
float64 with the switch at 2 (the bound of test_gpu_winograd4.py for the tile), the gates that leave the direct tile's launches and
bits alone, the 84-landmark network at 2 views with its profile records and a replayed graph, and the benchmark's size once with
the default switch against switch 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import seeded_images

pytestmark = pytest.mark.gpu

WINO4 = 2048  # MVLM_CONV_VARIANT_WINO4
CAP = 1024
SENTINEL = -12345.5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set(ctx, winograd=1, winograd4=1, padded=1):
    ctx.check(ctx.lib.mvlm_cnn_set_winograd(ctx.handle, winograd))
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4(ctx.handle, winograd4))
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4_padded(ctx.handle, padded))


def _count(ctx):
    """padded launches since the last call"""
    n = C.c_int64()
    ctx.check(ctx.lib.mvlm_conv_wino4_padded_launches(ctx.handle, C.byref(n), 1))
    return int(n.value)


def _conv2d(ctx, x, w, bias, force=-1, extra_images=0):
    """plain 3x3 (+ bias) through mvlm_conv2d; `extra_images` sentinel images behind the last one of the output buffer"""
    batch, cin, size, _ = x.shape
    cout = w.shape[0]
    xd = dev(x)
    yd = torch.full((batch + extra_images, cout, size, size), SENTINEL, dtype=torch.float32, device="cuda")
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, force))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(xd.data_ptr()), batch, cin, size, size, p(w), cout, 3, p(bias),
                                      None, None, None, None, None, 0, C.c_void_p(yd.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    return yd.cpu().numpy()


def _layer_data(cin, cout, size, batch, with_bias):
    rs = np.random.RandomState(cin * 7 + cout + size)
    x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    bias = rs.standard_normal(cout).astype(np.float32) if with_bias else None
    want = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                                      None if bias is None else torch.from_numpy(bias).double(), 1, 1).numpy()
    return x, w, bias, want


# --------------------------------------------------------------------------------------------------------------------------
# 1. single layers, switch 2, against torch float64; the direct tile's error (switch 0) beside it.
# (8, 84, 32, 1): two chunks (no steady loop), every border in one workgroup, the last column of workgroups holds 20 live channels
# of 32; (73, 84, 64, 3): a padded last chunk, interior tile edges, several images - a store past channel 83 of an image lands in
# the next image (or in the sentinel image behind the last) and shows in the compare; (256, 84, 32, 1): the LDS BatchNorm table's
# limit; (64, 73, 32, 2): cout_pad 80, the 80-row tile (variant 16), 9 live channels in the last column.
# Without a bias mvlm_conv2d packs 84 channels as cout_pad 96 (the 84-row tile is a conv + bias tile), and the dispatcher itself
# sends the layer to the tile under F(4,3) mode 2: the same kernel, cout 84 of cout_pad 96, no bias vector; no padded launch.
LAYER_CASES = [
    # cin, cout, size, batch, bias, padded launches expected
    (8, 84, 32, 1, True, 1),
    (73, 84, 64, 3, True, 1),
    (256, 84, 32, 1, True, 1),
    (8, 84, 32, 1, False, 0),
    (64, 73, 32, 2, True, 1),
]


@pytest.mark.parametrize("cin,cout,size,batch,with_bias,launches", LAYER_CASES)
def test_padded_layer_matches_torch(cin, cout, size, batch, with_bias, launches):
    from mvlm_amd import _lib

    ctx = _lib.get_context(0)
    x, w, bias, want = _layer_data(cin, cout, size, batch, with_bias)
    tol = 5e-6 * max(1.0, np.abs(want).max())
    try:
        _set(ctx, 1, 1 if with_bias else 2, 2)
        _count(ctx)
        got = _conv2d(ctx, x, w, bias, extra_images=1)
        n = _count(ctx)
        _set(ctx, 1, 1, 0)
        direct = _conv2d(ctx, x, w, bias)
        assert _count(ctx) == 0
    finally:
        _set(ctx)
    err_w, err_d = np.abs(got[:batch] - want).max(), np.abs(direct - want).max()
    print(f"\nwinograd4-padded-error {cin}->{cout} @{size} B{batch} bias {with_bias}: F(4,3) padded {err_w:.3e} direct {err_d:.3e} "
          f"ratio {err_w / err_d:.2f} bound {tol:.3e}; {n} padded launches")
    assert n == launches
    assert np.all(got[batch:] == SENTINEL)  # nothing behind the last image was written
    assert err_w < tol
    assert err_d < tol


# 2. the gates on a single layer: the output is the direct tile's, bit for bit, and nothing is handed over
@pytest.mark.parametrize("cin,cout,size,batch", [(73, 84, 64, 3), (64, 73, 32, 2)])
def test_gated_layer_is_the_direct_tile_bit_for_bit(cin, cout, size, batch):
    from mvlm_amd import _lib

    ctx = _lib.get_context(0)
    variant = 26 if cout == 84 else 16
    x, w, bias, _ = _layer_data(cin, cout, size, batch, True)
    try:
        _set(ctx, 0, 1, 0)
        _count(ctx)
        parent = _conv2d(ctx, x, w, bias, force=variant)  # the direct tile, as the parent ran this layer
        for name, modes, force in [("switch 0", (1, 1, 0), -1), ("F(4,3) mode 0", (1, 0, 2), -1), ("Winograd mode 0", (0, 1, 2), -1),
                                   ("variant forced", (1, 1, 2), variant)]:
            _set(ctx, *modes)
            got = _conv2d(ctx, x, w, bias, force=force)
            assert _count(ctx) == 0, name
            assert np.array_equal(got, parent), name
        # the hold of the table: every row starts at 96 views, so switch 1 hands nothing over at this batch
        _set(ctx, 1, 1, 1)
        got = _conv2d(ctx, x, w, bias)
        assert _count(ctx) == 0 and np.array_equal(got, parent)
        _set(ctx, 1, 1, 2)
        got = _conv2d(ctx, x, w, bias)
        assert _count(ctx) == 1 and not np.array_equal(got, parent)  # (the tile rounds differently: the gates above gated something)
        lib = ctx.lib
        assert lib.mvlm_cnn_set_winograd4_padded(ctx.handle, 3) != 0 and lib.mvlm_cnn_set_winograd4_padded(ctx.handle, -1) != 0
    finally:
        _set(ctx)


# --------------------------------------------------------------------------------------------------------------------------
def _predictor(nl, mode, seed):
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    return (BU3DFEPredictor if nl == 84 else DTU3DPredictor)(image_mode=mode, weights=f"synthetic:{seed}", verbose=False)


def _profile(pred, x):
    """(slot, variant, flops, shape[6]) of one launch-by-launch pass"""
    ctx = pred.ctx
    pred.set_execution(graphs=False)
    ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 1))
    try:
        pred.predict_device(x)
        slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
        fl, ms = (C.c_double * CAP)(), (C.c_float * CAP)()
        n = ctx.lib.mvlm_cnn_get_profile(ctx.handle, slot, var, fl, ms, CAP)
        assert 0 < n < CAP
        shapes = (C.c_int32 * (6 * CAP))()
        assert ctx.lib.mvlm_cnn_get_profile_shapes(ctx.handle, shapes, CAP) == n
        return [(slot[i], var[i], fl[i], tuple(shapes[6 * i:6 * i + 6])) for i in range(n)]
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 0))
        pred.set_execution(graphs=True)


def _rows84(recs):
    """the records of conv6 and conv10: 3x3, 256 -> 84 rows"""
    return [r for r in recs if r[0] >= 0 and r[3][0] == 3 and r[3][2] == 84]


def _near_tie_ok(heat_plane, got_rc, want_rc, rel=2e-4):  # (the rule of test_gpu_winograd4.py)
    gv = heat_plane[int(got_rc[0]) + 1, int(got_rc[1] + 0.5)]
    wv = heat_plane[int(want_rc[0]) + 1, int(want_rc[1] + 0.5)]
    return abs(gv - wv) <= rel * max(abs(wv), 1.0)


# 3. the 84-landmark network at 2 views, switch 2 against switch 0 (criteria of test_network_on_the_winograd4_tile_against_the_direct_path);
# at this size no other launch is on the F(4,3) tile (its table starts at 96 views), so conv6 and conv10 are all that differs
def test_network_with_conv6_and_conv10_on_the_tile():
    from oracle import cnn as ocnn

    pred = _predictor(84, "RGB+depth", 4)
    ctx = pred.ctx
    x = dev(seeded_images(21, 2))
    try:
        _set(ctx, 1, 1, 0)
        _count(ctx)
        recs0 = _profile(pred, x)
        heat0 = pred.heatmaps_device(x).cpu().numpy()
        lms0 = pred.predict_device(x).cpu().numpy()
        assert _count(ctx) == 0
        assert [r[1] for r in _rows84(recs0)] == [26, 26] and not [r for r in recs0 if r[1] == WINO4]
        _set(ctx, 1, 1, 2)
        recs2 = _profile(pred, x)
        assert _count(ctx) == 2
        # honest records: code 2048 and 4.5 taps' worth of FLOPs where the direct tile's record counts 9; every other record as it was
        assert [r[1] for r in _rows84(recs2)] == [WINO4, WINO4]
        assert [r[2] for r in _rows84(recs2)] == [0.5 * r[2] for r in _rows84(recs0)]
        assert [(r[0], r[3]) for r in recs2] == [(r[0], r[3]) for r in recs0]
        assert [r[:3] for r in recs2 if r[3][2] != 84] == [r[:3] for r in recs0 if r[3][2] != 84]
        heat2 = pred.heatmaps_device(x).cpu().numpy()
        scale = np.abs(heat0).max()
        d = np.abs(heat2 - heat0).max()
        print(f"\nwinograd4-padded-network: max |padded - direct| = {d:.3e} = {d / scale:.2e} of scale")
        assert 0 < d < 2e-4 * scale
        # the captured graph's replay: passes over the same buffers return the first pass's tensor
        pred.set_execution(graphs=True)
        out = torch.empty((84, 2, 3), dtype=torch.float32, device="cuda")
        s0 = pred.execution_stats()
        _count(ctx)
        first = pred.predict_device(x, out=out).clone()
        for _ in range(3):
            again = pred.predict_device(x, out=out)
            assert torch.equal(again, first)
        s1 = pred.execution_stats()
        assert s1["graph_replays"] > s0["graph_replays"] and s1["graph_failures"] == 0, (s0, s1)
        assert _count(ctx) == 4  # the eager pass and the capture issued two each; a replay issues none
        lms2 = first.cpu().numpy()
        np.testing.assert_array_equal(lms2, ocnn.maxima_fast(torch.from_numpy(heat2)))
        for lm, v in zip(*np.nonzero(~np.all(lms2[:, :, :2] == lms0[:, :, :2], axis=2))):
            assert _near_tie_ok(heat0[v, lm], lms2[lm, v], lms0[lm, v]), (lm, v)
        # the gates through the network: the same modes with the switch at 0 give the same tensor and records, nothing handed over
        for modes in [(1, 0, 2), (0, 1, 2)]:
            _set(ctx, *modes)
            recs = _profile(pred, x)
            y = pred.predict_device(x).clone()
            assert _count(ctx) == 0, modes
            assert [r[1] for r in _rows84(recs)] == [26, 26], modes
            _set(ctx, modes[0], modes[1], 0)
            assert [r[:3] for r in _profile(pred, x)] == [r[:3] for r in recs], modes
            assert torch.equal(pred.predict_device(x), y), modes
        # the hold: the default switch hands nothing over at 2 views
        _set(ctx, 1, 1, 1)
        assert torch.equal(pred.predict_device(x), torch.from_numpy(lms0).cuda()) and _count(ctx) == 0
    finally:
        _set(ctx)
        pred.set_execution(graphs=True)


# 4. the benchmark's size, the default switch against switch 0: acceptance of
# test_bench_sized_agreement_of_the_default_modes_with_the_direct_path
def test_bench_sized_agreement_of_the_default_switch_with_switch_0():
    from mvlm_amd import pipeline
    from mvlm_amd.utils.synthetic import face_like_mesh

    n = 96
    pipe = pipeline.create_pipeline("bu3dfe", n_views=n, weights="synthetic:0", verbose=False)
    pred = pipe.predictor_2d
    ctx = pred.ctx
    mesh = face_like_mesh(224, 512, seed=0)
    np.random.seed(3)
    poses = pipe.renderer_3d.generate_3d_transformations()
    state = np.random.get_state()
    images = pipe.renderer_3d.render_device(mesh, poses)
    out, count = {}, {}
    try:
        pred.set_execution(graphs=False)
        for sw in (0, 1):
            _set(ctx, 1, 1, sw)
            np.random.set_state(state)
            lm3d, _ = pipe.predict_mesh_device(mesh, poses)
            _count(ctx)
            out[sw] = (pred.predict_device(images).cpu().numpy(), np.asarray(lm3d))
            count[sw] = _count(ctx)  # (the launches of one pass)
        rows = _rows84(_profile(pred, images))
    finally:
        _set(ctx)
        pred.set_execution(graphs=True)
    nl = out[0][0].shape[0]
    differ = ~np.all(out[0][0][:, :, :2] == out[1][0][:, :, :2], axis=2)  # [NL, N]
    print(f"\nwinograd4-padded-bench-size: {count[1]} padded launches per pass with the default switch, {count[0]} at 0; "
          f"{int(differ.sum())} of {nl * n} planes with another argmax pixel")
    assert count == {0: 0, 1: 2}, count
    assert [r[1] for r in rows] == [WINO4, WINO4]
    assert differ.sum() <= 0.002 * nl * n
    if differ.any():
        _set(ctx, 1, 1, 0)
        try:
            for lm, v in zip(*np.nonzero(differ)):
                plane = pred.heatmaps_device(images[v:v + 1])[0, lm].cpu().numpy()
                assert _near_tie_ok(plane, out[1][0][lm, v], out[0][0][lm, v]), (lm, v)
        finally:
            _set(ctx)
    same = ~differ.any(axis=1)
    d = np.abs(out[0][1] - out[1][1]).max(axis=1)
    print(f"winograd4-padded-bench-size: landmarks with identical planes {int(same.sum())}/{nl}, max |default - switch 0| = {d[same].max():.3e} model units")
    assert d[same].max() < 1e-3
