"""-m gpu: the wide workgroup shape of the F(4,3) Winograd tile (conv_variants.h: MVLM_CONV_WINO4_WIDE_CFG, 64 output channels x 8 rows
x 32 pixels; mvlm_cnn_set_winograd4_wide / MVLM_WINOGRAD4_WIDE).

The shape stages an input tile once for 64 output channels and leaves the arithmetic of every output element alone - same products,
same K order, same transforms, same epilogue - so everything here is a comparison for equality, bit for bit, with the switch at 0:
single layers with code 2048 forced, the network with every servable layer on the tile, the default modes at the benchmark's size,
the setter, the environment default and the captured graphs, and the first launches of the two shapes in a fresh process."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import REPO, seeded_images

pytestmark = pytest.mark.gpu

WINO4 = 2048  # MVLM_CONV_VARIANT_WINO4: the code of both shapes
CAP = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set_wide(ctx, on):
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4_wide(ctx.handle, on))


def _wide_count(ctx, reset=True):
    """launches this context issued on the wide shape since the last reset"""
    n = C.c_int64()
    ctx.check(ctx.lib.mvlm_conv_wino4_wide_launches(ctx.handle, C.byref(n), int(reset)))
    return int(n.value)


# --------------------------------------------------------------------------------------------------------------------------
# 1. code 2048 forced through mvlm_conv2d, the switch at 1 against the switch at 0, the whole output.
# size 32, batch 1: four row tiles of the wide shape, every border, a top and a bottom quad in each; size 64, batch 3: interior tile
# edges and more than one image.  cin 4: one chunk, 8: two (no steady loop), 20: an odd count, 73 -> 76: a padded last chunk,
# 256: the LDS BatchNorm table's limit.  cout 64: one cout tile, 128: co0 != 0.  Options: those of test_gpu_winograd4.py::LAYER_CASES.
OPTION_SETS = [dict(), dict(pre=True, res=True), dict(bias=True, post=True)]
LAYERS = list(itertools.product([(32, 1), (64, 3)], [4, 8, 20, 73, 256], [64, 128], range(len(OPTION_SETS))))


def _tensors(cin, cout, size, batch, opts):
    rs = np.random.RandomState(cin * 7 + cout + size)
    x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    bias = rs.standard_normal(cout).astype(np.float32) if opts.get("bias") else None
    pre = (rs.uniform(0.5, 1.5, cin).astype(np.float32), rs.standard_normal(cin).astype(np.float32) * 0.3) if opts.get("pre") else None
    post = (rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.standard_normal(cout).astype(np.float32) * 0.3) if opts.get("post") else None
    res = rs.standard_normal((batch, cout, size, size)).astype(np.float32) if opts.get("res") else None
    return x, w, bias, pre, post, res


def _layer(ctx, xd, w, bias, pre, post, rd):
    batch, cin, size, _ = xd.shape
    cout = w.shape[0]
    yd = torch.full((batch, cout, size, size), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, WINO4))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(xd.data_ptr()), batch, cin, size, size, p(w), cout, 3, p(bias),
                                      p(pre[0]) if pre else None, p(pre[1]) if pre else None,
                                      p(post[0]) if post else None, p(post[1]) if post else None,
                                      C.c_void_p(rd.data_ptr()) if rd is not None else None, 0, C.c_void_p(yd.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    return yd.cpu().numpy()


def _both_shapes(cin, cout, size, batch, opts):
    """the layer's output with the switch at 1 and at 0, and the wide launches counted under each"""
    from mvlm_amd import _lib

    ctx = _lib.get_context(0)
    x, w, bias, pre, post, res = _tensors(cin, cout, size, batch, opts)
    xd, rd = dev(x), (dev(res) if res is not None else None)
    out, count = {}, {}
    try:
        for on in (1, 0):
            _set_wide(ctx, on)
            _wide_count(ctx)
            out[on] = _layer(ctx, xd, w, bias, pre, post, rd)
            count[on] = _wide_count(ctx)
    finally:
        _set_wide(ctx, 1)
    return out, count


@pytest.mark.parametrize("size_batch,cin,cout,opt", LAYERS)
def test_forced_layer_on_the_wide_shape_is_the_narrow_shape_bit_for_bit(size_batch, cin, cout, opt):
    size, batch = size_batch
    out, count = _both_shapes(cin, cout, size, batch, OPTION_SETS[opt])
    assert count == {1: 1, 0: 0}, count  # one launch per call on the wide shape, none with the switch off
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[1], out[0])


@pytest.mark.parametrize("cout", [32, 96])
def test_output_channels_that_do_not_come_in_64s_run_narrow_under_either_setting(cout):
    out, count = _both_shapes(20, cout, 32, 1, OPTION_SETS[1])
    assert count == {1: 0, 0: 0}, count
    assert np.isfinite(out[0]).all() and np.array_equal(out[1], out[0])


def test_the_query_names_the_shapes_the_wide_launch_takes():
    from mvlm_amd import _lib

    lib = _lib.load()
    assert lib.mvlm_conv_wino4_wide_serves(3, 256, 128, 128) and lib.mvlm_conv_wino4_wide_serves(3, 4, 64, 32)
    assert not lib.mvlm_conv_wino4_wide_serves(3, 64, 32, 64) and not lib.mvlm_conv_wino4_wide_serves(3, 64, 96, 64)  # cout_pad % 64
    assert not lib.mvlm_conv_wino4_wide_serves(3, 256, 128, 16) and not lib.mvlm_conv_wino4_wide_serves(1, 256, 128, 64)  # not the tile's
    assert not lib.mvlm_conv_wino4_wide_serves(3, 320, 64, 64)


# --------------------------------------------------------------------------------------------------------------------------
def _predictor(nl, mode, seed, **kw):
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    return (BU3DFEPredictor if nl == 84 else DTU3DPredictor)(image_mode=mode, weights=f"synthetic:{seed}", verbose=False, **kw)


def _set_modes(pred, winograd, winograd4):
    pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd(pred.ctx.handle, winograd))
    pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd4(pred.ctx.handle, winograd4))


def _profile_keys(pred, x):
    """(variant, (ksize, cin_pad, cout_pad, size, kind, batch)) of every launch of one launch-by-launch pass"""
    ctx = pred.ctx
    ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 1))
    try:
        pred.predict_device(x)
        slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
        n = ctx.lib.mvlm_cnn_get_profile(ctx.handle, slot, var, (C.c_double * CAP)(), (C.c_float * CAP)(), CAP)
        assert 0 < n < CAP
        shapes = (C.c_int32 * (6 * CAP))()
        assert ctx.lib.mvlm_cnn_get_profile_shapes(ctx.handle, shapes, CAP) == n
        return [(var[i], tuple(shapes[6 * i:6 * i + 6])) for i in range(n)]
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 0))


# 2. plain, scattering and pooling layers through the network, every servable layer on the tile (F(4,3) mode 2)
@pytest.mark.parametrize("nl,mode", [(73, "RGB"), (84, "RGB+depth")])
def test_network_on_the_wide_shape_is_the_narrow_shape_bit_for_bit(nl, mode):
    pred = _predictor(nl, mode, 4)
    ctx, lib = pred.ctx, pred.ctx.lib
    x = dev(seeded_images(21, 2))
    out, count = {}, {}
    try:
        _set_modes(pred, 1, 2)
        pred.set_execution(graphs=False)
        for on in (1, 0):
            _set_wide(ctx, on)
            heat = pred.heatmaps_device(x)
            _wide_count(ctx)
            out[on] = (heat, pred.predict_device(x))
            count[on] = _wide_count(ctx)  # (the launches of one pass)
        _set_wide(ctx, 1)
        keys = _profile_keys(pred, x)
    finally:
        _set_wide(ctx, 1)
        _set_modes(pred, 1, 1)
        pred.set_execution(graphs=True)
    wide = [k for v, k in keys if v == WINO4 and lib.mvlm_conv_wino4_wide_serves(k[0], k[1], k[2], k[3])]
    print(f"\nwinograd4-wide-network {nl} {mode}: {count[1]} launches of a pass on the wide shape, "
          f"{len([1 for v, _ in keys if v == WINO4])} on code 2048, kinds {sorted({k[4] for k in wide})}")
    assert count[0] == 0 and count[1] >= 20, count
    assert count[1] <= len(wide)  # the query names every launch that can take the wide shape (conv_wino4_wide_hold.h keeps some narrow)
    assert {0, 1, 2} <= {k[4] for k in wide}, sorted({k[4] for k in wide})
    assert torch.equal(out[1][0], out[0][0])
    assert torch.equal(out[1][1], out[0][1])


# 3. the benchmark's size, the default modes: set up as test_bench_sized_agreement_of_the_default_modes_with_the_direct_path
def test_bench_sized_pass_on_the_wide_shape_is_the_narrow_shape_bit_for_bit():
    from mvlm_amd import pipeline
    from mvlm_amd.utils.synthetic import face_like_mesh

    n = 96
    pipe = pipeline.create_pipeline("bu3dfe", n_views=n, weights="synthetic:0", verbose=False)
    pred = pipe.predictor_2d
    mesh = face_like_mesh(224, 512, seed=0)
    np.random.seed(3)
    poses = pipe.renderer_3d.generate_3d_transformations()
    state = np.random.get_state()
    images = pipe.renderer_3d.render_device(mesh, poses)
    out, count = {}, {}
    try:
        for on in (1, 0):
            _set_wide(pred.ctx, on)
            _wide_count(pred.ctx)
            np.random.set_state(state)
            lm3d, _ = pipe.predict_mesh_device(mesh, poses)
            out[on] = (pred.predict_device(images), np.asarray(lm3d))
            count[on] = _wide_count(pred.ctx)
    finally:
        _set_wide(pred.ctx, 1)
    print(f"\nwinograd4-wide-bench-size: {count[1]} launches issued on the wide shape with the switch at 1, {count[0]} at 0")
    assert count[1] > 0 and count[0] == 0, count
    assert torch.equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])


# 4. the setter's range, the environment default, and the captured graphs
def test_setter_environment_default_and_captured_graphs():
    x = dev(seeded_images(9, 2))
    a = _predictor(84, "RGB+depth", 6)
    lib = a.ctx.lib
    saved = os.environ.get("MVLM_WINOGRAD4_WIDE")
    os.environ["MVLM_WINOGRAD4_WIDE"] = "0"
    try:
        b = _predictor(84, "RGB+depth", 6)
    finally:
        if saved is None:
            del os.environ["MVLM_WINOGRAD4_WIDE"]
        else:
            os.environ["MVLM_WINOGRAD4_WIDE"] = saved
    try:
        for p in (a, b):
            _set_modes(p, 1, 2)
            p.set_execution(graphs=False)
            _wide_count(p.ctx)
        ya, yb = a.predict_device(x), b.predict_device(x)
        assert _wide_count(a.ctx) >= 20 and _wide_count(b.ctx) == 0  # b: the parent's kernels on every launch
        assert torch.equal(ya, yb)
        assert lib.mvlm_cnn_set_winograd4_wide(a.ctx.handle, 2) != 0 and lib.mvlm_cnn_set_winograd4_wide(a.ctx.handle, -1) != 0
        assert a.predict_device(x) is not None and _wide_count(a.ctx) >= 20  # a refused value changes nothing
        # a graph captured under one setting is not replayed under the other: the pass after a change is issued launch by launch
        # again (the first use of a key), on the other shape's kernels
        a.set_execution(graphs=True)
        for _ in range(3):
            y1 = a.predict_device(x)
        s1 = a.execution_stats()
        assert s1["graph_captures"] >= 1 and s1["graph_replays"] >= 1 and s1["graph_failures"] == 0, s1
        _set_wide(a.ctx, 0)
        _wide_count(a.ctx)
        y0 = a.predict_device(x)
        s0 = a.execution_stats()
        assert s0["graph_replays"] == s1["graph_replays"] and s0["eager_runs"] == s1["eager_runs"] + 1, (s1, s0)
        for _ in range(2):
            y0 = a.predict_device(x)
        s2 = a.execution_stats()
        assert s2["graph_captures"] == s1["graph_captures"] + 1 and s2["graph_replays"] > s0["graph_replays"], (s1, s2)
        assert _wide_count(a.ctx) == 0  # neither the eager pass nor the new capture issued a wide launch
        assert torch.equal(y1, y0) and torch.equal(y1, ya)
    finally:
        for p in (a, b):
            _set_wide(p.ctx, 1)
            _set_modes(p, 1, 1)
            p.set_execution(graphs=True)


# 5. the two shapes' launch attributes are remembered apart (a fresh process: a kernel's attributes, once set, hold for every
# context of the process, so only there does the first launch of each kernel show whether its own were set)
_SHAPE_ORDER = r"""
import ctypes as C, sys
import numpy as np, torch
from mvlm_amd import _lib
ctx = _lib.Context(0)
f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
rs = np.random.RandomState(0)
x = torch.randn(1, 8, 32, 32, device="cuda")
w = (rs.standard_normal((64, 8, 3, 3)) * 0.1).astype(np.float32)
def tile(wide):
    y = torch.full((1, 64, 32, 32), float("nan"), device="cuda")
    n = C.c_int64()
    ctx.check(ctx.lib.mvlm_cnn_set_winograd4_wide(ctx.handle, wide))
    ctx.check(ctx.lib.mvlm_conv_wino4_wide_launches(ctx.handle, None, 1))
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, 2048))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(x.data_ptr()), 1, 8, 32, 32, f(w), 64, 3, None, None, None, None, None, None, 0, C.c_void_p(y.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    ctx.check(ctx.lib.mvlm_conv_wino4_wide_launches(ctx.handle, C.byref(n), 1))
    assert n.value == wide, (wide, n.value)
    return y
ys = [tile(1), tile(0)] if sys.argv[1] == "wide-first" else [tile(0), tile(1)]
want = torch.nn.functional.conv2d(x, torch.from_numpy(w).cuda(), None, 1, 1)
errs = [(y - want).abs().max().item() for y in ys]
assert max(errs) < 1e-3, errs
assert torch.equal(ys[0], ys[1])
print("ok", errs)
"""


@pytest.mark.parametrize("order", ["wide-first", "narrow-first"])
def test_the_two_shapes_keep_their_launch_attributes_apart(order):
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", _SHAPE_ORDER, order], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
