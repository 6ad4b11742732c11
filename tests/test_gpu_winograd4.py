"""-m gpu: the F(4,3) Winograd tile of the 3x3 layers (conv_wino4.h; conv_cfg.h: Cfg::WINO4, variant conv3x3q_c32_t16x32, mvlm_cnn_set_winograd4).

Single layers with the variant forced against torch float64 (the bound of test_conv2d_matches_torch), the network with every
servable layer on the tile (F(4,3) mode 2) against the direct path (Winograd mode 0) and against the reference's own vectors,
F(4,3) mode 0 as the parent's launches, and the default modes at the benchmark's size."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, seeded_images

pytestmark = pytest.mark.gpu

MODES = {"RGB": 3, "depth": 1, "RGB+depth": 4, "geometry+depth": 2}
WINO4 = 2048  # MVLM_CONV_VARIANT_WINO4: a code of its own, beyond the base ids and their K-part forms
DIRECT = 3  # conv3x3_c32_t16x32, the direct tile of the same geometry
CAP = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _is_wino4(lib, variant):
    return variant >= 0 and lib.mvlm_conv_variant_name(variant).decode().startswith("conv3x3q_")


def test_the_library_names_the_variant_and_what_it_serves():
    from mvlm_amd import _lib

    lib = _lib.load()
    assert [v for v in range(4096) if _is_wino4(lib, v)] == [WINO4]  # (none of the base ids 0..63, whose table tests/golden/conv_routing.txt pins)
    # 3x3 layers of 32-pixel rows and whole row quads of a 16-row tile, output channels in 32s, up to 256 input channels, every kind
    assert all(lib.mvlm_conv_variant_serves(WINO4, 3, 256, 128, 128, k) for k in (0, 1, 2))
    assert lib.mvlm_conv_variant_serves(WINO4, 3, 64, 32, 32, 0)
    assert not lib.mvlm_conv_variant_serves(WINO4, 3, 256, 128, 16, 0) and not lib.mvlm_conv_variant_serves(WINO4, 3, 128, 84, 64, 0)
    assert not lib.mvlm_conv_variant_serves(WINO4, 3, 320, 64, 64, 0) and not lib.mvlm_conv_variant_serves(WINO4, 1, 256, 128, 64, 0)


# --------------------------------------------------------------------------------------------------------------------------
# 1. the variant forced, against torch float64; the direct tile's error on the same tensors beside it.
# size 32, batch 1: two row tiles, one column tile, every border in one workgroup; size 64, batch 3: interior tile edges and more
# than one image.  cin 4: one chunk, 8: two (no steady loop), 20: an odd count, 64; 73 -> 76: a padded last chunk; 256: the LDS
# BatchNorm table's limit.  cout 32: one cout tile, 64: two.
LAYER_CASES = [
    # cin, cout, size, batch, opts
    (4, 32, 32, 1, dict()),
    (8, 64, 32, 1, dict(pre=True, res=True)),
    (20, 32, 64, 3, dict(bias=True, post=True)),
    (64, 64, 64, 3, dict(pre=True, res=True)),
    (73, 32, 32, 1, dict(bias=True, post=True)),
    (73, 64, 64, 3, dict(pre=True, res=True)),
    (256, 64, 32, 1, dict()),
    (256, 32, 64, 3, dict(pre=True, res=True)),
]


def _layer(ctx, variant, x, w, bias, pre, post, res):
    batch, cin, size, _ = x.shape
    cout = w.shape[0]
    xd, yd = dev(x), torch.empty((batch, cout, size, size), dtype=torch.float32, device="cuda")
    rd = dev(res) if res is not None else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, variant))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(xd.data_ptr()), batch, cin, size, size, p(w), cout, 3, p(bias),
                                      p(pre[0]) if pre else None, p(pre[1]) if pre else None,
                                      p(post[0]) if post else None, p(post[1]) if post else None,
                                      C.c_void_p(rd.data_ptr()) if rd is not None else None, 0, C.c_void_p(yd.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    return yd.cpu().numpy()


@pytest.mark.parametrize("cin,cout,size,batch,opts", LAYER_CASES)
def test_forced_winograd4_layer_matches_torch(cin, cout, size, batch, opts):
    from mvlm_amd import _lib

    ctx = _lib.get_context(0)
    rs = np.random.RandomState(cin * 7 + cout + size)
    x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    bias = rs.standard_normal(cout).astype(np.float32) if opts.get("bias") else None
    pre = (rs.uniform(0.5, 1.5, cin).astype(np.float32), rs.standard_normal(cin).astype(np.float32) * 0.3) if opts.get("pre") else None
    post = (rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.standard_normal(cout).astype(np.float32) * 0.3) if opts.get("post") else None
    res = rs.standard_normal((batch, cout, size, size)).astype(np.float32) if opts.get("res") else None

    t = torch.from_numpy(x).double()
    if pre:
        t = torch.relu(t * torch.from_numpy(pre[0]).double()[None, :, None, None] + torch.from_numpy(pre[1]).double()[None, :, None, None])
    y = torch.nn.functional.conv2d(t, torch.from_numpy(w).double(), None if bias is None else torch.from_numpy(bias).double(), 1, 1)
    if post:
        y = torch.relu(y * torch.from_numpy(post[0]).double()[None, :, None, None] + torch.from_numpy(post[1]).double()[None, :, None, None])
    if res is not None:
        y = y + torch.from_numpy(res).double()
    want = y.numpy()
    tol = 5e-6 * max(1.0, np.abs(want).max())
    err_w = np.abs(_layer(ctx, WINO4, x, w, bias, pre, post, res) - want).max()
    err_d = np.abs(_layer(ctx, DIRECT, x, w, bias, pre, post, res) - want).max()
    print(f"\nwinograd4-error {cin}->{cout} @{size} B{batch} {sorted(opts)}: F(4,3) {err_w:.3e} direct {err_d:.3e} "
          f"ratio {err_w / err_d:.2f} bound {tol:.3e}")
    assert err_w < tol


# --------------------------------------------------------------------------------------------------------------------------
def _predictor(nl, mode, seed, **kw):
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    return (BU3DFEPredictor if nl == 84 else DTU3DPredictor)(image_mode=mode, weights=f"synthetic:{seed}", verbose=False, **kw)


def _set_modes(pred, winograd, winograd4):
    pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd(pred.ctx.handle, winograd))
    pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd4(pred.ctx.handle, winograd4))


def _profile(pred, x):
    """(slot, variant, flops, kind) of one launch-by-launch pass"""
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
        kinds = [shapes[6 * i + 4] for i in range(n)]
        return [(slot[i], var[i], fl[i], kinds[i]) for i in range(n)]
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 0))
        pred.set_execution(graphs=True)


# 2. pooled output, raw copy + residual slice and scatter-into-skip through the network: F(4,3) mode 2 against the direct path
@pytest.mark.parametrize("nl,mode", [(73, "RGB"), (84, "RGB+depth")])
def test_network_on_the_winograd4_tile_against_the_direct_path(nl, mode):
    from oracle import cnn as ocnn

    pred = _predictor(nl, mode, 4)
    x = dev(seeded_images(21, 2))
    try:
        _set_modes(pred, 0, 2)  # Winograd mode 0 is the direct path, whatever the new switch says
        recs0 = _profile(pred, x)
        assert not [r for r in recs0 if _is_wino4(pred.ctx.lib, r[1])]
        heat0 = pred.heatmaps_device(x).cpu().numpy()
        pools0 = len([r for r in recs0 if r[0] == -1])
        _set_modes(pred, 1, 2)
        recs = _profile(pred, x)
        lib = pred.ctx.lib
        q = [r for r in recs if _is_wino4(lib, r[1])]
        assert len(q) >= 30, len(q)
        assert {0, 1, 2} <= {r[3] for r in q}, sorted({r[3] for r in q})  # every kind of launch really on the new variant
        assert len([r for r in recs if r[0] == -1]) <= pools0  # no pool kernel more: the tile emits the pooled tensor itself
        heat2 = pred.heatmaps_device(x).cpu().numpy()
        scale = np.abs(heat0).max()
        d = np.abs(heat2 - heat0).max()
        print(f"\nwinograd4-network {nl} {mode}: {len(q)} of {len(recs)} launches on the F(4,3) tile, max |F(4,3) - direct| = {d:.3e} = {d / scale:.2e} of scale")
        assert d < 2e-4 * scale
        lms = pred.predict_device(x).cpu().numpy()
        np.testing.assert_array_equal(lms, ocnn.maxima_fast(torch.from_numpy(heat2)))
    finally:
        _set_modes(pred, 1, 1)


# 3. F(4,3) mode 2 against the reference's own vectors: cases and criteria of test_full_network_against_reference_vectors
def _near_tie_ok(heat_plane, got_rc, want_rc, rel=2e-4):
    gv = heat_plane[int(got_rc[0]) + 1, int(got_rc[1] + 0.5)]
    wv = heat_plane[int(want_rc[0]) + 1, int(want_rc[1] + 0.5)]
    return abs(gv - wv) <= rel * max(abs(wv), 1.0)


@pytest.mark.parametrize("nl,mode", [(73, "RGB"), (84, "RGB+depth"), (73, "geometry+depth"), (84, "depth")])
def test_winograd4_network_against_reference_vectors(golden, nl, mode):
    from mvlm_amd import arch, weights
    from oracle import cnn as ocnn

    g = golden("cnn_full.npz")
    tag = f"{nl}_{mode}"
    seed, img_seed = (int(v) for v in g[f"{tag}_seed"])
    imgs = seeded_images(img_seed, 2)
    pred = _predictor(nl, mode, seed)
    try:
        _set_modes(pred, 1, 2)
        heat = pred.heatmaps_device(dev(imgs)).cpu().numpy()
        ref_sub = g[f"{tag}_heat_sub"]
        scale = np.abs(ref_sub).max()
        assert np.abs(heat[:, :, 5::16, 3::16] - ref_sub).max() < 2e-4 * scale
        lms, valid = pred.predict_landmarks_from_images(imgs)
    finally:
        _set_modes(pred, 1, 1)
    assert valid.all() and lms.shape == (nl, 2, 3)
    want = g[f"{tag}_maxima"]
    np.testing.assert_array_equal(lms, ocnn.maxima_fast(torch.from_numpy(heat)))
    sd = weights.synthetic_state_dict(nl, MODES[mode], seed=seed)
    _, _, oheat = ocnn.predict_landmarks_from_images(sd, imgs, arch.CHANNEL_SELECT[mode], return_heatmaps=True)
    oheat = oheat.numpy()
    flips = 0
    for lm in range(nl):
        for v in range(2):
            if not np.array_equal(lms[lm, v, :2], want[lm, v, :2]):
                flips += 1
                assert _near_tie_ok(oheat[v, lm], lms[lm, v], want[lm, v]), (lm, v, lms[lm, v], want[lm, v])
            assert abs(lms[lm, v, 2] - want[lm, v, 2]) < 2e-4 * scale
    assert flips <= 0.02 * nl * 2, f"{flips} argmax differences"


# 4. F(4,3) mode 0 launches the parent's variants; FLOPs of a record; the environment default; the mode's range
def test_mode_0_launches_the_recorded_variants_and_the_environment_sets_the_default():
    x = dev(seeded_images(9, 2))
    a = _predictor(84, "RGB+depth", 6)
    try:
        # tests/golden/conv_slot_variants.json: the golden of test_gpu_conv_routing.py, which this tile did not move (its table holds
        # rows from 96 views on, the golden's passes run 1, 2 and 12) - the same seven passes with the F(4,3) switch at 0
        want = json.loads((REPO / "tests/golden/conv_slot_variants.json").read_text())
        images = dev(seeded_images(9, 12))
        for wino, pairing, batch in [(w, 1, b) for w in (0, 1) for b in (1, 2, 12)] + [(1, 0, 2)]:
            _set_modes(a, wino, 0)
            a.set_execution(graphs=False, pairing=pairing)
            a.ctx.check(a.ctx.lib.mvlm_cnn_set_profiling(a.ctx.handle, 1))
            try:
                a.predict_device(images[:batch].contiguous())
                slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
                n = a.ctx.lib.mvlm_cnn_get_profile(a.ctx.handle, slot, var, (C.c_double * CAP)(), (C.c_float * CAP)(), CAP)
            finally:
                a.ctx.check(a.ctx.lib.mvlm_cnn_set_profiling(a.ctx.handle, 0))
            assert [[slot[i], var[i]] for i in range(n)] == want[f"winograd{wino}_pairing{pairing}_batch{batch}"], (wino, pairing, batch)
        a.set_execution(graphs=False, pairing=1)
        _set_modes(a, 1, 0)
        recs0 = _profile(a, x)
        assert not [r for r in recs0 if _is_wino4(a.ctx.lib, r[1])]
        _set_modes(a, 0, 2)
        direct = {r[0]: r for r in _profile(a, x) if r[0] >= 0 and r[1] < 256}
        # Winograd mode 2 with the new switch at 0 or 1: no launch on the new tile
        for m4 in (0, 1):
            _set_modes(a, 2, m4)
            assert not [r for r in _profile(a, x) if _is_wino4(a.ctx.lib, r[1])]
        # FLOPs of a record are what its MFMAs execute: 4.5 taps' worth on the F(4,3) tile, 9 on a direct 3x3 tile
        _set_modes(a, 1, 2)
        checked = 0
        for s, v, fl, _ in _profile(a, x):
            if _is_wino4(a.ctx.lib, v) and s in direct:
                assert fl == 0.5 * direct[s][2]
                checked += 1
        assert checked >= 10
        _set_modes(a, 1, 0)
        saved = os.environ.get("MVLM_WINOGRAD4")
        os.environ["MVLM_WINOGRAD4"] = "0"
        try:
            b = _predictor(84, "RGB+depth", 6)
        finally:
            if saved is None:
                del os.environ["MVLM_WINOGRAD4"]
            else:
                os.environ["MVLM_WINOGRAD4"] = saved
        assert [r[:2] for r in _profile(b, x)] == [r[:2] for r in recs0]
        assert torch.equal(a.predict_device(x), b.predict_device(x))
        lib = a.ctx.lib
        assert lib.mvlm_cnn_set_winograd4(a.ctx.handle, 3) != 0 and lib.mvlm_cnn_set_winograd4(a.ctx.handle, -1) != 0
        assert lib.mvlm_cnn_set_winograd(a.ctx.handle, 3) != 0
    finally:
        _set_modes(a, 1, 1)
        a.set_execution(graphs=True, pairing=1)


# 5. the benchmark's size, the default modes against the direct path: criteria of
# test_bench_sized_agreement_of_the_default_mode_with_the_direct_path
def test_bench_sized_agreement_of_the_default_modes_with_the_direct_path():
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
    out = {}
    for m in (0, 1):
        _set_modes(pred, m, 1)
        np.random.set_state(state)
        lm3d, _ = pipe.predict_mesh_device(mesh, poses)
        out[m] = (pred.predict_device(images).cpu().numpy(), np.asarray(lm3d))
    nl = out[0][0].shape[0]
    # the default modes really route to the tile at this size (the table's rows), and the switch at 0 takes it out again
    try:
        on = [r for r in _profile(pred, images) if _is_wino4(pred.ctx.lib, r[1])]
        assert len(on) >= 30 and {0, 1, 2} <= {r[3] for r in on}, (len(on), sorted({r[3] for r in on}))
        _set_modes(pred, 1, 0)
        assert not [r for r in _profile(pred, images) if _is_wino4(pred.ctx.lib, r[1])]
    finally:
        _set_modes(pred, 1, 1)
    differ = ~np.all(out[0][0][:, :, :2] == out[1][0][:, :, :2], axis=2)  # [NL, N]
    print(f"\nwinograd4-bench-size: {len(on)} launches of the default pass on the F(4,3) tile; {int(differ.sum())} of {nl * n} planes with another argmax pixel")
    assert differ.sum() <= 0.002 * nl * n
    if differ.any():
        _set_modes(pred, 0, 1)
        for lm, v in zip(*np.nonzero(differ)):
            plane = pred.heatmaps_device(images[v:v + 1])[0, lm].cpu().numpy()
            assert _near_tie_ok(plane, out[1][0][lm, v], out[0][0][lm, v]), (lm, v)
    same = ~differ.any(axis=1)
    d = np.abs(out[0][1] - out[1][1]).max(axis=1)
    print(f"winograd4-bench-size: landmarks with identical planes {int(same.sum())}/{nl}, max |default - direct| = {d[same].max():.3e} model units")
    assert d[same].max() < 1e-3
    _set_modes(pred, 1, 1)


# 6. the tile's launch attributes are remembered apart from the other kernels' (a fresh process: a kernel's attributes, once set,
# hold for every context of the process, so only there does the first launch of each kernel show whether its own were set)
_ATTRIBUTE_ORDER = r"""
import ctypes as C, sys
import numpy as np, torch
from mvlm_amd import _lib
ctx = _lib.Context(0)
f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
rs = np.random.RandomState(0)
def tile():
    x = torch.randn(1, 8, 32, 32, device="cuda"); y = torch.empty(1, 32, 32, 32, device="cuda")
    w = (rs.standard_normal((32, 8, 3, 3)) * 0.1).astype(np.float32)
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, 2048))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(x.data_ptr()), 1, 8, 32, 32, f(w), 32, 3, None, None, None, None, None, None, 0, C.c_void_p(y.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    return (y - torch.nn.functional.conv2d(x, torch.from_numpy(w).cuda(), None, 1, 1)).abs().max().item()
def fast_general_64():  # bf16x3, 64 output channels, cin 73 != cin_pad: the general form, 155 KB of LDS
    x = torch.randn(1, 73, 32, 32, device="cuda"); y = torch.empty(1, 64, 32, 32, device="cuda")
    w = (rs.standard_normal((64, 73, 3, 3)) * 0.04).astype(np.float32)
    ctx.check(ctx.lib.mvlm_conv2d_fast(ctx.handle, C.c_void_p(x.data_ptr()), 1, 73, 32, 32, f(w), 64, None, None, None, None, None, None, C.c_void_p(y.data_ptr())))
    return (y - torch.nn.functional.conv2d(x, torch.from_numpy(w).cuda(), None, 1, 1)).abs().max().item()
errs = [tile(), fast_general_64()] if sys.argv[1] == "tile-first" else [fast_general_64(), tile()]
assert max(errs) < 1e-3, errs
print("ok", errs)
"""


@pytest.mark.parametrize("order", ["tile-first", "fast-first"])
def test_tile_and_fast_kernels_keep_their_launch_attributes_apart(order):
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", _ATTRIBUTE_ORDER, order], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
