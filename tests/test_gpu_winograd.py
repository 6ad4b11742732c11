"""-m gpu: the F(2,3) Winograd tiles of the large 3x3 layers (conv_wino.h; conv_cfg.h: Cfg::WINO, mvlm_cnn_set_winograd).

Single layers with the variant forced against torch float64 (the bound of test_conv2d_matches_torch), the network with every
servable layer on a Winograd tile (mode 2) against the direct path (mode 0) and against the reference's own vectors, mode 0 as
the direct path untouched, the default mode (1, the measured table) at the benchmark's size, and the routing as a function of
(shape, kind, batch) only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import seeded_images

pytestmark = pytest.mark.gpu

MODES = {"RGB": 3, "depth": 1, "RGB+depth": 4, "geometry+depth": 2}
WINO_IDS = [40]
CAP = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _is_wino(lib, variant):
    return 0 <= variant < 256 and lib.mvlm_conv_variant_name(variant).decode().startswith("conv3x3w_")


def test_the_library_names_the_winograd_variants():
    from mvlm_amd import _lib

    lib = _lib.load()
    for v in WINO_IDS:
        assert _is_wino(lib, v)
    named = [v for v in range(64) if _is_wino(lib, v)]
    assert named == WINO_IDS, named
    # a Winograd tile serves 3x3 layers of 32-pixel rows whose padded output channels fill its cout tile, in every kind
    assert all(lib.mvlm_conv_variant_serves(40, 3, 256, 128, 128, k) for k in (0, 1, 2))
    assert not lib.mvlm_conv_variant_serves(40, 3, 256, 128, 16, 0) and not lib.mvlm_conv_variant_serves(40, 3, 128, 32, 64, 0)
    assert not lib.mvlm_conv_variant_serves(40, 1, 256, 128, 64, 0)


# --------------------------------------------------------------------------------------------------------------------------
# 1. every Winograd variant forced, against torch float64; the direct tile's error on the same tensors beside it
LAYER_CASES = [
    # cin, cout, size, batch, opts
    (64, 64, 32, 1, dict()),
    (128, 64, 32, 3, dict(pre=True, res=True)),
    (256, 256, 32, 1, dict(bias=True, post=True)),
    (256, 128, 64, 3, dict(pre=True, res=True)),
    (64, 128, 64, 1, dict(bias=True, post=True)),
    (128, 128, 128, 1, dict(pre=True, res=True)),
    (256, 64, 128, 3, dict()),
    (128, 64, 128, 8, dict(pre=True, res=True)),   # 512 workgroups: two on every CU of the chip
    (73, 256, 32, 1, dict(bias=True, res=True)),   # cin 73 -> 76: a padded channel chunk
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


@pytest.mark.parametrize("variant", WINO_IDS)
@pytest.mark.parametrize("cin,cout,size,batch,opts", LAYER_CASES)
def test_forced_winograd_layer_matches_torch(variant, cin, cout, size, batch, opts):
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
    err_w = np.abs(_layer(ctx, variant, x, w, bias, pre, post, res) - want).max()
    err_d = np.abs(_layer(ctx, 10, x, w, bias, pre, post, res) - want).max()  # conv3x3_c64_t8x32, the direct tile of the same shape
    print(f"\nwinograd-error variant {variant} {cin}->{cout} @{size} B{batch} {sorted(opts)}: winograd {err_w:.3e} direct {err_d:.3e} "
          f"ratio {err_w / err_d:.2f} bound {tol:.3e}")
    assert err_w < tol


# --------------------------------------------------------------------------------------------------------------------------
def _predictor(nl, mode, seed, **kw):
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    return (BU3DFEPredictor if nl == 84 else DTU3DPredictor)(image_mode=mode, weights=f"synthetic:{seed}", verbose=False, **kw)


def _set_mode(pred, mode):
    pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd(pred.ctx.handle, mode))


def _profile(pred, x):
    """variants of one launch-by-launch pass"""
    ctx = pred.ctx
    pred.set_execution(graphs=False)
    ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 1))
    try:
        pred.predict_device(x)
        slot, var = (C.c_int32 * CAP)(), (C.c_int32 * CAP)()
        fl, ms = (C.c_double * CAP)(), (C.c_float * CAP)()
        n = ctx.lib.mvlm_cnn_get_profile(ctx.handle, slot, var, fl, ms, CAP)
        assert n > 0
        return [(slot[i], var[i], fl[i]) for i in range(n)]
    finally:
        ctx.check(ctx.lib.mvlm_cnn_set_profiling(ctx.handle, 0))
        pred.set_execution(graphs=True)


# 2. pooled output, raw copy + residual slice and scatter-into-skip through the network: mode 2 against mode 0
@pytest.mark.parametrize("nl,mode", [(73, "RGB"), (84, "RGB+depth")])
def test_network_on_winograd_tiles_against_the_direct_path(nl, mode):
    from oracle import cnn as ocnn

    pred = _predictor(nl, mode, 4)
    x = dev(seeded_images(21, 2))
    _set_mode(pred, 0)
    heat0 = pred.heatmaps_device(x).cpu().numpy()
    pools0 = len([r for r in _profile(pred, x) if r[0] == -1])
    _set_mode(pred, 2)
    recs = _profile(pred, x)
    lib = pred.ctx.lib
    wino = [r for r in recs if _is_wino(lib, r[1])]
    # the three layer kinds are really served: most of the 128x128 / 64x64 / 32x32 levels' 3x3 layers
    assert len(wino) >= 30, len(wino)
    assert len([r for r in recs if r[0] == -1]) <= pools0  # no pool kernel more: the Winograd tiles emit the pooled tensor themselves
    heat2 = pred.heatmaps_device(x).cpu().numpy()
    scale = np.abs(heat0).max()
    d = np.abs(heat2 - heat0).max()
    print(f"\nwinograd-network {nl} {mode}: {len(wino)} of {len(recs)} launches on Winograd tiles, max |mode 2 - mode 0| = {d:.3e} = {d / scale:.2e} of scale")
    assert d < 2e-4 * scale
    lms = pred.predict_device(x).cpu().numpy()
    np.testing.assert_array_equal(lms, ocnn.maxima_fast(torch.from_numpy(heat2)))


# 3. mode 2 against the reference's own vectors: cases and criteria of test_full_network_against_reference_vectors
def _near_tie_ok(heat_plane, got_rc, want_rc, rel=2e-4):
    gv = heat_plane[int(got_rc[0]) + 1, int(got_rc[1] + 0.5)]
    wv = heat_plane[int(want_rc[0]) + 1, int(want_rc[1] + 0.5)]
    return abs(gv - wv) <= rel * max(abs(wv), 1.0)


@pytest.mark.parametrize("nl,mode", [(73, "RGB"), (84, "RGB+depth"), (73, "geometry+depth"), (84, "depth")])
def test_winograd_network_against_reference_vectors(golden, nl, mode):
    from mvlm_amd import arch, weights
    from oracle import cnn as ocnn

    g = golden("cnn_full.npz")
    tag = f"{nl}_{mode}"
    seed, img_seed = (int(v) for v in g[f"{tag}_seed"])
    imgs = seeded_images(img_seed, 2)
    pred = _predictor(nl, mode, seed)
    _set_mode(pred, 2)
    heat = pred.heatmaps_device(dev(imgs)).cpu().numpy()
    ref_sub = g[f"{tag}_heat_sub"]
    scale = np.abs(ref_sub).max()
    assert np.abs(heat[:, :, 5::16, 3::16] - ref_sub).max() < 2e-4 * scale
    lms, valid = pred.predict_landmarks_from_images(imgs)
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


# 4. mode 0 is the direct path
def test_mode_0_runs_no_winograd_tile_and_the_environment_sets_the_default():
    x = dev(seeded_images(5, 3))
    a = _predictor(84, "RGB+depth", 2)
    _set_mode(a, 0)
    recs = _profile(a, x)
    assert recs and not [r for r in recs if _is_wino(a.ctx.lib, r[1])]
    # FLOPs of a record are what its MFMAs execute: 6 taps' worth on a Winograd tile, 9 on a direct 3x3 tile
    _set_mode(a, 2)
    recs2 = _profile(a, x)
    by_slot0 = {r[0]: r for r in recs if r[0] >= 0 and r[1] < 256}
    checked = 0
    for s, v, fl in recs2:
        if _is_wino(a.ctx.lib, v) and s in by_slot0:
            assert abs(fl / by_slot0[s][2] - 2.0 / 3.0) < 1e-12
            checked += 1
    assert checked >= 10
    _set_mode(a, 0)
    saved = os.environ.get("MVLM_WINOGRAD")
    os.environ["MVLM_WINOGRAD"] = "0"
    try:
        b = _predictor(84, "RGB+depth", 2)
    finally:
        if saved is None:
            del os.environ["MVLM_WINOGRAD"]
        else:
            os.environ["MVLM_WINOGRAD"] = saved
    assert not [r for r in _profile(b, x) if _is_wino(b.ctx.lib, r[1])]
    assert torch.equal(a.predict_device(x), b.predict_device(x))
    assert a.ctx.lib.mvlm_cnn_set_winograd(a.ctx.handle, 3) != 0 and a.ctx.lib.mvlm_cnn_set_winograd(a.ctx.handle, -1) != 0


# 5. the benchmark's size, the default mode against mode 0
def test_bench_sized_agreement_of_the_default_mode_with_the_direct_path():
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
        _set_mode(pred, m)
        np.random.set_state(state)
        lm3d, _ = pipe.predict_mesh_device(mesh, poses)
        out[m] = (pred.predict_device(images).cpu().numpy(), np.asarray(lm3d))
    nl = out[0][0].shape[0]
    differ = ~np.all(out[0][0][:, :, :2] == out[1][0][:, :, :2], axis=2)  # [NL, N]
    print(f"\nwinograd-bench-size: {int(differ.sum())} of {nl * n} planes with another argmax pixel")
    assert differ.sum() <= 0.002 * nl * n
    if differ.any():
        _set_mode(pred, 0)
        for lm, v in zip(*np.nonzero(differ)):
            plane = pred.heatmaps_device(images[v:v + 1])[0, lm].cpu().numpy()
            assert _near_tie_ok(plane, out[1][0][lm, v], out[0][0][lm, v]), (lm, v)
    same = ~differ.any(axis=1)
    d = np.abs(out[0][1] - out[1][1]).max(axis=1)
    print(f"winograd-bench-size: landmarks with identical planes {int(same.sum())}/{nl}, max |mode 1 - mode 0| = {d[same].max():.3e} model units")
    assert d[same].max() < 1e-3
    _set_mode(pred, 1)


# 6. routing is a function of (shape, kind, batch)
def test_routing_depends_on_shape_kind_and_batch_only():
    imgs = dev(seeded_images(9, 48))
    alone = _predictor(84, "RGB+depth", 6)
    sliced = _predictor(84, "RGB+depth", 6, device_batch=12)
    _set_mode(alone, 1)
    _set_mode(sliced, 1)
    all48 = sliced.predict_device(imgs)
    for s in (0, 24):
        assert torch.equal(alone.predict_device(imgs[s:s + 12].contiguous()), all48[:, s:s + 12])
