"""-m gpu: the K loop of the F(2,3) Winograd tile (conv_wino.h: wino_main) at the smallest shapes where it can go wrong.

The loop runs two channel groups per iteration with compile-time LDS stages, stages the last group of a layer apart from the
steady loop (the only one that can hold padded channels), lets lanes without a staging job repeat another lane's and folds the
border masks, the missing pre-activation and the ReLU floor into per-lane data.  Variant 40 is forced through mvlm_conv2d, as in
tests/test_gpu_winograd.py; the reference is torch float64 with that file's bound 5e-6 * max(1, |want|max); every case runs
twice and the two results must be bit-equal.

  cin 4: one group, no steady loop      cin 8: two groups, the tail alone      cin 12 / 16: odd / even group counts
  cin 73: padded to 76 with a partly empty last group (19 groups: the odd count's leading group, steady iterations, tail)
  cin 84: 21 groups      cout 64 / 128: one / two cout tiles      size 32: one tile column, both x halos are image border
  size 64: halos from neighbouring tiles      batch 1 / 3      with pre-BatchNorm; without it on inputs with negative values
  (a ReLU floor where there is no activation would show); bias + post-BN; a residual."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import seeded_images

pytestmark = pytest.mark.gpu

VARIANT = 40  # conv3x3w_c64_t8x32

CASES = [
    # cin, cout, size, batch, opts
    (4, 64, 32, 1, dict()),
    (4, 128, 64, 3, dict(pre=True, res=True)),
    (8, 64, 32, 3, dict(pre=True)),
    (8, 128, 64, 1, dict(bias=True, post=True)),
    (12, 64, 64, 1, dict(pre=True, res=True)),
    (12, 128, 32, 3, dict()),
    (16, 64, 32, 1, dict(bias=True, post=True)),
    (16, 128, 64, 3, dict(pre=True, res=True)),
    (73, 64, 32, 3, dict(pre=True, res=True)),
    (73, 128, 64, 1, dict()),
    (73, 64, 64, 1, dict(bias=True, post=True)),
    (84, 64, 64, 3, dict()),
    (84, 128, 32, 1, dict(pre=True, res=True)),
    (84, 128, 64, 1, dict(bias=True, post=True, res=True)),
]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layer(ctx, x, w, bias, pre, post, res):
    batch, cin, size, _ = x.shape
    cout = w.shape[0]
    xd, yd = dev(x), torch.empty((batch, cout, size, size), dtype=torch.float32, device="cuda")
    rd = dev(res) if res is not None else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, VARIANT))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(xd.data_ptr()), batch, cin, size, size, p(w), cout, 3, p(bias),
                                      p(pre[0]) if pre else None, p(pre[1]) if pre else None,
                                      p(post[0]) if post else None, p(post[1]) if post else None,
                                      C.c_void_p(rd.data_ptr()) if rd is not None else None, 0, C.c_void_p(yd.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    return yd.cpu().numpy()


@pytest.mark.parametrize("cin,cout,size,batch,opts", CASES)
def test_forced_winograd_loop_matches_torch_and_itself(cin, cout, size, batch, opts):
    from mvlm_amd import _lib

    ctx = _lib.get_context(0)
    cin_pad = (cin + 3) // 4 * 4
    for kind in (0, 1, 2):  # a refused shape is a failure, not a skip
        assert ctx.lib.mvlm_conv_variant_serves(VARIANT, 3, cin_pad, cout, size, kind), (cin_pad, cout, size, kind)
    rs = np.random.RandomState(cin * 11 + cout + size + batch)
    x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)  # (negative values: about half of them)
    assert (x < 0).mean() > 0.4
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
    got = _layer(ctx, x, w, bias, pre, post, res)
    again = _layer(ctx, x, w, bias, pre, post, res)
    err = np.abs(got - want).max()
    print(f"\nwinograd-loop {cin}->{cout} @{size} B{batch} {sorted(opts)}: error {err:.3e} bound {tol:.3e}")
    assert err < tol
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_network_pass_in_mode_2_repeats_bit_for_bit():
    """pooled output, the raw copy and the scatter into the skip tensor, through the 84-landmark RGB+depth predictor"""
    from mvlm_amd.prediction import BU3DFEPredictor

    pred = BU3DFEPredictor(image_mode="RGB+depth", weights="synthetic:4", verbose=False)
    pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd(pred.ctx.handle, 2))
    try:
        x = dev(seeded_images(21, 2))
        a = pred.heatmaps_device(x).cpu().numpy()
        b = pred.heatmaps_device(x).cpu().numpy()
    finally:
        pred.ctx.check(pred.ctx.lib.mvlm_cnn_set_winograd(pred.ctx.handle, 1))
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
