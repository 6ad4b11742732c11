"""The F(4,3)-along-y form of the 3x3 layers (mvlm_amd/csrc/conv_wino4.h; conv_cfg.h: Cfg::WINO4, points 0, 1, -1, 2, -1/2, inf) on the CPU:
a float64 numpy model of the tile's arithmetic - six transformed rows v_t per row quad, six transformed weight columns u_t, six
GEMMs over (kx, cin), the output transform - against the direct convolution, and the library's host weight transform against
the model's."""
import ctypes as C

import numpy as np
import torch


def transform_weights64(w):
    """w [cout, cin, 3(ky), 3(kx)] float64 -> u [6, cout, cin, 3(kx)]"""
    g0, g1, g2 = w[:, :, 0, :], w[:, :, 1, :], w[:, :, 2, :]
    return np.stack([g0, -(g0 + g1 + g2) / 3.0, (g0 - g1 + g2) / 3.0, (g0 + 2.0 * g1 + 4.0 * g2) / 15.0,
                     (-16.0 * g0 + 8.0 * g1 - 4.0 * g2) / 15.0, g2])


def transform_rows64(d):
    """d [cin, 6, W']: rows 4q-1 .. 4q+4 -> v [6, cin, W']"""
    d0, d1, d2, d3, d4, d5 = (d[:, r] for r in range(6))
    return np.stack([d0 + 1.5 * d1 - 2 * d2 - 1.5 * d3 + d4,
                     -d1 - 2.5 * d2 - 0.5 * d3 + d4,
                     d1 + 0.5 * d2 - 2.5 * d3 + d4,
                     -0.5 * d1 - d2 + 0.5 * d3 + d4,
                     2 * d1 - d2 - 2 * d3 + d4,
                     d1 + 1.5 * d2 - 2 * d3 - 1.5 * d4 + d5])


def winograd4_rows_model(x, w, pre=None):
    """x [cin, H, W], w [cout, cin, 3, 3]; BatchNorm + ReLU first, zero padding AFTER the activation, as the staging does"""
    x = x.astype(np.float64)
    if pre is not None:
        x = np.maximum(x * pre[0][:, None, None] + pre[1][:, None, None], 0.0)
    cin, H, W = x.shape
    cout = w.shape[0]
    xp = np.zeros((cin, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    u = transform_weights64(w.astype(np.float64))
    out = np.zeros((cout, H, W))
    for q in range(H // 4):
        v = transform_rows64(xp[:, 4 * q:4 * q + 6, :])  # padded rows 4q .. 4q+5 = image rows 4q-1 .. 4q+4
        m = np.zeros((6, cout, W))
        for kx in range(3):
            m += np.einsum("toc,tcx->tox", u[:, :, :, kx], v[:, :, kx:kx + W])
        s, d = m[1] + m[2], m[1] - m[2]
        out[:, 4 * q] = (m[0] + s) + (m[3] + m[4])
        out[:, 4 * q + 1] = d + (2 * m[3] - m[4] / 2)
        out[:, 4 * q + 2] = s + (4 * m[3] + m[4] / 4)
        out[:, 4 * q + 3] = (d + (8 * m[3] - m[4] / 8)) + m[5]
    return out


def direct64(x, w, pre=None):
    t = torch.from_numpy(x.astype(np.float64))[None]
    if pre is not None:
        t = torch.relu(t * torch.from_numpy(pre[0])[None, :, None, None] + torch.from_numpy(pre[1])[None, :, None, None])
    return torch.nn.functional.conv2d(t, torch.from_numpy(w.astype(np.float64)), None, 1, 1)[0].numpy()


def test_float64_model_equals_the_direct_convolution():
    rs = np.random.RandomState(5)
    for cin, cout, size in [(5, 7, 8), (12, 6, 16), (3, 4, 4), (8, 8, 32)]:
        x = rs.standard_normal((cin, size, size)).astype(np.float32)
        w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        # a positive shift: relu(shift) != 0, so padding before the activation would show at the borders
        pre = (rs.uniform(0.5, 1.5, cin), np.abs(rs.standard_normal(cin)) + 0.2)
        got, want = winograd4_rows_model(x, w, pre), direct64(x, w, pre)
        err = np.abs(got - want).max()
        print(f"cin {cin} cout {cout} size {size}: max |model - direct| = {err:.2e}")
        assert err < 1e-12, (cin, cout, size, err)
        assert np.abs(want[:, 0]).max() > 0.1 and np.abs(want[:, :, -1]).max() > 0.1  # the borders carry signal


def _pack9(w, cin_pad, cout_pad):
    cout, cin = w.shape[:2]
    out = np.zeros((9, cin_pad, cout_pad), np.float32)
    out[:, :cin, :cout] = w.reshape(cout, cin, 9).transpose(2, 1, 0)
    return out


def test_pack_winograd4_weights_is_the_float64_transform_rounded_once():
    from mvlm_amd import _lib

    lib = _lib.load()
    rs = np.random.RandomState(11)
    fp = C.POINTER(C.c_float)
    for cin, cout, cin_pad, cout_pad in [(73, 84, 76, 128), (256, 256, 256, 256), (3, 64, 4, 64)]:
        w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        w9 = _pack9(w, cin_pad, cout_pad)
        w18 = np.full((18, cin_pad, cout_pad), np.nan, np.float32)
        assert lib.mvlm_pack_winograd4_weights(w9.ctypes.data_as(fp), cin_pad, cout_pad, w18.ctypes.data_as(fp)) == 0
        u = transform_weights64(w.astype(np.float64))  # [6, cout, cin, kx]
        want = np.zeros((18, cin_pad, cout_pad), np.float32)
        for t in range(6):
            for kx in range(3):
                want[t * 3 + kx, :cin, :cout] = u[t, :, :, kx].T.astype(np.float32)
        assert np.array_equal(w18.view(np.uint32), want.view(np.uint32))
        assert not w18[:, cin:, :].any() and not w18[:, :, cout:].any()  # padded channels stay zero
    assert lib.mvlm_pack_winograd4_weights(None, 4, 64, None) != 0
    w9 = np.zeros((9, 4, 64), np.float32)
    assert lib.mvlm_pack_winograd4_weights(w9.ctypes.data_as(fp), 4, 64, None) != 0


def test_the_tile_has_a_code_of_its_own_outside_the_base_variant_table():
    """MVLM_CONV_VARIANT_WINO4 = 2048: none of the base ids 0..63 (the table tests/golden/conv_routing.txt pins) nor of their K-part
    forms up to 1023 is the tile; the code serves 3x3 layers of 32-pixel rows in whole 16-row tiles, output channels in 32s, up
    to 256 input channels, in every kind"""
    from mvlm_amd import _lib

    lib = _lib.load()
    name = lambda v: lib.mvlm_conv_variant_name(v).decode()
    assert name(2048) == "conv3x3q_c32_t16x32"
    assert not [v for v in range(1024) if name(v).startswith("conv3x3q_")]
    serves = lambda *a: bool(lib.mvlm_conv_variant_serves(2048, *a))
    assert all(serves(3, 256, 128, 128, k) for k in (0, 1, 2)) and serves(3, 4, 32, 32, 0) and serves(3, 76, 256, 64, 2)
    assert not serves(3, 256, 128, 128, 3) and not serves(3, 256, 128, 128, -1)
    assert not serves(3, 256, 128, 16, 0) and not serves(3, 128, 84, 64, 0) and not serves(3, 128, 80, 64, 0)
    assert not serves(3, 320, 64, 64, 0) and not serves(1, 256, 128, 64, 0) and not serves(2, 128, 96, 64, 0)
