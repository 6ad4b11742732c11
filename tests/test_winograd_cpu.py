"""The F(2,3)-along-y form of the large 3x3 layers (mvlm_amd/csrc/conv_wino.h; conv_cfg.h: Cfg::WINO) on the CPU: a float64 numpy model of
the tile's arithmetic - transformed rows v_t, transformed weight columns u_t, four GEMMs over (kx, cin), the output transform -
against the direct convolution, and the library's host weight transform against the model's."""
import ctypes as C

import numpy as np
import torch


def transform_weights64(w):
    """w [cout, cin, 3(ky), 3(kx)] float64 -> u [4, cout, cin, 3(kx)]"""
    g0, g1, g2 = w[:, :, 0, :], w[:, :, 1, :], w[:, :, 2, :]
    return np.stack([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2])


def winograd_rows_model(x, w, pre=None):
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
    for p in range(H // 2):
        d = xp[:, 2 * p:2 * p + 4, :]  # padded rows 2p .. 2p+3 = image rows 2p-1 .. 2p+2
        v = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]])  # [4, cin, W+2]
        m = np.zeros((4, cout, W))
        for kx in range(3):
            m += np.einsum("toc,tcx->tox", u[:, :, :, kx], v[:, :, kx:kx + W])
        out[:, 2 * p] = (m[0] + m[1]) + m[2]
        out[:, 2 * p + 1] = (m[1] - m[2]) - m[3]
    return out


def direct64(x, w, pre=None):
    t = torch.from_numpy(x.astype(np.float64))[None]
    if pre is not None:
        t = torch.relu(t * torch.from_numpy(pre[0])[None, :, None, None] + torch.from_numpy(pre[1])[None, :, None, None])
    return torch.nn.functional.conv2d(t, torch.from_numpy(w.astype(np.float64)), None, 1, 1)[0].numpy()


def test_float64_model_equals_the_direct_convolution():
    rs = np.random.RandomState(5)
    for cin, cout, size, with_pre in [(5, 7, 8, False), (12, 6, 16, True), (3, 4, 2, True), (8, 8, 32, True)]:
        x = rs.standard_normal((cin, size, size)).astype(np.float32)
        w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        # a positive shift: relu(shift) != 0, so padding before the activation would show at the borders
        pre = (rs.uniform(0.5, 1.5, cin), np.abs(rs.standard_normal(cin)) + 0.2) if with_pre else None
        got, want = winograd_rows_model(x, w, pre), direct64(x, w, pre)
        assert np.abs(got - want).max() < 1e-12, (cin, cout, size, np.abs(got - want).max())
        assert np.abs(want[:, 0]).max() > 0.1 and np.abs(want[:, :, -1]).max() > 0.1  # the borders carry signal


def _pack9(w, cin_pad, cout_pad):
    cout, cin = w.shape[:2]
    out = np.zeros((9, cin_pad, cout_pad), np.float32)
    out[:, :cin, :cout] = w.reshape(cout, cin, 9).transpose(2, 1, 0)
    return out


def test_pack_winograd_weights_is_the_float64_transform_rounded_once():
    from mvlm_amd import _lib

    lib = _lib.load()
    rs = np.random.RandomState(11)
    fp = C.POINTER(C.c_float)
    for cin, cout, cin_pad, cout_pad in [(73, 84, 76, 128), (256, 256, 256, 256), (3, 64, 4, 64)]:
        w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        w9 = _pack9(w, cin_pad, cout_pad)
        w12 = np.full((12, cin_pad, cout_pad), np.nan, np.float32)
        assert lib.mvlm_pack_winograd_weights(w9.ctypes.data_as(fp), cin_pad, cout_pad, w12.ctypes.data_as(fp)) == 0
        u = transform_weights64(w.astype(np.float64))  # [4, cout, cin, kx]
        want = np.zeros((12, cin_pad, cout_pad), np.float32)
        for t in range(4):
            for kx in range(3):
                want[t * 3 + kx, :cin, :cout] = u[t, :, :, kx].T.astype(np.float32)
        assert np.array_equal(w12.view(np.uint32), want.view(np.uint32))
        assert not w12[:, cin:, :].any() and not w12[:, :, cout:].any()  # padded channels stay zero
    assert lib.mvlm_pack_winograd_weights(None, 4, 64, None) != 0
