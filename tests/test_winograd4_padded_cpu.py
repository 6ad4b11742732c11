"""The F(4,3) weights of a 3x3 layer whose padded output channels are no multiple of 32 (84 rows, 80 rows), packed at a cout stride
of whole 32s for the tile (mvlm_pack_winograd4_weights_padded, mvlm_conv_wino4_padded_stride): the columns below cout_pad are
mvlm_pack_winograd4_weights' own, everything beyond is an exact zero, and so is the bias's tail.  No GPU."""
import ctypes as C

import numpy as np

FP = C.POINTER(C.c_float)


def _pack9(w, cin_pad, cout_pad):
    cout, cin = w.shape[:2]
    out = np.zeros((9, cin_pad, cout_pad), np.float32)
    out[:, :cin, :cout] = w.reshape(cout, cin, 9).transpose(2, 1, 0)
    return out


def test_the_stride_is_the_next_multiple_of_32():
    from mvlm_amd import _lib

    lib = _lib.load()
    assert [lib.mvlm_conv_wino4_padded_stride(c) for c in (84, 80, 96, 32, 33, 4, 128, 144)] == [96, 96, 96, 32, 64, 32, 128, 160]
    assert lib.mvlm_conv_wino4_padded_stride(0) == 0 and lib.mvlm_conv_wino4_padded_stride(-4) == 0


def test_padded_pack_is_the_plain_pack_with_zero_columns_behind():
    from mvlm_amd import _lib

    lib = _lib.load()
    rs = np.random.RandomState(12)
    # cin, cout, cin_pad, cout_pad: conv6 / conv10 of the 84- and the 73-landmark networks, a padded input chunk, a stride that stays
    for cin, cout, cin_pad, cout_pad in [(256, 84, 256, 84), (256, 73, 256, 80), (73, 84, 76, 84), (8, 73, 8, 80), (8, 64, 8, 64)]:
        P = lib.mvlm_conv_wino4_padded_stride(cout_pad)
        assert P == (cout_pad + 31) // 32 * 32
        w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        w9 = _pack9(w, cin_pad, cout_pad)
        bias = np.zeros(cout_pad, np.float32)
        bias[:cout] = rs.standard_normal(cout).astype(np.float32)
        plain = np.full((18, cin_pad, cout_pad), np.nan, np.float32)
        assert lib.mvlm_pack_winograd4_weights(w9.ctypes.data_as(FP), cin_pad, cout_pad, plain.ctypes.data_as(FP)) == 0
        wp = np.full((18, cin_pad, P), np.nan, np.float32)
        bp = np.full(P, np.nan, np.float32)
        assert lib.mvlm_pack_winograd4_weights_padded(w9.ctypes.data_as(FP), bias.ctypes.data_as(FP), cin_pad, cout_pad,
                                                      wp.ctypes.data_as(FP), bp.ctypes.data_as(FP)) == 0
        assert np.array_equal(wp[:, :, :cout_pad].view(np.uint32), plain.view(np.uint32))
        assert np.array_equal(wp[:, :, cout_pad:].view(np.uint32), np.zeros((18, cin_pad, P - cout_pad), np.uint32))  # +0, bit for bit
        assert np.array_equal(bp[:cout_pad].view(np.uint32), bias.view(np.uint32))
        assert np.array_equal(bp[cout_pad:].view(np.uint32), np.zeros(P - cout_pad, np.uint32))
        assert wp[:, :cin, :cout].all()  # the live block carries values
        # a layer without bias: the weights alone
        wp2 = np.full((18, cin_pad, P), np.nan, np.float32)
        assert lib.mvlm_pack_winograd4_weights_padded(w9.ctypes.data_as(FP), None, cin_pad, cout_pad, wp2.ctypes.data_as(FP), None) == 0
        assert np.array_equal(wp2.view(np.uint32), wp.view(np.uint32))


def test_padded_pack_refuses_null_and_empty_arguments():
    from mvlm_amd import _lib

    lib = _lib.load()
    w9 = np.zeros((9, 4, 84), np.float32)
    out = np.zeros((18, 4, 96), np.float32)
    bias = np.zeros(84, np.float32)
    p = lambda a: a.ctypes.data_as(FP)
    assert lib.mvlm_pack_winograd4_weights_padded(None, None, 4, 84, p(out), None) != 0
    assert lib.mvlm_pack_winograd4_weights_padded(p(w9), None, 4, 84, None, None) != 0
    assert lib.mvlm_pack_winograd4_weights_padded(p(w9), p(bias), 4, 84, p(out), None) != 0  # a bias with nowhere to go
    assert lib.mvlm_pack_winograd4_weights_padded(p(w9), None, 0, 84, p(out), None) != 0
    assert lib.mvlm_pack_winograd4_weights_padded(p(w9), None, 4, 0, p(out), None) != 0
