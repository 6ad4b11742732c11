"""The timing hook mvlm_conv_bench (mvlm_amd/csrc/conv_hooks.hip) on each form of the weights it hands out of its one zero arena:
an F(2,3) launch, an F(4,3) launch and a launch of the 84-row tile that the dispatcher runs on the F(4,3) tile over padded weights.
It shows that the arena (conv_pack.cpp: mvlm_conv_pack_arena_floats) holds every form; it times nothing."""
import ctypes as C

import pytest

from mvlm_amd import _lib

pytestmark = pytest.mark.gpu

WINO4 = 2048  # MVLM_CONV_VARIANT_WINO4


def _bench(ctx, cin, cout, flags, variant):
    ms, used = C.c_float(-1.0), C.c_int(-1)
    ctx.check(ctx.lib.mvlm_conv_bench(ctx.handle, 1, cin, cout, 3, 32, flags, variant, 2, C.byref(ms), C.byref(used)))
    ctx.synchronize()
    assert ms.value >= 0.0
    return used.value


@pytest.mark.parametrize("variant", [40, WINO4])
def test_bench_hook_on_a_winograd_form(variant):
    assert _bench(_lib.get_context(0), 8, 64, 0, variant) == variant


def test_bench_hook_on_the_padded_form(monkeypatch):
    monkeypatch.setenv("MVLM_WINOGRAD4_PADDED", "2")  # (a context reads it when it is made)
    ctx = _lib.Context(0)
    try:
        n = C.c_int64(-1)
        ctx.check(ctx.lib.mvlm_conv_wino4_padded_launches(ctx.handle, C.byref(n), 1))
        assert n.value == 0
        assert _bench(ctx, 8, 84, 4, -1) == WINO4  # (plain with bias: 84 rows unpadded; the launch that ran is reported)
        ctx.check(ctx.lib.mvlm_conv_wino4_padded_launches(ctx.handle, C.byref(n), 0))
        assert n.value == 3  # the warm-up and two timed launches
    finally:
        ctx.close()
