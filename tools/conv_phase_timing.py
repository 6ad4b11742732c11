#!/usr/bin/env python3
"""Where a convolution workgroup spends its cycles: prologue / K loop / epilogue of wave 0, summed over
the workgroups of one launch (diagnostic build of the library with -DMVLM_CONV_TIMING, see
mvlm_amd/csrc/conv_tile.h; the launch's side in conv_launch.h).  Run on the GPU box:

  make -C mvlm_amd/csrc timing        # builds mvlm_amd/lib/libmvlm_hip_timing.so
  MVLM_HIP_LIB=mvlm_amd/lib/libmvlm_hip_timing.so python tools/conv_phase_timing.py

MVLM_PHASE_WINO4_ALONE=1 runs every forced F(4,3) case a second time with one workgroup per CU (the timing build pads the launch's
dynamic LDS, MVLM_CONV_TIMING_WINO4_LDS), and both runs print their K loop in cycles per 4-channel chunk: with a partner the two
workgroups share the matrix pipe (2 x 36 MFMAs of 64 cycles = 4 608 per chunk), alone the pipe needs 2 304 and whatever else a chunk
costs is cycles in which the wave had no MFMA of its own to issue.
"""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mvlm_amd import _lib  # noqa: E402

CASES = [  # name, cin, cout, size, k, batch, pre-BN, residual, bias+post-BN  (MVLM_PHASE_BATCH overrides the batch)
    ("block conv1  256->128 @128 (c128)", 256, 128, 128, 3, 64, True, True, False),
    ("conv5        256->256 @128 (c128)", 256, 256, 128, 3, 64, False, False, True),
    ("block conv2  128-> 64 @128 (c64)", 128, 64, 128, 3, 64, True, True, False),
    ("block conv3   64-> 64 @128 (c64)", 64, 64, 128, 3, 64, True, True, False),
    ("stem conv1    64-> 64 @256 (c64)", 64, 64, 256, 3, 64, True, True, False),
    ("block conv1  256->128 @ 64 (c128)", 256, 128, 64, 3, 64, True, True, False),
    ("resample 1x1  64->128 @256", 64, 128, 256, 1, 64, True, False, False),
    ("conv6        256-> 73 @128 (c80)", 256, 73, 128, 3, 64, False, False, False),
    # the F(2,3) Winograd tile (variant 40, conv3x3w_c64_t8x32), forced: its own prologue / K loop / epilogue split
    ("winograd     256->128 @128 (w64)", 256, 128, 128, 3, 64, True, True, False, 40),
    ("winograd     128-> 64 @128 (w64)", 128, 64, 128, 3, 64, True, True, False, 40),
    ("winograd      64-> 64 @ 64 (w64)", 64, 64, 64, 3, 64, True, True, False, 40),
    # the F(4,3) Winograd tile (variant code 2048, conv3x3q_c32_t16x32), forced; the last field is mvlm_cnn_set_winograd4_wide:
    # q32 the 32 x 16 workgroup shape, q64 the wide one (64 output channels x 8 rows; a 32-channel layer has the first only)
    ("winograd4    256->128 @128 (q32)", 256, 128, 128, 3, 64, True, True, False, 2048, 0),
    ("winograd4    128-> 64 @128 (q32)", 128, 64, 128, 3, 64, True, True, False, 2048, 0),
    ("winograd4     64-> 64 @ 64 (q32)", 64, 64, 64, 3, 64, True, True, False, 2048, 0),
    ("winograd4     64-> 32 @256 (q32)", 64, 32, 256, 3, 64, True, True, False, 2048, 0),
    ("winograd4    256->128 @128 (q64)", 256, 128, 128, 3, 64, True, True, False, 2048, 1),
    ("winograd4    128-> 64 @128 (q64)", 128, 64, 128, 3, 64, True, True, False, 2048, 1),
    ("winograd4     64-> 64 @ 64 (q64)", 64, 64, 64, 3, 64, True, True, False, 2048, 1),
    ("direct        64-> 32 @256 (c32)", 64, 32, 256, 3, 64, True, True, False, 3),
]


SMALL = [  # the latency-bound levels of a 12-view batch (MVLM_PHASE_CASES=small; MVLM_PHASE_CASES=winograd: the forced Winograd cases alone, winograd4: the F(4,3) tile's)
    ("block conv1  256->128 @ 32 B12", 256, 128, 32, 3, 12, True, True, False),
    ("block conv2  128-> 64 @ 32 B12", 128, 64, 32, 3, 12, True, True, False),
    ("block conv1  256->128 @ 16 B12", 256, 128, 16, 3, 12, True, True, False),
    ("block conv2  128-> 64 @ 16 B12", 128, 64, 16, 3, 12, True, True, False),
    ("block conv3   64-> 64 @ 16 B12", 64, 64, 16, 3, 12, True, True, False),
    ("block conv1  256->128 @  8 B12", 256, 128, 8, 3, 12, True, True, False),
    ("block conv2  128-> 64 @  8 B12", 128, 64, 8, 3, 12, True, True, False),
    ("block conv3   64-> 64 @  8 B12", 64, 64, 8, 3, 12, True, True, False),
    ("block conv1  256->128 @  4 B12", 256, 128, 4, 3, 12, True, True, False),
    ("block conv3   64-> 64 @  4 B12", 64, 64, 4, 3, 12, True, True, False),
    ("block conv1  256->128 @ 64 B12", 256, 128, 64, 3, 12, True, True, False),
    ("block conv2  128-> 64 @ 64 B12", 128, 64, 64, 3, 12, True, True, False),
]


def main():
    global CASES
    if os.environ.get("MVLM_PHASE_CASES") == "small":
        CASES = SMALL
    ctx = _lib.get_context(0)
    buf = torch.zeros(4, dtype=torch.int64, device="cuda")
    os.environ["MVLM_CONV_TIMING_BUF"] = hex(buf.data_ptr())
    rs = np.random.RandomState(0)
    f = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    print(f"{'layer':40s} {'ms':>7s} {'TFLOP/s':>8s} | per workgroup, wave 0: prologue / K loop / epilogue (cycles, share)")
    if os.environ.get("MVLM_PHASE_CASES") == "winograd":
        CASES = [c for c in CASES if len(c) > 9]
    if os.environ.get("MVLM_PHASE_CASES") == "winograd4":
        CASES = [c for c in CASES if len(c) > 9 and c[9] == 2048]
    alone = os.environ.get("MVLM_PHASE_WINO4_ALONE") == "1"
    runs = [(c, wgs) for c in CASES for wgs in ((2, 1) if alone and len(c) > 9 and c[9] == 2048 else (2,))]
    for (name, cin, cout, size, k, batch, pre, res, post, *forced), wgs in runs:
        if wgs == 1:  # more than half of a CU's 160 KiB of LDS: one workgroup per CU
            os.environ["MVLM_CONV_TIMING_WINO4_LDS"] = str(96 * 1024)
            name += " alone"
        else:
            os.environ.pop("MVLM_CONV_TIMING_WINO4_LDS", None)
        batch = int(os.environ.get("MVLM_PHASE_BATCH", batch))
        x = torch.randn(batch, cin, size, size, device="cuda")
        y = torch.empty(batch, cout, size, size, device="cuda")
        r = torch.randn(batch, cout, size, size, device="cuda") if res else None
        w = (rs.standard_normal((cout, cin, k, k)) * 0.05).astype(np.float32)
        b = rs.standard_normal(cout).astype(np.float32) if (post or not pre) else None
        ps, pt = (rs.rand(cin).astype(np.float32) + 0.5, rs.standard_normal(cin).astype(np.float32)) if pre else (None, None)
        qs, qt = (rs.rand(cout).astype(np.float32) + 0.5, rs.standard_normal(cout).astype(np.float32)) if post else (None, None)
        times = []
        for it in range(3):
            buf.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            e0.record()
            if forced:
                ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, forced[0]))
            if len(forced) > 1:
                ctx.check(ctx.lib.mvlm_cnn_set_winograd4_wide(ctx.handle, forced[1]))
            try:
                ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(x.data_ptr()), batch, cin, size, size, f(w), cout, k, f(b),
                                              f(ps), f(pt), f(qs), f(qt), C.c_void_p(r.data_ptr()) if res else None, 0,
                                              C.c_void_p(y.data_ptr())))
            finally:
                if forced:
                    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
                if len(forced) > 1:
                    ctx.check(ctx.lib.mvlm_cnn_set_winograd4_wide(ctx.handle, 1))
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        t = buf.cpu().numpy().astype(np.float64)
        n = max(t[3], 1)
        tot = t[:3].sum()
        ms = min(times)  # includes the hook's host-side packing only before the launch; event pair brackets the kernel + H2D
        flops = 2.0 * cin * cout * k * k * size * size * batch
        print(f"{name:40s} {ms:7.3f} {flops / ms / 1e9:8.1f} | {t[0] / n:9.0f} {t[1] / n:9.0f} {t[2] / n:9.0f}   "
              f"{100 * t[0] / tot:4.1f}% {100 * t[1] / tot:4.1f}% {100 * t[2] / tot:4.1f}%   ({int(n)} workgroups)"
              + (f"   K loop {t[1] / n / (cin / 4):6.0f} cycles per chunk, {wgs} workgroup{'s' if wgs > 1 else ''} per CU" if forced and forced[0] == 2048 else ""))
        del x, y, r


if __name__ == "__main__":
    main()
