#!/usr/bin/env python3
"""The outputs of the F(4,3) Winograd tile on the shapes that reach every path of its chunk schedule, as sha256 digests.

    python tools/wino4_schedule_digests.py            print the table of the loaded library (MVLM_HIP_LIB names another build)
    python tools/wino4_schedule_digests.py --write    rewrite tests/golden/wino4_schedule_digests.json from it

A change to how a chunk of the tile is scheduled - where its loads, its staging arithmetic, its LDS writes, its waits and its
barrier sit among the MFMAs - keeps every product, every sum order and every store, so it must leave every output byte where it
was.  The committed table was written on an MI355X from the library of the commit BEFORE the staging was spread over the MFMA
gaps; tests/test_gpu_winograd4_schedule.py imports the cases and the tensors from here and holds the built library to it.

A case runs through mvlm_conv2d with the tile's code 2048 forced (the padded case: unforced, under mvlm_cnn_set_winograd4_padded 2,
where the dispatcher hands the 84-row layer to the tile), under mvlm_cnn_set_winograd4_wide 0 and 1.  The tensors are seeded and
drawn as tools/conv_identity.py::_tensors draws them.

Chunks are four input channels.  cin 4: one chunk (nothing staged in the loop); 8: two chunks, no steady loop; 12: three, the odd
entry, steady loop not entered; 16: the steady loop once, even count; 20: once, odd; 24: twice; 22: cin_pad 24 with a padded last
chunk behind a steady loop; 73: the longest.  cout 64 runs on either workgroup shape, cout 32 on the 32 x 16 shape only.  Size 32 is
one x tile with both side borders and the top and bottom borders in different row tiles; size 64 adds interior tile seams."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
TABLE = REPO / "tests" / "golden" / "wino4_schedule_digests.json"
WINO4 = 2048  # MVLM_CONV_VARIANT_WINO4
PLAIN, PRE_RES, BIAS_POST = dict(), dict(pre=True, res=True), dict(bias=True, post=True)  # test_gpu_winograd4.py::LAYER_CASES' options

CASES = [
    # cin, cout, size, batch, opts, padded (mvlm_cnn_set_winograd4_padded)
    (4, 64, 32, 1, PLAIN, 1),
    (8, 64, 32, 2, PRE_RES, 1),
    (12, 64, 32, 1, BIAS_POST, 1),
    (16, 64, 32, 3, PRE_RES, 1),
    (20, 64, 32, 1, PLAIN, 1),
    (24, 64, 32, 1, BIAS_POST, 1),
    (22, 64, 32, 2, PRE_RES, 1),
    (73, 64, 32, 1, PRE_RES, 1),
    (20, 64, 64, 2, BIAS_POST, 1),
    (4, 32, 32, 1, PRE_RES, 1),
    (12, 32, 32, 2, PLAIN, 1),
    (22, 32, 32, 1, BIAS_POST, 1),
    (24, 32, 32, 3, PRE_RES, 1),
    (16, 84, 32, 2, dict(bias=True), 2),
]
WIDE = (0, 1)


def case_id(case, wide) -> str:
    cin, cout, size, batch, opts, padded = case
    return f"{cin}_{cout}_{size}_b{batch}_{'-'.join(sorted(opts)) or 'plain'}_padded{padded}_wide{wide}"


def tensors(case):
    """x, w, bias, pre, post, res of a case: seeded and drawn as tools/conv_identity.py::_tensors"""
    cin, cout, size, batch, opts, _ = case
    rs = np.random.RandomState(cin * 7 + cout + size)
    x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    bias = rs.standard_normal(cout).astype(np.float32) if opts.get("bias") else None
    pre = (rs.uniform(0.5, 1.5, cin).astype(np.float32), rs.standard_normal(cin).astype(np.float32) * 0.3) if opts.get("pre") else None
    post = (rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.standard_normal(cout).astype(np.float32) * 0.3) if opts.get("post") else None
    res = rs.standard_normal((batch, cout, size, size)).astype(np.float32) if opts.get("res") else None
    return x, w, bias, pre, post, res


def run_case(ctx, case, wide, t=None) -> np.ndarray:
    """the layer's output on the loaded library; the switches are put back to their defaults"""
    import torch

    cin, cout, size, batch, _, padded = case
    x, w, bias, pre, post, res = t if t is not None else tensors(case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    xd, rd = dev(x), (dev(res) if res is not None else None)
    yd = torch.full((batch, cout, size, size), float("nan"), dtype=torch.float32, device="cuda")
    lib, h = ctx.lib, ctx.handle
    ctx.check(lib.mvlm_cnn_set_winograd4_wide(h, wide))
    ctx.check(lib.mvlm_cnn_set_winograd4_padded(h, padded))
    ctx.check(lib.mvlm_conv_force_variant(h, WINO4 if padded == 1 else -1))
    try:
        ctx.check(lib.mvlm_conv2d(h, C.c_void_p(xd.data_ptr()), batch, cin, size, size, p(w), cout, 3, p(bias),
                                  p(pre[0]) if pre else None, p(pre[1]) if pre else None, p(post[0]) if post else None,
                                  p(post[1]) if post else None, C.c_void_p(rd.data_ptr()) if rd is not None else None, 0,
                                  C.c_void_p(yd.data_ptr())))
    finally:
        ctx.check(lib.mvlm_conv_force_variant(h, -1))
        ctx.check(lib.mvlm_cnn_set_winograd4_padded(h, 1))
        ctx.check(lib.mvlm_cnn_set_winograd4_wide(h, 1))
    return yd.cpu().numpy()


def padded_launches(ctx) -> int:
    """launches the dispatcher handed to the tile as padded ones since the last call"""
    n = C.c_int64()
    ctx.check(ctx.lib.mvlm_conv_wino4_padded_launches(ctx.handle, C.byref(n), 1))
    return int(n.value)


def digest(y: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def table(ctx) -> dict:
    out = {}
    for case in CASES:
        t = tensors(case)
        for wide in WIDE:
            padded_launches(ctx)
            y = run_case(ctx, case, wide, t)
            assert np.isfinite(y).all() and np.abs(y).max() > 0, case
            assert padded_launches(ctx) == (1 if case[5] == 2 else 0), case
            out[case_id(case, wide)] = digest(y)
    return out


if __name__ == "__main__":
    from mvlm_amd import _lib

    print(f"library: {_lib.LIB_PATH}")
    rows = table(_lib.get_context(0))
    for k, v in rows.items():
        print(f"{v}  {k}")
    if "--write" in sys.argv:
        TABLE.write_text(json.dumps(rows, indent=1) + "\n")
        print(f"{len(rows)} digests -> {TABLE}")
