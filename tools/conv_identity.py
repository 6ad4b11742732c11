#!/usr/bin/env python3
"""Do the convolutions of two builds of the library compute the same bytes?

    MVLM_HIP_LIB=<one build>/libmvlm_hip.so     python tools/conv_identity.py dump DIR_A
    MVLM_HIP_LIB=<another build>/libmvlm_hip.so python tools/conv_identity.py dump DIR_B
    python tools/conv_identity.py compare DIR_A DIR_B [.npy names to compare as well]

`dump` writes DIR/conv_identity.json, name -> shape, dtype, sha256 of
  - every layer of tests/test_gpu_winograd.py::LAYER_CASES with variant 40 forced (same seeds, same tensors),
  - every layer of tests/test_gpu_winograd4.py::LAYER_CASES with the F(4,3) tile's code 2048 forced, likewise,
  - tests/test_gpu_parity.py::CONV_CASES through mvlm_conv2d,
  - tests/test_gpu_round4.py::PAIR_CASES through mvlm_conv2d_pair (both problems' outputs and raw copies),
  - the cases of test_two_column_split_k_tiles_match_torch with their variant forced,
  - the heatmaps (mvlm_cnn_heatmaps) and maxima (mvlm_cnn_maxima: values and indices) of both network families, 73 landmarks /
    3 channels and 84 / 4, with the seeded weights and images of tests/test_gpu_conv_routing.py, in each of its PASSES
    (Winograd mode x pairing x device batch) - the passes that reach the raw-copy, pooling, scatter, two-residual,
    second-input, K-parts and fused-argmax forms of the tile program.
`compare` compares two such tables entry by entry, and the named .npy files of the two directories (bench.py --dump-outputs
leaves landmarks.npy and ransac_error.npy) byte for byte; it exits 1 when anything differs or is missing.  A rewrite of the
tile program that keeps every product, sum order and store must leave every byte where it was."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
TABLE = "conv_identity.json"


def _entry(a) -> dict:
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def _tensors(rs, cin, cout, size, k, batch, opts):
    """the tensors of a single-layer test, drawn in its order"""
    s_in = size // 2 if opts.get("up") else size
    x = rs.standard_normal((batch, cin, s_in, s_in)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    bias = rs.standard_normal(cout).astype(np.float32) if opts.get("bias") else None
    pre = (rs.uniform(0.5, 1.5, cin).astype(np.float32), rs.standard_normal(cin).astype(np.float32) * 0.3) if opts.get("pre") else None
    post = (rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.standard_normal(cout).astype(np.float32) * 0.3) if opts.get("post") else None
    res = rs.standard_normal((batch, cout, size, size)).astype(np.float32) if opts.get("res") else None
    return x, w, bias, pre, post, res


def _conv2d(ctx, x, w, bias, pre, post, res, up=False, variant=-1):
    import torch

    batch, cin = x.shape[:2]
    cout, k = w.shape[0], w.shape[2]
    size = x.shape[2] * (2 if up else 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    xd, yd = dev(x), torch.empty((batch, cout, size, size), dtype=torch.float32, device="cuda")
    rd = dev(res) if res is not None else None
    ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, variant))
    try:
        ctx.check(ctx.lib.mvlm_conv2d(ctx.handle, C.c_void_p(xd.data_ptr()), batch, cin, size, size, p(w), cout, k, p(bias),
                                      p(pre[0]) if pre else None, p(pre[1]) if pre else None, p(post[0]) if post else None, p(post[1]) if post else None,
                                      C.c_void_p(rd.data_ptr()) if rd is not None else None, int(up), C.c_void_p(yd.data_ptr())))
    finally:
        ctx.check(ctx.lib.mvlm_conv_force_variant(ctx.handle, -1))
    y = yd.cpu().numpy()
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    return y


def _layers(ctx, table) -> None:
    import test_gpu_parity as TP
    import test_gpu_round4 as T4
    import test_gpu_winograd as TW
    import test_gpu_winograd4 as TW4
    import torch

    tag = lambda opts: "-".join(sorted(opts)) or "plain"
    for variant, cases in [(v, TW.LAYER_CASES) for v in TW.WINO_IDS] + [(TW4.WINO4, TW4.LAYER_CASES)]:
        for cin, cout, size, batch, opts in cases:
            t = _tensors(np.random.RandomState(cin * 7 + cout + size), cin, cout, size, 3, batch, opts)
            table[f"layer_v{variant}_{cin}_{cout}_{size}_b{batch}_{tag(opts)}"] = _entry(_conv2d(ctx, *t, variant=variant))
    for cin, cout, size, k, batch, opts in TP.CONV_CASES:
        t = _tensors(np.random.RandomState(cin * 7 + cout + size), cin, cout, size, k, batch, opts)
        table[f"conv_{cin}_{cout}_{size}_k{k}_b{batch}_{tag(opts)}"] = _entry(_conv2d(ctx, *t, up=bool(opts.get("up"))))
    for variant, _, cin, cout, size, batch, _ in T4.test_two_column_split_k_tiles_match_torch.pytestmark[0].args[1]:
        t = _tensors(np.random.RandomState(cin + size + batch + variant), cin, cout, size, 3, batch, dict(pre=True, res=True))
        table[f"twocol_v{variant}_{cin}_{cout}_{size}_b{batch}"] = _entry(_conv2d(ctx, *t, variant=variant))
    ptr, p = (lambda t: C.c_void_p(t.data_ptr())), T4.p
    for code, _, cin, cout, size, batch in T4.PAIR_CASES:
        rs = np.random.RandomState(code + cin + size + batch)
        pre = (rs.uniform(0.5, 1.5, cin).astype(np.float32), (rs.standard_normal(cin) * 0.3).astype(np.float32))
        xs, ws, res, ys, raws = [], [], [], [], []
        for s in (size, size // 2):
            xs.append(T4.dev(rs.standard_normal((batch, cin, s, s)).astype(np.float32)))
            ws.append((rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32))
            res.append(T4.dev(rs.standard_normal((batch, cout, s, s)).astype(np.float32)))
            ys.append(torch.full((batch, cout, s, s), np.nan, dtype=torch.float32, device="cuda"))
            raws.append(torch.full((batch, cout, s, s), np.nan, dtype=torch.float32, device="cuda"))
        ctx.check(ctx.lib.mvlm_conv2d_pair(ctx.handle, batch, cin, cout, ptr(xs[0]), size, p(ws[0]), ptr(res[0]), ptr(raws[0]), ptr(ys[0]),
                                           ptr(xs[1]), size // 2, p(ws[1]), ptr(res[1]), ptr(raws[1]), ptr(ys[1]), p(pre[0]), p(pre[1]), code))
        for i in range(2):
            assert bool(torch.isfinite(ys[i]).all()) and bool(torch.isfinite(raws[i]).all())
            table[f"pair_{code}_{cin}_{cout}_{size}_b{batch}_out{i}"] = _entry(ys[i].cpu().numpy())
            table[f"pair_{code}_{cin}_{cout}_{size}_b{batch}_raw{i}"] = _entry(raws[i].cpu().numpy())


def _networks(table) -> None:
    import test_gpu_conv_routing as TR
    import torch
    from conftest import seeded_images
    from mvlm_amd.prediction import BU3DFEPredictor, DTU3DPredictor

    images = torch.from_numpy(seeded_images(9, 12)).cuda()
    for name, cls, mode in (("nl73c3", DTU3DPredictor, "RGB"), ("nl84c4", BU3DFEPredictor, "RGB+depth")):
        pred = cls(image_mode=mode, weights="synthetic:6", verbose=False)
        ctx = pred.ctx
        try:
            for wino, pairing, batch in TR.PASSES:
                ctx.check(ctx.lib.mvlm_cnn_set_winograd(ctx.handle, wino))
                pred.set_execution(graphs=False, pairing=pairing)
                x = images[:batch].contiguous()
                key = f"{name}_winograd{wino}_pairing{pairing}_batch{batch}"
                table[key + "_maxima"] = _entry(pred.predict_device(x).cpu().numpy())
                table[key + "_heatmaps"] = _entry(pred.heatmaps_device(x).cpu().numpy())
        finally:
            ctx.check(ctx.lib.mvlm_cnn_set_winograd(ctx.handle, 1))
            pred.set_execution(graphs=True, pairing=1)


def dump(out: Path) -> None:
    from mvlm_amd import _lib

    out.mkdir(parents=True, exist_ok=True)
    print(f"library: {_lib.LIB_PATH}")
    table = {}
    _layers(_lib.get_context(0), table)
    _networks(table)
    (out / TABLE).write_text(json.dumps(table, indent=1) + "\n")
    print(f"{len(table)} tensors -> {out / TABLE}")


def compare(a: Path, b: Path, extra) -> int:
    ta, tb = json.loads((a / TABLE).read_text()), json.loads((b / TABLE).read_text())
    bad = 0
    for n in sorted(set(ta) | set(tb)):
        same = n in ta and n in tb and ta[n] == tb[n]
        e = ta.get(n) or tb[n]
        print(f"{n}: {e['dtype']}{e['shape']} identical {same}")
        bad += not same
    for n in extra:
        same = (a / n).is_file() and (b / n).is_file() and (a / n).read_bytes() == (b / n).read_bytes()
        print(f"{n}: file identical {same}")
        bad += not same
    total = len(set(ta) | set(tb)) + len(extra)
    print(f"{total} compared, {bad} differ")
    return 1 if bad or not total else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(Path(sys.argv[2]))
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(Path(sys.argv[2]), Path(sys.argv[3]), sys.argv[4:]))
    else:
        sys.exit(__doc__)
