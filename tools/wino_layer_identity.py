#!/usr/bin/env python3
"""Are the forced Winograd layers of two builds of the library the same bytes?

    MVLM_HIP_LIB=<one build>/libmvlm_hip.so     python tools/wino_layer_identity.py dump DIR_A
    MVLM_HIP_LIB=<another build>/libmvlm_hip.so python tools/wino_layer_identity.py dump DIR_B
    python tools/wino_layer_identity.py compare DIR_A DIR_B [more .npy names to compare as well]

`dump` runs every layer of tests/test_gpu_winograd.py::LAYER_CASES (same seeds, same tensors) with variant 40 forced through
mvlm_conv2d and writes the outputs as .npy; `compare` compares the files of two such directories byte for byte (also those
bench.py --dump-outputs left there) and exits 1 when one differs.  A rewrite of the tile's K loop that keeps products, their
order and both transforms must leave every byte where it was."""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))


def dump(out: Path) -> None:
    import test_gpu_winograd as T
    from mvlm_amd import _lib

    out.mkdir(parents=True, exist_ok=True)
    ctx = _lib.get_context(0)
    print(f"library: {_lib.LIB_PATH}")
    for variant in T.WINO_IDS:
        for cin, cout, size, batch, opts in T.LAYER_CASES:
            rs = np.random.RandomState(cin * 7 + cout + size)
            x = rs.standard_normal((batch, cin, size, size)).astype(np.float32)
            w = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
            bias = rs.standard_normal(cout).astype(np.float32) if opts.get("bias") else None
            pre = (rs.uniform(0.5, 1.5, cin).astype(np.float32), rs.standard_normal(cin).astype(np.float32) * 0.3) if opts.get("pre") else None
            post = (rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.standard_normal(cout).astype(np.float32) * 0.3) if opts.get("post") else None
            res = rs.standard_normal((batch, cout, size, size)).astype(np.float32) if opts.get("res") else None
            y = T._layer(ctx, variant, x, w, bias, pre, post, res)
            assert np.isfinite(y).all() and np.abs(y).max() > 0
            name = f"layer_v{variant}_{cin}_{cout}_{size}_b{batch}_{'-'.join(sorted(opts)) or 'plain'}.npy"
            np.save(out / name, y)
            print(f"{name}: {y.size} floats, |y|max {np.abs(y).max():.6f}")


def compare(a: Path, b: Path, extra) -> int:
    names = sorted(p.name for p in a.glob("layer_*.npy")) + list(extra)
    bad = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        d = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.shape == y.shape else float("nan")
        print(f"{n}: {x.dtype}{list(x.shape)} identical {same} max |diff| {d:.3e}")
        bad += not same
    print(f"{len(names)} files compared, {bad} differ")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(Path(sys.argv[2]))
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(Path(sys.argv[2]), Path(sys.argv[3]), sys.argv[4:]))
    else:
        sys.exit(__doc__)
