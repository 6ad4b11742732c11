"""The network's final heatmaps against a float64 forward pass, at every pixel and class by class.

`oracle.cnn.forward_last_stage` is functional over a `{key: array}` state dict, so it runs unchanged in float64 when the state
dict and the input are float64: that tensor is the reference here.  The fp32 oracle (pinned bit for bit to the reference's own
vectors, tests/test_oracle_pinning.py) is measured against it first, per class of pixels - border rows and columns, the four
parities of conv11's collapsed 2x2 forms, the seams of the 8-row / 32-column tiles and of the lower levels' 64-pixel footprint -
and the HIP path's heatmaps are then held to a small multiple `m` of the oracle's own error in every class.  No number in a bound
comes from the HIP path.  Test helper, CPU only (numpy + torch); used by tests/test_net_reference_cpu.py,
tests/test_gpu_net_every_pixel.py and tests/reports/parity_stats.py.
"""
from __future__ import annotations

import numpy as np
import torch

S = 256  # heatmap size


def heatmaps_f64(sd, images: np.ndarray, chan_sel) -> np.ndarray:
    """[N,256,256,4] f32 images -> [N,NL,256,256] float64 heatmaps of the network `sd` evaluated in float64.
    The input is permuted as oracle.cnn.predict_landmarks_from_images permutes it (BHWC -> BCHW view of the selected planes)."""
    from oracle import cnn as ocnn

    sd64 = {}
    for k, v in sd.items():
        a = np.asarray(v)
        sd64[k] = a.astype(np.float64) if a.dtype.kind == "f" else a
    x = torch.from_numpy(np.ascontiguousarray(images[..., list(chan_sel)]).astype(np.float64)).permute(0, 3, 1, 2)
    out = [ocnn.forward_last_stage(sd64, x[i:i + 1]) for i in range(x.shape[0])]   # one view at a time: memory
    heat = torch.cat(out, 0)
    assert heat.dtype == torch.float64
    return heat.numpy()


def heatmaps_oracle(sd, images: np.ndarray, chan_sel) -> np.ndarray:
    """The fp32 oracle's heatmaps [N,NL,256,256] of the same views."""
    from oracle import cnn as ocnn

    _, _, heat = ocnn.predict_landmarks_from_images(sd, images, chan_sel, return_heatmaps=True)
    return heat.numpy()


BORDER_CLASSES = ("row0", "row1", "row254", "row255", "col0", "col1", "col254", "col255")
PARITY_CLASSES = ("par00", "par01", "par10", "par11")
SEAM_CLASSES = ("rowseam8", "colseam32", "seam64")


def pixel_classes() -> dict[str, np.ndarray]:
    """Boolean [256,256] masks, in the order they are reported."""
    yy, xx = np.mgrid[0:S, 0:S]
    cls: dict[str, np.ndarray] = {}
    for r in (0, 1, S - 2, S - 1):
        cls[f"row{r}"] = yy == r
    for c in (0, 1, S - 2, S - 1):
        cls[f"col{c}"] = xx == c
    for py in (0, 1):
        for px in (0, 1):
            cls[f"par{py}{px}"] = (yy % 2 == py) & (xx % 2 == px)
    cls["rowseam8"] = (yy % 8 == 0) | (yy % 8 == 7)
    cls["colseam32"] = (xx % 32 == 0) | (xx % 32 == 31)
    cls["seam64"] = (yy % 64 == 0) | (yy % 64 == 63) | (xx % 64 == 0) | (xx % 64 == 63)
    special = np.zeros((S, S), bool)
    for k in BORDER_CLASSES + SEAM_CLASSES:
        special |= cls[k]
    cls["interior"] = ~special
    cls["all"] = np.ones((S, S), bool)
    return cls


_CLASSES = None


def _classes():
    global _CLASSES
    if _CLASSES is None:
        _CLASSES = pixel_classes()
    return _CLASSES


def error_table(heat: np.ndarray, ref64: np.ndarray) -> dict[str, tuple[float, float]]:
    """{class: (E, M)}: max and mean of |heat - ref64| over the class's pixels of every plane, in units of S = max |ref64|."""
    assert heat.shape == ref64.shape and ref64.dtype == np.float64 and heat.shape[-2:] == (S, S)
    scale = np.abs(ref64).max()
    err = np.abs(heat.astype(np.float64) - ref64)
    err = err.reshape(-1, S, S)
    pix_max = err.max(axis=0)        # a class's max / mean over planes and pixels = max / mean of the per-pixel max / mean
    pix_mean = err.mean(axis=0)
    table = {}
    for k, mask in _classes().items():
        table[k] = (float(pix_max[mask].max() / scale), float(pix_mean[mask].mean() / scale))
    return table


def bounds(table_ref, m: float) -> dict[str, tuple[float, float]]:
    """{class: (bound on E, bound on M)}.  The max of a border class (about 37 000 samples) is an extreme-value statistic that two
    fp32 summation orders need not share, hence its floor at half the whole tensor's; the mean needs none."""
    e_all = table_ref["all"][0]
    return {k: (m * max(e, 0.5 * e_all), m * mu) for k, (e, mu) in table_ref.items()}


def check_against(table_gpu, table_ref, m: float) -> list[tuple[str, str, float, float]]:
    """Violations (class, "max" | "mean", value, bound) of `table_gpu` against `m` times the reference's own error."""
    out = []
    for k, (b_max, b_mean) in bounds(table_ref, m).items():
        e, mu = table_gpu[k]
        if not e <= b_max:           # (a NaN is a violation)
            out.append((k, "max", e, b_max))
        if not mu <= b_mean:
            out.append((k, "mean", mu, b_mean))
    return out


def format_table(title: str, table, table_ref=None, m: float | None = None) -> str:
    """One line per class: the value, and with a reference table the oracle's value, their ratio and the bound."""
    lines = [title]
    bnd = bounds(table_ref, m) if table_ref is not None and m is not None else None
    for k, (e, mu) in table.items():
        if table_ref is None:
            lines.append(f"  {k:10s} max {e:.3e}  mean {mu:.3e}")
        else:
            re, rm = table_ref[k]
            lines.append(f"  {k:10s} max {e:.3e} (oracle {re:.3e}, ratio {e / re:5.2f}, bound {bnd[k][0]:.3e})  "
                         f"mean {mu:.3e} (oracle {rm:.3e}, ratio {mu / rm:5.2f}, bound {bnd[k][1]:.3e})")
    return "\n".join(lines)


def lattice_criterion(heat: np.ndarray, ref: np.ndarray) -> bool:
    """The older whole-network criterion (tests/test_gpu_parity.py::test_full_network_against_reference_vectors): one pixel in
    256, rows 5 mod 16 and columns 3 mod 16, within 2e-4 of the reference's scale."""
    ref_sub = ref[:, :, 5::16, 3::16]
    return bool(np.abs(heat[:, :, 5::16, 3::16] - ref_sub).max() < 2e-4 * np.abs(ref_sub).max())


# The three networks of the every-pixel tests: (landmarks, image mode, weights, image seed, views)
NETWORKS = {
    "73-rgb-seeded": (73, "RGB", "synthetic:1", 501, 2),
    "84-rgbd-seeded": (84, "RGB+depth", "synthetic:2", 502, 2),
    "84-rgbd-planted": (84, "RGB+depth", "planted-dense", 503, 1),
}


_CASES: dict[str, dict] = {}


def reference_case(name: str) -> dict:
    """One of NETWORKS with its float64 heatmaps, the fp32 oracle's heatmaps and the oracle's error table, computed once per
    process (a few seconds of CPU per view) and left unchanged by its users."""
    if name not in _CASES:
        nl, mode, sd, images, sel = network_case(name)
        ref64 = heatmaps_f64(sd, images, sel)
        oheat = heatmaps_oracle(sd, images, sel)
        for a in (ref64, oheat):
            a.setflags(write=False)
        _CASES[name] = dict(name=name, nl=nl, mode=mode, sd=sd, images=images, sel=sel, ref64=ref64, oheat=oheat,
                            table_ref=error_table(oheat, ref64), scale=float(np.abs(ref64).max()))
    return _CASES[name]


def network_case(name: str):
    """(nl, mode, state dict, images [N,256,256,4], channel selection) of one of NETWORKS."""
    import planted
    from conftest import seeded_images
    from mvlm_amd import arch, weights

    nl, mode, w, img_seed, n = NETWORKS[name]
    if w == "planted-dense":
        sd = planted.planted_state_dict(nl, mode, planted.landmark_knots(nl, 0), dense_eps=0.003)
    else:
        sd = weights.synthetic_state_dict(nl, arch.IMAGE_CHANNELS[mode], seed=int(w.split(":")[1]))
    return nl, mode, sd, seeded_images(img_seed, n), arch.CHANNEL_SELECT[mode]
