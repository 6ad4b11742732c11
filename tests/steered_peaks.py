"""Peaks of the planted detector (tests/planted.py) steered to chosen pixels, for the edges of the "moment" window.

`moment_refine_kernel` recomputes the 31x31 window around a peak from conv10's low-resolution output.  A peak in row 240 makes the
window's last row read low-resolution row 128 (the zero padding), a peak in row or column 16 puts the window's origin at an odd
pixel, and peaks at 15 and 241 must not be refined at all; seeded networks meet those rows and columns only by chance.

The construction: the detector without dense noise in the trunk; the image is R = G = 0 with uniform noise in B and in the depth
plane, and for landmark k with knots (i, j) and target (Y, X) the aligned 2x2 block at (2 (Y // 2), 2 (X // 2)) carries R = i / 16,
G = j / 16, so conv10's plane k peaks in one low-resolution pixel and the nearest-neighbour upsampling makes a four-way tie.
conv11.weight[k, k] gets +0.05 on the tap that sees the block's other row from row Y ((0, 1) for odd Y, (2, 1) for even) and on
the tap that sees its other column from column X ((1, 0) for odd X, (1, 2) for even): pixel (Y, X) wins with 1.10 of the peak
against 1.05.  Dense Gaussian noise on conv11.weight alone makes the window recomputation multiply full weight rows and stays
far below that gap.  Landmarks whose blocks are closer than 40 pixels go into different views.
Test helper, CPU only (numpy); used by tests/test_steered_peaks_cpu.py and tests/test_gpu_steered_peaks.py."""
from __future__ import annotations

import numpy as np

import planted

BOOST = 0.05
NOISE_EPS = 0.003   # of conv11's He scale: about 0.5 % of a peak on a plane's neighbourhood, against the 4.5 % gap of the boost
MIN_DISTANCE = 40
MAX_VIEWS = 6

EDGE_ROWS = [(15, 80), (16, 140), (240, 100), (241, 160)]           # thresholds of the refinement rule, interior column
EDGE_COLS = [(80, 15), (140, 16), (100, 240), (160, 241)]
CORNERS = [(16, 16), (16, 240), (240, 16), (240, 240), (15, 15), (241, 241), (15, 240), (240, 241)]
INTERIOR = [(100, 40), (61, 200), (180, 61), (201, 201)]            # one of each parity
IMAGE_CORNERS = [(0, 0), (0, 255), (255, 0), (255, 255)]            # for the simple selection
# every threshold value as a row and as a column within four landmarks (the 16-row and the 4-row strip of conv11's tile)
STRIP16 = [(15, 241), (241, 15), (16, 16), (240, 240)]
STRIP4 = [(15, 240), (240, 15), (16, 241), (241, 16)]


def refined(y: int, x: int) -> bool:
    """paulsenpredictor.py:131: the centroid replaces peaks more than 15 pixels inside."""
    return 15 < y < 241 and 15 < x < 241


def targets(nl: int) -> list[tuple[int, int, int]]:
    """(landmark, Y, X): the full list on channels 0..63 of conv11's tile, every threshold on the 16-row strip (64..79) and, for 84
    landmarks, on the 4-row strip (80..83)."""
    first = EDGE_ROWS + EDGE_COLS + CORNERS + INTERIOR + IMAGE_CORNERS
    out = [((5 * n) % 64, y, x) for n, (y, x) in enumerate(first)]
    strip16 = [64, 66, 69, 72] if nl == 73 else [64, 69, 74, 79]
    out += [(k, y, x) for k, (y, x) in zip(strip16, STRIP16)]
    if nl == 84:
        out += [(80 + n, y, x) for n, (y, x) in enumerate(STRIP4)]
    assert len({k for k, _, _ in out}) == len(out) and max(k for k, _, _ in out) < nl
    return out


def assign_views(tg) -> list[tuple[int, int, int, int]]:
    """(landmark, view, Y, X): each target in the first view whose blocks are all at least MIN_DISTANCE pixels from its own."""
    views: list[list[tuple[int, int]]] = []
    plan = []
    for k, y, x in tg:
        by, bx = 2 * (y // 2), 2 * (x // 2)
        for v, blocks in enumerate(views):
            if all(max(abs(by - oy), abs(bx - ox)) >= MIN_DISTANCE for oy, ox in blocks):
                break
        else:
            views.append([])
            v = len(views) - 1
        views[v].append((by, bx))
        plan.append((k, v, y, x))
    assert len(views) <= MAX_VIEWS, len(views)
    return plan


def steered_scene(nl: int, mode: str, seed: int = 0):
    """(state dict, images [V,256,256,4] f32, plan [(landmark, view, Y, X)])"""
    knots = planted.landmark_knots(nl, seed)
    sd = planted.planted_state_dict(nl, mode, knots)
    plan = assign_views(targets(nl))
    n_views = 1 + max(v for _, v, _, _ in plan)
    rs = np.random.RandomState(seed + 17)
    images = np.zeros((n_views, 256, 256, 4), np.float32)
    images[..., 2] = rs.randint(0, 256, (n_views, 256, 256)) / np.float32(255)
    images[..., 3] = rs.randint(0, 256, (n_views, 256, 256)) / np.float32(255)
    w11 = sd["conv11.weight"]
    for k, v, y, x in plan:
        by, bx = 2 * (y // 2), 2 * (x // 2)
        i, j = knots[k]
        images[v, by:by + 2, bx:bx + 2, 0] = i / planted.N_KNOTS
        images[v, by:by + 2, bx:bx + 2, 1] = j / planted.N_KNOTS
        w11[k, k, 0 if y % 2 else 2, 1] += BOOST
        w11[k, k, 1, 0 if x % 2 else 2] += BOOST
    fan_in = w11.shape[1] * 9
    w11 += (NOISE_EPS * np.sqrt(2.0 / fan_in) * rs.standard_normal(w11.shape)).astype(np.float32)
    return sd, images, plan


def check_targets(maxima_simple: np.ndarray, plan) -> list:
    """Steered planes whose argmax pixel in [NL,V,3] "simple" maxima (row - 1, col - 0.5, value) is not the target."""
    return [(k, v, y, x, tuple(maxima_simple[k, v, :2])) for k, v, y, x in plan
            if maxima_simple[k, v, 0] != y - 1 or maxima_simple[k, v, 1] != x - 0.5]
