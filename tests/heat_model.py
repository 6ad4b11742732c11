"""The heat-sheet contract ("Heat sheet") restated in numpy: the checker of mvlm_heat_plane_peaks and of
mvlm_render_heat_sheet.  It shares nothing with mvlm_amd/csrc/heat_sheet_math.h; the layout and the background are the view
sheet's, taken from tests/sheet_model.py.

Peak: m[v, l] = the largest finite value of heat[v, l] (float32), -inf when the plane has none.  Composition, per view pixel (v, y,
x) - heat pixel [row, col] lies over image pixel [row, col]: among the selected landmarks l in ascending order those with m[v, l]
finite and > 0 and h = heat[v, l, y, x] finite are candidates with t = float64(h) / float64(m); the largest t wins, the lowest l on
equal t.  No candidate, or t <= floor: the background stays.  Otherwise a = opacity * (t - floor) / (1.0 - floor) and per channel
out = int(bg + a * (col - bg) + 0.5), bg the background's byte and col the colour's as float64; the result fills the scale x scale
sheet pixels of the view pixel.  All float64, one rounding per operation."""
import numpy as np

import sheet_model as sm

RED = (255, 0, 0)


def peaks(heat) -> np.ndarray:
    """float32 [..., 256, 256] -> float32 [...]: the largest finite value of each plane, -inf where there is none."""
    h = np.asarray(heat, np.float32)
    flat = h.reshape(h.shape[:-2] + (-1,))
    masked = np.where(np.isfinite(flat), flat, np.float32(-np.inf))
    return masked.max(axis=-1).astype(np.float32)


def winners(heat_v, selected, floor):
    """One view's planes float32 [NL,256,256] -> (index [256,256] of the winning landmark, -1 where nothing is drawn; t [256,256])."""
    nl = heat_v.shape[0]
    m = peaks(heat_v)
    best_t = np.full(heat_v.shape[1:], -np.inf, np.float64)
    best_l = np.full(heat_v.shape[1:], -1, np.int64)
    for l in range(nl):
        if not selected[l] or not (np.isfinite(m[l]) and m[l] > 0):
            continue
        h = heat_v[l]
        ok = np.isfinite(h)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.where(ok, h, np.float32(0)).astype(np.float64) / np.float64(m[l])
        better = ok & (t > best_t)                          # strictly: the lowest index keeps a tie
        best_t = np.where(better, t, best_t)
        best_l = np.where(better, l, best_l)
    drawn = (best_l >= 0) & (best_t > np.float64(floor))
    return np.where(drawn, best_l, -1), best_t


def render(images, heat, landmarks=None, colors=None, background="rgb", cols=None, scale=1, gap=2, floor=0.25, opacity=0.75) -> np.ndarray:
    """-> uint8 [H,W,3], what render_heat_sheet gives."""
    images = np.asarray(images, np.float32)
    heat = np.asarray(heat, np.float32)
    n, nl = heat.shape[:2]
    sheet = sm.render(images, background=background, cols=cols, scale=scale, gap=gap)   # the views alone
    c, _, _, _ = sm.layout(n, cols, scale, gap)
    side = sm.VIEW * scale
    selected = np.ones(nl, bool) if landmarks is None else np.isin(np.arange(nl), np.asarray(list(landmarks), np.int64))
    colors = np.tile(np.asarray(RED, np.uint8), (nl, 1)) if colors is None else np.asarray(colors, np.uint8).reshape(nl, 3)
    floor, opacity = np.float64(floor), np.float64(opacity)
    for v in range(n):
        y0, x0 = gap + (v // c) * (side + gap), gap + (v % c) * (side + gap)
        bg = sheet[y0:y0 + side:scale, x0:x0 + side:scale].astype(np.float64)      # one sheet pixel per view pixel
        win, t = winners(heat[v], selected, floor)
        drawn = win >= 0
        with np.errstate(invalid="ignore"):
            a = opacity * (t - floor) / (np.float64(1.0) - floor)
        col = colors[np.where(drawn, win, 0)].astype(np.float64)
        with np.errstate(invalid="ignore"):
            mixed = (bg + a[..., None] * (col - bg) + 0.5)
        cell = np.where(drawn[..., None], np.where(drawn[..., None], mixed, 0.0).astype(np.int32), bg.astype(np.int32)).astype(np.uint8)
        sheet[y0:y0 + side, x0:x0 + side] = np.repeat(np.repeat(cell, scale, axis=0), scale, axis=1)
    return sheet
