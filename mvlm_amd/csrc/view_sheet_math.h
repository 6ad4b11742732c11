// Scalar arithmetic of the view sheet (view_sheet.hip): the layout of the cells, the record a prediction leaves per (view,
// landmark) and the two coverage tests a sheet pixel makes against it.  Host and device share it; everything that decides a pixel
// is float64 in the operation order written here (the Makefile's -ffp-contract=off keeps multiply and add apart), so numpy
// reproduces it.  The tests do NOT share this file: tests/sheet_model.py is an independent restatement ("View
// sheet").
#ifndef MVLM_VIEW_SHEET_MATH_H
#define MVLM_VIEW_SHEET_MATH_H

#include "raster_math.h"

#define VS_MAX_SIDE 4096 /* of the sheet: mvlm_png_encode's limit */
#define VS_MAX_SCALE 4
#define VS_MAX_GAP 16
#define VS_MAX_LANDMARKS 65536
#define VS_RADIUS_MIN 0.5
#define VS_RADIUS_MAX 16.0
#define VS_GREY 0x808080u /* gaps and empty cells */
#define VS_RED 0x0000FFu  /* residuals: r | g << 8 | b << 16 */
#define VS_BLUE 0xFF0000u /* markers without a colour of their own */
#define VS_MARKER 1u      /* the record draws a marker ... */
#define VS_RING 2u        /* ... as a ring (the view did not survive the filter) */
#define VS_SEGMENT 4u     /* the record draws a residual */

/* layout errors (mvlm_view_sheet_layout words them) */
#define VS_OK 0
#define VS_BAD_VIEWS 1
#define VS_BAD_COLS 2
#define VS_BAD_SCALE 3
#define VS_BAD_GAP 4
#define VS_TOO_LARGE 5

/* cols_in 0: ceil(sqrt(n_views)).  Cell (v / cols, v % cols) of 256 * scale pixels a side, gap pixels between cells and around the
 * sheet.  The extents are filled in for VS_TOO_LARGE too. */
RM_FN int vs_layout(int n_views, int cols_in, int scale, int gap, int* cols, int* rows, int* width, int* height) {
    if (n_views < 1 || n_views > 65536) return VS_BAD_VIEWS;
    if (cols_in < 0 || cols_in > 65536) return VS_BAD_COLS;
    if (scale < 1 || scale > VS_MAX_SCALE) return VS_BAD_SCALE;
    if (gap < 0 || gap > VS_MAX_GAP) return VS_BAD_GAP;
    int c = cols_in;
    if (c == 0)
        for (c = 1; c * c < n_views; ++c) {}
    const int r = (n_views + c - 1) / c;
    *cols = c;
    *rows = r;
    *width = c * RM_SIZE * scale + (c + 1) * gap;
    *height = r * RM_SIZE * scale + (r + 1) * gap;
    return (*width > VS_MAX_SIDE || *height > VS_MAX_SIDE) ? VS_TOO_LARGE : VS_OK;
}

/* One prediction in one view, in sheet pixels relative to its cell's origin (x right, y down; pixel (i, j) covers
 * [i, i + 1) x [j, j + 1)): the marker, the end of its residual, the colour, what to draw and the pixels it can touch. */
typedef struct __attribute__((aligned(16))) {
    double mx, my;               /* the marker: scale * X, scale * Y with X = b, Y = a + 1 */
    double ex, ey;               /* the residual's other end: scale * X', scale * Y' */
    uint32_t rgb, flags;         /* r | g << 8 | b << 16; VS_* */
    int16_t ix0, ix1, iy0, iy1;  /* conservative pixel box inside the cell; ix0 > ix1: nothing */
} vs_record;

RM_FN int vs_finite(double x) { return x - x == 0.0; }

/* half width of a residual in sheet pixels */
RM_FN double vs_half_width(int scale) { return scale > 1 ? 0.5 * (double)scale : 0.5; }

/* lo - 1 .. hi + 1, rounded outwards and cut to [0, side - 1]: 1 when pixels remain */
RM_FN int vs_span(double lo, double hi, double side, int16_t* i0, int16_t* i1) {
    double a = floor(lo) - 1.0, b = ceil(hi) + 1.0;
    if (b < 0.0 || a > side - 1.0) return 0;
    a = a < 0.0 ? 0.0 : a;
    b = b > side - 1.0 ? side - 1.0 : b;
    *i0 = (int16_t)a;
    *i1 = (int16_t)b;
    return 1;
}

/* (a, b, score): the predictor's maximum; m [9] row-major and p [3]: the view's rotation and the landmark, read when `residual` */
RM_FN vs_record vs_project(float a, float b, float score, const double* m, const double* p, int residual, uint32_t rgb, int used,
                           int scale, double radius) {
    vs_record r;
    r.mx = r.my = r.ex = r.ey = 0.0;
    r.rgb = rgb;
    r.flags = 0u;
    r.ix0 = r.iy0 = 1;
    r.ix1 = r.iy1 = 0;
    if (!(vs_finite((double)a) && vs_finite((double)b) && vs_finite((double)score))) return r;
    const double s = (double)scale, side = (double)RM_SIZE * s;
    const double X = (double)b, Y = (double)a + 1.0;
    r.mx = s * X;
    r.my = s * Y;
    const double rr = radius * s;
    double lox = r.mx - rr, hix = r.mx + rr, loy = r.my - rr, hiy = r.my + rr;
    uint32_t flags = VS_MARKER | (used ? 0u : VS_RING);
    if (residual && vs_finite(p[0]) && vs_finite(p[1]) && vs_finite(p[2])) {
        const double qx = (m[0] * p[0] + m[1] * p[1]) + m[2] * p[2];
        const double qy = (m[3] * p[0] + m[4] * p[1]) + m[5] * p[2];
        const double Xp = ((qx + 150.0) * 256.0) / 300.0;
        const double Yp = 256.0 - ((qy + 150.0) * 256.0) / 300.0;
        const double ex = s * Xp, ey = s * Yp;
        if (vs_finite(ex) && vs_finite(ey)) {
            const double hw = vs_half_width(scale);
            r.ex = ex;
            r.ey = ey;
            flags |= VS_SEGMENT;
            lox = ex - hw < lox ? ex - hw : lox;
            hix = ex + hw > hix ? ex + hw : hix;
            loy = ey - hw < loy ? ey - hw : loy;
            hiy = ey + hw > hiy ? ey + hw : hiy;
        }
    }
    if (vs_span(lox, hix, side, &r.ix0, &r.ix1) && vs_span(loy, hiy, side, &r.iy0, &r.iy1)) {
        r.flags = flags;
    } else {
        r.ix0 = 1;
        r.ix1 = 0;
    }
    return r;
}

/* the marker: pixel centre within radius * scale of it; a ring keeps only the outer max(1, scale) pixels of that disc */
RM_FN int vs_marker_covers(const vs_record* r, int i, int j, int scale, double radius) {
    const double dx = ((double)i + 0.5) - r->mx, dy = ((double)j + 0.5) - r->my;
    const double d2 = dx * dx + dy * dy;
    const double rr = radius * (double)scale;
    if (!(d2 <= rr * rr)) return 0;
    if (r->flags & VS_RING) {
        const double inner = rr - (double)(scale > 1 ? scale : 1);
        if (inner >= 0.0 && !(d2 > inner * inner)) return 0;
    }
    return 1;
}

/* the residual: pixel centre within vs_half_width of the segment marker -> end (a point when the two coincide) */
RM_FN int vs_segment_covers(const vs_record* r, int i, int j, int scale) {
    const double vx = r->ex - r->mx, vy = r->ey - r->my;
    const double wx = ((double)i + 0.5) - r->mx, wy = ((double)j + 0.5) - r->my;
    const double l2 = vx * vx + vy * vy;
    double t = 0.0;
    if (l2 > 0.0) {
        t = (wx * vx + wy * vy) / l2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double cx = wx - t * vx, cy = wy - t * vy;
    const double d2 = cx * cx + cy * cy;
    const double hw = vs_half_width(scale);
    return d2 <= hw * hw;
}

/* a plane's value k / 255 as its byte: float32, (int)(p * 255 + 0.5) cut to 0..255, NaN 0 */
RM_FN uint32_t vs_byte(float p) {
    float v = p * 255.0f + 0.5f;
    v = v >= 0.0f ? v : 0.0f;
    v = v > 255.0f ? 255.0f : v;
    return (uint32_t)(int)v;
}

#endif
