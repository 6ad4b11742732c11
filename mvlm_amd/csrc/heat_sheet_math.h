// Scalar arithmetic of the heat sheet (heat_sheet.hip): which heatmap values count, how a landmark's value becomes an opacity and how
// a colour is laid over the background byte.  Host and device share it; everything that decides a pixel is float64 in the operation
// order written here (the Makefile's -ffp-contract=off keeps multiply and add apart), so numpy reproduces it.  The tests do NOT
// share this file: tests/heat_model.py is an independent restatement ("Heat sheet").
#ifndef MVLM_HEAT_SHEET_MATH_H
#define MVLM_HEAT_SHEET_MATH_H

#include "raster_math.h"

#define HS_MAX_PLANES 32768     /* n_views * n_lm per call: 8 GiB of heatmaps */
#define HS_MAX_LANDMARKS 65536  /* as the view sheet's */
#define HS_RED 0x0000FFu        /* landmarks without a colour of their own: r | g << 8 | b << 16 */

/* neither NaN nor +-inf: what the peak counts and what the composition draws */
RM_FN int hs_finite(float v) { return v == v && fabsf(v) < INFINITY; }

/* a plane's peak m makes the plane a candidate: finite and above zero */
RM_FN int hs_peak_counts(float m) { return hs_finite(m) && m > 0.0f; }

/* the value h of a plane with peak m, as a share of that peak */
RM_FN double hs_share(float h, float m) { return (double)h / (double)m; }

/* the opacity of a share t above the floor: opacity at t == 1, towards 0 at the floor */
RM_FN double hs_alpha(double t, double floor_, double opacity) { return opacity * (t - floor_) / (1.0 - floor_); }

/* colour byte col laid over background byte bg with opacity a */
RM_FN uint32_t hs_blend(uint32_t bg, uint32_t col, double a) {
    const double b = (double)bg;
    return (uint32_t)(int)(b + a * ((double)col - b) + 0.5);
}

/* the three channels of r | g << 8 | b << 16 */
RM_FN uint32_t hs_blend_rgb(uint32_t bg, uint32_t col, double a) {
    return hs_blend(bg & 0xFFu, col & 0xFFu, a) | (hs_blend((bg >> 8) & 0xFFu, (col >> 8) & 0xFFu, a) << 8) |
           (hs_blend((bg >> 16) & 0xFFu, (col >> 16) & 0xFFu, a) << 16);
}

#endif
