// Scalar arithmetic of the surface heat (surface_backproject.hip): where a vertex lies in a rendered view, whether the view sees
// it, what a view's heatmap value there adds to the vertex's score, and the key that picks a landmark's best vertex.  Host and
// device share it; everything that decides a number is float64 or integer in the operation order written here (the Makefile's
// -ffp-contract=off keeps multiply and add apart), so numpy reproduces it.  The tests do NOT share this file:
// tests/backproject_model.py is an independent restatement ("Surface heat").
//
// The contract, for vertex v, view n, landmark l:
//   position    o = rm_transform(rot[n], v, sub_bits): the position the render used.  Pixel i = floor(o.X / 256), j = floor(o.Y / 256);
//               inside iff v is finite, 0 <= i, j < 256 and o.z in [0, 1].  The heat / image pixel is [row 255 - j, col i].
//   visibility  T_v = trunc(255 o.z); the pixel's depth byte B = trunc(images[n,row,col,3] * 255 + 0.5) gives T_pix = (256 - B) & 255,
//               the inverse of rm_depth_u8 (the background's byte 1 gives 255).  Visible iff inside and T_v <= T_pix + depth_tol.
//   term        m = the peak of plane (n, l) (mvlm_heat_plane_peaks), h = heat[n,l,row,col]: t = max(h / m, 0) where the plane
//               counts (hs_peak_counts) and h is finite, else 0.
//   score       n_vis = the views that see v; sum = ((0 + t_0) + t_1) + ... over the views that see v, in ascending n;
//               score[v,l] = (float)(sum / n_vis), 0 when n_vis == 0.
//   colour      the selected landmark of the largest score wins, the lowest index on a tie; score <= floor leaves the base colour
//               (the vertex's own, else its texel, else SB_BASE_GREY), else hs_blend_rgb(base, colour, hs_alpha(score, floor, opacity)).
//   peak        per landmark the vertex of the largest score > 0, the lowest id on a tie: the maximum of sb_key over the vertices.
#ifndef MVLM_SURFACE_BACKPROJECT_MATH_H
#define MVLM_SURFACE_BACKPROJECT_MATH_H

#include "heat_sheet_math.h"

#define SB_MAX_SCORES (1ll << 28) /* n_verts * n_lm per call: the score table, scratch when the caller keeps none (1 GiB) */
#define SB_MAX_DEPTH_TOL 255
#define SB_BASE_GREY 0xC8C8C8u /* a vertex without a colour or a texel of its own: (200, 200, 200) as r | g << 8 | b << 16 */

/* the view pixel (i, j), j counting up from the bottom row, of a transformed finite vertex; 0: outside the window or the clip range */
RM_FN int sb_pixel(rm_vert o, int* i, int* j) {
    *i = rm_floor_div(o.X, RM_SUB);
    *j = rm_floor_div(o.Y, RM_SUB);
    return *i >= 0 && *i < RM_SIZE && *j >= 0 && *j < RM_SIZE && o.z >= 0.0f && o.z <= 1.0f;
}

/* depth steps (1/255 of the clip range) of a z-buffer value in [0, 1]: what rm_depth_u8 truncates to */
RM_FN int sb_vertex_step(float z) { return (int)(255.0 * (double)z); }

/* depth steps of the rendered surface from the depth plane's value d = byte / 255: the inverse of rm_depth_u8 */
RM_FN int sb_pixel_step(float d) {
    const int b = (int)(d * 255.0f + 0.5f);
    return (256 - b) & 255;
}

RM_FN int sb_visible(int t_v, int t_pix, int depth_tol) { return t_v <= t_pix + depth_tol; }

/* what a view that sees the vertex adds: the heat value h there as a share of the plane's peak m, never below 0 */
RM_FN double sb_term(float h, float m) {
    if (!hs_peak_counts(m) || !hs_finite(h)) return 0.0;
    const double t = hs_share(h, m);
    return t > 0.0 ? t : 0.0;
}

RM_FN float sb_score(double sum, int n_vis) { return n_vis > 0 ? (float)(sum / (double)n_vis) : 0.0f; }

/* scores are floats >= 0: their bit pattern is monotone, and the larger key is the larger score, then the lower vertex */
RM_FN uint64_t sb_key(float score, uint32_t v) {
    union { float f; uint32_t u; } c;
    c.f = score;
    return ((uint64_t)c.u << 32) | (uint64_t)(0xFFFFFFFFu - v);
}
#define SB_KEY_NONE 0ull /* below every key of a score > 0 */
RM_FN int32_t sb_key_vertex(uint64_t k) { return k == SB_KEY_NONE ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFu)); }
RM_FN float sb_key_score(uint64_t k) {
    union { float f; uint32_t u; } c;
    c.u = (uint32_t)(k >> 32);
    return c.f;
}

#endif
