// Scalar arithmetic of the point-cloud (splat) renderer, written once for the kernels of raster_points.hip and the host
// code around them so they agree bit for bit.  Plain C99 subset, like raster_math.h, whose transform, key and depth byte it
// reuses unchanged.  The tests do NOT share this file: their checker, tests/points_model.py, is an independent restatement.
//
// The contract ("Point clouds").  The reference has nothing to restate here: vtkOBJReader yields no cells for
// a file without faces, its views stay white and its cell locator finds nothing - so this is a build-defined capability,
// like the geometry plane, and what pins it is this statement and its CPU twin.
//   * position and depth of a point: rm_transform, unchanged (M v in double, window (x + 150) 256 / 300, the snap to
//     2^-bits pixel on the 1/256 lattice, z = (500 - zv) / 1500); a point with a non-finite coordinate draws nothing,
//   * radius: r model units per mesh, R = floor(r * 256 / 300 * 256 + 0.5) lattice steps, admitted from 0.75 px (above
//     sqrt(2) / 2: every splat inside the window owns at least one pixel centre) to 8 px (a thread's box is at most 17 x 17
//     centres), i.e. R in [192, 2048],
//   * coverage: pixel (i, j), centre (256 i + 128, 256 j + 128), is covered iff dx * dx + dy * dy <= R * R in 64-bit
//     integers; the candidate box is rm_setup's - the centres inside [X - R, X + R], clipped to the window,
//   * depth of a covered pixel: a paraboloid, z_pix = z + (float)d2 * c as two separately rounded float32 operations (d2 is at
//     most 2^22: exact in float32), c = (float)((double)r / 1500.0 / ((double)R * R)) formed once on the host - the rim of a
//     splat lies r model units behind its centre, so neighbouring splats of similar depth split the screen between them
//     like a Voronoi diagram instead of the nearer disc swallowing the others; near / far clip on z_pix as the mesh path
//     clips its interpolated depth,
//   * key: rm_key(z_pix, point id) - smaller depth wins, at equal depth the higher id (LEQUAL in draw order),
//   * output: depth byte rm_depth_u8(z_pix) of the winner, RGB the winner's colour bytes (white without colours;
//     rm_color_u8(c / 255) == c, so no conversion is involved), white background, flipped and / 255 as tile_kernel writes.
#ifndef MVLM_RASTER_POINTS_MATH_H
#define MVLM_RASTER_POINTS_MATH_H

#include "raster_math.h"

#define RP_R_MIN 192  /* 0.75 px */
#define RP_R_MAX 2048 /* 8 px */
#define RP_PX_MIN 0.75
#define RP_PX_MAX 8.0

/* radius in model units -> lattice steps; returns 1 when the radius is admitted (finite, R in [RP_R_MIN, RP_R_MAX]) */
RM_FN int rp_radius_steps(double r, int32_t* R) {
    *R = 0;
    if (!(r > 0.0 && r < 1e6)) return 0; /* (NaN too) */
    const double s = floor(r * 256.0 / 300.0 * 256.0 + 0.5);
    *R = (int32_t)s;
    return *R >= RP_R_MIN && *R <= RP_R_MAX;
}

/* depth added per squared lattice step of distance from the splat's centre: r / 1500 at the rim */
RM_FN float rp_depth_coeff(double r, int32_t R) { return (float)(r / 1500.0 / ((double)R * (double)R)); }

RM_FN int rp_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

typedef struct {
    int32_t ix0, ix1, iy0, iy1; /* candidate pixel centres, clipped to the window; empty if ix0 > ix1 or iy0 > iy1 */
} rp_box;

RM_FN rp_box rp_setup(int32_t X, int32_t Y, int32_t R) {
    rp_box b;
    b.ix0 = -rm_floor_div(-(X - R - RM_HALF), RM_SUB);
    b.ix1 = rm_floor_div(X + R - RM_HALF, RM_SUB);
    b.iy0 = -rm_floor_div(-(Y - R - RM_HALF), RM_SUB);
    b.iy1 = rm_floor_div(Y + R - RM_HALF, RM_SUB);
    if (b.ix0 < 0) b.ix0 = 0;
    if (b.iy0 < 0) b.iy0 = 0;
    if (b.ix1 > RM_SIZE - 1) b.ix1 = RM_SIZE - 1;
    if (b.iy1 > RM_SIZE - 1) b.iy1 = RM_SIZE - 1;
    return b;
}

/* coverage of pixel (i, j) by the disc of R steps round (X, Y); *d2 = squared distance of its centre, in steps */
RM_FN int rp_cover(int32_t X, int32_t Y, int32_t R, int i, int j, int64_t* d2) {
    const int64_t dx = (int64_t)(i * RM_SUB + RM_HALF) - X, dy = (int64_t)(j * RM_SUB + RM_HALF) - Y;
    *d2 = dx * dx + dy * dy;
    return *d2 <= (int64_t)R * R;
}

/* the paraboloid: two float32 operations, each rounded (the build has -ffp-contract=off) */
RM_FN float rp_depth(float z, int64_t d2, float c) {
    const float lift = (float)d2 * c;
    return z + lift;
}

RM_FN int rp_clip(float z_pix) { return z_pix >= 0.0f && z_pix <= 1.0f; }

#endif
