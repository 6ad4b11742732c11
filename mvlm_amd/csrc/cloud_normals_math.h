// Scalar arithmetic of a point cloud's normals - the estimate (cloud_normals.hip: neighbour search, covariance, eigenvector) and
// the geometry shade of a splat - written once for the kernels and the host code around them.  Plain C99 subset, like
// raster_points_math.h.  The tests do NOT share this file: their checker, tests/cloud_normals_model.py, is an independent
// restatement (brute-force search, numpy.linalg.eigh).
//
// The contract ("Point clouds"):
//   * neighbourhood of a finite point p: the K = 16 finite points with the smallest (d2, id) in lexicographic order, p itself
//     included (d2 = 0), d2 = (dx * dx + dy * dy) + dz * dz in float64 from the float32 coordinates widened - the snap's formula;
//     fewer than 16 finite points: all of them.  A row of the table lists them in ascending (d2, id), unused slots -1; a
//     non-finite point is nobody's neighbour and its own row is all -1,
//   * normal: centroid and 3 x 3 covariance of the neighbourhood in float64, summed in the row's order; the unit eigenvector of
//     the smallest eigenvalue by cyclic Jacobi (CN_SWEEPS sweeps over (0,1), (0,2), (1,2); no closed trigonometric form), the
//     lowest index among equal eigenvalues, normalised in float64, stored as float32; its sign is unspecified,
//   * the normal is (0, 0, 0) for a non-finite point, a neighbourhood of fewer than 3 points and a zero covariance,
//   * shade of a splat: for the winner's float32 normal n and the view's rotation M (row-major float64, as rm_transform reads it),
//     nz = (M[6] n.x + M[7] n.y) + M[8] n.z, len = sqrt((n.x n.x + n.y n.y) + n.z n.z), shade = (int)(|nz| / len * 255 + 0.5), each
//     operation rounded separately in float64; 0 when len is zero or not finite (rm_geometry_u8 gives a degenerate triangle 0 too).
#ifndef MVLM_CLOUD_NORMALS_MATH_H
#define MVLM_CLOUD_NORMALS_MATH_H

#include "raster_math.h"

#define CN_K 16     /* neighbours of a point, itself included */
#define CN_SWEEPS 8 /* Jacobi sweeps: a 3 x 3 symmetric matrix is diagonal to the last bit after four or five */

RM_FN double cn_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

/* does (d2a, ia) come before (d2b, ib)? */
RM_FN int cn_before(double d2a, int32_t ia, double d2b, int32_t ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

/* One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix (r the third index): annihilates a_pq, rotates the two
 * columns p, q of the eigenvector matrix.  t is the smaller root of t^2 + 2 t theta - 1 = 0: no trigonometric function, no
 * cancellation.  By value in and out (no address of a caller's local is taken: a kernel keeps them all in registers). */
typedef struct {
    double app, aqq, apr, aqr, v0p, v0q, v1p, v1q, v2p, v2q;
} cn_rot;

RM_FN cn_rot cn_rotate(double apq, cn_rot in) {
    if (apq == 0.0) return in;
    const double theta = (in.aqq - in.app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)); /* (|theta| = inf: t = 0) */
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    cn_rot o;
    o.app = in.app - t * apq;
    o.aqq = in.aqq + t * apq;
    o.apr = c * in.apr - s * in.aqr;
    o.aqr = s * in.apr + c * in.aqr;
    o.v0p = c * in.v0p - s * in.v0q;
    o.v0q = s * in.v0p + c * in.v0q;
    o.v1p = c * in.v1p - s * in.v1q;
    o.v1q = s * in.v1p + c * in.v1q;
    o.v2p = c * in.v2p - s * in.v2q;
    o.v2q = s * in.v2p + c * in.v2q;
    return o;
}

/* The normal of a neighbourhood of n points with covariance (sums, not divided by n: the eigenvectors are the same)
 * [[cxx, cxy, cxz], [cxy, cyy, cyz], [cxz, cyz, czz]] -> out[3]; (0, 0, 0) for n < 3, a zero or a non-finite matrix. */
RM_FN void cn_normal(int n, double cxx, double cxy, double cxz, double cyy, double cyz, double czz, float* out) {
    out[0] = out[1] = out[2] = 0.0f;
    if (n < 3) return;
    if (cxx == 0.0 && cxy == 0.0 && cxz == 0.0 && cyy == 0.0 && cyz == 0.0 && czz == 0.0) return;
    double a00 = cxx, a01 = cxy, a02 = cxz, a11 = cyy, a12 = cyz, a22 = czz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < CN_SWEEPS; ++sweep) {
        cn_rot r, i;
        i.app = a00, i.aqq = a11, i.apr = a02, i.aqr = a12, i.v0p = v00, i.v0q = v01, i.v1p = v10, i.v1q = v11, i.v2p = v20, i.v2q = v21;
        r = cn_rotate(a01, i); /* (0, 1) */
        a01 = 0.0;
        a00 = r.app, a11 = r.aqq, a02 = r.apr, a12 = r.aqr, v00 = r.v0p, v01 = r.v0q, v10 = r.v1p, v11 = r.v1q, v20 = r.v2p, v21 = r.v2q;
        i.app = a00, i.aqq = a22, i.apr = a01, i.aqr = a12, i.v0p = v00, i.v0q = v02, i.v1p = v10, i.v1q = v12, i.v2p = v20, i.v2q = v22;
        r = cn_rotate(a02, i); /* (0, 2) */
        a02 = 0.0;
        a00 = r.app, a22 = r.aqq, a01 = r.apr, a12 = r.aqr, v00 = r.v0p, v02 = r.v0q, v10 = r.v1p, v12 = r.v1q, v20 = r.v2p, v22 = r.v2q;
        i.app = a11, i.aqq = a22, i.apr = a01, i.aqr = a02, i.v0p = v01, i.v0q = v02, i.v1p = v11, i.v1q = v12, i.v2p = v21, i.v2q = v22;
        r = cn_rotate(a12, i); /* (1, 2) */
        a12 = 0.0;
        a11 = r.app, a22 = r.aqq, a01 = r.apr, a02 = r.aqr, v01 = r.v0p, v02 = r.v0q, v11 = r.v1p, v12 = r.v1q, v21 = r.v2p, v22 = r.v2q;
    }
    double nx = v00, ny = v10, nz = v20, least = a00;
    if (a11 < least) {
        nx = v01, ny = v11, nz = v21, least = a11;
    }
    if (a22 < least) {
        nx = v02, ny = v12, nz = v22, least = a22;
    }
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0) || !isfinite(len)) return;
    out[0] = (float)(nx / len);
    out[1] = (float)(ny / len);
    out[2] = (float)(nz / len);
}

/* the geometry plane's byte for a splat whose point has the normal (nx, ny, nz): two-sided, so the sign does not matter */
RM_FN int cn_shade_u8(const double* m /*[9] row-major*/, float nx, float ny, float nz) {
    const double x = nx, y = ny, z = nz;
    const double vz = (m[6] * x + m[7] * y) + m[8] * z;
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0) || !isfinite(len)) return 0;
    return (int)(fabs(vz) / len * 255.0 + 0.5);
}

#endif
