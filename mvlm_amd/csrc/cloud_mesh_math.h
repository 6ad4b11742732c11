// Scalar arithmetic of a point cloud's triangulation (cloud_mesh.hip: mvlm_mesh_triangulate_points), written once for the kernels
// and the host code around them.  Plain C99 subset, like raster_points_math.h.  The tests do NOT share this file: their checker,
// tests/cloud_mesh_model.py, is an independent restatement with a brute-force star.
//
// The contract ("Point clouds").  Inputs: the cloud's float32 points v, its float32 normals n (the device copy's: a
// file's or the estimate's) and the neighbour table N, i32[V,16], as mvlm_mesh_estimate_normals leaves it (ascending (d2, id), -1
// for unused slots, a non-finite point's row all -1).  All arithmetic is float64 from those values, every sum of three products is
// (a + b) + c, nothing is contracted (-ffp-contract=off) and no value depends on scheduling.
//   * perturbed points: for point p, d2 = (dx dx + dy dy) + dz dz to every row entry, s = sqrt(least positive d2) * 0.00390625 (0
//     without a positive one); x = ((p + 1) * 0x9E3779B1) mod 2^32, then for c = 0, 1, 2 in turn, continuing from the same x:
//     x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16 (mod 2^32), h_c = (double)(x >> 8) / 8388608.0 - 1.0,
//     u_p[c] = v_p[c] + h_c * s.  The shift - 1/256 of the nearest-neighbour distance - depends on p alone: every star sees the same
//     points, and the exact co-circular ties of a regular scan grid break the same way everywhere.  Only the connectivity is
//     decided on u; the output indexes the original points.
//   * star of p: empty when L2 = (nx nx + ny ny) + nz nz is not finite or not above 0, or the row has fewer than two entries other
//     than p.  Else n^ = n / sqrt(L2); c the component of least |n^_c|, the lowest index on a tie; e1 = cross(n^, axis_c) divided by
//     its length; e2 = cross(n^, e1); cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx).  For each row entry m != p, in row
//     order: d = u_m - u_p, q = ((dx e1x + dy e1y) + dz e1z, the same with e2), r2 = qx qx + qy qy, an entry with r2 == 0 is left
//     out, w = (qx / r2, qy / r2) - the inversion that turns "empty circle through p" into "hull edge".  The unordered pair {a, b} is
//     in the star S(p) iff for one of its two orders  wx_a wy_b - wy_a wx_b > 0  and, for every other kept entry c,
//     (wx_b - wx_a)(wy_c - wy_a) - (wy_b - wy_a)(wx_c - wx_a) > 0.  Swapping b and c negates the second predicate exactly, so an
//     entry a starts at most one pair: the star has at most 16.  Flipping n negates every predicate exactly: the sign the
//     estimate leaves open does not matter.
//   * triangles: {i < j < k} is emitted iff {j,k} in S(i), {i,k} in S(j), {i,j} in S(k), and it is no sliver: with A2 the squared
//     length of cross(v_j - v_i, v_k - v_i) and L2m the largest squared edge (v_j - v_i, v_k - v_i, v_k - v_j), both from the
//     unperturbed points, A2 * 1024.0 > L2m * L2m - a height above 1/32 of the longest edge.  Rows (i, j, k) in ascending
//     lexicographic order; the winding is unspecified (rasteriser and geometry shade are two-sided).
#ifndef MVLM_CLOUD_MESH_MATH_H
#define MVLM_CLOUD_MESH_MATH_H

#include "raster_math.h"

#define CM_K 16      /* columns of the neighbour table (CN_K of cloud_normals_math.h) */
#define CM_STAR 16   /* pairs a star can hold */

typedef struct {
    double x, y, z;
} cm_vec3;

typedef struct {
    double x, y;
} cm_vec2;

RM_FN cm_vec3 cm_v3(double x, double y, double z) {
    cm_vec3 o;
    o.x = x, o.y = y, o.z = z;
    return o;
}

RM_FN cm_vec3 cm_sub(cm_vec3 a, cm_vec3 b) { return cm_v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RM_FN double cm_dot(cm_vec3 a, cm_vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RM_FN cm_vec3 cm_cross(cm_vec3 a, cm_vec3 b) { return cm_v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

/* one round of the hash: the state after it */
RM_FN uint32_t cm_hash_next(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
RM_FN uint32_t cm_hash_seed(int32_t p) { return ((uint32_t)p + 1u) * 0x9E3779B1u; }
/* a state's number in [-1, 1) */
RM_FN double cm_hash_unit(uint32_t x) { return (double)(x >> 8) / 8388608.0 - 1.0; }

/* the perturbation's length from the least positive squared distance of the row (0: none was positive) */
RM_FN double cm_shift(double least_d2) { return least_d2 > 0.0 ? sqrt(least_d2) * 0.00390625 : 0.0; }

/* the perturbed point: v + h s per component, the three rounds of the hash in turn */
RM_FN cm_vec3 cm_perturb(int32_t p, cm_vec3 v, double s) {
    uint32_t x = cm_hash_seed(p);
    cm_vec3 u;
    x = cm_hash_next(x);
    u.x = v.x + cm_hash_unit(x) * s;
    x = cm_hash_next(x);
    u.y = v.y + cm_hash_unit(x) * s;
    x = cm_hash_next(x);
    u.z = v.z + cm_hash_unit(x) * s;
    return u;
}

/* the tangent frame of a normal; ok = 0: the star is empty (L2 not finite or not above 0) */
typedef struct {
    cm_vec3 e1, e2;
    int ok;
} cm_frame;

RM_FN cm_frame cm_tangent_frame(cm_vec3 n) {
    cm_frame f;
    f.e1 = f.e2 = cm_v3(0.0, 0.0, 0.0);
    f.ok = 0;
    const double L2 = cm_dot(n, n);
    if (!isfinite(L2) || !(L2 > 0.0)) return f;
    const double len = sqrt(L2);
    const cm_vec3 nh = cm_v3(n.x / len, n.y / len, n.z / len);
    int c = 0;
    double least = fabs(nh.x);
    if (fabs(nh.y) < least) c = 1, least = fabs(nh.y);
    if (fabs(nh.z) < least) c = 2;
    const cm_vec3 t = cm_cross(nh, cm_v3(c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0));
    const double tl = sqrt(cm_dot(t, t));
    f.e1 = cm_v3(t.x / tl, t.y / tl, t.z / tl);
    f.e2 = cm_cross(nh, f.e1);
    f.ok = 1;
    return f;
}

/* a neighbour in the inverted tangent plane; kept = 0: r2 == 0, the entry is left out */
typedef struct {
    cm_vec2 w;
    int kept;
} cm_inverted;

RM_FN cm_inverted cm_invert(cm_vec3 e1, cm_vec3 e2, cm_vec3 d) {
    cm_inverted o;
    const double qx = cm_dot(d, e1), qy = cm_dot(d, e2);
    const double r2 = qx * qx + qy * qy;
    o.kept = !(r2 == 0.0);
    o.w.x = qx / r2;
    o.w.y = qy / r2;
    return o;
}

/* the first predicate of a pair in the order (a, b): the origin - p itself - lies to the left of a -> b */
RM_FN int cm_turns_left(cm_vec2 a, cm_vec2 b) { return a.x * b.y - a.y * b.x > 0.0; }
/* the second, for one other entry c */
RM_FN int cm_left_of(cm_vec2 a, cm_vec2 b, cm_vec2 c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x) > 0.0; }

/* no sliver: the unperturbed triangle's height is above 1/32 of its longest edge */
RM_FN int cm_not_sliver(cm_vec3 vi, cm_vec3 vj, cm_vec3 vk) {
    const cm_vec3 a = cm_sub(vj, vi), b = cm_sub(vk, vi), c = cm_sub(vk, vj);
    const cm_vec3 x = cm_cross(a, b);
    const double A2 = cm_dot(x, x);
    double L2m = cm_dot(a, a);
    const double lb = cm_dot(b, b), lc = cm_dot(c, c);
    if (lb > L2m) L2m = lb;
    if (lc > L2m) L2m = lc;
    return A2 * 1024.0 > L2m * L2m;
}

#endif
