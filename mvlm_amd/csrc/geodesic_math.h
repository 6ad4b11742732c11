// Scalar arithmetic of the surface distances between landmarks (geodesic.hip: mvlm_landmark_geodesics), written once for the
// kernels and for host code.  Plain C99 subset, like raster_points_math.h.  The tests do NOT share this file with their checker:
// tests/geodesic_model.py states the rule a second time in numpy; tests/native/geodesic_host.cpp compiles THIS file for the host
// and must equal the model bit for bit, as the kernels must.
//
// The rule ("Surface distances").  Everything is float64; a vertex is the device mesh's float32 coordinates widened
// to double; every sum of three products is (a + b) + c; nothing is contracted (-ffp-contract=off); sqrt and / are IEEE.
//   * valid triangle: its three indices are in [0, V) and its nine coordinates are finite.  Every other triangle is ignored in
//     every step.  Landmark i is attached iff tri[i] names a valid triangle and its snapped point P_i is finite; a landmark that is
//     not attached has no field, and its row and column of D are NaN.
//   * frame of a corner C over the edge (A, B):  ab = B - A, ac = C - A, bc = C - B, c = sqrt(ab.ab), lac = sqrt(ac.ac),
//     lbc = sqrt(bc.bc), and where c > 0: px = ac.ab / c, py = sqrt(max(ac.ac - px px, 0)); where c == 0 the frame has no interior.
//   * update u(da, db, frame) = min of
//       da + lac,  db + lbc                                    always (an infinite value gives an infinite candidate: no effect)
//       (da + k px) + py w   with k = (db - da) / c, w = sqrt(1 - k k)
//                                                              iff da and db are finite, c > 0, py > 0, |k| < 1 and
//                                                              s = px - (k py) / w  satisfies  0 < s < c
//     (w == 0 makes s infinite: the candidate does not count).  No special case for obtuse triangles.
//   * a triangle (i0, i1, i2) gives its corner i0 the edge (A, B) = (i1, i2), i1 the edge (i2, i0) and i2 the edge (i0, i1); a
//     target in it takes the same three edges.  A triangle with a repeated index is kept: its updates are never below what they read.
//   * initial set of source i: S = corners of tri[i]; init_rings times, every valid triangle with a corner in S (as S stood at the
//     start of the round) puts its three corners in S.  d[v] = |V_v - P_i| (gd_dist) in S, +inf elsewhere.
//   * sweep (Jacobi): new[v] = min(old[v], u over the valid triangles with v as a corner, v's edge as above), every read of old.
//     min is exact and commutative, so neither scheduling nor the order of a vertex's triangle list reaches a value.  sweeps[i] is
//     the index of the first sweep that changed no value.
//   * target: D[i, j] = min over the three edges (a, b) of tri[j] of u(d_i[a], d_i[b], frame(V_a, V_b, P_j)), and |P_i - P_j| as
//     well when tri[i] == tri[j]; D[i, i] = 0.  E[i, j] = |P_i - P_j| (gd_dist).
#ifndef MVLM_GEODESIC_MATH_H
#define MVLM_GEODESIC_MATH_H

#include "raster_math.h"

#define GD_MAX_RINGS 8
#define GD_MAX_LANDMARKS 65536
#define GD_DEFAULT_SWEEPS 4096
#define GD_MAX_SWEEPS 1048576
#define GD_DEFAULT_SCRATCH (512ll << 20)

typedef struct {
    double x, y, z;
} gd_vec3;

typedef struct {
    double lac, lbc, c, px, py;
} gd_frame;

RM_FN gd_vec3 gd_v3(double x, double y, double z) {
    gd_vec3 o;
    o.x = x, o.y = y, o.z = z;
    return o;
}
RM_FN gd_vec3 gd_sub(gd_vec3 a, gd_vec3 b) { return gd_v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RM_FN double gd_dot(gd_vec3 a, gd_vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RM_FN int gd_finite(double x) { return x - x == 0.0; }
RM_FN int gd_finite3(gd_vec3 a) { return gd_finite(a.x) && gd_finite(a.y) && gd_finite(a.z); }
RM_FN double gd_min(double a, double b) { return b < a ? b : a; } /* (no NaN reaches it) */
RM_FN double gd_inf(void) { return (double)INFINITY; }

RM_FN double gd_dist(gd_vec3 a, gd_vec3 b) {
    const gd_vec3 d = gd_sub(a, b);
    return sqrt(gd_dot(d, d));
}

RM_FN gd_frame gd_make_frame(gd_vec3 A, gd_vec3 B, gd_vec3 C) {
    const gd_vec3 ab = gd_sub(B, A), ac = gd_sub(C, A), bc = gd_sub(C, B);
    const double ac2 = gd_dot(ac, ac);
    gd_frame f;
    f.c = sqrt(gd_dot(ab, ab));
    f.lac = sqrt(ac2);
    f.lbc = sqrt(gd_dot(bc, bc));
    f.px = 0.0, f.py = 0.0;
    if (f.c > 0.0) {
        f.px = gd_dot(ac, ab) / f.c;
        const double h2 = ac2 - f.px * f.px;
        f.py = sqrt(h2 > 0.0 ? h2 : 0.0);
    }
    return f;
}

RM_FN double gd_update(double da, double db, gd_frame f) {
    double best = gd_min(da + f.lac, db + f.lbc);
    if (gd_finite(da) && gd_finite(db) && f.c > 0.0 && f.py > 0.0) {
        const double k = (db - da) / f.c;
        if (fabs(k) < 1.0) {
            const double w = sqrt(1.0 - k * k);
            const double s = f.px - (k * f.py) / w;
            if (s > 0.0 && s < f.c) best = gd_min(best, (da + k * f.px) + f.py * w);
        }
    }
    return best;
}

#endif
