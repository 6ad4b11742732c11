// Scalar arithmetic of the landmark view (raster_view.hip): raster_math.h's one-sample contract with the window generalised
// - side S, a frame (cx, cy, half) per view - and the analytic landmark spheres.  Plain C99 subset, like raster_math.h, which
// it includes for everything that does not depend on the window (edge functions and tie rule, attribute planes, the depth
// key, colour and texel conversions) and does not change.  The tests do NOT share this file: their checker,
// tests/native/landmark_view.c, is an independent restatement ("Landmark view").
#ifndef MVLM_RASTER_VIEW_MATH_H
#define MVLM_RASTER_VIEW_MATH_H

#include "raster_math.h"

#define RV_MIN_SIZE 64
#define RV_MAX_SIZE 2048
#define RV_MAX_PIXELS (8ll * RV_MAX_SIZE * RV_MAX_SIZE) /* n_views * S * S of one call */
#define RV_MAX_VIEWS 128 /* of one call, whatever the size: the scratch grows with n_views * (vertices + triangles) */

/* pixels per model unit: the window shows [c - half, c + half] on S pixels.  S = 256, half = 150: 256.0f / 300.0f, rm_transform's k */
RM_FN float rv_scale(int size, float half) { return (float)size / (2.0f * half); }

/* rm_transform with the window's frame: with cx = cy = 0, half = 150, k = rv_scale(256, 150) every intermediate value is
 * rm_transform's (xv - 0 = xv bit for bit) */
RM_FN rm_vert rv_transform(const double* m /*[9] row-major*/, float vx, float vy, float vz, int sub_bits, float cx, float cy,
                           float half, float k) {
    const double x = vx, y = vy, z = vz;
    const float xv = (float)((m[0] * x + m[1] * y) + m[2] * z);
    const float yv = (float)((m[3] * x + m[4] * y) + m[5] * z);
    const float zv = (float)((m[6] * x + m[7] * y) + m[8] * z);
    const float sub = (float)(1 << sub_bits);
    float fx = floorf((((xv - cx) + half) * k) * sub + 0.5f);
    float fy = floorf((((yv - cy) + half) * k) * sub + 0.5f);
    const float lim = (float)(RM_COORD_LIM >> (8 - sub_bits));
    fx = fx < -lim ? -lim : (fx > lim ? lim : fx);
    fy = fy < -lim ? -lim : (fy > lim ? lim : fy);
    rm_vert o;
    o.X = (int32_t)fx * (RM_SUB >> sub_bits);
    o.Y = (int32_t)fy * (RM_SUB >> sub_bits);
    o.z = (500.0f - zv) / 1500.0f;
    o.pad = 0.0f;
    return o;
}

/* rm_setup with the pixel-centre box clipped to a window of `size` pixels */
RM_FN rm_tri rv_setup(rm_vert a, rm_vert b, rm_vert c, int size) {
    rm_tri t;
    int64_t area = (int64_t)(b.X - a.X) * (c.Y - a.Y) - (int64_t)(b.Y - a.Y) * (c.X - a.X);
    t.swapped = 0;
    if (area < 0) {
        rm_vert s = b;
        b = c;
        c = s;
        area = -area;
        t.swapped = 1;
    }
    t.X0 = a.X; t.Y0 = a.Y; t.X1 = b.X; t.Y1 = b.Y; t.X2 = c.X; t.Y2 = c.Y;
    t.z0 = a.z; t.z1 = b.z; t.z2 = c.z;
    t.farea = (float)area;
    int32_t minx = a.X < b.X ? a.X : b.X; minx = minx < c.X ? minx : c.X;
    int32_t maxx = a.X > b.X ? a.X : b.X; maxx = maxx > c.X ? maxx : c.X;
    int32_t miny = a.Y < b.Y ? a.Y : b.Y; miny = miny < c.Y ? miny : c.Y;
    int32_t maxy = a.Y > b.Y ? a.Y : b.Y; maxy = maxy > c.Y ? maxy : c.Y;
    t.ix0 = -rm_floor_div(-(minx - RM_HALF), RM_SUB);
    t.ix1 = rm_floor_div(maxx - RM_HALF, RM_SUB);
    t.iy0 = -rm_floor_div(-(miny - RM_HALF), RM_SUB);
    t.iy1 = rm_floor_div(maxy - RM_HALF, RM_SUB);
    if (t.ix0 < 0) t.ix0 = 0;
    if (t.iy0 < 0) t.iy0 = 0;
    if (t.ix1 > size - 1) t.ix1 = size - 1;
    if (t.iy1 > size - 1) t.iy1 = size - 1;
    t.valid = area != 0 && t.ix0 <= t.ix1 && t.iy0 <= t.iy1;
    return t;
}

/* rm_geometry_u8 with the z-buffer unit converted at the window's scale: 1 unit = 1500 model units = 1500 k pixels = 1500 k 256
 * steps.  Formed as (384000 S) / (2 half) so that S = 256, half = 150 gives rm_geometry_u8's -327680 exactly (384000 * 256 is a
 * float, the quotient is 327680); through the rounded k it would not. */
RM_FN float rv_geometry_kz(int size, float half) { return -((384000.0f * (float)size) / (2.0f * half)); }
RM_FN int rv_geometry_u8(const rm_tri* t, float kz) {
    const float ax = (float)(t->X1 - t->X0), ay = (float)(t->Y1 - t->Y0), az = (t->z1 - t->z0) * kz;
    const float bx = (float)(t->X2 - t->X0), by = (float)(t->Y2 - t->Y0), bz = (t->z2 - t->z0) * kz;
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0f)) return 0;
    const float s = fabsf(nz) / len;
    return (int)(s * 255.0f + 0.5f);
}

/* ---- landmark spheres: analytic under the orthographic camera ------------------------------------------------------------ */
/* a projected landmark, 32 bytes: window position (pixels, y up, NOT snapped), z-buffer value of its centre, radius in pixels,
 * colour r | g << 8 | b << 16, and a pixel box that holds every pixel the sphere can cover (empty: ix0 > ix1) */
typedef struct __attribute__((aligned(16))) {
    float X, Y, z, R;
    uint32_t rgb;
    int16_t ix0, ix1, iy0, iy1;
    uint32_t pad;
} rv_sphere;

/* one axis of the box: pixel centres i + 0.5 with |i + 0.5 - c| < R lie in [floor(c - R) - 1, floor(c + R) + 1] whatever the
 * roundings; clamped as floats (a far landmark, an infinite R) before the conversion */
RM_FN void rv_sphere_span(float c, float R, int size, int16_t* lo, int16_t* hi) {
    const float a = floorf(c - R) - 1.0f, b = floorf(c + R) + 1.0f;
    const float fa = fminf(fmaxf(a, 0.0f), (float)size), fb = fmaxf(fminf(b, (float)(size - 1)), -1.0f);
    *lo = (int16_t)(int)fa;
    *hi = (int16_t)(int)fb;
}

RM_FN rv_sphere rv_project_landmark(const double* m, const double* p, float cx, float cy, float half, float k, float radius,
                                    uint32_t rgb, int size) {
    const float xv = (float)((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]);
    const float yv = (float)((m[3] * p[0] + m[4] * p[1]) + m[5] * p[2]);
    const float zv = (float)((m[6] * p[0] + m[7] * p[1]) + m[8] * p[2]);
    rv_sphere s;
    s.X = ((xv - cx) + half) * k;
    s.Y = ((yv - cy) + half) * k;
    s.z = (500.0f - zv) / 1500.0f;
    s.R = radius * k;
    s.rgb = rgb;
    rv_sphere_span(s.X, s.R, size, &s.ix0, &s.ix1);
    rv_sphere_span(s.Y, s.R, size, &s.iy0, &s.iy1);
    s.pad = 0;
    return s;
}

/* the sphere's fragment at pixel (i, j) (j counts up from the bottom row): 0 when the pixel centre is outside the disc or the
 * surface point outside the clip range; otherwise its depth and the head-light shade hgt / R */
RM_FN int rv_sphere_fragment(const rv_sphere* s, int i, int j, float k, float* zs, float* shade) {
    const float dx = ((float)i + 0.5f) - s->X, dy = ((float)j + 0.5f) - s->Y;
    const float d2 = dx * dx + dy * dy, rr = s->R * s->R;
    if (!(d2 < rr)) return 0;
    const float hgt = sqrtf(rr - d2);
    const float z = s->z - (hgt / k) / 1500.0f;
    if (!(z >= 0.0f && z <= 1.0f)) return 0;
    *zs = z;
    *shade = hgt / s->R;
    return 1;
}

/* VTK's default material under its head light, diffuse only: colour byte x shade, rounded */
RM_FN uint32_t rv_sphere_colour(uint32_t rgb, float shade) {
    const uint32_t r = (uint32_t)(int)((float)(rgb & 255u) * shade + 0.5f);
    const uint32_t g = (uint32_t)(int)((float)((rgb >> 8) & 255u) * shade + 0.5f);
    const uint32_t b = (uint32_t)(int)((float)((rgb >> 16) & 255u) * shade + 0.5f);
    return r | (g << 8) | (b << 16);
}

/* ---- rays (raster_rays.hip): capsules under the same camera --------------------------------------------------------------- */
/* A ray is the set of points within ray_radius of the segment a -> b.  Its record, 64 bytes: both ends projected as
 * rv_project_landmark projects a landmark (window pixels, NOT snapped, z-buffer depth), R = ray_radius * k, the colour, a pixel
 * box that holds every pixel the capsule can cover, and three per-ray terms of the side's arithmetic, in double:
 *   ux = (double)Xb - Xa, uy = (double)Yb - Ya, P2 = ux ux + uy uy            (projected length squared, pixels)
 *   uw = ((double)zb - za) * (1500.0 * (double)k), L2 = P2 + uw uw            (depth extent and 3-D length squared, pixels)
 *   cosi = sqrt(P2 / L2)                                                      (cosine of the inclination to the window plane)
 *   g = uw / sqrt(L2 * P2)
 * A ray whose projected length is at most R / 256 - P2 > (R R) 2^-16 fails, also for a zero-length or end-on ray, P2 = 0 -
 * is drawn from its caps alone (cosi = g = 0): the side could show only in a crescent at most R / 256 pixel wide beside the
 * nearer cap's disc, and below that length its quadratic's leading coefficient P2 is lost against the other terms.
 * A ray with a non-finite end (as given or projected) gets the empty box ix0 > ix1 and covers nothing. */
typedef struct __attribute__((aligned(16))) {
    float Xa, Ya, za, R;
    float Xb, Yb, zb;
    uint32_t rgb;
    int16_t ix0, ix1, iy0, iy1;
    double cosi, g, P2;
} rv_ray;

#define RV_MAX_RAYS 65536 /* of one call: 478 landmarks x 128 views */
#define RV_MAX_RAY_RECORDS (1ll << 20) /* n_views * n_rays of one call: 64 MB of records ("rays.rec", grow-only scratch); 3 x 61 184 uses 11.7 MB */
#define RV_RAY_RGB 0x1AE61Au /* the reference's (0.1, 0.9, 0.1) (ray_visualizer.py) as bytes (26, 230, 26): r | g << 8 | b << 16 */

RM_FN int rv_finite(double x) { return x - x == 0.0; }

RM_FN rv_ray rv_project_ray(const double* m, const double* a, const double* b, float cx, float cy, float half, float k,
                            float ray_radius, uint32_t rgb, int size) {
    const rv_sphere sa = rv_project_landmark(m, a, cx, cy, half, k, ray_radius, rgb, size);
    const rv_sphere sb = rv_project_landmark(m, b, cx, cy, half, k, ray_radius, rgb, size);
    rv_ray r;
    r.Xa = sa.X; r.Ya = sa.Y; r.za = sa.z; r.R = sa.R;
    r.Xb = sb.X; r.Yb = sb.Y; r.zb = sb.z;
    r.rgb = rgb;
    r.ix0 = sa.ix0 < sb.ix0 ? sa.ix0 : sb.ix0;
    r.ix1 = sa.ix1 > sb.ix1 ? sa.ix1 : sb.ix1;
    r.iy0 = sa.iy0 < sb.iy0 ? sa.iy0 : sb.iy0;
    r.iy1 = sa.iy1 > sb.iy1 ? sa.iy1 : sb.iy1;
    r.cosi = 0.0; r.g = 0.0; r.P2 = 0.0;
    int finite = rv_finite(sa.X) && rv_finite(sa.Y) && rv_finite(sa.z) && rv_finite(sb.X) && rv_finite(sb.Y) && rv_finite(sb.z) &&
                 rv_finite(sa.R);
    for (int c = 0; c < 3; ++c) finite = finite && rv_finite(a[c]) && rv_finite(b[c]);
    if (!finite) {
        r.Xa = r.Ya = r.za = r.Xb = r.Yb = r.zb = r.R = 0.0f;
        r.ix0 = r.iy0 = 1;
        r.ix1 = r.iy1 = 0;
        return r;
    }
    const double ux = (double)r.Xb - (double)r.Xa, uy = (double)r.Yb - (double)r.Ya;
    const double P2 = ux * ux + uy * uy;
    const double uw = ((double)r.zb - (double)r.za) * (1500.0 * (double)k);
    const double L2 = P2 + uw * uw;
    const double Rd = (double)r.R;
    if (P2 > (Rd * Rd) * (1.0 / 65536.0)) {
        r.P2 = P2;
        r.cosi = sqrt(P2 / L2);
        r.g = uw / sqrt(L2 * P2);
    }
    return r;
}

/* The ray's fragment at pixel (i, j): the capsule's point nearest the camera on the line of sight through the pixel centre
 * (px, py) = ((float)i + 0.5f, (float)j + 0.5f) - one of up to three candidates, then ONE clip test on its depth.
 *   cap A, cap B (float, rv_sphere_fragment's arithmetic before its clip): dx = px - X, dy = py - Y, d2 = dx dx + dy dy,
 *     candidate iff d2 < R R; hgt = sqrtf(R R - d2), z = z_end - (hgt / k) / 1500, shade = hgt / R
 *   side (double, only when cosi > 0): qx = (double)px - Xa, qy = (double)py - Ya, e = qx ux + qy uy, cr = qx uy - qy ux,
 *     h2 = R R - (cr cr) / P2, candidate iff h2 > 0 and 0 <= t <= 1 with hgt = sqrt(h2), t = e / P2 - g hgt (the axis
 *     parameter of the surface point); up = hgt cosi is the camera-ward part of the radius vector there;
 *     z = (float)((za + t (zb - za)) - (up / k) / 1500)  - the axis point's z-buffer value minus a height over k and 1500,
 *     as the sphere forms it, never a depth in pixels -;  shade = (float)(up / R)
 * The side's candidate, where there is one, IS the fragment: the capsule is convex, a surface point with 0 <= t <= 1 is where the
 * line of sight enters it, and the caps' points there lie behind or on it - by less than a float of z can tell at k = 50, so
 * they are not compared.  Otherwise the nearer cap, B only when strictly nearer than A.  No fragment without a candidate - the
 * union of the three is the 2-D capsule of radius R - or when the chosen z leaves [0, 1]. */
RM_FN int rv_ray_fragment(const rv_ray* r, int i, int j, float k, float* zr, float* shade) {
    const float px = (float)i + 0.5f, py = (float)j + 0.5f;
    const float rr = r->R * r->R;
    int found = 0;
    float z = 0.0f, s = 0.0f;
    {
        const float dx = px - r->Xa, dy = py - r->Ya;
        const float d2 = dx * dx + dy * dy;
        if (d2 < rr) {
            const float hgt = sqrtf(rr - d2);
            z = r->za - (hgt / k) / 1500.0f;
            s = hgt / r->R;
            found = 1;
        }
    }
    {
        const float dx = px - r->Xb, dy = py - r->Yb;
        const float d2 = dx * dx + dy * dy;
        if (d2 < rr) {
            const float hgt = sqrtf(rr - d2);
            const float zb = r->zb - (hgt / k) / 1500.0f;
            if (!found || zb < z) {
                z = zb;
                s = hgt / r->R;
                found = 1;
            }
        }
    }
    if (r->cosi > 0.0) {
        const double ux = (double)r->Xb - (double)r->Xa, uy = (double)r->Yb - (double)r->Ya;
        const double qx = (double)px - (double)r->Xa, qy = (double)py - (double)r->Ya;
        const double e = qx * ux + qy * uy, cr = qx * uy - qy * ux;
        const double Rd = (double)r->R;
        const double h2 = Rd * Rd - (cr * cr) / r->P2;
        if (h2 > 0.0) {
            const double hgt = sqrt(h2);
            const double t = e / r->P2 - r->g * hgt;
            if (t >= 0.0 && t <= 1.0) {
                const double up = hgt * r->cosi;
                z = (float)(((double)r->za + t * ((double)r->zb - (double)r->za)) - (up / (double)k) / 1500.0);
                s = (float)(up / Rd);
                found = 1;
            }
        }
    }
    if (!found || !(z >= 0.0f && z <= 1.0f)) return 0;
    *zr = z;
    *shade = s;
    return 1;
}

/* Conservative: 0 only where no pixel of the 16 x 16 tile at (tx0, ty0) can have a fragment of the ray.  The box first; then the
 * float distance from the centre of the tile's pixel centres to the projected segment against R + the half diagonal of those
 * centres (7.5 sqrt 2 < 10.75) + a margin for the roundings of this very distance: 1 pixel and 2^-18 of the coordinates'
 * magnitudes (the foot point's parameter carries a relative error of a few 2^-24 of them).  A NaN anywhere says "touches". */
RM_FN int rv_ray_touches_tile(const rv_ray* r, int tx0, int ty0) {
    if (!(r->ix0 <= tx0 + 15 && r->ix1 >= tx0 && r->iy0 <= ty0 + 15 && r->iy1 >= ty0)) return 0;
    const float ux = r->Xb - r->Xa, uy = r->Yb - r->Ya;
    const float qx = ((float)tx0 + 8.0f) - r->Xa, qy = ((float)ty0 + 8.0f) - r->Ya;
    const float p2 = ux * ux + uy * uy;
    float t = p2 > 0.0f ? (qx * ux + qy * uy) / p2 : 0.0f;
    t = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;
    const float dx = qx - t * ux, dy = qy - t * uy;
    const float thr = (r->R + 11.75f) + (((fabsf(r->Xa) + fabsf(r->Ya)) + (fabsf(r->Xb) + fabsf(r->Yb))) * (1.0f / 262144.0f));
    return !(dx * dx + dy * dy > thr * thr);
}

#endif
