/*
 * CPU model of the ray view (TEST INFRASTRUCTURE): mvlm_render_ray_view restated from the contract (DESIGN.md section 5.1,
 * "Ray view", and the operation order written down in raster_view_math.h), without any of the product's headers.  The mesh and the
 * spheres are the landmark view's model (landmark_view.c, included for its helpers; its passes are repeated here because the rays
 * go between them, into the same z-buffer):
 *
 *   - mesh, then rays in index order, then spheres in landmark order, all LEQUAL into one full-frame z-buffer: a ray wins an
 *     equal depth against the mesh, the later ray against an earlier one, a sphere against a ray;
 *   - a ray: both ends projected as a landmark is (unsnapped window position, z = (500 - zv) / 1500), R = ray_radius * k;
 *     skipped when a coordinate, given or projected, is not finite.  In double: ux, uy the projected axis, P2 = ux ux + uy uy,
 *     uw = (zb - za) * (1500 k), L2 = P2 + uw uw; caps only unless P2 > R R / 65536, else cosi = sqrt(P2 / L2),
 *     g = uw / sqrt(L2 P2);
 *   - its fragment at a pixel centre: the side's candidate where there is one, else the nearer of cap A and cap B (the sphere's
 *     float arithmetic, unclipped; B only when strictly nearer); the side
 *     (double: e = q.u, cr = q x u, h2 = R R - cr cr / P2 > 0, hgt = sqrt(h2), t = e / P2 - g hgt in [0, 1], up = hgt cosi,
 *     z = (float)((za + t (zb - za)) - (up / k) / 1500), shade (float)(up / R)); then one clip test 0 <= z <= 1; byte (int)((float)c * shade + 0.5f).
 * Every pixel of the ray's clamped bounding box is visited: no tile test to depend on.
 *
 * build (tests/ray_model.py): gcc -O2 -ffp-contract=off -fPIC -shared ray_view.c -o libray_view.so -lm
 */
#include "landmark_view.c"

#define RAY_CODE_BASE (-1000000) /* winner plane: ray r is RAY_CODE_BASE - r (below every sphere's -2 - l) */

static int finite_d(double x) { return x - x == 0.0; }

/* out, lm_pixels, winner as landmark_view's; ray_pixels i32[n_views,n_rays] or NULL; depth f32[n_views,size,size] or NULL, image
 * rows: the winner's z-buffer value, +inf on the background */
int ray_view(const float* verts, const float* uvs, int n_verts, const int32_t* tris, int n_tris, const uint8_t* tex, int th, int tw,
             const uint8_t* colors, const double* rot, int n_views, int size, const float* frame, const double* lms, int n_lm,
             float radius, const uint8_t* lm_rgb, const double* starts, const double* ends, int n_rays, float ray_radius,
             const uint8_t* ray_rgb, int shading, int bits, uint8_t* out, int32_t* lm_pixels, int32_t* ray_pixels, int32_t* winner,
             float* depth) {
    if (bits < 4 || bits > 8 || size < 16) return 2;
    const int32_t S = 1 << bits, H = S / 2, N = size;
    PV* pv = (PV*)malloc(sizeof(PV) * (size_t)(n_verts > 0 ? n_verts : 1));
    float* zbuf = (float*)malloc(sizeof(float) * (size_t)N * N);
    int32_t* owner = (int32_t*)malloc(sizeof(int32_t) * (size_t)N * N);
    uint8_t* srgb = (uint8_t*)malloc((size_t)N * N * 3);
    if (!pv || !zbuf || !owner || !srgb) return 1;
    for (int view = 0; view < n_views; ++view) {
        const double* m = rot + 9 * view;
        const float cx = frame[3 * view], cy = frame[3 * view + 1], half = frame[3 * view + 2];
        const float k = (float)size / (2.0f * half);
        for (int i = 0; i < n_verts; ++i) {
            const double x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
            const float xv = (float)((m[0] * x + m[1] * y) + m[2] * z);
            const float yv = (float)((m[3] * x + m[4] * y) + m[5] * z);
            const float zv = (float)((m[6] * x + m[7] * y) + m[8] * z);
            float fx = floorf((((xv - cx) + half) * k) * (float)S + 0.5f);
            float fy = floorf((((yv - cy) + half) * k) * (float)S + 0.5f);
            const float lim = (float)(1 << (14 + bits)); /* 16 384 pixels */
            if (fx < -lim) fx = -lim;
            if (fx > lim) fx = lim;
            if (fy < -lim) fy = -lim;
            if (fy > lim) fy = lim;
            pv[i].x = (int32_t)fx;
            pv[i].y = (int32_t)fy;
            pv[i].z = (500.0f - zv) / 1500.0f;
        }
        for (size_t p = 0; p < (size_t)N * N; ++p) {
            zbuf[p] = INFINITY;
            owner[p] = -1;
        }
        for (int t = 0; t < n_tris; ++t) {
            PV a = pv[tris[3 * t]], b = pv[tris[3 * t + 1]], c = pv[tris[3 * t + 2]];
            int64_t area = orient2(a, b, c.x, c.y);
            if (area == 0) continue;
            if (area < 0) {
                PV s = b; b = c; c = s;
                area = -area;
            }
            int32_t minx = a.x, maxx = a.x, miny = a.y, maxy = a.y;
            if (b.x < minx) minx = b.x;
            if (c.x < minx) minx = c.x;
            if (b.x > maxx) maxx = b.x;
            if (c.x > maxx) maxx = c.x;
            if (b.y < miny) miny = b.y;
            if (c.y < miny) miny = c.y;
            if (b.y > maxy) maxy = b.y;
            if (c.y > maxy) maxy = c.y;
            int i0 = -floordiv(-(minx - H), S), i1 = floordiv(maxx - H, S);
            int j0 = -floordiv(-(miny - H), S), j1 = floordiv(maxy - H, S);
            if (i0 < 0) i0 = 0;
            if (j0 < 0) j0 = 0;
            if (i1 > N - 1) i1 = N - 1;
            if (j1 > N - 1) j1 = N - 1;
            const float fa = (float)area;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) {
                    const int32_t px = i * S + H, py = j * S + H;
                    const int64_t w0 = orient2(b, c, px, py), w1 = orient2(c, a, px, py), w2 = orient2(a, b, px, py);
                    if (w0 < 0 || w1 < 0 || w2 < 0) continue;
                    if (w0 == 0 && !owns_edge(b, c)) continue;
                    if (w1 == 0 && !owns_edge(c, a)) continue;
                    if (w2 == 0 && !owns_edge(a, b)) continue;
                    const float b1 = (float)w1 / fa, b2 = (float)w2 / fa;
                    const float z = a.z + (b1 * (b.z - a.z) + b2 * (c.z - a.z));
                    if (!(z >= 0.0f && z <= 1.0f)) continue;
                    const size_t p = (size_t)j * N + i;
                    if (z <= zbuf[p]) {
                        zbuf[p] = z;
                        owner[p] = t;
                    }
                }
        }
        /* the rays, drawn after the mesh in index order, LEQUAL */
        for (int r = 0; r < n_rays; ++r) {
            const double* a = starts + 3 * (size_t)r;
            const double* b = ends + 3 * (size_t)r;
            const float xa = (float)((m[0] * a[0] + m[1] * a[1]) + m[2] * a[2]);
            const float ya = (float)((m[3] * a[0] + m[4] * a[1]) + m[5] * a[2]);
            const float wa = (float)((m[6] * a[0] + m[7] * a[1]) + m[8] * a[2]);
            const float xb = (float)((m[0] * b[0] + m[1] * b[1]) + m[2] * b[2]);
            const float yb = (float)((m[3] * b[0] + m[4] * b[1]) + m[5] * b[2]);
            const float wb = (float)((m[6] * b[0] + m[7] * b[1]) + m[8] * b[2]);
            const float Xa = ((xa - cx) + half) * k, Ya = ((ya - cy) + half) * k, za = (500.0f - wa) / 1500.0f;
            const float Xb = ((xb - cx) + half) * k, Yb = ((yb - cy) + half) * k, zb = (500.0f - wb) / 1500.0f;
            const float R = ray_radius * k;
            int ok = finite_d(Xa) && finite_d(Ya) && finite_d(za) && finite_d(Xb) && finite_d(Yb) && finite_d(zb) && finite_d(R);
            for (int c = 0; c < 3; ++c) ok = ok && finite_d(a[c]) && finite_d(b[c]);
            if (!ok) continue;
            const double ux = (double)Xb - (double)Xa, uy = (double)Yb - (double)Ya;
            const double P2 = ux * ux + uy * uy;
            const double uw = ((double)zb - (double)za) * (1500.0 * (double)k);
            const double L2 = P2 + uw * uw;
            const double Rd = (double)R;
            double cosi = 0.0, g = 0.0;
            if (P2 > (Rd * Rd) * (1.0 / 65536.0)) {
                cosi = sqrt(P2 / L2);
                g = uw / sqrt(L2 * P2);
            }
            double lo_x = floor(fmin(Xa, Xb) - Rd) - 2, hi_x = floor(fmax(Xa, Xb) + Rd) + 2;
            double lo_y = floor(fmin(Ya, Yb) - Rd) - 2, hi_y = floor(fmax(Ya, Yb) + Rd) + 2;
            if (!(lo_x > 0)) lo_x = 0;
            if (!(lo_y > 0)) lo_y = 0;
            if (!(hi_x < N - 1)) hi_x = N - 1;
            if (!(hi_y < N - 1)) hi_y = N - 1;
            if (lo_x > N) lo_x = N;
            if (lo_y > N) lo_y = N;
            if (hi_x < -1) hi_x = -1;
            if (hi_y < -1) hi_y = -1;
            const uint8_t base[3] = {ray_rgb ? ray_rgb[3 * r] : 26, ray_rgb ? ray_rgb[3 * r + 1] : 230, ray_rgb ? ray_rgb[3 * r + 2] : 26};
            for (int j = (int)lo_y; j <= (int)hi_y; ++j)
                for (int i = (int)lo_x; i <= (int)hi_x; ++i) {
                    const float px = (float)i + 0.5f, py = (float)j + 0.5f;
                    int found = 0;
                    float z = 0.0f, shade = 0.0f;
                    {
                        const float dx = px - Xa, dy = py - Ya;
                        const float d2 = dx * dx + dy * dy;
                        if (d2 < R * R) {
                            const float hgt = sqrtf(R * R - d2);
                            z = za - (hgt / k) / 1500.0f;
                            shade = hgt / R;
                            found = 1;
                        }
                    }
                    {
                        const float dx = px - Xb, dy = py - Yb;
                        const float d2 = dx * dx + dy * dy;
                        if (d2 < R * R) {
                            const float hgt = sqrtf(R * R - d2);
                            const float z2 = zb - (hgt / k) / 1500.0f;
                            if (!found || z2 < z) {
                                z = z2;
                                shade = hgt / R;
                                found = 1;
                            }
                        }
                    }
                    if (cosi > 0.0) {
                        const double qx = (double)px - (double)Xa, qy = (double)py - (double)Ya;
                        const double e = qx * ux + qy * uy, cr = qx * uy - qy * ux;
                        const double h2 = Rd * Rd - (cr * cr) / P2;
                        if (h2 > 0.0) {
                            const double hgt = sqrt(h2);
                            const double t = e / P2 - g * hgt;
                            if (t >= 0.0 && t <= 1.0) {
                                const double up = hgt * cosi;
                                z = (float)(((double)za + t * ((double)zb - (double)za)) - (up / (double)k) / 1500.0);
                                shade = (float)(up / Rd);
                                found = 1;
                            }
                        }
                    }
                    if (!found || !(z >= 0.0f && z <= 1.0f)) continue;
                    const size_t p = (size_t)j * N + i;
                    if (!(z <= zbuf[p])) continue;
                    zbuf[p] = z;
                    owner[p] = RAY_CODE_BASE - r;
                    for (int ch = 0; ch < 3; ++ch) srgb[3 * p + ch] = (uint8_t)(int)((float)base[ch] * shade + 0.5f);
                }
        }
        /* the spheres, drawn after the mesh in landmark order, LEQUAL */
        for (int l = 0; l < n_lm; ++l) {
            const double* q = lms + 3 * l;
            const float xv = (float)((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2]);
            const float yv = (float)((m[3] * q[0] + m[4] * q[1]) + m[5] * q[2]);
            const float zv = (float)((m[6] * q[0] + m[7] * q[1]) + m[8] * q[2]);
            const float Xl = ((xv - cx) + half) * k, Yl = ((yv - cy) + half) * k;
            const float zl = (500.0f - zv) / 1500.0f, R = radius * k;
            /* every pixel the disc can reach, with room for the float roundings (doubles: no overflow on the way) */
            double lo_x = floor((double)Xl - (double)R) - 2, hi_x = floor((double)Xl + (double)R) + 2;
            double lo_y = floor((double)Yl - (double)R) - 2, hi_y = floor((double)Yl + (double)R) + 2;
            if (!(lo_x > 0)) lo_x = 0; /* (also a NaN) */
            if (!(lo_y > 0)) lo_y = 0;
            if (!(hi_x < N - 1)) hi_x = N - 1;
            if (!(hi_y < N - 1)) hi_y = N - 1;
            if (lo_x > N) lo_x = N;
            if (lo_y > N) lo_y = N;
            if (hi_x < -1) hi_x = -1;
            if (hi_y < -1) hi_y = -1;
            const uint8_t base[3] = {lm_rgb ? lm_rgb[3 * l] : 0, lm_rgb ? lm_rgb[3 * l + 1] : 0, lm_rgb ? lm_rgb[3 * l + 2] : 255};
            for (int j = (int)lo_y; j <= (int)hi_y; ++j)
                for (int i = (int)lo_x; i <= (int)hi_x; ++i) {
                    const float dx = ((float)i + 0.5f) - Xl, dy = ((float)j + 0.5f) - Yl;
                    const float d2 = dx * dx + dy * dy;
                    if (!(d2 < R * R)) continue;
                    const float hgt = sqrtf(R * R - d2);
                    const float zs = zl - (hgt / k) / 1500.0f;
                    if (!(zs >= 0.0f && zs <= 1.0f)) continue;
                    const size_t p = (size_t)j * N + i;
                    if (!(zs <= zbuf[p])) continue;
                    zbuf[p] = zs;
                    owner[p] = -2 - l;
                    for (int ch = 0; ch < 3; ++ch) srgb[3 * p + ch] = (uint8_t)(int)((float)base[ch] * (hgt / R) + 0.5f);
                }
        }
        if (lm_pixels)
            for (int l = 0; l < n_lm; ++l) lm_pixels[(size_t)view * n_lm + l] = 0;
        if (ray_pixels)
            for (int r = 0; r < n_rays; ++r) ray_pixels[(size_t)view * n_rays + r] = 0;
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < N; ++i) {
                const size_t p = (size_t)j * N + i;
                int rgb[3] = {255, 255, 255};
                const int32_t t = owner[p];
                if (t <= RAY_CODE_BASE) {
                    for (int ch = 0; ch < 3; ++ch) rgb[ch] = srgb[3 * p + ch];
                    if (ray_pixels) ray_pixels[(size_t)view * n_rays + (RAY_CODE_BASE - t)] += 1;
                } else if (t <= -2) {
                    for (int ch = 0; ch < 3; ++ch) rgb[ch] = srgb[3 * p + ch];
                    if (lm_pixels) lm_pixels[(size_t)view * n_lm + (-2 - t)] += 1;
                } else if (t >= 0) {
                    int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
                    PV a = pv[ia], b = pv[ib], c = pv[ic];
                    int64_t area = orient2(a, b, c.x, c.y);
                    if (area < 0) {
                        PV s = b; b = c; c = s;
                        int y = ib; ib = ic; ic = y;
                        area = -area;
                    }
                    const int32_t px = i * S + H, py = j * S + H;
                    const float fa = (float)area;
                    const float b1 = (float)orient2(c, a, px, py) / fa, b2 = (float)orient2(a, b, px, py) / fa;
                    if (shading == 1) {
                        /* the normal from window coordinates in 1/256 pixel and depths converted to the same unit */
                        const float kz = -((384000.0f * (float)size) / (2.0f * half));
                        const float ax = (float)((b.x - a.x) * (256 >> bits)), ay = (float)((b.y - a.y) * (256 >> bits));
                        const float bx = (float)((c.x - a.x) * (256 >> bits)), by = (float)((c.y - a.y) * (256 >> bits));
                        const float az = (b.z - a.z) * kz, bz = (c.z - a.z) * kz;
                        const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
                        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
                        rgb[0] = rgb[1] = rgb[2] = len > 0.0f ? (int)((fabsf(nz) / len) * 255.0f + 0.5f) : 0;
                    } else if (colors && !(tex && uvs)) {
                        for (int ch = 0; ch < 3; ++ch) {
                            const float c0 = (float)colors[3 * ia + ch] / 255.0f, c1 = (float)colors[3 * ib + ch] / 255.0f,
                                        c2 = (float)colors[3 * ic + ch] / 255.0f;
                            rgb[ch] = colour_byte(c0 + (b1 * (c1 - c0) + b2 * (c2 - c0)));
                        }
                    } else if (tex && uvs) {
                        const float u0 = uvs[2 * ia], v0 = uvs[2 * ia + 1];
                        const float u = u0 + (b1 * (uvs[2 * ib] - u0) + b2 * (uvs[2 * ic] - u0));
                        const float v = v0 + (b1 * (uvs[2 * ib + 1] - v0) + b2 * (uvs[2 * ic + 1] - v0));
                        const float uu = u - floorf(u), vv = v - floorf(v);
                        int tx = (int)(uu * (float)tw), ty = (int)(vv * (float)th);
                        if (tx > tw - 1) tx = tw - 1;
                        if (ty > th - 1) ty = th - 1;
                        if (tx < 0) tx = 0;
                        if (ty < 0) ty = 0;
                        const uint8_t* texel = tex + ((size_t)(th - 1 - ty) * tw + tx) * 3;
                        rgb[0] = texel[0]; rgb[1] = texel[1]; rgb[2] = texel[2];
                    }
                }
                const size_t o = ((size_t)view * N + (N - 1 - j)) * N + i;
                out[4 * o] = (uint8_t)rgb[0];
                out[4 * o + 1] = (uint8_t)rgb[1];
                out[4 * o + 2] = (uint8_t)rgb[2];
                out[4 * o + 3] = 255;
                if (winner) winner[o] = t;
                if (depth) depth[o] = zbuf[p];
            }
    }
    free(pv);
    free(zbuf);
    free(owner);
    free(srgb);
    return 0;
}

