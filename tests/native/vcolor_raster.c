/*
 * CPU model of the renderer contract with per-vertex colours (TEST INFRASTRUCTURE, like oracle/raster.c, which it includes
 * for the projection, orientation, tie rule and geometry shade, and does not change).
 *
 * Written from the contract ("Per-vertex colours" and "Multisampling"), not from the kernels:
 *   - `samples` points per pixel: 1 = the pixel centre (8, 8) in 1/16 pixel, oracle/raster.c's contract bit for bit;
 *     4 = (3,6) (13,10) (6,13) (10,3), the multisampled contract of tests/native/msaa_raster.c;
 *   - coverage, depth (the plane through vertex a at the sample point) and the LEQUAL depth test per sample, with the
 *     LEFT / BOTTOM tie rule of the pixel centres;
 *   - a sample's colour is its winning triangle's colour evaluated ONCE per pixel at the pixel centre, with the centre's
 *     barycentric weights even where the centre lies outside the triangle (extrapolated);
 *   - that colour: with shading 0, colours given and no usable texture (uvs or tex missing), per channel
 *         f = c0/255 + (b1 * (c1/255 - c0/255) + b2 * (c2/255 - c0/255))      (float; vertices after the winding swap)
 *         f clamped to [0, 1];  c16 = (int)(f * 65535);  byte = (c16 - (c16 >> 8) + 128) >> 8
 *     with a texture and uvs the texel, colours or not; with shading 1 the geometry shade; otherwise white;
 *   - resolve: per byte the rounding-up average of samples 0 and 1, of 2 and 3, then of the two (an uncovered sample is
 *     white); the depth plane is the byte of sample 0's depth (1.0 when it is uncovered) and never sees a colour.
 * Organised as a full-frame z-buffer per sample, triangle after triangle in draw order - unlike the tile-binned kernels.
 *
 * build (tests/vcolor_model.py): gcc -O2 -ffp-contract=off -fPIC -shared vcolor_raster.c -o libvcolor_raster.so -lm
 */
#include "../../oracle/raster.c"

#define MAX_SAMPLES 4

static const int POS1[1][2] = {{8, 8}};
static const int POS4[4][2] = {{3, 6}, {13, 10}, {6, 13}, {10, 3}};

static int resolve_byte(const int* v, int ns) {
    if (ns == 1) return v[0];
    const int a = (v[0] + v[1] + 1) >> 1, b = (v[2] + v[3] + 1) >> 1;
    return (a + b + 1) >> 1;
}

static int colour_byte(float f) {
    if (f < 0.0f) f = 0.0f;
    if (f > 1.0f) f = 1.0f;
    const int c16 = (int)(f * 65535.0f); /* 16-bit fixed point, truncated */
    return (c16 - (c16 >> 8) + 128) >> 8;
}

/* verts f32[V,3], uvs f32[V,2] or NULL, tris i32[T,3], tex u8[th,tw,3] or NULL, colors u8[V,3] or NULL, rot f64[n_views,9]
 * -> out f32[n_views,256,256,4] (image rows, like oracle_render_bits);
 *    win_tri i32[n_views,256,256,samples] or NULL: each sample's winning triangle (-1: uncovered), GL rows (row 0 = bottom);
 *    win_rgb u8[n_views,256,256,samples,3] or NULL: each sample's colour before the resolve, GL rows */
int vcolor_render(const float* verts, const float* uvs, int n_verts, const int32_t* tris, int n_tris, const uint8_t* tex,
                  int th, int tw, const uint8_t* colors, const double* rot, int n_views, int shading, int subpixel_bits, int samples, float* out,
                int32_t* win_tri, uint8_t* win_rgb) {
    const int(*pos)[2] = samples == 1 ? POS1 : samples == 4 ? POS4 : NULL;
    if (!pos) return 3;
    if (subpixel_bits < 4 || subpixel_bits > 8 || (shading == 1 && subpixel_bits != 8)) return 2;
    const int32_t S = 1 << subpixel_bits, H = S / 2, NS = samples;
    int32_t ox[MAX_SAMPLES], oy[MAX_SAMPLES], oxmin = S, oxmax = 0, oymin = S, oymax = 0;
    for (int s = 0; s < NS; ++s) { /* 1/16 pixel -> the vertex lattice (exact for 4..8 bits) */
        ox[s] = pos[s][0] * (S / 16);
        oy[s] = pos[s][1] * (S / 16);
        if (ox[s] < oxmin) oxmin = ox[s];
        if (ox[s] > oxmax) oxmax = ox[s];
        if (oy[s] < oymin) oymin = oy[s];
        if (oy[s] > oymax) oymax = oy[s];
    }
    SV* sv = (SV*)malloc(sizeof(SV) * (size_t)n_verts);
    float* zbuf = (float*)malloc(sizeof(float) * N * N * NS);
    int32_t* owner = (int32_t*)malloc(sizeof(int32_t) * N * N * NS);
    if (!sv || !zbuf || !owner) return 1;
    for (int view = 0; view < n_views; ++view) {
        const double* m = rot + 9 * view;
        for (int i = 0; i < n_verts; ++i) sv[i] = project(m, verts + 3 * i, subpixel_bits);
        for (int p = 0; p < N * N * NS; ++p) {
            zbuf[p] = 2.0f;
            owner[p] = -1;
        }
        for (int t = 0; t < n_tris; ++t) {
            SV a = sv[tris[3 * t]], b = sv[tris[3 * t + 1]], c = sv[tris[3 * t + 2]];
            int64_t area = orient(a, b, c.x, c.y);
            if (area == 0) continue;
            if (area < 0) {
                SV x = b; b = c; c = x;
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
            /* pixels with a sample point that may lie in the box (the per-sample test below decides) */
            int i0 = -fdiv(-(minx - oxmax), S), i1 = fdiv(maxx - oxmin, S);
            int j0 = -fdiv(-(miny - oymax), S), j1 = fdiv(maxy - oymin, S);
            if (i0 < 0) i0 = 0;
            if (j0 < 0) j0 = 0;
            if (i1 > N - 1) i1 = N - 1;
            if (j1 > N - 1) j1 = N - 1;
            const float fa = (float)area;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i)
                    for (int s = 0; s < NS; ++s) {
                        const int32_t px = i * S + ox[s], py = j * S + oy[s];
                        int64_t w0 = orient(b, c, px, py), w1 = orient(c, a, px, py), w2 = orient(a, b, px, py);
                        if (w0 < 0 || w1 < 0 || w2 < 0) continue;
                        if (w0 == 0 && !owns(b, c)) continue;
                        if (w1 == 0 && !owns(c, a)) continue;
                        if (w2 == 0 && !owns(a, b)) continue;
                        float b1 = (float)w1 / fa, b2 = (float)w2 / fa;
                        float z = a.z + (b1 * (b.z - a.z) + b2 * (c.z - a.z));
                        if (!(z >= 0.0f && z <= 1.0f)) continue;
                        const int q = (j * N + i) * NS + s;
                        if (z <= zbuf[q]) {
                            zbuf[q] = z;
                            owner[q] = t;
                        }
                    }
        }
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < N; ++i) {
                int ch[3][MAX_SAMPLES];
                for (int s = 0; s < NS; ++s) {
                    const int q = (j * N + i) * NS + s, t = owner[q];
                    int rgb[3] = {255, 255, 255};
                    if (t >= 0) {
                        int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
                        SV a = sv[ia], b = sv[ib], c = sv[ic];
                        int64_t area = orient(a, b, c.x, c.y);
                        if (area < 0) {
                            SV x = b; b = c; c = x;
                            int y = ib; ib = ic; ic = y;
                            area = -area;
                        }
                        if (shading == 1) {
                            rgb[0] = rgb[1] = rgb[2] = geometry_u8(a, b, c);
                        } else if (colors && !(tex && uvs)) {
                            /* the vertex colours' plane through vertex a, at the centre like every varying */
                            const int32_t px = i * S + H, py = j * S + H;
                            const float fa = (float)area;
                            float b1 = (float)orient(c, a, px, py) / fa, b2 = (float)orient(a, b, px, py) / fa;
                            for (int k = 0; k < 3; ++k) {
                                const float c0 = (float)colors[3 * ia + k] / 255.0f, c1 = (float)colors[3 * ib + k] / 255.0f,
                                            c2 = (float)colors[3 * ic + k] / 255.0f;
                                rgb[k] = colour_byte(c0 + (b1 * (c1 - c0) + b2 * (c2 - c0)));
                            }
                        } else if (tex && uvs) {
                            /* once per pixel, at the centre, inside the triangle or not */
                            const int32_t px = i * S + H, py = j * S + H;
                            const float fa = (float)area;
                            float b1 = (float)orient(c, a, px, py) / fa, b2 = (float)orient(a, b, px, py) / fa;
                            float u0 = uvs[2 * ia], v0 = uvs[2 * ia + 1];
                            float u = u0 + (b1 * (uvs[2 * ib] - u0) + b2 * (uvs[2 * ic] - u0));
                            float v = v0 + (b1 * (uvs[2 * ib + 1] - v0) + b2 * (uvs[2 * ic + 1] - v0));
                            float uu = u - floorf(u), vv = v - floorf(v);
                            int tx = (int)(uu * (float)tw), ty = (int)(vv * (float)th);
                            if (tx > tw - 1) tx = tw - 1;
                            if (ty > th - 1) ty = th - 1;
                            if (tx < 0) tx = 0;
                            if (ty < 0) ty = 0;
                            const uint8_t* texel = tex + ((size_t)(th - 1 - ty) * tw + tx) * 3;
                            rgb[0] = texel[0]; rgb[1] = texel[1]; rgb[2] = texel[2];
                        }
                    }
                    const size_t wq = ((size_t)view * N * N + (size_t)j * N + i) * NS + s;
                    if (win_tri) win_tri[wq] = t;
                    for (int k = 0; k < 3; ++k) {
                        if (win_rgb) win_rgb[wq * 3 + k] = (uint8_t)rgb[k];
                        ch[k][s] = rgb[k];
                    }
                }
                const float z = owner[(j * N + i) * NS] >= 0 ? zbuf[(j * N + i) * NS] : 1.0f; /* sample 0 */
                int d8 = (256 - (int)(255.0 * (double)z)) & 255;
                float* o = out + (((size_t)view * N + (N - 1 - j)) * N + i) * 4;
                for (int k = 0; k < 3; ++k) o[k] = (float)resolve_byte(ch[k], NS) / 255.0f;
                o[3] = (float)d8 / 255.0f;
            }
    }
    free(sv);
    free(zbuf);
    free(owner);
    return 0;
}
