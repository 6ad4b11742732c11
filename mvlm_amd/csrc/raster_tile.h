// The tile stage of the multi-view rasteriser as function templates: one body per sample count, instantiated with and
// without per-vertex colours.  raster.hip (tile_kernel) and raster_ms.hip (tile_ms_kernel<4>) wrap the VCOL = false forms in
// kernels whose signatures the occupancy tables know; raster_vc.hip wraps the VCOL = true forms, which shade the RGB planes
// with the mesh's per-vertex colours instead of a texel ("Per-vertex colours").  Also here: what the bodies
// share with the classify kernels of their files - the 24-bit edge functions and the sample pattern.  (Their prologue: raster_bins.h.)
#ifndef MVLM_RASTER_TILE_H
#define MVLM_RASTER_TILE_H

#include "raster_common.h"

namespace {

// ---- 24-bit path ---------------------------------------------------------------------------------------------------------
// rm_setup / rm_cover evaluate the area and the three edge functions in 64-bit integers (window coordinates reach
// +-2^22 sub-pixel steps), and a 64-bit or a full 32-bit integer multiply runs at a quarter of the vector rate.  A
// triangle whose vertices lie within 2^14 steps (64 pixels) of each other
// in x and in y - every triangle of a dense scan - has |dx|, |dy| < 2^14 and, for a pixel centre inside its bounding box,
// |px - ax|, |py - ay| < 2^14: every product is below 2^28 and fits the full-rate 24-bit multiply (v_mul_i32_i24), every
// edge value and the area are below 2^29.  The integers are THE SAME as rm_setup's / rm_cover's, so are the floats made
// from them: a kernel may take either path per triangle and the image does not change by a bit (oracle/raster.c, the
// tests' checker, knows only the 64-bit form).  Worth 3-5 % of a render.  (RM_SMALL_EXTENT, small_extent: raster_common.h)
struct tri24 {
    int32_t X0, Y0, X1, Y1, X2, Y2;  // after the winding swap (vertices 1 and 2)
    float z0, z1, z2;
    float farea;
    int32_t swapped;
};

// rm_setup without the bounding box; false for a zero-area triangle
__device__ inline bool setup24(rm_vert a, rm_vert b, rm_vert c, tri24* t) {
    int32_t area = __mul24(b.X - a.X, c.Y - a.Y) - __mul24(b.Y - a.Y, c.X - a.X);
    t->swapped = 0;
    if (area < 0) {
        const rm_vert s = b;
        b = c;
        c = s;
        area = -area;
        t->swapped = 1;
    }
    t->X0 = a.X; t->Y0 = a.Y; t->X1 = b.X; t->Y1 = b.Y; t->X2 = c.X; t->Y2 = c.Y;
    t->z0 = a.z; t->z1 = b.z; t->z2 = c.z;
    t->farea = float(area);
    return area != 0;
}

// the geometry plane's shade (rm_geometry_u8 reads the swapped vertices and depths only)
__device__ inline int geometry24(const tri24* t) {
    rm_tri r = {};
    r.X0 = t->X0; r.Y0 = t->Y0; r.X1 = t->X1; r.Y1 = t->Y1; r.X2 = t->X2; r.Y2 = t->Y2;
    r.z0 = t->z0; r.z1 = t->z1; r.z2 = t->z2;
    return rm_geometry_u8(&r);
}

__device__ inline int edge24(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py, int32_t* w) {
    const int32_t dx = bx - ax, dy = by - ay;
    const int32_t e = __mul24(dx, py - ay) - __mul24(dy, px - ax);
    *w = e;
    if (e > 0) return 1;
    if (e < 0) return 0;
    return RM_OWNS(dx, dy);
}

// rm_cover for a pixel centre inside the triangle's bounding box (T: tri24, or an rm_tri of small extent)
template <class T>
__device__ inline int cover24(const T* t, int i, int j, float* b0, float* b1, float* b2) {
    const int32_t px = i * RM_SUB + RM_HALF, py = j * RM_SUB + RM_HALF;
    int32_t w0, w1, w2;
    const int in0 = edge24(t->X1, t->Y1, t->X2, t->Y2, px, py, &w0);
    const int in1 = edge24(t->X2, t->Y2, t->X0, t->Y0, px, py, &w1);
    const int in2 = edge24(t->X0, t->Y0, t->X1, t->Y1, px, py, &w2);
    if (!(in0 && in1 && in2)) return 0;
    *b0 = float(w0) / t->farea;
    *b1 = float(w1) / t->farea;
    *b2 = float(w2) / t->farea;
    return 1;
}

// One workgroup per (view, 16x16-pixel tile), one thread per pixel.  More pixels per thread with the loads of a stage
// (key, triangle, vertices and texture coordinates, texel) in flight together were built and measured (2 and 4 pixels:
// 161 / 163 us per render against 164): the kernel does not wait for latency, it moves its bytes at the rate the memory
// system gives - without the texel fetch 43 of its 76 us, without any shading 37 = key plane in, pixels out at 4 TB/s.
// VCOL: the unlit shade is the interpolated vertex colour (`colors`) - nothing is read from uvs / tex.
template <bool VCOL>
__device__ __forceinline__ void tile_body(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                          const float* __restrict__ uvs, const uint8_t* __restrict__ tex, int tex_w, int tex_h,
                                          const uchar4* __restrict__ colors, int n_verts, const int* __restrict__ counts,
                                          const int* __restrict__ offsets, const int* __restrict__ bins, int cap,
                                          unsigned long long* __restrict__ keys, int shading, int n_views,
                                          const int* __restrict__ overflow, int* __restrict__ overflow_host,
                                          float* __restrict__ out) {
    __shared__ rm_tri s_tri[256];  // (valid == 2: small extent, the 24-bit edge functions apply)
    __shared__ int s_id[256];
    int view, tile;
    if (!view_chunk(TILES, n_views, &view, &tile)) return;
    const int tid = threadIdx.x;
    const auto [x0, y0, i, j, tvv, n, list] = tile_prologue<int>(view, tile, RM_TILES, tv, n_verts, counts, offsets, bins, cap);

    unsigned long long* const key_slot = keys + (size_t(view) * RM_SIZE + j) * RM_SIZE + i;
    uint64_t best = *key_slot;  // what the small triangles left
    // The key plane is handed back EMPTY: this kernel reads every slot of the rendered views exactly once, so it also clears
    // what classify dirtied - instead of a 67 MB fill in front of every render (14 us + a launch gap at 128 views)
    if (best != RM_KEY_EMPTY) *key_slot = RM_KEY_EMPTY;
    publish_overflow(overflow, overflow_host);

    // ---- phase B: every pixel walks the tile's big triangles, set up into LDS a chunk at a time ----
    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if (tid < m) {
            const int t = list[base + tid];
            const rm_vert a = load_vert(tvv, tris[3 * t]), b = load_vert(tvv, tris[3 * t + 1]), c = load_vert(tvv, tris[3 * t + 2]);
            rm_tri tr = rm_setup(a, b, c);
            if (tr.valid && small_extent(a, b, c)) tr.valid = 2;
            s_id[tid] = t;
            s_tri[tid] = tr;
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const rm_tri* t = &s_tri[k];
            if (i < t->ix0 || i > t->ix1 || j < t->iy0 || j > t->iy1) continue;
            float b0, b1, b2;
            if (!(t->valid == 2 ? cover24(t, i, j, &b0, &b1, &b2) : rm_cover(t, i, j, &b0, &b1, &b2))) continue;
            const float z = rm_interp(b0, b1, b2, t->z0, t->z1, t->z2);
            if (!(z >= 0.0f && z <= 1.0f)) continue;  // near / far clip (render3d.py:136)
            const uint64_t key = rm_key(z, uint32_t(s_id[k]));
            best = key < best ? key : best;
        }
    }

    // ---- phase C: shade the winner ----
    float4 px = make_float4(1.f, 1.f, 1.f, float(rm_depth_u8(1.0f)) / 255.0f);  // white background, far plane
    if (best != RM_KEY_EMPTY) {
        const int t = int(rm_key_tri(best));
        int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
        const rm_vert va = load_vert(tvv, a), vb = load_vert(tvv, b), vc = load_vert(tvv, c);
        // the winner's barycentric weights at this pixel (it is covered: inside the triangle's box)
        float b0 = 0.f, b1 = 0.f, b2 = 0.f;
        bool swapped;
        float r = 255.f, g = 255.f, bl = 255.f;
        if (small_extent(va, vb, vc)) {
            tri24 tr;
            setup24(va, vb, vc, &tr);
            swapped = tr.swapped != 0;
            cover24(&tr, i, j, &b0, &b1, &b2);
            if (shading == 1) r = g = bl = float(geometry24(&tr));
        } else {
            const rm_tri tr = rm_setup(va, vb, vc);
            swapped = tr.swapped != 0;
            rm_cover(&tr, i, j, &b0, &b1, &b2);
            if (shading == 1) r = g = bl = float(rm_geometry_u8(&tr));
        }
        if (swapped) {
            const int s = b;
            b = c;
            c = s;
        }
        if constexpr (VCOL) {
            if (shading != 1) {
                const uint32_t rgb = vertex_colour(colors, a, b, c, b1, b2);
                r = float(rgb & 255u);
                g = float((rgb >> 8) & 255u);
                bl = float((rgb >> 16) & 255u);
            }
        } else if (shading != 1 && tex && uvs) {
            const float u = rm_interp(b0, b1, b2, uvs[2 * a], uvs[2 * b], uvs[2 * c]);
            const float v = rm_interp(b0, b1, b2, uvs[2 * a + 1], uvs[2 * b + 1], uvs[2 * c + 1]);
            const uint32_t rgb = fetch_texel(tex, u, v, tex_w, tex_h);
            r = float(rgb & 255u);
            g = float((rgb >> 8) & 255u);
            bl = float((rgb >> 16) & 255u);
        }
        px = make_float4(r / 255.0f, g / 255.0f, bl / 255.0f, float(rm_depth_u8(rm_key_z(best))) / 255.0f);
    }
    // np.flip(axis=1): GL row j (bottom-up) is image row 255 - j (render3d.py:177)
    reinterpret_cast<float4*>(out)[(size_t(view) * RM_SIZE + (RM_SIZE - 1 - j)) * RM_SIZE + i] = px;
}

// ---- multisampling (mvlm_set_render_multisamples) ------------------------------------------------------------------------
// S samples per pixel at fixed points, in 1/16 pixel from the pixel's lower-left corner (window coordinates, y up).  Coverage,
// depth (the plane through vertex 0 at the sample point) and the depth test are per sample, with the tie rule of the pixel
// centres; a sample's key is the one-sample key, (depth bits << 32) | ~id, in a plane of S keys per pixel.  The colour is
// evaluated once per pixel and winning triangle, at the pixel centre (extrapolated where the centre lies outside the
// triangle); the resolve averages the colour bytes pairwise, rounding up (ms_resolve), and keeps sample 0's depth.  What the OpenGL of
// tests/golden/gl_raster_msaa4.npz does; tests/native/msaa_raster.c is the CPU model.  The kernels are
// templated on S: another sample count is one more ms_pattern specialisation.
template <int S>
struct ms_pattern;
template <>
struct ms_pattern<4> {  // (3, 6) (13, 10) (6, 13) (10, 3): the rotated grid, ordered as the resolve pairs them
    __host__ __device__ static constexpr int x(int s) { return s == 0 ? 3 : s == 1 ? 13 : s == 2 ? 6 : 10; }
    __host__ __device__ static constexpr int y(int s) { return s == 0 ? 6 : s == 1 ? 10 : s == 2 ? 13 : 3; }
};
// a sample's offset from the pixel centre, in 1/256 pixel (the vertex lattice), and the extremes over the pattern
template <int S>
__host__ __device__ constexpr int ms_ox(int s) { return 16 * ms_pattern<S>::x(s) - RM_HALF; }
template <int S>
__host__ __device__ constexpr int ms_oy(int s) { return 16 * ms_pattern<S>::y(s) - RM_HALF; }
template <int S, bool X, bool MAX>
__host__ __device__ constexpr int ms_extreme() {
    int m = X ? ms_ox<S>(0) : ms_oy<S>(0);
    for (int s = 1; s < S; ++s) {
        const int o = X ? ms_ox<S>(s) : ms_oy<S>(s);
        m = (MAX ? o > m : o < m) ? o : m;
    }
    return m;
}

// Pixels that have a sample point inside [minx, maxx] x [miny, maxy] (the hull over the samples: pixel i's sample s lies at
// 256 i + 128 + ox(s)), clipped to the window.  This replaces the pixel-centre box in classify and in the binning.
template <int S>
__device__ inline void ms_box(int32_t minx, int32_t maxx, int32_t miny, int32_t maxy, int32_t* ix0, int32_t* ix1, int32_t* iy0,
                              int32_t* iy1) {
    // ceil / floor of a division by 256 as arithmetic shifts
    *ix0 = max((minx - RM_HALF - ms_extreme<S, true, true>() + RM_SUB - 1) >> 8, 0);
    *ix1 = min((maxx - RM_HALF - ms_extreme<S, true, false>()) >> 8, RM_SIZE - 1);
    *iy0 = max((miny - RM_HALF - ms_extreme<S, false, true>() + RM_SUB - 1) >> 8, 0);
    *iy1 = min((maxy - RM_HALF - ms_extreme<S, false, false>()) >> 8, RM_SIZE - 1);
}

// A triangle set up for the sample tests: rm_tri with the sample box in ix0..iy1, valid = 0 (zero area or no pixel),
// 1 (64-bit edge functions) or 2 (small extent: 24-bit ones, below).
template <int S>
__device__ inline rm_tri ms_setup(rm_vert a, rm_vert b, rm_vert c) {
    const bool small = small_extent(a, b, c);
    int64_t area = small ? int64_t(__mul24(b.X - a.X, c.Y - a.Y) - __mul24(b.Y - a.Y, c.X - a.X))
                         : int64_t(b.X - a.X) * (c.Y - a.Y) - int64_t(b.Y - a.Y) * (c.X - a.X);
    rm_tri t;
    t.swapped = 0;
    if (area < 0) {
        const rm_vert s = b;
        b = c;
        c = s;
        area = -area;
        t.swapped = 1;
    }
    t.X0 = a.X; t.Y0 = a.Y; t.X1 = b.X; t.Y1 = b.Y; t.X2 = c.X; t.Y2 = c.Y;
    t.z0 = a.z; t.z1 = b.z; t.z2 = c.z;
    t.farea = float(area);
    ms_box<S>(min(a.X, min(b.X, c.X)), max(a.X, max(b.X, c.X)), min(a.Y, min(b.Y, c.Y)), max(a.Y, max(b.Y, c.Y)), &t.ix0, &t.ix1,
              &t.iy0, &t.iy1);
    t.valid = area == 0 || t.ix0 > t.ix1 || t.iy0 > t.iy1 ? 0 : (small ? 2 : 1);
    return t;
}

// Coverage and depth of the S samples of pixel (i, j): bit s set when sample s is inside (tie rule of the pixel centres) and
// its depth inside the clip range, z[s] that depth.  Each edge function is evaluated once, at the pixel centre; a sample's
// value is that plus dx * oy - dy * ox for its constant offset (ox, oy) - the same integer as at the sample point itself.
// I = int32_t for a triangle of small extent: a pixel of the sample box has its centre within 2^14 + 128 steps of every vertex
// (the samples lie at most 128 steps from the centre), so the products keep 24-bit operands and every value stays below
// 2^30 - RM_SMALL_EXTENT's argument with the half pixel added.
template <int S, typename I>
__device__ inline unsigned ms_cover(const rm_tri* t, int i, int j, float* z) {
    const int32_t px = i * RM_SUB + RM_HALF, py = j * RM_SUB + RM_HALF;
    const int32_t ex[3] = {t->X2 - t->X1, t->X0 - t->X2, t->X1 - t->X0};
    const int32_t ey[3] = {t->Y2 - t->Y1, t->Y0 - t->Y2, t->Y1 - t->Y0};
    const int32_t ax[3] = {t->X1, t->X2, t->X0}, ay[3] = {t->Y1, t->Y2, t->Y0};
    I c[3];
    bool own[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if constexpr (sizeof(I) == 4)
            c[e] = __mul24(ex[e], py - ay[e]) - __mul24(ey[e], px - ax[e]);
        else
            c[e] = I(ex[e]) * (py - ay[e]) - I(ey[e]) * (px - ax[e]);
        own[e] = RM_OWNS(ex[e], ey[e]);
    }
    unsigned mask = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        bool in = true;
        I w[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            w[e] = c[e] + (I(ex[e]) * ms_oy<S>(s) - I(ey[e]) * ms_ox<S>(s));
            in = in && (w[e] > 0 || (w[e] == 0 && own[e]));
        }
        if (!in) continue;
        const float zs = rm_interp(0.f, float(w[1]) / t->farea, float(w[2]) / t->farea, t->z0, t->z1, t->z2);
        if (!(zs >= 0.0f && zs <= 1.0f)) continue;  // near / far clip (render3d.py:136)
        z[s] = zs;
        mask |= 1u << s;
    }
    return mask;
}

// The colour of triangle t at pixel (i, j) under multisampling: evaluated once per pixel at the pixel centre, with the
// centre's barycentric weights even where the centre lies outside the triangle (no inside test); r | g << 8 | b << 16.
// VCOL: the interpolated (there: extrapolated, hence rm_color_u8's clamp) vertex colour instead of a texel.
template <bool VCOL>
__device__ inline uint32_t ms_shade(const vert12* __restrict__ tvv, const int32_t* __restrict__ tris, const float* __restrict__ uvs,
                                    const uint8_t* __restrict__ tex, int tex_w, int tex_h, const uchar4* __restrict__ colors,
                                    int shading, int t, int i, int j) {
    int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    rm_vert va = load_vert(tvv, a), vb = load_vert(tvv, b), vc = load_vert(tvv, c);
    const bool small = small_extent(va, vb, vc);
    int64_t area = small ? int64_t(__mul24(vb.X - va.X, vc.Y - va.Y) - __mul24(vb.Y - va.Y, vc.X - va.X))
                         : int64_t(vb.X - va.X) * (vc.Y - va.Y) - int64_t(vb.Y - va.Y) * (vc.X - va.X);
    if (area < 0) {
        const rm_vert s = vb;
        vb = vc;
        vc = s;
        const int k = b;
        b = c;
        c = k;
        area = -area;
    }
    if (shading == 1) {
        rm_tri g = {};
        g.X0 = va.X; g.Y0 = va.Y; g.X1 = vb.X; g.Y1 = vb.Y; g.X2 = vc.X; g.Y2 = vc.Y;
        g.z0 = va.z; g.z1 = vb.z; g.z2 = vc.z;
        const uint32_t q = uint32_t(rm_geometry_u8(&g));
        return q | (q << 8) | (q << 16);
    }
    if constexpr (!VCOL)
        if (!tex || !uvs) return 0xFFFFFFu;
    const int32_t px = i * RM_SUB + RM_HALF, py = j * RM_SUB + RM_HALF;
    int64_t w1, w2;  // edges 2 -> 0 and 0 -> 1 at the centre (the winner has a sample in this pixel: 24-bit bound as in ms_cover)
    if (small) {
        w1 = __mul24(va.X - vc.X, py - vc.Y) - __mul24(va.Y - vc.Y, px - vc.X);
        w2 = __mul24(vb.X - va.X, py - va.Y) - __mul24(vb.Y - va.Y, px - va.X);
    } else {
        w1 = int64_t(va.X - vc.X) * (py - vc.Y) - int64_t(va.Y - vc.Y) * (px - vc.X);
        w2 = int64_t(vb.X - va.X) * (py - va.Y) - int64_t(vb.Y - va.Y) * (px - va.X);
    }
    const float farea = float(area), b1 = float(w1) / farea, b2 = float(w2) / farea;
    if constexpr (VCOL) {
        return vertex_colour(colors, a, b, c, b1, b2);
    } else {
        const float u = rm_interp(0.f, b1, b2, uvs[2 * a], uvs[2 * b], uvs[2 * c]);
        const float v = rm_interp(0.f, b1, b2, uvs[2 * a + 1], uvs[2 * b + 1], uvs[2 * c + 1]);
        return fetch_texel(tex, u, v, tex_w, tex_h);
    }
}

// The GL's resolve of one colour byte: the rounding-up average of samples 0 and 1, of 2 and 3, then of the two - not
// (sum + 2) >> 2, from which it differs in 3 of 4 random cases
template <int S>
__device__ inline unsigned ms_resolve(const uint32_t* rgb, int shift) {
    static_assert(S == 4, "the pairing of another sample count is not known");
    const unsigned a = (((rgb[0] >> shift) & 255u) + ((rgb[1] >> shift) & 255u) + 1u) >> 1;
    const unsigned b = (((rgb[2] >> shift) & 255u) + ((rgb[3] >> shift) & 255u) + 1u) >> 1;
    return (a + b + 1u) >> 1;
}

// tile_body with S keys per pixel: the pixel's keys are contiguous (32 bytes at S = 4: two 16-byte loads), handed back
// EMPTY like the one-sample plane; the colour is shaded once per distinct winning triangle (one texel fetch - or, VCOL, three
// colour loads - for the usual pixel, up to S on silhouettes and sub-pixel triangles) and resolved with the GL's rounding.
template <int S, bool VCOL>
__device__ __forceinline__ void tile_ms_body(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                             const float* __restrict__ uvs, const uint8_t* __restrict__ tex, int tex_w, int tex_h,
                                             const uchar4* __restrict__ colors, int n_verts, const int* __restrict__ counts,
                                             const int* __restrict__ offsets, const int* __restrict__ bins, int cap,
                                             unsigned long long* __restrict__ keys, int shading, int n_views,
                                             const int* __restrict__ overflow, int* __restrict__ overflow_host,
                                             float* __restrict__ out) {
    static_assert(S == 4, "the key loads below read a pixel's keys as two 16-byte words");
    __shared__ rm_tri s_tri[256];
    __shared__ int s_id[256];
    int view, tile;
    if (!view_chunk(TILES, n_views, &view, &tile)) return;
    const int tid = threadIdx.x;
    const auto [x0, y0, i, j, tvv, n, list] = tile_prologue<int>(view, tile, RM_TILES, tv, n_verts, counts, offsets, bins, cap);

    ulonglong2* const key_slot = reinterpret_cast<ulonglong2*>(keys + ((size_t(view) * RM_SIZE + j) * RM_SIZE + i) * S);
    const ulonglong2 k01 = key_slot[0], k23 = key_slot[1];
    uint64_t best[S] = {k01.x, k01.y, k23.x, k23.y};  // what the small triangles left
    if ((k01.x & k01.y) != RM_KEY_EMPTY) key_slot[0] = make_ulonglong2(RM_KEY_EMPTY, RM_KEY_EMPTY);
    if ((k23.x & k23.y) != RM_KEY_EMPTY) key_slot[1] = make_ulonglong2(RM_KEY_EMPTY, RM_KEY_EMPTY);
    publish_overflow(overflow, overflow_host);

    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if (tid < m) {
            const int t = list[base + tid];
            s_id[tid] = t;
            s_tri[tid] = ms_setup<S>(load_vert(tvv, tris[3 * t]), load_vert(tvv, tris[3 * t + 1]), load_vert(tvv, tris[3 * t + 2]));
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const rm_tri* t = &s_tri[k];
            if (!t->valid || i < t->ix0 || i > t->ix1 || j < t->iy0 || j > t->iy1) continue;
            float z[S];
            const unsigned cov = t->valid == 2 ? ms_cover<S, int32_t>(t, i, j, z) : ms_cover<S, int64_t>(t, i, j, z);
            if (!cov) continue;
            const uint32_t id = uint32_t(s_id[k]);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (cov & (1u << s)) {
                    const uint64_t key = rm_key(z[s], id);
                    best[s] = key < best[s] ? key : best[s];
                }
        }
    }

    // shade each distinct winner once, resolve
    int win[S];
    uint32_t rgb[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        win[s] = best[s] == RM_KEY_EMPTY ? -1 : int(rm_key_tri(best[s]));
        rgb[s] = 0xFFFFFFu;  // an uncovered sample is the white background
        bool seen = false;
#pragma unroll
        for (int q = 0; q < s; ++q)
            if (!seen && win[q] == win[s]) {
                rgb[s] = rgb[q];
                seen = true;
            }
        if (!seen && win[s] >= 0) rgb[s] = ms_shade<VCOL>(tvv, tris, uvs, tex, tex_w, tex_h, colors, shading, win[s], i, j);
    }
    const float z0 = best[0] == RM_KEY_EMPTY ? 1.0f : rm_key_z(best[0]);  // the resolved depth: sample 0's
    const float4 px = make_float4(float(ms_resolve<S>(rgb, 0)) / 255.0f, float(ms_resolve<S>(rgb, 8)) / 255.0f,
                                  float(ms_resolve<S>(rgb, 16)) / 255.0f, float(rm_depth_u8(z0)) / 255.0f);
    reinterpret_cast<float4*>(out)[(size_t(view) * RM_SIZE + (RM_SIZE - 1 - j)) * RM_SIZE + i] = px;
}

}  // namespace

#endif
