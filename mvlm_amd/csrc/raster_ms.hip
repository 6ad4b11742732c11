// Multisampled rendering (mvlm_set_render_multisamples): the classify, bin-fill and tile kernels at S samples per pixel.
// mvlm_render (raster.hip) runs them in place of its one-sample ones, around the same transform and scan kernels and on the
// same counters, offsets and bins; the key plane is a scratch entry of its own.  Built as an object of its own.
#include "raster_common.h"

namespace {

// ---- multisampling (mvlm_set_render_multisamples) ------------------------------------------------------------------------
// S samples per pixel at fixed points, in 1/16 pixel from the pixel's lower-left corner (window coordinates, y up).  Coverage,
// depth (the plane through vertex 0 at the sample point) and the depth test are per sample, with the tie rule of the pixel
// centres; a sample's key is the one-sample key, (depth bits << 32) | ~id, in a plane of S keys per pixel.  The colour is
// evaluated once per pixel and winning triangle, at the pixel centre (extrapolated where the centre lies outside the
// triangle); the resolve averages the colour bytes pairwise, rounding up (ms_resolve), and keeps sample 0's depth.  What the OpenGL of
// tests/golden/gl_raster_msaa4.npz does; tests/native/msaa_raster.c is the CPU model.  The kernels below are
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

template <int S>
__device__ inline bool classify_ms_one(int view, int t, const rm_vert& va, const rm_vert& vb, const rm_vert& vc,
                                       unsigned long long* __restrict__ keys, int* __restrict__ counts) {
    const int32_t minx = min(va.X, min(vb.X, vc.X)), maxx = max(va.X, max(vb.X, vc.X));
    const int32_t miny = min(va.Y, min(vb.Y, vc.Y)), maxy = max(va.Y, max(vb.Y, vc.Y));
    int32_t ix0, ix1, iy0, iy1;
    ms_box<S>(minx, maxx, miny, maxy, &ix0, &ix1, &iy0, &iy1);
    if (ix0 > ix1 || iy0 > iy1) return false;
    if ((ix1 - ix0 + 1) * (iy1 - iy0 + 1) <= SMALL_PIXELS) {
        const rm_tri tr = ms_setup<S>(va, vb, vc);
        if (!tr.valid) return false;
        unsigned long long* kv = keys + size_t(view) * RM_SIZE * RM_SIZE * S;
        for (int j = iy0; j <= iy1; ++j)
            for (int ii = ix0; ii <= ix1; ++ii) {
                float z[S];
                const unsigned m = tr.valid == 2 ? ms_cover<S, int32_t>(&tr, ii, j, z) : ms_cover<S, int64_t>(&tr, ii, j, z);
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (m & (1u << s)) atomicMin(&kv[(j * RM_SIZE + ii) * S + s], (unsigned long long)rm_key(z[s], uint32_t(t)));
            }
        return false;
    }
    if (maxx - minx < RM_SMALL_EXTENT && maxy - miny < RM_SMALL_EXTENT) {
        if (__mul24(vb.X - va.X, vc.Y - va.Y) == __mul24(vb.Y - va.Y, vc.X - va.X)) return false;
    } else if (int64_t(vb.X - va.X) * (vc.Y - va.Y) == int64_t(vb.Y - va.Y) * (vc.X - va.X)) {
        return false;
    }
    for (int ty = iy0 / RM_TILE; ty <= iy1 / RM_TILE; ++ty)
        for (int tx = ix0 / RM_TILE; tx <= ix1 / RM_TILE; ++tx) atomicAdd(&counts[view * TILES + ty * RM_TILES + tx], 1);
    return true;
}

// classify_kernel<1> with the sample box and a key per sample
template <int S>
__global__ __launch_bounds__(256) void classify_ms_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris, int n_verts,
                                                          int n_tris, int n_views, unsigned long long* __restrict__ keys,
                                                          int* __restrict__ counts, int* __restrict__ n_big, int* __restrict__ big_list) {
    int view, chunk;
    if (!view_chunk((n_tris + 255) / 256, n_views, &view, &chunk)) return;
    const vert12* const tvv = tv + size_t(view) * n_verts;
    const int t = chunk * 256 + int(threadIdx.x);
    const int tt = t < n_tris ? t : 0;
    const rm_vert va = load_vert(tvv, tris[3 * tt]), vb = load_vert(tvv, tris[3 * tt + 1]), vc = load_vert(tvv, tris[3 * tt + 2]);
    const int lane = int(threadIdx.x) & 63;
    const bool big = t < n_tris && classify_ms_one<S>(view, t, va, vb, vc, keys, counts);
    const unsigned long long m = __ballot(big);
    if (m) {  // (wave-uniform)
        const int leader = __ffsll(static_cast<long long>(m)) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&n_big[view], __popcll(m));
        base = __shfl(base, leader);
        if (big) big_list[size_t(view) * n_tris + base + __popcll(m & ((1ull << lane) - 1ull))] = t;
    }
}

// bin_fill_kernel with the tiles of the sample box
template <int S>
__global__ void bin_fill_ms_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris, int n_verts, int n_tris,
                                   int n_views, const int* __restrict__ n_big, const int* __restrict__ big_list,
                                   const int* __restrict__ offsets, int* __restrict__ cursors, int* __restrict__ bins, int cap,
                                   int* __restrict__ overflow) {
    int view, wg;
    if (!view_chunk(FILL_WGS, n_views, &view, &wg)) return;
    const int n = n_big[view];
    const vert12* const tvv = tv + size_t(view) * n_verts;
    for (int k = wg * 256 + int(threadIdx.x); k < n; k += FILL_WGS * 256) {
        const int t = big_list[size_t(view) * n_tris + k];
        const rm_vert a = load_vert(tvv, tris[3 * t]), b = load_vert(tvv, tris[3 * t + 1]), c = load_vert(tvv, tris[3 * t + 2]);
        int32_t ix0, ix1, iy0, iy1;
        ms_box<S>(min(a.X, min(b.X, c.X)), max(a.X, max(b.X, c.X)), min(a.Y, min(b.Y, c.Y)), max(a.Y, max(b.Y, c.Y)), &ix0, &ix1,
                  &iy0, &iy1);
        for (int ty = iy0 / RM_TILE; ty <= iy1 / RM_TILE; ++ty)
            for (int tx = ix0 / RM_TILE; tx <= ix1 / RM_TILE; ++tx) {
                const int tile = view * TILES + ty * RM_TILES + tx;
                const int pos = offsets[tile] + atomicAdd(&cursors[tile], 1);
                if (pos < cap)
                    bins[size_t(view) * cap + pos] = t;
                else
                    *overflow = 1;
            }
    }
}

// The colour of triangle t at pixel (i, j) under multisampling: evaluated once per pixel at the pixel centre, with the
// centre's barycentric weights even where the centre lies outside the triangle (no inside test); r | g << 8 | b << 16.
__device__ inline uint32_t ms_shade(const vert12* __restrict__ tvv, const int32_t* __restrict__ tris, const float* __restrict__ uvs,
                                    const uint8_t* __restrict__ tex, int tex_w, int tex_h, int shading, int t, int i, int j) {
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
    const float u = rm_interp(0.f, b1, b2, uvs[2 * a], uvs[2 * b], uvs[2 * c]);
    const float v = rm_interp(0.f, b1, b2, uvs[2 * a + 1], uvs[2 * b + 1], uvs[2 * c + 1]);
    uint32_t rgb;  // (the buffer carries 4 spare bytes behind the last texel, api.hip)
    __builtin_memcpy(&rgb, tex + size_t(rm_texel(u, v, tex_w, tex_h)) * 3, 4);
    return rgb & 0xFFFFFFu;
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

// tile_kernel with S keys per pixel: the pixel's keys are contiguous (32 bytes at S = 4: two 16-byte loads), handed back
// EMPTY like the one-sample plane; the colour is shaded once per distinct winning triangle (one texel fetch for the usual
// pixel, up to S on silhouettes and sub-pixel triangles) and resolved with the GL's rounding.
template <int S>
__global__ __launch_bounds__(256) void tile_ms_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                                      const float* __restrict__ uvs, const uint8_t* __restrict__ tex,
                                                      int tex_w, int tex_h, int n_verts, const int* __restrict__ counts,
                                                      const int* __restrict__ offsets, const int* __restrict__ bins,
                                                      int cap, unsigned long long* __restrict__ keys,
                                                      int shading, int n_views, const int* __restrict__ overflow,
                                                      int* __restrict__ overflow_host, float* __restrict__ out) {
    static_assert(S == 4, "the key loads below read a pixel's keys as two 16-byte words");
    __shared__ rm_tri s_tri[256];
    __shared__ int s_id[256];
    int view, tile;
    if (!view_chunk(TILES, n_views, &view, &tile)) return;
    const int vt = view * TILES + tile;
    const int tid = threadIdx.x;
    const int i = (tile % RM_TILES) * RM_TILE + (tid & (RM_TILE - 1));
    const int j = (tile / RM_TILES) * RM_TILE + (tid >> 4);
    const vert12* const tvv = tv + size_t(view) * n_verts;
    const int n = min(counts[vt], cap - offsets[vt]);
    const int* const list = bins + size_t(view) * cap + offsets[vt];

    ulonglong2* const key_slot = reinterpret_cast<ulonglong2*>(keys + ((size_t(view) * RM_SIZE + j) * RM_SIZE + i) * S);
    const ulonglong2 k01 = key_slot[0], k23 = key_slot[1];
    uint64_t best[S] = {k01.x, k01.y, k23.x, k23.y};  // what the small triangles left
    if ((k01.x & k01.y) != RM_KEY_EMPTY) key_slot[0] = make_ulonglong2(RM_KEY_EMPTY, RM_KEY_EMPTY);
    if ((k23.x & k23.y) != RM_KEY_EMPTY) key_slot[1] = make_ulonglong2(RM_KEY_EMPTY, RM_KEY_EMPTY);
    if (blockIdx.x == 0 && tid == 0) {
        __atomic_store_n(overflow_host, *overflow, __ATOMIC_RELAXED);
        __threadfence_system();
    }

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
        if (!seen && win[s] >= 0) rgb[s] = ms_shade(tvv, tris, uvs, tex, tex_w, tex_h, shading, win[s], i, j);
    }
    const float z0 = best[0] == RM_KEY_EMPTY ? 1.0f : rm_key_z(best[0]);  // the resolved depth: sample 0's
    const float4 px = make_float4(float(ms_resolve<S>(rgb, 0)) / 255.0f, float(ms_resolve<S>(rgb, 8)) / 255.0f,
                                  float(ms_resolve<S>(rgb, 16)) / 255.0f, float(rm_depth_u8(z0)) / 255.0f);
    reinterpret_cast<float4*>(out)[(size_t(view) * RM_SIZE + (RM_SIZE - 1 - j)) * RM_SIZE + i] = px;
}

}  // namespace

void raster_ms_classify(hipStream_t stream, int samples, const void* tv, const int32_t* tris, int n_verts, int n_tris,
                        int n_views, unsigned long long* keys, int* counts, int* n_big, int* big_list) {
    (void)samples;  // 4: the one sample count mvlm_set_render_multisamples admits
    hipLaunchKernelGGL(classify_ms_kernel<4>, dim3(view_chunk_grid((n_tris + 255) / 256, n_views)), dim3(256), 0, stream,
                       static_cast<const vert12*>(tv), tris, n_verts, n_tris, n_views, keys, counts, n_big, big_list);
}

void raster_ms_bin_and_tile(hipStream_t stream, int samples, const void* tv, const int32_t* tris, const float* uvs,
                            const uint8_t* tex, int tex_w, int tex_h, int n_verts, int n_tris, int n_views, const int* n_big,
                            const int* big_list, const int* counts, const int* offsets, int* cursors, int* bins, int cap,
                            unsigned long long* keys, int shading, int* overflow, int* overflow_host, float* out) {
    (void)samples;
    const vert12* const v = static_cast<const vert12*>(tv);
    hipLaunchKernelGGL(bin_fill_ms_kernel<4>, dim3(view_chunk_grid(FILL_WGS, n_views)), dim3(256), 0, stream, v, tris, n_verts,
                       n_tris, n_views, n_big, big_list, offsets, cursors, bins, cap, overflow);
    hipLaunchKernelGGL(tile_ms_kernel<4>, dim3(view_chunk_grid(TILES, n_views)), dim3(256), 0, stream, v, tris, uvs, tex, tex_w,
                       tex_h, n_verts, counts, offsets, bins, cap, keys, shading, n_views, overflow, overflow_host, out);
}
