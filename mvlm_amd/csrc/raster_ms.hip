// Multisampled rendering (mvlm_set_render_multisamples): the classify, bin-fill and tile kernels at S samples per pixel.
// mvlm_render (raster.hip) runs them in place of its one-sample ones, around the same transform and scan kernels and on the
// same counters, offsets and bins; the key plane is a scratch entry of its own.  Built as an object of its own.
#include "raster_tile.h"

namespace {

// (the sample pattern, ms_box, ms_setup and ms_cover, shared with the tile stage: raster_tile.h)
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
        unsigned long long* kv = keys + size_t(view) * RM_SIZE * RM_SIZE * S;  // (S keys per pixel: not resolve_small_box's form)
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
    count_tile_range<int>(counts, view, RM_TILES, ix0, ix1, iy0, iy1);
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
    const bool big = t < n_tris && classify_ms_one<S>(view, t, va, vb, vc, keys, counts);
    append_big(big, t, view, n_tris, n_big, big_list);
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
        scatter_tile_range<int>(view, RM_TILES, offsets, cursors, bins, cap, overflow, ix0, ix1, iy0, iy1, t);
    }
}

// The multisampled tile stage (raster_tile.h: tile_ms_body) without per-vertex colours; raster_vc.hip holds the coloured form.
template <int S>
__global__ __launch_bounds__(256) void tile_ms_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                                      const float* __restrict__ uvs, const uint8_t* __restrict__ tex,
                                                      int tex_w, int tex_h, int n_verts, const int* __restrict__ counts,
                                                      const int* __restrict__ offsets, const int* __restrict__ bins,
                                                      int cap, unsigned long long* __restrict__ keys,
                                                      int shading, int n_views, const int* __restrict__ overflow,
                                                      int* __restrict__ overflow_host, float* __restrict__ out) {
    tile_ms_body<S, false>(tv, tris, uvs, tex, tex_w, tex_h, nullptr, n_verts, counts, offsets, bins, cap, keys, shading, n_views,
                           overflow, overflow_host, out);
}

}  // namespace

void raster_ms_classify(hipStream_t stream, int samples, const void* tv, const int32_t* tris, int n_verts, int n_tris,
                        int n_views, unsigned long long* keys, const raster_bins& b) {
    (void)samples;  // 4: the one sample count mvlm_set_render_multisamples admits
    hipLaunchKernelGGL(classify_ms_kernel<4>, dim3(view_chunk_grid((n_tris + 255) / 256, n_views)), dim3(256), 0, stream,
                       static_cast<const vert12*>(tv), tris, n_verts, n_tris, n_views, keys, b.counts, b.n_big, b.big_list);
}

void raster_ms_bin_and_tile(hipStream_t stream, int samples, const void* tv, const int32_t* tris, const float* uvs,
                            const uint8_t* tex, int tex_w, int tex_h, int n_verts, int n_tris, int n_views, const raster_bins& b,
                            unsigned long long* keys, int shading, int* overflow_host, float* out, const uint8_t* colors) {
    (void)samples;
    const vert12* const v = static_cast<const vert12*>(tv);
    hipLaunchKernelGGL(bin_fill_ms_kernel<4>, dim3(view_chunk_grid(FILL_WGS, n_views)), dim3(256), 0, stream, v, tris, n_verts,
                       n_tris, n_views, b.n_big, b.big_list, b.offsets, b.cursors, b.bins, b.cap, b.overflow);
    if (colors)  // per-vertex colours: the tile stage of raster_vc.hip
        raster_vc_tile(stream, 4, tv, tris, colors, n_verts, n_views, b, keys, shading, overflow_host, out);
    else
        hipLaunchKernelGGL(tile_ms_kernel<4>, dim3(view_chunk_grid(TILES, n_views)), dim3(256), 0, stream, v, tris, uvs, tex, tex_w,
                           tex_h, n_verts, b.counts, b.offsets, b.bins, b.cap, keys, shading, n_views, b.overflow, overflow_host, out);
}
