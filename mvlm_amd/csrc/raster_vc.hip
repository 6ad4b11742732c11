// Per-vertex colours (mvlm_mesh_upload_colors): the tile kernels at one and at four samples per pixel whose unlit shade is the
// winning triangle's interpolated vertex colour instead of a texel - the VCOL forms of raster_tile.h's bodies.  mvlm_render
// (raster.hip) launches them in place of tile_kernel / tile_ms_kernel when the mesh carries colours, has no usable texture and
// the shading is the unlit one ("Per-vertex colours"); everything before the tile stage is shared.  A mesh
// with a texture AND colours renders with its texture alone: the texel x colour product VTK would form is not built.
// Built as an object of its own (build/vcolor/, tests/golden/kernel_occupancy_vcolor.json).
#include "raster_tile.h"

namespace {

__global__ __launch_bounds__(256) void tile_vc_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                                      const uchar4* __restrict__ colors, int n_verts,
                                                      const int* __restrict__ counts, const int* __restrict__ offsets,
                                                      const int* __restrict__ bins, int cap, unsigned long long* __restrict__ keys,
                                                      int shading, int n_views, const int* __restrict__ overflow,
                                                      int* __restrict__ overflow_host, float* __restrict__ out) {
    tile_body<true>(tv, tris, nullptr, nullptr, 0, 0, colors, n_verts, counts, offsets, bins, cap, keys, shading, n_views, overflow,
                    overflow_host, out);
}

template <int S>
__global__ __launch_bounds__(256) void tile_vc_ms_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                                         const uchar4* __restrict__ colors, int n_verts,
                                                         const int* __restrict__ counts, const int* __restrict__ offsets,
                                                         const int* __restrict__ bins, int cap,
                                                         unsigned long long* __restrict__ keys, int shading, int n_views,
                                                         const int* __restrict__ overflow, int* __restrict__ overflow_host,
                                                         float* __restrict__ out) {
    tile_ms_body<S, true>(tv, tris, nullptr, nullptr, 0, 0, colors, n_verts, counts, offsets, bins, cap, keys, shading, n_views,
                          overflow, overflow_host, out);
}

}  // namespace

void raster_vc_tile(hipStream_t stream, int samples, const void* tv, const int32_t* tris, const uint8_t* colors, int n_verts,
                    int n_views, const raster_bins& b, unsigned long long* keys, int shading, int* overflow_host, float* out) {
    const vert12* const v = static_cast<const vert12*>(tv);
    const uchar4* const col = reinterpret_cast<const uchar4*>(colors);
    if (samples == 0)
        hipLaunchKernelGGL(tile_vc_kernel, dim3(view_chunk_grid(TILES, n_views)), dim3(256), 0, stream, v, tris, col, n_verts, b.counts,
                           b.offsets, b.bins, b.cap, keys, shading, n_views, b.overflow, overflow_host, out);
    else  // 4: the one sample count mvlm_set_render_multisamples admits
        hipLaunchKernelGGL(tile_vc_ms_kernel<4>, dim3(view_chunk_grid(TILES, n_views)), dim3(256), 0, stream, v, tris, col, n_verts,
                           b.counts, b.offsets, b.bins, b.cap, keys, shading, n_views, b.overflow, overflow_host, out);
}
