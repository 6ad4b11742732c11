// Pieces of the multi-view rasteriser shared by its one-sample kernels (raster.hip), its multisampled ones (raster_ms.hip)
// and the per-vertex-colour tile kernels (raster_vc.hip) - the latter two objects of their own: tools/kernel_occupancy.py
// keeps a table of each one's kernels beside the main one.  The tile stage's bodies: raster_tile.h; the binning front end: raster_bins.h.
#ifndef MVLM_RASTER_COMMON_H
#define MVLM_RASTER_COMMON_H

#include "common.h"
#include "raster_math.h"

namespace {

constexpr int TILES = RM_TILES * RM_TILES;  // 256 per view

// Workgroup -> (view, chunk of that view's work) so that every view is worked on by ONE XCD: consecutive block ids
// go round-robin over the 8 XCDs, each with its own L2; a view's transformed vertices (0.8 MB), key plane (0.5 MB) and
// bins then live in one L2 instead of being fetched by all eight (speed heuristic only: any placement is correct).
// The grid holds ceil(n_views / 8) * 8 * chunks_per_view workgroups; surplus ones return at once.
__device__ inline bool view_chunk(int chunks_per_view, int n_views, int* view, int* chunk) {
    const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
    *view = (j / chunks_per_view) * 8 + xcd;
    *chunk = j % chunks_per_view;
    return *view < n_views;
}
inline unsigned view_chunk_grid(int chunks_per_view, int n_views) { return unsigned((n_views + 7) / 8 * 8) * unsigned(chunks_per_view); }

// a transformed vertex as stored (rm_vert without its padding word: a quarter less traffic on the largest scratch array)
struct vert12 {
    int32_t X, Y;
    float z;
};
__device__ inline rm_vert load_vert(const vert12* __restrict__ p, int i) {
    const vert12 v = p[i];
    rm_vert o;
    o.X = v.X;
    o.Y = v.Y;
    o.z = v.z;
    o.pad = 0.f;
    return o;
}

// a triangle whose vertices lie within 2^14 steps of each other takes the 24-bit edge functions (raster.hip, "24-bit path")
constexpr int RM_SMALL_EXTENT = 1 << 14;

__device__ inline bool small_extent(const rm_vert& a, const rm_vert& b, const rm_vert& c) {
    const int32_t minx = min(a.X, min(b.X, c.X)), maxx = max(a.X, max(b.X, c.X));
    const int32_t miny = min(a.Y, min(b.Y, c.Y)), maxy = max(a.Y, max(b.Y, c.Y));
    return maxx - minx < RM_SMALL_EXTENT && maxy - miny < RM_SMALL_EXTENT;
}

// A per-vertex colour attribute at the pixel: the three vertices' colours (one aligned 4-byte load each, u8[V,4] on the
// device) through rm_interp per channel, then rm_color_u8; r | g << 8 | b << 16.  b and c are the indices AFTER the winding
// swap, b1 and b2 the weights of those vertices.
__device__ inline uint32_t vertex_colour(const uchar4* __restrict__ colors, int a, int b, int c, float b1, float b2) {
    const uchar4 c0 = colors[a], c1 = colors[b], c2 = colors[c];
    const int r = rm_color_u8(rm_interp(0.f, b1, b2, float(c0.x) / 255.0f, float(c1.x) / 255.0f, float(c2.x) / 255.0f));
    const int g = rm_color_u8(rm_interp(0.f, b1, b2, float(c0.y) / 255.0f, float(c1.y) / 255.0f, float(c2.y) / 255.0f));
    const int bl = rm_color_u8(rm_interp(0.f, b1, b2, float(c0.z) / 255.0f, float(c1.z) / 255.0f, float(c2.z) / 255.0f));
    return uint32_t(r) | (uint32_t(g) << 8) | (uint32_t(bl) << 16);
}

// The nearest texel of (u, v), r | g << 8 | b << 16, with one (unaligned) 4-byte load: the buffer carries 4 spare bytes behind
// the last texel (api.hip).
__device__ inline uint32_t fetch_texel(const uint8_t* __restrict__ tex, float u, float v, int tex_w, int tex_h) {
    uint32_t rgb;
    __builtin_memcpy(&rgb, tex + size_t(rm_texel(u, v, tex_w, tex_h)) * 3, 4);
    return rgb & 0xFFFFFFu;
}

constexpr int SMALL_PIXELS = 16;  // triangles covering at most this many pixel centres skip the bins
constexpr int FILL_WGS = 32;      // bin-fill workgroups per view (raster.hip, bin_fill_kernel)

}  // namespace

#include "raster_bins.h"  // the binning front end, shared by every launch set

// The multisampled kernels of one mvlm_render at `samples` samples per pixel (raster_ms.hip); raster.hip launches the
// transform before and the scan between them.  `tv` is the transformed-vertex scratch (vert12[n_views][n_verts]).
// `colors` (u8[V,4] on the device, or null): the tile stage is raster_vc_tile's, shading with the per-vertex colours.
void raster_ms_classify(hipStream_t stream, int samples, const void* tv, const int32_t* tris, int n_verts, int n_tris,
                        int n_views, unsigned long long* keys, const raster_bins& b);
void raster_ms_bin_and_tile(hipStream_t stream, int samples, const void* tv, const int32_t* tris, const float* uvs,
                            const uint8_t* tex, int tex_w, int tex_h, int n_verts, int n_tris, int n_views, const raster_bins& b,
                            unsigned long long* keys, int shading, int* overflow_host, float* out, const uint8_t* colors);
// The tile stage with per-vertex colours (raster_vc.hip), at `samples` = 0 (one sample, in place of raster.hip's tile_kernel)
// or 4 (in place of tile_ms_kernel, behind raster_ms.hip's bin fill).
void raster_vc_tile(hipStream_t stream, int samples, const void* tv, const int32_t* tris, const uint8_t* colors, int n_verts,
                    int n_views, const raster_bins& b, unsigned long long* keys, int shading, int* overflow_host, float* out);
// The two kernels of a point mesh's render (raster_points.hip): splats into `keys`, then the tile stage, which hands the key plane
// back EMPTY.  `rot` f64[n_views,9] on the device; R / c: the mesh's radius in lattice steps and its depth coefficient
// (raster_points_math.h); `colors` u8[n_points,4] on the device or null (white); `stats` null, or two device counters the splat
// kernel's measuring form adds to (covered pixels, atomics issued); `between`: null, or an event to record between the two kernels.
void raster_points_launch(hipStream_t stream, const float* verts, const uint8_t* colors, int n_points, const double* rot,
                          int n_views, int sub_bits, int R, float c, unsigned long long* keys, unsigned long long* stats,
                          int* overflow_host, float* out, hipEvent_t between);
// The first of those two kernels alone, for a render whose tile stage is another one (cloud_normals.hip).
void raster_points_splat_launch(hipStream_t stream, const float* verts, int n_points, const double* rot, int n_views, int sub_bits,
                                int R, float c, unsigned long long* keys, unsigned long long* stats);
// The tile stage of a cloud's geometry-shaded render (cloud_normals.hip): key, EMPTY hand-back, depth byte, flip and overflow word as
// the points' tile kernel, planes 0..2 the two-sided shade of the winner's normal (cloud_normals_math.h); `normals` f32[n_points,3].
void cloud_normals_tile_launch(hipStream_t stream, const float* normals, const double* rot, int n_views, unsigned long long* keys,
                               int* overflow_host, float* out);

#endif
