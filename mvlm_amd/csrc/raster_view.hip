// The landmark view (mvlm_render_landmark_view): the reference's offscreen viewer (utils/viewer.py with save=True - the mesh
// and a sphere at every landmark in one window) as a rasteriser object of its own beside the network's 256 x 256 one.  The
// window has a side S of 64..2048 pixels and a frame per view; the mesh is drawn by the one-sample contract of raster_math.h
// with that window (raster_view_math.h), the spheres analytically, depth-tested against the mesh ("Landmark
// view").  One sample per pixel: the context's multisample setting does not apply here.
//
// Structure as raster.hip, with runtime tile counts ((S / 16)^2, up to 16 384 per view):
//   1. transform   one thread per (view, vertex)
//   2. classify    one thread per (view, triangle): boxes of <= 128 pixel centres (VIEW_SMALL_PIXELS) resolved with the 64-bit atomicMin of the
//                  (depth, id) key, larger ones counted into 16 x 16 tiles and appended to the view's big list, one atomic per wave
//   3. scan        one workgroup per view over its tile counters
//   4. bin fill    big triangles' ids into the per-tile lists
//   5. project     one thread per (view, landmark): window position, depth, radius in pixels, colour, pixel box - 32 bytes
//   6. tile        one workgroup per (view, tile), a thread per pixel: resolves and shades the mesh as tile_body does, then
//                  compacts the spheres whose box touches the tile into an LDS list (ballots, VIEW_SPHERE_CAP candidates a
//                  round, any number of rounds), every pixel walks the list; the winners' pixel counts are summed per tile in
//                  LDS and added to the global counts with one atomic per (tile, landmark) that is non-zero.
// Only the 64-bit edge functions are used (the 24-bit ones of raster_tile.h give the same integers).  The key plane
// ("view.keys", 32 MB per view at S = 2048) is filled inside every call.
// The tile stage's device code and the launch of the stages in front of it are shared with the ray view (raster_rays.hip):
// raster_view_tile.h.
#include "raster_view_tile.h"

namespace {

// A triangle whose pixel-centre box holds at most this many pixels is resolved by classify's atomics, not binned.  Larger than
// raster.hip's 16: the bench mesh's triangles span 5 x 5 pixel centres in a 1024^2 window and 10 x 10 at 2048^2, and with all of
// them binned every pixel of a tile walked ~55 triangles through the 64-bit edge functions - 353 of the view's 450 us at 1024^2
// (profiles/landmark_view_time.txt).  The key makes the image independent of which path a triangle takes.
constexpr int VIEW_SMALL_PIXELS = 128;

// (view_transform_kernel and view_scan_kernel beside raster.hip's transform_kernel and scan_kernel: raster_bins.h says why)
__global__ void view_transform_kernel(const float* __restrict__ verts, int n_verts, const double* __restrict__ rot,
                                      const view_frame* __restrict__ frames, int n_views, int sub_bits,
                                      vert12* __restrict__ tv) {
    int view, chunk;
    if (!view_chunk((n_verts + 255) / 256, n_views, &view, &chunk)) return;
    const int v = chunk * 256 + int(threadIdx.x);
    if (v >= n_verts) return;
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = rot[view * 9 + k];
    const view_frame f = frames[view];
    const rm_vert o = rv_transform(m, verts[3 * v], verts[3 * v + 1], verts[3 * v + 2], sub_bits, f.cx, f.cy, f.half, f.k);
    vert12 w;
    w.X = o.X;
    w.Y = o.Y;
    w.z = o.z;
    tv[size_t(view) * n_verts + v] = w;
}


// cull / resolve small boxes with atomics / count big ones into tiles; true for a big triangle (classify_one of raster.hip)
__device__ inline bool view_classify_one(int view, int t, const rm_vert& va, const rm_vert& vb, const rm_vert& vc, int size,
                                         unsigned long long* __restrict__ keys, int* __restrict__ counts) {
    const rm_tri tr = rv_setup(va, vb, vc, size);
    if (!tr.valid) return false;
    const int w = tr.ix1 - tr.ix0 + 1, h = tr.iy1 - tr.iy0 + 1;
    if (w * h <= VIEW_SMALL_PIXELS) {
        unsigned long long* kv = keys + size_t(view) * size * size;
        resolve_small_box<rm_tri, rm_cover, size_t>(kv, size, tr.ix0, tr.ix1, tr.iy0, tr.iy1, tr, t);
        return false;
    }
    const int tiles_x = size / RM_TILE;
    count_tile_range<size_t>(counts, view, tiles_x, tr.ix0, tr.ix1, tr.iy0, tr.iy1);
    return true;
}

__global__ __launch_bounds__(256) void view_classify_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                                            int n_verts, int n_tris, int n_views, int size,
                                                            unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                                            int* __restrict__ n_big, int* __restrict__ big_list) {
    int view, chunk;
    if (!view_chunk((n_tris + 255) / 256, n_views, &view, &chunk)) return;
    const vert12* const tvv = tv + size_t(view) * n_verts;
    const int t = chunk * 256 + int(threadIdx.x);
    const int tt = t < n_tris ? t : 0;
    const rm_vert va = load_vert(tvv, tris[3 * tt]), vb = load_vert(tvv, tris[3 * tt + 1]), vc = load_vert(tvv, tris[3 * tt + 2]);
    const bool big = t < n_tris && view_classify_one(view, t, va, vb, vc, size, keys, counts);
    append_big(big, t, view, n_tris, n_big, big_list);
}

// exclusive prefix sum over a view's tile counters (up to 16 384): a thread sums its run of `per` counters, the 256 run sums
// are scanned in LDS, the thread writes its run's offsets.  The sums are 64-bit - 16 384 tiles times the triangles of a folded
// or badly scaled mesh that all span the window pass 2^31 - and an offset is stored saturated at `cap`: a list beyond the
// capacity is empty (the tile kernel's min(count, cap - offset)), never in front of the buffer.
__global__ __launch_bounds__(256) void view_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets, int tiles,
                                                        int cap, int* __restrict__ overflow) {
    __shared__ long long s[256];
    const int view = blockIdx.x, t = threadIdx.x;
    const int per = (tiles + 255) / 256, lo = min(t * per, tiles), hi = min(lo + per, tiles);
    const int* const c = counts + size_t(view) * tiles;
    long long sum = 0;
    for (int q = lo; q < hi; ++q) sum += c[q];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    long long run = s[t] - sum;
    for (int q = lo; q < hi; ++q) {
        offsets[size_t(view) * tiles + q] = int(run < cap ? run : cap);
        run += c[q];
    }
    if (t == 255 && s[t] > cap) *overflow = 1;
}

__global__ void view_bin_fill_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris, int n_verts, int n_tris,
                                     int n_views, int size, const int* __restrict__ n_big, const int* __restrict__ big_list,
                                     const int* __restrict__ offsets, int* __restrict__ cursors, int* __restrict__ bins, int cap,
                                     int* __restrict__ overflow) {
    int view, wg;
    if (!view_chunk(FILL_WGS, n_views, &view, &wg)) return;
    const int n = n_big[view];
    const int tiles_x = size / RM_TILE;
    for (int k = wg * 256 + int(threadIdx.x); k < n; k += FILL_WGS * 256) {
        const int t = big_list[size_t(view) * n_tris + k];
        const rm_tri tr = view_load_tri(tv + size_t(view) * n_verts, tris, t, size);
        scatter_tile_range<size_t>(view, tiles_x, offsets, cursors, bins, cap, overflow, tr.ix0, tr.ix1, tr.iy0, tr.iy1, t);
    }
}

__global__ void view_project_kernel(const double* __restrict__ landmarks, const uint8_t* __restrict__ lm_rgb, int n_lm,
                                    const double* __restrict__ rot, const view_frame* __restrict__ frames, int n_views, int size,
                                    float radius, rv_sphere* __restrict__ spheres) {
    const int q = blockIdx.x * 256 + int(threadIdx.x);
    if (q >= n_views * n_lm) return;
    const int view = q / n_lm, l = q % n_lm;
    double m[9], p[3];
    for (int k = 0; k < 9; ++k) m[k] = rot[view * 9 + k];
    for (int k = 0; k < 3; ++k) p[k] = landmarks[3 * l + k];
    const view_frame f = frames[view];
    const uint32_t rgb = lm_rgb ? uint32_t(lm_rgb[3 * l]) | (uint32_t(lm_rgb[3 * l + 1]) << 8) | (uint32_t(lm_rgb[3 * l + 2]) << 16)
                                : 0xFF0000u;  // blue (viewer.py:71)
    spheres[q] = rv_project_landmark(m, p, f.cx, f.cy, f.half, f.k, radius, rgb, size);
}

__global__ __launch_bounds__(256) void view_tile_kernel(
    const vert12* __restrict__ tv, const int32_t* __restrict__ tris, const float* __restrict__ uvs, const uint8_t* __restrict__ tex,
    int tex_w, int tex_h, const uchar4* __restrict__ colors, int n_verts, const int* __restrict__ counts,
    const int* __restrict__ offsets, const int* __restrict__ bins, int cap, const unsigned long long* __restrict__ keys,
    const view_frame* __restrict__ frames, int shading, int n_views, int size, const rv_sphere* __restrict__ spheres, int n_lm,
    int* __restrict__ lm_pixels, const int* __restrict__ overflow, int* __restrict__ overflow_host, uint32_t* __restrict__ out) {
    __shared__ rm_tri s_tri[256];
    __shared__ int s_id[256];
    __shared__ rv_sphere s_sph[VIEW_SPHERE_CAP];
    __shared__ int s_sph_id[VIEW_SPHERE_CAP];
    __shared__ int s_wave[4];
    __shared__ int s_cnt[VIEW_COUNT_SPAN];
    const int tiles_x = size / RM_TILE;
    int view, tile;
    if (!view_chunk(tiles_x * tiles_x, n_views, &view, &tile)) return;
    const int tid = threadIdx.x;
    const auto [tx0, ty0, i, j, tvv, n, list] = tile_prologue<size_t>(view, tile, tiles_x, tv, n_verts, counts, offsets, bins, cap);
    const view_frame frame = frames[view];

    uint64_t best = keys[(size_t(view) * size + j) * size + i];  // what the small triangles left
    publish_overflow(overflow, overflow_host);

    best = view_tile_resolve(best, tvv, tris, list, n, size, i, j, tid, s_tri, s_id);
    float zbest;
    uint32_t rgb = view_tile_shade(best, tvv, tris, uvs, tex, tex_w, tex_h, colors, shading, frame, size, i, j, &zbest);
    const int win = view_tile_spheres(spheres, view, n_lm, tx0, ty0, i, j, tid, frame, s_sph, s_sph_id, s_wave, &zbest,
                                      &rgb);

    // RGBA, alpha 255, top row first: one aligned 4-byte store per pixel
    out[(size_t(view) * size + (size - 1 - j)) * size + i] = rgb | 0xFF000000u;

    view_tile_count(lm_pixels, view, n_lm, win, tid, s_cnt);
}

}  // namespace

// Scratch, copies, fills and the kernels in front of a tile stage: the mesh stages and the landmark projection, for the landmark
// view's launch set below and the ray view's (raster_rays.hip).  frames_host f32[n_views,4]: cx, cy, half, k = rv_scale(size, half).
int mvlm_view_launch_stages(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                            const float* frames_host, const double* landmarks_host, int n_lm, float radius,
                            const uint8_t* lm_rgb_host, int32_t* lm_pixels_dev, const char* what, mvlm_view_stages* out) {
    const std::string no_scratch = std::string(what) + ": scratch allocation failed";
    const int V = mesh->n_verts, T = mesh->n_tris;
    const int tiles_x = size / RM_TILE, tiles = tiles_x * tiles_x;
    const size_t key_bytes = size_t(n_views) * size * size * sizeof(unsigned long long);
    auto* tv = static_cast<vert12*>(ctx->get_scratch("view.tv", size_t(n_views) * V * sizeof(vert12)));
    auto* rot = static_cast<double*>(ctx->get_scratch("view.rot", size_t(n_views) * 9 * sizeof(double)));
    auto* frames = static_cast<view_frame*>(ctx->get_scratch("view.frames", size_t(n_views) * sizeof(view_frame)));
    raster_bins& b = out->bins;  // (tile-list entries per view: 4 T + 8 tiles)
    const bool have_bins = raster_bins_scratch(ctx, "view", n_views, tiles, T, 4 * T + 8 * tiles, &b);
    auto* keys = static_cast<unsigned long long*>(ctx->get_scratch("view.keys", key_bytes));
    MVLM_REQUIRE(ctx, tv && rot && frames && have_bins && keys, no_scratch);
    double* lm = nullptr;
    uint8_t* lm_rgb = nullptr;
    rv_sphere* spheres = nullptr;
    if (n_lm > 0) {
        lm = static_cast<double*>(ctx->get_scratch("view.lm", size_t(n_lm) * 3 * sizeof(double)));
        spheres = static_cast<rv_sphere*>(ctx->get_scratch("view.spheres", size_t(n_views) * n_lm * sizeof(rv_sphere)));
        MVLM_REQUIRE(ctx, lm && spheres, no_scratch);
        if (lm_rgb_host) {
            lm_rgb = static_cast<uint8_t*>(ctx->get_scratch("view.lm_rgb", size_t(n_lm) * 3));
            MVLM_REQUIRE(ctx, lm_rgb, no_scratch);
        }
    }
    hipStream_t st = ctx->stream;
    // mvlm_render_set_profiling: events between the stages, the first in front of the copies and fills (mvlm_landmark_view_stage_ms,
    // mvlm_ray_view_stage_ms); the caller records the rest on the same clock and marks it
    StageClock& clock = ctx->view_clock;
    if (clock.arm(ctx, 9)) return 1;
    clock.invalidate();
    if (clock.record(ctx, 0, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(rot, rot_host, size_t(n_views) * 9 * sizeof(double), hipMemcpyHostToDevice, st));
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(frames, frames_host, size_t(n_views) * sizeof(view_frame), hipMemcpyHostToDevice, st));
    if (n_lm > 0) {
        MVLM_CHECK_HIP(ctx, hipMemcpyAsync(lm, landmarks_host, size_t(n_lm) * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        if (lm_rgb) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(lm_rgb, lm_rgb_host, size_t(n_lm) * 3, hipMemcpyHostToDevice, st));
        if (lm_pixels_dev) MVLM_CHECK_HIP(ctx, hipMemsetAsync(lm_pixels_dev, 0, size_t(n_views) * n_lm * sizeof(int32_t), st));
    }
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(b.counts, 0, b.ctr_ints * sizeof(int), st));
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(keys, 0xFF, key_bytes, st));  // RM_KEY_EMPTY everywhere, in every call
    MVLM_REQUIRE(ctx, render_overflow_word(ctx), std::string(what) + ": pinned allocation failed");
    if (clock.record(ctx, 1, st)) return 1;
    hipLaunchKernelGGL(view_transform_kernel, dim3(view_chunk_grid((V + 255) / 256, n_views)), dim3(256), 0, st, mesh->verts, V, rot,
                       frames, n_views, ctx->render_subpixel_bits, tv);
    if (clock.record(ctx, 2, st)) return 1;
    hipLaunchKernelGGL(view_classify_kernel, dim3(view_chunk_grid((T + 255) / 256, n_views)), dim3(256), 0, st, tv, mesh->tris, V, T,
                       n_views, size, keys, b.counts, b.n_big, b.big_list);
    if (clock.record(ctx, 3, st)) return 1;
    hipLaunchKernelGGL(view_scan_kernel, dim3(n_views), dim3(256), 0, st, b.counts, b.offsets, tiles, b.cap, b.overflow);
    if (clock.record(ctx, 4, st)) return 1;
    hipLaunchKernelGGL(view_bin_fill_kernel, dim3(view_chunk_grid(FILL_WGS, n_views)), dim3(256), 0, st, tv, mesh->tris, V, T, n_views,
                       size, b.n_big, b.big_list, b.offsets, b.cursors, b.bins, b.cap, b.overflow);
    if (clock.record(ctx, 5, st)) return 1;
    if (n_lm > 0)
        hipLaunchKernelGGL(view_project_kernel, dim3((n_views * n_lm + 255) / 256), dim3(256), 0, st, lm, lm_rgb, n_lm, rot, frames,
                           n_views, size, radius, spheres);
    if (clock.record(ctx, 6, st)) return 1;
    out->tv = tv;
    out->frames = frames;
    out->rot = rot;
    out->keys = keys;
    out->spheres = spheres;
    out->vcol = ctx->render_shading == 0 && mesh->colors && !(mesh->tex && mesh->uvs) ? mesh->colors : nullptr;
    return 0;
}

// The launch set of one landmark view, for an entry point that holds the context and has checked its arguments (api.hip:
// mvlm_render_landmark_view).  frames_host f32[n_views,4]: cx, cy, half, k = rv_scale(size, half).
int mvlm_launch_landmark_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                              const float* frames_host, const double* landmarks_host, int n_lm, float radius,
                              const uint8_t* lm_rgb_host, uint8_t* out_dev, int32_t* lm_pixels_dev, const uint8_t* vert_rgba_dev) {
    mvlm_view_stages s;
    if (mvlm_view_launch_stages(ctx, mesh, rot_host, n_views, size, frames_host, landmarks_host, n_lm, radius, lm_rgb_host,
                                lm_pixels_dev, "landmark view", &s))
        return 1;
    const int tiles_x = size / RM_TILE, tiles = tiles_x * tiles_x;
    // the caller's colours: what a mesh uploaded with them as its vertex colours and no texture is drawn with under shading 0
    const bool given = vert_rgba_dev != nullptr;
    hipLaunchKernelGGL(view_tile_kernel, dim3(view_chunk_grid(tiles, n_views)), dim3(256), 0, ctx->stream, s.tv, mesh->tris,
                       given ? nullptr : mesh->uvs, given ? nullptr : mesh->tex, mesh->tex_w, mesh->tex_h,
                       reinterpret_cast<const uchar4*>(given ? vert_rgba_dev : s.vcol), mesh->n_verts, s.bins.counts,
                       s.bins.offsets, s.bins.bins, s.bins.cap, s.keys, s.frames, given ? 0 : ctx->render_shading, n_views, size, s.spheres, n_lm,
                       lm_pixels_dev, s.bins.overflow, ctx->render_overflow_host, reinterpret_cast<uint32_t*>(out_dev));
    if (ctx->view_clock.record(ctx, 7, ctx->stream)) return 1;
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    ctx->view_clock.mark(8);
    return 0;
}
