// The ray view (mvlm_render_ray_view): the reference's RayVisualizer (visualization/ray_visualizer.py) for the offscreen case -
// the landmark view's picture (raster_view.hip) with every view's ray for every landmark drawn between the mesh and the spheres
// as an opaque, head-lit capsule of ray_radius model units around the segment start -> end, depth-tested ("Ray
// view"; the arithmetic and its operation order: raster_view_math.h, rv_project_ray / rv_ray_fragment).
//
// The mesh stages and the landmark projection are the landmark view's own kernels, launched by mvlm_view_launch_stages; the
// tile stage's mesh, sphere and count code is raster_view_tile.h's.  Two kernels of this object:
//   project   one thread per (view, ray): the 64-byte record, straight from the device's float64 starts / ends
//   tile      one workgroup per (view, 16 x 16 tile), a thread per pixel, as view_tile_kernel; between the mesh and the spheres
//             it compacts the rays that rv_ray_touches_tile cannot rule out into an LDS list (ballots, RAYS_CAP candidates a
//             round, any number of rounds; a round nobody touches costs one barrier) and every pixel walks the list in index
//             order: a fragment wins on z <=, so the nearer ray wins and the higher index an equal depth, whatever superset of
//             the true candidates the list holds.  The pixels each ray won are counted after the spheres, one atomic per wave
//             and distinct winner.
#include "raster_view_tile.h"

namespace {

static_assert(sizeof(rv_ray) == 64 && alignof(rv_ray) == 16, "a ray record is four 16-byte words");
constexpr int RAYS_CAP = 256;  // rays in a tile's LDS list at a time: one candidate per thread and round

__global__ void rays_project_kernel(const double* __restrict__ starts, const double* __restrict__ ends,
                                    const uint8_t* __restrict__ ray_rgb, int n_rays, const double* __restrict__ rot,
                                    const view_frame* __restrict__ frames, int n_views, int size, float ray_radius,
                                    rv_ray* __restrict__ rays) {
    const size_t q = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (q >= size_t(n_views) * n_rays) return;
    const int view = int(q / n_rays), r = int(q % n_rays);
    double m[9], a[3], b[3];
    for (int k = 0; k < 9; ++k) m[k] = rot[view * 9 + k];
    for (int k = 0; k < 3; ++k) {
        a[k] = starts[3 * size_t(r) + k];
        b[k] = ends[3 * size_t(r) + k];
    }
    const view_frame f = frames[view];
    const uint32_t rgb = ray_rgb ? uint32_t(ray_rgb[3 * r]) | (uint32_t(ray_rgb[3 * r + 1]) << 8) | (uint32_t(ray_rgb[3 * r + 2]) << 16)
                                 : RV_RAY_RGB;
    rays[q] = rv_project_ray(m, a, b, f.cx, f.cy, f.half, f.k, ray_radius, rgb, size);
}

__global__ __launch_bounds__(256) void rays_tile_kernel(
    const vert12* __restrict__ tv, const int32_t* __restrict__ tris, const float* __restrict__ uvs, const uint8_t* __restrict__ tex,
    int tex_w, int tex_h, const uchar4* __restrict__ colors, int n_verts, const int* __restrict__ counts,
    const int* __restrict__ offsets, const int* __restrict__ bins, int cap, const unsigned long long* __restrict__ keys,
    const view_frame* __restrict__ frames, int shading, int n_views, int size, const rv_sphere* __restrict__ spheres, int n_lm,
    int* __restrict__ lm_pixels, const rv_ray* __restrict__ rays, int n_rays, int* __restrict__ ray_pixels,
    const int* __restrict__ overflow, int* __restrict__ overflow_host, uint32_t* __restrict__ out) {
    __shared__ rm_tri s_tri[256];
    __shared__ int s_id[256];
    __shared__ rv_sphere s_sph[VIEW_SPHERE_CAP];
    __shared__ int s_sph_id[VIEW_SPHERE_CAP];
    __shared__ int s_wave[4];
    __shared__ int s_cnt[VIEW_COUNT_SPAN];
    __shared__ rv_ray s_ray[RAYS_CAP];
    __shared__ int s_ray_id[RAYS_CAP];
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

    // ---- rays: after the mesh (they win ties against it), in ray order (the later one wins an equal depth) ----
    int rwin = -1;
    const rv_ray* const rv = rays + size_t(view) * n_rays;
    const int wave = tid >> 6, lane = tid & 63;
    for (int base = 0; base < n_rays; base += RAYS_CAP) {
        const int cand = base + tid;
        bool touch = false;
        uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0, w3 = w0;  // the record as four 16-byte words
        if (cand < n_rays) {
            const uint4* const src = reinterpret_cast<const uint4*>(rv + cand);
            w0 = src[0];
            w1 = src[1];
            w2 = src[2];
            rv_ray r;
            r.Xa = __uint_as_float(w0.x); r.Ya = __uint_as_float(w0.y); r.R = __uint_as_float(w0.w);
            r.Xb = __uint_as_float(w1.x); r.Yb = __uint_as_float(w1.y);
            r.ix0 = short(w2.x & 0xFFFFu); r.ix1 = short(w2.x >> 16); r.iy0 = short(w2.y & 0xFFFFu); r.iy1 = short(w2.y >> 16);
            touch = rv_ray_touches_tile(&r, tx0, ty0) != 0;
            if (touch) w3 = src[3];
        }
        if (!__syncthreads_or(touch)) continue;  // (a barrier: the previous round's walk is over)
        const unsigned long long m = __ballot(touch);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;  // (as in view_tile_spheres; why this is not a shared helper: raster_bins.h)
        for (int w = 0; w < 4; ++w) {
            off += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (touch) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
            uint4* const dst = reinterpret_cast<uint4*>(&s_ray[pos]);
            dst[0] = w0;
            dst[1] = w1;
            dst[2] = w2;
            dst[3] = w3;
            s_ray_id[pos] = cand;
        }
        __syncthreads();
        for (int q = 0; q < total; ++q) {
            float zr, shade;
            if (!rv_ray_fragment(&s_ray[q], i, j, frame.k, &zr, &shade)) continue;
            if (!(zr <= zbest)) continue;
            zbest = zr;
            rwin = s_ray_id[q];
            rgb = rv_sphere_colour(s_ray[q].rgb, shade);
        }
    }

    const int win = view_tile_spheres(spheres, view, n_lm, tx0, ty0, i, j, tid, frame, s_sph, s_sph_id, s_wave, &zbest,
                                      &rgb);
    if (win >= 0) rwin = -1;  // a sphere wins an equal depth against a ray

    // RGBA, alpha 255, top row first: one aligned 4-byte store per pixel
    out[(size_t(view) * size + (size - 1 - j)) * size + i] = rgb | 0xFF000000u;
    view_tile_count(lm_pixels, view, n_lm, win, tid, s_cnt);

    // ---- pixels each ray won: per wave, one atomic per distinct winner ----
    if (ray_pixels) {
        unsigned long long todo = __ballot(rwin >= 0);
        while (todo) {  // (wave-uniform)
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int id = __shfl(rwin, leader);
            const unsigned long long same = __ballot(rwin == id);
            if (lane == leader) atomicAdd(&ray_pixels[size_t(view) * n_rays + id], __popcll(same));
            todo &= ~same;
        }
    }
}

}  // namespace

// The launch set of one ray view, for an entry point that holds the context and has checked its arguments (api.hip:
// mvlm_render_ray_view).  frames_host f32[n_views,4] as mvlm_launch_landmark_view takes them; starts_dev / ends_dev f64[n_rays,3]
// on the device (null when n_rays == 0), ray_rgb_host u8[n_rays,3] or null.
int mvlm_launch_ray_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                         const float* frames_host, const double* landmarks_host, int n_lm, float radius, const uint8_t* lm_rgb_host,
                         const double* starts_dev, const double* ends_dev, int n_rays, float ray_radius, const uint8_t* ray_rgb_host,
                         uint8_t* out_dev, int32_t* lm_pixels_dev, int32_t* ray_pixels_dev) {
    rv_ray* rays = nullptr;
    uint8_t* ray_rgb = nullptr;
    if (n_rays > 0) {  // (before anything is enqueued)
        rays = static_cast<rv_ray*>(ctx->get_scratch("rays.rec", size_t(n_views) * n_rays * sizeof(rv_ray)));
        MVLM_REQUIRE(ctx, rays, "ray view: scratch allocation failed");
        if (ray_rgb_host) {
            ray_rgb = static_cast<uint8_t*>(ctx->get_scratch("rays.rgb", size_t(n_rays) * 3));
            MVLM_REQUIRE(ctx, ray_rgb, "ray view: scratch allocation failed");
        }
    }
    mvlm_view_stages s;
    if (mvlm_view_launch_stages(ctx, mesh, rot_host, n_views, size, frames_host, landmarks_host, n_lm, radius, lm_rgb_host,
                                lm_pixels_dev, "ray view", &s))
        return 1;
    hipStream_t st = ctx->stream;
    if (n_rays > 0) {
        if (ray_rgb) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(ray_rgb, ray_rgb_host, size_t(n_rays) * 3, hipMemcpyHostToDevice, st));
        if (ray_pixels_dev) MVLM_CHECK_HIP(ctx, hipMemsetAsync(ray_pixels_dev, 0, size_t(n_views) * n_rays * sizeof(int32_t), st));
        const size_t total = size_t(n_views) * n_rays;
        hipLaunchKernelGGL(rays_project_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, starts_dev, ends_dev, ray_rgb,
                           n_rays, s.rot, s.frames, n_views, size, ray_radius, rays);
    }
    if (ctx->view_clock.record(ctx, 7, st)) return 1;
    const int tiles_x = size / RM_TILE, tiles = tiles_x * tiles_x;
    hipLaunchKernelGGL(rays_tile_kernel, dim3(view_chunk_grid(tiles, n_views)), dim3(256), 0, st, s.tv, mesh->tris, mesh->uvs, mesh->tex,
                       mesh->tex_w, mesh->tex_h, reinterpret_cast<const uchar4*>(s.vcol), mesh->n_verts, s.bins.counts, s.bins.offsets, s.bins.bins,
                       s.bins.cap, s.keys, s.frames, ctx->render_shading, n_views, size, s.spheres, n_lm, lm_pixels_dev, rays, n_rays,
                       n_rays > 0 ? ray_pixels_dev : nullptr, s.bins.overflow, ctx->render_overflow_host,
                       reinterpret_cast<uint32_t*>(out_dev));
    if (ctx->view_clock.record(ctx, 8, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    ctx->view_clock.mark(9);
    return 0;
}
