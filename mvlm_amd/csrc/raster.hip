// Batched multi-view triangle rasteriser: every camera pose of a mesh in one launch set.
// Replaces the reference's per-pose VTK offscreen loop (src/mvlm/utils/render3d.py:139-170:
// CPU re-transform of all vertices + GL draw + two read-backs per pose).
//
// Pipeline (all views at once, nothing returns to the host):
//   1. transform   one thread per (view, vertex): M*v in double -> snapped window coords + z
//   2. classify    one thread per (view, triangle): covered pixel-centre box.  Most triangles of
//                  a 100k-face head are sub-pixel: empty boxes are culled, boxes of <= 16 pixel
//                  centres are resolved on the spot with a 64-bit atomicMin of the
//                  (depth, id) key per covered pixel, larger triangles are counted into
//                  16x16-pixel tiles and appended to the view's "big" list
//   3. scan        one workgroup per view: exclusive prefix sum over its 256 tile counters
//   4. bin fill    big triangles only: ids scattered into the per-tile lists
//   5. tile raster one workgroup per (view, tile), one thread per pixel: starts from the key the
//                  small triangles left, stages the tile's big-triangle list through LDS in
//                  chunks of 256 set-up triangles (each thread sets one up), every pixel walks
//                  the chunk (LDS broadcast reads) and keeps the winning key in a register;
//                  then shades (nearest texel, unlit - or, for a mesh with per-vertex colours and no
//                  texture, the interpolated colour: raster_vc.hip) and writes its RGBD texel; a tile row
//                  is 256 contiguous bytes of the [N,256,256,4] f32 stack.
// The key (depth bits << 32 | ~triangle id) makes the result independent of the order in which
// atomics and tiles run: least depth wins, the later-drawn triangle wins ties (GL_LEQUAL).
// Bandwidth-bound on its REAL traffic, measured (round 4): 0.74 GB through the L2s per 96 views at
// 4.5 TB/s = the 165 us it took - 100 MB of pixels, 160 MB of texels (a 3-byte nearest texel costs a 64-byte line; every
// sample lies in another one), 175 MB for the key plane (clear, atomics, read back), 216 MB of transformed vertices.
// Neither fewer instructions (the 24-bit path below: 3 %) nor more loads in flight per thread (TPT / PPT: nothing) nor
// keeping the keys in LDS with every survivor binned (built: 210 us - a cull pass, a survivor list, a fill pass and a
// per-tile gather cost more than the plane they save) beat this structure; fewer bytes per vertex do.
#include "raster_tile.h"

namespace {

// (transform_kernel and scan_kernel have a twin each in raster_view.hip; why the two pairs are not merged: raster_bins.h)
__global__ void transform_kernel(const float* __restrict__ verts, int n_verts, const double* __restrict__ rot,
                                 int n_views, int sub_bits, vert12* __restrict__ tv) {
    int view, chunk;
    if (!view_chunk((n_verts + 255) / 256, n_views, &view, &chunk)) return;
    const int v = chunk * 256 + int(threadIdx.x);
    if (v >= n_verts) return;
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = rot[view * 9 + k];
    const rm_vert o = rm_transform(m, verts[3 * v], verts[3 * v + 1], verts[3 * v + 2], sub_bits);
    vert12 w;
    w.X = o.X;
    w.Y = o.Y;
    w.z = o.z;
    tv[size_t(view) * n_verts + v] = w;
}

__device__ inline rm_tri load_tri(const vert12* tvv, const int32_t* tris, int t) {
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    return rm_setup(load_vert(tvv, a), load_vert(tvv, b), load_vert(tvv, c));
}

// (the 24-bit edge functions - tri24, setup24, cover24 - that classify_one shares with the tile stage: raster_tile.h)

// Classify every (view, triangle): cull / resolve small ones with atomics / count big ones.
// Order of the tests: the pixel-centre box first (integer shifts: most triangles of a dense scan lie between pixel
// centres and leave here), then the area; triangles of small extent take the 24-bit path (above).
// Returns true for a big triangle (the caller appends it to the view's list).
__device__ inline bool classify_one(int view, int t, const rm_vert& va, const rm_vert& vb, const rm_vert& vc,
                                    unsigned long long* __restrict__ keys, int* __restrict__ counts) {
    // rm_setup's box: pixel i has its centre at 256 i + 128; ceil / floor of a division by 256 as arithmetic shifts
    const int32_t minx = min(va.X, min(vb.X, vc.X)), maxx = max(va.X, max(vb.X, vc.X));
    const int32_t miny = min(va.Y, min(vb.Y, vc.Y)), maxy = max(va.Y, max(vb.Y, vc.Y));
    const int ix0 = max((minx + (RM_SUB - 1 - RM_HALF)) >> 8, 0), ix1 = min((maxx - RM_HALF) >> 8, RM_SIZE - 1);
    const int iy0 = max((miny + (RM_SUB - 1 - RM_HALF)) >> 8, 0), iy1 = min((maxy - RM_HALF) >> 8, RM_SIZE - 1);
    static_assert(RM_SUB == 256 && RM_HALF == 128, "the shifts above divide by RM_SUB");
    if (ix0 > ix1 || iy0 > iy1) return false;
    const int w = ix1 - ix0 + 1, h = iy1 - iy0 + 1;
    const bool small = maxx - minx < RM_SMALL_EXTENT && maxy - miny < RM_SMALL_EXTENT;
    if (w * h <= SMALL_PIXELS) {
        unsigned long long* kv = keys + size_t(view) * RM_SIZE * RM_SIZE;
        if (small) {
            tri24 tr;
            if (!setup24(va, vb, vc, &tr)) return false;
            // (resolve_small_box<tri24, cover24<tri24>, int> written out: through the helper the row prologue of this loop, which
            // every triangle of a dense scan takes, came out in another instruction order)
            for (int j = iy0; j <= iy1; ++j)
                for (int ii = ix0; ii <= ix1; ++ii) {
                    float b0, b1, b2;
                    if (!cover24(&tr, ii, j, &b0, &b1, &b2)) continue;
                    const float z = rm_interp(b0, b1, b2, tr.z0, tr.z1, tr.z2);
                    if (!(z >= 0.0f && z <= 1.0f)) continue;  // near / far clip (render3d.py:136)
                    atomicMin(&kv[j * RM_SIZE + ii], (unsigned long long)rm_key(z, uint32_t(t)));
                }
        } else {  // a long sliver that crosses the window's edge: few pixel centres inside, vertices far apart
            const rm_tri tr = rm_setup(va, vb, vc);
            if (!tr.valid) return false;
            resolve_small_box<rm_tri, rm_cover, int>(kv, RM_SIZE, tr.ix0, tr.ix1, tr.iy0, tr.iy1, tr, t);
        }
        return false;
    }
    // big: valid means a non-zero area (rm_setup)
    if (small) {
        if (__mul24(vb.X - va.X, vc.Y - va.Y) == __mul24(vb.Y - va.Y, vc.X - va.X)) return false;
    } else if (int64_t(vb.X - va.X) * (vc.Y - va.Y) == int64_t(vb.Y - va.Y) * (vc.X - va.X)) {
        return false;
    }
    count_tile_range<int>(counts, view, RM_TILES, ix0, ix1, iy0, iy1);
    return true;
}

// A thread takes TPT triangles and has all their loads (indices, then three vertices each) in flight together.  Measured
// (tools/raster_bench.py, 96 views of the bench mesh): TPT 1 / 2 / 4 = 164 / 161 / 163 us per render - the pass does not
// wait for latency (without its key atomics it still takes 43 of its 59 us: 9.5 M threads x four 12-byte gathers through
// the L1s), so TPT stays 1.  (The big triangles' ids go to the view's list with one atomic per wave: raster_bins.h, append_big.)
constexpr int CLASSIFY_TPT = 1;
template <int TPT>
__global__ __launch_bounds__(256) void classify_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris, int n_verts,
                                                       int n_tris, int n_views, unsigned long long* __restrict__ keys,
                                                       int* __restrict__ counts, int* __restrict__ n_big, int* __restrict__ big_list) {
    int view, chunk;
    if (!view_chunk((n_tris + 256 * TPT - 1) / (256 * TPT), n_views, &view, &chunk)) return;
    const vert12* const tvv = tv + size_t(view) * n_verts;
    int t[TPT];
    int ia[TPT], ib[TPT], ic[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        t[k] = (chunk * TPT + k) * 256 + int(threadIdx.x);
        const int tt = t[k] < n_tris ? t[k] : 0;  // (unconditional loads: all of them leave together)
        ia[k] = tris[3 * tt];
        ib[k] = tris[3 * tt + 1];
        ic[k] = tris[3 * tt + 2];
    }
    rm_vert va[TPT], vb[TPT], vc[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        va[k] = load_vert(tvv, ia[k]);
        vb[k] = load_vert(tvv, ib[k]);
        vc[k] = load_vert(tvv, ic[k]);
    }
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const bool big = t[k] < n_tris && classify_one(view, t[k], va[k], vb[k], vc[k], keys, counts);
        append_big(big, t[k], view, n_tris, n_big, big_list);
    }
}

// Scatter the big triangles' ids into the per-tile lists (offsets from the scan).  FILL_WGS workgroups per view stride
// over the view's big list: a grid sized for "every triangle is big" spent 11 us on dispatching 37 000 workgroups that
// found nothing to do (a dense scan has a handful of big triangles per view).
__global__ void bin_fill_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris, int n_verts,
                                int n_tris, int n_views, const int* __restrict__ n_big,
                                const int* __restrict__ big_list, const int* __restrict__ offsets,
                                int* __restrict__ cursors, int* __restrict__ bins, int cap,
                                int* __restrict__ overflow) {
    int view, wg;
    if (!view_chunk(FILL_WGS, n_views, &view, &wg)) return;
    const int n = n_big[view];
    for (int k = wg * 256 + int(threadIdx.x); k < n; k += FILL_WGS * 256) {
        const int t = big_list[size_t(view) * n_tris + k];
        const rm_tri tr = load_tri(tv + size_t(view) * n_verts, tris, t);
        scatter_tile_range<int>(view, RM_TILES, offsets, cursors, bins, cap, overflow, tr.ix0, tr.ix1, tr.iy0, tr.iy1, t);
    }
}

__global__ void scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets, int cap,
                            int* __restrict__ overflow) {
    __shared__ int s[TILES];
    const int view = blockIdx.x, t = threadIdx.x;
    s[t] = counts[view * TILES + t];
    __syncthreads();
    for (int d = 1; d < TILES; d <<= 1) {
        const int v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    offsets[view * TILES + t] = s[t] - counts[view * TILES + t];
    if (t == TILES - 1 && s[t] > cap) *overflow = 1;
}

// The tile stage (raster_tile.h: tile_body) without per-vertex colours; raster_vc.hip holds the coloured form.
__global__ __launch_bounds__(256) void tile_kernel(const vert12* __restrict__ tv, const int32_t* __restrict__ tris,
                                                   const float* __restrict__ uvs, const uint8_t* __restrict__ tex,
                                                   int tex_w, int tex_h, int n_verts, const int* __restrict__ counts,
                                                   const int* __restrict__ offsets, const int* __restrict__ bins,
                                                   int cap, unsigned long long* __restrict__ keys,
                                                   int shading, int n_views, const int* __restrict__ overflow,
                                                   int* __restrict__ overflow_host, float* __restrict__ out) {
    tile_body<false>(tv, tris, uvs, tex, tex_w, tex_h, nullptr, n_verts, counts, offsets, bins, cap, keys, shading, n_views,
                     overflow, overflow_host, out);
}

}  // namespace

extern "C" int mvlm_render(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, float* out_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, mesh && rot_host && out_dev && n_views > 0, "render: bad arguments");
    MVLM_REQUIRE(ctx, mesh->n_verts > 0 && mesh->n_tris >= 0, "render: empty mesh");
    // A point mesh (n_tris == 0) is drawn as splats by the kernels of raster_points.hip; what it does not have is refused here,
    // before anything is enqueued.
    const bool cloud = mesh->n_tris == 0;
    // (with normals - a file's, or estimated: point_normals="estimate" / mvlm_mesh_estimate_normals - a cloud is geometry-shaded)
    MVLM_REQUIRE(ctx, !cloud || ctx->render_shading == 0 || mesh->normals,
                 "render: geometry shading of a point cloud is not supported without normals (this cloud has none: upload a file's, "
                 "or have them estimated - point_normals=\"estimate\", mvlm_mesh_estimate_normals)");
    MVLM_REQUIRE(ctx, !cloud || ctx->render_multisamples == 0, "render: multisampled rendering of a point cloud is not supported");
    MVLM_REQUIRE(ctx, !cloud || n_views <= 65535, "render: at most 65535 views of a point cloud per call");
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;  // the upload runs on a stream of its own
    const int V = mesh->n_verts, T = mesh->n_tris;
    vert12* tv = nullptr;
    auto* rot = static_cast<double*>(ctx->get_scratch("raster.rot", size_t(n_views) * 9 * sizeof(double)));
    raster_bins b;  // (tile-list entries per view: 4 T + 16 384)
    bool have_bins = true;
    if (!cloud) {  // (a cloud's splats go straight to the key plane: no transformed vertices, no bins)
        tv = static_cast<vert12*>(ctx->get_scratch("raster.tv", size_t(n_views) * V * sizeof(vert12)));
        have_bins = raster_bins_scratch(ctx, "raster", n_views, TILES, T, 4 * T + 16384, &b);
    }
    // one key per pixel, or S per pixel in a plane of its own when multisampling (allocated only then)
    const int S = ctx->render_multisamples;
    // per-vertex colours shade the RGB planes of the unlit render of a mesh without a usable texture
    const uint8_t* const vcol = ctx->render_shading == 0 && mesh->colors && !(mesh->tex && mesh->uvs) ? mesh->colors : nullptr;
    const char* const key_name = S ? "raster.keys4" : "raster.keys";
    const size_t key_bytes = size_t(n_views) * RM_SIZE * RM_SIZE * size_t(S ? S : 1) * sizeof(unsigned long long);
    auto* keys = static_cast<unsigned long long*>(ctx->get_scratch(key_name, key_bytes));
    MVLM_REQUIRE(ctx, (cloud || tv) && rot && have_bins && keys, "render: scratch allocation failed");
    unsigned long long* point_stats = nullptr;  // (mvlm_points_set_counting: the splat kernel's measuring form)
    if (cloud && ctx->points_counting) {
        point_stats = static_cast<unsigned long long*>(ctx->get_scratch("points.stats", 2 * sizeof(unsigned long long)));
        MVLM_REQUIRE(ctx, point_stats, "render: scratch allocation failed");
    }
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(rot, rot_host, size_t(n_views) * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!cloud) MVLM_CHECK_HIP(ctx, hipMemsetAsync(b.counts, 0, b.ctr_ints * sizeof(int), ctx->stream));
    if (point_stats) MVLM_CHECK_HIP(ctx, hipMemsetAsync(point_stats, 0, 2 * sizeof(unsigned long long), ctx->stream));
    // The key plane is EMPTY between renders (tile_kernel clears what it reads); it is filled here only when the buffer is new
    // or a render did not run to its end.  `clean` = the buffer and capacity it was last known clean at: a buffer that
    // get_scratch replaced (after a failed allocation, say) is filled even when its size is the old one.
    mvlm_ctx::KeyPlaneState& clean = S ? ctx->raster_keys4_clean : ctx->raster_keys_clean;
    const size_t keys_cap = ctx->scratch[key_name].second;
    if (clean.ptr != keys || clean.cap != keys_cap)
        MVLM_CHECK_HIP(ctx, hipMemsetAsync(keys, 0xFF, keys_cap, ctx->stream));  // RM_KEY_EMPTY everywhere
    clean = mvlm_ctx::KeyPlaneState{};  // (until this call has enqueued its tile kernel)
    int* const overflow_host = render_overflow_word(ctx);
    MVLM_REQUIRE(ctx, overflow_host, "render: pinned allocation failed");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->render_profiling) {  // HIP events on the launch stream around the five kernels of this call
        if (ctx->render_event_cursor + 2 > ctx->render_events.size()) ctx->render_events.resize(ctx->render_event_cursor + 2, nullptr);
        for (int k = 0; k < 2; ++k) {
            hipEvent_t& e = ctx->render_events[ctx->render_event_cursor + k];
            if (!e) MVLM_CHECK_HIP(ctx, hipEventCreate(&e));
        }
        e0 = ctx->render_events[ctx->render_event_cursor];
        e1 = ctx->render_events[ctx->render_event_cursor + 1];
        ctx->render_event_cursor += 2;
        MVLM_CHECK_HIP(ctx, hipEventRecord(e0, ctx->stream));
    }
    if (cloud) {
        StageClock& clock = ctx->points_clock;  // (profiling: events of the cloud's own round its two kernels, mvlm_points_stage_ms)
        clock.invalidate();
        if (clock.arm(ctx, 3) || clock.record(ctx, 0, ctx->stream)) return 1;
        // per-point colours shade the RGB planes (white without them); a texture or uvs on a faceless mesh are ignored
        if (ctx->render_shading == 1) {  // the same splats, then the tile stage that shades with the normals (cloud_normals.hip)
            raster_points_splat_launch(ctx->stream, mesh->verts, V, rot, n_views, ctx->render_subpixel_bits, mesh->point_R, mesh->point_c,
                                       keys, point_stats);
            if (clock.record(ctx, 1, ctx->stream)) return 1;
            cloud_normals_tile_launch(ctx->stream, mesh->normals, rot, n_views, keys, overflow_host, out_dev);
        } else {
            raster_points_launch(ctx->stream, mesh->verts, mesh->colors, V, rot, n_views, ctx->render_subpixel_bits, mesh->point_R,
                                 mesh->point_c, keys, point_stats, overflow_host, out_dev, clock.event(1));
        }
        if (clock.record(ctx, 2, ctx->stream)) return 1;
        clock.mark(3);
    } else {
        hipLaunchKernelGGL(transform_kernel, dim3(view_chunk_grid((V + 255) / 256, n_views)), dim3(256), 0, ctx->stream,
                           mesh->verts, V, rot, n_views, ctx->render_subpixel_bits, tv);
        if (S == 0) {
            hipLaunchKernelGGL(classify_kernel<CLASSIFY_TPT>, dim3(view_chunk_grid((T + 256 * CLASSIFY_TPT - 1) / (256 * CLASSIFY_TPT), n_views)), dim3(256), 0,
                               ctx->stream, tv, mesh->tris, V, T, n_views, keys, b.counts, b.n_big, b.big_list);
            hipLaunchKernelGGL(scan_kernel, dim3(n_views), dim3(TILES), 0, ctx->stream, b.counts, b.offsets, b.cap, b.overflow);
            hipLaunchKernelGGL(bin_fill_kernel, dim3(view_chunk_grid(FILL_WGS, n_views)), dim3(256), 0, ctx->stream, tv,
                               mesh->tris, V, T, n_views, b.n_big, b.big_list, b.offsets, b.cursors, b.bins, b.cap, b.overflow);
            if (vcol)
                raster_vc_tile(ctx->stream, 0, tv, mesh->tris, vcol, V, n_views, b, keys, ctx->render_shading, overflow_host, out_dev);
            else
                hipLaunchKernelGGL(tile_kernel, dim3(view_chunk_grid(TILES, n_views)), dim3(256), 0, ctx->stream, tv, mesh->tris,
                                   mesh->uvs, mesh->tex, mesh->tex_w, mesh->tex_h, V, b.counts, b.offsets, b.bins, b.cap, keys,
                                   ctx->render_shading, n_views, b.overflow, overflow_host, out_dev);
        } else {  // S == 4 (mvlm_set_render_multisamples admits nothing else): the kernels of raster_ms.hip
            raster_ms_classify(ctx->stream, S, tv, mesh->tris, V, T, n_views, keys, b);
            hipLaunchKernelGGL(scan_kernel, dim3(n_views), dim3(TILES), 0, ctx->stream, b.counts, b.offsets, b.cap, b.overflow);
            raster_ms_bin_and_tile(ctx->stream, S, tv, mesh->tris, mesh->uvs, mesh->tex, mesh->tex_w, mesh->tex_h, V, T, n_views, b,
                                   keys, ctx->render_shading, overflow_host, out_dev, vcol);
        }
    }
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    clean = mvlm_ctx::KeyPlaneState{keys, keys_cap};
    if (e1) {
        MVLM_CHECK_HIP(ctx, hipEventRecord(e1, ctx->stream));
        ctx->render_prof.push_back({n_views, V, T, e0, e1});
    }
    // (the tile kernel carries the overflow flag to pinned host memory; mvlm_render_check reads it after the caller's synchronisation)
    return 0;
}

// The rotations of the last mvlm_render on this context, f64[n_views, 9] on the device (its scratch: valid until the next
// render): the estimator's rays of the same views need the same table (estimator3d.py:57) and read it from here.
extern "C" int mvlm_render_rotations_dev(mvlm_ctx* ctx, const double** rot_dev) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    MVLM_REQUIRE(ctx, rot_dev, "render_rotations_dev: null pointer");
    const auto it = ctx->scratch.find("raster.rot");
    *rot_dev = it == ctx->scratch.end() ? nullptr : static_cast<const double*>(it->second.first);
    MVLM_REQUIRE(ctx, *rot_dev, "render_rotations_dev: nothing has been rendered on this context");
    return 0;
}

extern "C" int mvlm_render_check(mvlm_ctx* ctx) {
    MVLM_ENTER(ctx);
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MVLM_REQUIRE(ctx, !ctx->render_overflow_host || *ctx->render_overflow_host == 0,
                 "render: per-view tile lists overflowed (mesh has too many screen-filling triangles)");
    return 0;
}

extern "C" int mvlm_render_set_profiling(mvlm_ctx* ctx, int enabled) {
    MVLM_ENTER(ctx);
    ctx->render_profiling = enabled != 0;
    ctx->render_prof.clear();
    ctx->render_event_cursor = 0;
    return 0;
}

extern "C" int mvlm_render_get_profile(mvlm_ctx* ctx, int32_t* n_views, int32_t* n_verts, int32_t* n_tris, float* ms,
                                       int cap) {
    std::lock_guard<std::mutex> lk(ctx->mu);  // returns a record count, -1 on failure; clears the records
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    int n = 0;
    for (const auto& r : ctx->render_prof) {
        if (n >= cap) break;
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) return -1;
        n_views[n] = r.n_views;
        n_verts[n] = r.n_verts;
        n_tris[n] = r.n_tris;
        ms[n] = t;
        ++n;
    }
    ctx->render_prof.clear();
    ctx->render_event_cursor = 0;
    return n;
}

extern "C" int mvlm_set_render_subpixel_bits(mvlm_ctx* ctx, int bits) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    MVLM_REQUIRE(ctx, bits >= 4 && bits <= 8, "render: subpixel bits must be 4..8 (GL_SUBPIXEL_BITS of the OpenGL to match; 8 = GPUs)");
    ctx->render_subpixel_bits = bits;
    return 0;
}

extern "C" int mvlm_set_render_multisamples(mvlm_ctx* ctx, int samples) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    MVLM_REQUIRE(ctx, samples == 0 || samples == 4,
                 "render: multisamples must be 0 (one sample at the pixel centre, the default) or 4 (" + std::to_string(samples) +
                     " given)");
    ctx->render_multisamples = samples;
    return 0;
}

extern "C" int mvlm_set_render_shading(mvlm_ctx* ctx, int shading) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    MVLM_REQUIRE(ctx, shading == 0 || shading == 1, "render: shading must be 0 (unlit texture) or 1 (geometry)");
    ctx->render_shading = shading;
    return 0;
}
