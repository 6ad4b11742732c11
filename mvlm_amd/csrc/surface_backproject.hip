// The surface heat (mvlm_surface_heat): all views' heatmaps laid on the scan.  Every vertex is carried into every rendered view
// with the render's own transform, tested against the depth plane the network saw, and where the view sees it the view's heatmap
// values at its pixel are added up per landmark: a score per (vertex, landmark), a colour per vertex in the layout the landmark
// view's tile kernel reads, and per landmark the vertex where the views together believe it lies ("Surface heat";
// surface_backproject_math.h holds the arithmetic and the contract).
//
// Behind the heat sheet's own peak kernel (mvlm_heat_launch_peaks), three kernels on the context's stream:
//   1. score   a workgroup owns 256 consecutive vertices x BP_LM consecutive landmarks and walks the views in ascending order: a
//              thread transforms its vertex and tests its depth once per view, then gathers the chunk's heat values at its pixel
//              (loads of the whole chunk issued together) and adds their shares to BP_LM float64 sums in registers.  The rotation
//              and the peaks are the same for the whole workgroup.  No atomics: a sum has one owner and a fixed order.
//   2. paint   a workgroup per 256 vertices takes their scores through LDS BP_PAINT_LM landmarks at a time: a thread per vertex
//              picks its winner along its row, a thread per (landmark, 32 vertices) the best key down its column; one 64-bit
//              atomicMax per (workgroup, landmark) that has a score above 0 - a maximum, so the order does not matter.
//   3. peaks   a thread per landmark takes its key apart.
// Built as an object of its own (build/backproject/, tests/golden/kernel_occupancy_backproject.json).
#include "common.h"
#include "surface_backproject_math.h"

#include <cmath>

namespace {

constexpr int BP_PLANE = RM_SIZE * RM_SIZE;  // floats in a heatmap plane
#ifndef MVLM_BP_LM
#define MVLM_BP_LM 16  // (-DMVLM_BP_LM=n: a build for measuring another chunk; profiles/surface_heat_time.txt)
#endif
constexpr int BP_LM = MVLM_BP_LM;            // landmarks whose sums a thread of the score kernel holds
constexpr int BP_PAINT_LM = 32;              // landmarks whose scores the paint kernel holds in LDS at a time

__global__ __launch_bounds__(256) void backproject_score_kernel(const float* __restrict__ verts, int n_verts,
                                                                const double* __restrict__ rot, const float* __restrict__ images,
                                                                const float* __restrict__ heat, const float* __restrict__ peaks,
                                                                int n_views, int n_lm, int sub_bits, int depth_tol,
                                                                float* __restrict__ score, int32_t* __restrict__ n_vis_out) {
    const int v = blockIdx.x * 256 + int(threadIdx.x);
    const int l0 = blockIdx.y * BP_LM;
    if (v >= n_verts) return;
    const float vx = verts[3 * size_t(v)], vy = verts[3 * size_t(v) + 1], vz = verts[3 * size_t(v) + 2];
    double sum[BP_LM];
#pragma unroll
    for (int u = 0; u < BP_LM; ++u) sum[u] = 0.0;
    int n_vis = 0;
    if (hs_finite(vx) && hs_finite(vy) && hs_finite(vz)) {
        for (int n = 0; n < n_views; ++n) {
            double m[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = rot[size_t(n) * 9 + k];
            const rm_vert o = rm_transform(m, vx, vy, vz, sub_bits);
            int i, j;
            if (!sb_pixel(o, &i, &j)) continue;
            const int pix = (RM_SIZE - 1 - j) * RM_SIZE + i;
            const float d = images[(size_t(n) * BP_PLANE + pix) * 4 + 3];
            if (!sb_visible(sb_vertex_step(o.z), sb_pixel_step(d), depth_tol)) continue;
            ++n_vis;
            const float* const at = heat + (size_t(n) * n_lm + l0) * BP_PLANE + pix;  // in plane l0 of the view
            float pk[BP_LM], h[BP_LM];
#pragma unroll
            for (int u = 0; u < BP_LM; ++u) {  // (pk is the same for the whole workgroup: the loads of a view are issued together)
                pk[u] = l0 + u < n_lm ? peaks[size_t(n) * n_lm + l0 + u] : 0.0f;
                h[u] = 0.0f;
                if (hs_peak_counts(pk[u])) h[u] = at[size_t(u) * BP_PLANE];
            }
#pragma unroll
            for (int u = 0; u < BP_LM; ++u) sum[u] = sum[u] + sb_term(h[u], pk[u]);  // (+ 0.0 where the plane does not count)
        }
    }
#pragma unroll
    for (int u = 0; u < BP_LM; ++u)
        if (l0 + u < n_lm) score[size_t(v) * n_lm + l0 + u] = sb_score(sum[u], n_vis);
    if (n_vis_out && blockIdx.y == 0) n_vis_out[v] = n_vis;
}

__global__ __launch_bounds__(256) void backproject_paint_kernel(const float* __restrict__ score, int n_verts, int n_lm,
                                                                const uint8_t* __restrict__ sel, const uint8_t* __restrict__ lm_rgb,
                                                                const uchar4* __restrict__ colors, const float* __restrict__ uvs,
                                                                const uint8_t* __restrict__ tex, int tex_w, int tex_h, double floor_,
                                                                double opacity, uint32_t* __restrict__ out,
                                                                unsigned long long* __restrict__ keys) {
    __shared__ float s_score[256][BP_PAINT_LM + 1];  // (+ 1: a row walk and a column walk both meet every bank once)
    __shared__ unsigned long long s_key[8][BP_PAINT_LM];
    const int tid = threadIdx.x;
    const int v0 = blockIdx.x * 256;
    const int nv = n_verts - v0 < 256 ? n_verts - v0 : 256;
    const int col = tid & (BP_PAINT_LM - 1), part = tid / BP_PAINT_LM;  // the column walk: 8 parts of 32 vertices
    float best = -1.0f;
    int best_l = -1;
    for (int base = 0; base < n_lm; base += BP_PAINT_LM) {
        const int cnt = n_lm - base < BP_PAINT_LM ? n_lm - base : BP_PAINT_LM;
        __syncthreads();  // (the previous round's walks are over)
        for (int q = tid; q < nv * cnt; q += 256) {
            const int vl = q / cnt, k = q - vl * cnt;
            s_score[vl][k] = score[size_t(v0 + vl) * n_lm + base + k];
        }
        __syncthreads();
        if (tid < nv)
            for (int k = 0; k < cnt; ++k) {  // ascending landmarks, a later one must be larger: the lowest index wins a tie
                if (sel && !sel[base + k]) continue;
                const float s = s_score[tid][k];
                if (s > best) {
                    best = s;
                    best_l = base + k;
                }
            }
        unsigned long long key = SB_KEY_NONE;
        if (col < cnt) {
            const int hi = part * 32 + 32 < nv ? part * 32 + 32 : nv;
            for (int vl = part * 32; vl < hi; ++vl) {
                const float s = s_score[vl][col];
                if (s > 0.0f) {
                    const unsigned long long c = sb_key(s, uint32_t(v0 + vl));
                    key = c > key ? c : key;
                }
            }
        }
        s_key[part][col] = key;
        __syncthreads();
        if (tid < cnt) {
            unsigned long long top = s_key[0][tid];
            for (int p = 1; p < 8; ++p) top = s_key[p][tid] > top ? s_key[p][tid] : top;
            if (top != SB_KEY_NONE) atomicMax(&keys[base + tid], top);
        }
    }
    if (tid >= nv) return;
    const int v = v0 + tid;
    uint32_t rgb = SB_BASE_GREY;
    if (colors) {
        const uchar4 c = colors[v];
        rgb = uint32_t(c.x) | (uint32_t(c.y) << 8) | (uint32_t(c.z) << 16);
    } else if (tex && uvs) {
        const uint8_t* const t = tex + size_t(rm_texel(uvs[2 * size_t(v)], uvs[2 * size_t(v) + 1], tex_w, tex_h)) * 3;
        rgb = uint32_t(t[0]) | (uint32_t(t[1]) << 8) | (uint32_t(t[2]) << 16);
    }
    if (best_l >= 0 && double(best) > floor_) {
        const uint32_t c = lm_rgb ? uint32_t(lm_rgb[3 * best_l]) | (uint32_t(lm_rgb[3 * best_l + 1]) << 8) | (uint32_t(lm_rgb[3 * best_l + 2]) << 16)
                                  : HS_RED;
        rgb = hs_blend_rgb(rgb, c, hs_alpha(double(best), floor_, opacity));
    }
    out[v] = rgb | 0xFF000000u;  // r g b 255: the uchar4 the landmark view's tile kernel loads
}

__global__ void backproject_peaks_kernel(const unsigned long long* __restrict__ keys, int n_lm, int32_t* __restrict__ peak_vertex,
                                         float* __restrict__ peak_score) {
    const int l = blockIdx.x * 256 + int(threadIdx.x);
    if (l >= n_lm) return;
    const unsigned long long k = keys[l];
    peak_vertex[l] = sb_key_vertex(k);
    peak_score[l] = k == SB_KEY_NONE ? 0.0f : sb_key_score(k);
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

// Checks the arguments - a bad one returns an error and launches nothing - then enqueues peak, score, paint and peaks.
extern "C" int mvlm_surface_heat(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_dev, const float* images_dev,
                                 const float* heat_dev, int n_views, int n_lm, const uint8_t* sel_host, const uint8_t* lm_rgb_host,
                                 double floor_, double opacity, int depth_tol, uint8_t* vert_rgba_dev, float* score_dev,
                                 int32_t* n_vis_dev, int32_t* peak_vertex_dev, float* peak_score_dev) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    ctx->backproject_clock.invalidate();
    MVLM_REQUIRE(ctx, mesh && rot_dev && images_dev && heat_dev && vert_rgba_dev && peak_vertex_dev && peak_score_dev,
                 "surface heat: null pointer");
    MVLM_REQUIRE(ctx, mesh->n_verts > 0, "surface heat: empty mesh");
    MVLM_REQUIRE(ctx, mesh->n_tris > 0, "surface heat: a point cloud is not supported here (the mesh has no triangles)");
    MVLM_REQUIRE(ctx, aligned(heat_dev, 16), "surface heat: the heatmaps must be 16-byte aligned");
    MVLM_REQUIRE(ctx, aligned(images_dev, 16), "surface heat: the images must be 16-byte aligned");
    MVLM_REQUIRE(ctx, aligned(rot_dev, 8), "surface heat: the rotations must be 8-byte aligned");
    MVLM_REQUIRE(ctx, aligned(vert_rgba_dev, 4) && aligned(score_dev, 4) && aligned(n_vis_dev, 4) && aligned(peak_vertex_dev, 4) &&
                          aligned(peak_score_dev, 4),
                 "surface heat: the outputs must be 4-byte aligned");
    MVLM_REQUIRE(ctx, n_views >= 1, "surface heat: at least one view (" + std::to_string(n_views) + " given)");
    MVLM_REQUIRE(ctx, n_lm >= 1 && n_lm <= HS_MAX_LANDMARKS, "surface heat: 1..65536 landmarks per call (" + std::to_string(n_lm) + " given)");
    MVLM_REQUIRE(ctx, (long long)n_views * n_lm <= HS_MAX_PLANES,
                 "surface heat: n_views * n_lm is " + std::to_string((long long)n_views * n_lm) + ", above 32768 planes per call");
    MVLM_REQUIRE(ctx, (long long)mesh->n_verts * n_lm <= SB_MAX_SCORES,
                 "surface heat: vertices * n_lm is " + std::to_string((long long)mesh->n_verts * n_lm) + ", above 268435456 scores per call");
    MVLM_REQUIRE(ctx, std::isfinite(floor_) && floor_ >= 0.0 && floor_ < 1.0, "surface heat: floor must be finite and in [0, 1)");
    MVLM_REQUIRE(ctx, std::isfinite(opacity) && opacity > 0.0 && opacity <= 1.0, "surface heat: opacity must be finite and in (0, 1]");
    MVLM_REQUIRE(ctx, depth_tol >= 0 && depth_tol <= SB_MAX_DEPTH_TOL,
                 "surface heat: depth_tol must be in 0..255 (" + std::to_string(depth_tol) + " given)");

    const int V = mesh->n_verts;
    const size_t n_planes = size_t(n_views) * n_lm;
    auto* peaks = static_cast<float*>(ctx->get_scratch("backproject.peaks", n_planes * sizeof(float)));
    auto* keys = static_cast<unsigned long long*>(ctx->get_scratch("backproject.keys", size_t(n_lm) * sizeof(unsigned long long)));
    float* score = score_dev ? score_dev : static_cast<float*>(ctx->get_scratch("backproject.score", size_t(V) * n_lm * sizeof(float)));
    MVLM_REQUIRE(ctx, peaks && keys && score, "surface heat: scratch allocation failed");
    uint8_t *sel = nullptr, *lm_rgb = nullptr;
    if (sel_host) {
        sel = static_cast<uint8_t*>(ctx->get_scratch("backproject.sel", size_t(n_lm)));
        MVLM_REQUIRE(ctx, sel, "surface heat: scratch allocation failed");
    }
    if (lm_rgb_host) {
        lm_rgb = static_cast<uint8_t*>(ctx->get_scratch("backproject.lm_rgb", size_t(n_lm) * 3));
        MVLM_REQUIRE(ctx, lm_rgb, "surface heat: scratch allocation failed");
    }
    StageClock& clock = ctx->backproject_clock;
    if (clock.arm(ctx, 4)) return 1;
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;  // the upload runs on a stream of its own
    hipStream_t st = ctx->stream;
    if (sel) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(sel, sel_host, size_t(n_lm), hipMemcpyHostToDevice, st));
    if (lm_rgb) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(lm_rgb, lm_rgb_host, size_t(n_lm) * 3, hipMemcpyHostToDevice, st));
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(keys, 0, size_t(n_lm) * sizeof(unsigned long long), st));  // SB_KEY_NONE
    if (clock.record(ctx, 0, st)) return 1;
    mvlm_heat_launch_peaks(ctx, heat_dev, int(n_planes), peaks);
    if (clock.record(ctx, 1, st)) return 1;
    hipLaunchKernelGGL(backproject_score_kernel, dim3(unsigned((V + 255) / 256), unsigned((n_lm + BP_LM - 1) / BP_LM)), dim3(256), 0, st,
                       mesh->verts, V, rot_dev, images_dev, heat_dev, peaks, n_views, n_lm, ctx->render_subpixel_bits, depth_tol, score,
                       n_vis_dev);
    if (clock.record(ctx, 2, st)) return 1;
    const bool textured = mesh->tex && mesh->uvs;
    hipLaunchKernelGGL(backproject_paint_kernel, dim3(unsigned((V + 255) / 256)), dim3(256), 0, st, score, V, n_lm, sel, lm_rgb,
                       reinterpret_cast<const uchar4*>(mesh->colors), textured ? mesh->uvs : nullptr, textured ? mesh->tex : nullptr,
                       mesh->tex_w, mesh->tex_h, floor_, opacity, reinterpret_cast<uint32_t*>(vert_rgba_dev), keys);
    hipLaunchKernelGGL(backproject_peaks_kernel, dim3(unsigned((n_lm + 255) / 256)), dim3(256), 0, st, keys, n_lm, peak_vertex_dev,
                       peak_score_dev);
    if (clock.record(ctx, 3, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    clock.mark(4);
    return 0;
}

// Gives the surface heat's scratch ("backproject.*": the peaks, the keys, the two small tables and, where a caller kept no score
// table, the scores) back to the allocator, once the stream has run what reads it; the next call allocates again.
extern "C" int mvlm_surface_heat_release(mvlm_ctx* ctx) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto it = ctx->scratch.begin(); it != ctx->scratch.end();) {
        if (it->first.rfind("backproject.", 0) == 0) {
            if (it->second.first) (void)hipFree(it->second.first);
            it = ctx->scratch.erase(it);
        } else {
            ++it;
        }
    }
    return 0;
}

// Milliseconds of the last surface heat's peak, back-projection (score) and paint (with the peaks) while mvlm_render_set_profiling
// is on; waits for the stream.
extern "C" int mvlm_surface_heat_stage_ms(mvlm_ctx* ctx, float* ms3) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms3, "surface_heat_stage_ms: null pointer");
    return ctx->backproject_clock.read(ctx, 3, ms3, "surface_heat_stage_ms: no surface heat was computed with render profiling on");
}
