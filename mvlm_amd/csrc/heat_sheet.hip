// The heat sheet (mvlm_render_heat_sheet): every rendered view of a prediction in one picture - the view sheet's cells - with the
// network's heatmaps laid over it: per view pixel the selected landmark whose value is the largest share of its plane's peak, in
// that landmark's colour, the more opaque the nearer to the peak ("Heat sheet"; heat_sheet_math.h holds the
// arithmetic).  Heat pixel [row, col] lies over image pixel [row, col].
//
// Behind the view sheet's own background (mvlm_view_sheet_draw: its tile and fill kernels, no markers), two kernels on the
// context's stream:
//   1. peak     one workgroup per (view, landmark) plane of 65 536 floats: the largest finite value, -inf without one.  16-byte
//               loads, 1 KiB in a row per wave and load, a butterfly over the wave's 64 lanes, then LDS across the four waves
//   2. compose  one workgroup per (view, row), a thread per view pixel: the view's peaks go through LDS HEAT_CHUNK landmarks at a
//               time - a landmark that is deselected or whose peak does not count costs no load - and the winner is laid over
//               the byte triple the background left at the pixel's place in its cell
// Neither has an atomic: a value is the same whatever the scheduling.  Built as an object of its own (build/heat/,
// tests/golden/kernel_occupancy_heat.json).
#include "common.h"
#include "heat_sheet_math.h"
#include "view_sheet_math.h"

#include <cmath>

namespace {

constexpr int HEAT_PLANE = RM_SIZE * RM_SIZE;  // floats in a plane
constexpr int HEAT_CHUNK = 1024;               // landmarks whose peaks are in LDS at a time
constexpr int HEAT_UNROLL = 8;                 // planes a thread has loads in flight for
static_assert(HEAT_CHUNK % HEAT_UNROLL == 0 && HEAT_PLANE % (4 * 256) == 0, "whole rounds");

__device__ inline float heat_counted(float v) { return hs_finite(v) ? v : -INFINITY; }

__global__ __launch_bounds__(256) void heat_peak_kernel(const float4* __restrict__ heat, float* __restrict__ peaks) {
    __shared__ float s_wave[4];
    const int tid = threadIdx.x;
    const float4* const plane = heat + size_t(blockIdx.x) * (HEAT_PLANE / 4);
    float m = -INFINITY;
#pragma unroll 8
    for (int it = 0; it < HEAT_PLANE / 4 / 256; ++it) {
        const float4 v = plane[it * 256 + tid];
        m = fmaxf(fmaxf(m, heat_counted(v.x)), fmaxf(heat_counted(v.y), fmaxf(heat_counted(v.z), heat_counted(v.w))));
    }
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) s_wave[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) peaks[blockIdx.x] = fmaxf(fmaxf(s_wave[0], s_wave[1]), fmaxf(s_wave[2], s_wave[3]));
}

__global__ __launch_bounds__(256) void heat_compose_kernel(const float* __restrict__ heat, const float* __restrict__ peaks,
                                                           const uint8_t* __restrict__ sel, const uint8_t* __restrict__ lm_rgb, int n_lm,
                                                           int cols, int scale, int gap, int width, double floor_, double opacity,
                                                           uint32_t* __restrict__ out) {
    __shared__ float s_peak[HEAT_CHUNK];  // a candidate's peak; 0: deselected, or a peak that does not count
    const int view = blockIdx.y, y = blockIdx.x, x = threadIdx.x;
    const float* const pixel = heat + size_t(view) * n_lm * HEAT_PLANE + size_t(y) * RM_SIZE + size_t(x);  // in plane 0 of the view
    double best_t = -INFINITY;
    int best_l = -1;
    for (int base = 0; base < n_lm; base += HEAT_CHUNK) {
        const int n = n_lm - base < HEAT_CHUNK ? n_lm - base : HEAT_CHUNK;
        const int n_round = (n + HEAT_UNROLL - 1) / HEAT_UNROLL * HEAT_UNROLL;
        __syncthreads();  // (the previous chunk's walk is over)
        for (int k = x; k < n_round; k += 256) {
            float m = 0.0f;
            if (k < n && (!sel || sel[base + k])) {
                const float p = peaks[size_t(view) * n_lm + base + k];
                m = hs_peak_counts(p) ? p : 0.0f;
            }
            s_peak[k] = m;
        }
        __syncthreads();
        for (int k = 0; k < n_round; k += HEAT_UNROLL) {
            float m[HEAT_UNROLL], h[HEAT_UNROLL];
#pragma unroll
            for (int u = 0; u < HEAT_UNROLL; ++u) {  // (m is the same for the whole workgroup: the loads of a round are issued together)
                m[u] = s_peak[k + u];
                h[u] = 0.0f;
                if (m[u] > 0.0f) h[u] = pixel[size_t(base + k + u) * HEAT_PLANE];
            }
#pragma unroll
            for (int u = 0; u < HEAT_UNROLL; ++u) {  // ascending landmarks, a later one must be larger: the lowest index wins a tie
                if (!(m[u] > 0.0f) || !hs_finite(h[u])) continue;
                const double t = hs_share(h[u], m[u]);
                if (t > best_t) {
                    best_t = t;
                    best_l = base + k + u;
                }
            }
        }
    }
    if (best_l < 0 || !(best_t > floor_)) return;  // the background stays

    const int side = RM_SIZE * scale;
    const size_t px = size_t(gap) + size_t(view % cols) * size_t(side + gap) + size_t(x) * scale;
    const size_t py = size_t(gap) + size_t(view / cols) * size_t(side + gap) + size_t(y) * scale;
    const uint32_t bg = out[py * size_t(width) + px];  // (every sheet pixel of this view pixel holds the same bytes)
    const uint32_t col = lm_rgb ? uint32_t(lm_rgb[3 * best_l]) | (uint32_t(lm_rgb[3 * best_l + 1]) << 8) | (uint32_t(lm_rgb[3 * best_l + 2]) << 16)
                                : HS_RED;
    const uint32_t rgba = hs_blend_rgb(bg, col, hs_alpha(best_t, floor_, opacity)) | 0xFF000000u;
    for (int dy = 0; dy < scale; ++dy)
        for (int dx = 0; dx < scale; ++dx) out[(py + dy) * size_t(width) + px + dx] = rgba;
}

}  // namespace

// The peak kernel's launch on the context's stream, for an entry point that holds the context and has checked its arguments (this
// file's two, and the surface heat: surface_backproject.hip).
void mvlm_heat_launch_peaks(mvlm_ctx* ctx, const float* heat_dev, int n_planes, float* peaks_dev) {
    hipLaunchKernelGGL(heat_peak_kernel, dim3(unsigned(n_planes)), dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(heat_dev),
                       peaks_dev);
}

extern "C" int mvlm_heat_plane_peaks(mvlm_ctx* ctx, const float* heat_dev, int n_planes, float* peaks_dev) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, heat_dev && peaks_dev, "heat sheet: null pointer");
    MVLM_REQUIRE(ctx, reinterpret_cast<uintptr_t>(heat_dev) % 16 == 0, "heat sheet: the heatmaps must be 16-byte aligned");
    MVLM_REQUIRE(ctx, n_planes >= 1 && n_planes <= HS_MAX_PLANES, "heat sheet: 1..32768 planes per call (" + std::to_string(n_planes) + " given)");
    mvlm_heat_launch_peaks(ctx, heat_dev, n_planes, peaks_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

// Checks the arguments - a bad one returns an error and launches nothing - then draws the views alone and lays the heat over them.
extern "C" int mvlm_render_heat_sheet(mvlm_ctx* ctx, const float* images_dev, const float* heat_dev, int n_views, int n_lm,
                                      const uint8_t* sel_host, const uint8_t* lm_rgb_host, int background, int cols_in, int scale, int gap,
                                      double floor_, double opacity, uint8_t* out_dev) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    ctx->heat_clock.invalidate();
    MVLM_REQUIRE(ctx, images_dev && heat_dev && out_dev, "heat sheet: null pointer");
    MVLM_REQUIRE(ctx, reinterpret_cast<uintptr_t>(heat_dev) % 16 == 0, "heat sheet: the heatmaps must be 16-byte aligned");
    int cols = 0, rows = 0, width = 0, height = 0;
    char why[512];
    if (mvlm_view_sheet_layout(n_views, cols_in, scale, gap, &cols, &rows, &width, &height, why, int(sizeof(why))) != 0)
        return ctx->fail(std::string("heat sheet: ") + why);
    MVLM_REQUIRE(ctx, background == 0 || background == 1, "heat sheet: background must be 0 (rgb) or 1 (depth)");
    MVLM_REQUIRE(ctx, n_lm >= 1 && n_lm <= HS_MAX_LANDMARKS, "heat sheet: 1..65536 landmarks per call (" + std::to_string(n_lm) + " given)");
    MVLM_REQUIRE(ctx, (long long)n_views * n_lm <= HS_MAX_PLANES,
                 "heat sheet: n_views * n_lm is " + std::to_string((long long)n_views * n_lm) + ", above 32768 planes per call");
    MVLM_REQUIRE(ctx, std::isfinite(floor_) && floor_ >= 0.0 && floor_ < 1.0, "heat sheet: floor must be finite and in [0, 1)");
    MVLM_REQUIRE(ctx, std::isfinite(opacity) && opacity > 0.0 && opacity <= 1.0, "heat sheet: opacity must be finite and in (0, 1]");

    const size_t n_planes = size_t(n_views) * n_lm;
    auto* peaks = static_cast<float*>(ctx->get_scratch("heat.peaks", n_planes * sizeof(float)));
    MVLM_REQUIRE(ctx, peaks, "heat sheet: scratch allocation failed");
    uint8_t *sel = nullptr, *lm_rgb = nullptr;
    if (sel_host) {
        sel = static_cast<uint8_t*>(ctx->get_scratch("heat.sel", size_t(n_lm)));
        MVLM_REQUIRE(ctx, sel, "heat sheet: scratch allocation failed");
    }
    if (lm_rgb_host) {
        lm_rgb = static_cast<uint8_t*>(ctx->get_scratch("heat.lm_rgb", size_t(n_lm) * 3));
        MVLM_REQUIRE(ctx, lm_rgb, "heat sheet: scratch allocation failed");
    }
    StageClock& clock = ctx->heat_clock;
    if (clock.arm(ctx, 4)) return 1;
    hipStream_t st = ctx->stream;
    if (clock.record(ctx, 0, st)) return 1;
    // the views alone: the view sheet's own code (the marker radius is not read without maxima)
    if (mvlm_view_sheet_draw(ctx, images_dev, n_views, nullptr, 0, nullptr, nullptr, nullptr, nullptr, background, cols_in, scale, gap,
                             VS_RADIUS_MIN, out_dev))
        return 1;
    if (sel) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(sel, sel_host, size_t(n_lm), hipMemcpyHostToDevice, st));
    if (lm_rgb) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(lm_rgb, lm_rgb_host, size_t(n_lm) * 3, hipMemcpyHostToDevice, st));
    if (clock.record(ctx, 1, st)) return 1;
    mvlm_heat_launch_peaks(ctx, heat_dev, int(n_planes), peaks);
    if (clock.record(ctx, 2, st)) return 1;
    hipLaunchKernelGGL(heat_compose_kernel, dim3(RM_SIZE, unsigned(n_views)), dim3(256), 0, st, heat_dev, peaks, sel, lm_rgb, n_lm, cols,
                       scale, gap, width, floor_, opacity, reinterpret_cast<uint32_t*>(out_dev));
    if (clock.record(ctx, 3, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    clock.mark(4);
    return 0;
}

// Milliseconds of the last heat sheet's background, peak and compose while mvlm_render_set_profiling is on; waits for the stream.
extern "C" int mvlm_heat_sheet_stage_ms(mvlm_ctx* ctx, float* ms3) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms3, "heat_sheet_stage_ms: null pointer");
    return ctx->heat_clock.read(ctx, 3, ms3, "heat_sheet_stage_ms: no heat sheet was drawn with render profiling on");
}
