// The view sheet (mvlm_render_view_sheet): every rendered view of a prediction in one picture, with the network's 2-D prediction of
// every landmark drawn on it as a marker and, when the landmarks are given, the residual from the marker to where the consensus
// landmark projects in that view - the reference's Predictor2D.draw_image_with_landmarks for all views at once, on the stack as
// it lies on the device ("View sheet"; view_sheet_math.h holds the arithmetic).
//
// Three kernels on the context's stream:
//   1. project  one thread per (view, landmark): the 48-byte record - marker, residual end, colour, flags, pixel box in the cell
//   2. tile     one workgroup per (view, 16 x 16 tile of its cell), a thread per sheet pixel: fetches the background, compacts the
//               view's records whose box touches the tile into LDS (ballots, SHEET_CAP candidates a round, any number of rounds,
//               as view_tile_spheres of raster_view_tile.h does) and walks the list: residuals under markers, landmark order
//               within each, so a pixel does not depend on the scheduling
//   3. fill     one thread per sheet pixel: the gaps and the cells beyond the last view, grey; the cells' pixels are the tile
//               kernel's alone
// No atomics.  Built as an object of its own (build/sheet/, tests/golden/kernel_occupancy_sheet.json).
#include "common.h"
#include "view_sheet_math.h"

#include <cmath>

namespace {

static_assert(sizeof(vs_record) == 48 && alignof(vs_record) == 16, "the tile kernel moves a record as three 16-byte words");
constexpr int SHEET_CAP = 256;  // records in a tile's LDS list at a time: one candidate per thread and round

__global__ __launch_bounds__(256) void sheet_project_kernel(const float* __restrict__ maxima, const double* __restrict__ rot,
                                                            const double* __restrict__ landmarks, const uint8_t* __restrict__ lm_rgb,
                                                            const uint8_t* __restrict__ used, int n_lm, int n_views, int scale,
                                                            double radius, vs_record* __restrict__ records) {
    const int q = blockIdx.x * 256 + int(threadIdx.x);
    if (q >= n_views * n_lm) return;
    const int view = q / n_lm, l = q % n_lm;
    const float* const mx = maxima + (size_t(l) * n_views + view) * 3;  // [NL,N,3]: a, b, score
    const bool residual = rot && landmarks;
    double m[9], p[3];
    for (int k = 0; k < 9; ++k) m[k] = residual ? rot[view * 9 + k] : 0.0;
    for (int k = 0; k < 3; ++k) p[k] = residual ? landmarks[3 * l + k] : 0.0;
    const uint32_t rgb = lm_rgb ? uint32_t(lm_rgb[3 * l]) | (uint32_t(lm_rgb[3 * l + 1]) << 8) | (uint32_t(lm_rgb[3 * l + 2]) << 16)
                                : VS_BLUE;
    const int u = used ? int(used[size_t(l) * n_views + view]) : 1;
    records[q] = vs_project(mx[0], mx[1], mx[2], m, p, residual, rgb, u, scale, radius);
}

__global__ __launch_bounds__(256) void sheet_tile_kernel(const float4* __restrict__ images, const vs_record* __restrict__ records,
                                                         int n_lm, int cols, int scale, int gap, int width, int background,
                                                         double radius, uint32_t* __restrict__ out) {
    __shared__ vs_record s_rec[SHEET_CAP];
    __shared__ int s_wave[4];
    const int view = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tiles_x = RM_SIZE / RM_TILE * scale;
    const int tx0 = (tile % tiles_x) * RM_TILE, ty0 = (tile / tiles_x) * RM_TILE;
    const int i = tx0 + (tid & (RM_TILE - 1)), j = ty0 + tid / RM_TILE;  // the pixel in its cell

    const float4 px = images[(size_t(view) * RM_SIZE + size_t(j / scale)) * RM_SIZE + size_t(i / scale)];
    uint32_t rgb;
    if (background == 1) {
        const uint32_t g = vs_byte(px.w);
        rgb = g | (g << 8) | (g << 16);
    } else {
        rgb = vs_byte(px.x) | (vs_byte(px.y) << 8) | (vs_byte(px.z) << 16);
    }

    bool residual = false, marked = false;
    uint32_t marker_rgb = 0;
    for (int base = 0; base < n_lm; base += SHEET_CAP) {
        const int cand = base + tid;
        bool touch = false;
        uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0;  // mx my | ex ey | rgb, flags, x box, y box
        if (cand < n_lm) {
            const uint4* const src = reinterpret_cast<const uint4*>(records + size_t(view) * n_lm + cand);
            w0 = src[0];
            w1 = src[1];
            w2 = src[2];
            const int ix0 = short(w2.z & 0xFFFFu), ix1 = short(w2.z >> 16), iy0 = short(w2.w & 0xFFFFu), iy1 = short(w2.w >> 16);
            touch = w2.y != 0u && ix0 <= tx0 + RM_TILE - 1 && ix1 >= tx0 && iy0 <= ty0 + RM_TILE - 1 && iy1 >= ty0;
        }
        const unsigned long long m = __ballot(touch);
        const int wave = tid >> 6, lane = tid & 63;
        __syncthreads();  // (the previous round's walk is over)
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            off += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (touch) {
            uint4* const dst = reinterpret_cast<uint4*>(&s_rec[off + __popcll(m & ((1ull << lane) - 1ull))]);
            dst[0] = w0;
            dst[1] = w1;
            dst[2] = w2;
        }
        __syncthreads();
        for (int q = 0; q < total; ++q) {  // (landmark order: the compaction keeps it)
            const vs_record* const r = &s_rec[q];
            if (i < r->ix0 || i > r->ix1 || j < r->iy0 || j > r->iy1) continue;
            if ((r->flags & VS_SEGMENT) && vs_segment_covers(r, i, j, scale)) residual = true;
            if ((r->flags & VS_MARKER) && vs_marker_covers(r, i, j, scale, radius)) {
                marked = true;
                marker_rgb = r->rgb;
            }
        }
    }
    if (residual) rgb = VS_RED;
    if (marked) rgb = marker_rgb;

    // RGBA, alpha 255: one aligned 4-byte store per pixel, 64 bytes in a row per tile row
    const int side = RM_SIZE * scale;
    const size_t x = size_t(gap) + size_t(view % cols) * size_t(side + gap) + size_t(i);
    const size_t y = size_t(gap) + size_t(view / cols) * size_t(side + gap) + size_t(j);
    out[y * size_t(width) + x] = rgb | 0xFF000000u;
}

__global__ __launch_bounds__(256) void sheet_fill_kernel(int n_views, int cols, int scale, int gap, int width, int height,
                                                         uint32_t* __restrict__ out) {
    const size_t g = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (g >= size_t(width) * size_t(height)) return;
    const int x = int(g % size_t(width)), y = int(g / size_t(width));
    const int period = RM_SIZE * scale + gap;  // a gap and the cell behind it
    const bool in_gap = x % period < gap || y % period < gap;
    if (!in_gap && (y / period) * cols + x / period < n_views) return;  // a view's pixel: the tile kernel writes it
    out[g] = VS_GREY | 0xFF000000u;
}

void layout_words(int code, int n_views, int cols_in, int scale, int gap, int cols, int rows, int width, int height, std::string& why) {
    switch (code) {
    case VS_BAD_VIEWS: why = "n_views must be 1..65536 (" + std::to_string(n_views) + " given)"; break;
    case VS_BAD_COLS: why = "cols must be at least 1 (" + std::to_string(cols_in) + " given)"; break;
    case VS_BAD_SCALE: why = "scale must be 1..4 (" + std::to_string(scale) + " given)"; break;
    case VS_BAD_GAP: why = "gap must be 0..16 (" + std::to_string(gap) + " given)"; break;
    case VS_TOO_LARGE: {
        int best = 0, c, r, w, h;
        for (int s = VS_MAX_SCALE; s >= 1 && !best; --s)
            if (vs_layout(n_views, cols_in, s, gap, &c, &r, &w, &h) == VS_OK) best = s;
        why = std::to_string(n_views) + " views in " + std::to_string(cols) + " columns and " + std::to_string(rows) + " rows at scale " +
              std::to_string(scale) + " make a sheet of " + std::to_string(width) + " x " + std::to_string(height) +
              " pixels, above 4096 a side: " +
              (best ? "the largest scale that fits is " + std::to_string(best) : std::string("no scale fits this many columns and rows"));
        break;
    }
    default: why.clear();
    }
}

}  // namespace

// Host only: no context, no GPU.
extern "C" int mvlm_view_sheet_layout(int n_views, int cols_in, int scale, int gap, int* cols, int* rows, int* width, int* height,
                                      char* why, int why_len) {
    int c = 0, r = 0, w = 0, h = 0;
    const int code = vs_layout(n_views, cols_in, scale, gap, &c, &r, &w, &h);
    if (why && why_len > 0) {
        std::string words;
        layout_words(code, n_views, cols_in, scale, gap, c, r, w, h, words);
        std::snprintf(why, size_t(why_len), "%s", words.c_str());
    }
    if (code != VS_OK) return code;
    if (cols) *cols = c;
    if (rows) *rows = r;
    if (width) *width = w;
    if (height) *height = h;
    return 0;
}

// Checks the arguments - a bad one returns an error and launches nothing - then copies the small host tables and launches.  The
// caller has entered the context: mvlm_render_view_sheet, and mvlm_render_heat_sheet (heat_sheet.hip) for its background.
int mvlm_view_sheet_draw(mvlm_ctx* ctx, const float* images_dev, int n_views, const float* maxima_dev, int n_lm, const double* rot_host,
                         const double* landmarks_host, const uint8_t* lm_rgb_host, const uint8_t* used_host, int background, int cols_in,
                         int scale, int gap, double marker_radius, uint8_t* out_dev) {
    MVLM_REQUIRE(ctx, images_dev && out_dev, "view sheet: bad arguments");
    int cols = 0, rows = 0, width = 0, height = 0;
    const int code = vs_layout(n_views, cols_in, scale, gap, &cols, &rows, &width, &height);
    if (code != VS_OK) {
        std::string words;
        layout_words(code, n_views, cols_in, scale, gap, cols, rows, width, height, words);
        return ctx->fail("view sheet: " + words);
    }
    MVLM_REQUIRE(ctx, background == 0 || background == 1, "view sheet: background must be 0 (rgb) or 1 (depth)");
    MVLM_REQUIRE(ctx, std::isfinite(marker_radius) && marker_radius >= VS_RADIUS_MIN && marker_radius <= VS_RADIUS_MAX,
                 "view sheet: marker_radius must be finite and in 0.5..16");
    MVLM_REQUIRE(ctx, n_lm >= 0 && n_lm <= VS_MAX_LANDMARKS,
                 "view sheet: 0..65536 landmarks per call (" + std::to_string(n_lm) + " given)");
    if (!maxima_dev) n_lm = 0;  // nothing to mark: the views alone
    const bool residual = n_lm > 0 && rot_host && landmarks_host;
    if (residual)
        for (int k = 0; k < n_views * 9; ++k) MVLM_REQUIRE(ctx, std::isfinite(rot_host[k]), "view sheet: non-finite rotation");

    vs_record* records = nullptr;
    double *rot = nullptr, *lm = nullptr;
    uint8_t *lm_rgb = nullptr, *used = nullptr;
    hipStream_t st = ctx->stream;
    if (n_lm > 0) {
        records = static_cast<vs_record*>(ctx->get_scratch("sheet.records", size_t(n_views) * n_lm * sizeof(vs_record)));
        MVLM_REQUIRE(ctx, records, "view sheet: scratch allocation failed");
        if (residual) {
            rot = static_cast<double*>(ctx->get_scratch("sheet.rot", size_t(n_views) * 9 * sizeof(double)));
            lm = static_cast<double*>(ctx->get_scratch("sheet.lm", size_t(n_lm) * 3 * sizeof(double)));
            MVLM_REQUIRE(ctx, rot && lm, "view sheet: scratch allocation failed");
        }
        if (lm_rgb_host) {
            lm_rgb = static_cast<uint8_t*>(ctx->get_scratch("sheet.lm_rgb", size_t(n_lm) * 3));
            MVLM_REQUIRE(ctx, lm_rgb, "view sheet: scratch allocation failed");
        }
        if (used_host) {
            used = static_cast<uint8_t*>(ctx->get_scratch("sheet.used", size_t(n_lm) * n_views));
            MVLM_REQUIRE(ctx, used, "view sheet: scratch allocation failed");
        }
        if (residual) {
            MVLM_CHECK_HIP(ctx, hipMemcpyAsync(rot, rot_host, size_t(n_views) * 9 * sizeof(double), hipMemcpyHostToDevice, st));
            MVLM_CHECK_HIP(ctx, hipMemcpyAsync(lm, landmarks_host, size_t(n_lm) * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        }
        if (lm_rgb) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(lm_rgb, lm_rgb_host, size_t(n_lm) * 3, hipMemcpyHostToDevice, st));
        if (used) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(used, used_host, size_t(n_lm) * n_views, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(sheet_project_kernel, dim3(unsigned((size_t(n_views) * n_lm + 255) / 256)), dim3(256), 0, st, maxima_dev, rot,
                           lm, lm_rgb, used, n_lm, n_views, scale, marker_radius, records);
    }
    const int tiles_x = RM_SIZE / RM_TILE * scale;
    hipLaunchKernelGGL(sheet_tile_kernel, dim3(unsigned(tiles_x * tiles_x), unsigned(n_views)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(images_dev), records, n_lm, cols, scale, gap, width, background, marker_radius,
                       reinterpret_cast<uint32_t*>(out_dev));
    const size_t n_pixels = size_t(width) * size_t(height);
    hipLaunchKernelGGL(sheet_fill_kernel, dim3(unsigned((n_pixels + 255) / 256)), dim3(256), 0, st, n_views, cols, scale, gap, width,
                       height, reinterpret_cast<uint32_t*>(out_dev));
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

extern "C" int mvlm_render_view_sheet(mvlm_ctx* ctx, const float* images_dev, int n_views, const float* maxima_dev, int n_lm,
                                      const double* rot_host, const double* landmarks_host, const uint8_t* lm_rgb_host,
                                      const uint8_t* used_host, int background, int cols_in, int scale, int gap, double marker_radius,
                                      uint8_t* out_dev) {
    MVLM_ENTER(ctx);
    return mvlm_view_sheet_draw(ctx, images_dev, n_views, maxima_dev, n_lm, rot_host, landmarks_host, lm_rgb_host, used_host, background,
                                cols_in, scale, gap, marker_radius, out_dev);
}
