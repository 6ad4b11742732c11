// Device code the landmark view's tile kernel (raster_view.hip: view_tile_kernel) and the ray view's (raster_rays.hip:
// rays_tile_kernel) have in common - resolve the tile's big triangles, shade the mesh's winner, compact and walk the spheres, count
// the winners - and the handles of the stages in front of them (mvlm_view_launch_stages, raster_view.hip), which both launch sets
// call.  The kernels of those stages stay in raster_view.hip.
#ifndef MVLM_RASTER_VIEW_TILE_H
#define MVLM_RASTER_VIEW_TILE_H

#include "raster_common.h"
#include "raster_view_math.h"

namespace {

static_assert(sizeof(rv_sphere) == 32 && alignof(rv_sphere) == 16, "the tile kernel moves a sphere as two 16-byte words");
constexpr int VIEW_SPHERE_CAP = 256;   // spheres in a tile's LDS list at a time: one candidate per thread and round
constexpr int VIEW_COUNT_SPAN = 1024;  // landmarks whose per-tile pixel counts are held in LDS at a time

struct view_frame {  // per view: the window's centre in view space, model units from centre to border, pixels per model unit
    float cx, cy, half, k;
};

__device__ inline rm_tri view_load_tri(const vert12* tvv, const int32_t* tris, int t, int size) {
    return rv_setup(load_vert(tvv, tris[3 * t]), load_vert(tvv, tris[3 * t + 1]), load_vert(tvv, tris[3 * t + 2]), size);
}

// ---- the tile's big triangles, set up into LDS a chunk at a time: the best key of pixel (i, j) ----
__device__ __forceinline__ uint64_t view_tile_resolve(uint64_t best, const vert12* tvv, const int32_t* __restrict__ tris,
                                                      const int* list, int n, int size, int i, int j, int tid, rm_tri* s_tri,
                                                      int* s_id) {
    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if (tid < m) {
            const int t = list[base + tid];
            s_id[tid] = t;
            s_tri[tid] = view_load_tri(tvv, tris, t, size);
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const rm_tri* t = &s_tri[k];
            if (i < t->ix0 || i > t->ix1 || j < t->iy0 || j > t->iy1) continue;
            float b0, b1, b2;
            if (!rm_cover(t, i, j, &b0, &b1, &b2)) continue;
            const float z = rm_interp(b0, b1, b2, t->z0, t->z1, t->z2);
            if (!(z >= 0.0f && z <= 1.0f)) continue;  // near / far clip
            const uint64_t key = rm_key(z, uint32_t(s_id[k]));
            best = key < best ? key : best;
        }
    }
    return best;
}

// ---- shade the mesh's winner: the byte mvlm_render divides by 255; *zbest: its depth, +inf where no triangle covers the pixel ----
__device__ __forceinline__ uint32_t view_tile_shade(uint64_t best, const vert12* tvv, const int32_t* __restrict__ tris,
                                                    const float* __restrict__ uvs, const uint8_t* __restrict__ tex, int tex_w,
                                                    int tex_h, const uchar4* __restrict__ colors, int shading,
                                                    const view_frame& frame, int size, int i, int j, float* zbest_out) {
    uint32_t rgb = 0xFFFFFFu;  // white background
    float zbest = INFINITY;    // depth the spheres are tested against: +inf where no triangle covers the pixel
    if (best != RM_KEY_EMPTY) {
        const int t = int(rm_key_tri(best));
        int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
        const rm_tri tr = rv_setup(load_vert(tvv, a), load_vert(tvv, b), load_vert(tvv, c), size);
        float b0 = 0.f, b1 = 0.f, b2 = 0.f;
        rm_cover(&tr, i, j, &b0, &b1, &b2);
        if (tr.swapped) {
            const int s = b;
            b = c;
            c = s;
        }
        if (shading == 1) {
            const uint32_t g = uint32_t(rv_geometry_u8(&tr, rv_geometry_kz(size, frame.half)));
            rgb = g | (g << 8) | (g << 16);
        } else if (colors) {
            rgb = vertex_colour(colors, a, b, c, b1, b2);
        } else if (tex && uvs) {
            const float u = rm_interp(b0, b1, b2, uvs[2 * a], uvs[2 * b], uvs[2 * c]);
            const float v = rm_interp(b0, b1, b2, uvs[2 * a + 1], uvs[2 * b + 1], uvs[2 * c + 1]);
            rgb = fetch_texel(tex, u, v, tex_w, tex_h);
        }
        zbest = rm_key_z(best);
    }
    *zbest_out = zbest;
    return rgb;
}

// ---- spheres: drawn after the mesh (they win ties), in landmark order (the later one wins an equal depth) ----
// `spheres`: every view's n_lm records; -> the winning landmark or -1
__device__ __forceinline__ int view_tile_spheres(const rv_sphere* __restrict__ spheres, int view, int n_lm, int tx0, int ty0, int i, int j,
                                                 int tid, const view_frame& frame, rv_sphere* s_sph, int* s_sph_id, int* s_wave,
                                                 float* zbest_io, uint32_t* rgb_io) {
    float zbest = *zbest_io;
    uint32_t rgb = *rgb_io;
    int win = -1;
    for (int base = 0; base < n_lm; base += VIEW_SPHERE_CAP) {
        const int cand = base + tid;
        bool touch = false;
        uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;  // the record as two 16-byte words: X Y z R | rgb, x box, y box, pad
        if (cand < n_lm) {
            const uint4* const src = reinterpret_cast<const uint4*>(spheres + size_t(view) * n_lm + cand);
            w0 = src[0];
            w1 = src[1];
            const int ix0 = short(w1.y & 0xFFFFu), ix1 = short(w1.y >> 16), iy0 = short(w1.z & 0xFFFFu), iy1 = short(w1.z >> 16);
            touch = ix0 <= tx0 + RM_TILE - 1 && ix1 >= tx0 && iy0 <= ty0 + RM_TILE - 1 && iy1 >= ty0;
        }
        const unsigned long long m = __ballot(touch);
        const int wave = tid >> 6, lane = tid & 63;
        __syncthreads();  // (the previous round's walk is over)
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;  // (as in rays_tile_kernel; why this is not a shared helper: raster_bins.h)
        for (int w = 0; w < 4; ++w) {
            off += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (touch) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
            uint4* const dst = reinterpret_cast<uint4*>(&s_sph[pos]);
            dst[0] = w0;
            dst[1] = w1;
            s_sph_id[pos] = cand;
        }
        __syncthreads();
        for (int q = 0; q < total; ++q) {
            float zs, shade;
            if (!rv_sphere_fragment(&s_sph[q], i, j, frame.k, &zs, &shade)) continue;
            if (!(zs <= zbest)) continue;
            zbest = zs;
            win = s_sph_id[q];
            rgb = rv_sphere_colour(s_sph[q].rgb, shade);
        }
    }
    *zbest_io = zbest;
    *rgb_io = rgb;
    return win;
}

// ---- pixels each landmark's sphere won in this tile, added to the view's counts ----
__device__ __forceinline__ void view_tile_count(int* __restrict__ lm_pixels, int view, int n_lm, int win, int tid, int* s_cnt) {
    if (lm_pixels && n_lm > 0 && __syncthreads_or(win >= 0)) {
        for (int base = 0; base < n_lm; base += VIEW_COUNT_SPAN) {
            for (int q = tid; q < VIEW_COUNT_SPAN; q += 256) s_cnt[q] = 0;
            __syncthreads();
            if (win >= base && win < base + VIEW_COUNT_SPAN) atomicAdd(&s_cnt[win - base], 1);
            __syncthreads();
            for (int q = tid; q < VIEW_COUNT_SPAN && base + q < n_lm; q += 256)
                if (s_cnt[q]) atomicAdd(&lm_pixels[size_t(view) * n_lm + base + q], s_cnt[q]);
            __syncthreads();
        }
    }
}

}  // namespace

// What mvlm_view_launch_stages leaves for the tile kernel that follows it (device pointers into the context's "view.*" scratch).
struct mvlm_view_stages {
    const vert12* tv;
    const view_frame* frames;
    const double* rot;
    raster_bins bins;  // counters, offsets, lists and the overflow flag (raster_bins.h)
    const unsigned long long* keys;
    const rv_sphere* spheres;  // null when n_lm == 0
    const uint8_t* vcol;       // the per-vertex colours the tile stage shades with, or null
};
// raster_view.hip: scratch, copies, fills and the kernels of the mesh stages (transform, classify, scan, bin fill) and of the
// landmark projection, for a launch set that holds the context and has checked its arguments; `what` starts its error messages.
// Under render profiling it arms ctx->view_clock and records its events 0..6; the caller records the rest and marks the clock.
int mvlm_view_launch_stages(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                            const float* frames_host, const double* landmarks_host, int n_lm, float radius,
                            const uint8_t* lm_rgb_host, int32_t* lm_pixels_dev, const char* what, mvlm_view_stages* out);

#endif
