// Point clouds (a mesh uploaded with n_tris == 0): every point of the scan drawn as a screen-space disc - a splat - whose
// depth rises towards its rim (raster_points_math.h holds the contract, DESIGN.md 5.1 "Point clouds").  mvlm_render
// (raster.hip) branches here in host code; its triangle kernels are untouched.
//
// Two kernels, all views at once:
//   1. splat   one thread per (view, point): M*v in double -> snapped window coords + z (rm_transform), then the box of
//              candidate pixel centres (at most 17 x 17 at the largest radius, 1..4 centres on a dense scan's 0.75 px floor)
//              and per covered centre one 64-bit atomicMin of rm_key(z_pix, id) into the renderer's key plane - the case
//              "triangle of at most 16 pixel centres" of classify_kernel without the edge functions, so nothing is binned.
//              The stored key is read first: where it is already smaller the atomic is skipped (keys only ever fall during
//              a render, so a stale read costs an atomic, never a pixel).
//   2. tile    one thread per pixel: reads the key, hands the slot back EMPTY (the key plane's invariant between renders,
//              raster.hip), looks up the winner's colour and writes the RGBD texel.
// The key makes the picture independent of the order in which the atomics land.  No list can overflow here; the tile
// kernel still publishes the (zero) overflow word so that mvlm_render_check reads a fresh value.
// Built as an object of its own (build/points/, tests/golden/kernel_occupancy_points.json).
#include "raster_common.h"
#include "raster_points_math.h"

#include <algorithm>
#include <cmath>

namespace {

// COUNT: the measuring form (mvlm_points_set_counting) also counts covered-and-unclipped pixels and issued atomics
template <bool COUNT>
__global__ __launch_bounds__(256) void points_splat_kernel(const float* __restrict__ verts, int n_points,
                                                           const double* __restrict__ rot, int sub_bits, int R, float c,
                                                           unsigned long long* __restrict__ keys,
                                                           unsigned long long* __restrict__ stats) {
    const size_t view = blockIdx.y;
    const size_t p = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (p >= size_t(n_points)) return;
    const float vx = verts[3 * p], vy = verts[3 * p + 1], vz = verts[3 * p + 2];
    if (!rp_finite3(vx, vy, vz)) return;
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = rot[view * 9 + k];  // (uniform: scalar loads)
    const rm_vert o = rm_transform(m, vx, vy, vz, sub_bits);
    const rp_box b = rp_setup(o.X, o.Y, R);
    unsigned long long* const kv = keys + view * RM_SIZE * RM_SIZE;
    unsigned covered = 0, issued = 0;
    for (int j = b.iy0; j <= b.iy1; ++j)
        for (int i = b.ix0; i <= b.ix1; ++i) {
            int64_t d2;
            if (!rp_cover(o.X, o.Y, R, i, j, &d2)) continue;
            const float z = rp_depth(o.z, d2, c);
            if (!rp_clip(z)) continue;  // near / far clip (render3d.py:136)
            const unsigned long long key = rm_key(z, uint32_t(p));
            unsigned long long* const slot = &kv[j * RM_SIZE + i];
            if (COUNT) ++covered;
            if (__atomic_load_n(slot, __ATOMIC_RELAXED) <= key) continue;
            if (COUNT) ++issued;
            atomicMin(slot, key);
        }
    if (COUNT) {
        if (covered) atomicAdd(&stats[0], (unsigned long long)covered);
        if (issued) atomicAdd(&stats[1], (unsigned long long)issued);
    }
}

__global__ __launch_bounds__(256) void points_tile_kernel(const uchar4* __restrict__ colors,
                                                          unsigned long long* __restrict__ keys, size_t n_pixels,
                                                          int* __restrict__ overflow_host, float* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (nothing can overflow: mvlm_render_check reads a zero of this render)
        __atomic_store_n(overflow_host, 0, __ATOMIC_RELAXED);
        __threadfence_system();
    }
    const size_t g = size_t(blockIdx.x) * 256 + threadIdx.x;  // view * 65536 + j * 256 + i, j counting up from the bottom row
    if (g >= n_pixels) return;
    const uint64_t best = keys[g];
    if (best != RM_KEY_EMPTY) keys[g] = RM_KEY_EMPTY;
    float4 px = make_float4(1.f, 1.f, 1.f, float(rm_depth_u8(1.0f)) / 255.0f);  // white background, far plane
    if (best != RM_KEY_EMPTY) {
        float r = 255.f, gr = 255.f, bl = 255.f;
        if (colors) {
            const uchar4 col = colors[rm_key_tri(best)];
            r = float(col.x);
            gr = float(col.y);
            bl = float(col.z);
        }
        px = make_float4(r / 255.0f, gr / 255.0f, bl / 255.0f, float(rm_depth_u8(rm_key_z(best))) / 255.0f);
    }
    const size_t view = g / (RM_SIZE * RM_SIZE);
    const int j = int((g / RM_SIZE) % RM_SIZE), i = int(g % RM_SIZE);
    // np.flip(axis=1): GL row j (bottom-up) is image row 255 - j (render3d.py:177)
    reinterpret_cast<float4*>(out)[(view * RM_SIZE + size_t(RM_SIZE - 1 - j)) * RM_SIZE + i] = px;
}

}  // namespace

void raster_points_splat_launch(hipStream_t stream, const float* verts, int n_points, const double* rot, int n_views, int sub_bits,
                                int R, float c, unsigned long long* keys, unsigned long long* stats) {
    const dim3 grid(unsigned((n_points + 255) / 256), unsigned(n_views));
    if (stats)
        hipLaunchKernelGGL(points_splat_kernel<true>, grid, dim3(256), 0, stream, verts, n_points, rot, sub_bits, R, c, keys, stats);
    else
        hipLaunchKernelGGL(points_splat_kernel<false>, grid, dim3(256), 0, stream, verts, n_points, rot, sub_bits, R, c, keys, stats);
}

void raster_points_launch(hipStream_t stream, const float* verts, const uint8_t* colors, int n_points, const double* rot,
                          int n_views, int sub_bits, int R, float c, unsigned long long* keys, unsigned long long* stats,
                          int* overflow_host, float* out, hipEvent_t between) {
    raster_points_splat_launch(stream, verts, n_points, rot, n_views, sub_bits, R, c, keys, stats);
    if (between) (void)hipEventRecord(between, stream);
    const size_t n_pixels = size_t(n_views) * RM_SIZE * RM_SIZE;
    hipLaunchKernelGGL(points_tile_kernel, dim3(unsigned((n_pixels + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uchar4*>(colors), keys, n_pixels, overflow_host, out);
}

// The radius a cloud gets when its owner names none (host only, no ctx): the bounding box of the finite points, extents
// sorted ex >= ey >= ez, s = sqrt(ex * ey / n) with n the number of finite points - the spacing of a regular grid of n
// points over the box's largest face - and r = clamp(1.25 s, 0.75, 8.0) pixels, in model units (x 300 / 256).  A regular grid
// of spacing s leaves no pixel centre farther than 0.71 s from a point, projection under rotation only shrinks spacing, 1.25
// leaves room for irregular sampling; a dense scan (100 k points on a face) lands on the 0.75 px floor.  A cloud of one
// point, a collinear one and one without a finite point have s = 0 and get the floor.
extern "C" int mvlm_points_auto_radius(const float* verts, int n, double* r_out) {
    if (!verts || n <= 0 || !r_out) return 1;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    long n_finite = 0;
    for (long p = 0; p < n; ++p) {
        const float* v = verts + 3 * p;
        if (!rp_finite3(v[0], v[1], v[2])) continue;
        ++n_finite;
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], double(v[k]));
            hi[k] = std::max(hi[k], double(v[k]));
        }
    }
    double s = 0.0;
    if (n_finite > 0) {
        double e[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
        std::sort(e, e + 3);  // ascending: e[2] >= e[1] >= e[0]
        s = std::sqrt(e[2] * e[1] / double(n_finite));
    }
    double px = 1.25 * s;
    px = px < RP_PX_MIN ? RP_PX_MIN : (px > RP_PX_MAX ? RP_PX_MAX : px);
    *r_out = px * 300.0 / 256.0;
    return 0;
}
