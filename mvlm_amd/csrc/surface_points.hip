// The surface snap of a point cloud (a mesh uploaded with n_tris == 0): every landmark goes to the NEAREST POINT of the
// cloud, the result of testing every (landmark, point) pair in float64 - d2 = (dx * dx + dy * dy) + dz * dz with the float32
// coordinates widened, lowest point id on ties, a point with a non-finite coordinate never the nearest, a landmark with a
// non-finite coordinate (no finite distance to anything) passed through unchanged.  The result is the point's own
// coordinates.  mvlm_project_to_surface (surface.hip) branches here in host code.
// Two passes in the triangle snap's shape: one workgroup per (POINTS_CHUNK points, POINTS_GROUP landmarks) leaves the chunk's
// winner per landmark - a thread reads its points once and tests them against the group's landmarks, which are
// wave-uniform and stay in scalar registers - then one wavefront per landmark picks among the chunks.
// Built with raster_points.hip in build/points/ (tests/golden/kernel_occupancy_points.json).
#include "common.h"

namespace {

constexpr int POINTS_CHUNK = 1024;
constexpr int POINTS_GROUP = 8;

__device__ inline bool nearer(double od, int oi, double bd, int bi) { return od < bd || (od == bd && oi < bi); }

__global__ __launch_bounds__(256) void points_nearest_partial_kernel(const float* __restrict__ verts, int n_verts,
                                                                     const double* __restrict__ pts, int n_points, int n_chunks,
                                                                     double* __restrict__ part_d, int* __restrict__ part_i) {
    __shared__ double s_d[POINTS_GROUP][4];
    __shared__ int s_i[POINTS_GROUP][4];
    const int chunk = blockIdx.x, lm0 = blockIdx.y * POINTS_GROUP;
    const int n_lm = min(POINTS_GROUP, n_points - lm0);
    double qx[POINTS_GROUP], qy[POINTS_GROUP], qz[POINTS_GROUP];  // (uniform: scalar registers)
#pragma unroll
    for (int g = 0; g < POINTS_GROUP; ++g) {
        const int lm = lm0 + min(g, n_lm - 1);  // (the tail group repeats its last landmark)
        qx[g] = pts[size_t(lm) * 3];
        qy[g] = pts[size_t(lm) * 3 + 1];
        qz[g] = pts[size_t(lm) * 3 + 2];
    }
    double best[POINTS_GROUP];
    int best_i[POINTS_GROUP];
#pragma unroll
    for (int g = 0; g < POINTS_GROUP; ++g) {
        best[g] = INFINITY;
        best_i[g] = 0x7fffffff;
    }
    constexpr int PPT = POINTS_CHUNK / 256;
    const int v0 = chunk * POINTS_CHUNK + int(threadIdx.x);
    float xyz[PPT][3];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int v = min(v0 + k * 256, n_verts - 1);  // (unconditional loads: all of them leave together)
#pragma unroll
        for (int e = 0; e < 3; ++e) xyz[k][e] = verts[size_t(v) * 3 + e];
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int v = v0 + k * 256;
        if (v >= n_verts) break;
        const double x = xyz[k][0], y = xyz[k][1], z = xyz[k][2];
#pragma unroll
        for (int g = 0; g < POINTS_GROUP; ++g) {
            const double dx = x - qx[g], dy = y - qy[g], dz = z - qz[g];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best[g]) {  // ascending v per thread: first minimum; false for NaN and for inf
                best[g] = d2;
                best_i[g] = v;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < POINTS_GROUP; ++g) {
        double bd = best[g];
        int bi = best_i[g];
        for (int s = 32; s >= 1; s >>= 1) {
            const double od = __shfl_down(bd, s);
            const int oi = __shfl_down(bi, s);
            if (nearer(od, oi, bd, bi)) {
                bd = od;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_d[g][wave] = bd;
            s_i[g][wave] = bi;
        }
    }
    __syncthreads();
    if (int(threadIdx.x) < n_lm) {
        const int g = threadIdx.x;
        double bd = s_d[g][0];
        int bi = s_i[g][0];
        for (int w = 1; w < 4; ++w)
            if (nearer(s_d[g][w], s_i[g][w], bd, bi)) {
                bd = s_d[g][w];
                bi = s_i[g][w];
            }
        part_d[size_t(lm0 + g) * n_chunks + chunk] = bd;
        part_i[size_t(lm0 + g) * n_chunks + chunk] = bi;
    }
}

__global__ __launch_bounds__(64) void points_nearest_final_kernel(const float* __restrict__ verts, const double* __restrict__ pts,
                                                                  int n_chunks, const double* __restrict__ part_d,
                                                                  const int* __restrict__ part_i, double* __restrict__ out) {
    const int lm = blockIdx.x;
    double best = INFINITY;
    int best_i = 0x7fffffff;
    for (int c = threadIdx.x; c < n_chunks; c += 64) {
        const double od = part_d[size_t(lm) * n_chunks + c];
        const int oi = part_i[size_t(lm) * n_chunks + c];
        if (nearer(od, oi, best, best_i)) {
            best = od;
            best_i = oi;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const double od = __shfl_down(best, s);
        const int oi = __shfl_down(best_i, s);
        if (nearer(od, oi, best, best_i)) {
            best = od;
            best_i = oi;
        }
    }
    if (threadIdx.x != 0) return;
    double q[3] = {pts[size_t(lm) * 3], pts[size_t(lm) * 3 + 1], pts[size_t(lm) * 3 + 2]};
    if (best_i != 0x7fffffff)
        for (int e = 0; e < 3; ++e) q[e] = double(verts[size_t(best_i) * 3 + e]);
    for (int e = 0; e < 3; ++e) out[size_t(lm) * 3 + e] = q[e];
}

}  // namespace

// For mvlm_project_to_surface, which has validated its arguments and holds the context.
int mvlm_points_nearest(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points, double* out_dev) {
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;
    MVLM_REQUIRE(ctx, n_points <= 65535, "project_to_surface: at most 65535 points per call");
    const int n_chunks = (mesh->n_verts + POINTS_CHUNK - 1) / POINTS_CHUNK, n_groups = (n_points + POINTS_GROUP - 1) / POINTS_GROUP;
    auto* part_d = static_cast<double*>(ctx->get_scratch("points.part_d", size_t(n_points) * n_chunks * sizeof(double)));
    auto* part_i = static_cast<int*>(ctx->get_scratch("points.part_i", size_t(n_points) * n_chunks * sizeof(int)));
    MVLM_REQUIRE(ctx, part_d && part_i, "project_to_surface: scratch allocation failed");
    hipLaunchKernelGGL(points_nearest_partial_kernel, dim3(n_chunks, n_groups), dim3(256), 0, ctx->stream, mesh->verts, mesh->n_verts,
                       pts_dev, n_points, n_chunks, part_d, part_i);
    hipLaunchKernelGGL(points_nearest_final_kernel, dim3(n_points), dim3(64), 0, ctx->stream, mesh->verts, pts_dev, n_chunks, part_d,
                       part_i, out_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}
