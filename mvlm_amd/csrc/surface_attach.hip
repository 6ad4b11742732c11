// The surface snap with its attachment: besides the closest point (mvlm_project_to_surface's, bit for bit) the triangle that
// holds it, the point's barycentric coordinates in that triangle and the texture coordinates interpolated there.  Passes 0 and
// 1 are the snap's own (surface.hip: mvlm_project_partials); this translation unit supplies the final kernel.
#include "common.h"
#include "surface_math.h"

namespace {

// closest_on_triangle's walk once more, answering with the weights of (a, b, c) instead of the point: the same comparisons
// on the same values, so the region is the one the point came from.
__device__ void closest_barycentric(V3 p, V3 a, V3 b, V3 c, double w[3]) {
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    w[0] = 1.0, w[1] = 0.0, w[2] = 0.0;
    if (d1 <= 0 && d2 <= 0) return;
    const V3 bp = sub(p, b);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0 && d4 <= d3) {
        w[0] = 0.0, w[1] = 1.0;
        return;
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0 && d1 > d3) {
        const double t = d1 / (d1 - d3);
        w[0] = 1.0 - t, w[1] = t;
        return;
    }
    const V3 cp = sub(p, c);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0 && d5 <= d6) {
        w[0] = 0.0, w[2] = 1.0;
        return;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double t = d2 / (d2 - d6);
        w[0] = 1.0 - t, w[2] = t;
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        w[0] = 0.0, w[1] = 1.0 - t, w[2] = t;
        return;
    }
    const double denom = 1.0 / (va + vb + vc);
    const double v = vb * denom, ww = vc * denom;
    // (v + ww can round to a hair above 1 when va is positive but minute: the first weight never goes below 0)
    w[0] = fmax(0.0, 1.0 - v - ww), w[1] = v, w[2] = ww;
}

// Pass 2 of the snap (project_final_kernel's selection: nearest chunk winner, lowest triangle id on ties) with the
// attachment.  A landmark without a finite distance to any triangle is passed through: tri -1, bary and uv NaN.
__global__ __launch_bounds__(64) void attach_final_kernel(const float* __restrict__ verts, const float* __restrict__ uvs,
                                                          const int32_t* __restrict__ tris, const double* __restrict__ pts,
                                                          int n_chunks, const double* __restrict__ part_d,
                                                          const int* __restrict__ part_t, double* __restrict__ out,
                                                          int* __restrict__ tri, double* __restrict__ bary,
                                                          double* __restrict__ uv) {
    const int lm = blockIdx.x;
    double best = INFINITY;
    int best_t = 0x7fffffff;
    for (int c = threadIdx.x; c < n_chunks; c += 64) {
        const double od = part_d[size_t(lm) * n_chunks + c];
        const int ot = part_t[size_t(lm) * n_chunks + c];
        if (od < best || (od == best && ot < best_t)) {
            best = od;
            best_t = ot;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const double od = __shfl_down(best, s);
        const int ot = __shfl_down(best_t, s);
        if (od < best || (od == best && ot < best_t)) {
            best = od;
            best_t = ot;
        }
    }
    if (threadIdx.x != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const V3 p = {pts[lm * 3], pts[lm * 3 + 1], pts[lm * 3 + 2]};
    V3 q = p;
    double w[3] = {nan, nan, nan}, tu = nan, tv = nan;
    if (best_t != 0x7fffffff) {
        const int ia = tris[3 * best_t], ib = tris[3 * best_t + 1], ic = tris[3 * best_t + 2];
        const V3 a = {verts[3 * ia], verts[3 * ia + 1], verts[3 * ia + 2]};
        const V3 b = {verts[3 * ib], verts[3 * ib + 1], verts[3 * ib + 2]};
        const V3 c = {verts[3 * ic], verts[3 * ic + 1], verts[3 * ic + 2]};
        q = closest_on_triangle(p, a, b, c);
        closest_barycentric(p, a, b, c, w);
        if (uvs) {
            tu = w[0] * double(uvs[2 * ia]) + w[1] * double(uvs[2 * ib]) + w[2] * double(uvs[2 * ic]);
            tv = w[0] * double(uvs[2 * ia + 1]) + w[1] * double(uvs[2 * ib + 1]) + w[2] * double(uvs[2 * ic + 1]);
        }
    }
    out[lm * 3] = q.x;
    out[lm * 3 + 1] = q.y;
    out[lm * 3 + 2] = q.z;
    tri[lm] = best_t != 0x7fffffff ? best_t : -1;
    bary[lm * 3] = w[0];
    bary[lm * 3 + 1] = w[1];
    bary[lm * 3 + 2] = w[2];
    uv[lm * 2] = tu;
    uv[lm * 2 + 1] = tv;
}

}  // namespace

int mvlm_launch_surface_attach(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points, double* snapped_dev,
                               int32_t* tri_dev, double* bary_dev, double* uv_dev) {
    MVLM_REQUIRE(ctx, mesh && pts_dev && snapped_dev && tri_dev && bary_dev && uv_dev && n_points > 0,
                 "surface_attach: bad arguments");
    MVLM_REQUIRE(ctx, mesh->n_tris > 0, "surface_attach: the surface attachment of a point cloud is not supported (the mesh has no triangles)");
    int n_chunks = 0;
    const double* part_d = nullptr;
    const int* part_t = nullptr;
    if (mvlm_project_partials(ctx, mesh, pts_dev, n_points, &n_chunks, &part_d, &part_t)) return 1;
    hipLaunchKernelGGL(attach_final_kernel, dim3(n_points), dim3(64), 0, ctx->stream, mesh->verts, mesh->uvs, mesh->tris,
                       pts_dev, n_chunks, part_d, part_t, snapped_dev, tri_dev, bary_dev, uv_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

extern "C" int mvlm_surface_attach(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points,
                                   double* snapped_dev, int32_t* tri_dev, double* bary_dev, double* uv_dev) {
    MVLM_ENTER(ctx);
    return mvlm_launch_surface_attach(ctx, mesh, pts_dev, n_points, snapped_dev, tri_dev, bary_dev, uv_dev);
}
