// A triangle surface for a point cloud (a mesh uploaded with n_tris == 0): mvlm_mesh_triangulate_points.  Every point votes for
// the triangles of its own star - the Delaunay neighbours of its 16 nearest points in its tangent plane - and a triangle is kept
// where its three corners agree (cloud_mesh_math.h holds the contract, DESIGN.md 5.1 "Point clouds").  The neighbour table and the
// normals are mvlm_mesh_estimate_normals' (cloud_normals.hip); nothing here touches the cloud's device copy or the render's key plane.
//
// Five stages on the launch stream, nothing returns to the host:
//   perturb  one thread per point: the point shifted by 1/256 of its nearest-neighbour distance in a direction hashed from its id
//   star     one thread per point: its neighbours' inverted tangent-plane positions w in LDS as [k][thread] (the neighbour search
//            keeps its list the same way), the hull's edges by the contract's plain form - for an entry a the one b with the
//            origin and every other entry to the left of a -> b - noted as slot numbers in two registers; then the pairs' point
//            ids, sorted ascending in the same LDS, go to the context's scratch (16 pairs per point)
//   count    one thread per point i: the pairs (j, k) of its star with i < j whose other two corners have the matching pairs and
//            that pass the sliver test - a 16-bit mask and its population
//   scan     exclusive prefix sum over the populations (per-block sums, one block over those, per-block apply), the total to the
//            caller's counter
//   emit     one thread per point: its rows (i, j, k), in the star's order, from its start; rows at or beyond the caller's cap are
//            not written
// A star's pairs are sorted and a point's rows start where the scan puts them: the array is in ascending (i, j, k) and the same
// bytes from run to run.  No atomics.  The scan is this file's own for the reason raster_bins.h gives for its helpers.
// Built as an object of its own (build/cloudmesh/, tests/golden/kernel_occupancy_cloudmesh.json): no kernel here uses scratch memory.
#include "common.h"
#include "cloud_mesh_math.h"

#include <algorithm>

namespace {

constexpr int STAR_WG = 128;         // threads of a star workgroup: 2 x 16 doubles of LDS per thread, 32 KB
constexpr int SCAN_PER_THREAD = 16;  // counters per thread of a scan block
constexpr int SCAN_BLOCK = 256 * SCAN_PER_THREAD;

__device__ inline cm_vec3 load_point(const float* __restrict__ verts, int p) {
    return cm_v3(double(verts[3 * size_t(p)]), double(verts[3 * size_t(p) + 1]), double(verts[3 * size_t(p) + 2]));
}
__device__ inline cm_vec3 load_shifted(const double* __restrict__ shifted, int p) {
    return cm_v3(shifted[3 * size_t(p)], shifted[3 * size_t(p) + 1], shifted[3 * size_t(p) + 2]);
}

__global__ __launch_bounds__(256) void cloudmesh_perturb_kernel(const float* __restrict__ verts, int n_points,
                                                                const int32_t* __restrict__ neighbors, double* __restrict__ shifted) {
    const int p = blockIdx.x * 256 + int(threadIdx.x);
    if (p >= n_points) return;
    const cm_vec3 v = load_point(verts, p);
    const int32_t* const row = neighbors + size_t(p) * CM_K;
    double least = 0.0;
    for (int k = 0; k < CM_K; ++k) {
        const int m = row[k];
        if (m < 0 || m >= n_points) continue;
        const cm_vec3 d = cm_sub(load_point(verts, m), v);
        const double d2 = cm_dot(d, d);
        if (d2 > 0.0 && (least == 0.0 || d2 < least)) least = d2;
    }
    const cm_vec3 u = cm_perturb(p, v, cm_shift(least));
    shifted[3 * size_t(p)] = u.x;
    shifted[3 * size_t(p) + 1] = u.y;
    shifted[3 * size_t(p) + 2] = u.z;
}

// star_n[p] pairs in star[p * CM_STAR ...], each (lower id, higher id), ascending
__global__ __launch_bounds__(STAR_WG) void cloudmesh_star_kernel(const float* __restrict__ normals, int n_points,
                                                                 const int32_t* __restrict__ neighbors,
                                                                 const double* __restrict__ shifted, int2* __restrict__ star,
                                                                 int* __restrict__ star_n) {
    __shared__ double s_wx[CM_K][STAR_WG];
    __shared__ double s_wy[CM_K][STAR_WG];
    const int t = threadIdx.x;
    const int p = blockIdx.x * STAR_WG + t;
    if (p >= n_points) return;
    const int32_t* const row = neighbors + size_t(p) * CM_K;
    const cm_frame f = cm_tangent_frame(
        cm_v3(double(normals[3 * size_t(p)]), double(normals[3 * size_t(p) + 1]), double(normals[3 * size_t(p) + 2])));
    unsigned others = 0, kept = 0;  // bit k: row slot k holds a point other than p / is one of the star's entries
    for (int k = 0; k < CM_K; ++k) {
        const int m = row[k];
        if (m >= 0 && m < n_points && m != p) others |= 1u << k;
    }
    int n_pairs = 0;
    unsigned long long pairs_lo = 0, pairs_hi = 0;  // pair e: slots (a, b) as the byte a | b << 4, eight pairs a word
    if (f.ok && __popc(others) >= 2) {
        const cm_vec3 up = load_shifted(shifted, p);
        for (int k = 0; k < CM_K; ++k) {
            if (!(others >> k & 1u)) continue;
            const cm_inverted w = cm_invert(f.e1, f.e2, cm_sub(load_shifted(shifted, row[k]), up));
            if (!w.kept) continue;
            kept |= 1u << k;
            s_wx[k][t] = w.w.x;
            s_wy[k][t] = w.w.y;
        }
        for (int a = 0; a < CM_K; ++a) {
            if (!(kept >> a & 1u)) continue;
            cm_vec2 wa;
            wa.x = s_wx[a][t], wa.y = s_wy[a][t];
            for (int b = 0; b < CM_K; ++b) {
                if (b == a || !(kept >> b & 1u)) continue;
                cm_vec2 wb;
                wb.x = s_wx[b][t], wb.y = s_wy[b][t];
                if (!cm_turns_left(wa, wb)) continue;
                bool all_left = true;
                for (int c = 0; c < CM_K && all_left; ++c) {
                    if (c == a || c == b || !(kept >> c & 1u)) continue;
                    cm_vec2 wc;
                    wc.x = s_wx[c][t], wc.y = s_wy[c][t];
                    all_left = cm_left_of(wa, wb, wc);
                }
                if (!all_left) continue;
                if (n_pairs < CM_STAR) {  // (always: an entry starts at most one pair, cloud_mesh_math.h)
                    const unsigned long long code = (unsigned long long)(a | b << 4) << (8 * (n_pairs & 7));
                    if (n_pairs < 8) pairs_lo |= code;
                    else pairs_hi |= code;
                    ++n_pairs;
                }
                break;  // (no other b can pass for this a)
            }
        }
    }
    // the pairs' ids, sorted by (lower, higher), in the LDS the w list no longer needs: pair e of thread t at s_wx[e][t]
    // (a key travels as the double with its bits: the array keeps its type)
    for (int e = 0; e < n_pairs; ++e) {
        const unsigned code = unsigned((e < 8 ? pairs_lo : pairs_hi) >> (8 * (e & 7))) & 0xFFu;
        const int ia = row[code & 15u], ib = row[code >> 4];
        const long long key = (long long)min(ia, ib) << 32 | (long long)max(ia, ib);
        int j = e;
        while (j > 0 && __double_as_longlong(s_wx[j - 1][t]) > key) {
            s_wx[j][t] = s_wx[j - 1][t];
            --j;
        }
        s_wx[j][t] = __longlong_as_double(key);
    }
    for (int e = 0; e < n_pairs; ++e) {
        const long long key = __double_as_longlong(s_wx[e][t]);
        star[size_t(p) * CM_STAR + e] = make_int2(int(key >> 32), int(key & 0xFFFFFFFFll));
    }
    star_n[p] = n_pairs;
}

// is the pair (lo, hi) in the star of q?
__device__ inline bool star_has(const int2* __restrict__ star, const int* __restrict__ star_n, int q, int lo, int hi) {
    const int n = star_n[q];
    const int2* const s = star + size_t(q) * CM_STAR;
    for (int e = 0; e < n; ++e) {
        const int2 pr = s[e];
        if (pr.x == lo && pr.y == hi) return true;
    }
    return false;
}

// mask[i] bit e: pair e of i's star, (j, k), makes the triangle i < j < k; counts[i] the mask's population
__global__ __launch_bounds__(256) void cloudmesh_count_kernel(const float* __restrict__ verts, int n_points,
                                                              const int2* __restrict__ star, const int* __restrict__ star_n,
                                                              int* __restrict__ mask, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + int(threadIdx.x);
    if (i >= n_points) return;
    const int n = star_n[i];
    unsigned m = 0;
    if (n > 0) {
        const cm_vec3 vi = load_point(verts, i);
        for (int e = 0; e < n; ++e) {
            const int2 pr = star[size_t(i) * CM_STAR + e];  // (pr.x < pr.y)
            if (pr.x <= i) continue;
            if (!star_has(star, star_n, pr.x, i, pr.y) || !star_has(star, star_n, pr.y, i, pr.x)) continue;
            if (cm_not_sliver(vi, load_point(verts, pr.x), load_point(verts, pr.y))) m |= 1u << e;
        }
    }
    mask[i] = int(m);
    counts[i] = __popc(m);
}

// inclusive scan of one value per thread over a workgroup of 256; returns the thread's inclusive sum, *total the workgroup's
__device__ inline int block_scan_256(int v, int* s /*[256]*/, int* total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int o = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += o;
        __syncthreads();
    }
    const int r = s[t];
    *total = s[255];
    __syncthreads();
    return r;
}

// (counts is padded with zeros to a whole number of scan blocks)
__global__ __launch_bounds__(256) void cloudmesh_scan_sums_kernel(const int* __restrict__ counts, int* __restrict__ block_sums) {
    __shared__ int s[256];
    const int4* src = reinterpret_cast<const int4*>(counts + size_t(blockIdx.x) * SCAN_BLOCK + size_t(threadIdx.x) * SCAN_PER_THREAD);
    int sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD / 4; ++k) {
        const int4 q = src[k];
        sum += (q.x + q.y) + (q.z + q.w);
    }
    int total;
    (void)block_scan_256(sum, s, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// exclusive scan of the block sums in place: one workgroup, any number of blocks (a carry runs over slices of 256); the grand
// total goes to the caller's counter
__global__ __launch_bounds__(256) void cloudmesh_scan_top_kernel(int* __restrict__ block_sums, int n_blocks, int32_t* __restrict__ n_tris) {
    __shared__ int s[256];
    int carry = 0;
    for (int base = 0; base < n_blocks; base += 256) {
        const int i = base + int(threadIdx.x);
        const int v = i < n_blocks ? block_sums[i] : 0;
        int total;
        const int incl = block_scan_256(v, s, &total);
        if (i < n_blocks) block_sums[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) *n_tris = carry;
}

__global__ __launch_bounds__(256) void cloudmesh_scan_apply_kernel(const int* __restrict__ counts, const int* __restrict__ block_sums,
                                                                   int* __restrict__ starts) {
    __shared__ int s[256];
    const size_t at = size_t(blockIdx.x) * SCAN_BLOCK + size_t(threadIdx.x) * SCAN_PER_THREAD;
    const int4* src = reinterpret_cast<const int4*>(counts + at);
    int4 q[SCAN_PER_THREAD / 4];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD / 4; ++k) {
        q[k] = src[k];
        sum += (q[k].x + q[k].y) + (q[k].z + q[k].w);
    }
    int total;
    int run = block_sums[blockIdx.x] + block_scan_256(sum, s, &total) - sum;
    int4* dst = reinterpret_cast<int4*>(starts + at);
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD / 4; ++k) {
        int4 o;
        o.x = run;
        o.y = o.x + q[k].x;
        o.z = o.y + q[k].y;
        o.w = o.z + q[k].z;
        run = o.w + q[k].w;
        dst[k] = o;
    }
}

__global__ __launch_bounds__(256) void cloudmesh_emit_kernel(int n_points, const int2* __restrict__ star, const int* __restrict__ mask,
                                                             const int* __restrict__ starts, int32_t* __restrict__ tris, long long cap) {
    const int i = blockIdx.x * 256 + int(threadIdx.x);
    if (i >= n_points) return;
    unsigned m = unsigned(mask[i]);
    long long at = starts[i];
    while (m && at < cap) {
        const int e = __ffs(m) - 1;
        m &= m - 1;
        const int2 pr = star[size_t(i) * CM_STAR + e];
        tris[3 * at] = i;
        tris[3 * at + 1] = pr.x;
        tris[3 * at + 2] = pr.y;
        ++at;
    }
}

}  // namespace

extern "C" int mvlm_mesh_triangulate_points(mvlm_ctx* ctx, const mvlm_mesh* cloud, const int32_t* neighbors_dev, int32_t* tris_dev,
                                            long long cap, int32_t* n_tris_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, cloud, "triangulate points: null mesh");
    MVLM_REQUIRE(ctx, cloud->n_tris == 0, "triangulate points: the mesh has triangles (a surface is built for a point cloud)");
    MVLM_REQUIRE(ctx, cloud->normals, "triangulate points: the cloud has no normals (mvlm_mesh_estimate_normals leaves them and the table)");
    MVLM_REQUIRE(ctx, neighbors_dev && n_tris_dev, "triangulate points: null neighbour table or counter");
    MVLM_REQUIRE(ctx, cap >= 0, "triangulate points: negative cap");
    MVLM_REQUIRE(ctx, cloud->n_verts > 0 && cloud->n_verts <= (1 << 26), "triangulate points: 1 to 67108864 points");
    const int V = cloud->n_verts;
    const int n_blocks = (V + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const size_t n_ctr = size_t(n_blocks) * SCAN_BLOCK;
    auto* shifted = static_cast<double*>(ctx->get_scratch("cloudmesh.shifted", size_t(V) * 3 * sizeof(double)));
    auto* star = static_cast<int2*>(ctx->get_scratch("cloudmesh.star", size_t(V) * CM_STAR * sizeof(int2)));
    auto* star_n = static_cast<int*>(ctx->get_scratch("cloudmesh.star_n", size_t(V) * sizeof(int)));
    auto* mask = static_cast<int*>(ctx->get_scratch("cloudmesh.mask", size_t(V) * sizeof(int)));
    auto* counts = static_cast<int*>(ctx->get_scratch("cloudmesh.counts", n_ctr * sizeof(int)));
    auto* starts = static_cast<int*>(ctx->get_scratch("cloudmesh.starts", n_ctr * sizeof(int)));
    auto* sums = static_cast<int*>(ctx->get_scratch("cloudmesh.sums", size_t(n_blocks) * sizeof(int)));
    MVLM_REQUIRE(ctx, shifted && star && star_n && mask && counts && starts && sums, "triangulate points: scratch allocation failed");
    if (mvlm_mesh_wait_ready(ctx, cloud, ctx->stream)) return 1;
    StageClock& clock = ctx->cloudmesh_clock;  // (profiling: events round the three stages, mvlm_cloud_mesh_stage_ms)
    clock.invalidate();
    if (clock.arm(ctx, 4) || clock.record(ctx, 0, ctx->stream)) return 1;
    const dim3 per_point(unsigned((V + 255) / 256)), wg(256);
    hipLaunchKernelGGL(cloudmesh_perturb_kernel, per_point, wg, 0, ctx->stream, cloud->verts, V, neighbors_dev, shifted);
    hipLaunchKernelGGL(cloudmesh_star_kernel, dim3(unsigned((V + STAR_WG - 1) / STAR_WG)), dim3(STAR_WG), 0, ctx->stream, cloud->normals, V,
                       neighbors_dev, shifted, star, star_n);
    if (clock.record(ctx, 1, ctx->stream)) return 1;
    if (n_ctr > size_t(V))  // the last scan block's counters past the points
        MVLM_CHECK_HIP(ctx, hipMemsetAsync(counts + V, 0, (n_ctr - size_t(V)) * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(cloudmesh_count_kernel, per_point, wg, 0, ctx->stream, cloud->verts, V, star, star_n, mask, counts);
    hipLaunchKernelGGL(cloudmesh_scan_sums_kernel, dim3(n_blocks), wg, 0, ctx->stream, counts, sums);
    hipLaunchKernelGGL(cloudmesh_scan_top_kernel, dim3(1), wg, 0, ctx->stream, sums, n_blocks, n_tris_dev);
    hipLaunchKernelGGL(cloudmesh_scan_apply_kernel, dim3(n_blocks), wg, 0, ctx->stream, counts, sums, starts);
    if (clock.record(ctx, 2, ctx->stream)) return 1;
    if (tris_dev && cap > 0)
        hipLaunchKernelGGL(cloudmesh_emit_kernel, per_point, wg, 0, ctx->stream, V, star, mask, starts, tris_dev, cap);
    if (clock.record(ctx, 3, ctx->stream)) return 1;
    clock.mark(4);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

// Milliseconds of the last triangulation's three stages - star (with perturb), count and scan, emit - while
// mvlm_render_set_profiling is on; waits for the stream.
extern "C" int mvlm_cloud_mesh_stage_ms(mvlm_ctx* ctx, float* ms3) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms3, "cloud_mesh_stage_ms: null pointer");
    return ctx->cloudmesh_clock.read(ctx, 3, ms3, "cloud_mesh_stage_ms: no cloud was triangulated with render profiling on");
}
