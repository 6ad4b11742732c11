// Surface distances between landmarks: mvlm_landmark_geodesics.  One distance field per source landmark over the scan's triangles
// by the first-order fast-marching update (Hopf-Lax over a triangle's edge), iterated Jacobi-fashion to its fixed point, then read
// at every target landmark.  geodesic_math.h holds the rule and every operation's order ("Surface distances"); the
// values do not depend on scheduling: every sweep reads one buffer and writes the other, and a vertex's value is a min.
//
// Stages on the launch stream:
//   attach     the snap with its triangle (surface_attach.hip's launcher), then one flag per landmark: attached or not
//   adjacency  vertex -> incident valid triangles as a CSR of (A, B) pairs, the corner's edge: count (integer atomics), scan, fill
//              (a cursor per vertex: the order within a row is free, the min does not see it)
//   init       per source group: the source triangle's corners, widened init_rings times through the CSR (a gather: no race)
//   sweeps     one kernel per sweep - the sweep boundary IS the kernel boundary, there is no barrier between workgroups and no
//              wait on another workgroup anywhere.  A thread owns one vertex and GD_SRC_PER sources: an incidence's frame (three
//              square roots, a division) is computed once and serves them all.  A sweep adds its changed values to a counter per
//              source; three counter slots rotate (sweep k adds to k % 3, reads (k - 1) % 3, clears (k + 1) % 3), so no slot is
//              written and read in one launch.  A source whose previous sweep changed nothing is settled: its kernels return at once.
//   targets    per (source, target): the update over the target triangle's three edges
// The host enqueues GD_BATCH sweeps, then reads the group's settled flags (the one wait of the call), until all are settled.
// Every device loop runs to a count read before it starts (a CSR row, a fixed 3 or GD_SRC_PER).
// Built as an object of its own (build/geodesic/, tests/golden/kernel_occupancy_geodesic.json): no kernel here uses scratch memory.
#include "common.h"
#include "geodesic_math.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int GD_SRC_PER = 4;   // sources a sweep thread serves
constexpr int GD_BATCH = 32;    // sweeps enqueued between two reads of the settled flags
constexpr int SCAN_PER_THREAD = 16;
constexpr int SCAN_BLOCK = 256 * SCAN_PER_THREAD;

__device__ inline gd_vec3 load_vert(const float* __restrict__ verts, int v) {
    return gd_v3(double(verts[3 * size_t(v)]), double(verts[3 * size_t(v) + 1]), double(verts[3 * size_t(v) + 2]));
}
__device__ inline gd_vec3 load_point(const double* __restrict__ pts, int i) {
    return gd_v3(pts[3 * size_t(i)], pts[3 * size_t(i) + 1], pts[3 * size_t(i) + 2]);
}
__device__ inline double gd_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the rule's "valid triangle": indices in range, nine finite coordinates
__device__ inline bool tri_valid(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris, int t, int idx[3]) {
    idx[0] = tris[3 * size_t(t)], idx[1] = tris[3 * size_t(t) + 1], idx[2] = tris[3 * size_t(t) + 2];
    for (int e = 0; e < 3; ++e)
        if (idx[e] < 0 || idx[e] >= V) return false;
    return gd_finite3(load_vert(verts, idx[0])) && gd_finite3(load_vert(verts, idx[1])) && gd_finite3(load_vert(verts, idx[2]));
}

__global__ __launch_bounds__(256) void geodesic_count_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris,
                                                             int T, int* __restrict__ counts) {
    const int t = blockIdx.x * 256 + int(threadIdx.x);
    if (t >= T) return;
    int idx[3];
    if (!tri_valid(verts, V, tris, t, idx)) return;
    for (int e = 0; e < 3; ++e) atomicAdd(&counts[idx[e]], 1);
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

// (counts is padded with zeros to a whole number of scan blocks, at least one counter past the vertices)
__global__ __launch_bounds__(256) void geodesic_scan_sums_kernel(const int* __restrict__ counts, int* __restrict__ block_sums) {
    __shared__ int s[256];
    const int* src = counts + size_t(blockIdx.x) * SCAN_BLOCK + size_t(threadIdx.x) * SCAN_PER_THREAD;
    int sum = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) sum += src[k];
    int total;
    (void)block_scan_256(sum, s, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// exclusive scan of the block sums in place: one workgroup, a carry over slices of 256
__global__ __launch_bounds__(256) void geodesic_scan_top_kernel(int* __restrict__ block_sums, int n_blocks) {
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
}

__global__ __launch_bounds__(256) void geodesic_scan_apply_kernel(const int* __restrict__ counts, const int* __restrict__ block_sums,
                                                                  int* __restrict__ starts) {
    __shared__ int s[256];
    const size_t at = size_t(blockIdx.x) * SCAN_BLOCK + size_t(threadIdx.x) * SCAN_PER_THREAD;
    int q[SCAN_PER_THREAD];
    int sum = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        q[k] = counts[at + k];
        sum += q[k];
    }
    int total;
    int run = block_sums[blockIdx.x] + block_scan_256(sum, s, &total) - sum;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        starts[at + k] = run;
        run += q[k];
    }
}

// adj[starts[v] ...]: for every valid triangle with v as a corner, the corner's edge (A, B)
__global__ __launch_bounds__(256) void geodesic_fill_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris,
                                                            int T, const int* __restrict__ starts, int* __restrict__ cursor,
                                                            int2* __restrict__ adj) {
    const int t = blockIdx.x * 256 + int(threadIdx.x);
    if (t >= T) return;
    int idx[3];
    if (!tri_valid(verts, V, tris, t, idx)) return;
    for (int e = 0; e < 3; ++e) {
        const int v = idx[e];
        const int at = starts[v] + atomicAdd(&cursor[v], 1);
        if (at < starts[v + 1]) adj[at] = make_int2(idx[(e + 1) % 3], idx[(e + 2) % 3]);  // (always: the count was of the same triangles)
    }
}

// ok[i]: landmark i is attached - a valid triangle and a finite snapped point
__global__ __launch_bounds__(256) void geodesic_attached_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris,
                                                                int T, const double* __restrict__ snapped,
                                                                const int32_t* __restrict__ tri, int n, int* __restrict__ ok) {
    const int i = blockIdx.x * 256 + int(threadIdx.x);
    if (i >= n) return;
    const int t = tri[i];
    int idx[3];
    ok[i] = t >= 0 && t < T && tri_valid(verts, V, tris, t, idx) && gd_finite3(load_point(snapped, i));
}

// the source triangle's corners; grid (vertex chunk, source of the group).  Also the group's flags: a source that is not attached
// is settled from the start.
__global__ __launch_bounds__(256) void geodesic_init_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris,
                                                            const double* __restrict__ snapped, const int32_t* __restrict__ tri,
                                                            const int* __restrict__ ok, const int* __restrict__ src_lm,
                                                            double* __restrict__ d, int* __restrict__ state) {
    const int s = blockIdx.y, lm = src_lm[s];
    const int v = blockIdx.x * 256 + int(threadIdx.x);
    const bool attached = ok[lm] != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) state[s] = attached ? -1 : 0;
    if (v >= V) return;
    double out = gd_inf();
    if (attached) {
        const int t = tri[lm];
        if (tris[3 * size_t(t)] == v || tris[3 * size_t(t) + 1] == v || tris[3 * size_t(t) + 2] == v)
            out = gd_dist(load_vert(verts, v), load_point(snapped, lm));
    }
    d[size_t(s) * V + v] = out;
}

// one ring: a vertex joins when a valid triangle of its own has a corner in the set as `old` holds it
__global__ __launch_bounds__(256) void geodesic_ring_kernel(const float* __restrict__ verts, int V, const int* __restrict__ starts,
                                                            const int2* __restrict__ adj, const double* __restrict__ snapped,
                                                            const int* __restrict__ src_lm, const double* __restrict__ old,
                                                            double* __restrict__ out) {
    const int s = blockIdx.y;
    const int v = blockIdx.x * 256 + int(threadIdx.x);
    if (v >= V) return;
    const double* const o = old + size_t(s) * V;
    double val = o[v];
    if (!gd_finite(val)) {
        bool joins = false;
        const int e1 = starts[v + 1];
        for (int e = starts[v]; e < e1; ++e) {
            const int2 ab = adj[e];
            joins = joins || gd_finite(o[ab.x]) || gd_finite(o[ab.y]);
        }
        if (joins) val = gd_dist(load_vert(verts, v), load_point(snapped, src_lm[s]));
    }
    out[size_t(s) * V + v] = val;
}

// Sweep k of a group of g sources; grid (vertex chunk, GD_SRC_PER sources).  cnt i32[3][g], state i32[g] (-1: running, else the
// index of the first sweep that changed nothing).
__global__ __launch_bounds__(256) void geodesic_sweep_kernel(const float* __restrict__ verts, int V, const int* __restrict__ starts,
                                                             const int2* __restrict__ adj, int g, int k,
                                                             const double* __restrict__ old, double* __restrict__ out,
                                                             int* __restrict__ cnt, int* __restrict__ state) {
    const int s0 = blockIdx.y * GD_SRC_PER;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    bool run[GD_SRC_PER];
    bool any = false;
    for (int q = 0; q < GD_SRC_PER; ++q) {
        const int s = s0 + q;
        run[q] = false;
        if (s >= g) continue;
        if (first) cnt[((k + 1) % 3) * g + s] = 0;
        if (state[s] >= 0) continue;
        if (k > 0 && cnt[((k - 1) % 3) * g + s] == 0) {  // the previous sweep changed nothing: settled, for every workgroup alike
            if (first) state[s] = k - 1;
            continue;
        }
        run[q] = true;
        any = true;
    }
    if (!any) return;  // (the same answer in every thread of the launch)
    const int v = blockIdx.x * 256 + int(threadIdx.x);
    double cur[GD_SRC_PER], best[GD_SRC_PER];
    for (int q = 0; q < GD_SRC_PER; ++q) cur[q] = best[q] = 0.0;
    if (v < V) {
        for (int q = 0; q < GD_SRC_PER; ++q)
            if (run[q]) cur[q] = best[q] = old[size_t(s0 + q) * V + v];
        const gd_vec3 C = load_vert(verts, v);
        const int e1 = starts[v + 1];
        for (int e = starts[v]; e < e1; ++e) {
            const int2 ab = adj[e];
            const gd_frame f = gd_make_frame(load_vert(verts, ab.x), load_vert(verts, ab.y), C);
            for (int q = 0; q < GD_SRC_PER; ++q) {
                if (!run[q]) continue;
                const double* const o = old + size_t(s0 + q) * V;
                best[q] = gd_min(best[q], gd_update(o[ab.x], o[ab.y], f));
            }
        }
        for (int q = 0; q < GD_SRC_PER; ++q)
            if (run[q]) out[size_t(s0 + q) * V + v] = best[q];
    }
    for (int q = 0; q < GD_SRC_PER; ++q) {
        if (!run[q]) continue;  // (uniform)
        const int n = __syncthreads_count(best[q] != cur[q]);
        if (threadIdx.x == 0 && n) atomicAdd(&cnt[(k % 3) * g + s0 + q], n);
    }
}

// behind the last sweep of a batch, index k: what sweep k + 1 would have noted
__global__ __launch_bounds__(256) void geodesic_settle_kernel(int g, int k, const int* __restrict__ cnt, int* __restrict__ state) {
    const int s = blockIdx.x * 256 + int(threadIdx.x);
    if (s < g && state[s] < 0 && cnt[(k % 3) * g + s] == 0) state[s] = k;
}

// D for the sources [g0, g0 + g) of this group.  Without pairs: grid (target chunk, source of the group).  With pairs i32[m,2]:
// one thread per directed item w in [0, 2m) - (i, j) for w < m, (j, i) of pair w - m beyond -, those whose source is in the group.
__global__ __launch_bounds__(256) void geodesic_target_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris,
                                                              const double* __restrict__ snapped, const int32_t* __restrict__ tri,
                                                              const int* __restrict__ ok, int n, const int* __restrict__ src_lm,
                                                              const int* __restrict__ slot, int g0, int g,
                                                              const int32_t* __restrict__ pairs, int m,
                                                              const double* __restrict__ field, double* __restrict__ D) {
    int i, j, s;
    const int w = blockIdx.x * 256 + int(threadIdx.x);
    if (pairs) {
        if (w >= 2 * m) return;
        i = w < m ? pairs[2 * w] : pairs[2 * (w - m) + 1];
        j = w < m ? pairs[2 * w + 1] : pairs[2 * (w - m)];
        s = slot[i] - g0;
        if (s < 0 || s >= g) return;
    } else {
        if (w >= n) return;
        s = blockIdx.y;
        i = src_lm[g0 + s];
        j = w;
    }
    double out = gd_nan();
    if (ok[i] && ok[j]) {
        if (i == j) {
            out = 0.0;
        } else {
            const double* const d = field + size_t(s) * V;
            const gd_vec3 P = load_point(snapped, j);
            const int t = tri[j];
            int idx[3] = {tris[3 * size_t(t)], tris[3 * size_t(t) + 1], tris[3 * size_t(t) + 2]};
            out = gd_inf();
            for (int e = 0; e < 3; ++e) {
                const int a = idx[(e + 1) % 3], b = idx[(e + 2) % 3];
                out = gd_min(out, gd_update(d[a], d[b], gd_make_frame(load_vert(verts, a), load_vert(verts, b), P)));
            }
            if (tri[i] == t) out = gd_min(out, gd_dist(load_point(snapped, i), P));
        }
    }
    D[size_t(i) * n + j] = out;
}

__global__ __launch_bounds__(256) void geodesic_euclid_kernel(const double* __restrict__ snapped, int n, double* __restrict__ E) {
    const size_t w = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (w >= size_t(n) * n) return;
    E[w] = gd_dist(load_point(snapped, int(w / n)), load_point(snapped, int(w % n)));
}

// a group's sweep counts and, where the caller keeps them, its fields; grid (vertex chunk or 1, source of the group)
__global__ __launch_bounds__(256) void geodesic_finish_kernel(int V, const int* __restrict__ ok, const int* __restrict__ src_lm,
                                                              const int* __restrict__ state, const double* __restrict__ field,
                                                              int32_t* __restrict__ sweeps, double* __restrict__ field_out) {
    const int s = blockIdx.y, lm = src_lm[s];
    if (!ok[lm]) return;  // (sweeps -1, the field's row NaN: as the host left them)
    if (blockIdx.x == 0 && threadIdx.x == 0) sweeps[lm] = state[s];
    const int v = blockIdx.x * 256 + int(threadIdx.x);
    if (field_out && v < V) field_out[size_t(lm) * V + v] = field[size_t(s) * V + v];
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

// Checks the arguments - a bad one returns an error that starts with "geodesics:" and launches nothing - then enqueues the
// stages above.  WAITS FOR THE STREAM: after every batch of sweeps the host reads the group's settled flags.
extern "C" int mvlm_landmark_geodesics(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n, int init_rings,
                                       int max_sweeps, long long max_scratch_bytes, const int32_t* pairs_host, int n_pairs,
                                       double* snapped_dev, int32_t* tri_dev, double* D_dev, double* E_dev, int32_t* sweeps_dev,
                                       double* field_dev) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    ctx->geodesic_clock.invalidate();
    MVLM_REQUIRE(ctx, mesh, "geodesics: null mesh");
    MVLM_REQUIRE(ctx, mesh->n_tris > 0, "geodesics: a point cloud is not supported (the mesh has no triangles; give it some first: "
                                        "mvlm_mesh_triangulate_points)");
    MVLM_REQUIRE(ctx, pts_dev && snapped_dev && tri_dev && D_dev && E_dev && sweeps_dev, "geodesics: null pointer");
    MVLM_REQUIRE(ctx, aligned(pts_dev, 8) && aligned(snapped_dev, 8) && aligned(D_dev, 8) && aligned(E_dev, 8) && aligned(field_dev, 8),
                 "geodesics: the float64 arrays must be 8-byte aligned");
    MVLM_REQUIRE(ctx, aligned(tri_dev, 4) && aligned(sweeps_dev, 4), "geodesics: the int32 arrays must be 4-byte aligned");
    MVLM_REQUIRE(ctx, n >= 1 && n <= GD_MAX_LANDMARKS, "geodesics: 1..65536 landmarks per call (" + std::to_string(n) + " given)");
    MVLM_REQUIRE(ctx, init_rings >= 0 && init_rings <= GD_MAX_RINGS, "geodesics: init_rings must be in 0..8 (" + std::to_string(init_rings) + " given)");
    MVLM_REQUIRE(ctx, max_sweeps >= 0 && max_sweeps <= GD_MAX_SWEEPS,
                 "geodesics: max_sweeps must be in 1..1048576, or 0 for 4096 (" + std::to_string(max_sweeps) + " given)");
    MVLM_REQUIRE(ctx, max_scratch_bytes >= 0, "geodesics: max_scratch_bytes must not be negative (0: 512 MiB)");
    MVLM_REQUIRE(ctx, mesh->n_verts > 0 && mesh->n_verts <= (1 << 28) && mesh->n_tris <= (1 << 29), "geodesics: mesh too large or empty");
    MVLM_REQUIRE(ctx, n_pairs >= 0 && n_pairs <= (1 << 28) && (pairs_host || n_pairs == 0), "geodesics: bad pair list");
    if (max_sweeps == 0) max_sweeps = GD_DEFAULT_SWEEPS;
    if (max_scratch_bytes == 0) max_scratch_bytes = GD_DEFAULT_SCRATCH;
    const int V = mesh->n_verts, T = mesh->n_tris;

    // the sources, ascending, and each landmark's place among them
    std::vector<int> slot(size_t(n), -1), src;
    if (pairs_host) {
        for (long long p = 0; p < 2ll * n_pairs; ++p) {
            const int i = pairs_host[p];
            MVLM_REQUIRE(ctx, i >= 0 && i < n, "geodesics: pair index " + std::to_string(i) + " is outside 0.." + std::to_string(n - 1));
            slot[i] = 0;
        }
        for (int i = 0; i < n; ++i)
            if (slot[i] == 0) {
                slot[i] = int(src.size());
                src.push_back(i);
            }
    } else {
        for (int i = 0; i < n; ++i) slot[i] = i, src.push_back(i);
    }
    const int n_src = int(src.size());
    // a group's two buffers, with the quarter of headroom the context's scratch adds, stay under the cap
    const size_t per_source = size_t(V) * 2 * sizeof(double);
    const long long usable = (max_scratch_bytes - 256) / 5 * 4;
    const long long fit = usable > 0 ? usable / (long long)per_source : 0;
    MVLM_REQUIRE(ctx, fit >= 1, "geodesics: max_scratch_bytes (" + std::to_string(max_scratch_bytes) + ") cannot hold one source's two buffers of " +
                                    std::to_string(V) + " vertices (" + std::to_string(per_source + per_source / 4 + 256) + " bytes)");
    const int group = int(std::min<long long>(std::min<long long>(fit, 32768), std::max(n_src, 1)));  // (a grid's second dimension)
    const int n_groups = n_src ? (n_src + group - 1) / group : 0;

    const int n_blocks = (V + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const size_t n_ctr = size_t(n_blocks) * SCAN_BLOCK;
    auto* counts = static_cast<int*>(ctx->get_scratch("geodesic.counts", n_ctr * sizeof(int)));
    auto* starts = static_cast<int*>(ctx->get_scratch("geodesic.starts", n_ctr * sizeof(int)));
    auto* cursor = static_cast<int*>(ctx->get_scratch("geodesic.cursor", size_t(V) * sizeof(int)));
    auto* sums = static_cast<int*>(ctx->get_scratch("geodesic.sums", size_t(n_blocks) * sizeof(int)));
    auto* adj = static_cast<int2*>(ctx->get_scratch("geodesic.adj", size_t(T) * 3 * sizeof(int2)));
    auto* bary = static_cast<double*>(ctx->get_scratch("geodesic.bary", size_t(n) * 5 * sizeof(double)));
    auto* ok = static_cast<int*>(ctx->get_scratch("geodesic.ok", size_t(n) * sizeof(int)));
    auto* slot_dev = static_cast<int*>(ctx->get_scratch("geodesic.slot", size_t(n) * sizeof(int)));
    auto* src_dev = static_cast<int*>(ctx->get_scratch("geodesic.src", size_t(std::max(n_src, 1)) * sizeof(int)));
    auto* flags = static_cast<int*>(ctx->get_scratch("geodesic.flags", size_t(group) * 4 * sizeof(int)));  // cnt[3][g], state[g]
    auto* field = static_cast<double*>(ctx->get_scratch("geodesic.field", size_t(group) * per_source));
    int32_t* pairs_dev = nullptr;
    if (pairs_host) pairs_dev = static_cast<int32_t*>(ctx->get_scratch("geodesic.pairs", size_t(std::max(n_pairs, 1)) * 2 * sizeof(int32_t)));
    MVLM_REQUIRE(ctx, counts && starts && cursor && sums && adj && bary && ok && slot_dev && src_dev && flags && field &&
                          (pairs_dev || !pairs_host),
                 "geodesics: scratch allocation failed");

    hipStream_t st = ctx->stream;
    StageClock& clock = ctx->geodesic_clock;
    ctx->geodesic_groups = n_groups;
    if (clock.arm(ctx, 2 + 3 * n_groups) || clock.record(ctx, 0, st)) return 1;
    // the attachment (waits for the mesh's upload itself), then what the caller's arrays hold where nothing is computed
    if (mvlm_launch_surface_attach(ctx, mesh, pts_dev, n, snapped_dev, tri_dev, bary, bary + size_t(n) * 3)) return 1;
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(D_dev, 0xFF, size_t(n) * n * sizeof(double), st));  // NaN
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(sweeps_dev, 0xFF, size_t(n) * sizeof(int32_t), st));  // -1
    if (field_dev) MVLM_CHECK_HIP(ctx, hipMemsetAsync(field_dev, 0xFF, size_t(n) * V * sizeof(double), st));
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(slot_dev, slot.data(), size_t(n) * sizeof(int), hipMemcpyHostToDevice, st));
    if (n_src) MVLM_CHECK_HIP(ctx, hipMemcpyAsync(src_dev, src.data(), size_t(n_src) * sizeof(int), hipMemcpyHostToDevice, st));
    if (pairs_dev && n_pairs)
        MVLM_CHECK_HIP(ctx, hipMemcpyAsync(pairs_dev, pairs_host, size_t(n_pairs) * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const dim3 wg(256), per_tri(unsigned((T + 255) / 256)), per_lm(unsigned((n + 255) / 256));
    const unsigned v_chunks = unsigned((V + 255) / 256);
    hipLaunchKernelGGL(geodesic_attached_kernel, per_lm, wg, 0, st, mesh->verts, V, mesh->tris, T, snapped_dev, tri_dev, n, ok);
    hipLaunchKernelGGL(geodesic_euclid_kernel, dim3(unsigned((size_t(n) * n + 255) / 256)), wg, 0, st, snapped_dev, n, E_dev);
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, n_ctr * sizeof(int), st));
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(cursor, 0, size_t(V) * sizeof(int), st));
    hipLaunchKernelGGL(geodesic_count_kernel, per_tri, wg, 0, st, mesh->verts, V, mesh->tris, T, counts);
    hipLaunchKernelGGL(geodesic_scan_sums_kernel, dim3(n_blocks), wg, 0, st, counts, sums);
    hipLaunchKernelGGL(geodesic_scan_top_kernel, dim3(1), wg, 0, st, sums, n_blocks);
    hipLaunchKernelGGL(geodesic_scan_apply_kernel, dim3(n_blocks), wg, 0, st, counts, sums, starts);
    hipLaunchKernelGGL(geodesic_fill_kernel, per_tri, wg, 0, st, mesh->verts, V, mesh->tris, T, starts, cursor, adj);
    if (clock.record(ctx, 1, st)) return 1;
    MVLM_CHECK_HIP(ctx, hipGetLastError());

    std::vector<int> state_host(size_t(group), 0);
    for (int gi = 0; gi < n_groups; ++gi) {
        const int g0 = gi * group, g = std::min(group, n_src - g0);
        double* buf[2] = {field, field + size_t(g) * V};
        int* const cnt = flags;
        int* const state = flags + 3 * size_t(g);
        const dim3 per_source_grid(v_chunks, unsigned(g));
        MVLM_CHECK_HIP(ctx, hipMemsetAsync(cnt, 0, size_t(g) * 3 * sizeof(int), st));
        hipLaunchKernelGGL(geodesic_init_kernel, per_source_grid, wg, 0, st, mesh->verts, V, mesh->tris, snapped_dev, tri_dev, ok,
                           src_dev + g0, buf[0], state);
        for (int r = 1; r <= init_rings; ++r)
            hipLaunchKernelGGL(geodesic_ring_kernel, per_source_grid, wg, 0, st, mesh->verts, V, starts, adj, snapped_dev, src_dev + g0,
                               buf[(r - 1) & 1], buf[r & 1]);
        if (clock.record(ctx, 2 + 3 * gi, st)) return 1;
        int k = 0, running = -1;  // (the first source found running at the last read)
        bool settled = false;
        while (!settled && k < max_sweeps) {
            const int k_end = std::min(k + GD_BATCH, max_sweeps);
            for (; k < k_end; ++k)
                hipLaunchKernelGGL(geodesic_sweep_kernel, dim3(v_chunks, unsigned((g + GD_SRC_PER - 1) / GD_SRC_PER)), wg, 0, st, mesh->verts,
                                   V, starts, adj, g, k, buf[(init_rings + k) & 1], buf[(init_rings + k + 1) & 1], cnt, state);
            hipLaunchKernelGGL(geodesic_settle_kernel, dim3(unsigned((g + 255) / 256)), wg, 0, st, g, k - 1, cnt, state);
            MVLM_CHECK_HIP(ctx, hipMemcpyAsync(state_host.data(), state, size_t(g) * sizeof(int), hipMemcpyDeviceToHost, st));
            MVLM_CHECK_HIP(ctx, hipStreamSynchronize(st));
            settled = true;
            for (int s = 0; s < g && settled; ++s)
                if (state_host[s] < 0) settled = false, running = src[g0 + s];
        }
        if (!settled) {
            // no partial result: the caller's arrays say nothing
            (void)hipMemsetAsync(D_dev, 0xFF, size_t(n) * n * sizeof(double), st);
            (void)hipMemsetAsync(sweeps_dev, 0xFF, size_t(n) * sizeof(int32_t), st);
            if (field_dev) (void)hipMemsetAsync(field_dev, 0xFF, size_t(n) * V * sizeof(double), st);
            return ctx->fail("geodesics: source landmark " + std::to_string(running) + " did not settle within max_sweeps = " +
                             std::to_string(max_sweeps) + " sweeps");
        }
        if (clock.record(ctx, 3 + 3 * gi, st)) return 1;
        // (a settled source's two buffers hold the same field)
        if (pairs_dev) {
            if (n_pairs)
                hipLaunchKernelGGL(geodesic_target_kernel, dim3(unsigned((2ll * n_pairs + 255) / 256)), wg, 0, st, mesh->verts, V, mesh->tris,
                                   snapped_dev, tri_dev, ok, n, src_dev, slot_dev, g0, g, pairs_dev, n_pairs, buf[0], D_dev);
        } else {
            hipLaunchKernelGGL(geodesic_target_kernel, dim3(per_lm.x, unsigned(g)), wg, 0, st, mesh->verts, V, mesh->tris, snapped_dev, tri_dev,
                               ok, n, src_dev, slot_dev, g0, g, pairs_dev, 0, buf[0], D_dev);
        }
        hipLaunchKernelGGL(geodesic_finish_kernel, dim3(field_dev ? v_chunks : 1u, unsigned(g)), wg, 0, st, V, ok, src_dev + g0, state,
                           buf[0], sweeps_dev, field_dev);
        if (clock.record(ctx, 4 + 3 * gi, st)) return 1;
    }
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    clock.mark(2 + 3 * n_groups);
    return 0;
}

// Gives the scratch of the surface distances ("geodesic.*": the adjacency, the two field buffers, the small tables) back to the
// allocator, once the stream has run what reads it; the next call allocates again.
extern "C" int mvlm_geodesic_release(mvlm_ctx* ctx) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto it = ctx->scratch.begin(); it != ctx->scratch.end();) {
        if (it->first.rfind("geodesic.", 0) == 0) {
            if (it->second.first) (void)hipFree(it->second.first);
            it = ctx->scratch.erase(it);
        } else {
            ++it;
        }
    }
    return 0;
}

// Milliseconds of the last call's adjacency (with the attachment), init, sweeps and targets - the last three added up over the
// call's source groups - while mvlm_render_set_profiling is on; waits for the stream.
extern "C" int mvlm_geodesic_stage_ms(mvlm_ctx* ctx, float* ms4) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms4, "geodesic_stage_ms: null pointer");
    const int m = 1 + 3 * ctx->geodesic_groups;
    std::vector<float> ms(size_t(m), 0.f);
    if (ctx->geodesic_clock.read(ctx, m, ms.data(), "geodesic_stage_ms: no surface distances were computed with render profiling on")) return 1;
    ms4[0] = ms[0], ms4[1] = ms4[2] = ms4[3] = 0.f;
    for (int gi = 0; gi < ctx->geodesic_groups; ++gi)
        for (int q = 0; q < 3; ++q) ms4[1 + q] += ms[1 + 3 * gi + q];
    return 0;
}
