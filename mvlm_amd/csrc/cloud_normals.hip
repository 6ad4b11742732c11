// Normals of a point cloud (a mesh uploaded with n_tris == 0): the estimate - per point the least-variance direction of its 16
// nearest neighbours - and the tile stage that shades a cloud's splats with them (cloud_normals_math.h holds the contract,
// DESIGN.md 5.1 "Point clouds").  mvlm_render (raster.hip) branches to the tile stage in host code; the splat kernel of
// raster_points.hip runs before it, unchanged.
//
// The estimate, mvlm_mesh_estimate_normals, in three stages, nothing returns to the host:
//   grid    bounds   bounding box and number of the finite points (order-independent atomics: max of encoded floats, a count)
//           grid     one thread: the cell edge h = 2 s, s the spacing mvlm_points_auto_radius derives (sqrt(ex ey / n)), grown
//                    until the cells fit the budget; a zero extent gives one layer of cells
//           count    one thread per point: its cell, one atomicAdd on the cell's counter
//           scan     exclusive prefix sum over the counters: per-block sums, one block over those, per-block apply
//           scatter  one thread per point: (x, y, z, id) into its cell's slice of the sorted array
//   search  one thread per sorted slot - a wave's threads sit in the same few cells and walk the same ones: Chebyshev shells
//           r = 0, 1, 2, ... of cells round the point's own, every row of a shell one contiguous slice of the sorted array; the
//           16 best (d2, id) are kept in LDS, sorted; after shell r nothing unvisited is nearer than r h, so the walk ends when the
//           list is full and its last d2 lies strictly below ((1 - 1e-6) r h)^2 - the margin covers the rounding of a cell index -
//           and in any case when the shells cover the grid
//   solve   one thread per point: centroid, covariance and the Jacobi eigenvector of its row (cn_normal)
// The order of the sorted array inside a cell depends on how the scatter's atomics land; the list of the 16 least (d2, id) does
// not, and the sums run in the list's order: the table and the normals are the same bytes from run to run.
// Built as an object of its own (build/normals/, tests/golden/kernel_occupancy_normals.json): no kernel here uses scratch memory.
#include "raster_common.h"
#include "raster_points_math.h"
#include "cloud_normals_math.h"

#include <algorithm>

namespace {

constexpr int MAX_CELLS = 1 << 21;   // the grid's budget of cells is min(max(8 V, 64), this)
constexpr int SCAN_PER_THREAD = 16;  // counters per thread of a scan block
constexpr int SCAN_BLOCK = 256 * SCAN_PER_THREAD;

// What the grid kernels hand to each other (device memory, cleared by one memset before the bounds kernel).
struct cn_grid {
    unsigned neg_lo[3], hi[3];  // max of ~enc(x) and of enc(x) over the finite points, enc: order-preserving float -> unsigned
    int n_finite;
    int dims[3], n_cells, r_max;
    double lo[3], h, inv_h;
};

__device__ inline unsigned enc_float(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float dec_float(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }

// At most BOUNDS_WGS workgroups stride over the points and leave seven atomics each: one per wave of a grid sized by the points
// (110 000 atomics on seven addresses at 1 M points) took 1.24 ms.
constexpr int BOUNDS_WGS = 256;
__global__ __launch_bounds__(256) void normals_bounds_kernel(const float* __restrict__ verts, int n_points, cn_grid* __restrict__ g) {
    __shared__ unsigned s_v[4][6];
    __shared__ int s_n[4];
    unsigned v[6] = {0, 0, 0, 0, 0, 0};
    int n = 0;
    for (size_t p = size_t(blockIdx.x) * 256 + threadIdx.x; p < size_t(n_points); p += size_t(gridDim.x) * 256) {
        const float x = verts[3 * p], y = verts[3 * p + 1], z = verts[3 * p + 2];
        if (rp_finite3(x, y, z)) {
            ++n;
            v[0] = max(v[0], ~enc_float(x)), v[1] = max(v[1], ~enc_float(y)), v[2] = max(v[2], ~enc_float(z));
            v[3] = max(v[3], enc_float(x)), v[4] = max(v[4], enc_float(y)), v[5] = max(v[5], enc_float(z));
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = max(v[k], __shfl_down(v[k], s));
        n += __shfl_down(n, s);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_v[wave][k] = v[k];
        s_n[wave] = n;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        const unsigned m = max(max(s_v[0][k], s_v[1][k]), max(s_v[2][k], s_v[3][k]));
        if (m) atomicMax(k < 3 ? &g->neg_lo[k] : &g->hi[k - 3], m);  // (0: no finite point here, and the cleared word's value)
    } else if (threadIdx.x == 6) {
        const int total = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
        if (total) atomicAdd(&g->n_finite, total);
    }
}

// cells along an extent e at edge h, as a double (at least 1; huge ratios stay finite)
__device__ inline double cells_along(double e, double h) {
    const double d = floor(e / h) + 1.0;
    return d < 1.0 ? 1.0 : (d > 4.0e9 ? 4.0e9 : d);
}

__global__ void normals_grid_kernel(cn_grid* __restrict__ g, int budget) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n = g->n_finite;
    double lo[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
    if (n > 0)
        for (int k = 0; k < 3; ++k) {
            lo[k] = double(dec_float(~g->neg_lo[k]));
            e[k] = double(dec_float(g->hi[k])) - lo[k];
        }
    const double e2 = fmax(e[0], fmax(e[1], e[2])), e0 = fmin(e[0], fmin(e[1], e[2])), e1 = ((e[0] + e[1]) + e[2]) - e2 - e0;
    const double emid = fmin(fmax(e1, e0), e2);  // (the middle extent; the sum above may round: kept inside [e0, e2])
    double h = n > 0 ? 2.0 * sqrt(e2 * emid / double(n)) : 1.0;
    if (!(h > 0.0) || !isfinite(h)) h = n > 0 ? 2.0 * e2 / double(n) : 1.0;  // collinear points: twice their spacing
    if (!(h > 0.0) || !isfinite(h)) h = 1.0;                                   // one location
    double d[3] = {1.0, 1.0, 1.0};
    bool fits = false;
    for (int it = 0; it < 96 && !fits; ++it) {
        for (int k = 0; k < 3; ++k) d[k] = cells_along(e[k], h);
        const double cells = d[0] * d[1] * d[2];
        fits = cells <= double(budget);
        if (!fits) h *= fmax(1.05, cbrt(cells / double(budget)));
    }
    if (!fits || !isfinite(h)) {  // (not reached by finite extents; one cell is always right)
        d[0] = d[1] = d[2] = 1.0;
        h = fmax(e2, 1.0) * 2.0;
    }
    for (int k = 0; k < 3; ++k) {
        g->dims[k] = int(d[k]);
        g->lo[k] = lo[k];
    }
    g->n_cells = int(d[0]) * int(d[1]) * int(d[2]);
    g->r_max = max(int(d[0]), max(int(d[1]), int(d[2]))) - 1;
    g->h = h;
    g->inv_h = 1.0 / h;
}

__device__ inline int cell_coord(double x, double lo, double inv_h, int dim) {
    const int c = int(floor((x - lo) * inv_h));
    return c < 0 ? 0 : (c > dim - 1 ? dim - 1 : c);
}

// the cell of every point (-1: not finite) and the cells' populations
__global__ __launch_bounds__(256) void normals_count_kernel(const float* __restrict__ verts, int n_points, const cn_grid* __restrict__ g,
                                                            int* __restrict__ cell_of, int* __restrict__ counts) {
    const int p = blockIdx.x * 256 + int(threadIdx.x);
    if (p >= n_points) return;
    const float x = verts[3 * size_t(p)], y = verts[3 * size_t(p) + 1], z = verts[3 * size_t(p) + 2];
    int cell = -1;
    if (rp_finite3(x, y, z)) {
        const int cx = cell_coord(x, g->lo[0], g->inv_h, g->dims[0]), cy = cell_coord(y, g->lo[1], g->inv_h, g->dims[1]),
                  cz = cell_coord(z, g->lo[2], g->inv_h, g->dims[2]);
        cell = (cz * g->dims[1] + cy) * g->dims[0] + cx;  // x runs fastest: a row of cells along x is one slice of the sorted array
        atomicAdd(&counts[cell], 1);
    }
    cell_of[p] = cell;
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

__global__ __launch_bounds__(256) void normals_scan_sums_kernel(const int* __restrict__ counts, int* __restrict__ block_sums) {
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

// exclusive scan of the block sums in place: one workgroup, any number of blocks (a carry runs over slices of 256)
__global__ __launch_bounds__(256) void normals_scan_top_kernel(int* __restrict__ block_sums, int n_blocks) {
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

__global__ __launch_bounds__(256) void normals_scan_apply_kernel(const int* __restrict__ counts, const int* __restrict__ block_sums,
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

__global__ __launch_bounds__(256) void normals_scatter_kernel(const float* __restrict__ verts, int n_points, const int* __restrict__ cell_of,
                                                              const int* __restrict__ starts, int* __restrict__ cursors,
                                                              float4* __restrict__ sorted) {
    const int p = blockIdx.x * 256 + int(threadIdx.x);
    if (p >= n_points) return;
    const int cell = cell_of[p];
    if (cell < 0) return;
    const int pos = starts[cell] + atomicAdd(&cursors[cell], 1);
    sorted[pos] = make_float4(verts[3 * size_t(p)], verts[3 * size_t(p) + 1], verts[3 * size_t(p) + 2], __int_as_float(p));
}

// The thread's list of the CN_K least (d2, id), ascending, in LDS: element k of thread t at [k][t] (no bank conflicts).
struct top_list {
    double (*d)[256];
    int (*i)[256];
    int n;
    double worst_d;  // of the last element once the list is full
    int worst_i;
};

// returns whether the candidate entered the list
__device__ inline bool top_insert(top_list& L, double d2, int id) {
    const int t = threadIdx.x;
    if (L.n == CN_K && !cn_before(d2, id, L.worst_d, L.worst_i)) return false;
    int j = L.n < CN_K ? L.n : CN_K - 1;  // the slot that opens: behind the list, or its last element drops out
    while (j > 0 && cn_before(d2, id, L.d[j - 1][t], L.i[j - 1][t])) {
        L.d[j][t] = L.d[j - 1][t];
        L.i[j][t] = L.i[j - 1][t];
        --j;
    }
    L.d[j][t] = d2;
    L.i[j][t] = id;
    if (L.n < CN_K) ++L.n;
    if (L.n == CN_K) {
        L.worst_d = L.d[CN_K - 1][t];
        L.worst_i = L.i[CN_K - 1][t];
    }
    return true;
}

// the candidates of one slice of the sorted array; returns how many of them entered the list
__device__ inline unsigned top_visit(top_list& L, const float4* __restrict__ sorted, int a, int b, double px, double py, double pz) {
    unsigned entered = 0;
    for (int q = a; q < b; ++q) {
        const float4 c = sorted[q];
        entered += top_insert(L, cn_d2(double(c.x), double(c.y), double(c.z), px, py, pz), __float_as_int(c.w)) ? 1u : 0u;
    }
    return entered;
}

// COUNT: the measuring form (mvlm_points_set_counting) also sums, over all points, the shells walked, the candidates tested and the
// candidates that entered a list (mvlm_normals_get_stats)
template <bool COUNT>
__global__ __launch_bounds__(256) void normals_search_kernel(const float4* __restrict__ sorted, const int* __restrict__ starts,
                                                             const cn_grid* __restrict__ g, int32_t* __restrict__ neighbors,
                                                             unsigned long long* __restrict__ stats) {
    __shared__ double s_d[CN_K][256];
    __shared__ int s_i[CN_K][256];
    const int slot = blockIdx.x * 256 + int(threadIdx.x);
    if (slot >= g->n_finite) return;
    const int nx = g->dims[0], ny = g->dims[1], nz = g->dims[2], r_max = g->r_max;
    const double h = g->h;
    const float4 me = sorted[slot];
    const double px = me.x, py = me.y, pz = me.z;
    const int cx = cell_coord(px, g->lo[0], g->inv_h, nx), cy = cell_coord(py, g->lo[1], g->inv_h, ny),
              cz = cell_coord(pz, g->lo[2], g->inv_h, nz);
    top_list L{s_d, s_i, 0, 0.0, 0};
    unsigned shells = 0, tested = 0, entered = 0;
    for (int r = 0; r <= r_max; ++r) {
        if (COUNT) ++shells;
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * ny + y) * nx;
                if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {  // a face of the shell: the whole row of cells
                    const int a = starts[row + x0], b = starts[row + x1 + 1];
                    const unsigned e = top_visit(L, sorted, a, b, px, py, pz);
                    if (COUNT) tested += unsigned(b - a), entered += e;
                } else {  // inside: the two end cells, where the grid has them
                    if (cx - r >= 0) {
                        const int a = starts[row + cx - r], b = starts[row + cx - r + 1];
                        const unsigned e = top_visit(L, sorted, a, b, px, py, pz);
                        if (COUNT) tested += unsigned(b - a), entered += e;
                    }
                    if (cx + r <= nx - 1) {
                        const int a = starts[row + cx + r], b = starts[row + cx + r + 1];
                        const unsigned e = top_visit(L, sorted, a, b, px, py, pz);
                        if (COUNT) tested += unsigned(b - a), entered += e;
                    }
                }
            }
        const double reach = (1.0 - 1e-6) * (double(r) * h);
        if (L.n == CN_K && L.worst_d < reach * reach) break;
    }
    const int id = __float_as_int(me.w);
#pragma unroll
    for (int k = 0; k < CN_K; ++k) neighbors[size_t(id) * CN_K + k] = k < L.n ? s_i[k][threadIdx.x] : -1;
    if (COUNT) {
        atomicAdd(&stats[0], (unsigned long long)shells);
        atomicAdd(&stats[1], (unsigned long long)tested);
        atomicAdd(&stats[2], (unsigned long long)entered);
    }
}

__global__ __launch_bounds__(256) void normals_solve_kernel(const float* __restrict__ verts, int n_points,
                                                            const int32_t* __restrict__ neighbors, float* __restrict__ normals) {
    const int p = blockIdx.x * 256 + int(threadIdx.x);
    if (p >= n_points) return;
    const int32_t* const row = neighbors + size_t(p) * CN_K;
    int n = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = 0; k < CN_K; ++k) {
        const int q = row[k];
        if (q < 0) break;
        sx += double(verts[3 * size_t(q)]);
        sy += double(verts[3 * size_t(q) + 1]);
        sz += double(verts[3 * size_t(q) + 2]);
        ++n;
    }
    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    if (n > 0) {
        const double mx = sx / double(n), my = sy / double(n), mz = sz / double(n);
        for (int k = 0; k < n; ++k) {
            const int q = row[k];
            const double dx = double(verts[3 * size_t(q)]) - mx, dy = double(verts[3 * size_t(q) + 1]) - my,
                         dz = double(verts[3 * size_t(q) + 2]) - mz;
            cxx += dx * dx;
            cxy += dx * dy;
            cxz += dx * dz;
            cyy += dy * dy;
            cyz += dy * dz;
            czz += dz * dz;
        }
    }
    float out[3];
    cn_normal(n, cxx, cxy, cxz, cyy, cyz, czz, out);
    normals[3 * size_t(p)] = out[0];
    normals[3 * size_t(p) + 1] = out[1];
    normals[3 * size_t(p) + 2] = out[2];
}

// points_tile_kernel (raster_points.hip) with the shade of the winner's normal in planes 0..2
__global__ __launch_bounds__(256) void normals_tile_kernel(const float* __restrict__ normals, const double* __restrict__ rot,
                                                           unsigned long long* __restrict__ keys, size_t n_pixels,
                                                           int* __restrict__ overflow_host, float* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (nothing can overflow: mvlm_render_check reads a zero of this render)
        __atomic_store_n(overflow_host, 0, __ATOMIC_RELAXED);
        __threadfence_system();
    }
    const size_t g = size_t(blockIdx.x) * 256 + threadIdx.x;  // view * 65536 + j * 256 + i, j counting up from the bottom row
    if (g >= n_pixels) return;
    const uint64_t best = keys[g];
    const size_t view = g / (RM_SIZE * RM_SIZE);
    float4 px = make_float4(1.f, 1.f, 1.f, float(rm_depth_u8(1.0f)) / 255.0f);  // white background, far plane
    if (best != RM_KEY_EMPTY) {
        keys[g] = RM_KEY_EMPTY;
        const size_t p = rm_key_tri(best);
        const float s = float(cn_shade_u8(rot + view * 9, normals[3 * p], normals[3 * p + 1], normals[3 * p + 2])) / 255.0f;
        px = make_float4(s, s, s, float(rm_depth_u8(rm_key_z(best))) / 255.0f);
    }
    const int j = int((g / RM_SIZE) % RM_SIZE), i = int(g % RM_SIZE);
    // np.flip(axis=1): GL row j (bottom-up) is image row 255 - j (render3d.py:177)
    reinterpret_cast<float4*>(out)[(view * RM_SIZE + size_t(RM_SIZE - 1 - j)) * RM_SIZE + i] = px;
}

}  // namespace

void cloud_normals_tile_launch(hipStream_t stream, const float* normals, const double* rot, int n_views, unsigned long long* keys,
                               int* overflow_host, float* out) {
    const size_t n_pixels = size_t(n_views) * RM_SIZE * RM_SIZE;
    hipLaunchKernelGGL(normals_tile_kernel, dim3(unsigned((n_pixels + 255) / 256)), dim3(256), 0, stream, normals, rot, keys, n_pixels,
                       overflow_host, out);
}

extern "C" int mvlm_mesh_estimate_normals(mvlm_ctx* ctx, mvlm_mesh* mesh, int32_t* neighbors_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, mesh, "mesh_estimate_normals: null mesh");
    MVLM_REQUIRE(ctx, mesh->n_tris == 0, "mesh_estimate_normals: the mesh has triangles (normals are estimated for a point cloud)");
    MVLM_REQUIRE(ctx, mesh->n_verts > 0 && mesh->n_verts <= (1 << 27), "mesh_estimate_normals: 1 to 134217728 points");
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;
    const int V = mesh->n_verts;
    const int budget = int(std::min<long long>(std::max<long long>(8ll * V, 64), MAX_CELLS));
    const int n_blocks = (budget + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;  // (one counter past the last cell: starts[n_cells] is read)
    const size_t n_ctr = size_t(n_blocks) * SCAN_BLOCK;
    auto* grid = static_cast<cn_grid*>(ctx->get_scratch("normals.grid", sizeof(cn_grid)));
    auto* ctr = static_cast<int*>(ctx->get_scratch("normals.ctr", 2 * n_ctr * sizeof(int)));  // counts | cursors: one memset
    auto* starts = static_cast<int*>(ctx->get_scratch("normals.starts", n_ctr * sizeof(int)));
    auto* sums = static_cast<int*>(ctx->get_scratch("normals.sums", size_t(n_blocks) * sizeof(int)));
    auto* cell_of = static_cast<int*>(ctx->get_scratch("normals.cell", size_t(V) * sizeof(int)));
    auto* sorted = static_cast<float4*>(ctx->get_scratch("normals.sorted", size_t(V) * sizeof(float4)));
    int32_t* nbr = neighbors_dev;
    if (!nbr) nbr = static_cast<int32_t*>(ctx->get_scratch("normals.nbr", size_t(V) * CN_K * sizeof(int32_t)));
    MVLM_REQUIRE(ctx, grid && ctr && starts && sums && cell_of && sorted && nbr, "mesh_estimate_normals: scratch allocation failed");
    unsigned long long* stats = nullptr;  // (mvlm_points_set_counting: the search kernel's measuring form)
    if (ctx->points_counting) {
        stats = static_cast<unsigned long long*>(ctx->get_scratch("normals.stats", 3 * sizeof(unsigned long long)));
        MVLM_REQUIRE(ctx, stats, "mesh_estimate_normals: scratch allocation failed");
        MVLM_CHECK_HIP(ctx, hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), ctx->stream));
    }
    float* const normals = mvlm_mesh_normals_buffer(ctx, mesh);
    MVLM_REQUIRE(ctx, normals, "mesh_estimate_normals: device allocation failed");
    StageClock& clock = ctx->normals_clock;  // (profiling: events round the three stages, mvlm_normals_stage_ms)
    clock.invalidate();
    if (clock.arm(ctx, 4) || clock.record(ctx, 0, ctx->stream)) return 1;
    const dim3 per_point(unsigned((V + 255) / 256)), wg(256);
    int* const counts = ctr;
    int* const cursors = ctr + n_ctr;
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(grid, 0, sizeof(cn_grid), ctx->stream));
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(ctr, 0, 2 * n_ctr * sizeof(int), ctx->stream));
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(nbr, 0xFF, size_t(V) * CN_K * sizeof(int32_t), ctx->stream));  // -1: rows nobody writes
    hipLaunchKernelGGL(normals_bounds_kernel, dim3(std::min(per_point.x, unsigned(BOUNDS_WGS))), wg, 0, ctx->stream, mesh->verts, V, grid);
    hipLaunchKernelGGL(normals_grid_kernel, dim3(1), dim3(64), 0, ctx->stream, grid, budget);
    hipLaunchKernelGGL(normals_count_kernel, per_point, wg, 0, ctx->stream, mesh->verts, V, grid, cell_of, counts);
    hipLaunchKernelGGL(normals_scan_sums_kernel, dim3(n_blocks), wg, 0, ctx->stream, counts, sums);
    hipLaunchKernelGGL(normals_scan_top_kernel, dim3(1), wg, 0, ctx->stream, sums, n_blocks);
    hipLaunchKernelGGL(normals_scan_apply_kernel, dim3(n_blocks), wg, 0, ctx->stream, counts, sums, starts);
    hipLaunchKernelGGL(normals_scatter_kernel, per_point, wg, 0, ctx->stream, mesh->verts, V, cell_of, starts, cursors, sorted);
    if (clock.record(ctx, 1, ctx->stream)) return 1;
    if (stats)
        hipLaunchKernelGGL(normals_search_kernel<true>, per_point, wg, 0, ctx->stream, sorted, starts, grid, nbr, stats);
    else
        hipLaunchKernelGGL(normals_search_kernel<false>, per_point, wg, 0, ctx->stream, sorted, starts, grid, nbr, stats);
    if (clock.record(ctx, 2, ctx->stream)) return 1;
    hipLaunchKernelGGL(normals_solve_kernel, per_point, wg, 0, ctx->stream, mesh->verts, V, nbr, normals);
    if (clock.record(ctx, 3, ctx->stream)) return 1;
    clock.mark(4);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    mesh->normals = normals;
    return 0;
}

extern "C" int mvlm_mesh_copy_normals(mvlm_ctx* ctx, const mvlm_mesh* mesh, float* normals_host) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, mesh && normals_host, "mesh_copy_normals: null pointer");
    MVLM_REQUIRE(ctx, mesh->normals, "mesh_copy_normals: the mesh has no normals");
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(normals_host, mesh->normals, size_t(mesh->n_verts) * 3 * sizeof(float), hipMemcpyDeviceToHost,
                                       ctx->stream));
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Measuring hook (tools/cloud_normals_bench.py): what the LAST estimate made with mvlm_points_set_counting on summed over all
// points - stats3[0] shells walked, [1] candidates tested, [2] candidates that entered a list; waits for the stream.
extern "C" int mvlm_normals_get_stats(mvlm_ctx* ctx, unsigned long long* stats3) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, stats3, "normals_get_stats: null pointer");
    const auto it = ctx->scratch.find("normals.stats");
    MVLM_REQUIRE(ctx, it != ctx->scratch.end() && it->second.first, "normals_get_stats: no normals have been estimated with counting on");
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(stats3, it->second.first, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Milliseconds of the last estimate's three stages - grid build, search, solve - while mvlm_render_set_profiling is on; waits for
// the stream.
extern "C" int mvlm_normals_stage_ms(mvlm_ctx* ctx, float* ms3) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms3, "normals_stage_ms: null pointer");
    return ctx->normals_clock.read(ctx, 3, ms3, "normals_stage_ms: no normals were estimated with render profiling on");
}
