// The binning front end of the rasteriser, stated once for its four launch sets - the network's render (raster.hip), its
// 4-sample form (raster_ms.hip, raster_vc.hip), the landmark view (raster_view.hip) and the ray view (raster_rays.hip): append
// the big triangles, count them into tiles, scatter them into the per-tile lists, resolve the small ones, the tile stage's
// prologue and overflow word, and on the host the scratch the stages share.  Included through raster_common.h, whose names it
// uses.  The kernels keep their names and signatures; their machine code stays what it was (tools/device_code_diff.py), which
// is why an index is formed inside a helper, in the type its caller formed it in (the Index parameters).
// Not here, for want of shared text: the two transform kernels (rm_transform / rv_transform); the two scan kernels (scan_kernel:
// one thread per counter over exactly 256 tiles, in every step of the network path; view_scan_kernel: any tile count, saturated
// offsets, 64-bit sums); the walk over a tile's big triangles (tile_body has the 24-bit path, view_tile_resolve has not); the
// multisampled small-box resolve (S keys per pixel) and shading.  Not here because classify_kernel / the views' tile kernels came
// out of every helper tried as other machine code: classify_one's 24-bit small-box loop; the ballot compaction of spheres and of
// rays into LDS lists (five shared lines; their barriers differ on purpose).
#ifndef MVLM_RASTER_BINS_H
#define MVLM_RASTER_BINS_H

namespace {

// The ids of a wave's big triangles are appended to the view's list (n_tris entries) with ONE atomicAdd per wave: a coarse mesh -
// every triangle big - made 3 000 returning atomics on one counter per view, 54 us for 3 042 triangles (now 6).
__device__ __forceinline__ void append_big(bool big, int t, int view, int n_tris, int* __restrict__ n_big,
                                           int* __restrict__ big_list) {
    const int lane = int(threadIdx.x) & 63;
    const unsigned long long m = __ballot(big);
    if (m) {  // (wave-uniform)
        const int leader = __ffsll(static_cast<long long>(m)) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&n_big[view], __popcll(m));
        base = __shfl(base, leader);
        if (big) big_list[size_t(view) * n_tris + base + __popcll(m & ((1ull << lane) - 1ull))] = t;
    }
}

// A big triangle with the pixel box [ix0, ix1] x [iy0, iy1] is counted into every 16 x 16 tile the box touches.  Index: the type
// a (view, tile) index is formed in - int where a view has the constant 256 tiles, size_t for a runtime count (up to 16 384).
template <class Index>
__device__ __forceinline__ void count_tile_range(int* __restrict__ counts, int view, int tiles_x, int ix0, int ix1, int iy0,
                                                 int iy1) {
    const int tx0 = ix0 / RM_TILE, tx1 = ix1 / RM_TILE, ty0 = iy0 / RM_TILE, ty1 = iy1 / RM_TILE;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&counts[Index(view) * tiles_x * tiles_x + ty * tiles_x + tx], 1);
}

// The small-triangle loop: every pixel centre of the box that `cover` finds inside the triangle and whose depth lies in the
// clip range takes the (depth, id) key with a 64-bit atomicMin.  kv: the view's key plane; Index: int for the 256 x 256 window.
template <class Tri, int (*cover)(const Tri*, int, int, float*, float*, float*), class Index>
__device__ __forceinline__ void resolve_small_box(unsigned long long* kv, int row_stride, int ix0, int ix1, int iy0, int iy1,
                                                  const Tri& __restrict__ tr, int id) {
    for (int j = iy0; j <= iy1; ++j)
        for (int ii = ix0; ii <= ix1; ++ii) {
            float b0, b1, b2;
            if (!cover(&tr, ii, j, &b0, &b1, &b2)) continue;
            const float z = rm_interp(b0, b1, b2, tr.z0, tr.z1, tr.z2);
            if (!(z >= 0.0f && z <= 1.0f)) continue;  // near / far clip (render3d.py:136)
            atomicMin(&kv[Index(j) * row_stride + ii], (unsigned long long)rm_key(z, uint32_t(id)));
        }
}

// Triangle t into the list of every tile its pixel box touches (offsets from the scan).  An entry outside the view's `cap` entries
// of bins - a negative position among them: no input gives one today, offsets are sums of counts - is dropped and raises the flag.
template <class Index>
__device__ __forceinline__ void scatter_tile_range(int view, int tiles_x, const int* __restrict__ offsets, int* __restrict__ cursors,
                                                   int* __restrict__ bins, int cap, int* __restrict__ overflow, int ix0, int ix1,
                                                   int iy0, int iy1, int t) {
    const int tx0 = ix0 / RM_TILE, tx1 = ix1 / RM_TILE, ty0 = iy0 / RM_TILE, ty1 = iy1 / RM_TILE;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const Index tile = Index(view) * tiles_x * tiles_x + ty * tiles_x + tx;
            const int pos = offsets[tile] + atomicAdd(&cursors[tile], 1);
            if (pos >= 0 && pos < cap)
                bins[size_t(view) * cap + pos] = t;
            else
                *overflow = 1;
        }
}

// What a workgroup of a tile stage - one per (view, 16 x 16 tile) as view_chunk hands them out, a thread per pixel - works on
// (Index: as in count_tile_range).
struct tile_slot {
    int x0, y0, i, j;   // the tile's first pixel, the thread's pixel
    const vert12* tvv;  // the view's transformed vertices
    int n;              // big triangles in the tile's list: what fits the view's capacity
    const int* list;    // their ids
};
template <class Index>
__device__ __forceinline__ tile_slot tile_prologue(int view, int tile, int tiles_x, const vert12* __restrict__ tv, int n_verts,
                                                   const int* __restrict__ counts, const int* __restrict__ offsets,
                                                   const int* __restrict__ bins, int cap) {
    const Index vt = Index(view) * (tiles_x * tiles_x) + tile;
    const int tid = threadIdx.x;
    tile_slot s;
    s.x0 = (tile % tiles_x) * RM_TILE;
    s.y0 = (tile / tiles_x) * RM_TILE;
    s.i = s.x0 + (tid & (RM_TILE - 1));
    s.j = s.y0 + (tid >> 4);
    s.tvv = tv + size_t(view) * n_verts;
    s.n = min(counts[vt], cap - offsets[vt]);
    s.list = bins + size_t(view) * cap + offsets[vt];
    return s;
}

// The first workgroup carries the overflow flag of the kernels before the tile stage to the host's pinned word (no copy node).
__device__ __forceinline__ void publish_overflow(const int* __restrict__ overflow, int* __restrict__ overflow_host) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        __atomic_store_n(overflow_host, *overflow, __ATOMIC_RELAXED);
        __threadfence_system();
    }
}

}  // namespace

// The scratch of one launch set's binning stages: the context's "<prefix>.ctr" (counts | cursors | n_big | overflow: ctr_ints
// ints from `counts` on, cleared by one memset), ".off", ".bins" and ".big".
struct raster_bins {
    int *counts, *cursors, *n_big, *overflow, *offsets, *bins, *big_list;
    int cap;  // tile-list entries per view; larger lists raise an error (mvlm_render_check)
    size_t ctr_ints;
};
// prefix: "raster" (mvlm_render) or "view" (landmark and ray views); tiles: per view; T: triangles.  False: an allocation failed.
inline bool raster_bins_scratch(mvlm_ctx* ctx, const char* prefix, int n_views, int tiles, int T, int cap, raster_bins* b) {
    const std::string p(prefix);
    const size_t n_ctr = size_t(n_views) * tiles;
    b->cap = cap;
    b->ctr_ints = 2 * n_ctr + n_views + 4;
    b->counts = static_cast<int*>(ctx->get_scratch((p + ".ctr").c_str(), b->ctr_ints * sizeof(int)));
    b->offsets = static_cast<int*>(ctx->get_scratch((p + ".off").c_str(), n_ctr * sizeof(int)));
    b->bins = static_cast<int*>(ctx->get_scratch((p + ".bins").c_str(), size_t(n_views) * cap * sizeof(int)));
    b->big_list = static_cast<int*>(ctx->get_scratch((p + ".big").c_str(), size_t(n_views) * T * sizeof(int)));
    if (!(b->counts && b->offsets && b->bins && b->big_list)) return false;
    b->cursors = b->counts + n_ctr;
    b->n_big = b->counts + 2 * n_ctr;
    b->overflow = b->n_big + n_views;
    return true;
}

// The pinned host word of publish_overflow, allocated and zeroed on first use (a launch set that fails before its tile kernel
// leaves no garbage for mvlm_render_check); null when the allocation failed.
inline int* render_overflow_word(mvlm_ctx* ctx) {
    if (!ctx->render_overflow_host) {
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->render_overflow_host), sizeof(int)) != hipSuccess) return nullptr;
        *ctx->render_overflow_host = 0;
    }
    return ctx->render_overflow_host;
}

#endif
