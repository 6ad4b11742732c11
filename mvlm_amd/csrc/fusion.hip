// Heatmap maxima -> 3-D view rays -> per-landmark consensus, one wavefront per landmark.
// Replaces three pure-Python double loops of the reference:
//   Estimator3D.estimate_landmark_lines            src/mvlm/utils/estimator3d.py:31-90
//   filter_lines_based_on_heatmap_value_*          estimator3d.py:140-155
//   compute_intersection_between_lines_ransac      estimator3d.py:92-137
//   compute_intersection_between_lines (pinv 3x3)  src/mvlm/utils/utils3d.py:99-124
// The arithmetic keeps the reference's dtypes: pixel -> model units in float32 (numpy
// float32 scalars with weak python ints), everything after that in float64.  The build
// uses -ffp-contract=off so no fused multiply-add changes a rounding.
#include "common.h"
#include "consensus_math.h"

namespace {

__global__ void lines_kernel(const float* __restrict__ maxima, const double* __restrict__ rot, int n_views, int nl,
                             float img_size, double* __restrict__ starts, double* __restrict__ ends) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_views * nl) return;
    const int v = i % n_views;
    float y = maxima[size_t(i) * 3 + 0];
    float x = maxima[size_t(i) * 3 + 1];
    // estimator3d.py:66-67 (heatmap size == image size) and :73-78, all float32
    y = y / img_size * img_size;
    x = x / img_size * img_size;
    const float px = (x / img_size) * 300.0f + (-150.0f);
    const float py = ((img_size - 1.0f - y) / img_size) * 300.0f + (-150.0f);
    // points = t.T @ [px, py, +-500, 1]  with t[0:3,0:3] = M (estimator3d.py:56-57, :83)
    const double* m = rot + size_t(v) * 9;
    const double dx = px, dy = py;
    for (int k = 0; k < 3; ++k) {
        const double base = m[0 * 3 + k] * dx + m[1 * 3 + k] * dy;
        starts[size_t(i) * 3 + k] = base + m[2 * 3 + k] * 500.0;
        ends[size_t(i) * 3 + k] = base + m[2 * 3 + k] * -500.0;
    }
}

// One wave per landmark.  np.quantile(values, q) with method "linear" on a float32 vector
// (numpy >= 2: q is cast to the array dtype, the interpolation runs in float32), then
// mask = values > threshold (estimator3d.py:141-143); or the absolute test (:151-152).
__global__ __launch_bounds__(64) void mask_kernel(const float* __restrict__ maxima, int n_views, int mode, float q,
                                                  float thr_abs, uint8_t* __restrict__ mask,
                                                  int* __restrict__ count) {
    __shared__ float vals[MAX_VIEWS];
    const int lm = blockIdx.x, lane = threadIdx.x;
    for (int v = lane; v < n_views; v += 64) vals[v] = maxima[(size_t(lm) * n_views + v) * 3 + 2];
    __syncthreads();
    float thr = thr_abs;
    if (mode == MVLM_MODE_QUANTILE) {
        const float vi = float(n_views - 1) * q;
        int lo = int(floorf(vi)), hi = lo + 1;
        if (vi >= float(n_views - 1)) lo = hi = n_views - 1;
        if (vi < 0.f) lo = hi = 0;
        if (hi > n_views - 1) hi = n_views - 1;
        const float gamma = vi - floorf(vi);
        // order statistics by rank counting (stable for ties); NaN anywhere -> NaN result
        float a = 0.f, b = 0.f;
        bool have_a = false, have_b = false, any_nan = false;
        for (int i = lane; i < n_views; i += 64) {
            const float x = vals[i];
            if (x != x) any_nan = true;
            int rank = 0;
            for (int j = 0; j < n_views; ++j) {
                const float yv = vals[j];
                rank += (yv < x) || (yv == x && j < i);
            }
            if (rank == lo) {
                a = x;
                have_a = true;
            }
            if (rank == hi) {
                b = x;
                have_b = true;
            }
        }
        // broadcast the two order statistics
        const unsigned long long ma = __ballot(have_a), mb = __ballot(have_b);
        any_nan = __any(any_nan);
        a = __shfl(a, ma ? __ffsll((long long)ma) - 1 : 0);
        b = __shfl(b, mb ? __ffsll((long long)mb) - 1 : 0);
        // numpy _lerp: a + (b-a)*t, replaced by b - (b-a)*(1-t) where t >= 0.5
        const float diff = b - a;
        float r = a + diff * gamma;
        if (gamma >= 0.5f) r = b - diff * (1.0f - gamma);
        thr = any_nan ? NAN : r;
    }
    int local = 0;
    for (int v = lane; v < n_views; v += 64) {
        const bool keep = vals[v] > thr;
        mask[size_t(lm) * n_views + v] = keep;
        local += keep;
    }
    for (int s = 32; s >= 1; s >>= 1) local += __shfl_xor(local, s);
    if (lane == 0) count[lm] = local;
}

__global__ __launch_bounds__(64) void solve_kernel(const double* __restrict__ starts, const double* __restrict__ ends,
                                                   const uint8_t* __restrict__ mask, const int* __restrict__ count,
                                                   const int* __restrict__ draws, int n_views,
                                                   double* __restrict__ out, double* __restrict__ err) {
    __shared__ int sel[MAX_VIEWS];
    __shared__ uint8_t inl[MAX_VIEWS];
    const int lm = blockIdx.x, lane = threadIdx.x;
    const double* S = starts + size_t(lm) * n_views * 3;
    const double* E = ends + size_t(lm) * n_views * 3;
    // compact the surviving views in view order (pa[idx], estimator3d.py:145-146)
    int k = 0;
    for (int base = 0; base < n_views; base += 64) {
        const int v = base + lane;
        const bool keep = v < n_views && mask[size_t(lm) * n_views + v];
        const unsigned long long bal = __ballot(keep);
        if (keep) sel[k + __popcll(bal & ((1ull << lane) - 1))] = v;
        k += __popcll(bal);
    }
    __syncthreads();
    (void)count;
    double p[3];
    double e_out = 0.0;
    if (k < 3) {
        // "Not enough points": plain least squares over what is left (estimator3d.py:174-176)
        double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = lane; i < k; i += 64) lsq_accum(load_line(S, E, sel[i]), acc);
        lsq_solve(acc, p);
    } else {
        // one draw of 8 lines with replacement (estimator3d.py:105-107)
        double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (lane < 8) {
            int d = draws[lm * 8 + lane];
            d = d < 0 ? 0 : (d > k - 1 ? k - 1 : d);
            lsq_accum(load_line(S, E, sel[d]), acc);
        }
        lsq_solve(acc, p);
        // inliers among all surviving lines (:109-113)
        int n_in = 0;
        for (int i = lane; i < k; i += 64) {
            const bool in = sq_dist(load_line(S, E, sel[i]), p) < 100.0;
            inl[i] = in;
            n_in += in;
        }
        for (int s = 32; s >= 1; s >>= 1) n_in += __shfl_xor(n_in, s);
        __syncthreads();
        double best_error = 100000000.0;
        bool used = false;
        if (double(n_in) > double(k) / 3.0) {
            for (int z = 0; z < 9; ++z) acc[z] = 0.0;
            for (int i = lane; i < k; i += 64)
                if (inl[i]) lsq_accum(load_line(S, E, sel[i]), acc);
            lsq_solve(acc, p);
            double dsum = 0.0;
            for (int i = lane; i < k; i += 64)
                if (inl[i]) dsum += sq_dist(load_line(S, E, sel[i]), p);
            dsum = wave_sum(dsum);
            const double sum_squared = dsum / double(n_in);
            if (sum_squared < best_error) {
                best_error = sum_squared;
                used = true;
            }
        }
        if (!used) {
            // "Ransac failed - estimating from all lines"; the error stays 1e8 (:131-133)
            for (int z = 0; z < 9; ++z) acc[z] = 0.0;
            for (int i = lane; i < k; i += 64) lsq_accum(load_line(S, E, sel[i]), acc);
            lsq_solve(acc, p);
        }
        e_out = best_error;
    }
    if (lane == 0) {
        out[lm * 3 + 0] = p[0];
        out[lm * 3 + 1] = p[1];
        out[lm * 3 + 2] = p[2];
        err[lm] = e_out;
    }
}

}  // namespace

extern "C" int mvlm_estimate_lines(mvlm_ctx* ctx, const float* maxima_dev, const double* rot_dev, int n_views,
                                   int n_landmarks, int image_size, double* starts_dev, double* ends_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, maxima_dev && rot_dev && starts_dev && ends_dev, "estimate_lines: null pointer");
    MVLM_REQUIRE(ctx, n_views > 0 && n_landmarks > 0 && image_size > 0, "estimate_lines: empty problem");
    const int total = n_views * n_landmarks;
    hipLaunchKernelGGL(lines_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, maxima_dev, rot_dev, n_views,
                       n_landmarks, float(image_size), starts_dev, ends_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

extern "C" int mvlm_consensus_mask(mvlm_ctx* ctx, const float* maxima_dev, int n_views, int n_landmarks, int mode,
                                   double q, double thr, uint8_t* mask_dev, int32_t* count_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, maxima_dev && mask_dev && count_dev, "consensus_mask: null pointer");
    MVLM_REQUIRE(ctx, n_views > 0 && n_views <= MAX_VIEWS && n_landmarks > 0, "consensus_mask: 1..1024 views supported");
    MVLM_REQUIRE(ctx, mode == MVLM_MODE_QUANTILE || mode == MVLM_MODE_ABSOLUTE,
                 "Unknown mode for line matching in Estimator");
    MVLM_REQUIRE(ctx, mode != MVLM_MODE_QUANTILE || (q >= 0.0 && q <= 1.0), "Quantiles must be in the range [0, 1]");
    hipLaunchKernelGGL(mask_kernel, dim3(n_landmarks), dim3(64), 0, ctx->stream, maxima_dev, n_views, mode, float(q),
                       float(thr), mask_dev, count_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

extern "C" int mvlm_consensus_solve(mvlm_ctx* ctx, const double* starts_dev, const double* ends_dev,
                                    const uint8_t* mask_dev, const int32_t* count_dev, const int32_t* draws_dev,
                                    int n_views, int n_landmarks, double* out_dev, double* err_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, starts_dev && ends_dev && mask_dev && draws_dev && out_dev && err_dev,
                 "consensus_solve: null pointer");
    MVLM_REQUIRE(ctx, n_views > 0 && n_views <= MAX_VIEWS && n_landmarks > 0, "consensus_solve: 1..1024 views supported");
    hipLaunchKernelGGL(solve_kernel, dim3(n_landmarks), dim3(64), 0, ctx->stream, starts_dev, ends_dev, mask_dev,
                       count_dev, draws_dev, n_views, out_dev, err_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}
