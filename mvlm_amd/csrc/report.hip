// Per-landmark quality report of the consensus: what solve_kernel (fusion.hip) decides for a landmark and drops - which views
// survived the filter, which lines the one-shot draw took, which were its inliers, which branch of
// compute_intersection_between_lines_ransac (src/mvlm/utils/estimator3d.py:92-137, :174-176) produced the point - plus how
// far every view's ray passes from the point and the covariance that spread implies.  One wavefront per landmark repeats the
// solve with the device functions of consensus_math.h in solve_kernel's order, so its point and error are solve_kernel's,
// bit for bit (the build uses -ffp-contract=off); nothing the pipeline returns is computed here.
#include "common.h"
#include "consensus_math.h"

namespace {

// stats f64[NL][MVLM_REPORT_STATS]: rms, max_dist, sigma2, cov xx yy zz xy xz yz; counts i32[NL][4]: k, n_inliers, n_used, branch
__global__ __launch_bounds__(64) void report_kernel(const double* __restrict__ starts, const double* __restrict__ ends,
                                                    const uint8_t* __restrict__ mask, const int* __restrict__ draws,
                                                    int n_views, double* __restrict__ out, double* __restrict__ err,
                                                    double* __restrict__ stats, int* __restrict__ counts,
                                                    double* __restrict__ dist2, uint8_t* __restrict__ flags) {
    __shared__ int sel[MAX_VIEWS];
    __shared__ uint8_t inl[MAX_VIEWS];
    __shared__ uint8_t drawn[MAX_VIEWS];  // by position in sel, like inl
    __shared__ uint8_t fl[MAX_VIEWS];     // by view
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
    for (int v = lane; v < n_views; v += 64) {
        inl[v] = 0;
        drawn[v] = 0;
        fl[v] = 0;
    }
    __syncthreads();
    double p[3];
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // after the last lsq_solve: the final fit's sums (acc[0..5] = -A)
    double e_out = 0.0;
    int branch = 0, n_in = 0, n_used = k;
    if (k < 3) {
        // "Not enough points": plain least squares over what is left (estimator3d.py:174-176)
        for (int i = lane; i < k; i += 64) lsq_accum(load_line(S, E, sel[i]), acc);
        lsq_solve(acc, p);
    } else {
        // one draw of 8 lines with replacement (estimator3d.py:105-107)
        if (lane < 8) {
            int d = draws[lm * 8 + lane];
            d = d < 0 ? 0 : (d > k - 1 ? k - 1 : d);
            lsq_accum(load_line(S, E, sel[d]), acc);
            drawn[d] = 1;  // (lanes that drew the same line write the same value)
        }
        lsq_solve(acc, p);
        // inliers among all surviving lines (:109-113)
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
        branch = used ? 1 : 2;
        n_used = used ? n_in : k;
    }
    // ---- the report: nothing below feeds back into p or e_out ----
    for (int i = lane; i < k; i += 64) {
        const bool in_fit = branch == 1 ? inl[i] != 0 : true;
        fl[sel[i]] = uint8_t(1 | (drawn[i] << 1) | (inl[i] << 2) | (in_fit ? 8 : 0));
    }
    __syncthreads();
    // every view's squared distance to the final point (estimator3d.py:109-111), survivors or not
    double dsum = 0.0, dmax = 0.0;
    for (int v = lane; v < n_views; v += 64) {
        const double d2 = sq_dist(load_line(S, E, v), p);
        const uint8_t f = fl[v];
        dist2[size_t(lm) * n_views + v] = d2;
        flags[size_t(lm) * n_views + v] = f;
        if (f & 8) {
            dsum += d2;
            dmax = d2 > dmax || d2 != d2 ? d2 : dmax;  // (a NaN distance stays visible)
        }
    }
    dsum = wave_sum(dsum);
    for (int s = 32; s >= 1; s >>= 1) {
        const double o = __shfl_xor(dmax, s);
        dmax = o > dmax || o != o ? o : dmax;
    }
    // cov = sigma2 * pinv(A), A = sum over the used lines of (I - n n^T) = -(acc[0..5]); the columns of pinv(A) are the
    // existing Jacobi pinv applied to the unit vectors
    // (all 64 lanes run the three pseudo-inverses, as they run lsq_solve's, and lane 0 stores: the wavefront's lanes go in
    //  lockstep, so a guard on the lane would idle 63 of them for the same time)
    const double a6[6] = {-acc[0], -acc[1], -acc[2], -acc[3], -acc[4], -acc[5]};
    double col[3][3];
    for (int j = 0; j < 3; ++j) {
        const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        pinv3_apply(a6, e, col[j]);
    }
    if (lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        out[lm * 3 + 0] = p[0];
        out[lm * 3 + 1] = p[1];
        out[lm * 3 + 2] = p[2];
        err[lm] = e_out;
        counts[lm * 4 + 0] = k;
        counts[lm * 4 + 1] = n_in;
        counts[lm * 4 + 2] = n_used;
        counts[lm * 4 + 3] = branch;
        const double sigma2 = 2 * n_used > 3 ? dsum / double(2 * n_used - 3) : nan;
        double* st = stats + size_t(lm) * MVLM_REPORT_STATS;
        st[0] = n_used > 0 ? sqrt(dsum / double(n_used)) : nan;
        st[1] = n_used > 0 ? sqrt(dmax) : nan;
        st[2] = sigma2;
        st[3] = sigma2 * col[0][0];
        st[4] = sigma2 * col[1][1];
        st[5] = sigma2 * col[2][2];
        st[6] = sigma2 * col[0][1];
        st[7] = sigma2 * col[0][2];
        st[8] = sigma2 * col[1][2];
    }
}

}  // namespace

extern "C" int mvlm_consensus_report(mvlm_ctx* ctx, const double* starts_dev, const double* ends_dev, const uint8_t* mask_dev,
                                     const int32_t* draws_dev, int n_views, int n_landmarks, double* out_dev, double* err_dev,
                                     double* stats_dev, int32_t* counts_dev, double* dist2_dev, uint8_t* flags_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, starts_dev && ends_dev && mask_dev && draws_dev && out_dev && err_dev && stats_dev && counts_dev &&
                          dist2_dev && flags_dev,
                 "consensus_report: null pointer");
    MVLM_REQUIRE(ctx, n_views > 0 && n_views <= MAX_VIEWS && n_landmarks > 0, "consensus_report: 1..1024 views supported");
    hipLaunchKernelGGL(report_kernel, dim3(n_landmarks), dim3(64), 0, ctx->stream, starts_dev, ends_dev, mask_dev, draws_dev,
                       n_views, out_dev, err_dev, stats_dev, counts_dev, dist2_dev, flags_dev);
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}
