// The direct tiles' K loop (conv_kernel.h lists the headers of the convolution kernel): the register state of a staged
// chunk, the staging items and compute_chunk.  Every `class C` below is a Cfg<> (conv_cfg.h).
#ifndef MVLM_CONV_LOOP_H
#define MVLM_CONV_LOOP_H
#include <type_traits>

#include "common.h"
#include "conv_cfg.h"

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

namespace {

constexpr unsigned INVALID_OFF = 0xFFFFFFFFu;

// compile-time loop: the body sees its index as a constant, so register arrays indexed by it
// can never be demoted to scratch by an unrolling heuristic
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// ---- pieces of the main loop, as force-inlined functions over register arrays -----------
// One "item" is one staged element per thread: items [0, X_ITERS) are input-tile floats,
// items [X_ITERS, X_ITERS + W_ITERS) are float4s of the weight slice.
template <class C>
struct StageRegs {
    float xv[C::X_ITERS];
    float xv2[C::X_ITERS];  // IN2 kernels only: the low-resolution tensor's value of the same element
    f32x4 wv[C::W_ITERS];
    float bn_s[C::X_ITERS], bn_t[C::X_ITERS];
};

// 4-row strip (TAIL4): lane l supplies the weight of channel 32 MT + 16 + (l & 3) (A row of every 4x4 block) and the
// input of ITS pixel (B column l & 3 of block l >> 2); accumulator register v = channel 32 MT + 16 + v at the lane's pixel
struct Strip4 {
    int woff4 = 0, pixoff4 = 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
};

// Split-K tiles: what a lane keeps from the start of the kernel for its share of the epilogue (see conv_mfma_kernel)
struct SplitKTail {
    bool ok = false;
    unsigned b = 0, pix = 0;
    int y = 0, x = 0;
    float res[4] = {0.f, 0.f, 0.f, 0.f};
};
template <int N>
struct SplitKTails {
    SplitKTail t[N];
};

// Issue the global load of item T for K-chunk cb.  Loads are unconditional (out-of-tile /
// padding elements read element 0 and are zeroed at write time): a branch around a load makes
// the compiler wait for each one separately.
template <class C, int T, bool BN_FROM_GLOBAL = false, bool IN2 = false>
__device__ __forceinline__ void issue_item(const ConvArgs& a, int cb, int tid, unsigned HWin, const float* sbn,
                                           const unsigned (&goff)[C::X_ITERS], const unsigned (&woff_g)[C::W_ITERS],
                                           StageRegs<C>& r, float* st_dst, const unsigned (&goff2)[C::X_ITERS]) {
    if constexpr (T < C::X_ITERS) {
        const int c = cb + (tid + T * 256) / C::PLANE;
        const bool ok = goff[T] != INVALID_OFF && c < a.cin;
        // wave-uniform base; one unconditional load per lane (masked lanes read a valid element)
        const float* const base = a.in + size_t(cb < a.cin ? cb : 0) * HWin;
        r.xv[T] = base[ok ? goff[T] : 0u];
        if constexpr (IN2) {  // the same element of the half-resolution tensor (four staged elements share one: L1 / L2 hits)
            const float* const base2 = a.in2 + size_t(cb < a.cin ? cb : 0) * (HWin >> 2);
            r.xv2[T] = base2[ok ? goff2[T] : 0u];
        }
        if (a.pre_scale != nullptr) {  // this element's BatchNorm scale / shift from the LDS copy
            const int cc = c < a.cin_pad ? c : 0;
            if constexpr (BN_FROM_GLOBAL) {  // first chunk: the LDS copy is still being filled
                r.bn_s[T] = a.pre_scale[cc];
                r.bn_t[T] = a.pre_shift[cc];
            } else {
                r.bn_s[T] = sbn[cc];
                r.bn_t[T] = sbn[C::BN_MAXC + cc];
            }
        }
    } else {
        constexpr int I = T - C::X_ITERS;
        const float* const base = a.w + size_t(cb) * a.cout_pad;  // wave-uniform
        r.wv[I] = *reinterpret_cast<const f32x4*>(base + (woff_g[I] != INVALID_OFF ? woff_g[I] : 0u));
    }
}

// BatchNorm + ReLU (pre-activation block), zero padding AFTER the activation, then the LDS write
template <class C, int T, bool IN2 = false>
__device__ __forceinline__ void write_item(const ConvArgs& a, int cb, int tid, float* st,
                                           const unsigned (&goff)[C::X_ITERS], const StageRegs<C>& r) {
    if constexpr (T < C::X_ITERS) {
        const int e = tid + T * 256;
        const int c = cb + e / C::PLANE;
        const bool ok = goff[T] != INVALID_OFF && c < a.cin;
        float v = r.xv[T];
        if constexpr (IN2) v += r.xv2[T];  // skip + upsampled low: the sum the scatter form leaves in the skip tensor, bit for bit
        if (a.pre_scale != nullptr) v = fmaxf(fmaf(v, r.bn_s[T], r.bn_t[T]), 0.f);
        v = ok ? v : 0.f;
        if (e < C::XT) st[e] = v;
    } else {
        constexpr int I = T - C::X_ITERS;
        const int f = tid + I * 256;
        if (f < C::WT / 4) reinterpret_cast<f32x4*>(st + C::XT_PAD)[f] = r.wv[I];
    }
}

// The MFMAs of one K-chunk out of LDS stage `st`.  Operands of k-step s+1 are fetched from LDS
// while the MFMAs of step s issue.  With STAGE_NEXT the staging of the next chunk (cb_next) is
// spread over the k-steps so its address arithmetic, loads, BatchNorm and LDS writes run in the
// shadow of the 64-cycle MFMAs: loads are issued during the first half of the steps, written to
// the other stage `st_next` half a chunk (~9k cycles) later.
// TR: the accumulators hold the TRANSPOSED tile (rows = pixels, columns = output channels): the operands of
// every MFMA are swapped, nothing else changes.  The fused-argmax launches use it: a lane then owns ONE output
// channel and 16 pixels per tile, so the per-channel maximum is a chain of in-register compares.
template <class C, bool STAGE_NEXT, bool TR = false, bool IN2 = false>
__device__ __forceinline__ void compute_chunk(const ConvArgs& a, const float* st, float* st_next, int cb_next, int tid,
                                              unsigned HWin, const float* sbn, int woff, const int (&pixoff)[C::NT],
                                              const unsigned (&goff)[C::X_ITERS], const unsigned (&woff_g)[C::W_ITERS],
                                              StageRegs<C>& r, f32x16 (&acc)[C::MT][C::NT], int woff16,
                                              const int (&pixoff16)[C::NT16], f32x4 (&acc16)[C::NT16], Strip4& s4,
                                              const unsigned (&goff2)[C::X_ITERS]) {
    constexpr int T_TOT = C::X_ITERS + C::W_ITERS;
    // staging schedule of the next chunk: loads issued over the first ISSUE_SPAN k-steps, LDS writes over the last WRITE_SPAN
#if !defined(MVLM_STAGE_ISSUE_DIV)
#define MVLM_STAGE_ISSUE_DIV 2
#endif
#if !defined(MVLM_STAGE_WRITE_DIV)
#define MVLM_STAGE_WRITE_DIV 2
#endif
    constexpr int ISSUE_SPAN = C::KSTEPS / MVLM_STAGE_ISSUE_DIV > 0 ? C::KSTEPS / MVLM_STAGE_ISSUE_DIV : 1;
    constexpr int WRITE_SPAN = C::KSTEPS / MVLM_STAGE_WRITE_DIV > 0 ? C::KSTEPS / MVLM_STAGE_WRITE_DIV : 1;
    constexpr int WRITE_START = C::KSTEPS - WRITE_SPAN;
    float av[2][C::MT], bv[2][C::NT];
    float a16 = 0.f, b16[C::NT16];  // 16-row strip: operands of one tap's four channels (two k-steps)
    float a4[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, b4[2][2] = {{0.f, 0.f}, {0.f, 0.f}};  // 4-row strip: [k-step parity][channel of the pair]
    if constexpr (C::TAIL4) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            a4[0][c] = st[s4.woff4 + c * C::COUT_T];
            b4[0][c] = st[s4.pixoff4 + c * C::PLANE];
        }
    }
#pragma unroll
    for (int m = 0; m < C::MT; ++m) av[0][m] = st[woff + m * 32];
#pragma unroll
    for (int n = 0; n < C::NT; ++n) bv[0][n] = st[pixoff[n]];
    static_for<0, C::KSTEPS>([&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;
        constexpr int nx = ks + 1;
        if constexpr (nx < C::KSTEPS) {
            constexpr int tap = nx / (C::CKW / 2), cp = nx % (C::CKW / 2);
            constexpr int toff = (tap / C::KS) * C::PW + (tap % C::KS);
#pragma unroll
            for (int m = 0; m < C::MT; ++m) av[nx & 1][m] = st[woff + (tap * C::CK + 2 * cp) * C::COUT_T + m * 32];
#pragma unroll
            for (int n = 0; n < C::NT; ++n) bv[nx & 1][n] = st[2 * cp * C::PLANE + pixoff[n] + toff];
        }
        if constexpr (C::TAIL4 && nx < C::KSTEPS) {
            constexpr int tap4 = nx / (C::CKW / 2), cp4 = nx % (C::CKW / 2);
            constexpr int toff4 = (tap4 / C::KS) * C::PW + (tap4 % C::KS);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                a4[nx & 1][c] = st[s4.woff4 + (tap4 * C::CK + 2 * cp4 + c) * C::COUT_T];
                b4[nx & 1][c] = st[s4.pixoff4 + (2 * cp4 + c) * C::PLANE + toff4];
            }
        }
        if constexpr (C::TAIL16 && (ks & 1) == 0) {
            // the strip's A (16 channels x 4 k) and B (4 k x 16 pixels) fragments of this tap, used
            // by the 16x16x4 MFMAs of the tap's second k-step
            constexpr int tap16 = ks / 2;
            constexpr int toff16 = (tap16 / C::KS) * C::PW + (tap16 % C::KS);
            a16 = st[woff16 + tap16 * C::CK * C::COUT_T];
#pragma unroll
            for (int j = 0; j < C::NT16; ++j) b16[j] = st[pixoff16[j] + toff16];
        }
        // two MFMAs first, then this step's share of the staging work, then the rest: the side
        // work's LDS / VMEM operations complete in the shadow of the remaining MFMAs instead of
        // being waited for at the next step's lgkmcnt(0)
#if !defined(MVLM_MFMA_LEAD)
#define MVLM_MFMA_LEAD 2
#endif
        constexpr int LEAD = (C::MT * C::NT >= 4) ? (MVLM_MFMA_LEAD < C::MT * C::NT ? MVLM_MFMA_LEAD : C::MT * C::NT) : 1;
        static_for<0, C::MT * C::NT>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int m = i / C::NT, n = i % C::NT;
            if constexpr (i < LEAD)
                acc[m][n] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(bv[ks & 1][n], av[ks & 1][m], acc[m][n], 0, 0, 0)
                               : __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks & 1][m], bv[ks & 1][n], acc[m][n], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STAGE_NEXT) {
            static_for<0, T_TOT>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
#if !defined(MVLM_ABLATE_NO_LOADS)
                if constexpr ((t * ISSUE_SPAN) / T_TOT == ks) issue_item<C, t, false, IN2>(a, cb_next, tid, HWin, sbn, goff, woff_g, r, st_next, goff2);
#endif
#if !defined(MVLM_ABLATE_NO_WRITES)
                if constexpr (WRITE_START + (t * WRITE_SPAN) / T_TOT == ks) write_item<C, t, IN2>(a, cb_next, tid, st_next, goff, r);
#endif
            });
            __builtin_amdgcn_sched_barrier(0);
        }
        // two waves share a SIMD (two workgroups per CU): the one inside its MFMA run keeps the pipe
        __builtin_amdgcn_s_setprio(1);
        static_for<0, C::MT * C::NT>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int m = i / C::NT, n = i % C::NT;
            if constexpr (i >= LEAD)
                acc[m][n] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(bv[ks & 1][n], av[ks & 1][m], acc[m][n], 0, 0, 0)
                               : __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks & 1][m], bv[ks & 1][n], acc[m][n], 0, 0, 0);
        });
        if constexpr (C::TAIL16 && (ks & 1) == 1) {
#pragma unroll
            for (int j = 0; j < C::NT16; ++j)
                acc16[j] = TR ? __builtin_amdgcn_mfma_f32_16x16x4f32(b16[j], a16, acc16[j], 0, 0, 0)
                              : __builtin_amdgcn_mfma_f32_16x16x4f32(a16, b16[j], acc16[j], 0, 0, 0);
        }
        if constexpr (C::TAIL4) {
            // (the strip has one form: with TR the 32-row and 16-row tiles are transposed around it, register v of the
            //  strip stays channel 32 MT + 16 + v at the lane's pixel)
#pragma unroll
            for (int c = 0; c < 2; ++c) s4.acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4[ks & 1][c], b4[ks & 1][c], s4.acc, 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        // keep each step's LDS prefetch and side work inside its own MFMA shadow
        __builtin_amdgcn_sched_barrier(0);
    });
}

}  // namespace
#endif
