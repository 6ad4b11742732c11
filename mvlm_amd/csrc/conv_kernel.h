// Kernel template of the implicit-GEMM convolution (see conv_mfma.hip for the overview); included by
// the translation units that instantiate groups of variants (conv_inst_g*.hip).
#ifndef MVLM_CONV_KERNEL_H
#define MVLM_CONV_KERNEL_H
#include <cstdlib>
#include <string>
#include <type_traits>

#include "common.h"

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

// COUT_T x (TW x TRI x NIMG) output tile, KS x KS taps, CK input channels per LDS stage
// (PIX_T == 64, round 4: TWO 32-pixel columns per workgroup on one staged weight slice - a launch of the small levels is
//  bound by staging 36 bytes of weights per input channel and output row for 32 pixels of matrix work; a second column
//  halves that traffic per MFMA.  These tiles have no K-parts form and no fused argmax.)
// SPLITK: the four waves of a workgroup share ONE 32x32 output tile and each sums a quarter of
// every K-chunk's channels (latency-bound tiny feature maps: 4x more workgroups, 4x shorter serial
// K loop per wave); the partial sums are added in wave order through LDS, i.e. deterministically.
// KS_ == 32 (WINO): a 3x3 convolution as F(2,3) Winograd along y.  Output rows 2p, 2p+1 come from the input rows
// d0..d3 = 2p-1 .. 2p+2 (after BatchNorm + ReLU and the zero padding): the staged planes hold, per channel and row pair,
// the four transformed rows v0 = d0 - d2, v1 = d1 + d2, v2 = d2 - d1, v3 = d1 - d3 ([cin][p][x][t]: the four values of a
// column are 16 bytes, one LDS write of the staging job and one LDS read of the lane that multiplies them), the weight slice the
// host-transformed columns u_t ([t * 3 + kx][cin][cout], 12 "taps").  Four GEMMs m_t over K = (kx, cin) - a tap is an x
// offset only - and out[2p] = (m0 + m1) + m2, out[2p+1] = (m1 - m2) - m3 in the registers of one lane: 4 MFMAs per
// output pair and (kx, cin) instead of 6, and the epilogue sees the register layout of the direct tile.
// KS_ == 34 (WINO4): a 3x3 convolution as F(4,3) Winograd along y on the points 0, 1, -1, 2, -1/2, inf.  Output rows 4q .. 4q+3
// come from the input rows d0..d5 = 4q-1 .. 4q+4: six transformed rows v_t per channel and row quad, six host-transformed weight
// columns u_t ([t * 3 + kx][cin][cout], 18 "taps"), six GEMMs m_t over K = (kx, cin) and the output transform in the registers
// of one lane - 6 MFMAs per four output rows and (kx, cin) where F(2,3) spends 8 and the direct form 12 (see "F(4,3) Winograd
// tiles" below for the transforms and the fixed order of their sums).
template <int COUT_T_, int TW_, int TRI_, int NIMG_, int KS_, int CK_, bool SPLITK_ = false>
struct Cfg {
    static constexpr bool WINO = KS_ == 32;
    static constexpr bool WINO4 = KS_ == 34;
    static constexpr int COUT_T = COUT_T_, TW = TW_, TRI = TRI_, NIMG = NIMG_, KS = (WINO || WINO4) ? 3 : KS_, CK = CK_;
    static constexpr bool SPLITK = SPLITK_;
    static constexpr int CKW = SPLITK ? CK / 4 : CK;  // channels of a chunk one wave multiplies
    static constexpr int TAPS = WINO4 ? 18 : WINO ? 12 : KS * KS;
    static constexpr int HALO = KS == 1 ? 0 : 1;  // KS == 2: a 2x2 window inside the 3x3 halo tile
    static constexpr int PW = TW + 2 * HALO;
    static constexpr int PH = WINO4 ? 6 * TRI / 4 : WINO ? 2 * TRI : TRI + 2 * HALO;  // WINO: four transformed rows per output row pair, WINO4: six per row quad
    static constexpr int PLANE = NIMG * PH * PW;  // floats per channel in sX
    static constexpr int PIX_T = TW * TRI * NIMG;
    static constexpr int XT = CK * PLANE;
    static constexpr int XT_PAD = (XT + 3) / 4 * 4;
    static constexpr int WT = TAPS * CK * COUT_T;
    static constexpr int STAGE = XT_PAD + WT;  // floats per LDS stage (two stages)
    static constexpr int MT = COUT_T / 32;  // full 32-row MFMA tiles
    // COUT_T = 32*MT + 16: the last 16 output channels run on v_mfma_f32_16x16x4_f32 (same FLOP rate,
    // half the rows), so a 73-landmark layer pads to 80 rows instead of 96
    // COUT_T = 32*MT + 16 + 4: a further 4-row strip on v_mfma_f32_4x4x1_16b_f32 (16 blocks of 4 channels x 4 pixels per
    // instruction, one k each) - 84 landmarks fit exactly instead of padding to 96
    static constexpr bool TAIL4 = COUT_T % 32 == 20;
    static constexpr bool TAIL16 = COUT_T % 32 == 16 || TAIL4;
    // the fused argmax serves the last layer only (73 / 84 landmarks -> 80 / 96-row tiles of 8x32 pixels)
    static constexpr bool HAS_AMAX = NIMG == 1 && TW == 32 && TRI == 8 && KS != 1 && (COUT_T == 80 || COUT_T == 96 || (COUT_T == 84 && KS == 2));
    static constexpr int NT = SPLITK ? PIX_T / 32 : PIX_T / 4 / 32;  // split-K: every wave multiplies all (one or two) 32-pixel columns
    static constexpr int NT16 = TAIL16 ? 2 * NT : 1;  // 16-pixel column groups of a wave
    // The epilogue's geometry, apart from the staging geometry above: a wave finishes EMT 32-row cout tiles x ENT 32-pixel columns,
    // EPIX consecutive pixels of the tile, out of ECOUT channels.  They differ on the wide F(4,3) shape only (WINO4 with 64 output
    // channels: wave w = cout half w >> 1, row quad w & 1), whose wave holds what the narrow shape's does - one quad of 32 channels.
    static constexpr bool WIDE4 = WINO4 && COUT_T == 64;
    static constexpr int EMT = WIDE4 ? 1 : MT, ENT = WIDE4 ? 4 : NT, EPIX = WIDE4 ? 128 : PIX_T / 4, ECOUT = WIDE4 ? 32 : COUT_T;
    static constexpr int KSTEPS = (WINO || WINO4) ? 3 * CK / 2 : TAPS * CKW / 2;  // WINO: (kx, channel pair), four GEMMs per step (WINO4: six)
    static constexpr int WP = PIX_T / 4 / 64;              // WINO: row pairs of a wave
    static constexpr int WJOBS = CK * (WINO4 ? TRI / 4 : TRI / 2) * PW;  // WINO: staging jobs of a chunk = (channel, row pair, x); WINO4: (channel, row quad, x)
    static constexpr int X_ITERS = (WINO || WINO4) ? (WJOBS + 255) / 256 : (XT + 255) / 256;
    static constexpr int W_ITERS = (WT / 4 + 255) / 256;
    static constexpr int BN_MAXC = 256;  // pre-BN scale/shift of up to 256 input channels live in LDS
    static constexpr size_t LDS_BYTES = size_t(2 * STAGE + 2 * BN_MAXC) * 4;
    // accumulators + staged tile + operands: above ~200 registers the kernel is told it owns
    // the whole SIMD register file (one wave per SIMD) instead of spilling for occupancy
    static constexpr int ACC_REGS = ((COUT_T / 32) * (SPLITK ? PIX_T / 32 : TW * TRI * NIMG / 128) * 16 + (TAIL16 ? 4 * NT16 : 0) + (TAIL4 ? 4 : 0)) * (WINO ? 4 : WINO4 ? 3 : 2) / 2;
    // register budget per lane: 168 at three workgroups per CU, 256 at two
    // (four per CU = 128 registers makes the 64-accumulator tiles spill; measured slower)
    static constexpr int MIN_BLOCKS_PER_CU = (ACC_REGS <= 64 && TW * TRI * NIMG <= 256) ? 3 : 2;
    // fused 2x2 max-pool in the epilogue.  POOL32: the 32-pixel-row tiles - the rows of a pair are two pixel registers of a
    // lane, the columns two neighbouring lanes.  POOL_SMALL (round 5): tiles narrower than 32 pixels (and the split-K tiles) -
    // a 32-pixel MFMA column then holds 32 / TW consecutive rows of ONE image, so the row partner of lane l is lane l ^ TW and
    // the column partner lane l ^ 1; TRI even keeps the pairs inside the tile.  max is exact: the pooled tensor is bit for bit
    // what the pool kernel makes of the full-resolution one.
    static constexpr bool POOL32 = !SPLITK && TW == 32 && NIMG == 1 && (PIX_T / 4 / 32) % 2 == 0 && COUT_T % 32 == 0;
    static constexpr bool POOL_SMALL = TW < 32 && TRI % 2 == 0 && COUT_T % 32 == 0;
    static constexpr bool CAN_POOL_ANY = POOL32 || POOL_SMALL;
    // the tile that also exists with a second input tensor added on the load (ConvArgs::in2): the dominant 128 x (8 x 32) tile
    static constexpr bool HAS_IN2 = !WINO && !WINO4 && !SPLITK && COUT_T == 128 && TW == 32 && TRI == 8 && NIMG == 1 && KS == 3 && CK == 4;
    // variants that also exist as a two-problem launch (conv_pair_kernel): the tiles of the residual blocks' 3x3 convolutions
    static constexpr bool PAIRABLE = !WINO && !WINO4 && KS == 3 && COUT_T % 32 == 0 && COUT_T != 96 && !(SPLITK && PIX_T != 32);
    static_assert(SPLITK ? ((PIX_T == 32 || PIX_T == 64) && COUT_T == 32 && CK % 8 == 0) : (PIX_T % 128 == 0),
                  "pixel tile must split into 4 waves x 32-pixel MFMA columns (or be one or two columns for split-K)");
    static_assert(!TAIL4 || PIX_T == 256, "the 4-row strip gives every lane of a wave one pixel: 64 pixels per wave");
    static_assert(COUT_T % 32 == 0 || (TAIL16 && !SPLITK && CK == 4 && TW == 32 && NIMG == 1),
                  "cout tile must be a multiple of the 32-row MFMA tile (+ one 16-row strip on the 32-pixel-row tiles)");
    static_assert(CK % 2 == 0, "the f32 MFMA consumes two k values per step");
    static_assert(!WINO || (!SPLITK && TW == 32 && NIMG == 1 && PIX_T % 256 == 0 && COUT_T % 32 == 0),
                  "Winograd tiles: 32-pixel rows, one image, whole row pairs per wave, no strips");
    static_assert(!WINO4 || (!SPLITK && TW == 32 && NIMG == 1 && COUT_T % 32 == 0 && TRI % 4 == 0 && (COUT_T / 32) * (TRI / 4) == 4),
                  "F(4,3) Winograd tile: 32-pixel rows, one image, one row quad and one 32-row cout tile per wave: 32 x 16 rows or 64 x 8");
    static_assert(LDS_BYTES <= 160 * 1024, "two stages must fit the CU's 160 KiB LDS");
};

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


// ---- F(2,3) Winograd tiles (Cfg::WINO) ----------------------------------------------------------------------------------
// Staging job = one (channel, row pair, x) of a chunk: four loads (rows 2p-1 .. 2p+2), one BatchNorm pair, ONE 16-byte LDS write
// of the four transformed values into [cin][p][x][t].
// Everything a job needs that does not change from chunk to chunk is decided ONCE, before the K loop, and kept as data of
// the lane, so that the chunk body is straight-line code without a compare:
//   - a row outside the image (or a column outside it) is a zero AND-mask and a load offset of 0 (a valid element);
//   - a lane without a job of its own (544 jobs on 3 x 256 lanes) repeats the job WJOBS earlier: same loads, same values,
//     same LDS address - every lane loads and writes;
//   - a layer without pre-activation reads the neutral BatchNorm pair (1, -0) and clamps at -inf instead of 0: v * 1 + (-0)
//     and max(v, -inf) are v, bit for bit, for every finite and infinite v.  (A NaN in the input of such a layer comes out
//     of the max as -inf where the earlier loop's branch passed it on; no tensor of the network holds one.)
//     The table is filled for all cin_pad channels in either case, so the kernel needs cin_pad <= BN_MAXC also for a layer
//     without pre-BatchNorm: the routing asks it of every Winograd launch (wino_candidate, mvlm_conv_variant_serves) and the
//     launch itself refuses a wider layer;
//   - the channels a padded last chunk has beyond cin are masked by wino_mask_tail() before that one chunk is staged.
template <class C>
struct WinoStage {
    static constexpr int N = C::WINO ? C::X_ITERS : 1;
    unsigned off[N][4];  // BYTE offset of row 2p - 1 + q at the job's x from the chunk's first channel in this image (0: masked row)
    unsigned msk[N][3];  // all ones: the column and row 2p - 1 (0), rows 2p and 2p + 1 (1), row 2p + 2 (2) lie inside the image; 0: padding
    int lds[N];          // stage offset of the job's t = 0 value
    int bn[N];           // the job's channel within the chunk
    unsigned woff;  // BYTE offset of the lane's first float4 of the weight slice from the chunk's first channel row
    float xw[N][4];
    float bn_s[N], bn_t[N];
    f32x4 wv[C::W_ITERS];
    float floor;  // ReLU of the pre-activation: 0; no pre-activation: -inf
    int abase[C::MT];  // operand reads: the lane's weight of cout tile m, tap 0, channel 0 of stage 0 ...
    int bbase[2][C::CK / 2];  // ... and its pixel of transformed row 0 in stage s, channel pair cp
};

// Makes the compiler forget what it knows about a value in a vector register (no instruction).  The LDS bases above are
// kept apart this way: one register per (stage, channel pair) and every access an immediate offset from it, where the
// compiler would rather derive each address from ONE base with an addition per access.  A global load's 32-bit offset
// passes through it inside the loop, so that it reaches the load as base (scalar) + offset (vector) and is not widened
// to 64 bits ahead of the loop.
template <class T>
__device__ __forceinline__ void wino_opaque(T& v) {
    asm volatile("" : "+v"(v));
}

// Global loads of item T for the chunk that starts at channel cb (items [0, X_ITERS): jobs, then the weight float4s).
// in_cb / w_cb: wave-uniform bases of that chunk; w_step: bytes from a lane's float4 to its next (256 float4s = whole taps on).
template <class C, int T>
__device__ __forceinline__ void issue_item_wino(const char* in_cb, const char* w_cb, size_t w_step, WinoStage<C>& ws) {
    if constexpr (T < C::X_ITERS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            wino_opaque(ws.off[T][q]);
            ws.xw[T][q] = *reinterpret_cast<const float*>(in_cb + ws.off[T][q]);
        }
    } else {
        constexpr int I = T - C::X_ITERS;
        wino_opaque(ws.woff);
        ws.wv[I] = *reinterpret_cast<const f32x4*>(w_cb + I * w_step + ws.woff);
    }
}

// the BatchNorm pair of job T's channel from the LDS table ((scale, shift) interleaved: one 8-byte read)
template <class C, int T>
__device__ __forceinline__ void bn_item_wino(const float* sbn, int cb, WinoStage<C>& ws) {
    if constexpr (T < C::X_ITERS) {
        const float2 st = *reinterpret_cast<const float2*>(sbn + 2 * (cb + ws.bn[T]));
        ws.bn_s[T] = st.x;
        ws.bn_t[T] = st.y;
    }
}

// BatchNorm + ReLU, zero padding AFTER the activation, the input transform, one 16-byte LDS write into stage NEXT
template <class C, int T, int NEXT>
__device__ __forceinline__ void write_item_wino(float* smem, int tid, const WinoStage<C>& ws) {
    if constexpr (T < C::X_ITERS) {
        float d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = fmaxf(fmaf(ws.xw[T][q], ws.bn_s[T], ws.bn_t[T]), ws.floor);
            d[q] = __uint_as_float(__float_as_uint(v) & ws.msk[T][q == 0 ? 0 : q == 3 ? 2 : 1]);
        }
        *reinterpret_cast<f32x4*>(smem + NEXT * C::STAGE + ws.lds[T]) = f32x4{d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]};
    } else {
        constexpr int I = T - C::X_ITERS;
        reinterpret_cast<f32x4*>(smem + NEXT * C::STAGE + C::XT_PAD)[tid + I * 256] = ws.wv[I];
    }
}

// The MFMAs of one K-chunk out of LDS stage CUR (a compile-time constant: every LDS access is a per-lane base register plus
// an immediate offset): k-steps (kx, channel pair) in a fixed order, per step the four GEMMs t = 0..3 of every row pair of
// the wave on MT cout tiles; operands of the next step are fetched while this one's MFMAs issue.  With STAGE_NEXT the next
// chunk (first channel cb_next) is staged into the other stage in the MFMAs' shadow: loads over the first half of the
// k-steps, BatchNorm, transform and LDS writes over the second.
template <class C, int CUR, bool STAGE_NEXT>
__device__ __forceinline__ void compute_chunk_wino(float* smem, const float* sbn, const char* in_cb, const char* w_cb, size_t w_step, int cb_next, int tid,
                                                   WinoStage<C>& ws, f32x16 (&acc)[C::MT][4 * C::WP]) {
    constexpr int T_TOT = C::X_ITERS + C::W_ITERS;
    constexpr int ISSUE_SPAN = C::KSTEPS / 2 > 0 ? C::KSTEPS / 2 : 1;
    constexpr int WRITE_SPAN = ISSUE_SPAN;
    constexpr int WRITE_START = C::KSTEPS - WRITE_SPAN;
    constexpr int NQ = 4 * C::WP;
    const float* const st = smem + CUR * C::STAGE;
    float av[2][4][C::MT];
    f32x4 bv[2][C::WP];  // the four transformed rows of the lane's pixel column: one 16-byte read
#pragma unroll
    for (int m = 0; m < C::MT; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) av[0][t][m] = st[ws.abase[m] + t * 3 * C::CK * C::COUT_T];
#pragma unroll
    for (int w = 0; w < C::WP; ++w) bv[0][w] = *reinterpret_cast<const f32x4*>(smem + ws.bbase[CUR][0] + w * 4 * C::PW);
    static_for<0, C::KSTEPS>([&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;
        constexpr int nx = ks + 1;
        // ONE wait per k-step: this step's operands (requested a step ago) and the side work's LDS traffic have arrived, the
        // next step's reads go out behind it and nothing in the step waits again
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (nx < C::KSTEPS) {
            constexpr int kx = nx / (C::CK / 2), cp = nx % (C::CK / 2);
#pragma unroll
            for (int m = 0; m < C::MT; ++m)
#pragma unroll
                for (int t = 0; t < 4; ++t) av[nx & 1][t][m] = st[ws.abase[m] + ((t * 3 + kx) * C::CK + 2 * cp) * C::COUT_T];
#pragma unroll
            for (int w = 0; w < C::WP; ++w) bv[nx & 1][w] = *reinterpret_cast<const f32x4*>(smem + ws.bbase[CUR][cp] + (w * C::PW + kx) * 4);
        }
        constexpr int LEAD = 2;
        static_for<0, C::MT * NQ>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int m = i / NQ, q = i % NQ;
            if constexpr (i < LEAD) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks & 1][q & 3][m], bv[ks & 1][q >> 2][q & 3], acc[m][q], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STAGE_NEXT) {
            // ONE wait for the global loads a k-step writes to LDS: loads return in the order of their issue, so what may stay
            // in flight is what was requested after the last item written here
            if constexpr (ks >= WRITE_START) {
                constexpr int t_last = ((ks - WRITE_START + 1) * T_TOT + WRITE_SPAN - 1) / WRITE_SPAN - 1;  // last item with WRITE_START + t * WRITE_SPAN / T_TOT == ks
                static_assert(WRITE_START + (t_last * WRITE_SPAN) / T_TOT == ks && (t_last + 1 == T_TOT || WRITE_START + ((t_last + 1) * WRITE_SPAN) / T_TOT > ks));
                constexpr int later = (t_last + 1 < C::X_ITERS ? 4 * (C::X_ITERS - t_last - 1) + C::W_ITERS : T_TOT - t_last - 1);  // a job is four loads, a weight float4 one
                static_assert(later < 16);
                __builtin_amdgcn_s_waitcnt(0x0F70 | later);  // vmcnt(later)
                __builtin_amdgcn_sched_barrier(0);
            }
            static_for<0, T_TOT>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if constexpr ((t * ISSUE_SPAN) / T_TOT == ks) {
                    issue_item_wino<C, t>(in_cb, w_cb, w_step, ws);
                    bn_item_wino<C, t>(sbn, cb_next, ws);
                }
                if constexpr (WRITE_START + (t * WRITE_SPAN) / T_TOT == ks) write_item_wino<C, t, CUR ^ 1>(smem, tid, ws);
            });
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(1);
        static_for<0, C::MT * NQ>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int m = i / NQ, q = i % NQ;
            if constexpr (i >= LEAD) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks & 1][q & 3][m], bv[ks & 1][q >> 2][q & 3], acc[m][q], 0, 0, 0);
        });
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// Between the copies of the chunk body (ahead of, inside and after the steady loop): addresses derived from the LDS bases for
// one copy are not kept in registers across another
template <class C>
__device__ __forceinline__ void wino_forget_bases(WinoStage<C>& ws) {
#pragma unroll
    for (int m = 0; m < C::MT; ++m) wino_opaque(ws.abase[m]);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int cp = 0; cp < C::CK / 2; ++cp) wino_opaque(ws.bbase[s][cp]);
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) wino_opaque(ws.lds[i]);
}

// the channel of job i of lane tid within its chunk (a lane without a job repeats the job WJOBS earlier)
template <class C>
__device__ __forceinline__ int wino_job_channel(int tid, int i) {
    const int e = tid + i * 256;
    return (e < C::WJOBS ? e : e - C::WJOBS) / ((C::TRI / 2) * C::PW);
}

// The channels of a padded last chunk beyond cin: their jobs become padding (mask 0, load offset 0) - called once, before
// the one staging pass that reads the chunk starting at channel cb
template <class C>
__device__ __forceinline__ void wino_mask_tail(const ConvArgs& a, int cb, int tid, WinoStage<C>& ws) {
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) {
        const bool okc = cb + wino_job_channel<C>(tid, i) < a.cin;  // (recomputed: nothing of it stays live over the K loop)
#pragma unroll
        for (int q = 0; q < 3; ++q) ws.msk[i][q] = okc ? ws.msk[i][q] : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) ws.off[i][q] = okc ? ws.off[i][q] : 0u;
    }
}

// The whole K loop of a Winograd tile and the output transform into the direct tile's accumulator layout
// (acc[m][n]: n = output row of the wave, 32 pixels x 16 channel registers).  The chunk loop is unrolled by two, so that
// the stage a chunk reads and the stage it fills are compile-time constants; one barrier per chunk as before.  Chunk i
// multiplies out of stage i & 1 and stages chunk i + 1; the steady loop never stages the LAST chunk of the layer (the
// only one that can hold channels beyond cin), the tail below does, after wino_mask_tail().
template <class C>
__device__ __forceinline__ void wino_main(const ConvArgs& a, float* smem, const int tid, const int y0, const int x0, const int b0,
                                          const int co0, const unsigned HWin, const int woff, f32x16 (&acc)[C::MT][C::NT], long long* t_loop) {
    static_assert(!C::WINO || (C::WT / 4) % 256 == 0, "every lane owns whole float4s of the weight slice");
    static_assert(!C::WINO || 256 * C::X_ITERS - C::WJOBS <= C::WJOBS, "a lane without a job repeats an earlier job");
    static_assert(!C::WINO || C::TRI % 2 == 0, "rows 2p and 2p + 1 of a tile share one mask: a tile is whole row pairs of an image whose height is a multiple of it");
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    WinoStage<C> ws;
    constexpr int JPC = (C::TRI / 2) * C::PW;  // jobs per channel
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) {
        const int e0 = tid + i * 256;
        const int e = e0 < C::WJOBS ? e0 : e0 - C::WJOBS;
        const int c = e / JPC;
        const int rem = e - c * JPC;
        const int p = rem / C::PW;
        const int xx = rem - p * C::PW;
        const int y = y0 + 2 * p - 1, x = x0 + xx - 1;
        const bool okx = x >= 0 && x < a.W && b0 < a.B;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // (rows 2p and 2p + 1 are rows of the tile: the image's height is a multiple of the tile's)
            const bool ok = okx && y + q >= 0 && y + q < a.H;
            ws.msk[i][q == 0 ? 0 : q == 3 ? 2 : 1] = ok ? 0xFFFFFFFFu : 0u;
            ws.off[i][q] = ok ? (unsigned(c) * HWin + unsigned((y + q) * a.W + x)) * 4u : 0u;
        }
        ws.lds[i] = c * C::PLANE + (p * C::PW + xx) * 4;
        ws.bn[i] = c;
    }
    {  // float4 index f -> (tap, c, cout4), as the direct tiles' slice; 256 float4s on is the same (c, cout4) TAPS_STEP taps on
        const int row = tid / (C::COUT_T / 4);
        const int c4 = tid - row * (C::COUT_T / 4);
        const int tap = row / C::CK;
        const int c = row - tap * C::CK;
        ws.woff = unsigned((tap * a.cin_pad + c) * a.cout_pad + co0 + c4 * 4) * 4u;
    }
    constexpr int TAPS_STEP = 256 / ((C::COUT_T / 4) * C::CK);
    static_assert(!C::WINO || 256 % ((C::COUT_T / 4) * C::CK) == 0, "256 float4s of the weight slice are whole taps");
    const size_t w_step = size_t(TAPS_STEP) * a.cin_pad * a.cout_pad * 4;
    ws.floor = __int_as_float(__builtin_amdgcn_readfirstlane(a.pre_scale != nullptr ? 0 : int(0xFF800000u)));  // (a scalar)
#pragma unroll
    for (int m = 0; m < C::MT; ++m) {
        ws.abase[m] = woff + m * 32;
        wino_opaque(ws.abase[m]);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int cp = 0; cp < C::CK / 2; ++cp) {
            ws.bbase[s][cp] = s * C::STAGE + (2 * cp + half) * C::PLANE + (wave * C::WP * C::PW + l31) * 4;
            wino_opaque(ws.bbase[s][cp]);
        }
    float* const sbn = smem + 2 * C::STAGE;
    // wave-uniform bases of chunk 0
    const char* const in0 = reinterpret_cast<const char*>(a.in + size_t((b0 < a.B ? b0 : 0) * a.in_ctot + a.in_coff) * HWin);
    const char* const w0 = reinterpret_cast<const char*>(a.w);
    constexpr int T_TOT = C::X_ITERS + C::W_ITERS;
    const int last = a.cin_pad - C::CK;  // first channel of the last chunk
    const bool odd = (a.cin_pad / C::CK) & 1;
    // prologue: chunk 0's loads, the BatchNorm table and the first barrier are one memory round trip.  The LAST chunk is
    // multiplied out of stage 1, the one before out of stage 0 and so on: chunk 0 goes to stage 1 where the count is odd.
    if (last == 0) wino_mask_tail<C>(a, 0, tid, ws);
    static_for<0, T_TOT>([&](auto tc) { issue_item_wino<C, decltype(tc)::value>(in0, w0, w_step, ws); });
    // (all cin_pad channels, with or without pre-BatchNorm: 2 * cin_pad <= 2 * BN_MAXC floats, see the note at WinoStage)
    for (int i = tid; i < a.cin_pad; i += 256) {
        sbn[2 * i] = a.pre_scale != nullptr ? a.pre_scale[i] : 1.f;
        sbn[2 * i + 1] = a.pre_scale != nullptr ? a.pre_shift[i] : -0.f;
    }
    __syncthreads();
    static_for<0, T_TOT>([&](auto tc) { bn_item_wino<C, decltype(tc)::value>(sbn, 0, ws); });
    if (odd) {
        static_for<0, T_TOT>([&](auto tc) { write_item_wino<C, decltype(tc)::value, 1>(smem, tid, ws); });
    } else {
        static_for<0, T_TOT>([&](auto tc) { write_item_wino<C, decltype(tc)::value, 0>(smem, tid, ws); });
    }
    __syncthreads();
#if defined(MVLM_CONV_TIMING)
    *t_loop = clock64();
#endif
    f32x16 wacc[C::MT][4 * C::WP];
#pragma unroll
    for (int m = 0; m < C::MT; ++m)
#pragma unroll
        for (int q = 0; q < 4 * C::WP; ++q) wacc[m][q] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (last > 0) {
        int cb = 0;  // the chunk to multiply next
        // wave-uniform bases of the chunk to stage next, moved on by one chunk after every staging pass
        const size_t in_step = size_t(C::CK) * HWin * 4, w_cstep = size_t(C::CK) * a.cout_pad * 4;
        const char* in_nx = in0 + in_step;
        const char* w_nx = w0 + w_cstep;
        if (odd) {  // (three chunks or more: chunk 1 is not the last)
            compute_chunk_wino<C, 1, true>(smem, sbn, in_nx, w_nx, w_step, C::CK, tid, ws, wacc);
            __syncthreads();  // next stage complete; everybody is done reading this one
            cb = C::CK, in_nx += in_step, w_nx += w_cstep;
        }
        wino_forget_bases<C>(ws);
        // an even number of chunks is left: two per iteration while there are more than two
        for (; cb + C::CK < last; cb += 2 * C::CK) {
            compute_chunk_wino<C, 0, true>(smem, sbn, in_nx, w_nx, w_step, cb + C::CK, tid, ws, wacc);
            __syncthreads();
            in_nx += in_step, w_nx += w_cstep;
            compute_chunk_wino<C, 1, true>(smem, sbn, in_nx, w_nx, w_step, cb + 2 * C::CK, tid, ws, wacc);
            __syncthreads();
            in_nx += in_step, w_nx += w_cstep;
        }
        wino_forget_bases<C>(ws);
        wino_mask_tail<C>(a, last, tid, ws);
        compute_chunk_wino<C, 0, true>(smem, sbn, in_nx, w_nx, w_step, last, tid, ws, wacc);
        __syncthreads();
    }
    compute_chunk_wino<C, 1, false>(smem, sbn, nullptr, nullptr, 0, 0, tid, ws, wacc);
    static_for<0, C::MT>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        static_for<0, C::WP>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m0 = wacc[m][4 * p][r], m1 = wacc[m][4 * p + 1][r], m2 = wacc[m][4 * p + 2][r], m3 = wacc[m][4 * p + 3][r];
                acc[m][2 * p][r] = (m0 + m1) + m2;
                acc[m][2 * p + 1][r] = (m1 - m2) - m3;
            }
        });
    });
    (void)t_loop;
}

// ---- F(4,3) Winograd tiles (Cfg::WINO4) ---------------------------------------------------------------------------------
// The tile of conv3x3_c32_t16x32 (32 cout x 16 rows x 32 pixels, one row quad per wave) with the structure of the F(2,3)
// tiles above.  Quad q covers output rows 4q .. 4q+3 and reads d0..d5 = rows 4q-1 .. 4q+4 (after BatchNorm + ReLU and the
// zero padding).  All coefficients are dyadic, so every product is exact and only the sums round; they are summed left to
// right as written, each step one fused multiply-add (= the exact product, added with one rounding):
//   v0 = d0 + 1.5 d1 - 2 d2 - 1.5 d3 + d4      v1 = -d1 - 2.5 d2 - 0.5 d3 + d4      v2 = d1 + 0.5 d2 - 2.5 d3 + d4
//   v3 = -d2 - 0.5 d1 + 0.5 d3 + d4            v4 = -d2 + 2 d1 - 2 d3 + d4          v5 = d1 + 1.5 d2 - 2 d3 - 1.5 d4 + d5
// weights (host, float64, rounded once: mvlm_winograd4_transform):
//   u0 = g0, u1 = -(g0 + g1 + g2) / 3, u2 = (g0 - g1 + g2) / 3, u3 = (g0 + 2 g1 + 4 g2) / 15, u4 = (-16 g0 + 8 g1 - 4 g2) / 15, u5 = g2
// six GEMMs m_t = sum over (kx, cin) of u_t v_t, and with s = m1 + m2, d = m1 - m2:
//   o0 = (m0 + s) + (m3 + m4)    o1 = d + (2 m3 - m4 / 2)    o2 = s + (4 m3 + m4 / 4)    o3 = (d + (8 m3 - m4 / 8)) + m5
// A channel's plane of a stage is [q][x][4] (v0..v3, one 16-byte write and read) followed by [q][x][2] (v4, v5, 8 bytes):
// neighbouring lanes read neighbouring 16- / 8-byte words.  The weight slice is [t * 3 + kx][cin][cout] as in global memory.
// The wide shape (Cfg::WIDE4: 64 cout x 8 rows x 32 pixels) runs the same program with wave w = (cout half w >> 1, row quad w & 1): two
// waves read the same staged quad against the two 32-channel halves of a 64-channel weight slice, so a staging job serves twice the MFMAs.
// Staging job = one (channel, row quad, x) of a chunk: six loads, one BatchNorm pair, two LDS writes.  Masks, repeated jobs,
// the neutral BatchNorm pair and the padded last chunk are handled as for the F(2,3) tiles (see WinoStage).
template <class C>
struct Wino4Stage {
    static constexpr int N = C::WINO4 ? C::X_ITERS : 1;
    static constexpr int NW = C::WINO4 ? C::W_ITERS : 1;
    unsigned off[N][6];  // BYTE offset of row 4q - 1 + r at the job's x from the chunk's first channel in this image (0: masked row)
    unsigned msk[N][3];  // all ones: the column and row 4q - 1 (0), rows 4q .. 4q + 3 (1), row 4q + 4 (2) lie inside the image; 0: padding
    int lds4[N], lds2[N];  // stage offsets of the job's v0 and v4
    int bn[N];             // the job's channel in the chunk that is staged next
    unsigned woff[NW];     // BYTE offset of the lane's float4 i of the weight slice from the chunk's first channel row ...
    int wlds[NW];          // ... and its float4 index in the staged slice (a lane without a float4 i repeats its float4 i - 1)
    float xw[N][6];  // the job's six rows as loaded, then (in place) after BatchNorm + ReLU and the padding mask
    float bn_s[N], bn_t[N];
    f32x4 wv[NW];
    float floor;  // ReLU of the pre-activation: 0; no pre-activation: -inf
    int abase;    // operand reads: the lane's weight of tap 0, channel 0 of stage 0 ...
    int bbase4[2][C::CK / 2], bbase2[2][C::CK / 2];  // ... and its pixel's v0 / v4 in stage s, channel pair cp
};

// Where the slices of a chunk's staging sit among its MFMAs.  A chunk is 6 * KSTEPS MFMAs; gap g is what a wave issues between
// MFMA g and MFMA g + 1 (the first gap of a k-step also holds the next k-step's operand reads, its last gap the next k-step's
// wait, the chunk's last gap the barrier).  A staging item is cut into slices of at most eight instructions, and a gap takes one
// slice of the loads and one of the writes at most, so a 64-cycle MFMA covers what is issued behind it.  An x-item (six loads,
// BatchNorm + ReLU + mask, the input transform, two LDS writes) is four issue slices (three load pairs, the BatchNorm pair's LDS
// read) and six write slices (rows 0-1 behind the item's ONE counted vmcnt, rows 2-3, rows 4-5, v0 v1, v2 v3 + the 16-byte write,
// v4 v5 + the 8-byte write); a weight float4 is one slice of either kind.  Both kinds run in the order x-item 0, its share of the
// weight float4s, x-item 1, ...: the loads from gap 0 on, one per gap outside the k-steps' last gaps, the writes one per gap so
// that the last one sits in the gap before the chunk's last MFMA.
template <class C>
struct Wino4Plan {
    static constexpr int NX = C::WINO4 ? C::X_ITERS : 1, NW = C::WINO4 ? C::W_ITERS : 1;
    static constexpr int GAPS = 6 * C::KSTEPS;
    static constexpr int XI = 4, XW = 6;  // issue / write slices of an x-item
    static constexpr int NI = XI * NX + NW, NWR = XW * NX + NW;
    static constexpr int ADVANCE = 6 * (C::KSTEPS / 2) - 1;  // the gap that steps the chunk's bases on, behind the last issue slice
    static constexpr int wfirst(int i) { return i * NW / NX; }  // the weight float4s [wfirst(i), wfirst(i + 1)) follow x-item i
    static constexpr int slices(int t, int per) { return t < NX ? per : 1; }
    static constexpr int seq(int t, int p, int per) {  // position of slice p of item t in its kind's order
        if (t < NX) return t * per + wfirst(t) + p;
        int i = 0;
        while (wfirst(i + 1) <= t - NX) ++i;
        return (i + 1) * per + (t - NX);
    }
    static constexpr int issue_gap(int t, int p) { return (seq(t, p, XI) / 5) * 6 + seq(t, p, XI) % 5; }
    static constexpr int write_gap(int t, int p) { return GAPS - 1 - NWR + seq(t, p, XW); }
    static constexpr int loads(int t, int p) { return t >= NX ? 1 : p < 3 ? 2 : 0; }
    // global loads that may still be in flight when item t's first write slice runs: those requested behind the item's own and
    // before that gap's write slice (loads return in order; a gap's issue slice precedes its write slice)
    static constexpr int later(int t) {
        int n = 0;
        for (int u = 0; u < NX + NW; ++u)
            for (int q = 0; q < slices(u, XI); ++q)
                if (seq(u, q, XI) > seq(t, slices(t, XI) - 1, XI) && issue_gap(u, q) <= write_gap(t, 0)) n += loads(u, q);
        return n;
    }
    static constexpr bool ordered() {  // every load is requested before its item's first write slice, and before the bases move
        for (int t = 0; t < NX + NW; ++t)
            if (issue_gap(t, slices(t, XI) - 1) >= write_gap(t, 0) || issue_gap(t, slices(t, XI) - 1) > ADVANCE || later(t) >= 16) return false;
        return true;
    }
};

// Issue slice P of staging item T: an x-item's rows 2P, 2P + 1 (P < 3) or its BatchNorm pair (P == 3); a weight float4
template <class C, int T, int P>
__device__ __forceinline__ void issue_slice_wino4(const char* in_cb, const char* w_cb, const float* sbn, Wino4Stage<C>& ws) {
    if constexpr (T < C::X_ITERS) {
        if constexpr (P < 3) {
#pragma unroll
            for (int r = 2 * P; r < 2 * P + 2; ++r) {
                wino_opaque(ws.off[T][r]);
                ws.xw[T][r] = *reinterpret_cast<const float*>(in_cb + ws.off[T][r]);
            }
        } else {
            const float2 st = *reinterpret_cast<const float2*>(sbn + 2 * ws.bn[T]);
            ws.bn_s[T] = st.x;
            ws.bn_t[T] = st.y;
        }
    } else {
        constexpr int I = T - C::X_ITERS;
        wino_opaque(ws.woff[I]);
        ws.wv[I] = *reinterpret_cast<const f32x4*>(w_cb + ws.woff[I]);
    }
}

template <class C, int T>
__device__ __forceinline__ void issue_item_wino4(const char* in_cb, const char* w_cb, Wino4Stage<C>& ws) {
    if constexpr (T < C::X_ITERS) {
        static_for<0, 3>([&](auto pc) { issue_slice_wino4<C, T, decltype(pc)::value>(in_cb, w_cb, nullptr, ws); });
    } else {
        issue_slice_wino4<C, T, 0>(in_cb, w_cb, nullptr, ws);
    }
}

template <class C, int T>
__device__ __forceinline__ void bn_item_wino4(const float* sbn, Wino4Stage<C>& ws) {
    if constexpr (T < C::X_ITERS) issue_slice_wino4<C, T, 3>(nullptr, nullptr, sbn, ws);
}

// Write slice P of staging item T into stage NEXT (v01: the item's v0, v1 from slice 3 to slice 4).  An x-item: BatchNorm + ReLU
// and the zero padding AFTER the activation of rows 2P, 2P + 1 (P < 3, in place), then the input transform: v0 v1 (P == 3), v2 v3
// and the 16-byte LDS write (4), v4 v5 and the 8-byte write (5).  A weight float4: its LDS write.
template <class C, int T, int P, int NEXT>
__device__ __forceinline__ void write_slice_wino4(float* smem, Wino4Stage<C>& ws, float (&v01)[2]) {
    if constexpr (T < C::X_ITERS) {
        float(&d)[6] = ws.xw[T];
        if constexpr (P < 3) {
#pragma unroll
            for (int r = 2 * P; r < 2 * P + 2; ++r) {
                const float v = fmaxf(fmaf(d[r], ws.bn_s[T], ws.bn_t[T]), ws.floor);
                d[r] = __uint_as_float(__float_as_uint(v) & ws.msk[T][r == 0 ? 0 : r == 5 ? 2 : 1]);
            }
        } else if constexpr (P == 3) {
            v01[0] = fmaf(-1.5f, d[3], fmaf(-2.f, d[2], fmaf(1.5f, d[1], d[0]))) + d[4];
            v01[1] = fmaf(-0.5f, d[3], fmaf(-2.5f, d[2], -d[1])) + d[4];
        } else if constexpr (P == 4) {
            const float v2 = fmaf(-2.5f, d[3], fmaf(0.5f, d[2], d[1])) + d[4];
            const float v3 = fmaf(0.5f, d[3], fmaf(-0.5f, d[1], -d[2])) + d[4];
            *reinterpret_cast<f32x4*>(smem + NEXT * C::STAGE + ws.lds4[T]) = f32x4{v01[0], v01[1], v2, v3};
        } else {
            const float v4 = fmaf(-2.f, d[3], fmaf(2.f, d[1], -d[2])) + d[4];
            const float v5 = fmaf(-1.5f, d[4], fmaf(-2.f, d[3], fmaf(1.5f, d[2], d[1]))) + d[5];
            *reinterpret_cast<float2*>(smem + NEXT * C::STAGE + ws.lds2[T]) = make_float2(v4, v5);
        }
    } else {
        constexpr int I = T - C::X_ITERS;
        reinterpret_cast<f32x4*>(smem + NEXT * C::STAGE + C::XT_PAD)[ws.wlds[I]] = ws.wv[I];
    }
}

template <class C, int T, int NEXT>
__device__ __forceinline__ void write_item_wino4(float* smem, Wino4Stage<C>& ws) {
    float v01[2];
    static_for<0, Wino4Plan<C>::slices(T, Wino4Plan<C>::XW)>([&](auto pc) { write_slice_wino4<C, T, decltype(pc)::value, NEXT>(smem, ws, v01); });
}

// The bases of the chunk after the one being staged: stepped inside the chunk, not in the gap that holds its barrier
template <class C>
__device__ __forceinline__ void wino4_advance(const char*& in_cb, const char*& w_cb, size_t in_step, size_t w_step, Wino4Stage<C>& ws) {
    in_cb += in_step, w_cb += w_step;
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) ws.bn[i] += C::CK;
}

// The slices of gap G while stage NEXT is being filled: the issue slice first, then the write slice, whose item waits ONCE, at
// its first slice, for its own loads (Wino4Plan::later)
template <class C, int G, int NEXT>
__device__ __forceinline__ void gap_wino4(float* smem, const float* sbn, const char*& in_cb, const char*& w_cb, size_t in_step, size_t w_step,
                                          Wino4Stage<C>& ws, float (&v01)[2]) {
    using P = Wino4Plan<C>;
    static_for<0, P::NX + P::NW>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        static_for<0, P::slices(t, P::XI)>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
            if constexpr (P::issue_gap(t, p) == G) issue_slice_wino4<C, t, p>(in_cb, w_cb, sbn, ws);
        });
    });
    static_for<0, P::NX + P::NW>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        static_for<0, P::slices(t, P::XW)>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
            if constexpr (P::write_gap(t, p) == G) {
                if constexpr (p == 0) {
                    __builtin_amdgcn_s_waitcnt(0x0F70 | P::later(t));  // vmcnt(later)
                    __builtin_amdgcn_sched_barrier(0);
                }
                write_slice_wino4<C, t, p, NEXT>(smem, ws, v01);
            }
        });
    });
    if constexpr (G == P::ADVANCE) wino4_advance<C>(in_cb, w_cb, in_step, w_step, ws);
}

// The MFMAs of one K-chunk out of LDS stage CUR, as compute_chunk_wino: k-steps (kx, channel pair) in a fixed order, per step
// the six GEMMs t = 0..5 of the wave's row quad; with STAGE_NEXT the chunk at in_cb / w_cb is staged in the MFMAs' shadow, slice by
// slice in the gaps between single MFMAs (Wino4Plan), and the bases are stepped on to the chunk after it.
template <class C, int CUR, bool STAGE_NEXT>
__device__ __forceinline__ void compute_chunk_wino4(float* smem, const float* sbn, const char*& in_cb, const char*& w_cb, size_t in_step,
                                                    size_t w_step, Wino4Stage<C>& ws, f32x16 (&acc)[6]) {
    using P = Wino4Plan<C>;
    static_assert(P::NI <= 5 * (C::KSTEPS / 2) && P::NWR <= P::GAPS - 1 && P::ordered(), "loads in the first half of the k-steps, every write behind its loads");
    const float* const st = smem + CUR * C::STAGE;
    float av[2][6];
    f32x4 bv4[2];  // v0..v3 of the lane's pixel column: one 16-byte read
    float2 bv2[2];  // v4, v5: one 8-byte read
    float v01[2];   // (one x-item at a time is between its write slices 3 and 4)
#pragma unroll
    for (int t = 0; t < 6; ++t) av[0][t] = st[ws.abase + t * 3 * C::CK * C::COUT_T];
    bv4[0] = *reinterpret_cast<const f32x4*>(smem + ws.bbase4[CUR][0]);
    bv2[0] = *reinterpret_cast<const float2*>(smem + ws.bbase2[CUR][0]);
    static_for<0, C::KSTEPS>([&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;
        constexpr int nx = ks + 1;
        // ONE wait per k-step (see compute_chunk_wino): this step's operands, and the LDS traffic of the slices behind them
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (nx < C::KSTEPS) {
            constexpr int kx = nx / (C::CK / 2), cp = nx % (C::CK / 2);
#pragma unroll
            for (int t = 0; t < 6; ++t) av[nx & 1][t] = st[ws.abase + ((t * 3 + kx) * C::CK + 2 * cp) * C::COUT_T];
            bv4[nx & 1] = *reinterpret_cast<const f32x4*>(smem + ws.bbase4[CUR][cp] + kx * 4);
            bv2[nx & 1] = *reinterpret_cast<const float2*>(smem + ws.bbase2[CUR][cp] + kx * 2);
        }
        auto bval = [&](auto tc) {
            constexpr int t = decltype(tc)::value;
            if constexpr (t < 4) return bv4[ks & 1][t];
            else if constexpr (t == 4) return bv2[ks & 1].x;
            else return bv2[ks & 1].y;
        };
        static_for<0, 6>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks & 1][t], bval(tc), acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (STAGE_NEXT) {
                gap_wino4<C, 6 * ks + t, CUR ^ 1>(smem, sbn, in_cb, w_cb, in_step, w_step, ws, v01);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
    });
}

template <class C>
__device__ __forceinline__ void wino4_forget_bases(Wino4Stage<C>& ws) {
    wino_opaque(ws.abase);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int cp = 0; cp < C::CK / 2; ++cp) {
            wino_opaque(ws.bbase4[s][cp]);
            wino_opaque(ws.bbase2[s][cp]);
        }
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) {
        wino_opaque(ws.lds4[i]);
        wino_opaque(ws.lds2[i]);
    }
}

// the channel of job i of lane tid within its chunk (a lane without a job repeats the job WJOBS earlier)
template <class C>
__device__ __forceinline__ int wino4_job_channel(int tid, int i) {
    const int e = tid + i * 256;
    return (e < C::WJOBS ? e : e - C::WJOBS) / ((C::TRI / 4) * C::PW);
}

// The channels of a padded last chunk beyond cin: their jobs become padding (mask 0, load offset 0)
template <class C>
__device__ __forceinline__ void wino4_mask_tail(const ConvArgs& a, int cb, int tid, Wino4Stage<C>& ws) {
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) {
        const bool okc = cb + wino4_job_channel<C>(tid, i) < a.cin;
#pragma unroll
        for (int q = 0; q < 3; ++q) ws.msk[i][q] = okc ? ws.msk[i][q] : 0u;
#pragma unroll
        for (int r = 0; r < 6; ++r) ws.off[i][r] = okc ? ws.off[i][r] : 0u;
    }
}

// The whole K loop of an F(4,3) tile and the output transform into the direct tile's accumulator layout (acc[0][n]: n = output
// row of the wave's quad).  The chunk schedule is wino_main's: unrolled by two, one barrier per chunk, the last chunk (the
// only one that can hold channels beyond cin) staged after wino4_mask_tail().
template <class C>
__device__ __forceinline__ void wino4_main(const ConvArgs& a, float* smem, const int tid, const int y0, const int x0, const int b0,
                                           const int co0, const unsigned HWin, const int woff, f32x16 (&acc)[C::EMT][C::ENT], long long* t_loop) {
    static_assert(!C::WINO4 || 256 * C::X_ITERS - C::WJOBS <= C::WJOBS, "a lane without a job repeats an earlier job");
    static_assert(!C::WINO4 || (C::TRI % 4 == 0 && C::ENT == 4 && C::EMT == 1), "one row quad per wave; rows 4q .. 4q + 3 of a tile share one mask");
    static_assert(!C::WINO4 || (C::WT / 4 > 256 * (C::W_ITERS - 1) && C::WT / 4 >= 256), "a lane without a float4 repeats its previous one");
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int wq = C::WIDE4 ? (wave & 1) : wave;  // the wave's row quad ...
    const int wh = C::WIDE4 ? (wave >> 1) : 0;    // ... and its 32-row half of the staged cout tile
    Wino4Stage<C> ws;
    constexpr int JPC = (C::TRI / 4) * C::PW;  // jobs per channel
    constexpr int Q4 = JPC * 4;                // floats of a channel's [q][x][4] part
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) {
        const int e0 = tid + i * 256;
        const int e = e0 < C::WJOBS ? e0 : e0 - C::WJOBS;
        const int c = e / JPC;
        const int rem = e - c * JPC;
        const int q = rem / C::PW;
        const int xx = rem - q * C::PW;
        const int y = y0 + 4 * q - 1, x = x0 + xx - 1;
        const bool okx = x >= 0 && x < a.W && b0 < a.B;
#pragma unroll
        for (int r = 0; r < 6; ++r) {  // (rows 4q .. 4q + 3 are rows of the tile: the image's height is a multiple of the tile's)
            const bool ok = okx && y + r >= 0 && y + r < a.H;
            if (r == 0 || r == 1 || r == 5) ws.msk[i][r == 0 ? 0 : r == 5 ? 2 : 1] = ok ? 0xFFFFFFFFu : 0u;
            ws.off[i][r] = ok ? (unsigned(c) * HWin + unsigned((y + r) * a.W + x)) * 4u : 0u;
        }
        ws.lds4[i] = c * C::PLANE + rem * 4;
        ws.lds2[i] = c * C::PLANE + Q4 + rem * 2;
        ws.bn[i] = c;
    }
#pragma unroll
    for (int i = 0; i < C::W_ITERS; ++i) {  // float4 index f -> (tap, c, cout4), as the direct tiles' slice
        const int f0 = tid + i * 256;
        const int f = f0 < C::WT / 4 ? f0 : f0 - 256;
        const int row = f / (C::COUT_T / 4);
        const int c4 = f - row * (C::COUT_T / 4);
        const int tap = row / C::CK;
        const int c = row - tap * C::CK;
        ws.woff[i] = unsigned((tap * a.cin_pad + c) * a.cout_pad + co0 + c4 * 4) * 4u;
        ws.wlds[i] = f;
    }
    ws.floor = __int_as_float(__builtin_amdgcn_readfirstlane(a.pre_scale != nullptr ? 0 : int(0xFF800000u)));  // (a scalar)
    ws.abase = woff + 32 * wh;
    wino_opaque(ws.abase);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int cp = 0; cp < C::CK / 2; ++cp) {
            ws.bbase4[s][cp] = s * C::STAGE + (2 * cp + half) * C::PLANE + (wq * C::PW + l31) * 4;
            ws.bbase2[s][cp] = s * C::STAGE + (2 * cp + half) * C::PLANE + Q4 + (wq * C::PW + l31) * 2;
            wino_opaque(ws.bbase4[s][cp]);
            wino_opaque(ws.bbase2[s][cp]);
        }
    float* const sbn = smem + 2 * C::STAGE;
    // wave-uniform bases of chunk 0
    const char* const in0 = reinterpret_cast<const char*>(a.in + size_t((b0 < a.B ? b0 : 0) * a.in_ctot + a.in_coff) * HWin);
    const char* const w0 = reinterpret_cast<const char*>(a.w);
    constexpr int T_TOT = C::X_ITERS + C::W_ITERS;
    const int last = a.cin_pad - C::CK;  // first channel of the last chunk
    const bool odd = (a.cin_pad / C::CK) & 1;
    // prologue as wino_main's: the LAST chunk is multiplied out of stage 1, so chunk 0 goes to stage 1 where the count is odd
    if (last == 0) wino4_mask_tail<C>(a, 0, tid, ws);
    static_for<0, T_TOT>([&](auto tc) { issue_item_wino4<C, decltype(tc)::value>(in0, w0, ws); });
    for (int i = tid; i < a.cin_pad; i += 256) {
        sbn[2 * i] = a.pre_scale != nullptr ? a.pre_scale[i] : 1.f;
        sbn[2 * i + 1] = a.pre_scale != nullptr ? a.pre_shift[i] : -0.f;
    }
    __syncthreads();
    static_for<0, T_TOT>([&](auto tc) { bn_item_wino4<C, decltype(tc)::value>(sbn, ws); });
    if (odd) {
        static_for<0, T_TOT>([&](auto tc) { write_item_wino4<C, decltype(tc)::value, 1>(smem, ws); });
    } else {
        static_for<0, T_TOT>([&](auto tc) { write_item_wino4<C, decltype(tc)::value, 0>(smem, ws); });
    }
    __syncthreads();
#if defined(MVLM_CONV_TIMING)
    *t_loop = clock64();
#endif
    f32x16 wacc[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) wacc[t] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (last > 0) {
        int cb = 0;  // the chunk to multiply next
        const size_t in_step = size_t(C::CK) * HWin * 4, w_cstep = size_t(C::CK) * a.cout_pad * 4;
        const char* in_nx = in0;  // the chunk to stage next: chunk 1 (compute_chunk_wino4 steps the bases on)
        const char* w_nx = w0;
        wino4_advance<C>(in_nx, w_nx, in_step, w_cstep, ws);
        if (odd) {  // (three chunks or more: chunk 1 is not the last)
            compute_chunk_wino4<C, 1, true>(smem, sbn, in_nx, w_nx, in_step, w_cstep, ws, wacc);
            __syncthreads();  // next stage complete; everybody is done reading this one
            cb = C::CK;
        }
        wino4_forget_bases<C>(ws);
        for (; cb + C::CK < last; cb += 2 * C::CK) {
            compute_chunk_wino4<C, 0, true>(smem, sbn, in_nx, w_nx, in_step, w_cstep, ws, wacc);
            __syncthreads();
            compute_chunk_wino4<C, 1, true>(smem, sbn, in_nx, w_nx, in_step, w_cstep, ws, wacc);
            __syncthreads();
        }
        wino4_forget_bases<C>(ws);
        wino4_mask_tail<C>(a, last, tid, ws);
        compute_chunk_wino4<C, 0, true>(smem, sbn, in_nx, w_nx, in_step, w_cstep, ws, wacc);
        __syncthreads();
    }
    const char* none = nullptr;
    compute_chunk_wino4<C, 1, false>(smem, sbn, none, none, 0, 0, ws, wacc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float m0 = wacc[0][r], m1 = wacc[1][r], m2 = wacc[2][r], m3 = wacc[3][r], m4 = wacc[4][r], m5 = wacc[5][r];
        const float s = m1 + m2, d = m1 - m2;
        acc[0][0][r] = (m0 + s) + (m3 + m4);
        acc[0][1][r] = d + fmaf(-0.5f, m4, 2.f * m3);
        acc[0][2][r] = s + fmaf(0.25f, m4, 4.f * m3);
        acc[0][3][r] = (d + fmaf(-0.125f, m4, 8.f * m3)) + m5;
    }
    (void)t_loop;
}

// Software-pipelined main loop, one workgroup (4 waves, one per SIMD) per CU-resident tile:
//   while the MFMAs of K-chunk c run out of LDS stage c&1, the global loads of chunk c+1 are
//   in flight into registers; after the MFMAs they get their BatchNorm+ReLU and are written to
//   the other stage; ONE barrier per chunk.  The kernel may use the whole 512-register file
//   (launch bounds 256,1), so nothing spills and the 128 accumulators stay in registers.
//
// conv_tile is the whole workgroup program; the kernels below only say which problem a workgroup belongs to:
// conv_mfma_kernel = one convolution per launch (block `bid` of `nblk`), conv_pair_kernel = two independent convolutions
// of the same tile configuration in one grid.
template <class C, bool AMAX, bool IN2 = false>
__device__ __forceinline__ void conv_tile(const ConvArgs& a_in, const int tiles_x, const int tiles_y, const int cout_tiles,
                                          const int bid, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    // XCD-aware tile order: consecutive block ids land on different XCDs, so give every
    // XCD a contiguous run of tiles (cout tiles of one pixel tile share its input in L2).
    int lid;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
        lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    // conv11 as four 2x2 parity convolutions in ONE launch (ConvArgs::n_par == 4): the four parities of a tile are
    // neighbouring workgroups of one XCD, so the low-resolution input tile they all stage comes out of that L2 once, and
    // a small batch gives the chip 4x the workgroups per launch.  Everything that depends on the parity is patched into
    // a private copy of the arguments (wave-uniform values); other kernels use the launch arguments as they are.
    ConvArgs a_par;
    if constexpr (C::KS == 2) {
        a_par = a_in;
        if (a_in.n_par == 4) {
            const int pl = lid & 3;
            lid >>= 2;
            a_par.sub_y = pl >> 1;
            a_par.sub_x = pl & 1;
            a_par.w = a_in.w_par[pl];
            a_par.amax_part0 = a_in.amax_part0 + pl * a_in.amax_par_stride;
        }
    }
    const ConvArgs& a = C::KS == 2 ? a_par : a_in;
    // split-K tiles may also split the input channels over `kparts` workgroups (grid = tiles x kparts, the parts of a
    // tile adjacent): each sums its channel range, the last one to finish adds the partial tiles in part order
    int kp = 0;
    if constexpr (C::SPLITK) {
        if (a.kparts > 1) {
            kp = lid % a.kparts;
            lid /= a.kparts;
        }
    }
    const int tile_id = lid;
    const int ct = lid % cout_tiles;
    const int pt = lid / cout_tiles;
    const int tx = pt % tiles_x;
    const int ty = (pt / tiles_x) % tiles_y;
    const int tb = pt / (tiles_x * tiles_y);
    const int x0 = tx * C::TW, y0 = ty * C::TRI, b0 = tb * C::NIMG, co0 = ct * C::COUT_T;

#if defined(MVLM_CONV_TIMING)
    const long long t_start = clock64();
    long long t_loop = t_start;
#endif
    const int H = a.H, W = a.W;
    const int Hin = a.up_in ? (H >> 1) : H, Win = a.up_in ? (W >> 1) : W;
    const unsigned HWin = unsigned(Hin) * unsigned(Win);

    // ---- per-thread staging plan for the input tile (fixed across K-chunks) ----------
    unsigned goff[C::X_ITERS];
    unsigned goff2[C::X_ITERS];  // IN2: offsets into the half-resolution tensor
#pragma unroll
    for (int i = 0; i < C::X_ITERS; ++i) {
        const int e = tid + i * 256;
        const int c = e / C::PLANE;
        const int rem = e - c * C::PLANE;
        const int img = rem / (C::PH * C::PW);
        const int rem2 = rem - img * (C::PH * C::PW);
        const int yy = rem2 / C::PW;
        const int xx = rem2 - yy * C::PW;
        const int y = y0 + yy - C::HALO, x = x0 + xx - C::HALO, b = b0 + img;
        const bool ok = (e < C::XT) && y >= 0 && y < H && x >= 0 && x < W && b < a.B;
        const int ys = a.up_in ? (y >> 1) : y, xs = a.up_in ? (x >> 1) : x;
        goff[i] = ok ? (unsigned(b * a.in_ctot + a.in_coff + c) * HWin + unsigned(ys * Win + xs)) : INVALID_OFF;
        goff2[i] = (IN2 && ok) ? (unsigned(b * a.in2_ctot + c) * (HWin >> 2) + unsigned((ys >> 1) * (Win >> 1) + (xs >> 1))) : 0u;
    }
    // weight slice: float4 index f -> (tap, c, cout4); the source offset is chunk-invariant
    // apart from the channel base
    unsigned woff_g[C::W_ITERS];
#pragma unroll
    for (int i = 0; i < C::W_ITERS; ++i) {
        const int f = tid + i * 256;
        const int row = f / (C::COUT_T / 4);
        const int c4 = f - row * (C::COUT_T / 4);
        const int tap = row / C::CK;
        const int c = row - tap * C::CK;
        woff_g[i] = (f < C::WT / 4) ? unsigned((tap * a.cin_pad + c) * a.cout_pad + co0 + c4 * 4) : INVALID_OFF;
    }

    // ---- per-lane operand offsets inside a stage ---------------------------------------
    int pixoff[C::NT];
#pragma unroll
    for (int n = 0; n < C::NT; ++n) {
        const int p = (C::SPLITK ? 0 : wave * (C::PIX_T / 4)) + n * 32 + l31;
        const int x = p % C::TW;
        const int rr = p / C::TW;
        const int yl = rr % C::TRI;
        const int img = rr / C::TRI;
        pixoff[n] = (img * C::PH + yl) * C::PW + x + half * C::PLANE + (C::KS == 2 ? a.sub_y * C::PW + a.sub_x : 0) +
                    (C::SPLITK ? wave * C::CKW * C::PLANE : 0);
    }
    const int woff = C::XT_PAD + half * C::COUT_T + l31 + (C::SPLITK ? wave * C::CKW * C::COUT_T : 0);

    f32x16 acc[C::EMT][C::ENT];
#pragma unroll
    for (int m = 0; m < C::EMT; ++m)
#pragma unroll
        for (int n = 0; n < C::ENT; ++n) acc[m][n] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // 16-row strip (TAIL16): lane l multiplies channel 32*MT + (l & 15) with k = l >> 4 of a tap's four
    // channels; result register i of column group j is channel 32*MT + 4*(l >> 4) + i at pixel 16*j + (l & 15)
    const int q16 = lane >> 4, i16 = lane & 15;
    const int woff16 = C::XT_PAD + q16 * C::COUT_T + C::MT * 32 + i16;
    int pixoff16[C::NT16];
    f32x4 acc16[C::NT16];
#pragma unroll
    for (int j = 0; j < C::NT16; ++j) {
        const int p = wave * (C::PIX_T / 4) + j * 16 + i16;
        pixoff16[j] = (p / C::TW % C::TRI) * C::PW + p % C::TW + q16 * C::PLANE + (C::KS == 2 ? a.sub_y * C::PW + a.sub_x : 0);
        acc16[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    Strip4 s4;
    if constexpr (C::TAIL4) {
        const int p = wave * (C::PIX_T / 4) + lane;  // this lane's pixel of the tile
        s4.woff4 = C::XT_PAD + C::MT * 32 + 16 + (lane & 3);
        s4.pixoff4 = (p / C::TW % C::TRI) * C::PW + p % C::TW + (C::KS == 2 ? a.sub_y * C::PW + a.sub_x : 0);
    }
    // The consumer-side BatchNorm (scale, shift per input channel) is read from an LDS copy.  The first
    // chunk takes its parameters straight from global memory, so the table fill, the first input tile
    // and the first weight slice are ONE memory round trip, closed by the barrier below.
    float* sbn = smem + 2 * C::STAGE;
    StageRegs<C> regs;
    constexpr int T_TOT = C::X_ITERS + C::W_ITERS;
    int cb0 = 0, cb1 = a.cin_pad;  // this workgroup's input channels
    if constexpr (C::SPLITK) {
        const int span = a.cin_pad / a.kparts;
        cb0 = kp * span;
        cb1 = cb0 + span;
    }
    // Split-K tiles (one 32x32 tile per workgroup, no K parts over workgroups): after the reduction wave w owns the
    // accumulator registers 4w..4w+3 = the channels co0 + 8w + 4 half + (0..3) and finishes them alone, so the four
    // waves' epilogues run side by side.  Its residual values are requested HERE, before the K loop: the epilogue of
    // these latency-bound launches then adds and stores without a memory round trip of its own.
    SplitKTails<C::SPLITK ? C::NT : 1> sks;
    if constexpr (C::SPLITK) {
        if (a.kparts <= 1) {
#pragma unroll
            for (int n = 0; n < C::NT; ++n) {
                SplitKTail& sk = sks.t[n];
                const int p = n * 32 + l31;
                const int rr = p / C::TW;
                const int b = b0 + rr / C::TRI;
                const int y = y0 + rr % C::TRI, x = x0 + p % C::TW;
                sk.ok = C::NIMG == 1 ? true : (b < a.B);
                sk.b = sk.ok ? unsigned(b) : 0u;
                sk.pix = unsigned(y * a.W + x);
                sk.y = y;
                sk.x = x;
                const unsigned HWo = unsigned(a.H) * unsigned(a.W);
                const int cl = co0 + 8 * wave + 4 * half;  // this lane's first channel
                if (a.res1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cs = (cl + j < a.cout) ? cl + j : 0;  // padded channel rows read inside the tensor
                        sk.res[j] = a.res1[(size_t(sk.b) * a.res1_ctot + a.res1_coff + cs) * HWo + sk.pix];
                    }
                    if (a.res2) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int cs = (cl + j < a.cout) ? cl + j : 0;
                            sk.res[j] += a.res2[(size_t(sk.b) * a.res2_ctot + a.res2_coff + cs) * HWo + sk.pix];
                        }
                    }
                }
            }
        }
    }
    if constexpr (C::WINO4) {
#if defined(MVLM_CONV_TIMING)
        wino4_main<C>(a, smem, tid, y0, x0, b0, co0, HWin, woff, acc, &t_loop);
#else
        wino4_main<C>(a, smem, tid, y0, x0, b0, co0, HWin, woff, acc, nullptr);
#endif
    } else if constexpr (C::WINO) {
#if defined(MVLM_CONV_TIMING)
        wino_main<C>(a, smem, tid, y0, x0, b0, co0, HWin, woff, acc, &t_loop);
#else
        wino_main<C>(a, smem, tid, y0, x0, b0, co0, HWin, woff, acc, nullptr);
#endif
    } else {
        static_for<0, T_TOT>([&](auto tc) { issue_item<C, decltype(tc)::value, true, IN2>(a, cb0, tid, HWin, sbn, goff, woff_g, regs, smem, goff2); });
        if (a.pre_scale != nullptr) {
            for (int i = tid; i < a.cin_pad; i += 256) {
                sbn[i] = a.pre_scale[i];
                sbn[C::BN_MAXC + i] = a.pre_shift[i];
            }
        }
        static_for<0, T_TOT>([&](auto tc) { write_item<C, decltype(tc)::value, IN2>(a, cb0, tid, smem, goff, regs); });
        __syncthreads();

#if defined(MVLM_CONV_TIMING)
        t_loop = clock64();
#endif
        int cur = 0;
        for (int cb = cb0 + C::CK; cb < cb1; cb += C::CK) {
#if defined(MVLM_ABLATE_NO_STAGING)  // timing experiment only: wrong results
            compute_chunk<C, false, AMAX, IN2>(a, smem + cur * C::STAGE, smem + (cur ^ 1) * C::STAGE, cb, tid, HWin, sbn, woff, pixoff,
                                    goff, woff_g, regs, acc, woff16, pixoff16, acc16, s4, goff2);
#else
            compute_chunk<C, true, AMAX, IN2>(a, smem + cur * C::STAGE, smem + (cur ^ 1) * C::STAGE, cb, tid, HWin, sbn, woff, pixoff,
                                   goff, woff_g, regs, acc, woff16, pixoff16, acc16, s4, goff2);
#endif
#if !defined(MVLM_ABLATE_NO_BARRIER)
            __syncthreads();  // next stage complete; everybody is done reading this one
#endif
            cur ^= 1;
        }
        compute_chunk<C, false, AMAX, IN2>(a, smem + cur * C::STAGE, nullptr, 0, tid, HWin, sbn, woff, pixoff, goff, woff_g, regs, acc, woff16, pixoff16, acc16, s4, goff2);
    }
#if defined(MVLM_CONV_TIMING)
    const long long t_epi = clock64();
#endif

#if defined(MVLM_ABLATE_NO_EPILOGUE)  // timing experiment only: wrong results
    {
        float sacc = 0.f;
        static_for<0, C::EMT>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
#pragma unroll
            for (int n = 0; n < C::ENT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc += acc[m][n][r];
        });
        if (sacc == 123.456f) a.out[0] = sacc;
        return;
    }
#endif
    if constexpr (C::SPLITK && !AMAX) {
        if (a.kparts <= 1) {
            // every wave leaves its partial tile in LDS, then wave w adds registers 4w..4w+3 of the four partials in wave
            // order ((w0 + w1) + w2) + w3 - the order of the single-wave reduction below, bit for bit - and finishes them;
            // a two-column tile does that column by column through the same buffer
            static_assert(!C::SPLITK || 2 * C::STAGE >= 4 * 16 * 64, "the four partial tiles must fit the two stages");
            float* const red = smem;
            const unsigned HWo = unsigned(a.H) * unsigned(a.W);
            const int cl = co0 + 8 * wave + 4 * half;
            f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, ps4 = {1.f, 1.f, 1.f, 1.f}, pt4 = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) bias4 = *reinterpret_cast<const f32x4*>(a.bias + cl);  // padded to cout_pad: never out of bounds
            if (a.post_scale) {
                ps4 = *reinterpret_cast<const f32x4*>(a.post_scale + cl);
                pt4 = *reinterpret_cast<const f32x4*>(a.post_shift + cl);
            }
            static_for<0, C::NT>([&](auto nc) {
                constexpr int n = decltype(nc)::value;
                const SplitKTail& sk = sks.t[n];
                __syncthreads();  // every wave is done reading the stages (or the previous column's partials): reuse them as the exchange buffer
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[0][n][r];
                __syncthreads();
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = red[(0 * 16 + 4 * wave + j) * 64 + lane];
                    t += red[(1 * 16 + 4 * wave + j) * 64 + lane];
                    t += red[(2 * 16 + 4 * wave + j) * 64 + lane];
                    t += red[(3 * 16 + 4 * wave + j) * 64 + lane];
                    v[j] = t;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (a.bias) v[j] += bias4[j];
                    if (a.post_scale) v[j] = fmaxf(fmaf(v[j], ps4[j], pt4[j]), 0.f);
                }
                if (a.out_raw) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (sk.ok && cl + j < a.cout) a.out_raw[(size_t(sk.b) * a.raw_ctot + a.raw_coff + cl + j) * HWo + sk.pix] = v[j];
                }
                if (a.res1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += sk.res[j];
                }
                if constexpr (C::POOL_SMALL) {
                    if (a.pool_out) {  // (wave-uniform: every lane takes part in the exchanges)
                        const unsigned o_pool = unsigned((sk.y >> 1) * (a.W >> 1) + (sk.x >> 1));
                        const bool writer = sk.ok && (l31 & C::TW) == 0 && (l31 & 1) == 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float m1 = fmaxf(v[j], __shfl_xor(v[j], C::TW));  // the row below / above
                            const int mi = __float_as_int(m1);
                            const float m2 = fmaxf(m1, __int_as_float(__builtin_amdgcn_update_dpp(mi, mi, 0xB1, 0xf, 0xf, false)));  // lane ^ 1
                            if (writer && cl + j < a.cout) a.pool_out[(size_t(sk.b) * a.pool_ctot + a.pool_coff + cl + j) * (HWo / 4) + o_pool] = m2;
                        }
                    }
                }
                if (a.out) {
                    if (!a.up_out) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (sk.ok && cl + j < a.cout) a.out[(size_t(sk.b) * a.out_ctot + a.out_coff + cl + j) * HWo + sk.pix] = v[j];
                    } else if (a.up_out == 2) {
                        const unsigned o2 = unsigned(2 * sk.y + a.sub_y) * unsigned(2 * a.W) + unsigned(2 * sk.x + a.sub_x);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (sk.ok && cl + j < a.cout) a.out[(size_t(sk.b) * a.out_ctot + a.out_coff + cl + j) * (4u * HWo) + o2] = v[j];
                    } else {
                        // hourglass up-path: the value goes to its 2x2 block of the skip tensor, added in place (:334-359)
                        const unsigned W2 = 2u * unsigned(a.W);
                        const unsigned o2 = unsigned(2 * sk.y) * W2 + unsigned(2 * sk.x);
                        float2 s0[4], s1[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int cs = (cl + j < a.cout) ? cl + j : 0;
                            const float* const ps = a.skip + (size_t(sk.b) * a.skip_ctot + a.skip_coff + cs) * (4u * HWo) + o2;
                            s0[j] = *reinterpret_cast<const float2*>(ps);
                            s1[j] = *reinterpret_cast<const float2*>(ps + W2);
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (sk.ok && cl + j < a.cout) {
                                float* const po = a.out + (size_t(sk.b) * a.out_ctot + a.out_coff + cl + j) * (4u * HWo) + o2;
                                *reinterpret_cast<float2*>(po) = make_float2(v[j] + s0[j].x, v[j] + s0[j].y);
                                *reinterpret_cast<float2*>(po + W2) = make_float2(v[j] + s1[j].x, v[j] + s1[j].y);
                            }
                        }
                    }
                }
            });
            return;
        }
    }
    if constexpr (C::SPLITK) {
        // (input channels also divided over workgroups, or a fused-argmax launch) add the four waves' partial tiles in wave
        // order (deterministic), wave 0 finishes alone
        __syncthreads();  // every wave is done reading the stages: reuse them as the exchange buffer
        float* red = smem;
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[0][0][r];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][0][r] += red[(w * 16 + r) * 64 + lane];
        if (a.kparts > 1) {
            // partial tile -> workspace; the workgroup that takes the last ticket of this tile sums all parts in part
            // order (its own from memory too, so the order does not depend on who arrives last) and runs the epilogue
            float* const mine = a.kws + (size_t(tile_id) * a.kparts + kp) * 1024;
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[r * 64 + lane] = acc[0][0][r];
            __threadfence();  // release: the partial is visible device-wide before the ticket
            unsigned ticket = 0;
            if (lane == 0) ticket = atomicAdd(a.kcnt + tile_id, 1u);
            ticket = __builtin_amdgcn_readfirstlane(ticket);
            if (ticket != unsigned(a.kparts - 1)) return;
            __threadfence();  // acquire: the other parts' stores
            if (lane == 0) a.kcnt[tile_id] = 0;  // ready for the next launch on this stream
            const float* const all = a.kws + size_t(tile_id) * a.kparts * 1024;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][0][r] = __builtin_nontemporal_load(all + r * 64 + lane);
            for (int q = 1; q < a.kparts; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][0][r] += __builtin_nontemporal_load(all + q * 1024 + r * 64 + lane);
        }
    }

    if constexpr (AMAX) {
        // Fused heatmap argmax (paulsenpredictor.py:123) on the TRANSPOSED accumulators: conv11 has no residual /
        // post-BN, so the heatmap value is acc + bias.  Lane (half, l31) owns output channel co0 + 32 m + l31 and, of
        // every 32-pixel row segment n of its wave, the pixels x0 + (r & 3) + 8 (r >> 2) + 4 half: the maximum over a
        // lane's pixels is a chain of compares on registers (np.argmax order through argmax_key: NaN = maximum,
        // first maximum in row-major order wins), one exchange between the half-waves finishes a wave's partial.
        const int W = a.W;
        constexpr int ROWS_PER_WAVE = C::PIX_T / 4 / C::TW;  // = NT for the 32-pixel-row tiles
        static_assert(C::TW == 32 && C::NIMG == 1 && ROWS_PER_WAVE == C::NT, "fused argmax expects 32-pixel row tiles");
        const size_t part = size_t(a.amax_part0) + (size_t(ty) * tiles_x + tx) * 4 + wave;
        auto pixel_index = [&](int y, int x) {
            return a.up_out == 2 ? (2 * y + a.sub_y) * (2 * W) + 2 * x + a.sub_x : y * W + x;
        };
        static_for<0, C::MT>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            const int co = co0 + m * 32 + l31;
            const float bias = (a.bias && co < a.cout) ? a.bias[co] : 0.f;
            int best_k = int(0x807fffff);  // argmax_key(-inf)
            int best_i = 0x7fffffff;
#pragma unroll
            for (int n = 0; n < C::NT; ++n) {
                const int y = y0 + wave * ROWS_PER_WAVE + n;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int x = x0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const int k = argmax_key(acc[m][n][r] + bias);
                    const int pix = pixel_index(y, x);
                    const bool better = k > best_k;  // ascending pixel order within the lane: strict > keeps the first
                    best_k = better ? k : best_k;
                    best_i = better ? pix : best_i;
                }
            }
            // the other half-wave holds the other pixels of the same channel
            const int ok = __shfl_xor(best_k, 32), oi = __shfl_xor(best_i, 32);
            if (ok > best_k || (ok == best_k && oi < best_i)) {
                best_k = ok;
                best_i = oi;
            }
            if (half == 0 && co < a.cout && b0 < a.B) {
                const size_t o = (size_t(b0) * a.cout + co) * a.amax_parts + part;
                a.amax_val[o] = argmax_value(best_k);
                a.amax_idx[o] = best_i;
            }
        });
        if constexpr (C::TAIL16) {
            // strip (transposed 16x16x4 tiles): lane (q16, i16) owns channel co0 + 32 MT + i16 and the pixels
            // 16 j + 4 q16 + i of its wave's pixel range
            const int co = co0 + C::MT * 32 + i16;
            const float bias = (a.bias && co < a.cout) ? a.bias[co] : 0.f;
            int best_k = int(0x807fffff);
            int best_i = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < C::NT16; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int p = wave * (C::PIX_T / 4) + j * 16 + 4 * q16 + i;
                    const int k = argmax_key(acc16[j][i] + bias);
                    const int pix = pixel_index(y0 + p / C::TW, x0 + p % C::TW);
                    const bool better = k > best_k || (k == best_k && pix < best_i);
                    best_k = better ? k : best_k;
                    best_i = better ? pix : best_i;
                }
#pragma unroll
            for (int s = 16; s <= 32; s <<= 1) {
                const int ok = __shfl_xor(best_k, s), oi = __shfl_xor(best_i, s);
                if (ok > best_k || (ok == best_k && oi < best_i)) {
                    best_k = ok;
                    best_i = oi;
                }
            }
            if (q16 == 0 && co < a.cout && b0 < a.B) {
                const size_t o = (size_t(b0) * a.cout + co) * a.amax_parts + part;
                a.amax_val[o] = argmax_value(best_k);
                a.amax_idx[o] = best_i;
            }
        }
        if constexpr (C::TAIL4) {
            // 4-row strip: register v = channel co0 + 32 MT + 16 + v at THIS lane's pixel (64 consecutive pixels of the
            // tile per wave): the wave's partial of a channel is a 64-lane reduction, first maximum in row-major order
            const int p = wave * (C::PIX_T / 4) + lane;
            const int pix = pixel_index(y0 + p / C::TW, x0 + p % C::TW);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int co = co0 + C::MT * 32 + 16 + v;
                const float bias = (a.bias && co < a.cout) ? a.bias[co] : 0.f;
                int best_k = argmax_key(s4.acc[v] + bias), best_i = pix;
#pragma unroll
                for (int sft = 1; sft <= 32; sft <<= 1) {
                    const int ok = __shfl_xor(best_k, sft), oi = __shfl_xor(best_i, sft);
                    if (ok > best_k || (ok == best_k && oi < best_i)) {
                        best_k = ok;
                        best_i = oi;
                    }
                }
                if (lane == 0 && co < a.cout && b0 < a.B) {
                    const size_t o = (size_t(b0) * a.cout + co) * a.amax_parts + part;
                    a.amax_val[o] = argmax_value(best_k);
                    a.amax_idx[o] = best_i;
                }
            }
        }
        return;
    }

    // ---------------------------------- epilogue ---------------------------------------
    // Addresses are wave-uniform channel bases (scalar registers) + one 32-bit per-lane offset per
    // tensor and pixel column, so an element costs a load/add/store, not 64-bit vector arithmetic.
    const unsigned HW = unsigned(H) * unsigned(W);
    // the wave's place in the epilogue's geometry (Cfg::EMT ...): the wide F(4,3) shape's wave finishes row quad wave & 1 of the
    // cout half wave >> 1, every other tile's wave its quarter of the pixels of all channels
    const int ewave = C::WIDE4 ? (wave & 1) : wave;
    const int eco0 = C::WIDE4 ? co0 + 32 * (wave >> 1) : co0;
    bool lane_ok[C::ENT];
    int ppix[C::ENT];
    unsigned o_raw[C::ENT], o_r1[C::ENT], o_r2[C::ENT], o_out[C::ENT], o_skip[C::ENT];
    // fused 2x2 max-pool: the rows of a pair are two pixel registers of one lane (n, n+1), the columns two
    // neighbouring lanes, so it needs 32-pixel tile rows, one image per tile and an even row count per wave
    constexpr bool CAN_POOL = !C::SPLITK && C::TW == 32 && C::NIMG == 1 && C::ENT % 2 == 0;
    constexpr bool POOLS = C::POOL_SMALL;  // narrow tiles: partner lanes l ^ TW (row) and l ^ 1 (column), see Cfg
    unsigned o_pool[C::ENT / 2 > 0 ? C::ENT / 2 : 1];
    unsigned o_pool_s[POOLS ? C::ENT : 1];
    const bool pool_writer = (l31 & (C::TW & 31)) == 0 && (l31 & 1) == 0;
#pragma unroll
    for (int n = 0; n < C::ENT; ++n) {
        const int p = (C::SPLITK ? 0 : ewave * C::EPIX) + n * 32 + l31;
        const int rr = p / C::TW;
        const int b = b0 + rr / C::TRI;
        const int y = y0 + rr % C::TRI, x = x0 + p % C::TW;
        lane_ok[n] = C::NIMG == 1 ? true : (b < a.B);
        const unsigned bb = lane_ok[n] ? unsigned(b) : 0u;
        const unsigned pix = unsigned(y * W + x);
        const unsigned h4 = 4u * unsigned(half);
        ppix[n] = int(pix);
        o_raw[n] = (bb * a.raw_ctot + a.raw_coff + h4) * HW + pix;
        o_r1[n] = (bb * a.res1_ctot + a.res1_coff + h4) * HW + pix;
        o_r2[n] = (bb * a.res2_ctot + a.res2_coff + h4) * HW + pix;
        if constexpr (CAN_POOL)
            if ((n & 1) == 0) o_pool[n / 2] = (bb * a.pool_ctot + a.pool_coff + h4) * (HW / 4) + unsigned((y >> 1) * (W >> 1) + (x >> 1));
        if constexpr (POOLS) o_pool_s[n] = (bb * a.pool_ctot + a.pool_coff + h4) * (HW / 4) + unsigned((y >> 1) * (W >> 1) + (x >> 1));
        if (!a.up_out) {
            o_out[n] = (bb * a.out_ctot + a.out_coff + h4) * HW + pix;
            o_skip[n] = 0;
        } else if (a.up_out == 2) {
            const unsigned o2 = unsigned(2 * y + a.sub_y) * unsigned(2 * W) + unsigned(2 * x + a.sub_x);
            o_out[n] = (bb * a.out_ctot + a.out_coff + h4) * (4u * HW) + o2;
            o_skip[n] = 0;
            ppix[n] = int(o2);  // the argmax runs over full-resolution pixel indices
        } else {
            const unsigned o2 = unsigned(2 * y) * unsigned(2 * W) + unsigned(2 * x);
            o_out[n] = (bb * a.out_ctot + a.out_coff + h4) * (4u * HW) + o2;
            o_skip[n] = (bb * a.skip_ctot + a.skip_coff + h4) * (4u * HW) + o2;
        }
    }
    // Channels are walked in groups of four accumulator registers (= four consecutive channels
    // per half-wave).  The residual values of group g+1 are loaded (unconditionally, clamped
    // addresses) before group g is finished and stored, so a load's latency is paid once per
    // group of 4*NT elements instead of once per element, and the feature flags cost one
    // wave-uniform branch per group.
    constexpr int GE = 4 * C::ENT;       // elements per group
    constexpr int NG = C::EMT * 4;       // groups per wave
    auto epilogue = [&](auto full_c) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_c)::value;  // every channel row of this tile exists
        // The tensors may share storage (a block adds into its own residual slice in place, the
        // hourglass adds into its skip tensor), but only element-wise: a value is stored to the
        // address it was loaded from, never to another group's.  __restrict__ tells the compiler
        // exactly that, so it stops draining the memory pipeline (s_waitcnt vmcnt(0)) between one
        // group's stores and the next group's loads.
        const float* __restrict__ const t_res1 = a.res1;
        const float* __restrict__ const t_res2 = a.res2;
        const float* __restrict__ const t_skip = a.skip;
        float* __restrict__ const t_raw = a.out_raw;
        float* __restrict__ const t_out = a.out;
        float* __restrict__ const t_pool = a.pool_out;
        float resv[2][GE];
        auto group_base = [&](int g) { return eco0 + (g >> 2) * 32 + 8 * (g & 3); };  // wave-uniform first channel
        auto load_group = [&](auto gc, float (&dst)[GE]) {
            constexpr int g = decltype(gc)::value;
            if (a.res1) {
                const int cs0 = group_base(g);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // clamp the row so padded channel rows still read inside the tensor
                    const int cs = (FULL || cs0 + j + 4 < a.cout) ? cs0 + j : 0;
                    const float* const p1 = t_res1 + size_t(cs) * HW;
#pragma unroll
                    for (int n = 0; n < C::ENT; ++n) dst[j * C::ENT + n] = p1[o_r1[n]];
                }
                if (a.res2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cs = (FULL || cs0 + j + 4 < a.cout) ? cs0 + j : 0;
                        const float* const p2 = t_res2 + size_t(cs) * HW;
#pragma unroll
                        for (int n = 0; n < C::ENT; ++n) dst[j * C::ENT + n] += p2[o_r2[n]];
                    }
                }
            }
        };
        load_group(std::integral_constant<int, 0>{}, resv[0]);
        static_for<0, NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            constexpr int m = g >> 2, rg = g & 3;
            if constexpr (g + 1 < NG) load_group(std::integral_constant<int, g + 1>{}, resv[(g + 1) & 1]);
            // keep the next group's loads HERE: the scheduler otherwise sinks them to their first use and
            // every group pays a full memory round trip
            __builtin_amdgcn_sched_barrier(0);
            const int cs0 = group_base(g);
            // bias / post-BN parameters of this lane's four channels: ONE 16-byte load each (the
            // vectors are padded to cout_pad, so rows beyond cout read zeros, never out of bounds)
            const int cl = cs0 + 4 * half;
            f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, ps4 = {1.f, 1.f, 1.f, 1.f}, pt4 = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) bias4 = *reinterpret_cast<const f32x4*>(a.bias + cl);
            if (a.post_scale) {
                ps4 = *reinterpret_cast<const f32x4*>(a.post_scale + cl);
                pt4 = *reinterpret_cast<const f32x4*>(a.post_shift + cl);
            }
            float vals[GE];
            bool okc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                okc[j] = FULL || cl + j < a.cout;
#pragma unroll
                for (int n = 0; n < C::ENT; ++n) {
                    float v = acc[m][n][4 * rg + j];
                    if (a.bias) v += bias4[j];
                    if (a.post_scale) v = fmaxf(fmaf(v, ps4[j], pt4[j]), 0.f);
                    vals[j * C::ENT + n] = v;
                }
            }
            if (a.out_raw) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float* const p = t_raw + size_t(cs0 + j) * HW;
#pragma unroll
                    for (int n = 0; n < C::ENT; ++n)
                        if (okc[j] && lane_ok[n]) p[o_raw[n]] = vals[j * C::ENT + n];
                }
            }
            if (a.res1) {
#pragma unroll
                for (int e = 0; e < GE; ++e) vals[e] += resv[g & 1][e];
            }
            if constexpr (CAN_POOL) {
                if (a.pool_out) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float* const p = t_pool + size_t(cs0 + j) * (HW / 4);
#pragma unroll
                        for (int q = 0; q < C::ENT / 2; ++q) {
                            const float v2 = fmaxf(vals[j * C::ENT + 2 * q], vals[j * C::ENT + 2 * q + 1]);
                            const int vi = __float_as_int(v2);
                            const float other = __int_as_float(__builtin_amdgcn_update_dpp(vi, vi, 0xB1, 0xf, 0xf, false));  // lane ^ 1
                            if (okc[j] && (l31 & 1) == 0) p[o_pool[q]] = fmaxf(v2, other);
                        }
                    }
                }
            }
            if constexpr (POOLS) {
                if (a.pool_out) {  // (wave-uniform)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float* const p = t_pool + size_t(cs0 + j) * (HW / 4);
#pragma unroll
                        for (int n = 0; n < C::ENT; ++n) {
                            const float m1 = fmaxf(vals[j * C::ENT + n], __shfl_xor(vals[j * C::ENT + n], C::TW));
                            const int mi = __float_as_int(m1);
                            const float m2 = fmaxf(m1, __int_as_float(__builtin_amdgcn_update_dpp(mi, mi, 0xB1, 0xf, 0xf, false)));  // lane ^ 1
                            if (okc[j] && lane_ok[n] && pool_writer) p[o_pool_s[n]] = m2;
                        }
                    }
                }
            }
            if (a.out) {
                if (a.up_out != 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float* const p = t_out + size_t(cs0 + j) * HW * (a.up_out ? 4 : 1);
#pragma unroll
                        for (int n = 0; n < C::ENT; ++n)
                            if (okc[j] && lane_ok[n]) p[o_out[n]] = vals[j * C::ENT + n];
                    }
                } else {
                    const unsigned W2 = 2u * unsigned(W);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // the row's skip loads first, then its 2x2 scatter
                        const int cs = okc[j] ? cs0 + j : 0;
                        const float* const ps = t_skip + size_t(cs) * HW * 4;
                        float* const p = t_out + size_t(cs0 + j) * HW * 4;
                        float2 s0[C::ENT], s1[C::ENT];
#pragma unroll
                        for (int n = 0; n < C::ENT; ++n) {
                            s0[n] = *reinterpret_cast<const float2*>(ps + o_skip[n]);
                            s1[n] = *reinterpret_cast<const float2*>(ps + o_skip[n] + W2);
                        }
#pragma unroll
                        for (int n = 0; n < C::ENT; ++n) {
                            if (okc[j] && lane_ok[n]) {
                                const float v = vals[j * C::ENT + n];
                                *reinterpret_cast<float2*>(p + o_out[n]) = make_float2(v + s0[n].x, v + s0[n].y);
                                *reinterpret_cast<float2*>(p + o_out[n] + W2) = make_float2(v + s1[n].x, v + s1[n].y);
                            }
                        }
                    }
                }
            }
        });
    };
    // Branch-free epilogues for the layer kinds that carry the time (full channel tiles, plain
    // NCHW output).  The general epilogue above tests its feature flags per group; at every join
    // of such a branch the compiler has to assume the worst about outstanding memory operations
    // and drains the pipeline (s_waitcnt vmcnt(0)) - which serialises "load residual, add, store"
    // into one memory round trip per group (measured: 74k of a c128 tile's 1.3M cycles).  With
    // the flags as template parameters every load and store is unconditional, the waits are exact
    // and the residual / parameter prefetch really runs ahead.
    //   RAW: also store the pre-residual value (input of the block's next conv)
    //   RES: add the residual slice        PAR: 0 none, 1 bias, 2 bias + post-BatchNorm + ReLU
    //   POOL: also store the 2x2 max-pooled value
    //   RES 2: two residuals, (res1 + res2) + value (conv7: r3 + ll1 + conv7(x), paulsenpredictor.py:422)
    //   SCAT: the hourglass up-path - the value goes to its 2x2 block of the skip tensor, added in place (:334-359)
    auto epilogue_fast = [&](auto raw_c, auto res_c, auto par_c, auto pool_c, auto scat_c) __attribute__((always_inline)) {
        constexpr bool RAW = decltype(raw_c)::value, RES = decltype(res_c)::value != 0, RES2 = decltype(res_c)::value == 2;
        constexpr bool POOL = decltype(pool_c)::value != 0, FULL_OUT = decltype(pool_c)::value != 2;  // 2: pooled tensor only
        constexpr bool SCAT = decltype(scat_c)::value;
        constexpr int PAR = decltype(par_c)::value;
        // residual prefetch distance in groups (measured: 3 and 5 perform alike, 6 spills on the
        // 128-accumulator tiles)
        constexpr int PF_WANT = (GE <= 8 && !RES2 && !SCAT) ? 3 : 1;  // (two residual rings / the skip blocks: registers)
        constexpr int PF = RES ? (PF_WANT < NG ? PF_WANT : NG) : 0;
        constexpr int RING = PF + 1;
        float resv[RING][GE];
        float resv2[RES2 ? RING : 1][GE];
        f32x4 bias_r[2], ps_r[2], pt_r[2];
        auto chan0 = [&](int g) { return eco0 + (g >> 2) * 32 + 8 * (g & 3); };  // wave-uniform first channel
        auto ld_res = [&](auto gc) __attribute__((always_inline)) {
            constexpr int g = decltype(gc)::value;
            if constexpr (RES) {
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    const float* const p1 = a.res1 + size_t(chan0(g) + j) * HW;
                    static_for<0, C::ENT>([&](auto nc) {
                        constexpr int n = decltype(nc)::value;
                        resv[g % RING][j * C::ENT + n] = p1[o_r1[n]];
                    });
                    if constexpr (RES2) {
                        const float* const p2 = a.res2 + size_t(chan0(g) + j) * HW;
                        static_for<0, C::ENT>([&](auto nc) {
                            constexpr int n = decltype(nc)::value;
                            resv2[g % RING][j * C::ENT + n] = p2[o_r2[n]];
                        });
                    }
                });
            }
        };
        auto ld_par = [&](auto gc) __attribute__((always_inline)) {
            constexpr int g = decltype(gc)::value;
            if constexpr (PAR >= 1) bias_r[g & 1] = *reinterpret_cast<const f32x4*>(a.bias + chan0(g) + 4 * half);
            if constexpr (PAR == 2) {
                ps_r[g & 1] = *reinterpret_cast<const f32x4*>(a.post_scale + chan0(g) + 4 * half);
                pt_r[g & 1] = *reinterpret_cast<const f32x4*>(a.post_shift + chan0(g) + 4 * half);
            }
        };
        static_for<0, (PF < NG ? PF : NG)>([&](auto gc) { ld_res(gc); });
        ld_par(std::integral_constant<int, 0>{});
        static_for<0, NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            constexpr int m = g >> 2, rg = g & 3;
            if constexpr (g + PF < NG) ld_res(std::integral_constant<int, g + PF>{});
            if constexpr (g + 1 < NG) ld_par(std::integral_constant<int, g + 1>{});
            const int cs0 = chan0(g);
            // the group's 2x2 blocks of the skip tensor, SK_CH channels at a time, requested before those channels' other
            // work (two where the registers allow it: pipelining a channel ahead, or a whole group at once, spilled on the
            // 168-register tiles)
            constexpr int SK_CH = (C::MIN_BLOCKS_PER_CU == 2 && C::ENT <= 2) ? 2 : 1;
            float2 sk0[SCAT ? SK_CH * C::ENT : 1], sk1[SCAT ? SK_CH * C::ENT : 1];
            auto ld_skip = [&](auto hc) __attribute__((always_inline)) {
                constexpr int h = decltype(hc)::value;  // channels SK_CH h ... of the group
                if constexpr (SCAT) {
                    const unsigned W2 = 2u * unsigned(W);
                    static_for<0, SK_CH>([&](auto jc) {
                        constexpr int jj = decltype(jc)::value, j = SK_CH * h + jj;
                        const float* const ps = a.skip + size_t(cs0 + j) * HW * 4;
                        static_for<0, C::ENT>([&](auto nc) {
                            constexpr int n = decltype(nc)::value;
                            sk0[jj * C::ENT + n] = *reinterpret_cast<const float2*>(ps + o_skip[n]);
                            sk1[jj * C::ENT + n] = *reinterpret_cast<const float2*>(ps + o_skip[n] + W2);
                        });
                    });
                }
            };
            if constexpr (SK_CH == 2) ld_skip(std::integral_constant<int, 0>{});
            __builtin_amdgcn_sched_barrier(0);  // the prefetches stay ahead of this group's work
            float vals[GE];
            static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                static_for<0, C::ENT>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    float v = acc[m][n][4 * rg + j];
                    if constexpr (PAR >= 1) v += bias_r[g & 1][j];
                    if constexpr (PAR == 2) v = fmaxf(fmaf(v, ps_r[g & 1][j], pt_r[g & 1][j]), 0.f);
                    vals[j * C::ENT + n] = v;
                });
            });
            if constexpr (RAW) {
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    float* const p = a.out_raw + size_t(cs0 + j) * HW;
                    static_for<0, C::ENT>([&](auto nc) {
                        constexpr int n = decltype(nc)::value;
                        if (lane_ok[n]) p[o_raw[n]] = vals[j * C::ENT + n];
                    });
                });
            }
            if constexpr (RES2) {
                static_for<0, GE>([&](auto ec) { vals[decltype(ec)::value] += resv[g % RING][decltype(ec)::value] + resv2[g % RING][decltype(ec)::value]; });
            } else if constexpr (RES) {
                static_for<0, GE>([&](auto ec) { vals[decltype(ec)::value] += resv[g % RING][decltype(ec)::value]; });
            }
            if constexpr (POOL && CAN_POOL) {
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    float* const p = a.pool_out + size_t(cs0 + j) * (HW / 4);
                    static_for<0, C::ENT / 2>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        const float v2 = fmaxf(vals[j * C::ENT + 2 * q], vals[j * C::ENT + 2 * q + 1]);
                        const int vi = __float_as_int(v2);
                        const float other = __int_as_float(__builtin_amdgcn_update_dpp(vi, vi, 0xB1, 0xf, 0xf, false));  // lane ^ 1
                        if ((l31 & 1) == 0) p[o_pool[q]] = fmaxf(v2, other);
                    });
                });
            }
            if constexpr (POOL && POOLS) {
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    float* const p = a.pool_out + size_t(cs0 + j) * (HW / 4);
                    static_for<0, C::ENT>([&](auto nc) {
                        constexpr int n = decltype(nc)::value;
                        const float m1 = fmaxf(vals[j * C::ENT + n], __shfl_xor(vals[j * C::ENT + n], C::TW));
                        const int mi = __float_as_int(m1);
                        const float m2 = fmaxf(m1, __int_as_float(__builtin_amdgcn_update_dpp(mi, mi, 0xB1, 0xf, 0xf, false)));  // lane ^ 1
                        if (lane_ok[n] && pool_writer) p[o_pool_s[n]] = m2;
                    });
                });
            }
            if constexpr (SCAT) {
                const unsigned W2 = 2u * unsigned(W);
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    if constexpr (SK_CH == 1) ld_skip(jc);
                    if constexpr (SK_CH == 2 && j == 2) ld_skip(std::integral_constant<int, 1>{});
                    float* const p = a.out + size_t(cs0 + j) * HW * 4;
                    static_for<0, C::ENT>([&](auto nc) {
                        constexpr int n = decltype(nc)::value;
                        if (lane_ok[n]) {
                            const float v = vals[j * C::ENT + n];
                            const float2 s0 = sk0[(j % SK_CH) * C::ENT + n], s1 = sk1[(j % SK_CH) * C::ENT + n];
                            *reinterpret_cast<float2*>(p + o_out[n]) = make_float2(v + s0.x, v + s0.y);
                            *reinterpret_cast<float2*>(p + o_out[n] + W2) = make_float2(v + s1.x, v + s1.y);
                        }
                    });
                });
            } else if constexpr (FULL_OUT) {
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    float* const p = a.out + size_t(cs0 + j) * HW;
                    static_for<0, C::ENT>([&](auto nc) {
                        constexpr int n = decltype(nc)::value;
                        if (lane_ok[n]) p[o_out[n]] = vals[j * C::ENT + n];
                    });
                });
            }
        });
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    using P0 = std::integral_constant<int, 0>;
    using P2 = std::integral_constant<int, 2>;
    const bool full_tile = eco0 + C::ECOUT <= a.cout;
    const bool has_raw = a.out_raw != nullptr, has_res = a.res1 != nullptr, has_pool = a.pool_out != nullptr;
    const bool scat = a.up_out == 1 && a.skip != nullptr && a.out != nullptr;
    const bool fast_ok = full_tile && !C::SPLITK && (a.out || has_pool) && (!a.up_out || scat) && (!a.skip || scat) && (CAN_POOL || POOLS || !has_pool);
    const int par = a.post_scale ? (a.bias ? 2 : -1) : (a.bias ? 1 : 0);
    const int pool_mode = has_pool ? (a.out ? 1 : 2) : 0;
    const int res_mode = has_res ? (a.res2 ? 2 : 1) : 0;
    using M0 = std::integral_constant<int, 0>;
    using M1 = std::integral_constant<int, 1>;
    using M2 = std::integral_constant<int, 2>;
    using R0 = std::integral_constant<int, 0>;
    using R1 = std::integral_constant<int, 1>;
    using R2 = std::integral_constant<int, 2>;
    using P1 = std::integral_constant<int, 1>;
    const bool plain = fast_ok && !scat;  // the layer kinds of rounds 1-3
    if (plain && has_raw && res_mode == 1 && par == 0 && pool_mode == 0)
        epilogue_fast(T_{}, R1{}, P0{}, M0{}, F_{});  // block conv1 / conv2
    else if (plain && !has_raw && res_mode == 1 && par == 0 && pool_mode == 0)
        epilogue_fast(F_{}, R1{}, P0{}, M0{}, F_{});  // block conv3
    else if (plain && has_raw && res_mode == 1 && par == 0 && pool_mode == 1)
        epilogue_fast(T_{}, R1{}, P0{}, M1{}, F_{});  // ... of a block that is pooled next
    else if (plain && !has_raw && res_mode == 1 && par == 0 && pool_mode == 1)
        epilogue_fast(F_{}, R1{}, P0{}, M1{}, F_{});
    else if (plain && has_raw && res_mode == 1 && par == 0 && pool_mode == 2)
        epilogue_fast(T_{}, R1{}, P0{}, M2{}, F_{});  // ... whose full-resolution output nobody reads (stem)
    else if (plain && !has_raw && res_mode == 1 && par == 0 && pool_mode == 2)
        epilogue_fast(F_{}, R1{}, P0{}, M2{}, F_{});
    else if (plain && !has_raw && res_mode == 0 && par == 2 && pool_mode == 0)
        epilogue_fast(F_{}, R0{}, P2{}, M0{}, F_{});  // conv1, conv5, conv9
    else if (plain && !has_raw && res_mode == 0 && par == 0 && pool_mode == 0)
        epilogue_fast(F_{}, R0{}, P0{}, M0{}, F_{});  // 1x1 resample
    // (the two kinds below only where such a layer can run - 3x3 tiles without a strip: every kind compiled into a tile
    //  costs it registers, and the 80-row tile fell from three resident workgroups per CU to two with them: 166 -> 191)
    else if (C::KS == 3 && !C::TAIL16 && plain && !has_raw && res_mode == 2 && par == 1 && pool_mode == 1) {
        if constexpr (C::KS == 3 && !C::TAIL16) epilogue_fast(F_{}, R2{}, P1{}, M1{}, F_{});  // conv7 (+ the pooled copy the second hourglass starts from)
    } else if (C::KS == 3 && !C::TAIL16 && fast_ok && scat && has_raw && res_mode == 1 && par == 0 && pool_mode == 0) {
        if constexpr (C::KS == 3 && !C::TAIL16) epilogue_fast(T_{}, R1{}, P0{}, M0{}, T_{});  // conv1 / conv2 of a level's last block on the way up
    } else if (C::KS == 3 && !C::TAIL16 && fast_ok && scat && !has_raw && res_mode == 1 && par == 0 && pool_mode == 0) {
        if constexpr (C::KS == 3 && !C::TAIL16) epilogue_fast(F_{}, R1{}, P0{}, M0{}, T_{});  // ... its conv3
    }
    else if (full_tile)
        epilogue(std::true_type{});
    else
        epilogue(std::false_type{});
#if defined(MVLM_CONV_TIMING)
    if (a.timing && tid == 0) {
        __builtin_amdgcn_s_waitcnt(0);  // the epilogue's stores have left the wave
        const long long t_end = clock64();
        atomicAdd(a.timing + 0, (unsigned long long)(t_loop - t_start));
        atomicAdd(a.timing + 1, (unsigned long long)(t_epi - t_loop));
        atomicAdd(a.timing + 2, (unsigned long long)(t_end - t_epi));
        atomicAdd(a.timing + 3, 1ull);
    }
#endif

    // ---- the 16-row strip: plain conv + bias layers only (conv6, conv10, conv11; checked on the host) ----
    int pix16[C::NT16];            // output pixel index of column group j (full resolution for up_out == 2)
    float val16[C::NT16][4];       // acc + bias, kept for the fused argmax
    bool ok16[4];
    if constexpr (C::TAIL16) {
        const unsigned b = unsigned(b0);
#pragma unroll
        for (int j = 0; j < C::NT16; ++j) {
            const int p = wave * (C::PIX_T / 4) + j * 16 + i16;
            const int y = y0 + p / C::TW, x = x0 + p % C::TW;
            pix16[j] = a.up_out == 2 ? (2 * y + a.sub_y) * (2 * W) + 2 * x + a.sub_x : y * W + x;
        }
        const unsigned plane = a.up_out == 2 ? 4u * HW : HW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + C::MT * 32 + 4 * q16 + i;
            ok16[i] = co < a.cout;
            const int coc = ok16[i] ? co : 0;
            const float bias = a.bias ? a.bias[coc] : 0.f;
            float* const po = a.out ? a.out + (size_t(b) * a.out_ctot + a.out_coff + coc) * plane : nullptr;
#pragma unroll
            for (int j = 0; j < C::NT16; ++j) {
                val16[j][i] = acc16[j][i] + bias;
                if (po && ok16[i]) po[pix16[j]] = val16[j][i];
            }
        }
    }
    // ---- the 4-row strip: register v = channel co0 + 32 MT + 16 + v at this lane's pixel (64 consecutive pixels per wave)
    if constexpr (C::TAIL4) {
        const int p = wave * (C::PIX_T / 4) + lane;
        const int y = y0 + p / C::TW, x = x0 + p % C::TW;
        const unsigned pix = a.up_out == 2 ? unsigned(2 * y + a.sub_y) * unsigned(2 * W) + unsigned(2 * x + a.sub_x)
                                           : unsigned(y) * unsigned(W) + unsigned(x);
        const unsigned plane = a.up_out == 2 ? 4u * HW : HW;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int co = co0 + C::MT * 32 + 16 + v;
            if (co < a.cout && a.out)
                a.out[(size_t(b0) * a.out_ctot + a.out_coff + co) * plane + pix] = s4.acc[v] + (a.bias ? a.bias[co] : 0.f);
        }
    }

}

template <class C, bool AMAX, bool IN2 = false>
__global__ __launch_bounds__(256, C::MIN_BLOCKS_PER_CU) void conv_mfma_kernel(const ConvArgs a_in, const int tiles_x, const int tiles_y,
                                                           const int cout_tiles) {
    conv_tile<C, AMAX, IN2>(a_in, tiles_x, tiles_y, cout_tiles, int(blockIdx.x), int(gridDim.x));
}

// Two independent convolutions in ONE grid (same tile configuration; e.g. conv j of a hourglass level's skip block and
// conv j of the block that starts the next lower level - paulsenpredictor.py:301-361, up1 = rb(x) beside low1 =
// rb(pool(x))): workgroups [0, nblk[0]) belong to problem 0, [nblk0_pad, gridDim.x) to problem 1 (nblk0_pad = nblk[0] rounded
// up to a multiple of 8, so that blockIdx & 7 is the XCD in both ranges; the workgroups between exit).  A latency-bound
// launch of a small level then rides in the tail of the larger one without any cross-queue dependency, and the pair pays
// one grid fill and drain instead of two.  Results are those of the two separate launches with this variant, bit for bit.
struct ConvPairArgs {
    ConvArgs a[2];
    int tiles_x[2], tiles_y[2], cout_tiles[2], nblk[2];
    int nblk0_pad;
};

template <class C>
__global__ __launch_bounds__(256, C::MIN_BLOCKS_PER_CU) void conv_pair_kernel(const ConvPairArgs p) {
    const int bid = int(blockIdx.x);
    const int which = bid >= p.nblk0_pad ? 1 : 0;
    if (!which && bid >= p.nblk[0]) return;
    conv_tile<C, false>(p.a[which], p.tiles_x[which], p.tiles_y[which], p.cout_tiles[which], which ? bid - p.nblk0_pad : bid,
                        p.nblk[which]);
}

// ---- launchers -------------------------------------------------------------------------
struct ConvGrid {
    int tiles_x = 0, tiles_y = 0, cout_tiles = 0;
    long tiles = 0;  // output tiles (x parities); the grid has tiles * kparts workgroups
    long nblk = 0;
};

// host-side checks of one problem against a variant's tile geometry; fills the grid
template <class C>
int check_variant(mvlm_ctx* ctx, ConvArgs& a, ConvGrid& g) {
    const int tiles_x = a.W / C::TW, tiles_y = a.H / C::TRI;
    const int tiles_b = (a.B + C::NIMG - 1) / C::NIMG;
    const int cout_tiles = a.cout_pad / C::COUT_T;
    MVLM_REQUIRE(ctx, a.ksize == C::KS, "conv: kernel variant built for another kernel size");
    MVLM_REQUIRE(ctx, !a.in2 || (C::HAS_IN2 && !a.up_in && !a.amax_val && a.in_coff == 0 && a.in2_ctot >= a.cin && !(a.H & 1) && !(a.W & 1) && a.kparts <= 1),
                 "conv: a second input tensor (upsample + skip on the load) is served by the 128-channel 8x32 tile only");
    MVLM_REQUIRE(ctx, !C::WINO || (!a.up_in && !a.in2 && !a.amax_val && a.up_out != 2 && a.n_par == 1 && a.kparts <= 1),
                 "conv: the Winograd tiles serve plain, pooling and scattering 3x3 layers (no upsampled / second input, no fused argmax, no K parts)");
    MVLM_REQUIRE(ctx, !C::WINO4 || (!a.up_in && !a.in2 && !a.amax_val && a.up_out != 2 && a.n_par == 1 && a.kparts <= 1),
                 "conv: the F(4,3) Winograd tile serves plain, pooling and scattering 3x3 layers (no upsampled / second input, no fused argmax, no K parts)");
    MVLM_REQUIRE(ctx, a.W % C::TW == 0 && a.H % C::TRI == 0, "conv: spatial size not a multiple of the tile");
    MVLM_REQUIRE(ctx, !C::SPLITK || a.cin_pad % 32 == 0, "conv: split-K tiles need 32-channel chunks");
    MVLM_REQUIRE(ctx, !(C::SPLITK && C::NT > 1) || (a.kparts <= 1 && !a.amax_val), "conv: the two-column split-K tiles have no K-parts / argmax form");
    MVLM_REQUIRE(ctx, a.cout_pad % C::COUT_T == 0, "conv: cout_pad not a multiple of the cout tile");
    MVLM_REQUIRE(ctx, a.cin_pad % C::CK == 0, "conv: cin_pad must be a multiple of the K-chunk");
    MVLM_REQUIRE(ctx, !a.pre_scale || a.cin_pad <= C::BN_MAXC, "conv: pre-activation BatchNorm supports up to 256 input channels");
    MVLM_REQUIRE(ctx, !C::WINO || a.cin_pad <= C::BN_MAXC, "conv: the Winograd tiles keep a BatchNorm pair of every input channel in LDS, with or without pre-activation (up to 256)");
    MVLM_REQUIRE(ctx, !C::WINO4 || a.cin_pad <= C::BN_MAXC, "conv: the F(4,3) Winograd tile keeps a BatchNorm pair of every input channel in LDS, with or without pre-activation (up to 256)");
    if (C::TAIL4) MVLM_REQUIRE(ctx, a.up_out != 1 && (a.out || (a.amax_val && C::HAS_AMAX)), "conv: the 84-channel tile writes a plain (or parity) output tensor or argmax partials");
    if (C::TAIL16)
        MVLM_REQUIRE(ctx, !a.res1 && !a.res2 && !a.out_raw && !a.post_scale && a.up_out != 1 && !a.pool_out,
                     "conv: the 80-channel tiles serve plain conv + bias layers only");
    if (a.amax_val) {
        MVLM_REQUIRE(ctx, C::NIMG == 1, "conv: fused argmax needs one image per tile");
        MVLM_REQUIRE(ctx, a.amax_part0 >= 0 && a.amax_part0 + tiles_x * tiles_y * 4 <= a.amax_parts,
                     "conv: argmax partial range mismatch");
        MVLM_REQUIRE(ctx, !a.res1 && !a.post_scale && a.up_out != 1, "conv: fused argmax expects a plain conv + bias layer");
        MVLM_REQUIRE(ctx, !a.out && !a.out_raw && !a.pool_out, "conv: a fused-argmax launch does not materialise the heatmap");
    }
    long nblk = long(tiles_x) * tiles_y * tiles_b * cout_tiles;
    if (a.n_par != 1) {
        MVLM_REQUIRE(ctx, a.n_par == 4 && C::KS == 2 && a.up_out == 2, "conv: four parities per launch are a 2x2-kernel feature");
        MVLM_REQUIRE(ctx, a.w_par[0] && a.w_par[1] && a.w_par[2] && a.w_par[3], "conv: parity weights missing");
        MVLM_REQUIRE(ctx, !a.amax_val || (a.amax_par_stride >= tiles_x * tiles_y * 4 &&
                                          a.amax_part0 + 3 * a.amax_par_stride + tiles_x * tiles_y * 4 <= a.amax_parts),
                     "conv: argmax partial range mismatch (four parities)");
        nblk *= 4;
    }
    MVLM_REQUIRE(ctx, nblk > 0 && nblk < (1l << 31), "conv: bad grid");
    a.kparts = a.kparts > 1 ? a.kparts : 1;
    g.tiles = nblk;
    if (a.kparts > 1) {
        MVLM_REQUIRE(ctx, C::SPLITK, "conv: only the split-K tiles divide the input channels over workgroups");
        MVLM_REQUIRE(ctx, a.cin_pad % (a.kparts * C::CK) == 0, "conv: input channels do not divide into the requested K parts");
        nblk *= a.kparts;
    }
    MVLM_REQUIRE(ctx, nblk < (1l << 31), "conv: bad grid");
    g.tiles_x = tiles_x;
    g.tiles_y = tiles_y;
    g.cout_tiles = cout_tiles;
    g.nblk = nblk;
    return 0;
}

// dynamic-LDS limit of this variant's kernels: set once per context, i.e. per device (hipFuncSetAttribute
// applies to the current device's copy of the function; the ctx mutex held by every entry point guards the mask)
// attr_bit: the variant's bit of mvlm_ctx::conv_attr_mask (a base id, MVLM_CONV_WINO4_ATTR_BIT)
template <class C>
int set_variant_attributes(mvlm_ctx* ctx, int attr_bit) {
    if ((ctx->conv_attr_mask >> attr_bit) & 1ull) return 0;
    MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, false>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    if constexpr (C::HAS_AMAX)
        MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    if constexpr (C::PAIRABLE)
        MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_pair_kernel<C>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    if constexpr (C::HAS_IN2)
        MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, false, true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    ctx->conv_attr_mask |= 1ull << attr_bit;
    return 0;
}

template <class C>
int launch_variant(mvlm_ctx* ctx, const ConvArgs& a_in, int attr_bit) {
    ConvArgs a = a_in;
#if defined(MVLM_CONV_TIMING)  // diagnostic build: the tool passes its counter buffer through the environment
    if (const char* e = getenv("MVLM_CONV_TIMING_BUF")) a.timing = reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0));
#endif
    ConvGrid g;
    if (check_variant<C>(ctx, a, g)) return 1;
    if (a.kparts > 1) {
        MVLM_REQUIRE(ctx, g.tiles <= MVLM_KPARTS_MAX_TILES && g.nblk <= MVLM_KPARTS_MAX_PARTS, "conv: too many tiles for the K-part workspace");
        if (mvlm_conv_kparts_workspace(ctx, &a.kws, &a.kcnt)) return 1;
    }
    if (set_variant_attributes<C>(ctx, attr_bit)) return 1;
#if defined(MVLM_CONV_TIMING)  // diagnostic build: MVLM_CONV_TIMING_WINO4_LDS = dynamic LDS bytes an F(4,3) launch asks for at least.
    // More than half of a CU's 160 KiB leaves one workgroup per CU: the K loop's rate without a partner on the matrix pipe.
    if constexpr (C::WINO4) {
        if (const char* e = getenv("MVLM_CONV_TIMING_WINO4_LDS")) {
            const size_t lds = strtoull(e, nullptr, 0);
            if (lds > size_t(C::LDS_BYTES) && !a.amax_val && !a.in2) {
                MVLM_REQUIRE(ctx, lds <= 160 * 1024, "conv: MVLM_CONV_TIMING_WINO4_LDS beyond a CU's LDS");
                MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, false>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
                hipLaunchKernelGGL((conv_mfma_kernel<C, false>), dim3((unsigned)g.nblk), dim3(256), lds, ctx->cur_stream(), a,
                                   g.tiles_x, g.tiles_y, g.cout_tiles);
                MVLM_CHECK_HIP(ctx, hipGetLastError());
                return 0;
            }
        }
    }
#endif
    if (a.amax_val) {
        if constexpr (C::HAS_AMAX) {
            hipLaunchKernelGGL((conv_mfma_kernel<C, true>), dim3((unsigned)g.nblk), dim3(256), C::LDS_BYTES, ctx->cur_stream(),
                               a, g.tiles_x, g.tiles_y, g.cout_tiles);
        } else {
            return ctx->fail("conv: fused argmax is only built for the 8x32-pixel tile variants");
        }
    } else if (a.in2) {
        if constexpr (C::HAS_IN2) {
            hipLaunchKernelGGL((conv_mfma_kernel<C, false, true>), dim3((unsigned)g.nblk), dim3(256), C::LDS_BYTES, ctx->cur_stream(), a,
                               g.tiles_x, g.tiles_y, g.cout_tiles);
        } else {
            return ctx->fail("conv: this kernel variant has no second-input form");
        }
    } else {
        hipLaunchKernelGGL((conv_mfma_kernel<C, false>), dim3((unsigned)g.nblk), dim3(256), C::LDS_BYTES, ctx->cur_stream(), a,
                           g.tiles_x, g.tiles_y, g.cout_tiles);
    }
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

// two independent convolutions on this variant's tiles in one grid (conv_pair_kernel); kparts of each problem in its ConvArgs
template <class C>
int launch_variant_pair(mvlm_ctx* ctx, const ConvArgs& a0, const ConvArgs& a1, int attr_bit) {
    if constexpr (!C::PAIRABLE) {
        return ctx->fail("conv: this kernel variant has no two-problem form");
    } else {
        ConvPairArgs p;
        p.a[0] = a0;
        p.a[1] = a1;
        ConvGrid g[2];
        for (int i = 0; i < 2; ++i) {
            ConvArgs& a = p.a[i];
            MVLM_REQUIRE(ctx, !a.amax_val && a.n_par == 1 && !a.timing && !a.in2, "conv: a paired launch takes plain convolutions");
            if (check_variant<C>(ctx, a, g[i])) return 1;
        }
        if (p.a[0].kparts > 1 || p.a[1].kparts > 1) {
            // one workspace per launch stream: problem 1's partial tiles and counters follow problem 0's
            const long t0 = p.a[0].kparts > 1 ? g[0].tiles : 0, n0 = p.a[0].kparts > 1 ? g[0].nblk : 0;
            const long t1 = p.a[1].kparts > 1 ? g[1].tiles : 0, n1 = p.a[1].kparts > 1 ? g[1].nblk : 0;
            MVLM_REQUIRE(ctx, t0 + t1 <= MVLM_KPARTS_MAX_TILES && n0 + n1 <= MVLM_KPARTS_MAX_PARTS, "conv: too many tiles for the K-part workspace");
            float* kws = nullptr;
            unsigned* kcnt = nullptr;
            if (mvlm_conv_kparts_workspace(ctx, &kws, &kcnt)) return 1;
            p.a[0].kws = kws;
            p.a[0].kcnt = kcnt;
            p.a[1].kws = kws + size_t(n0) * 1024;
            p.a[1].kcnt = kcnt + t0;
        }
        for (int i = 0; i < 2; ++i) {
            p.tiles_x[i] = g[i].tiles_x;
            p.tiles_y[i] = g[i].tiles_y;
            p.cout_tiles[i] = g[i].cout_tiles;
            p.nblk[i] = int(g[i].nblk);
        }
        p.nblk0_pad = (p.nblk[0] + 7) / 8 * 8;
        const long total = long(p.nblk0_pad) + p.nblk[1];
        MVLM_REQUIRE(ctx, total < (1l << 31), "conv: bad grid");
        if (set_variant_attributes<C>(ctx, attr_bit)) return 1;
        hipLaunchKernelGGL((conv_pair_kernel<C>), dim3((unsigned)total), dim3(256), C::LDS_BYTES, ctx->cur_stream(), p);
        MVLM_CHECK_HIP(ctx, hipGetLastError());
        return 0;
    }
}


}  // namespace
#endif
