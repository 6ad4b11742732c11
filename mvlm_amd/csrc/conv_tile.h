// The workgroup program conv_tile and its two kernels (conv_kernel.h lists the headers of the convolution kernel).
// conv_tile stays ONE long function on purpose: moving statements out of it changes the machine code (registers, instruction
// order) - see CHANGELOG, "Two comparison tools for kernel refactors" and "conv_kernel.h cut into six headers".
#ifndef MVLM_CONV_TILE_H
#define MVLM_CONV_TILE_H
#include <type_traits>

#include "conv_loop.h"
#include "conv_wino.h"
#include "conv_wino4.h"

namespace {

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

}  // namespace
#endif
