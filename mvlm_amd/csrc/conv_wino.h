// The F(2,3) Winograd tiles' K loop (conv_kernel.h lists the headers of the convolution kernel).
#ifndef MVLM_CONV_WINO_H
#define MVLM_CONV_WINO_H
#include "conv_loop.h"

namespace {

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

}  // namespace
#endif
