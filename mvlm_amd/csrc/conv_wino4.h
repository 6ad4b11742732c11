// The F(4,3) Winograd tiles' K loop with its gap plan (conv_kernel.h lists the headers of the convolution kernel).
// conv_wino.h: wino_opaque, and the notes at WinoStage that the staging below refers to.
#ifndef MVLM_CONV_WINO4_H
#define MVLM_CONV_WINO4_H
#include "conv_wino.h"

namespace {

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

}  // namespace
#endif
