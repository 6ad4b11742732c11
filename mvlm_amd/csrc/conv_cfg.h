// Tile geometry of the implicit-GEMM convolution: Cfg<> and nothing else.  Pure constexpr arithmetic - no HIP header, no
// vector type, no device code - so the dispatcher (conv_mfma.hip) and host-only tests take it without parsing a kernel.
#ifndef MVLM_CONV_CFG_H
#define MVLM_CONV_CFG_H
#include <cstddef>

namespace {

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
// tiles" in conv_wino4.h for the transforms and the fixed order of their sums).
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

}  // namespace
#endif
