// Implicit-GEMM 3x3 / 1x1 convolution on the CDNA4 matrix cores, exact fp32.
//
// This is the kernel the landmark network (reference: MVLMModel,
// src/mvlm/prediction/paulsenpredictor.py:364-432) spends ~99 % of its time in.
//
// Mapping (gfx950, wave64):
//   GEMM  D[cout][pixel] = sum_k W[cout][k] * X[k][pixel],   k = (tap, cin)
//   v_mfma_f32_32x32x2_f32: A = weights (lane l: cout = l&31, k = l>>5),
//                           B = activations (lane l: pixel = l&31, k = l>>5),
//   so an accumulator register holds 32 consecutive pixels of one output channel per
//   half-wave -> 128-byte coalesced stores into planar NCHW tensors.
//   The MFMA is a k-ordered fp32 fma chain (bit-exact fp32, no reduced precision), which
//   is what the 1e-3 landmark parity bound needs.
//
//   A workgroup (4 waves) owns COUT_T output channels x PIX_T pixels.  Per K-chunk of 8
//   input channels it stages into LDS
//     sX [8][NIMG][TRI+2][TW+2]  the haloed input tile, with the consumer's BatchNorm+ReLU
//                                (pre-activation blocks, paulsenpredictor.py:269-271)
//                                applied on the way in and the zero padding inserted
//                                AFTER the activation, optionally read through a nearest
//                                2x upsample (paulsenpredictor.py:428-429),
//     sW [taps][8][COUT_T]       the weight slice (host-packed [tap][cin][cout]),
//   then issues taps*4 k-steps of MT x NT MFMAs straight out of LDS (conflict-free:
//   32 consecutive floats per half-wave for both operands).
//   Several workgroups are resident per CU (<= 48 KB LDS, <= 168 VGPRs), so one group's
//   staging overlaps another's MFMA stream.
//
//   The epilogue fuses bias, post-BatchNorm+ReLU, the residual-block concat/add
//   (paulsenpredictor.py:273), the hourglass "upsample + skip add" (:334-359) as a 2x2
//   scatter, and for the last layer the per-(view, landmark) argmax
//   (paulsenpredictor.py:123) so the [N,NL,256,256] heatmaps never reach HBM.
//
//   The large stride-1 3x3 layers also exist as F(2,3) Winograd along y (conv_cfg.h: Cfg::WINO, variants conv3x3w_*):
//   row pairs of transformed inputs x load-time-transformed weights, four GEMMs over K = (kx, cin), 4 MFMAs per output pair
//   where the direct form spends 6 - same instruction, fp32 in and out.  mvlm_conv_wino_variant() routes a launch there where
//   the measured table conv_tuned_wino.h says it is faster (mvlm_cnn_set_winograd / MVLM_WINOGRAD: 0 never, 1 table, 2 always).
//   A profile record of such a launch counts the FLOPs its MFMAs execute (12 Cin Cout H W B, not 18).
//   The F(4,3) form along y (Cfg::WINO4, conv3x3q_c32_t16x32) likewise: six GEMMs per four output rows, 9 Cin Cout H W B.  What the
//   two forms differ in for the dispatcher (which channels a tile serves, which ConvArgs member carries the weights) is
//   mvlm_wino_form() below; the weights themselves are made by conv_pack.cpp.
//
// How a launch finds its kernel.  Every variant of conv_variants.h, the F(4,3) tile included, has one row in VARIANTS below
// (tile geometry, features, Winograd form, launchers); tile_fits() is the one statement of "this tile divides this layer", and
// decode_variant() the one reading of a variant code (the F(4,3) tile's own code 2048; base id + 256 log2(K parts) below 1024).
// A launch is looked up by its ConvKey (ksize, cin_pad, cout_pad, size, kind, batch), in this order:
//   1. a tuning override of the context for the key's shape and kind (mvlm_conv_set_override),
//   2. the Winograd routing (mvlm_conv_wino_variant: the F(4,3) tile before the F(2,3) tiles, each by its mode - 0 never, 2 wherever
//      it can serve, 1 its measured table conv_tuned_wino4.h / conv_tuned_wino.h),
//   3. the in-network table conv_tuned_net.h, 4. the single-layer table conv_tuned.h - both by the entry of the smallest
//      tuned batch >= the launch's, 5. the rules (pick_variant_rules).
// Launches with a fused argmax, an upsampled input or a parity output and the 2x2 layers go straight to the rules: one
// kernel can serve them.
//   6. With the variant code in hand, however it was chosen, f43_plan() decides how the launch runs on the F(4,3) tile: code 2048 on
//      the tile's wide workgroup shape (conv_inst_q1.hip) or its 32 x 16 shape (conv_inst_q0.hip), and a launch of the 80- or 84-row
//      direct tile on the 32 x 16 shape over weights padded to whole 32-channel columns.  The launchers only launch.
// Every decision is pinned by tests/golden/conv_routing.txt and, for launches that carry the F(4,3) weights,
// tests/golden/conv_routing_wino4.txt; step 6 by tests/golden/conv_routing_f43.txt (tests/test_conv_routing_cpu.py).
#include <algorithm>
#include <array>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "common.h"
#include "conv_cfg.h"      // Cfg<> (tile geometry) for the variant table below; kernels are not instantiated here
#include "conv_variants.h"
#include "conv_tuned.h"
#include "conv_tuned_net.h"
#include "conv_pair_tuned.h"
#include "conv_tuned_wino.h"
#include "conv_tuned_wino4.h"
#include "conv_wino4_wide_hold.h"
#include "conv_tuned_wino4_pad.h"

// one launcher per variant, defined in conv_inst_g*.hip
#define X(id, name, ...)                                         \
    int mvlm_conv_launch_##id(mvlm_ctx* ctx, const ConvArgs& a); \
    int mvlm_conv_pair_launch_##id(mvlm_ctx* ctx, const ConvArgs& a0, const ConvArgs& a1);
MVLM_CONV_VARIANTS(X)
#undef X
// the F(4,3) tile's two workgroup shapes: 32 x 16 (conv_inst_q0.hip) and wide (conv_inst_q1.hip)
int mvlm_conv_launch_wino4_narrow(mvlm_ctx* ctx, const ConvArgs& a);
int mvlm_conv_launch_wino4_wide(mvlm_ctx* ctx, const ConvArgs& a);

// ---- the two Winograd forms (common.h: WinoForm) ----------------------------------------------------------------------------
const WinoForm& mvlm_wino_form(int form) {
    static const WinoForm forms[MVLM_WINO_FORMS_N] = {
        {mvlm_conv_wino_serves_slot, &ConvArgs::w_wino, 6.0, "mvlm_pack_winograd_weights"},
        {mvlm_conv_wino4_serves_slot, &ConvArgs::w_wino4, 4.5, "mvlm_pack_winograd4_weights"},
    };
    return forms[form];
}

namespace {

// ---- the variant table ------------------------------------------------------------------------------------------------------
struct ConvVariantInfo {
    int id;  // a base id, or the F(4,3) tile's own code
    const char* name;
    int KS, TW, TRI, NIMG, COUT_T, CK, PIX_T, NT, BN_MAXC;
    int form;  // MVLM_WINO_F23 / MVLM_WINO_F43 (mvlm_wino_form), -1: a direct tile
    bool SPLITK, TAIL16, PAIRABLE, CAN_POOL_ANY, HAS_IN2;
    int (*launch)(mvlm_ctx*, const ConvArgs&);
    int (*launch_pair)(mvlm_ctx*, const ConvArgs&, const ConvArgs&);  // (null: the F(4,3) tile, which no pair code names)
};
constexpr int MAX_VARIANT_ID = 64;  // base ids live in the low byte of a variant code; the table is indexed by them

// A base id is also the variant's bit of mvlm_ctx::conv_attr_mask (common.h: the partition of its 64 bits).
template <int ID, class V>
constexpr ConvVariantInfo variant_info(const char* name, int (*launch)(mvlm_ctx*, const ConvArgs&),
                                       int (*launch_pair)(mvlm_ctx*, const ConvArgs&, const ConvArgs&)) {
    static_assert(ID == MVLM_CONV_VARIANT_WINO4 || (ID >= 0 && ID < MVLM_CONV_FAST_ATTR_BIT0 && ID != MVLM_CONV_WINO4_ATTR_BIT && ID != MVLM_CONV_WINO4_WIDE_ATTR_BIT),
                  "base ids are below the fast kernels' attribute bits and leave the F(4,3) tile's two free");
    static_assert((ID == MVLM_CONV_VARIANT_WINO4) == V::WINO4, "the F(4,3) tile has the code of its own, and nothing else has");
    return {ID, name, V::KS, V::TW, V::TRI, V::NIMG, V::COUT_T, V::CK, V::PIX_T, V::NT, V::BN_MAXC,
            V::WINO ? MVLM_WINO_F23 : V::WINO4 ? MVLM_WINO_F43 : -1, V::SPLITK, V::TAIL16, V::PAIRABLE, V::CAN_POOL_ANY, V::HAS_IN2, launch, launch_pair};
}

constexpr ConvVariantInfo VARIANTS[] = {
#define X(id, name, ...) variant_info<id, __VA_ARGS__>(name, mvlm_conv_launch_##id, mvlm_conv_pair_launch_##id),
    MVLM_CONV_VARIANTS(X)
#undef X
    variant_info<MVLM_CONV_VARIANT_WINO4, MVLM_CONV_WINO4_CFG>(MVLM_CONV_WINO4_NAME, mvlm_conv_launch_wino4_narrow, nullptr),  // (the last row; f43_plan chooses the shape)
};

// the row of this base id or of the F(4,3) tile's code, or null
const ConvVariantInfo* conv_variant(int id) {
    static const std::array<const ConvVariantInfo*, MAX_VARIANT_ID> by_id = [] {
        std::array<const ConvVariantInfo*, MAX_VARIANT_ID> t{};
        for (const ConvVariantInfo& v : VARIANTS)
            if (v.id < MAX_VARIANT_ID) t[size_t(v.id)] = &v;
        return t;
    }();
    if (id == MVLM_CONV_VARIANT_WINO4) return &VARIANTS[sizeof VARIANTS / sizeof VARIANTS[0] - 1];
    return id >= 0 && id < MAX_VARIANT_ID ? by_id[size_t(id)] : nullptr;
}

// What the variant code of a single launch names: 2048 the F(4,3) tile's row on one K part; a code below 1024 the row of its low
// byte (null: no such base id) on 1 << (code >> 8) K parts; any other code nothing (kparts 0).
struct VariantCode {
    const ConvVariantInfo* row;
    int kparts;
};
VariantCode decode_variant(int v) {
    if (v == MVLM_CONV_VARIANT_WINO4) return {conv_variant(v), 1};
    if (v >= 0 && v < 1024) return {conv_variant(v & 255), 1 << (v >> 8)};
    return {nullptr, 0};
}
// the row behind any code, a pair's and a garbled one included: they carry a base id in the low byte
const ConvVariantInfo* variant_row(int v) { return conv_variant(v == MVLM_CONV_VARIANT_WINO4 ? v : v & 255); }

// Does the tile divide this layer?  Every "can this variant serve ..." question is this plus the caller's own conditions.
// (check_variant<C> in conv_launch.h states the same once more at the launch, as the last line of defence.)
bool tile_fits(const ConvVariantInfo& t, int ksize, int cin_pad, int cout_pad, int H, int W) {
    return ksize == t.KS && W % t.TW == 0 && H % t.TRI == 0 && cout_pad % t.COUT_T == 0 && cin_pad % t.CK == 0 &&
           (!t.SPLITK || cin_pad % 32 == 0);
}

// ---- keys and measured tables -----------------------------------------------------------------------------------------------
// The entry of the smallest tuned batch >= `batch` among those whose leading fields `lead_of(entry)` (a tuple, in the
// table's sort order) equal `lead`, or null.  The tables are sorted by (leading fields, batch).
template <class E, class Lead, class LeadOf>
const E* tuned_entry(const E* table, int n, const Lead& lead, short batch, LeadOf lead_of) {
    const E* end = table + n;
    const E* it = std::lower_bound(table, end, std::make_pair(lead, batch),
                                   [&](const E& e, const std::pair<Lead, short>& key) { return std::make_pair(lead_of(e), e.batch) < key; });
    return it != end && lead_of(*it) == lead ? it : nullptr;
}

// the tuning override of this context for the key's shape and kind, or null
const ConvOverride* find_override(const mvlm_ctx* ctx, const ConvKey& k) {
    if (ctx)
        for (const ConvOverride& o : ctx->conv_overrides)
            if (o.ksize == k.ksize && o.cin_pad == k.cin_pad && o.cout_pad == k.cout_pad && o.size == k.size && o.kind == k.kind) return &o;
    return nullptr;
}

// level holds at most this many pixels in total -> latency-bound launch, split-K tiles
constexpr long SPLITK_MAX_PIXELS = 8192;

int pick_variant_rules(const ConvArgs& a) {
    if (a.ksize == 1) return (a.W >= 32 && a.cout_pad % 128 == 0) ? 4 : -1;
    if (a.ksize == 2) return (a.W >= 32 && a.H % 8 == 0) ? (a.cout_pad == 96 ? 11 : a.cout_pad == 80 ? 17 : a.cout_pad == 84 ? 29 : -1) : -1;
    if (a.cout_pad == 80) return (a.W >= 32 && a.H % 8 == 0) ? 16 : -1;  // 64 rows + one 16-row strip
    if (a.cout_pad % 32 == 20)  // 64 + 16 + 4 rows: plain layers writing a plain tensor (conv6 / conv10 of the 84-landmark net)
        return (a.cout_pad == 84 && a.W >= 32 && a.H % 8 == 0 && !a.amax_val && !a.up_out) ? 26 : -1;
    const long px = long(a.B) * a.H * a.W;
    // tiny feature maps / small batches: few pixels in total -> the split-K tiles (32 pixels per
    // workgroup, four waves share the K loop) shorten the serial chain; larger batches keep the
    // 128-pixel tiles
    const bool sk = a.cin_pad % 32 == 0 && px <= SPLITK_MAX_PIXELS && !a.amax_val;
    if (a.W == 32 && sk) return 15;
    if (a.W >= 32) {
        // two workgroups fit a CU: below ~512 workgroups the 128-pixel tiles fill the chip better
        if (a.cout_pad % 128 == 0) {
            const long blocks = px / 256 * (a.cout_pad / 128);
            return (blocks < 512 && !a.amax_val) ? 8 : 0;
        }
        if (a.cout_pad % 96 == 0) return 1;
        if (a.cout_pad % 64 == 0) {
            const long blocks = px / 256 * (a.cout_pad / 64);
            return blocks < 768 ? 9 : 10;
        }
        return (a.H % 16 == 0) ? 3 : -1;
    }
    if (a.W == 16) return sk ? 12 : (a.cin_pad % 16 == 0 ? 5 : -1);
    if (a.W == 8) return sk ? 13 : (a.cin_pad % 16 == 0 ? 6 : -1);
    if (a.W == 4) return sk ? 14 : (a.cin_pad % 16 == 0 ? 7 : -1);
    return -1;
}

// The direct tiles' choice: measured first, the rules otherwise.  Order: a tuning override of this context
// (tools/tune_in_network.py), the in-network table (conv_tuned_net.h: every layer kind timed INSIDE a forward pass on real
// activations - a launch whose tensors come from HBM behind other layers ranks the tiles differently from one that re-reads
// them out of the MALL), the single-layer table (conv_tuned.h: mvlm_conv_bench on idle data, plain layers only).  The fused
// argmax / upsampling launches have one kernel that can serve them.
int pick_variant(const mvlm_ctx* ctx, const ConvArgs& a, bool rules_only = false) {
    const int by_rule = pick_variant_rules(a);
    if (rules_only || a.amax_val || a.up_in || a.up_out == 2 || a.ksize == 2 || a.H != a.W) return by_rule;
    const ConvKey k = mvlm_conv_key(a);
    if (const ConvOverride* o = find_override(ctx, k)) return o->variant;
    const auto shape = std::make_tuple(k.ksize, k.cin_pad, k.cout_pad, k.size);
    if (const ConvTunedNet* e = tuned_entry(MVLM_CONV_TUNED_NET, MVLM_CONV_TUNED_NET_N, std::tuple_cat(shape, std::make_tuple(k.kind)), k.batch,
                                            [](const ConvTunedNet& e) { return std::make_tuple(e.ksize, e.cin_pad, e.cout_pad, e.size, e.kind); }))
        return e->variant;
    if (const ConvTuned* e = tuned_entry(MVLM_CONV_TUNED, MVLM_CONV_TUNED_N, shape, k.batch,
                                         [](const ConvTuned& e) { return std::make_tuple(e.ksize, e.cin_pad, e.cout_pad, e.size); }))
        return e->variant;
    return by_rule;
}

// The variant of this Winograd form that can serve this launch at all (shape and features), or -1.
int wino_candidate(const ConvArgs& a, int form) {
    if (a.ksize != 3 || a.up_in || a.in2 || a.amax_val || a.up_out == 2 || a.n_par != 1 || a.H != a.W) return -1;
    // (cin_pad <= BN_MAXC: the pre-BN parameters must fit the LDS; asked whether or not this layer has a pre-BN)
    for (const ConvVariantInfo& t : VARIANTS)
        if (t.form == form && tile_fits(t, a.ksize, a.cin_pad, a.cout_pad, a.H, a.W) && a.cin_pad <= t.BN_MAXC) return t.id;
    return -1;
}

// A slot has channels but no size yet: can a tile of this form serve it at the tile's own size?
bool form_serves_slot(int form, int ksize, int cin_pad, int cout_pad, bool bn_bound) {
    for (const ConvVariantInfo& t : VARIANTS)
        if (t.form == form && tile_fits(t, ksize, cin_pad, cout_pad, t.TRI, t.TW) && (!bn_bound || cin_pad <= t.BN_MAXC)) return true;
    return false;
}

// The row of a measured F(4,3) / Winograd table for this (shape, kind), or null: every such table begins {cin_pad, cout_pad, size,
// kind} and has one row per key.  What else a row says (min_batch, variant) is the caller's to apply.
template <class E>
const E* shape_kind_row(const E* table, int n, int cin_pad, int cout_pad, int size, int kind) {
    for (int i = 0; i < n; ++i)
        if (table[i].cin_pad == cin_pad && table[i].cout_pad == cout_pad && table[i].size == size && table[i].kind == kind) return &table[i];
    return nullptr;
}

// the variant a measured Winograd table ({..., min_batch, variant}) sends this key to, or -1
template <class E>
int wino_table_variant(const E* table, int n, const ConvKey& k) {
    const E* e = shape_kind_row(table, n, k.cin_pad, k.cout_pad, k.size, k.kind);
    return e && k.batch >= e->min_batch ? e->variant : -1;
}

// ---- how a launch runs on the F(4,3) tile -------------------------------------------------------------------------------------
// A pure function of the context's settings, the launch, its variant row and its K parts.
//   wide / narrow: the row is the F(4,3) tile's (code 2048: routed, overridden or forced).  Wide where the context's switch is on,
//     the output channels come in 64s and the (shape, kind) did not run slower that way inside the network (conv_wino4_wide_hold.h).
//   padded: the row is a 3x3 direct tile with a 16-row strip (the 80- and 84-row tiles: their cout_pad is no multiple of 32, so
//     tile_fits never sends such a layer to the F(4,3) tile) and the launch carries weights and bias padded to whole 32-channel
//     columns (ConvArgs::wino4_pad).  A plain 3x3 layer writing a plain tensor, not forced, no mode at 0, and padded mode 2 or a row
//     of conv_tuned_wino4_pad.h from its min_batch on: the kernel guards every store by cout, and the columns beyond cout_pad
//     multiply zeros.
enum class F43Plan { none, narrow, wide, padded };

F43Plan f43_plan(const mvlm_ctx* ctx, const ConvArgs& a, const ConvVariantInfo& t, int kparts) {
    const int kind = mvlm_conv_kind(a);
    if (t.form == MVLM_WINO_F43) {
        const bool wide = ctx->conv_winograd4_wide && mvlm_conv_wino4_wide_shape_ok(a.cout_pad, a.H) &&
                          !shape_kind_row(MVLM_CONV_WINO4_WIDE_HOLD, MVLM_CONV_WINO4_WIDE_HOLD_N, a.cin_pad, a.cout_pad, a.H, kind);
        return wide ? F43Plan::wide : F43Plan::narrow;
    }
    if (t.form >= 0 || !t.TAIL16 || t.KS != 3) return F43Plan::none;
    if (a.wino4_pad <= 0 || size_t(a.wino4_pad) > ctx->conv_wino4_pads.size()) return F43Plan::none;
    const ConvWino4Pad& pad = ctx->conv_wino4_pads[size_t(a.wino4_pad) - 1];
    if (!pad.w || (a.bias && !pad.bias)) return F43Plan::none;
    // a plain 3x3 layer writing a plain tensor, as the two direct tiles serve it
    if (a.ksize != 3 || a.up_in || a.in2 || a.amax_val || a.res1 || a.res2 || a.post_scale || a.out_raw || a.pool_out || a.up_out || !a.out || a.n_par != 1 ||
        kparts > 1 || a.H != a.W || a.H % 16 != 0 || a.cin_pad > 256)
        return F43Plan::none;
    if (ctx->conv_force_variant >= 0) return F43Plan::none;  // tools and tests force 16 / 26 to get the direct tile
    if (ctx->conv_winograd == 0 || ctx->conv_winograd4 == 0 || ctx->conv_winograd4_padded == 0) return F43Plan::none;
    if (ctx->conv_winograd4_padded == 2) return F43Plan::padded;
    const ConvTunedWino4Pad* e = shape_kind_row(MVLM_CONV_TUNED_WINO4_PAD, MVLM_CONV_TUNED_WINO4_PAD_N, a.cin_pad, a.cout_pad, a.H, kind);
    return e && a.B >= e->min_batch ? F43Plan::padded : F43Plan::none;
}

}  // namespace

ConvKey mvlm_conv_key(const ConvArgs& a) {
    return {short(a.ksize), short(a.cin_pad), short(a.cout_pad), short(a.H), short(mvlm_conv_kind(a)), short(a.B > 32767 ? 32767 : a.B)};
}

bool mvlm_conv_variant_is_wino(int v) {
    const ConvVariantInfo* t = conv_variant(v);
    return t && t->form == MVLM_WINO_F23;
}

bool mvlm_conv_variant_is_wino4(int v) {
    const ConvVariantInfo* t = conv_variant(v);
    return t && t->form == MVLM_WINO_F43;
}

bool mvlm_conv_wino4_serves_slot(int ksize, int cin_pad, int cout_pad) { return form_serves_slot(MVLM_WINO_F43, ksize, cin_pad, cout_pad, true); }

// No cin_pad <= BN_MAXC here (historical: a wider slot gets transformed weights that no launch is routed to).
bool mvlm_conv_wino_serves_slot(int ksize, int cin_pad, int cout_pad) { return form_serves_slot(MVLM_WINO_F23, ksize, cin_pad, cout_pad, false); }

// Winograd routing of the exact path, a pure function of (shape, kind, batch) and the context's settings: a tuning override
// that names a Winograd variant first; then mode 0 never, 2 wherever a variant can serve, 1 the measured table
// (conv_tuned_wino.h: the Winograd launch beat what runs otherwise from `min_batch` views per device batch on).
// The F(4,3) tile comes first, for a launch that carries its weights (ConvArgs::w_wino4) and while the Winograd mode is not 0:
// F(4,3) mode 2 wherever the tile can serve, mode 1 its own measured table (conv_tuned_wino4.h) - consulted in Winograd mode 1
// only, so that Winograd mode 2 stays "every layer on the F(2,3) tile" unless F(4,3) mode 2 asks otherwise.
int mvlm_conv_wino_variant(const mvlm_ctx* ctx, const ConvArgs& a) {
    const int cand = wino_candidate(a, MVLM_WINO_F23);
    const int cand4 = a.w_wino4 ? wino_candidate(a, MVLM_WINO_F43) : -1;
    if (cand < 0 && cand4 < 0) return -1;
    const ConvKey k = mvlm_conv_key(a);
    if (const ConvOverride* o = find_override(ctx, k))
        return ((cand >= 0 && mvlm_conv_variant_is_wino(o->variant)) || (cand4 >= 0 && mvlm_conv_variant_is_wino4(o->variant))) ? o->variant : -1;
    const int mode = ctx ? ctx->conv_winograd : 1;
    if (mode == 0) return -1;
    const int mode4 = ctx ? ctx->conv_winograd4 : 1;
    if (cand4 >= 0 && mode4 == 2) return cand4;
    if (cand4 >= 0 && mode4 == 1 && mode == 1) {
        const int v = wino_table_variant(MVLM_CONV_TUNED_WINO4, MVLM_CONV_TUNED_WINO4_N, k);
        if (v >= 0) return v;
    }
    if (cand < 0) return -1;
    return mode == 2 ? cand : wino_table_variant(MVLM_CONV_TUNED_WINO, MVLM_CONV_TUNED_WINO_N, k);
}

// the variant a launch runs on: the Winograd routing first, the direct tiles' tables and rules otherwise
static int route_variant(const mvlm_ctx* ctx, const ConvArgs& a) {
    const int w = mvlm_conv_wino_variant(ctx, a);
    return w >= 0 ? w : pick_variant(ctx, a);
}

// Variant ids >= 256 are a split-K variant (low byte) whose input channels are divided over 2 / 4 / 8 workgroups per
// output tile (id = base + 256 log2(parts)); the partial tiles meet in a per-context workspace (one per launch stream).
int mvlm_conv_kparts_workspace(mvlm_ctx* ctx, float** ws, unsigned** cnt) {
    const int which = (ctx->launch_stream && ctx->launch_stream == ctx->cnn.side_stream) ? 1 : 0;
    if (!ctx->kparts_ws[0]) {  // both at once, outside any stream capture (a key's first pass is launch by launch)
        for (int i = 0; i < 2; ++i) {
            MVLM_CHECK_HIP(ctx, hipMalloc(&ctx->kparts_ws[i], size_t(MVLM_KPARTS_MAX_PARTS) * 1024 * sizeof(float)));
            MVLM_CHECK_HIP(ctx, hipMalloc(&ctx->kparts_cnt[i], size_t(MVLM_KPARTS_MAX_TILES) * sizeof(unsigned)));
            MVLM_CHECK_HIP(ctx, hipMemset(ctx->kparts_cnt[i], 0, size_t(MVLM_KPARTS_MAX_TILES) * sizeof(unsigned)));
        }
    }
    *ws = ctx->kparts_ws[which];
    *cnt = ctx->kparts_cnt[which];
    return 0;
}

const char* mvlm_conv_variant_name_impl(int v) {
    if (const ConvVariantInfo* t = conv_variant(v)) return t->name;
    if (v == MVLM_CONV_VARIANT_FAST) return "conv3x3_bf16x3_t8x32";
    if (v == MVLM_CONV_VARIANT_FAST16) return "conv3x3_f16x2_t8x32";
    if (v >= 256) {
        // "<split-K variant>_k<parts>" and "<variant>_pair[_k<parts0>k<parts1>]": built on first use, kept for the process
        static std::mutex mu;
        static std::map<int, std::string> names;
        std::lock_guard<std::mutex> lk(mu);
        auto it = names.find(v);
        if (it == names.end()) {
            std::string n = mvlm_conv_variant_name_impl(v & 255);
            if (v & MVLM_CONV_PAIR_FLAG) {
                n += "_pair";
                const int l0 = (v >> 8) & 3, l1 = (v >> 10) & 3;
                if (l0 || l1) n += "_k" + std::to_string(1 << l0) + "k" + std::to_string(1 << l1);
            } else {
                n += "_k" + std::to_string(1 << ((v >> 8) & 3));
            }
            it = names.emplace(v, n).first;
        }
        return it->second.c_str();
    }
    return "?";
}

// Would the dispatcher run this layer on the tile that can add a second, half-resolution input tensor on its load
// (ConvArgs::in2: the hourglass's "upsample x 2 + skip" on the consumer's side)?  The measured choice is respected: only where
// that tile is what the tables / rules pick anyway.
bool mvlm_conv_in2_ok(const mvlm_ctx* ctx, const ConvArgs& a) {
    if (a.ksize != 3 || a.up_in || a.up_out || a.amax_val || a.in_coff != 0 || (a.H & 1) || a.H != a.W) return false;
    if (ctx && ctx->conv_force_variant != -1) return false;
    return route_variant(ctx, a) == 0;  // (the one variant with HAS_IN2; a Winograd tile has no second-input form)
}

int mvlm_conv_kind(const ConvArgs& a) { return a.up_out == 1 ? 1 : ((a.pool_out || a.pool_hint) ? 2 : 0); }

bool mvlm_conv_can_pool(const mvlm_ctx* ctx, const ConvArgs& a_in) {
    if (a_in.up_out || a_in.amax_val || (a_in.H & 1) || (a_in.W & 1)) return false;
    ConvArgs a = a_in;
    a.pool_hint = 1;
    return mvlm_conv_variant_can_pool((ctx && ctx->conv_force_variant >= 0) ? ctx->conv_force_variant : route_variant(ctx, a));
}

bool mvlm_conv_variant_can_pool(int v) {
    const ConvVariantInfo* t = variant_row(v);
    return t && t->CAN_POOL_ANY;
}

namespace {
// can variant `v` (base id) serve this problem, and does it exist as a two-problem kernel?
// (no cin_pad <= BN_MAXC: the launch checks it where the layer has a pre-BN, as for every direct tile)
bool pair_variant_serves(int v, const ConvArgs& a) {
    const ConvVariantInfo* t = conv_variant(v);
    return t && t->PAIRABLE && tile_fits(*t, a.ksize, a.cin_pad, a.cout_pad, a.H, a.W);
}
}  // namespace

// Should these two independent convolutions share a launch, and on which tiles?  Returns the pair's variant code
// (MVLM_CONV_PAIR_FLAG | base id | log2(kparts of problem 0) << 8 | log2(kparts of problem 1) << 10) or -1 (two launches).
//   mode 1: the measured table (conv_pair_tuned.h, tools/tune_conv_pairs.py: pairs that beat the two tuned single launches)
//   mode 2: always, on the tiles the dispatcher would give problem 0 when they can serve both (tests, tuning)
int mvlm_conv_pair_variant(const ConvArgs& a0, const ConvArgs& a1, int mode) {
    if (mode <= 0) return -1;
    for (const ConvArgs* a : {&a0, &a1})
        if (a->ksize != 3 || a->amax_val || a->up_in || a->up_out == 2 || a->n_par != 1 || a->H != a->W) return -1;
    if (a0.B != a1.B) return -1;
    if (mode == 2) {
        for (int cand : {pick_variant(nullptr, a0), pick_variant(nullptr, a1), pick_variant_rules(a0), pick_variant_rules(a1)}) {
            if (cand < 0) continue;
            const int base = cand & 255, lg = cand >> 8;
            if (pair_variant_serves(base, a0) && pair_variant_serves(base, a1)) return base | (lg << 8) | (lg << 10) | MVLM_CONV_PAIR_FLAG;
        }
        return -1;
    }
    if (a0.cin_pad != a1.cin_pad || a0.cout_pad != a1.cout_pad || a0.H != 2 * a1.H) return -1;
    const ConvKey k = mvlm_conv_key(a0);
    const ConvPairTuned* e = tuned_entry(MVLM_CONV_PAIR_TUNED, MVLM_CONV_PAIR_TUNED_N, std::make_tuple(k.cin_pad, k.cout_pad, k.size), k.batch,
                                         [](const ConvPairTuned& e) { return std::make_tuple(e.cin_pad, e.cout_pad, e.size); });
    if (!e || e->variant < 0) return -1;
    const int v = e->variant;
    if (!pair_variant_serves(v & 255, a0) || !pair_variant_serves(v & 255, a1)) return -1;
    // The table was measured without the pool kernel that follows a block whose tiles cannot emit the pooled tensor.  Since
    // round 5 every pairable tile but the one-row split-K tiles (t1x32) pools in its epilogue; for those, keep the pair only
    // if the single launch could not pool either (then the pool kernel runs in both forms and the comparison stands).
    for (const ConvArgs* a : {&a0, &a1})
        if (a->pool_hint && !mvlm_conv_variant_can_pool(v) && mvlm_conv_can_pool(nullptr, *a)) return -1;
    return v | MVLM_CONV_PAIR_FLAG;
}

int mvlm_launch_conv_pair(mvlm_ctx* ctx, const ConvArgs& a0, const ConvArgs& a1, int pair_variant) {
    MVLM_REQUIRE(ctx, pair_variant >= 0 && (pair_variant & MVLM_CONV_PAIR_FLAG) && pair_variant < 2 * MVLM_CONV_PAIR_FLAG, "conv: not a pair variant");
    ConvArgs b[2] = {a0, a1};
    for (int i = 0; i < 2; ++i) {
        const ConvArgs& a = b[i];
        MVLM_REQUIRE(ctx, a.in && a.w && a.B > 0 && a.H > 0 && a.W > 0 && a.H == a.W, "conv: null input / weights or bad shape");
        MVLM_REQUIRE(ctx, !a.up_in && a.up_out != 2 && (a.up_out != 1 || a.skip), "conv: a paired launch takes plain or scattering 3x3 convolutions");
        const double px = double(a.B) * a.H * a.W, lim = 4294967295.0;
        MVLM_REQUIRE(ctx, px * a.in_ctot < lim && (!a.out_raw || px * a.raw_ctot < lim) && (!a.res1 || px * a.res1_ctot < lim) &&
                              (!a.res2 || px * a.res2_ctot < lim) && (!a.out || px * a.out_ctot * (a.up_out ? 4 : 1) < lim) &&
                              (a.up_out != 1 || px * a.skip_ctot * 4 < lim) && (!a.pool_out || px / 4 * a.pool_ctot < lim),
                     "conv: a tensor exceeds 32-bit element offsets (lower the batch)");
        MVLM_REQUIRE(ctx, a.out || a.pool_out, "conv: no output requested");
        MVLM_REQUIRE(ctx, !a.pool_out || (mvlm_conv_variant_can_pool(pair_variant) && !(a.H & 1) && !a.up_out), "conv: this pair's kernel variant cannot emit the pooled tensor");
    }
    b[0].kparts = 1 << ((pair_variant >> 8) & 3);
    b[1].kparts = 1 << ((pair_variant >> 10) & 3);
    const ConvVariantInfo* t = conv_variant(pair_variant & 255);
    return t ? t->launch_pair(ctx, b[0], b[1]) : ctx->fail("conv: unreachable variant");
}

int mvlm_conv_amax_parts(int H, int W) {
    // fused argmax is only built for the 8x32-pixel tiles (4 waves x one partial each)
    return (W / 32) * (H / 8) * 4;
}

int mvlm_launch_conv(mvlm_ctx* ctx, const ConvArgs& a, int* variant_out) {
    MVLM_REQUIRE(ctx, a.in && a.w && a.B > 0 && a.H > 0 && a.W > 0, "conv: null input / weights or empty shape");
    MVLM_REQUIRE(ctx, a.H == a.W, "conv: square feature maps only");
    MVLM_REQUIRE(ctx, !a.up_in || (a.H % 2 == 0), "conv: upsampled input needs even size");
    MVLM_REQUIRE(ctx, a.up_out != 1 || a.skip, "conv: up_out needs a skip tensor");
    MVLM_REQUIRE(ctx, a.ksize != 2 || ((a.sub_y | a.sub_x) & ~1) == 0, "conv: 2x2 window offset must be 0 or 1");
    // (a failed check's message ends in the source text of its condition, so these stay spelled out here and in the pair launch)
    const double px = double(a.B) * a.H * a.W, lim = 4294967295.0;
    MVLM_REQUIRE(ctx, px * a.in_ctot < lim, "conv: input tensor exceeds 32-bit element offsets (lower the batch)");
    MVLM_REQUIRE(ctx, !a.out_raw || px * a.raw_ctot < lim, "conv: raw output exceeds 32-bit element offsets");
    MVLM_REQUIRE(ctx, !a.res1 || px * a.res1_ctot < lim, "conv: residual exceeds 32-bit element offsets");
    MVLM_REQUIRE(ctx, !a.res2 || px * a.res2_ctot < lim, "conv: residual exceeds 32-bit element offsets");
    MVLM_REQUIRE(ctx, !a.out || px * a.out_ctot * (a.up_out ? 4 : 1) < lim, "conv: output exceeds 32-bit element offsets");
    MVLM_REQUIRE(ctx, a.up_out != 1 || px * a.skip_ctot * 4 < lim, "conv: skip tensor exceeds 32-bit element offsets");
    // conv_force_variant (mvlm_conv_bench only): >= 0 that variant, -2 the rules without the tuned table
    const int v = ctx->conv_force_variant >= 0 ? ctx->conv_force_variant
                  : ctx->conv_force_variant == -2 ? pick_variant(ctx, a, true) : route_variant(ctx, a);
    MVLM_REQUIRE(ctx, v >= 0, "conv: no kernel variant for this shape");
    const VariantCode d = decode_variant(v);
    const WinoForm* form = d.row && d.row->form >= 0 ? &mvlm_wino_form(d.row->form) : nullptr;  // the row says which weights the launch gets
    MVLM_REQUIRE(ctx, !form || a.*form->weights, std::string("conv: a Winograd tile needs the layer's transformed weights (") + form->pack_fn + ")");
    MVLM_REQUIRE(ctx, !a.in2 || v == 0, "conv: a second input tensor needs the 128-channel 8x32 tile (ask mvlm_conv_in2_ok first)");
    MVLM_REQUIRE(ctx, !a.in2 || px / 4 * a.in2_ctot < lim, "conv: second input exceeds 32-bit element offsets");
    MVLM_REQUIRE(ctx, !a.pool_out || mvlm_conv_variant_can_pool(v), "conv: this shape's kernel variant cannot emit the pooled tensor");
    MVLM_REQUIRE(ctx, !a.pool_out || px / 4 * a.pool_ctot < lim, "conv: pooled output exceeds 32-bit element offsets");
    MVLM_REQUIRE(ctx, !form || !a.amax_val || a.out || a.pool_out, "conv: a Winograd tile has no fused argmax, and no other output is requested");
    MVLM_REQUIRE(ctx, a.out || a.pool_out || a.amax_val, "conv: no output requested");
    if (variant_out) *variant_out = v;
    MVLM_REQUIRE(ctx, d.kparts > 0, "conv: unknown kernel variant");
    ConvArgs b = a;
    b.kparts = d.kparts;
    if (form) b.w = a.*form->weights;
    if (!d.row) return ctx->fail("conv: unreachable variant");
    // (check_variant<> at the launch refuses what the tile cannot serve)
    switch (f43_plan(ctx, a, *d.row, d.kparts)) {
    case F43Plan::wide:
        if (mvlm_conv_launch_wino4_wide(ctx, b)) return 1;
        ++ctx->conv_wino4_wide_launches;
        return 0;
    case F43Plan::padded: {
        const ConvWino4Pad& pad = ctx->conv_wino4_pads[size_t(a.wino4_pad) - 1];
        b.w = pad.w;
        b.bias = a.bias ? pad.bias : nullptr;
        b.cout_pad = mvlm_conv_wino4_padded_cout(a.cout_pad);  // (cout stays: the epilogue stores no channel beyond it)
        if (mvlm_conv_launch_wino4_narrow(ctx, b)) return 1;
        ++ctx->conv_wino4_padded_launches;
        if (variant_out) *variant_out = MVLM_CONV_VARIANT_WINO4;  // a profile record counts the FLOPs of the kernel that ran
        return 0;
    }
    default: return d.row->launch(ctx, b);  // (narrow: the F(4,3) row's own launcher)
    }
}

// ---- tuning hooks (tools/tune_in_network.py) --------------------------------------------------------------------------------
// can kernel variant `variant` (>= 256: a split-K variant with its input channels over 2 / 4 workgroups) run a 3x3 layer of
// this shape and kind?  (kind 2: a tile that cannot pool in its epilogue is followed by the pool kernel; the 80- / 84-row tiles
// serve conv6 / conv10 only)
extern "C" int mvlm_conv_variant_serves(int variant, int ksize, int cin_pad, int cout_pad, int size, int kind) {
    const VariantCode d = decode_variant(variant);
    const ConvVariantInfo* t = d.row;
    if (!t || ksize != 3 || kind < 0 || kind > 2 || !tile_fits(*t, ksize, cin_pad, cout_pad, size, size)) return 0;
    const int parts = d.kparts;
    const bool residual_block_tile = !t->TAIL16 && t->COUT_T != 96;                // (the 80-, 84- and 96-row tiles serve the last layers only)
    const bool bn_fits = t->form < 0 || cin_pad <= t->BN_MAXC;                      // (as wino_candidate; the direct tiles check it at the launch)
    const bool parts_ok = parts == 1 || (t->SPLITK && t->PIX_T == 32 && cin_pad % (parts * t->CK) == 0);
    return residual_block_tile && bn_fits && parts_ok;
}

// Would a launch of this shape on the F(4,3) tile (code 2048) take the wide workgroup shape while the context's switch is on?
// A pure query: what the tile serves at all, and output channels in 64s (common.h: mvlm_conv_wino4_wide_shape_ok).
extern "C" int mvlm_conv_wino4_wide_serves(int ksize, int cin_pad, int cout_pad, int size) {
    return mvlm_conv_variant_serves(MVLM_CONV_VARIANT_WINO4, ksize, cin_pad, cout_pad, size, 0) && mvlm_conv_wino4_wide_shape_ok(cout_pad, size);
}

// kernel variant for every launch of this (shape, kind) on this context, ahead of all tables; variant < 0 removes the
// entry, ksize == 0 removes all.  Captured launch graphs are dropped (they encode the kernels).
extern "C" int mvlm_conv_set_override(mvlm_ctx* ctx, int ksize, int cin_pad, int cout_pad, int size, int kind, int variant) {
    MVLM_ENTER(ctx);
    auto& ov = ctx->conv_overrides;
    if (ksize == 0) {
        ov.clear();
    } else {
        const ConvKey k = {short(ksize), short(cin_pad), short(cout_pad), short(size), short(kind), 0};
        // (an argument beyond the entries' 16-bit fields matches none of them)
        const bool fits = k.ksize == ksize && k.cin_pad == cin_pad && k.cout_pad == cout_pad && k.size == size && k.kind == kind;
        while (const ConvOverride* o = fits ? find_override(ctx, k) : nullptr) ov.erase(ov.begin() + (o - ov.data()));
        if (variant >= 0) {
            MVLM_REQUIRE(ctx, mvlm_conv_variant_serves(variant, ksize, cin_pad, cout_pad, size, kind), "conv_set_override: the variant cannot serve this shape");
            ov.push_back({k.ksize, k.cin_pad, k.cout_pad, k.size, k.kind, variant});
        }
    }
    ctx->cnn.drop_graphs();
    return 0;
}
