// Host side of a convolution layer's weights: the [tap][cin_pad][cout_pad] layout, its Winograd forms and the padding rule of
// the single-layer entry points (conv_pack.cpp).  Plain C++, no HIP: tests/test_conv_pack_cpu.py builds it with g++ -fsanitize.
#pragma once
#include <cstddef>
#include <vector>

// The two Winograd forms of a 3x3 layer's weights (common.h: WinoForm says what the dispatcher and the executor know of a form).
enum { MVLM_WINO_F23 = 0, MVLM_WINO_F43 = 1, MVLM_WINO_FORMS_N = 2 };

// The cout stride of the padded F(4,3) weights (common.h: ConvWino4Pad): whole 32-channel columns of the tile.  84 -> 96, 80 -> 96.
inline int mvlm_conv_wino4_padded_cout(int cout_pad) { return (cout_pad + 31) / 32 * 32; }

// packed [9][cin_pad][cout_pad] -> [12][cin_pad][cout_pad] (u_t per kx: t * 3 + kx), float64 arithmetic, one rounding
void mvlm_winograd_transform(const float* w9, int cin_pad, int cout_pad, float* w12);
// packed [9][cin_pad][cout_pad] -> [18][cin_pad][cout_pad] (u_t per kx: t * 3 + kx), float64 arithmetic, one rounding
void mvlm_winograd4_transform(const float* w9, int cin_pad, int cout_pad, float* w18);
// packed [9][cin_pad][cout_pad] -> [18][cin_pad][P], columns below cout_pad as mvlm_winograd4_transform, zeros beyond;
// bias [cout_pad] or null -> [P] likewise (bias_pad may be null then)
void mvlm_winograd4_pack_padded(const float* w9, const float* bias, int cin_pad, int cout_pad, float* w18_pad, float* bias_pad);

// OIHW [cout][cin][ksize][ksize] -> [tap][cin_pad][cout_pad] in `out`, which the caller has zeroed (the padding stays zero)
void mvlm_conv_pack_transpose(const float* w_oihw, int cout, int cin, int ksize, int cin_pad, int cout_pad, float* out);

// The forms of one layer beside its direct weights: the two Winograd forms, and the F(4,3) form at the cout stride
// mvlm_conv_wino4_padded_cout with the bias padded alike.  Which of them a layer gets is the caller's to say (WinoForm::serves_slot,
// mvlm_conv_wino4_pad_serves_slot), so this unit knows nothing of the variant table: it names the host blob each form is appended
// to, null for a form that is not made.  One blob for all (a single-layer hook) or one per form (mvlm_cnn_load, whose device
// buffers are per form).
struct ConvPackTargets {
    std::vector<float>* wino[MVLM_WINO_FORMS_N] = {nullptr, nullptr};
    std::vector<float>* wino4_pad = nullptr;  // the padded bias follows the weights in it
};
// where they went: float offsets into their blobs, -1 absent (wino4_pad_bias: also where the layer has no bias)
struct ConvPackOffsets {
    long wino[MVLM_WINO_FORMS_N] = {-1, -1};
    long wino4_pad = -1, wino4_pad_bias = -1;
};
// the floats each occupies, the direct weights first (a 1x1 layer has no other form: zeros)
struct ConvPackSizes {
    size_t w = 0, wino[MVLM_WINO_FORMS_N] = {0, 0}, wino4_pad = 0, wino4_pad_bias = 0;
};
ConvPackSizes mvlm_conv_pack_sizes(int ksize, int cin_pad, int cout_pad);

// Appends the forms of the packed weights w9 (and bias, [cout_pad] or null) that `to` names a blob for, every one at a multiple of
// four floats (16 bytes, as the packed layer's own sub-arrays).  w9 and bias may lie in such a blob when the caller has reserved
// the room (mvlm_conv_pack_sizes): that blob must not move while it grows.
ConvPackOffsets mvlm_conv_pack_forms(const ConvPackTargets& to, const float* w9, const float* bias, int cin_pad, int cout_pad);

// The zero arena the two timing hooks put every form of the weights in: all forms begin at its start, so it is as long as the
// longest of them.
size_t mvlm_conv_pack_arena_floats(int ksize, int cin_pad, int cout_pad);

// ---- the channel padding of the single-layer entry points -------------------------------------------------------------------
// What mvlm_amd/weights.py decides by a slot's name, the hooks decide by what the call carries.  cin_pad: whole 8s for a 1x1
// layer, whole 4s otherwise.  cout_pad: 80 where the layer may end in one 16-row strip and its channels round to 80, 84 where it
// may end in a 16- and a 4-row strip and has exactly 84 channels, whole 32s otherwise.  A layer is plain when it has no pre- and
// no post-BatchNorm and no residual.  The sites differ, and keep their differences:
//   mvlm_conv2d          the strip: a plain 3x3 layer of 32-pixel rows (w >= 32, h % 8 == 0), with or without a bias, its input
//                        upsampled or not; exactly 84: the same with a bias and an input that is not upsampled
//   mvlm_conv_bench      the strip: a plain layer with a bias, of either kernel size and any size; exactly 84: the same, 3x3 only
//   the two pair hooks   whole 32s always (3x3 residual-block layers)
enum ConvHookSite { MVLM_HOOK_CONV2D, MVLM_HOOK_CONV_BENCH, MVLM_HOOK_PAIR };
struct ConvHookLayer {
    int ksize, cin, cout;
    bool bias = false, pre = false, post = false, residual = false, upsample_in = false;
    int w = 0, h = 0;
};
struct ConvPadding {
    int cin_pad, cout_pad;
};
ConvPadding mvlm_conv_hook_padding(ConvHookSite site, const ConvHookLayer& l);
