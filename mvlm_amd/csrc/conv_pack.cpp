// A convolution layer's weights on the host (conv_pack.h): layout, Winograd forms, the hooks' padding rule.  No device code.
//
// Winograd weights.  The large stride-1 3x3 layers also run as F(2,3) and F(4,3) Winograd along y (conv_wino.h, conv_wino4.h): the
// kernels multiply row-transformed inputs by weights transformed here, once, when a layer is loaded or a hook packs one.  Both
// transforms take each filter column g0, g1, g2 (ky = 0, 1, 2) of every (kx, cin, cout) in float64 from the fp32 weights and round
// once; slice t * 3 + kx of the result is u_t at kx, and padded channels stay zero.  Built with -ffp-contract=off: a fused
// multiply-add would round the sums differently.
#include "conv_pack.h"

#include <algorithm>
#include <cassert>
#include <functional>

#include "../../include/mvlm_hip.h"

// u0 = g0, u1 = (g0 + g1 + g2) / 2, u2 = (g0 - g1 + g2) / 2, u3 = g2
void mvlm_winograd_transform(const float* w9, int cin_pad, int cout_pad, float* w12) {
    const size_t n = size_t(cin_pad) * cout_pad;
    for (int kx = 0; kx < 3; ++kx)
        for (size_t i = 0; i < n; ++i) {
            const double g0 = w9[size_t(kx) * n + i], g1 = w9[size_t(3 + kx) * n + i], g2 = w9[size_t(6 + kx) * n + i];
            w12[size_t(kx) * n + i] = float(g0);
            w12[size_t(3 + kx) * n + i] = float((g0 + g1 + g2) * 0.5);
            w12[size_t(6 + kx) * n + i] = float((g0 - g1 + g2) * 0.5);
            w12[size_t(9 + kx) * n + i] = float(g2);
        }
}

// The F(4,3) form on the points 0, 1, -1, 2, -1/2, inf: u0 = g0, u1 = -(g0 + g1 + g2) / 3, u2 = (g0 - g1 + g2) / 3,
// u3 = (g0 + 2 g1 + 4 g2) / 15, u4 = (-16 g0 + 8 g1 - 4 g2) / 15, u5 = g2
void mvlm_winograd4_transform(const float* w9, int cin_pad, int cout_pad, float* w18) {
    const size_t n = size_t(cin_pad) * cout_pad;
    for (int kx = 0; kx < 3; ++kx)
        for (size_t i = 0; i < n; ++i) {
            const double g0 = w9[size_t(kx) * n + i], g1 = w9[size_t(3 + kx) * n + i], g2 = w9[size_t(6 + kx) * n + i];
            w18[size_t(kx) * n + i] = float(g0);
            w18[size_t(3 + kx) * n + i] = float(0.0 - (g0 + g1 + g2) / 3.0);  // (0 - x: a padded channel stays +0)
            w18[size_t(6 + kx) * n + i] = float((g0 - g1 + g2) / 3.0);
            w18[size_t(9 + kx) * n + i] = float((g0 + 2.0 * g1 + 4.0 * g2) / 15.0);
            w18[size_t(12 + kx) * n + i] = float((-16.0 * g0 + 8.0 * g1 - 4.0 * g2) / 15.0);
            w18[size_t(15 + kx) * n + i] = float(g2);
        }
}

// The same values at the cout stride P = mvlm_conv_wino4_padded_cout(cout_pad): the transform at its own stride, then every row of
// cout_pad columns moved to the front of a row of P, zeros behind; the bias likewise.
void mvlm_winograd4_pack_padded(const float* w9, const float* bias, int cin_pad, int cout_pad, float* w18_pad, float* bias_pad) {
    const int P = mvlm_conv_wino4_padded_cout(cout_pad);
    const size_t rows = size_t(18) * cin_pad;
    std::vector<float> w18(rows * cout_pad);
    mvlm_winograd4_transform(w9, cin_pad, cout_pad, w18.data());
    for (size_t r = 0; r < rows; ++r) {
        std::copy(w18.begin() + r * cout_pad, w18.begin() + (r + 1) * cout_pad, w18_pad + r * P);
        std::fill(w18_pad + r * P + cout_pad, w18_pad + (r + 1) * P, 0.f);
    }
    if (bias && bias_pad) {
        std::copy(bias, bias + cout_pad, bias_pad);
        std::fill(bias_pad + cout_pad, bias_pad + P, 0.f);
    }
}

extern "C" int mvlm_pack_winograd_weights(const float* w9_host, int cin_pad, int cout_pad, float* w12_host) {
    if (!w9_host || !w12_host || cin_pad <= 0 || cout_pad <= 0) return 1;
    mvlm_winograd_transform(w9_host, cin_pad, cout_pad, w12_host);
    return 0;
}

extern "C" int mvlm_pack_winograd4_weights(const float* w9_host, int cin_pad, int cout_pad, float* w18_host) {
    if (!w9_host || !w18_host || cin_pad <= 0 || cout_pad <= 0) return 1;
    mvlm_winograd4_transform(w9_host, cin_pad, cout_pad, w18_host);
    return 0;
}

extern "C" int mvlm_conv_wino4_padded_stride(int cout_pad) { return cout_pad > 0 ? mvlm_conv_wino4_padded_cout(cout_pad) : 0; }

extern "C" int mvlm_pack_winograd4_weights_padded(const float* w9_host, const float* bias_host, int cin_pad, int cout_pad, float* w18_pad_host,
                                                  float* bias_pad_host) {
    if (!w9_host || !w18_pad_host || cin_pad <= 0 || cout_pad <= 0 || (bias_host && !bias_pad_host)) return 1;
    mvlm_winograd4_pack_padded(w9_host, bias_host, cin_pad, cout_pad, w18_pad_host, bias_pad_host);
    return 0;
}

void mvlm_conv_pack_transpose(const float* w_oihw, int cout, int cin, int ksize, int cin_pad, int cout_pad, float* out) {
    const int taps = ksize * ksize;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) out[(size_t(t) * cin_pad + ci) * cout_pad + co] = w_oihw[(size_t(co) * cin + ci) * taps + t];
}

ConvPackSizes mvlm_conv_pack_sizes(int ksize, int cin_pad, int cout_pad) {
    const size_t n = size_t(cin_pad) * cout_pad;
    ConvPackSizes s;
    s.w = size_t(ksize) * ksize * n;
    if (ksize != 3) return s;
    s.wino[MVLM_WINO_F23] = 12 * n;
    s.wino[MVLM_WINO_F43] = 18 * n;
    s.wino4_pad_bias = size_t(mvlm_conv_wino4_padded_cout(cout_pad));
    s.wino4_pad = size_t(18) * cin_pad * s.wino4_pad_bias;
    return s;
}

ConvPackOffsets mvlm_conv_pack_forms(const ConvPackTargets& to, const float* w9, const float* bias, int cin_pad, int cout_pad) {
    const ConvPackSizes sizes = mvlm_conv_pack_sizes(3, cin_pad, cout_pad);
    const std::less<const float*> before;
    auto push = [&](std::vector<float>* blob, size_t n) -> long {
        if (!blob) return -1;
        const float* const was = blob->data();
        const bool holds_w9 = !blob->empty() && !before(w9, was) && before(w9, was + blob->size());
        const size_t off = (blob->size() + 3) / 4 * 4;
        blob->resize(off + n, 0.f);
        assert((!holds_w9 || blob->data() == was) && "sources inside a blob: the caller reserves the room, so it does not move");
        (void)holds_w9;
        return long(off);
    };
    ConvPackOffsets o;
    for (int f = 0; f < MVLM_WINO_FORMS_N; ++f) o.wino[f] = push(to.wino[f], sizes.wino[f]);
    o.wino4_pad = push(to.wino4_pad, sizes.wino4_pad);
    if (o.wino4_pad >= 0 && bias) o.wino4_pad_bias = push(to.wino4_pad, sizes.wino4_pad_bias);
    if (o.wino[MVLM_WINO_F23] >= 0) mvlm_winograd_transform(w9, cin_pad, cout_pad, to.wino[MVLM_WINO_F23]->data() + o.wino[MVLM_WINO_F23]);
    if (o.wino[MVLM_WINO_F43] >= 0) mvlm_winograd4_transform(w9, cin_pad, cout_pad, to.wino[MVLM_WINO_F43]->data() + o.wino[MVLM_WINO_F43]);
    if (o.wino4_pad >= 0)
        mvlm_winograd4_pack_padded(w9, bias, cin_pad, cout_pad, to.wino4_pad->data() + o.wino4_pad, o.wino4_pad_bias < 0 ? nullptr : to.wino4_pad->data() + o.wino4_pad_bias);
    return o;
}

size_t mvlm_conv_pack_arena_floats(int ksize, int cin_pad, int cout_pad) {
    const ConvPackSizes s = mvlm_conv_pack_sizes(ksize, cin_pad, cout_pad);
    const size_t longest = std::max({s.w, s.wino[MVLM_WINO_F23], s.wino[MVLM_WINO_F43], s.wino4_pad});
    // (and never shorter than the bound this replaced, the direct weights at the padded stride: longer for a 1x1 layer on 80 columns only)
    return std::max(longest, size_t(ksize) * ksize * cin_pad * mvlm_conv_wino4_padded_cout(cout_pad));
}

ConvPadding mvlm_conv_hook_padding(ConvHookSite site, const ConvHookLayer& l) {
    const bool plain = !l.pre && !l.post && !l.residual, rows32 = l.w >= 32 && l.h % 8 == 0;
    bool strip16 = false, exact84 = false;
    switch (site) {
    case MVLM_HOOK_CONV2D:
        strip16 = l.ksize == 3 && plain && rows32;
        exact84 = strip16 && l.bias && !l.upsample_in;
        break;
    case MVLM_HOOK_CONV_BENCH:
        strip16 = plain && l.bias;
        exact84 = strip16 && l.ksize == 3;
        break;
    case MVLM_HOOK_PAIR: break;
    }
    const int cout16 = (l.cout + 15) / 16 * 16;
    return {l.ksize == 1 ? (l.cin + 7) / 8 * 8 : (l.cin + 3) / 4 * 4,
            strip16 && cout16 == 80 ? 80 : exact84 && l.cout == 84 ? 84 : (l.cout + 31) / 32 * 32};
}
