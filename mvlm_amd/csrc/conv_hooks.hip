// The single-layer entry points of the convolution: the test hooks mvlm_conv2d / mvlm_conv2d_pair and the tuning hooks
// mvlm_conv_bench / mvlm_conv_pair_bench.  Each pads a layer by the one rule of conv_pack.h (mvlm_conv_hook_padding), lays its
// weights out with conv_pack.cpp - every form the dispatcher may route it to - and hands the dispatcher a ConvArgs; this unit knows
// neither the tile geometry nor a kernel.
#include <algorithm>

#include "common.h"
#include "conv_pack.h"

namespace {

// where a layer's arrays lie from one device base pointer, in floats (-1: absent)
struct LayerOffsets {
    long w = 0, bias = -1, pre_scale = -1, pre_shift = -1, post_scale = -1, post_shift = -1;
    ConvPackOffsets forms;
};

struct LayerDims {
    int batch, cin, cin_pad, cout, cout_pad, ksize, h, w;
};

// the forms of the weights the dispatcher may ask for on these channels, all of them into `blob`
ConvPackTargets forms_served(int ksize, int cin_pad, int cout_pad, std::vector<float>* blob) {
    ConvPackTargets to;
    for (int f = 0; f < MVLM_WINO_FORMS_N; ++f) to.wino[f] = mvlm_wino_form(f).serves_slot(ksize, cin_pad, cout_pad) ? blob : nullptr;
    to.wino4_pad = mvlm_conv_wino4_pad_serves_slot(ksize, cin_pad, cout_pad) ? blob : nullptr;
    return to;
}

// The launch of a layer whose channel counts are its tensors' own: weights, vectors and shape; the caller adds the tensors.
ConvArgs layer_args(const float* base, const LayerOffsets& o, const LayerDims& d) {
    auto at = [&](long off) { return off < 0 ? nullptr : base + off; };
    ConvArgs a;
    a.in_ctot = a.cin = d.cin;
    a.cin_pad = d.cin_pad;
    a.B = d.batch;
    a.H = d.h;
    a.W = d.w;
    a.w = at(o.w);
    for (int f = 0; f < MVLM_WINO_FORMS_N; ++f) a.*mvlm_wino_form(f).weights = at(o.forms.wino[f]);
    a.wino4_pad = o.forms.wino4_pad < 0 ? 0 : 1;  // (the single-layer entry of mvlm_ctx::conv_wino4_pads: wino4_pad_entry)
    a.cout = a.out_ctot = d.cout;
    a.cout_pad = d.cout_pad;
    a.ksize = d.ksize;
    a.bias = at(o.bias);
    a.pre_scale = at(o.pre_scale);
    a.pre_shift = at(o.pre_shift);
    a.post_scale = at(o.post_scale);
    a.post_shift = at(o.post_shift);
    return a;
}

// the launch's tensors: input and output, residual and raw copy (null: none) - the last three [B][cout][H][W]
void set_tensors(ConvArgs& a, const float* in, const float* res, float* raw, float* out) {
    a.in = in;
    a.out = out;
    a.res1 = res;
    a.out_raw = raw;
    if (res) a.res1_ctot = a.cout;
    if (raw) a.raw_ctot = a.cout;
}

// mvlm_ctx::conv_wino4_pads[0] for the call in flight (null: this layer has no padded form)
ConvWino4Pad wino4_pad_entry(const float* base, const ConvPackOffsets& o) {
    return {o.wino4_pad < 0 ? nullptr : base + o.wino4_pad, o.wino4_pad_bias < 0 ? nullptr : base + o.wino4_pad_bias};
}

// One warm-up launch (it also sets the launch attributes; `first` receives what it reports), then `iters` launches between two
// events on the context's stream.
template <class Launch>
int timed_launches(mvlm_ctx* ctx, const std::string& who, int iters, Launch launch, int* first, float* ms_per_launch) {
    int rc = launch(first);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = ctx->fail(who + ": hipEventCreate failed");
    if (!rc) {
        hipEventRecord(e0, ctx->stream);
        for (int i = 0; i < iters && !rc; ++i) rc = launch(nullptr);
        hipEventRecord(e1, ctx->stream);
        if (!rc && hipEventSynchronize(e1) != hipSuccess) rc = ctx->fail(who + ": kernel failed");
        float ms = 0.f;
        if (!rc) hipEventElapsedTime(&ms, e0, e1);
        *ms_per_launch = ms / iters;
    }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    return rc;
}

size_t round4(size_t n) { return (n + 3) / 4 * 4; }

}  // namespace

// test / tuning hook: the next mvlm_conv2d calls on this ctx use exactly this kernel variant (-1: the dispatcher's choice)
extern "C" int mvlm_conv_force_variant(mvlm_ctx* ctx, int variant) {
    MVLM_ENTER(ctx);
    ctx->conv_force_variant = variant < 0 ? -1 : variant;
    return 0;
}

// ---- single convolution (test hook): packs the weights like mvlm_amd/weights.py does -------
extern "C" int mvlm_conv2d(mvlm_ctx* ctx, const float* x_dev, int batch, int cin, int h, int w, const float* w_host,
                           int cout, int ksize, const float* bias_host, const float* pre_scale_host,
                           const float* pre_shift_host, const float* post_scale_host, const float* post_shift_host,
                           const float* r_dev, int upsample_in, float* y_dev) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, x_dev && w_host && y_dev, "conv2d: null pointer");
    MVLM_REQUIRE(ctx, ksize == 1 || ksize == 3, "conv2d: kernel size must be 1 or 3");
    MVLM_REQUIRE(ctx, (pre_scale_host == nullptr) == (pre_shift_host == nullptr), "conv2d: pre scale/shift come in pairs");
    MVLM_REQUIRE(ctx, (post_scale_host == nullptr) == (post_shift_host == nullptr), "conv2d: post scale/shift come in pairs");
    const ConvPadding pad = mvlm_conv_hook_padding(
        MVLM_HOOK_CONV2D, {ksize, cin, cout, bias_host != nullptr, pre_scale_host != nullptr, post_scale_host != nullptr, r_dev != nullptr, upsample_in != 0, w, h});
    const int cin_pad = pad.cin_pad, cout_pad = pad.cout_pad;
    // the layer as weights.py packs it, then the Winograd forms beside it where such a tile could be chosen or forced and the
    // padded F(4,3) form where the dispatcher may run the 80- or 84-row tile's launch on that tile (room for all of it first: the
    // forms are made from weights in the blob)
    const ConvPackSizes sizes = mvlm_conv_pack_sizes(ksize, cin_pad, cout_pad);
    std::vector<float> blob;
    blob.reserve(round4(sizes.w) + round4(sizes.wino[0]) + round4(sizes.wino[1]) + round4(sizes.wino4_pad) + round4(sizes.wino4_pad_bias) +
                 2 * round4(size_t(cin_pad)) + 3 * round4(size_t(cout_pad)));
    auto push = [&](size_t n) {
        const size_t off = blob.size();
        blob.resize(off + round4(n), 0.f);
        return long(off);
    };
    auto vec = [&](const float* src, int n, int n_pad) -> long {
        if (!src) return -1;
        const long off = push(size_t(n_pad));
        std::copy(src, src + n, blob.begin() + off);
        return off;
    };
    LayerOffsets o;
    o.w = push(sizes.w);
    mvlm_conv_pack_transpose(w_host, cout, cin, ksize, cin_pad, cout_pad, blob.data() + o.w);
    o.bias = vec(bias_host, cout, cout_pad);
    o.pre_scale = vec(pre_scale_host, cin, cin_pad);
    o.pre_shift = vec(pre_shift_host, cin, cin_pad);
    o.post_scale = vec(post_scale_host, cout, cout_pad);
    o.post_shift = vec(post_shift_host, cout, cout_pad);
    o.forms = mvlm_conv_pack_forms(forms_served(ksize, cin_pad, cout_pad, &blob), blob.data() + o.w, o.bias < 0 ? nullptr : blob.data() + o.bias, cin_pad, cout_pad);
    auto* d = static_cast<float*>(ctx->get_scratch("conv2d.blob", blob.size() * 4));
    MVLM_REQUIRE(ctx, d, "conv2d: scratch allocation failed");
    MVLM_CHECK_HIP(ctx, hipMemcpy(d, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    ConvArgs a = layer_args(d, o, {batch, cin, cin_pad, cout, cout_pad, ksize, h, w});
    set_tensors(a, x_dev, r_dev, nullptr, y_dev);
    a.up_in = upsample_in;
    ctx->conv_wino4_pads[0] = wino4_pad_entry(d, o.forms);
    if (mvlm_launch_conv(ctx, a, nullptr)) return 1;
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- kernel-variant timing (tools/tune_conv.py): one layer shape, dummy data, a forced variant ----------
// Times `iters` launches of one convolution with HIP events on the ctx stream.  flags: 1 = pre-BN+ReLU on the
// input, 2 = residual add + raw copy (a residual block's conv1 / conv2), 4 = bias, 8 = post-BN+ReLU.
// variant -1: the dispatcher's own choice, -2: its rules without the tuned table (returned in *variant_used).
// Shapes a variant cannot serve fail.
extern "C" int mvlm_conv_bench(mvlm_ctx* ctx, int batch, int cin, int cout, int ksize, int size, int flags, int variant,
                               int iters, float* ms_per_launch, int* variant_used) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, batch > 0 && cin > 0 && cout > 0 && size > 0 && iters > 0 && ms_per_launch, "conv_bench: bad arguments");
    MVLM_REQUIRE(ctx, ksize == 1 || ksize == 3, "conv_bench: kernel size must be 1 or 3");
    const ConvPadding pad = mvlm_conv_hook_padding(
        MVLM_HOOK_CONV_BENCH, {ksize, cin, cout, (flags & 4) != 0, (flags & 1) != 0, (flags & 8) != 0, (flags & 2) != 0, false, size, size});
    const int cin_pad = pad.cin_pad, cout_pad = pad.cout_pad;
    const size_t px = size_t(batch) * size * size;
    // zero data serves every form of the weights (the transformed weights are zeros too): they all begin at the arena's start
    const size_t n_w = mvlm_conv_pack_arena_floats(ksize, cin_pad, cout_pad), n_vec = size_t(cin_pad) * 2 + size_t(cout_pad) * 3;
    const size_t n_x = px * cin, n_y = px * cout;
    const size_t total = n_w + n_vec + n_x + 3 * n_y + 64;
    auto* base = static_cast<float*>(ctx->get_scratch("conv_bench", total * sizeof(float)));
    MVLM_REQUIRE(ctx, base, "conv_bench: scratch allocation failed");
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(base, 0, total * sizeof(float), ctx->stream));
    const long vec = long(n_w);  // pre scale, pre shift [cin_pad], bias, post scale, post shift [cout_pad]
    float* x = base + vec + round4(n_vec);
    float* y = x + round4(n_x);
    float* raw = y + round4(n_y);
    float* res = raw + round4(n_y);
    std::vector<float> none;
    const ConvPackTargets which = forms_served(ksize, cin_pad, cout_pad, &none);  // (asked only which forms; nothing is packed)
    LayerOffsets o;
    for (int f = 0; f < MVLM_WINO_FORMS_N; ++f) o.forms.wino[f] = which.wino[f] ? 0 : -1;
    if (which.wino4_pad) {
        o.forms.wino4_pad = 0;
        o.forms.wino4_pad_bias = vec + 2 * cin_pad;  // (the zero bias: cout_pad floats, the two post vectors behind them)
    }
    if (flags & 1) {
        o.pre_scale = vec;
        o.pre_shift = vec + cin_pad;
    }
    if (flags & 4) o.bias = vec + 2 * cin_pad;
    if (flags & 8) {
        o.post_scale = vec + 2 * cin_pad + cout_pad;
        o.post_shift = vec + 2 * cin_pad + 2 * cout_pad;
    }
    ConvArgs a = layer_args(base, o, {batch, cin, cin_pad, cout, cout_pad, ksize, size, size});
    ctx->conv_wino4_pads[0] = wino4_pad_entry(base, o.forms);
    set_tensors(a, x, (flags & 2) ? res : nullptr, (flags & 2) ? raw : nullptr, y);
    const int saved = ctx->conv_force_variant;
    ctx->conv_force_variant = variant >= 0 ? variant : (variant == -2 ? -2 : -1);
    int used = -1;
    unsigned short* wq = nullptr;
    // the opt-in split kernels on zero weights: 62 bf16x3, 61 f16x2
    const int splits = variant == MVLM_CONV_VARIANT_FAST ? 3 : (variant == MVLM_CONV_VARIANT_FAST16 ? 2 : 0);
    if (splits) {
        a.cin_pad = (cin + 15) / 16 * 16;
        a.cout_pad = mvlm_fast_cout_pad(cout);
        const size_t n16 = size_t(a.cin_pad / 16) * 9 * 2 * splits * a.cout_pad * 8;
        wq = static_cast<unsigned short*>(ctx->get_scratch("conv_bench.wq", n16 * 2));
        if (!wq || !mvlm_conv_fast_ok(a, splits)) {
            ctx->conv_force_variant = saved;
            return ctx->fail("conv_bench: shape not eligible for the fast kernel");
        }
        (void)hipMemsetAsync(wq, 0, n16 * 2, ctx->stream);
    }
    auto launch = [&](int* v) { return wq ? mvlm_launch_conv_fast(ctx, a, wq, splits, 1.f) : mvlm_launch_conv(ctx, a, v); };
    const int rc = timed_launches(ctx, "conv_bench", iters, launch, &used, ms_per_launch);
    ctx->conv_force_variant = saved;
    if (variant_used) *variant_used = used;
    return rc;
}

// ---- two independent 3x3 convolutions in one launch (test hook for conv_pair_kernel) -----------------------------------
// Problem i: x_i f32[B,cin,size_i,size_i] * w_i f32[cout,cin,3,3] (+ shared pre-BN+ReLU, + residual r_i, raw copy raw_i)
// -> y_i; `variant` as in mvlm_conv_pair_bench.  The results must equal mvlm_conv2d's with the same kernel variant forced.
extern "C" int mvlm_conv2d_pair(mvlm_ctx* ctx, int batch, int cin, int cout, const float* x0_dev, int size0, const float* w0_host,
                                const float* r0_dev, float* raw0_dev, float* y0_dev, const float* x1_dev, int size1,
                                const float* w1_host, const float* r1_dev, float* raw1_dev, float* y1_dev,
                                const float* pre_scale_host, const float* pre_shift_host, int variant) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, x0_dev && x1_dev && w0_host && w1_host && y0_dev && y1_dev && variant >= 0, "conv2d_pair: bad arguments");
    MVLM_REQUIRE(ctx, (pre_scale_host == nullptr) == (pre_shift_host == nullptr), "conv2d_pair: pre scale/shift come in pairs");
    const ConvPadding pad = mvlm_conv_hook_padding(MVLM_HOOK_PAIR, {3, cin, cout});
    const int cin_pad = pad.cin_pad, cout_pad = pad.cout_pad;
    // the two layers' weights, then the pre-BN vectors they share
    const size_t n_w = round4(mvlm_conv_pack_sizes(3, cin_pad, cout_pad).w);
    std::vector<float> blob(2 * n_w + 2 * size_t(cin_pad), 0.f);
    const float* ws[2] = {w0_host, w1_host};
    for (int i = 0; i < 2; ++i) mvlm_conv_pack_transpose(ws[i], cout, cin, 3, cin_pad, cout_pad, blob.data() + i * n_w);
    if (pre_scale_host) {
        std::copy(pre_scale_host, pre_scale_host + cin, blob.begin() + 2 * n_w);
        std::copy(pre_shift_host, pre_shift_host + cin, blob.begin() + 2 * n_w + cin_pad);
    }
    auto* d = static_cast<float*>(ctx->get_scratch("conv2d.blob", blob.size() * 4));
    MVLM_REQUIRE(ctx, d, "conv2d_pair: scratch allocation failed");
    MVLM_CHECK_HIP(ctx, hipMemcpy(d, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    ConvArgs a[2];
    const float* xs[2] = {x0_dev, x1_dev};
    const float* rs[2] = {r0_dev, r1_dev};
    float* raws[2] = {raw0_dev, raw1_dev};
    float* ys[2] = {y0_dev, y1_dev};
    const int sizes[2] = {size0, size1};
    for (int i = 0; i < 2; ++i) {
        LayerOffsets o;
        o.w = long(i * n_w);
        if (pre_scale_host) {
            o.pre_scale = long(2 * n_w);
            o.pre_shift = long(2 * n_w) + cin_pad;
        }
        a[i] = layer_args(d, o, {batch, cin, cin_pad, cout, cout_pad, 3, sizes[i], sizes[i]});
        set_tensors(a[i], xs[i], rs[i], raws[i], ys[i]);
    }
    if (mvlm_launch_conv_pair(ctx, a[0], a[1], (variant & 0xfff) | MVLM_CONV_PAIR_FLAG)) return 1;
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Tuning hook for tools/tune_conv_pairs.py: conv j of a hourglass level's skip block at `size` and of the next level's first
// block at size / 2 (same channels, pre-BN + residual + raw copy as in the network) on zero data.  variant < 0: the two
// tuned single launches back to back; variant >= 0: ONE two-problem launch of kernel variant (variant & 255) with
// 1 << ((variant >> 8) & 3) / 1 << ((variant >> 10) & 3) K parts for the size / size / 2 problem.
extern "C" int mvlm_conv_pair_bench(mvlm_ctx* ctx, int batch, int cin, int cout, int size, int flags, int variant, int iters,
                                    float* ms_per_launch) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, batch > 0 && cin > 0 && cout > 0 && size >= 8 && size % 2 == 0 && iters > 0 && ms_per_launch, "conv_pair_bench: bad arguments");
    const ConvPadding pad = mvlm_conv_hook_padding(MVLM_HOOK_PAIR, {3, cin, cout});
    const int cin_pad = pad.cin_pad, cout_pad = pad.cout_pad;
    // (the direct weights only: these launches carry no other form)
    const size_t n_w = mvlm_conv_pack_sizes(3, cin_pad, cout_pad).w, n_vec = round4(size_t(cin_pad) * 2 + size_t(cout_pad) * 3);
    size_t px[2] = {size_t(batch) * size * size, size_t(batch) * (size / 2) * (size / 2)};
    size_t total = n_w + n_vec + 64;
    for (int i = 0; i < 2; ++i) total += round4(px[i] * cin) + 3 * round4(px[i] * cout);
    auto* base = static_cast<float*>(ctx->get_scratch("conv_bench", total * sizeof(float)));
    MVLM_REQUIRE(ctx, base, "conv_pair_bench: scratch allocation failed");
    MVLM_CHECK_HIP(ctx, hipMemsetAsync(base, 0, total * sizeof(float), ctx->stream));
    LayerOffsets o;
    if (flags & 1) {
        o.pre_scale = long(n_w);
        o.pre_shift = long(n_w) + cin_pad;
    }
    float* cur = base + n_w + n_vec;
    ConvArgs a[2];
    for (int i = 0; i < 2; ++i) {
        const int s = i ? size / 2 : size;
        a[i] = layer_args(base, o, {batch, cin, cin_pad, cout, cout_pad, 3, s, s});
        const size_t n_x = round4(px[i] * cin), n_y = round4(px[i] * cout);
        float* y = cur + n_x;  // input, output, raw copy, residual
        set_tensors(a[i], cur, (flags & 2) ? y + 2 * n_y : nullptr, (flags & 2) ? y + n_y : nullptr, y);
        cur = y + 3 * n_y;
    }
    const int saved = ctx->conv_force_variant;
    ctx->conv_force_variant = -1;
    auto launch = [&](int*) -> int {
        if (variant < 0) return mvlm_launch_conv(ctx, a[0], nullptr) || mvlm_launch_conv(ctx, a[1], nullptr);
        return mvlm_launch_conv_pair(ctx, a[0], a[1], (variant & 0xfff) | MVLM_CONV_PAIR_FLAG);
    };
    const int rc = timed_launches(ctx, "conv_pair_bench", iters, launch, nullptr, ms_per_launch);
    ctx->conv_force_variant = saved;
    return rc;
}
