// Stand-alone driver of mvlm_amd/csrc/conv_pack.cpp for tests/test_conv_pack_cpu.py (built with -fsanitize=address,undefined).
//   harness CASES OUT TABLE
// CASES: layers, each u32 ksize, cin, cout, has_bias, then the OIHW weights and the bias as f32.  Every layer is padded as
// mvlm_conv2d pads a 32 x 8 layer and packed as it packs one - the layer and its vectors first, the forms made from the weights
// inside the same, reserved blob - and once more as mvlm_cnn_load does it, from sources outside a blob that moves as it grows.
// OUT: per layer u32 cin_pad, cout_pad, n_floats, six i64 offsets (weights, bias, F(2,3), F(4,3), padded F(4,3), padded bias) and
// the blob.  TABLE: lines "site ksize cin cout bias pre post residual upsample_in w h cin_pad cout_pad" (site 0 mvlm_conv2d,
// 1 mvlm_conv_bench, 2 the pair hooks): the padding function must give every line's pair.  Then the timing hooks' arena is held
// against every pointer they hand out.  A line with INVARIANT and exit status 1 where any of it fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../mvlm_amd/csrc/conv_pack.h"

static size_t round4(size_t n) { return (n + 3) / 4 * 4; }

static int pack_cases(FILE* in, FILE* out) {
    uint32_t head[4];
    for (int index = 0; fread(head, 4, 4, in) == 4; ++index) {
        const int ksize = int(head[0]), cin = int(head[1]), cout = int(head[2]);
        const bool has_bias = head[3] != 0;
        std::vector<float> w(size_t(cout) * cin * ksize * ksize), bias(has_bias ? size_t(cout) : 0);
        if (fread(w.data(), 4, w.size(), in) != w.size() || fread(bias.data(), 4, bias.size(), in) != bias.size()) return 2;
        const ConvPadding pad = mvlm_conv_hook_padding(MVLM_HOOK_CONV2D, {ksize, cin, cout, has_bias, false, false, false, false, 32, 8});
        const ConvPackSizes sizes = mvlm_conv_pack_sizes(ksize, pad.cin_pad, pad.cout_pad);
        std::vector<float> blob;
        ConvPackTargets to;
        to.wino[MVLM_WINO_F23] = to.wino[MVLM_WINO_F43] = to.wino4_pad = ksize == 3 ? &blob : nullptr;
        blob.reserve(round4(sizes.w) + round4(size_t(pad.cout_pad)) + sizes.wino[0] + sizes.wino[1] + sizes.wino4_pad + sizes.wino4_pad_bias);
        const float* const reserved = blob.data();
        blob.resize(round4(sizes.w), 0.f);
        mvlm_conv_pack_transpose(w.data(), cout, cin, ksize, pad.cin_pad, pad.cout_pad, blob.data());
        long bias_off = -1;
        if (has_bias) {
            bias_off = long(blob.size());
            blob.resize(blob.size() + round4(size_t(pad.cout_pad)), 0.f);
            std::memcpy(blob.data() + bias_off, bias.data(), bias.size() * 4);
        }
        const ConvPackOffsets o = mvlm_conv_pack_forms(to, blob.data(), has_bias ? blob.data() + bias_off : nullptr, pad.cin_pad, pad.cout_pad);
        if (blob.data() != reserved) {
            printf("case %d INVARIANT the reserved blob moved\n", index);
            return 1;
        }
        // the loader's way: sources outside, a blob that is not empty, not a multiple of four long and not reserved
        const std::vector<float> w9(blob.begin(), blob.begin() + long(sizes.w)), b(blob.begin() + (has_bias ? bias_off : 0), blob.begin() + (has_bias ? bias_off + pad.cout_pad : 0));
        std::vector<float> other(3, 1.f);
        to.wino[MVLM_WINO_F23] = to.wino[MVLM_WINO_F43] = to.wino4_pad = ksize == 3 ? &other : nullptr;
        const ConvPackOffsets p = mvlm_conv_pack_forms(to, w9.data(), has_bias ? b.data() : nullptr, pad.cin_pad, pad.cout_pad);
        const long a_off[4] = {o.wino[0], o.wino[1], o.wino4_pad, o.wino4_pad_bias}, b_off[4] = {p.wino[0], p.wino[1], p.wino4_pad, p.wino4_pad_bias};
        const size_t len[4] = {sizes.wino[0], sizes.wino[1], sizes.wino4_pad, sizes.wino4_pad_bias};
        for (int k = 0; k < 4; ++k) {
            const bool same = (a_off[k] < 0) == (b_off[k] < 0) && (b_off[k] < 0 || (b_off[k] % 4 == 0 && b_off[k] >= 3 && size_t(b_off[k]) + len[k] <= other.size() &&
                                                                                      !std::memcmp(blob.data() + a_off[k], other.data() + b_off[k], len[k] * 4)));
            if (!same) {
                printf("case %d INVARIANT form %d differs between the two ways of packing\n", index, k);
                return 1;
            }
        }
        const uint32_t dims[3] = {uint32_t(pad.cin_pad), uint32_t(pad.cout_pad), uint32_t(blob.size())};
        const int64_t offs[6] = {0, bias_off, o.wino[0], o.wino[1], o.wino4_pad, o.wino4_pad_bias};
        fwrite(dims, 4, 3, out);
        fwrite(offs, 8, 6, out);
        fwrite(blob.data(), 4, blob.size(), out);
        printf("case %d k%d %d->%d padded %d->%d floats %zu\n", index, ksize, cin, cout, pad.cin_pad, pad.cout_pad, blob.size());
    }
    return 0;
}

static int padding_table(FILE* table, std::set<int>& bench_cout_pads) {
    int site, ksize, cin, cout, bias, pre, post, res, up, w, h, cin_pad, cout_pad;
    long rows = 0;
    while (fscanf(table, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &site, &ksize, &cin, &cout, &bias, &pre, &post, &res, &up, &w, &h, &cin_pad, &cout_pad) == 13) {
        if (site < 0 || site > 2) return 2;
        const ConvPadding pad = mvlm_conv_hook_padding(ConvHookSite(site), {ksize, cin, cout, bias != 0, pre != 0, post != 0, res != 0, up != 0, w, h});
        if (pad.cin_pad != cin_pad || pad.cout_pad != cout_pad) {
            printf("INVARIANT padding of table row %ld: %d %d, the table says %d %d\n", rows, pad.cin_pad, pad.cout_pad, cin_pad, cout_pad);
            return 1;
        }
        if (site == MVLM_HOOK_CONV_BENCH) bench_cout_pads.insert(pad.cout_pad);
        ++rows;
    }
    printf("padding rows %ld\n", rows);
    return feof(table) ? 0 : 2;
}

// mvlm_conv_bench puts every form of the weights at the arena's start, the vectors behind it (pre scale, pre shift [cin_pad],
// bias, post scale, post shift [cout_pad]) and hands the padded launch the bias as its [P] bias
static int arenas(const std::set<int>& cout_pads) {
    long checked = 0;
    for (int ksize : {1, 3})
        for (int cin_pad : {4, 8, 32, 256})
            for (int cout_pad : cout_pads) {
                const ConvPackSizes s = mvlm_conv_pack_sizes(ksize, cin_pad, cout_pad);
                const size_t arena = mvlm_conv_pack_arena_floats(ksize, cin_pad, cout_pad), P = size_t(mvlm_conv_wino4_padded_cout(cout_pad));
                const size_t before = size_t(ksize == 3 ? 18 : 1) * cin_pad * P;  // the bound the function replaced
                const bool ok = arena >= s.w && arena >= s.wino[MVLM_WINO_F23] && arena >= s.wino[MVLM_WINO_F43] && arena >= s.wino4_pad && arena >= before &&
                                s.wino4_pad_bias <= 3 * size_t(cout_pad);
                if (!ok) {
                    printf("INVARIANT arena k%d cin_pad %d cout_pad %d: %zu floats\n", ksize, cin_pad, cout_pad, arena);
                    return 1;
                }
                ++checked;
            }
    printf("arenas %ld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    FILE* table = fopen(argv[3], "r");
    if (!in || !out || !table) return 2;
    std::set<int> bench_cout_pads;
    int rc = pack_cases(in, out);
    if (!rc) rc = padding_table(table, bench_cout_pads);
    if (!rc) rc = arenas(bench_cout_pads);
    fclose(in);
    fclose(out);
    fclose(table);
    return rc;
}
