// Prints what the convolution dispatcher (mvlm_amd/csrc/conv_mfma.hip) decides, as a text table, without a GPU.
// Built by tests/test_conv_routing_cpu.py: this file and conv_mfma.hip are compiled host-only and linked without the kernels'
// translation units and without the HIP runtime.  The launchers mvlm_conv_launch_<id> / mvlm_conv_pair_launch_<id> are stubs
// that record which one was reached and what it was given; the few HIP calls the dispatcher's entry points make are stubs
// that succeed.  No data pointer is ever dereferenced: they all point at one dummy float.
// The output (tests/golden/conv_routing.txt) is run-length encoded over the batch axis (BATCHES) and grouped: one line
//   <what> {<case> <case> ...} | <batches> <result>, <batches> <result>, ...
// for all cases of <what> (context states, input channels, launch features ...) that decide alike at every batch.
// Run with the argument "wino4", the same program gives every launch the F(4,3) tile's weights as well (ConvArgs::w_wino4) and
// adds what only that tile decides: the Winograd mode x F(4,3) mode axis over the shapes of both Winograd tables, the launch
// features with and without w_wino4, code 2048 as override and as forced variant, and the per-variant queries for the codes
// 1024..4200 (tests/golden/conv_routing_wino4.txt).  There a refused launch prints a bare E: which launches are refused, which
// succeed and where they land is pinned, not the wording.
// Run with the argument "f43", it prints only how launches run on the F(4,3) tile once they have their variant code (conv_mfma.hip:
// f43_plan), driven through mvlm_launch_conv: the tile's wide or 32 x 16 workgroup shape for code 2048, and the 80- / 84-row direct
// tiles' launches on that tile over padded weights (tests/golden/conv_routing_f43.txt; the format is in its first lines).  The tile
// has a stub per workgroup shape; in the first two passes both report as code 2048, so those goldens do not see the shape.
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../mvlm_amd/csrc/common.h"
#include "../../mvlm_amd/csrc/conv_variants.h"
#include "../../mvlm_amd/csrc/conv_tuned.h"
#include "../../mvlm_amd/csrc/conv_tuned_net.h"
#include "../../mvlm_amd/csrc/conv_pair_tuned.h"
#include "../../mvlm_amd/csrc/conv_tuned_wino.h"
#include "../../mvlm_amd/csrc/conv_tuned_wino4.h"
#include "../../mvlm_amd/csrc/conv_wino4_wide_hold.h"
#include "../../mvlm_amd/csrc/conv_tuned_wino4_pad.h"

// ---- stubs ------------------------------------------------------------------------------------------------------------------
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip stub"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipMalloc(void**, size_t) { return hipErrorOutOfMemory; }
hipError_t hipMemset(void*, int, size_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }  // (mvlm_ctx's stage clocks: none has an event here)
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }

namespace {
struct Reached {
    int id = -1, kparts0 = 0, kparts1 = 0;
    const float* w = nullptr;
    char f43_shape = 0;  // 'n' / 'w': the F(4,3) tile's 32 x 16 / wide stub
    const float* bias = nullptr;
    int cout_pad = 0;
} g_reached;
}  // namespace

#define X(id, name, ...)                                                                    \
    int mvlm_conv_launch_##id(mvlm_ctx*, const ConvArgs& a) {                               \
        g_reached = {id, a.kparts, 0, a.w, 0, a.bias, a.cout_pad};                          \
        return 0;                                                                           \
    }                                                                                       \
    int mvlm_conv_pair_launch_##id(mvlm_ctx*, const ConvArgs& a0, const ConvArgs& a1) {     \
        g_reached = {id, a0.kparts, a1.kparts, a0.w};                                       \
        return 0;                                                                           \
    }
MVLM_CONV_VARIANTS(X)
#undef X
int mvlm_conv_launch_wino4_narrow(mvlm_ctx*, const ConvArgs& a) {
    g_reached = {MVLM_CONV_VARIANT_WINO4, a.kparts, 0, a.w, 'n', a.bias, a.cout_pad};
    return 0;
}
int mvlm_conv_launch_wino4_wide(mvlm_ctx*, const ConvArgs& a) {
    g_reached = {MVLM_CONV_VARIANT_WINO4, a.kparts, 0, a.w, 'w', a.bias, a.cout_pad};
    return 0;
}

namespace {

float g_dummy, g_dummy_wino, g_dummy_wino4;
int g_dummy_int;
bool g_wino4 = false;  // the second pass: every launch carries w_wino4

std::vector<int> batches() {
    std::vector<int> b;
    for (int i = 1; i <= 130; ++i) b.push_back(i);
    b.push_back(40000);  // beyond the tables' 16-bit batch field: the clamp
    return b;
}
const std::vector<int> BATCHES = batches();

// error messages, numbered in order of first appearance; the legend is printed last
std::vector<std::string> g_errors;
std::string error_token(const std::string& e) {
    size_t i = 0;
    while (i < g_errors.size() && g_errors[i] != e) ++i;
    if (i == g_errors.size()) g_errors.push_back(e);
    return "E" + std::to_string(i + 1);
}

// "<first>-<last> <result>, ..." over BATCHES
std::string runs(const std::function<std::string(int)>& result_at) {
    std::string out, cur;
    int first = 0, last = 0;
    auto flush = [&] { out += (out.empty() ? "" : ", ") + std::to_string(first) + (last != first ? "-" + std::to_string(last) : "") + " " + cur; };
    for (int b : BATCHES) {
        const std::string r = result_at(b);
        if (first && r == cur) {
            last = b;
            continue;
        }
        if (first) flush();
        cur = r;
        first = last = b;
    }
    flush();
    return out;
}

// rows (what, case, result) printed as one line per group of cases of a `what` with equal results, in order of appearance
struct Grouped {
    std::vector<std::string> order;
    std::map<std::string, std::vector<std::pair<std::string, std::string>>> rows;
    void add(const std::string& what, const std::string& which, const std::string& result) {
        if (!rows.count(what)) order.push_back(what);
        rows[what].push_back({which, result});
    }
    void print() {
        for (const std::string& what : order) {
            const auto& r = rows[what];
            std::vector<bool> done(r.size(), false);
            for (size_t i = 0; i < r.size(); ++i) {
                if (done[i]) continue;
                std::string cases;
                for (size_t j = i; j < r.size(); ++j)
                    if (r[j].second == r[i].second) {
                        done[j] = true;
                        cases += (cases.empty() ? "" : " ") + r[j].first;
                    }
                std::printf("%s {%s} | %s\n", what.c_str(), cases.c_str(), r[i].second.c_str());
            }
        }
        order.clear();
        rows.clear();
    }
};

using Shape = std::tuple<int, int, int, int>;  // ksize, cin_pad, cout_pad, size

std::string shape_label(const Shape& s) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "k%d %d>%d @%d", std::get<0>(s), std::get<1>(s), std::get<2>(s), std::get<3>(s));
    return buf;
}

// kind 0 plain, 1 scatter into the skip tensor, 2 the pooled tensor is wanted
ConvArgs make_args(const Shape& s, int kind, int batch) {
    ConvArgs a;
    a.ksize = std::get<0>(s);
    a.cin = a.cin_pad = a.in_ctot = std::get<1>(s);
    a.cout = a.cout_pad = a.out_ctot = std::get<2>(s);
    a.H = a.W = std::get<3>(s);
    a.B = batch;
    a.in = a.w = &g_dummy;
    a.w_wino = &g_dummy_wino;
    if (g_wino4) a.w_wino4 = &g_dummy_wino4;
    a.out = &g_dummy;
    if (kind == 1) {
        a.up_out = 1;
        a.skip = &g_dummy;
        a.skip_ctot = a.cout_pad;
    }
    if (kind == 2) {
        a.pool_hint = 1;
        a.pool_ctot = a.cout_pad;
    }
    return a;
}

// One launch as a token: "<variant_out>" when mvlm_launch_conv succeeded, "E<n>" (+ "@<variant_out>" if it was set) when not,
// then a letter per query that says yes: p mvlm_conv_can_pool, i mvlm_conv_in2_ok, w mvlm_conv_wino_variant >= 0 (+ its id
// where that is not variant_out), s the stub received w_wino as its weights, q it received w_wino4.  A successful launch must
// reach stub variant_out & 255 with kparts 1 << (variant_out >> 8), code 2048 the F(4,3) stub with kparts 1; otherwise
// "!<stub>/<kparts>" follows.  The second pass prints a refusal as "E[@<variant_out>]", without the message's number.
// pool_as_asked: give the launch a pooled output exactly where mvlm_conv_can_pool allows one, as the network does
std::string single(mvlm_ctx& ctx, ConvArgs a, bool pool_as_asked = true) {
    const int pool = mvlm_conv_can_pool(&ctx, a), in2 = mvlm_conv_in2_ok(&ctx, a), wino = mvlm_conv_wino_variant(&ctx, a);
    if (pool_as_asked && a.pool_hint && pool) a.pool_out = &g_dummy;
    g_reached = Reached();
    ctx.err.clear();
    int v = -9;
    const int rc = mvlm_launch_conv(&ctx, a, &v);
    std::string t = rc ? (g_wino4 ? "E" : error_token(ctx.err)) + (v != -9 ? "@" + std::to_string(v) : "") : std::to_string(v);
    if (pool) t += "p";
    if (in2) t += "i";
    if (wino >= 0) t += wino == v ? "w" : "w" + std::to_string(wino);
    if (g_reached.w == &g_dummy_wino) t += "s";
    if (g_reached.w == &g_dummy_wino4) t += "q";
    const bool is4 = v == MVLM_CONV_VARIANT_WINO4;
    if (rc ? g_reached.id != -1 : (g_reached.id != (is4 ? v : v & 255) || g_reached.kparts0 != (is4 ? 1 : 1 << (v >> 8))))
        t += "!" + std::to_string(g_reached.id) + "/" + std::to_string(g_reached.kparts0);
    return t;
}

// "-" no pair, else the pair's variant code; a failed launch adds " E<n>"; the stub must be code & 255 and the kparts
// 1 << (code >> 8 & 3), 1 << (code >> 10 & 3), otherwise "!<stub>/<kparts0>/<kparts1>" follows
std::string pair_launch(mvlm_ctx& ctx, const ConvArgs& a0, const ConvArgs& a1, int pv) {
    g_reached = Reached();
    ctx.err.clear();
    const int rc = mvlm_launch_conv_pair(&ctx, a0, a1, pv);
    std::string t = std::to_string(pv) + (rc ? " " + error_token(ctx.err) : "");
    if (rc ? g_reached.id != -1 : (g_reached.id != (pv & 255) || g_reached.kparts0 != 1 << ((pv >> 8) & 3) || g_reached.kparts1 != 1 << ((pv >> 10) & 3)))
        t += "!" + std::to_string(g_reached.id) + "/" + std::to_string(g_reached.kparts0) + "/" + std::to_string(g_reached.kparts1);
    return t;
}
std::string pair(mvlm_ctx& ctx, ConvArgs a0, ConvArgs a1, int mode) {
    const int pv = mvlm_conv_pair_variant(a0, a1, mode);
    if (pv < 0) return "-";
    for (ConvArgs* a : {&a0, &a1})  // the pooled output where the pair's tile can emit it, as the network does
        if (a->pool_hint && mvlm_conv_variant_can_pool(pv)) a->pool_out = &g_dummy;
    return pair_launch(ctx, a0, a1, pv);
}

struct State {
    const char* name;
    int winograd, force, winograd4 = 1;
};
void set_state(mvlm_ctx& ctx, const State& st) {
    ctx.conv_winograd = st.winograd;
    ctx.conv_winograd4 = st.winograd4;
    ctx.conv_force_variant = st.force;
}
const State DEFAULT_STATE = {"w1", 1, -1};

// every shape in every kind under this state
void singles(mvlm_ctx& ctx, Grouped& g, const std::vector<Shape>& shapes, const State& st) {
    set_state(ctx, st);
    for (const Shape& s : shapes)
        for (int kind = 0; kind < 3; ++kind)
            g.add(shape_label(s) + " kind" + std::to_string(kind), st.name, runs([&](int b) { return single(ctx, make_args(s, kind, b)); }));
    set_state(ctx, DEFAULT_STATE);
}

// launch features beyond the kind, for the fixed list
const char* const FEATURES[] = {"plain", "kind1", "amax", "up_in", "up_out2", "up_out2x4", "in2", "pool_out", "no_w_wino", "no_w_wino4"};
ConvArgs feature_args(const Shape& s, int feature, int batch) {
    ConvArgs a = make_args(s, feature == 1 ? 1 : 0, batch);
    switch (feature) {
    case 2:
        a.amax_val = &g_dummy;
        a.amax_idx = &g_dummy_int;
        a.out = nullptr;
        break;
    case 3: a.up_in = 1; break;
    case 4:
    case 5:
        a.up_out = 2;
        a.sub_y = 1;
        a.n_par = feature == 5 ? 4 : 1;
        break;
    case 6:
        a.in2 = &g_dummy;
        a.in2_ctot = a.cin_pad;
        break;
    case 7:  // the pooled output whether or not the tile can emit it
        a.pool_hint = 1;
        a.pool_out = &g_dummy;
        a.pool_ctot = a.cout_pad;
        break;
    case 8: a.w_wino = nullptr; break;
    case 9: a.w_wino4 = nullptr; break;
    }
    return a;
}

// ---- the third pass: how a launch runs on the F(4,3) tile (conv_mfma.hip: f43_plan) ----------------------------------------------
float g_pad_w, g_pad_bias, g_bias;
std::set<std::string> g_f43_failed;  // the statements of the golden's first lines that did not hold
void expect(bool ok, const std::string& statement) {
    if (!ok) g_f43_failed.insert(statement);
}

// One launch through mvlm_launch_conv.  The token: "<variant_out>" or "E[@<variant_out>]"; where it ran - n / w the F(4,3) tile's
// 32 x 16 / wide stub, p<cout_pad> the 32 x 16 stub with the pad entry's weights, d another tile's stub, - none; "!" if the stub's
// weights, bias or cout_pad are not what that way of running gives it; then the deltas of the two counters, wide/padded.
struct F43Run {
    std::string token;
    char where;
    int variant_out;
    int cout_pad;
    long long wide, padded;
};
F43Run f43_run(mvlm_ctx& ctx, ConvArgs a) {
    if (a.pool_hint && !a.pool_out && mvlm_conv_can_pool(&ctx, a)) a.pool_out = &g_dummy;  // as the network does
    const long long wide0 = ctx.conv_wino4_wide_launches, padded0 = ctx.conv_wino4_padded_launches;
    g_reached = Reached();
    ctx.err.clear();
    int v = -9;
    const int rc = mvlm_launch_conv(&ctx, a, &v);
    F43Run r;
    r.where = g_reached.id == -1 ? '-' : !g_reached.f43_shape ? 'd' : g_reached.w == &g_pad_w ? 'p' : g_reached.f43_shape;
    r.variant_out = v;
    r.cout_pad = g_reached.cout_pad;
    r.wide = ctx.conv_wino4_wide_launches - wide0;
    r.padded = ctx.conv_wino4_padded_launches - padded0;
    r.token = rc ? "E" + (v != -9 ? "@" + std::to_string(v) : std::string()) : std::to_string(v);
    r.token += r.where;
    bool as_given = true;
    if (r.where == 'p') {
        r.token += std::to_string(r.cout_pad);
        as_given = g_reached.f43_shape == 'n' && g_reached.bias == (a.bias ? &g_pad_bias : nullptr);
    } else if (r.where == 'n' || r.where == 'w') {
        as_given = g_reached.w == a.w_wino4 && g_reached.bias == a.bias && r.cout_pad == a.cout_pad;
    } else if (r.where == 'd') {
        as_given = (g_reached.w == a.w || g_reached.w == a.w_wino) && g_reached.bias == a.bias && r.cout_pad == a.cout_pad;
    }
    if (!as_given || (rc != 0) != (r.where == '-')) r.token += "!";
    r.token += " " + std::to_string(r.wide) + "/" + std::to_string(r.padded);
    return r;
}

int f43_pass() {
    mvlm_ctx ctx;
    Grouped g;
    const auto reset = [&] {
        set_state(ctx, DEFAULT_STATE);
        ctx.conv_winograd4_wide = 1;
        ctx.conv_winograd4_padded = 1;
    };
    reset();
    std::printf("# How a launch runs on the F(4,3) tile once it has its variant code, through mvlm_launch_conv.  A result, run-length encoded over\n"
                "# the batches: <variant_out> or E[@<variant_out>], then n = the tile's 32 x 16 stub, w = its wide stub, p<cout_pad> = the 32 x 16\n"
                "# stub with the pad entry's weights, its bias where the launch has one, and this cout_pad, d = another tile's stub, - = no stub\n"
                "# (refused); ! = the stub did not get what that way of running gives it; then <wide launches>/<padded launches> counted.\n"
                "# This file is written by the code it pins.  What can be read off the parent's launchers by eye, and is checked by the harness:\n"
                "#  a. the keys of conv_wino4_wide_hold.h reach n at every batch with the switch on, and w in their other kinds;\n"
                "#  b. k3 256>84 @128 and k3 256>80 @128 (kind 0) reach p96 from batch 96 on and d below in padded mode 1 (p1w1q1f-1), p96 at every\n"
                "#     batch in mode 2 (p2w1q1f-1), and never with padded mode 0, Winograd or F(4,3) mode 0, or the variant forced;\n"
                "#  c. a launch with one more feature, one that lacks the pad entry, its weights or its bias, 260 input channels or a size that\n"
                "#     is no multiple of 16 never reaches the F(4,3) tile, and both counters stay 0 (no_bias is the exception: it reaches p);\n"
                "#  d. variant_out is 2048 exactly where p is printed; a wide launch counts 1/0, a padded one 0/1, any other 0/0.\n"
                "# (A launch refused before any stub, as at batch 40000 for its tensors' size, is outside a. to c.)\n");

    // -- the wide shape
    std::printf("# -- code 2048: <shape> <kind> {<how>:s<wide switch>}, how = q2 routed by F(4,3) mode 2, f forced; the shapes of conv_tuned_wino4.h\n"
                "# and conv_wino4_wide_hold.h, output channels not in 64s (32, 96), and @40, a size the tile does not divide (routed elsewhere; forced\n"
                "# and refused only at the real launch)\n");
    g_wino4 = true;
    std::set<Shape> wide_set = {Shape{3, 64, 32, 64}, Shape{3, 64, 96, 64}, Shape{3, 64, 64, 40}};
    for (int i = 0; i < MVLM_CONV_TUNED_WINO4_N; ++i) wide_set.insert({3, MVLM_CONV_TUNED_WINO4[i].cin_pad, MVLM_CONV_TUNED_WINO4[i].cout_pad, MVLM_CONV_TUNED_WINO4[i].size});
    for (int i = 0; i < MVLM_CONV_WINO4_WIDE_HOLD_N; ++i) wide_set.insert({3, MVLM_CONV_WINO4_WIDE_HOLD[i].cin_pad, MVLM_CONV_WINO4_WIDE_HOLD[i].cout_pad, MVLM_CONV_WINO4_WIDE_HOLD[i].size});
    for (const Shape& s : wide_set)
        for (int kind = 0; kind < 3; ++kind) {
            int held = 0, held_other_kind = 0;
            for (int i = 0; i < MVLM_CONV_WINO4_WIDE_HOLD_N; ++i) {
                const ConvWino4WideHold& e = MVLM_CONV_WINO4_WIDE_HOLD[i];
                if (Shape{3, e.cin_pad, e.cout_pad, e.size} == s) (e.kind == kind ? held : held_other_kind) = 1;
            }
            for (int forced = 0; forced < 2; ++forced)
                for (int sw = 0; sw < 2; ++sw) {
                    ctx.conv_winograd4 = forced ? 1 : 2;
                    ctx.conv_force_variant = forced ? MVLM_CONV_VARIANT_WINO4 : -1;
                    ctx.conv_winograd4_wide = sw;
                    g.add("wide " + shape_label(s) + " kind" + std::to_string(kind), std::string(forced ? "f" : "q2") + ":s" + std::to_string(sw), runs([&](int b) {
                        const F43Run r = f43_run(ctx, make_args(s, kind, b));
                        if (sw && held && r.where != '-') expect(r.where == 'n', "a");
                        if (sw && !held && held_other_kind && r.where != '-') expect(r.where == 'w', "a");
                        if (!sw) expect(r.where != 'w', "a");
                        expect(r.padded == 0 && r.wide == (r.where == 'w'), "d");
                        return r.token;
                    }));
                }
        }
    g.print();
    reset();
    g_wino4 = false;  // (a layer on 80 or 84 rows has no F(4,3) weights of its own: the tile does not divide it)

    // -- the padded launches
    ctx.conv_wino4_pads = {ConvWino4Pad{}, ConvWino4Pad{&g_pad_w, &g_pad_bias}, ConvWino4Pad{nullptr, &g_pad_bias}, ConvWino4Pad{&g_pad_w, nullptr}};
    const int PAD_FULL = 2, PAD_NO_W = 3, PAD_NO_BIAS = 4;  // (ConvArgs::wino4_pad is 1 + the index)
    const auto padded_args = [&](const Shape& s, int b) {
        ConvArgs a = make_args(s, 0, b);
        a.bias = &g_bias;
        a.wino4_pad = PAD_FULL;
        return a;
    };
    const auto check_d = [](const F43Run& r) {
        expect((r.where == 'p') == (r.variant_out == MVLM_CONV_VARIANT_WINO4), "d");
        expect(r.wide == 0 && r.padded == (r.where == 'p'), "d");
    };
    const Shape pad_shapes[] = {Shape{3, 256, 84, 128}, Shape{3, 256, 80, 128}, Shape{3, 8, 84, 32}, Shape{3, 64, 80, 32}};
    std::printf("# -- the 84- / 80-row tiles' launches with a pad entry: <shape> {p<padded mode>w<Winograd mode>q<F(4,3) mode>f<conv_force_variant>}\n");
    for (const Shape& s : pad_shapes) {
        const bool in_table = std::get<1>(s) == 256;
        const int direct = std::get<2>(s) == 84 ? 26 : 16;
        for (int pm = 0; pm < 3; ++pm)
            for (int wm = 0; wm < 2; ++wm)
                for (int qm = 0; qm < 2; ++qm)
                    for (int force : {-1, -2, direct}) {
                        set_state(ctx, State{"", wm, force, qm});
                        ctx.conv_winograd4_padded = pm;
                        const std::string name = "p" + std::to_string(pm) + "w" + std::to_string(wm) + "q" + std::to_string(qm) + "f" + std::to_string(force);
                        g.add("padded " + shape_label(s), name, runs([&](int b) {
                            const F43Run r = f43_run(ctx, padded_args(s, b));
                            check_d(r);
                            if (r.where == 'p') expect(r.cout_pad == 96, "b");
                            if (r.where == '-') return r.token;
                            if (pm == 0 || wm == 0 || qm == 0 || force >= 0) expect(r.where == 'd' && r.variant_out == direct, "b");
                            else if (force == -1 && in_table) expect(pm == 2 || b >= 96 ? r.where == 'p' : r.where == 'd' && r.variant_out == direct, "b");
                            return r.token;
                        }));
                    }
    }
    g.print();
    reset();

    std::printf("# -- the same in padded mode 2, one thing changed: <shape> {<what>}\n");
    ctx.conv_winograd4_padded = 2;
    using Change = std::function<void(ConvArgs&)>;
    const std::pair<const char*, Change> changes[] = {
        {"none", [](ConvArgs&) {}},
        {"res1", [](ConvArgs& a) { a.res1 = &g_dummy, a.res1_ctot = a.cout_pad; }},
        {"res2", [](ConvArgs& a) { a.res2 = &g_dummy, a.res2_ctot = a.cout_pad; }},
        {"post_scale", [](ConvArgs& a) { a.post_scale = a.post_shift = &g_dummy; }},
        {"out_raw", [](ConvArgs& a) { a.out_raw = &g_dummy, a.raw_ctot = a.cout_pad; }},
        {"up_out1", [](ConvArgs& a) { a.up_out = 1, a.skip = &g_dummy, a.skip_ctot = a.cout_pad; }},
        {"amax_val", [](ConvArgs& a) { a.amax_val = &g_dummy, a.amax_idx = &g_dummy_int; }},
        {"in2", [](ConvArgs& a) { a.in2 = &g_dummy, a.in2_ctot = a.cin_pad; }},
        {"pool_out", [](ConvArgs& a) { a.pool_hint = 1, a.pool_out = &g_dummy, a.pool_ctot = a.cout_pad; }},
        {"wino4_pad0", [](ConvArgs& a) { a.wino4_pad = 0; }},
        {"wino4_pad_beyond", [](ConvArgs& a) { a.wino4_pad = 5; }},
        {"pad_without_w", [&](ConvArgs& a) { a.wino4_pad = PAD_NO_W; }},
        {"pad_without_bias", [&](ConvArgs& a) { a.wino4_pad = PAD_NO_BIAS; }},
        {"no_bias", [](ConvArgs& a) { a.bias = nullptr; }},
        {"no_bias_pad_without_bias", [&](ConvArgs& a) { a.bias = nullptr, a.wino4_pad = PAD_NO_BIAS; }},
        {"cin_pad260", [](ConvArgs& a) { a.cin = a.cin_pad = a.in_ctot = 260; }},
        {"@40", [](ConvArgs& a) { a.H = a.W = 40; }},
    };
    for (const Shape& s : pad_shapes)
        for (const auto& c : changes) {
            const std::string what = c.first;
            g.add("padded " + shape_label(s), what, runs([&](int b) {
                ConvArgs a = padded_args(s, b);
                c.second(a);
                const F43Run r = f43_run(ctx, a);
                check_d(r);
                if (what == "none" || what.rfind("no_bias", 0) == 0) expect(r.where == 'p' || r.where == '-', "c");
                else expect((r.where == 'd' || r.where == '-') && r.wide == 0 && r.padded == 0, "c");
                return r.token;
            }));
        }
    g.print();

    for (const std::string& f : g_f43_failed) std::fprintf(stderr, "statement %s of the first lines does not hold\n", f.c_str());
    return g_f43_failed.empty() ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "f43")) return f43_pass();
    g_wino4 = argc > 1 && !std::strcmp(argv[1], "wino4");
    const int n_features = g_wino4 ? 10 : 9;  // (no_w_wino4 says something in the second pass only)
    mvlm_ctx ctx;
    set_state(ctx, DEFAULT_STATE);
    Grouped g;

    // every shape of the four tuned tables (the pair table's at both of its sizes)
    std::set<Shape> table_set;
    for (int i = 0; i < MVLM_CONV_TUNED_N; ++i) {
        const ConvTuned& e = MVLM_CONV_TUNED[i];
        table_set.insert({e.ksize, e.cin_pad, e.cout_pad, e.size});
    }
    for (int i = 0; i < MVLM_CONV_TUNED_NET_N; ++i) {
        const ConvTunedNet& e = MVLM_CONV_TUNED_NET[i];
        table_set.insert({e.ksize, e.cin_pad, e.cout_pad, e.size});
    }
    std::set<std::tuple<int, int, int>> pair_set;
    for (int i = 0; i < MVLM_CONV_PAIR_TUNED_N; ++i) {
        const ConvPairTuned& e = MVLM_CONV_PAIR_TUNED[i];
        pair_set.insert({e.cin_pad, e.cout_pad, e.size});
        table_set.insert({3, e.cin_pad, e.cout_pad, e.size});
        table_set.insert({3, e.cin_pad, e.cout_pad, e.size / 2});
    }
    for (int i = 0; i < MVLM_CONV_TUNED_WINO_N; ++i) {
        const ConvTunedWino& e = MVLM_CONV_TUNED_WINO[i];
        table_set.insert({3, e.cin_pad, e.cout_pad, e.size});
    }
    std::set<Shape> wino_set;  // the shapes of the two Winograd tables (all of them among the tables' shapes already)
    for (int i = 0; i < MVLM_CONV_TUNED_WINO_N; ++i) wino_set.insert({3, MVLM_CONV_TUNED_WINO[i].cin_pad, MVLM_CONV_TUNED_WINO[i].cout_pad, MVLM_CONV_TUNED_WINO[i].size});
    for (int i = 0; i < MVLM_CONV_TUNED_WINO4_N; ++i) wino_set.insert({3, MVLM_CONV_TUNED_WINO4[i].cin_pad, MVLM_CONV_TUNED_WINO4[i].cout_pad, MVLM_CONV_TUNED_WINO4[i].size});
    const std::vector<Shape> table_shapes(table_set.begin(), table_set.end()), wino_shapes(wino_set.begin(), wino_set.end());

    std::printf("# single launches.  Result of a launch: <variant_out> or E<n>[@<variant_out>], then p = can_pool, i = in2_ok, w[<id>] = routed to a\n"
                "# Winograd variant, s = the weights were swapped for w_wino.  Context states: w<m> Winograd mode m; rules conv_force_variant -2;\n"
                "# force10 conv_force_variant 10; ov<v> after mvlm_conv_set_override(3, 128, 64, 64, kind 0, v)\n");
    std::printf("# -- shapes of the tuned tables: <shape> <kind> {states}\n");
    for (const State& st : {State{"w0", 0, -1}, DEFAULT_STATE, State{"w2", 2, -1}, State{"rules", 1, -2}}) singles(ctx, g, table_shapes, st);
    g.print();

    if (g_wino4) {
        std::printf("# -- second pass: every launch carries w_wino4; q = the weights were swapped for it; a refusal is E[@<variant_out>].\n"
                    "# Shapes of the two Winograd tables, Winograd mode x F(4,3) mode: <shape> <kind> {w<mode>q<mode4>}\n");
        for (int m = 0; m < 3; ++m)
            for (int m4 = 0; m4 < 3; ++m4) {
                const std::string name = "w" + std::to_string(m) + "q" + std::to_string(m4);
                singles(ctx, g, wino_shapes, State{name.c_str(), m, -1, m4});
            }
        g.print();
    }

    const int couts[] = {32, 64, 80, 84, 96, 128}, sizes[] = {4, 8, 16, 32, 64, 128, 256}, cins[] = {4, 16, 32, 64, 128, 256, 320};
    std::vector<State> fixed_states = {State{"w0", 0, -1}, DEFAULT_STATE, State{"w2", 2, -1}, State{"rules", 1, -2}};
    if (g_wino4) fixed_states.insert(fixed_states.end(), {State{"w1q2", 1, -1, 2}, State{"w2q2", 2, -1, 2}, State{"w1q0", 1, -1, 0}});
    std::printf("# -- fixed list, plain 3x3 layers: k3 *><cout_pad> @<size> {<state>:<cin_pad>}\n");
    for (const State& st : fixed_states) {
        set_state(ctx, st);
        for (int co : couts)
            for (int s : sizes)
                for (int ci : cins)
                    g.add("k3 *>" + std::to_string(co) + " @" + std::to_string(s), std::string(st.name) + ":" + std::to_string(ci),
                          runs([&](int b) { return single(ctx, feature_args(Shape{3, ci, co, s}, 0, b)); }));
    }
    g.print();
    std::printf("# -- fixed list, 1x1, 2x2 and the launch features at 128 input channels: <shape> {<state>:<feature>}\n");
    for (const State& st : fixed_states) {
        if (st.winograd == 0) continue;  // (mode 0 on these channels: the plain layers above and the tables' shapes)
        set_state(ctx, st);
        for (int ks : {1, 2, 3})
            for (int co : couts)
                for (int s : {16, 32, 128})
                    for (int f = ks == 3 ? 1 : 0; f < n_features; ++f) {
                        // (the plain 3x3 layers are above; 1x1 and 2x2 do not look at the Winograd mode)
                        if (ks != 3 && (st.winograd == 2 || st.winograd4 != 1)) continue;
                        if (ks == 1 && f != 0 && f != 1 && f != 7) continue;
                        if (ks == 2 && (f == 1 || f == 3 || f == 7 || f == 8 || f == 9)) continue;
                        const Shape sh{ks, 128, co, s};
                        g.add(shape_label(sh), std::string(st.name) + ":" + FEATURES[f], runs([&](int b) { return single(ctx, feature_args(sh, f, b), false); }));
                    }
    }
    set_state(ctx, DEFAULT_STATE);
    g.print();

    std::printf("# -- a forced variant and tuning overrides: 128>64 shapes of the tables from 64x64 on\n");
    std::vector<Shape> ov_shapes;
    for (const Shape& s : table_shapes)
        if (std::get<1>(s) == 128 && std::get<2>(s) == 64 && std::get<3>(s) >= 64) ov_shapes.push_back(s);
    singles(ctx, g, ov_shapes, {"force10", 1, 10});
    if (g_wino4) {
        singles(ctx, g, ov_shapes, {"force2048", 1, MVLM_CONV_VARIANT_WINO4});
        // the forced F(4,3) tile with each feature: a shape it divides, one too small for it, one with more channels than its LDS table
        ctx.conv_force_variant = MVLM_CONV_VARIANT_WINO4;
        for (const Shape& sh : {Shape{3, 128, 64, 64}, Shape{3, 128, 64, 8}, Shape{3, 320, 64, 64}})
            for (int f = 0; f < n_features; ++f)
                g.add(shape_label(sh), std::string("force2048:") + FEATURES[f], runs([&](int b) { return single(ctx, feature_args(sh, f, b), false); }));
        ctx.conv_force_variant = -1;
    }
    std::vector<int> ov_variants = {9, 40, -1, 0, 265};
    if (g_wino4) {
        ov_variants.push_back(MVLM_CONV_VARIANT_WINO4);
        ctx.err.clear();
        const int rc = mvlm_conv_set_override(&ctx, 3, 128, 64, 8, 0, MVLM_CONV_VARIANT_WINO4);  // (8x8: the tile does not divide it)
        std::printf("set_override %d at size 8 -> %d%s, %d entries\n", MVLM_CONV_VARIANT_WINO4, rc, rc ? (" " + error_token(ctx.err)).c_str() : "", int(ctx.conv_overrides.size()));
    }
    for (int variant : ov_variants) {
        ctx.err.clear();
        const int rc = mvlm_conv_set_override(&ctx, 3, 128, 64, 64, 0, variant);
        std::printf("set_override %d -> %d%s, %d entries\n", variant, rc, rc ? (" " + error_token(ctx.err)).c_str() : "", int(ctx.conv_overrides.size()));
        singles(ctx, g, ov_shapes, {("ov" + std::to_string(variant)).c_str(), 1, -1});
        // an argument beyond the entries' 16-bit fields (65600 = 65536 + 64) names no entry: nothing is removed
        if (variant == 40) std::printf("set_override -1 at size 65600 -> %d, %d entries\n", mvlm_conv_set_override(&ctx, 3, 128, 64, 65600, 0, -1), int(ctx.conv_overrides.size()));
    }
    std::printf("set_override clear -> %d", mvlm_conv_set_override(&ctx, 0, 0, 0, 0, 0, 0));
    std::printf(", %d entries\n", int(ctx.conv_overrides.size()));
    g.print();

    std::printf("# -- 32-bit element offsets and the other launch checks: k3 128>128 @256 B40, one field changed\n");
    {
        const Shape sh{3, 128, 128, 256};
        const int big = 2048;
        using Change = std::function<void(ConvArgs&)>;
        auto check = [&](const char* what, const Shape& shape, int kind, const Change& change) {
            ConvArgs a = make_args(shape, kind, 40);
            change(a);
            std::printf("check %s | %s\n", what, single(ctx, a, false).c_str());
        };
        check("none", sh, 0, [](ConvArgs&) {});
        check("in_ctot", sh, 0, [&](ConvArgs& a) { a.in_ctot = big; });
        check("raw_ctot", sh, 0, [&](ConvArgs& a) { a.out_raw = &g_dummy, a.raw_ctot = big; });
        check("res1_ctot", sh, 0, [&](ConvArgs& a) { a.res1 = &g_dummy, a.res1_ctot = big; });
        check("res2_ctot", sh, 0, [&](ConvArgs& a) { a.res2 = &g_dummy, a.res2_ctot = big; });
        check("out_ctot", sh, 0, [&](ConvArgs& a) { a.out_ctot = big; });
        check("out_ctot up_out", sh, 1, [&](ConvArgs& a) { a.out_ctot = big / 4; });
        check("skip_ctot", sh, 1, [&](ConvArgs& a) { a.skip_ctot = big / 4; });
        check("in2_ctot", sh, 0, [&](ConvArgs& a) { a.in2 = &g_dummy, a.in2_ctot = big * 4; });
        check("pool_ctot", sh, 2, [&](ConvArgs& a) { a.pool_out = &g_dummy, a.pool_ctot = big * 4; });
        check("null in", sh, 0, [](ConvArgs& a) { a.in = nullptr; });
        check("not square", sh, 0, [](ConvArgs& a) { a.W = 128; });
        check("odd up_in", Shape{3, 128, 128, 33}, 0, [](ConvArgs& a) { a.up_in = 1; });
        check("no skip", sh, 1, [](ConvArgs& a) { a.skip = nullptr; });
        check("sub_x", Shape{2, 128, 96, 256}, 0, [](ConvArgs& a) { a.sub_x = 2; });
        check("no output", sh, 0, [](ConvArgs& a) { a.out = nullptr; });
        for (int force : {1024 + 15, 63, 256 + 15}) {
            ctx.conv_force_variant = force;
            check(("force " + std::to_string(force)).c_str(), sh, 0, [](ConvArgs&) {});
        }
        ctx.conv_force_variant = -1;

        // pairs: problem 0 as above with one field changed, problem 1 the same layer at half the size
        const int pv = MVLM_CONV_PAIR_FLAG | 0, pv_sk = MVLM_CONV_PAIR_FLAG | 15 | (1 << 8) | (2 << 10);
        auto check_pair = [&](const char* what, int pair_variant, int kind, const Change& change) {
            ConvArgs a0 = make_args(sh, kind, 40), a1 = make_args(Shape{3, 128, 128, 128}, 0, 40);
            change(a0);
            std::printf("check pair %s | %s\n", what, pair_launch(ctx, a0, a1, pair_variant).c_str());
        };
        check_pair("none", pv, 0, [](ConvArgs&) {});
        check_pair("split-K", pv_sk, 0, [](ConvArgs&) {});
        check_pair("not a pair variant", 0, 0, [](ConvArgs&) {});
        check_pair("beyond the pair codes", 2 * MVLM_CONV_PAIR_FLAG, 0, [](ConvArgs&) {});
        check_pair("unknown base", MVLM_CONV_PAIR_FLAG | 63, 0, [](ConvArgs&) {});
        check_pair("in_ctot", pv, 0, [&](ConvArgs& a) { a.in_ctot = big; });
        check_pair("raw_ctot", pv, 0, [&](ConvArgs& a) { a.out_raw = &g_dummy, a.raw_ctot = big; });
        check_pair("res1_ctot", pv, 0, [&](ConvArgs& a) { a.res1 = &g_dummy, a.res1_ctot = big; });
        check_pair("res2_ctot", pv, 0, [&](ConvArgs& a) { a.res2 = &g_dummy, a.res2_ctot = big; });
        check_pair("out_ctot", pv, 0, [&](ConvArgs& a) { a.out_ctot = big; });
        check_pair("kind 1", pv, 1, [](ConvArgs&) {});
        check_pair("out_ctot up_out", pv, 1, [&](ConvArgs& a) { a.out_ctot = big / 4; });
        check_pair("skip_ctot", pv, 1, [&](ConvArgs& a) { a.skip_ctot = big / 4; });
        check_pair("pooled", pv, 2, [](ConvArgs& a) { a.pool_out = &g_dummy; });
        check_pair("pooled on a tile that cannot", pv_sk, 2, [](ConvArgs& a) { a.pool_out = &g_dummy; });
        check_pair("pool_ctot", pv, 2, [&](ConvArgs& a) { a.pool_out = &g_dummy, a.pool_ctot = big * 4; });
        check_pair("in2 (not among a pair's tensors)", pv, 0, [&](ConvArgs& a) { a.in2 = &g_dummy, a.in2_ctot = big * 4; });
        check_pair("up_in", pv, 0, [](ConvArgs& a) { a.up_in = 1; });
        check_pair("no output", pv, 0, [](ConvArgs& a) { a.out = nullptr; });
        check_pair("null w", pv, 0, [](ConvArgs& a) { a.w = nullptr; });
    }

    std::printf("# pairs: <cin_pad>><cout_pad> @<size>+@<size/2> {p<mode>h<pool_hint of problem 0 + 2 * of problem 1>} | <batches> <pair variant code or ->\n");
    {
        std::vector<std::tuple<int, int, int>> pair_shapes(pair_set.begin(), pair_set.end());
        pair_shapes.push_back({64, 96, 64});   // no pair variant serves these two
        pair_shapes.push_back({128, 80, 128});
        for (int mode = 0; mode < 3; ++mode)
            for (const auto& p : pair_shapes)
                for (int hint = 0; hint < 4; ++hint) {
                    const int ci = std::get<0>(p), co = std::get<1>(p), s = std::get<2>(p);
                    char what[96];
                    std::snprintf(what, sizeof what, "pair %d>%d @%d+@%d", ci, co, s, s / 2);
                    g.add(what, "p" + std::to_string(mode) + "h" + std::to_string(hint), runs([&](int b) {
                        return pair(ctx, make_args(Shape{3, ci, co, s}, (hint & 1) ? 2 : 0, b), make_args(Shape{3, ci, co, s / 2}, (hint & 2) ? 2 : 0, b), mode);
                    }));
                }
        g.print();
    }

    // the ids of first..last that serve every shape of the list, per kind
    auto serves = [&](int first, int last) {
        std::printf("# mvlm_conv_variant_serves: k<ksize> *><cout_pad> @<size> {<cin_pad>:<kinds of -1..3 with this answer>} | the ids of %d..%d that serve\n", first, last);
        std::vector<Shape> shapes = table_shapes;
        for (int co : couts)
            for (int s : sizes)
                for (int ci : cins) shapes.push_back(Shape{3, ci, co, s});
        for (const Shape& s : shapes) {
            Grouped kinds;  // the kinds of this shape with equal answers
            for (int kind = -1; kind <= 3; ++kind) {
                std::string ids;
                for (int v = first; v <= last; ++v)
                    if (mvlm_conv_variant_serves(v, std::get<0>(s), std::get<1>(s), std::get<2>(s), std::get<3>(s), kind)) ids += " " + std::to_string(v);
                kinds.add(ids, std::to_string(kind), "");
            }
            for (const std::string& ids : kinds.order) {
                std::string which;
                for (const auto& k : kinds.rows[ids]) which += (which.empty() ? "" : ",") + k.first;
                char what[64];
                std::snprintf(what, sizeof what, "serves k%d *>%d @%d", std::get<0>(s), std::get<2>(s), std::get<3>(s));
                g.add(what, std::to_string(std::get<1>(s)) + ":" + which, ids.empty() ? "none" : ids.substr(1));
            }
        }
        g.print();
    };
    serves(-1, 1023);
    if (g_wino4) serves(1024, 4200);

    std::printf("# variant ids -1..255: <first>-<last> | name is_wino can_pool\n");
    {
        auto describe = [](int v) {
            return std::string(mvlm_conv_variant_name_impl(v)) + " " + std::to_string(int(mvlm_conv_variant_is_wino(v))) + " " +
                   std::to_string(int(mvlm_conv_variant_can_pool(v)));
        };
        std::string cur;
        int first = -1;
        for (int v = -1; v <= 256; ++v) {
            const std::string d = v <= 255 ? describe(v) : std::string();
            if (v > -1 && d == cur) continue;
            if (v > -1) std::printf("id %d-%d | %s\n", first, v - 1, cur.c_str());
            cur = d;
            first = v;
        }
        // 256..1100: "<name of id & 255>_k<1 << (id >> 8 & 3)>", never Winograd, pools as id & 255 does; the exceptions are listed
        int exceptions = 0;
        for (int v = 256; v <= 1100; ++v) {
            const std::string name = std::string(mvlm_conv_variant_name_impl(v & 255)) + "_k" + std::to_string(1 << ((v >> 8) & 3));
            if (name != mvlm_conv_variant_name_impl(v) || mvlm_conv_variant_is_wino(v) || mvlm_conv_variant_can_pool(v) != mvlm_conv_variant_can_pool(v & 255)) {
                std::printf("id %d | %s\n", v, describe(v).c_str());
                ++exceptions;
            }
        }
        std::printf("ids 256-1100 | <name of id & 255>_k<1 << (id >> 8 & 3)> 0 <can_pool of id & 255>, %d exceptions\n", exceptions);
        const int P = MVLM_CONV_PAIR_FLAG;
        for (int v : {260, 527, 808, 1063, P | 0, P | 10, P | 15 | (1 << 8) | (2 << 10), P | 13 | (3 << 10), P | 40, P | 63, 2 * P | 10})
            std::printf("id %d | %s\n", v, describe(v).c_str());
    }
    if (g_wino4) {
        std::printf("# variant codes 1024..4200: <first>-<last> | name is_wino is_wino4 can_pool\n");
        auto describe = [](int v) {
            return std::string(mvlm_conv_variant_name_impl(v)) + " " + std::to_string(int(mvlm_conv_variant_is_wino(v))) + " " +
                   std::to_string(int(mvlm_conv_variant_is_wino4(v))) + " " + std::to_string(int(mvlm_conv_variant_can_pool(v)));
        };
        std::string cur = describe(1024);
        int first = 1024;
        for (int v = 1025; v <= 4201; ++v) {
            const std::string d = v <= 4200 ? describe(v) : std::string();
            if (d == cur) continue;
            std::printf("code %d-%d | %s\n", first, v - 1, cur.c_str());
            cur = d;
            first = v;
        }
    }

    std::printf("# mvlm_conv_wino_serves_slot: k<ksize> {cin_pad} | the cout_pad it serves\n");
    for (int ks : {1, 2, 3})
        for (int ci : {3, 4, 6, 16, 32, 64, 76, 84, 128, 256, 320}) {
            std::string cos;
            for (int co : {32, 64, 80, 84, 96, 128, 192, 256})
                if (mvlm_conv_wino_serves_slot(ks, ci, co)) cos += " " + std::to_string(co);
            g.add("slot k" + std::to_string(ks), std::to_string(ci), cos.empty() ? "none" : cos.substr(1));
        }
    g.print();
    if (g_wino4) {
        std::printf("# mvlm_conv_wino4_serves_slot: k<ksize> {cin_pad} | the cout_pad it serves\n");
        for (int ks : {1, 2, 3})
            for (int ci : {3, 4, 6, 16, 32, 64, 76, 84, 128, 256, 320}) {
                std::string cos;
                for (int co : {32, 64, 80, 84, 96, 128, 192, 256})
                    if (mvlm_conv_wino4_serves_slot(ks, ci, co)) cos += " " + std::to_string(co);
                g.add("slot4 k" + std::to_string(ks), std::to_string(ci), cos.empty() ? "none" : cos.substr(1));
            }
        g.print();
    }

    std::printf("# error messages\n");
    for (size_t i = 0; i < g_errors.size(); ++i) std::printf("E%d: %s\n", int(i) + 1, g_errors[i].c_str());
    return 0;
}
