// Internal declarations shared by the HIP translation units of libmvlm_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mvlm_hip.h"
#include "conv_pack.h"
#include "jpeg_plan.h"

#define MVLM_CHECK_HIP(ctx, expr)                                                            \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            (ctx)->fail(std::string(#expr) + ": " + hipGetErrorString(_e));                  \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

// every entry point: serialise callers of this context and make its GPU the calling thread's
// current device (a process may hold contexts for several GPUs)
#define MVLM_ENTER(ctx)                               \
    std::lock_guard<std::mutex> _mvlm_lock((ctx)->mu); \
    MvlmOrderGuard _mvlm_order{(ctx)};                 \
    MVLM_CHECK_HIP(ctx, hipSetDevice((ctx)->device))

#define MVLM_REQUIRE(ctx, cond, msg)                                                         \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            (ctx)->fail(std::string(msg) + " [" #cond "]");                                  \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

// ---------------------------------------------------------------------------------------
// np.argmax order on floats (paulsenpredictor.py:123): NaN counts as the maximum, the first one wins; otherwise the
// larger value, the lower index on ties (+0 == -0).  argmax_key maps a float to an int whose integer order is that
// order; argmax_value maps the winning key back (a NaN comes back as a quiet NaN).
__host__ __device__ inline int argmax_key(float v) {
    v = v + 0.0f;  // -0 -> +0
    int b;
    __builtin_memcpy(&b, &v, 4);
    if (v != v) return 0x7fffffff;
    return b >= 0 ? b : (b ^ 0x7fffffff);
}
__host__ __device__ inline float argmax_value(int key) {
    int b = key == 0x7fffffff ? 0x7fc00000 : (key >= 0 ? key : (key ^ 0x7fffffff));
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}
// does (ov, oi) precede (bv, bi) in that order?
__host__ __device__ inline bool argmax_better(float ov, int oi, float bv, int bi) {
    const int ok = argmax_key(ov), bk = argmax_key(bv);
    return ok > bk || (ok == bk && oi < bi);
}

// ---------------------------------------------------------------------------------------
// One convolution launch.  All tensors are planar NCHW f32; a tensor argument is a base
// pointer + total channel count + first channel, so a launch can read or write a channel
// slice of a wider tensor (the residual block's concat, paulsenpredictor.py:273).
struct ConvArgs {
    // input
    const float* in = nullptr;
    int in_ctot = 0, in_coff = 0;
    int cin = 0, cin_pad = 0;
    int up_in = 0;  // 1: input tensor is [B][C][H/2][W/2], read through nearest 2x upsampling
    const float* pre_scale = nullptr;  // [cin_pad] BN+ReLU applied to the input; null = raw
    const float* pre_shift = nullptr;
    // geometry (output == conv-input spatial size)
    int B = 0, H = 0, W = 0;
    // weights [taps][cin_pad][cout_pad]
    const float* w = nullptr;
    int cout = 0, cout_pad = 0, ksize = 3;
    // 1 + the index in mvlm_ctx::conv_wino4_pads of this layer's F(4,3) weights and bias at a cout stride of whole 32s
    // (mvlm_conv_wino4_padded_cout), where its cout_pad is none and the tile could serve it otherwise; 0: none.  Host only: it sits in
    // the four bytes of padding between ksize and bias, so every field a kernel reads keeps its offset (the static_assert below).
    int wino4_pad = 0;
    const float* bias = nullptr;        // [cout_pad] or null
    const float* post_scale = nullptr;  // [cout_pad] relu(v*s+t) or null
    const float* post_shift = nullptr;
    // residual(s): y = v + (res1 [+ res2])
    const float* res1 = nullptr;
    int res1_ctot = 0, res1_coff = 0;
    const float* res2 = nullptr;
    int res2_ctot = 0, res2_coff = 0;
    // outputs
    float* out_raw = nullptr;  // v (before residual)
    int raw_ctot = 0, raw_coff = 0;
    float* out = nullptr;  // v + residual
    int out_ctot = 0, out_coff = 0;
    // 1: out is [B][out_ctot][2H][2W]; each value is written to its 2x2 block, + skip there
    // 2: out is [B][out_ctot][2H][2W]; the value goes to pixel (2y + sub_y, 2x + sub_x) only
    int up_out = 0;
    int sub_y = 0, sub_x = 0;  // up_out == 2 / ksize == 2: output parity = 2x2 window offset in the halo tile
    // ksize == 2, up_out == 2: all four output parities in one launch (grid x 4): parity pl = 2 sub_y + sub_x uses the
    // weights w_par[pl] and, with a fused argmax, the partials from amax_part0 + pl * amax_par_stride
    int n_par = 1;
    const float* w_par[4] = {nullptr, nullptr, nullptr, nullptr};
    int amax_par_stride = 0;
    const float* skip = nullptr;
    int skip_ctot = 0, skip_coff = 0;
    // consumer-side "upsample x 2 + skip" (round 5; paulsenpredictor.py:334-359 seen from the layer that READS the sum): the
    // input value is in[b][c][y][x] + in2[b][c][y >> 1][x >> 1], in2 = [B][in2_ctot][H/2][W/2] - the hourglass's last block
    // then writes its plain output instead of scattering every value into its 2x2 block of the skip tensor.  Served by the
    // dominant tile only (conv5 / conv9: mvlm_conv_in2_ok).
    const float* in2 = nullptr;
    int in2_ctot = 0;
    // split-K tiles only: input channels divided over `kparts` workgroups per output tile (set by the variant id);
    // kws = partial tiles [tile][part][16][64] f32, kcnt = one arrival counter per tile (zero between launches)
    int kparts = 1;
    float* kws = nullptr;
    unsigned* kcnt = nullptr;
    // fused per-(image, channel) argmax partials (conv11): [B][cout][n_part]
    float* amax_val = nullptr;
    int* amax_idx = nullptr;
    int amax_parts = 0;   // partials per (image, channel) in the buffers
    int amax_part0 = 0;   // first partial this launch writes (parity launches share one buffer)
    // fused 2x2 max-pool of the final values (F.max_pool2d(x, 2, 2), paulsenpredictor.py:304, :413):
    // pool_out is [B][pool_ctot][H/2][W/2]; `out` may be null when only the pooled tensor is consumed
    float* pool_out = nullptr;
    int pool_ctot = 0, pool_coff = 0;
    float fast_unscale = 1.f;  // f16x2 kernel only: inverse of the power-of-two scale its packed weights carry
    int pool_hint = 0;  // the caller wants the pooled tensor too (set for the variant choice, before pool_out is decided; host only)
    unsigned* fast_ovf = nullptr;  // f16x2 kernel only: set to 1 when an activation lies outside fp16's range
    // the layer's weights in the F(4,3) Winograd tile's form ([18][cin_pad][cout_pad], mvlm_pack_winograd4_weights) where it has
    // one (host only, as w_wino below).  It sits where pool_hint and its padding were: the struct is a kernel argument, and
    // every field a kernel reads keeps its offset (see the static_assert below).
    const float* w_wino4 = nullptr;
    // -DMVLM_CONV_TIMING builds only (tools/conv_phase_timing.py): u64[4] = summed cycles of wave 0 in
    // prologue / K loop / epilogue, number of workgroups
    unsigned long long* timing = nullptr;
    // the layer's weights in the Winograd tiles' form ([12][cin_pad][cout_pad], mvlm_pack_winograd_weights) where it has one:
    // mvlm_launch_conv puts it in `w` when it routes the launch to such a tile
    const float* w_wino = nullptr;
};
static_assert(sizeof(ConvArgs) == 360 && offsetof(ConvArgs, wino4_pad) == 84 && offsetof(ConvArgs, bias) == 88 && offsetof(ConvArgs, fast_ovf) == 328 &&
                  offsetof(ConvArgs, timing) == 344,
              "ConvArgs is passed to the kernels by value: moving a field changes the device code of every convolution kernel");

// A layer's F(4,3) weights [18][cin_pad][P] and bias [P] at the cout stride P = mvlm_conv_wino4_padded_cout(cout_pad), zeros beyond
// cout_pad (device pointers; bias null: the layer has none).  ConvArgs::wino4_pad names an entry of mvlm_ctx::conv_wino4_pads.
struct ConvWino4Pad {
    const float* w = nullptr;
    const float* bias = nullptr;
};

struct ConvProfileRec {
    int slot, variant;
    double flops;
    hipEvent_t e0, e1;
    short shape[6] = {0, 0, 0, 0, 0, 0};  // ksize, cin_pad, cout_pad, size, kind (conv_kind), batch; slot -1 = the pool kernel
};

// Dispatch key of a convolution launch beyond its shape: 0 plain / residual-block layer, 1 the value is scattered 2x2 into
// the skip tensor (hourglass way up), 2 the 2x2 max-pooled tensor is wanted as well.  The measured tables and the tuning
// overrides are kept per kind: the epilogues differ, and so does the best tile.
struct ConvOverride {
    short ksize, cin_pad, cout_pad, size, kind;
    int variant;
};
// What the dispatcher looks a launch up by (conv_mfma.hip: mvlm_conv_key); also the shape[6] of a profile record.
struct ConvKey {
    short ksize, cin_pad, cout_pad, size, kind, batch;  // batch: clamped to the 16-bit field of the measured tables
};

// one captured forward pass (hipGraph) of the network for a fixed set of buffers and shapes
struct CnnGraphEntry {
    const void* images = nullptr;
    const void* out = nullptr;   // maxima or heatmap pointer
    const void* ws = nullptr;
    size_t ws_bytes = 0;
    int nb = 0, view0 = 0, n_total = 0, heat = 0;
    int sel4[4] = {0, 0, 0, 0};
    int uses = 0;                // calls seen with this key; the graph is captured on the second one
    hipGraphExec_t exec = nullptr;
};

// The two Winograd forms of a 3x3 layer's weights (conv_pack.h: MVLM_WINO_F23, MVLM_WINO_F43), described once (conv_mfma.hip:
// mvlm_wino_form): what loading, the executor and the dispatcher need to know about a form; conv_pack.cpp makes the weights.  A
// variant's row names its form (ConvVariantInfo::form).
struct WinoForm {
    bool (*serves_slot)(int ksize, int cin_pad, int cout_pad);                   // a tile of this form exists for these channels
    const float* ConvArgs::*weights;                                             // the launch's member that carries them
    double macs;                                                                 // multiply-adds per output and input channel (direct: 9)
    const char* pack_fn;                                                         // the C entry point that makes them, for messages
};
const WinoForm& mvlm_wino_form(int form);

// One row of the network's descriptor table by name (mvlm_amd/weights.py: pack_for_device): the *_off fields are float offsets
// into the packed weights, -1 absent.
struct ConvSlotDesc {
    int32_t present, cin, cout, ksize, cin_pad, cout_pad, w_off, bias_off, pre_scale_off, pre_shift_off, post_scale_off, post_shift_off;
};
static_assert(sizeof(ConvSlotDesc) == MVLM_CONV_DESC_INTS * sizeof(int32_t), "a row is the 12 ints of include/mvlm_hip.h");
// The table's slots (mvlm_amd/arch.py: conv_slots): conv1, four per residual block (the 1x1 resample, conv1..conv3) of the 43
// blocks, conv5..conv11 (conv8 is dead at inference and has no slot), conv11's four output parities as 2x2 layers.
enum {
    MVLM_SLOT_CONV5 = 1 + 4 * 43,
    MVLM_SLOT_CONV6,
    MVLM_SLOT_CONV7,
    MVLM_SLOT_CONV9,
    MVLM_SLOT_CONV10,
    MVLM_SLOT_CONV11,
    MVLM_SLOT_PARITY0,
    MVLM_N_SLOTS = MVLM_SLOT_PARITY0 + 4,
};
static_assert(MVLM_N_SLOTS == 183, "the descriptor table has 183 conv slots");

struct CnnState {
    bool loaded = false;
    int n_landmarks = 0, in_channels = 0;
    float* blob = nullptr;  // device copy of the packed weights
    std::vector<ConvSlotDesc> desc;  // host copy of the descriptor table
    bool profiling = false;
    std::vector<ConvProfileRec> prof;
    std::vector<hipEvent_t> event_pool;
    size_t event_cursor = 0;
    // second stream + fork / join events of the executor (created on first use), captured graphs
    hipStream_t side_stream = nullptr;
    hipStream_t capture_stream = nullptr;  // passes are recorded here (the caller's stream may be the null stream)
    std::vector<hipEvent_t> sync_events;
    size_t sync_cursor = 0;
    int graph_mode = 1;            // 0: always eager, 1: replay captured graphs when not profiling
    int concurrency = 0;           // 0: one stream (default), 1: lower hourglass pyramid on a side stream (small batches)
    int selection = 0;             // heatmap maxima of mvlm_cnn_maxima: 0 "simple" (argmax pixel), 1 "moment" (31x31 centroid around it)
    int pairing = 1;               // independent residual blocks of a hourglass level share launches: 0 never, 1 where the measured
                                   // table says so (default), 2 wherever one kernel variant can serve both (tests, tuning)
    // opt-in "fast" precision (conv_fast.hip): bf16x3-split weights of the eligible 3x3 layers, per conv slot
    unsigned short* fast_blob = nullptr;
    std::vector<long long> fast_off;   // u16 element offset per slot, -1 = the layer stays on the exact kernel
    int fast = 0;                      // 1: eligible layers run on the bf16x3 kernel, 2: on the f16x2 kernel
    unsigned short* fast16_blob = nullptr;   // the f16x2 form's packed weights, offsets and per-layer inverse scales
    std::vector<long long> fast16_off;
    std::vector<float> fast16_unscale;
    unsigned* fast16_flag = nullptr;         // device word: an f16x2 launch of the current pass met |x| >= 65504
    // per Winograd form, the transformed weights of the 3x3 slots a tile of that form can serve (exact path) and the float offset
    // per slot (-1: none)
    struct WinoWeights {
        float* blob = nullptr;
        std::vector<long long> off;
    } wino[MVLM_WINO_FORMS_N];
    // the F(4,3) form at a cout stride of whole 32s, and the bias alike, of the slots whose cout_pad is no multiple of 32 (conv6 /
    // conv10 on 80 or 84 rows), and per slot the ConvArgs::wino4_pad that names its entry of mvlm_ctx::conv_wino4_pads (0: none)
    float* wino4_pad_blob = nullptr;
    std::vector<int> wino4_pad_id;
    std::vector<CnnGraphEntry> graphs;
    long graph_replays = 0, graph_captures = 0, eager_runs = 0, graph_failures = 0;
    // forget the captured passes: they encode the kernels, their order and pointers into the weight blobs
    void drop_graphs() {
        for (CnnGraphEntry& g : graphs)
            if (g.exec) hipGraphExecDestroy(g.exec);
        graphs.clear();
    }
};

struct mvlm_mesh {
    float* verts = nullptr;   // [V,3]
    float* uvs = nullptr;     // [V,2] or null
    int32_t* tris = nullptr;  // [T,3]
    uint8_t* tex = nullptr;   // [H,W,3] or null
    uint8_t* colors = nullptr;  // [V,4] per-vertex r g b 255 (one aligned 4-byte load per vertex) or null: mvlm_mesh_upload_colors
    float* normals = nullptr;   // [V,3] per-point normals of a cloud or null: mvlm_mesh_upload_normals, mvlm_mesh_estimate_normals
    float* normals_buf = nullptr;  // the buffer they live in, allocated on first use (api.hip: mvlm_mesh_normals_buffer); normals is it or null
    int n_verts = 0, n_tris = 0, tex_h = 0, tex_w = 0;
    // a point mesh (n_tris == 0, tris == null; raster_points_math.h): the splat radius in model units, the same in lattice
    // steps and the paraboloid's coefficient - the automatic radius at upload, mvlm_mesh_set_point_radius replaces it
    double point_radius = 0.0;
    int32_t point_R = 0;
    float point_c = 0.f;
    unsigned long long uid = 0;  // unique per upload (an address can be recycled): key of per-mesh derived data a context keeps
    size_t cap[6] = {0, 0, 0, 0, 0, 0};  // allocation sizes of verts / uvs / tris / tex / colors / normals (for the ctx's mesh pool)
    // recorded on the context's upload stream behind the host-to-device copies (again behind the colours' copy, when they
    // follow); every consumer's stream waits for it
    hipEvent_t ready = nullptr;
    hipEvent_t waited[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // "previous owner is done" events of recycled buffers
};

struct RenderProfileRec {
    int n_views, n_verts, n_tris;
    hipEvent_t e0, e1;
};

// per-thread copy of the last error message and the context it belongs to (api.hip: mvlm_last_error)
inline std::string& mvlm_thread_error() {
    thread_local std::string s;
    return s;
}
inline const void*& mvlm_thread_error_ctx() {
    thread_local const void* c = nullptr;
    return c;
}

struct mvlm_ctx;

// The HIP events round one feature's stages while mvlm_render_set_profiling is on, and how many of them the last call that ran
// through recorded (0: none).  Host only; a plain member of mvlm_ctx per feature, freed with the context by its destructor
// (mvlm_ctx_destroy has made the device current by then).  A launch function invalidates, arms, records between its stages and
// marks at its end; the feature's mvlm_*_stage_ms entry point reads.  (The bodies follow mvlm_ctx::fail below.)
struct StageClock {
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock() {
        for (hipEvent_t e : events) hipEventDestroy(e);
    }
    void invalidate() { recorded = 0; }  // nothing recorded from here on
    // Profiling off: off, and record() enqueues nothing until the next arm().  On: n events exist (those it has are kept).
    int arm(mvlm_ctx* ctx, int n);
    int record(mvlm_ctx* ctx, int k, hipStream_t stream);              // event k behind what the stream holds; a no-op when off
    hipEvent_t event(int k) const { return armed ? events[k] : nullptr; }  // for a launcher that records it itself; null when off
    void mark(int n) { recorded = armed ? n : 0; }                     // the end of a call that ran through
    // the m stage times between the m + 1 events of the last call; refuses with `none` unless that call marked m + 1; waits for the stream
    int read(mvlm_ctx* ctx, int m, float* ms, const char* none);

private:
    std::vector<hipEvent_t> events;
    int recorded = 0;
    bool armed = false;
};

struct mvlm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // where the network executor's launchers enqueue right now: null = `stream`; the executor points it at
    // its side stream while it issues the branch of the graph that runs beside the main one (cnn_graph.hip)
    hipStream_t launch_stream = nullptr;
    hipStream_t cur_stream() const { return launch_stream ? launch_stream : stream; }
    // mvlm_set_stream: orders the context's work across a change of stream.  A context that has only ever run on the null
    // stream (which cannot be destroyed) records nothing; from its first change of stream on, every entry point leaves
    // switch_event behind the work it enqueued (MvlmOrderGuard), so a later change never touches the previous stream's
    // handle - its owner may have destroyed it by then.
    // surface snap: which upload the scratch's de-indexed triangle copy and vertex -> triangle table were made for
    unsigned long long snap_mesh_uid = 0;
    const void* snap_soup = nullptr;
    const void* snap_vert_tri = nullptr;
    hipEvent_t switch_event = nullptr;
    bool track_order = false;      // the context has been moved between streams: record switch_event at every exit
    bool order_recorded = false;   // switch_event stands behind everything enqueued so far
    std::mutex mu;
    std::string err;
    CnnState cnn;
    // grow-only internal scratch (raster bins, transformed vertices, small staging)
    std::map<std::string, std::pair<void*, size_t>> scratch;
    float* kparts_ws[2] = {nullptr, nullptr};      // split-K over workgroups: partial tiles, arrival counters
    unsigned* kparts_cnt[2] = {nullptr, nullptr};  // ([0] main launch stream, [1] the executor's side stream)
    int conv_force_variant = -1;            // >= 0: mvlm_conv_bench times exactly this kernel variant
    // Winograd tiles on the exact path: 0 never, 1 where the measured table (conv_tuned_wino.h) has an entry, 2 every layer a
    // Winograd variant can serve (tests); a new context takes MVLM_WINOGRAD from the environment (default 1)
    int conv_winograd = [] { const char* e = getenv("MVLM_WINOGRAD"); return (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : 1; }();
    // the F(4,3) Winograd tile, where Winograd mode is not 0 and the launch carries ConvArgs::w_wino4: 0 never, 1 where the measured
    // table (conv_tuned_wino4.h) has an entry and Winograd mode is 1, 2 every layer the tile can serve (tests); MVLM_WINOGRAD4 (default 1)
    int conv_winograd4 = [] { const char* e = getenv("MVLM_WINOGRAD4"); return (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : 1; }();
    // the workgroup shape of the F(4,3) tile's launches (the dispatcher decides, conv_mfma.hip: f43_plan): 1 the wide shape, 64 output channels
    // x 8 rows on one staged input tile, where cout_pad is a multiple of 64; 0 the 32 x 16 shape on every launch; MVLM_WINOGRAD4_WIDE (default 1)
    int conv_winograd4_wide = [] { const char* e = getenv("MVLM_WINOGRAD4_WIDE"); return (e && e[0] >= '0' && e[0] <= '1' && !e[1]) ? e[0] - '0' : 1; }();
    long long conv_wino4_wide_launches = 0;  // launches issued on the wide shape (mvlm_conv_wino4_wide_launches)
    // The dispatcher runs an eligible launch of the 80- and 84-row direct tiles (variants 16 and 26) on the F(4,3) tile over weights
    // padded to whole 32-channel columns (conv_mfma.hip: f43_plan): 0 never, 1 where the measured table
    // conv_tuned_wino4_pad.h has a row, 2 every eligible launch (tests); MVLM_WINOGRAD4_PADDED (default 1)
    int conv_winograd4_padded = [] { const char* e = getenv("MVLM_WINOGRAD4_PADDED"); return (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : 1; }();
    long long conv_wino4_padded_launches = 0;  // launches run that way (mvlm_conv_wino4_padded_launches)
    // the padded weights such launches read: [0] the layer of the mvlm_conv2d / mvlm_conv_bench call in flight, then the loaded
    // network's slots (mvlm_cnn_load); ConvArgs::wino4_pad is 1 + the index
    std::vector<ConvWino4Pad> conv_wino4_pads = std::vector<ConvWino4Pad>(1);
    std::vector<ConvOverride> conv_overrides;  // tools/tune_in_network.py: kernel variant per (shape, kind), before any table
    // Conv kernels whose launch attributes are set on this ctx's device.  The 64 bits: a base variant's bit is its id (all below
    // MVLM_CONV_FAST_ATTR_BIT0, none MVLM_CONV_WINO4_ATTR_BIT or MVLM_CONV_WINO4_WIDE_ATTR_BIT: conv_mfma.hip asserts it), the F(4,3)
    // tile has bit 41 and its wide shape bit 42, the fast kernels (conv_fast.hip) the bits from 54 on.
    unsigned long long conv_attr_mask = 0;
    // a depth-key plane's buffer and capacity when it was last left all-EMPTY ({nullptr, 0}: not known clean); keyed on both,
    // so a buffer that get_scratch replaced by one of the same size is filled again
    struct KeyPlaneState {
        const void* ptr = nullptr;
        size_t cap = 0;
    };
    KeyPlaneState raster_keys_clean;   // "raster.keys": one key per pixel
    KeyPlaneState raster_keys4_clean;  // "raster.keys4": four per pixel (multisampling)
    int render_subpixel_bits = 8;  // vertex snap 2^-bits pixel (GL_SUBPIXEL_BITS of the OpenGL to match)
    int render_multisamples = 0;   // 0: one sample at the pixel centre (the default contract); 4: four samples per pixel
    int render_shading = 0;  // 0: unlit nearest-texel RGB (reference), 1: build-defined geometry shading
    int* render_overflow_host = nullptr;  // pinned; written asynchronously by mvlm_render
    bool points_counting = false;  // mvlm_points_set_counting: a cloud's splat kernel also counts covered pixels and atomics
    bool render_profiling = false;        // mvlm_render_set_profiling: HIP events around each render's kernels
    std::vector<RenderProfileRec> render_prof;
    std::vector<hipEvent_t> render_events;
    size_t render_event_cursor = 0;
    // under render profiling, one clock per feature (a new feature: a member here, its calls in the launch function, one read)
    StageClock points_clock;     // a cloud's render (raster.hip): splat, tile; mvlm_points_stage_ms
    StageClock normals_clock;    // a cloud's normal estimate (cloud_normals.hip): grid build, search, solve; mvlm_normals_stage_ms
    StageClock cloudmesh_clock;  // a cloud's triangulation (cloud_mesh.hip): star, count + scan, emit; mvlm_cloud_mesh_stage_ms
    // the landmark view (raster_view.hip: seven stages, copies and fills first, eight events; mvlm_landmark_view_stage_ms) and the
    // ray view (raster_rays.hip: eight stages, nine events; mvlm_ray_view_stage_ms) share one: each reader refuses after the other's call
    StageClock view_clock;
    StageClock png_clock;          // the PNG encoder (png_encode.hip): its four stages; mvlm_png_stage_ms
    StageClock heat_clock;         // the heat sheet (heat_sheet.hip): background, peak, compose; mvlm_heat_sheet_stage_ms
    StageClock backproject_clock;  // the surface heat (surface_backproject.hip): peak, score, paint; mvlm_surface_heat_stage_ms
    // the surface distances (geodesic.hip): attachment + adjacency first, then init, sweeps and targets of each of the last call's
    // geodesic_groups source groups (2 + 3 groups events); mvlm_geodesic_stage_ms adds the groups up
    StageClock geodesic_clock;
    int geodesic_groups = 0;
    // device buffers of freed meshes, reused by the next upload: a folder of scans would otherwise pay
    // four hipMalloc + four (device-synchronising) hipFree per scan
    struct PoolEntry {
        void* p;
        size_t cap;
        hipEvent_t freed;  // recorded on the launch stream when the owning mesh was freed: work enqueued before may read p
    };
    std::vector<PoolEntry> mesh_pool;  // oldest first
    size_t mesh_pool_bytes = 0;
    // mesh uploads: pinned staging (two slots) -> hipMemcpyAsync on a stream of their own, so a reader thread's upload of
    // the next scan runs beside the current scan's kernels and never makes a host wait for the launch stream
    std::mutex upload_mu;  // staging slots + upload stream; taken before `mu`, never the other way round
    hipStream_t upload_stream = nullptr;
    void* upload_stage[2] = {nullptr, nullptr};
    size_t upload_stage_cap[2] = {0, 0};
    hipEvent_t upload_stage_done[2] = {nullptr, nullptr};
    int upload_stage_next = 0;
    // JPEG textures decoded on the device (jpeg.hip): scratch of the upload path, guarded by upload_mu
    void* jpeg_scratch = nullptr;
    size_t jpeg_scratch_cap = 0;
    int32_t* jpeg_flags_host = nullptr;  // pinned
    std::vector<hipEvent_t> event_free;  // recycled (timing-disabled) events
    hipEvent_t take_event() {
        if (!event_free.empty()) {
            hipEvent_t e = event_free.back();
            event_free.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        return e;
    }
    // The message of a failed call belongs to the calling thread: reader threads upload meshes while another thread
    // launches (predict_files), and both may fail.  `err` keeps the context's latest message (under err_mu) for a
    // thread that has none of its own; mvlm_last_error hands out the calling thread's copy.
    std::mutex err_mu;
    int fail(const std::string& m);
    void* get_scratch(const char* name, size_t bytes);
};

inline int mvlm_ctx::fail(const std::string& m) {
    {
        std::lock_guard<std::mutex> lock(err_mu);
        err = m;
    }
    mvlm_thread_error() = m;
    mvlm_thread_error_ctx() = this;
    return 1;
}

inline int StageClock::arm(mvlm_ctx* ctx, int n) {
    armed = false;
    if (!ctx->render_profiling) return 0;
    while (int(events.size()) < n) {
        hipEvent_t e = nullptr;
        MVLM_CHECK_HIP(ctx, hipEventCreate(&e));
        events.push_back(e);
    }
    armed = true;
    return 0;
}
inline int StageClock::record(mvlm_ctx* ctx, int k, hipStream_t stream) {
    if (armed) MVLM_CHECK_HIP(ctx, hipEventRecord(events[k], stream));
    return 0;
}
inline int StageClock::read(mvlm_ctx* ctx, int m, float* ms, const char* none) {
    if (recorded != m + 1) return ctx->fail(none);
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < m; ++k) MVLM_CHECK_HIP(ctx, hipEventElapsedTime(&ms[k], events[k], events[k + 1]));
    return 0;
}

// End of every entry point (declared by MVLM_ENTER, destroyed before the context's mutex is released): once a context has
// been moved between streams, leave switch_event behind whatever this call enqueued on the current one.
struct MvlmOrderGuard {
    mvlm_ctx* ctx;
    ~MvlmOrderGuard() {
        if (!ctx->track_order || !ctx->switch_event) return;
        if (hipEventRecord(ctx->switch_event, ctx->stream) == hipSuccess)
            ctx->order_recorded = true;
        else
            (void)hipGetLastError();
    }
};

// a mesh's device copy is complete once its `ready` event has fired: consumers make their stream wait for it
inline int mvlm_mesh_wait_ready(mvlm_ctx* ctx, const mvlm_mesh* m, hipStream_t stream) {
    if (m->ready && hipStreamWaitEvent(stream, m->ready, 0) != hipSuccess) return ctx->fail("mesh: hipStreamWaitEvent failed");
    return 0;
}

// jpeg.hip (the host parser and its declarations: jpeg_plan.h / jpeg_plan.cpp)
int mvlm_jpeg_run(mvlm_ctx* ctx, MvlmJpegPlan& plan, const uint8_t* stage_pinned, uint8_t* rgb_dev, hipStream_t stream,
                  std::string& why, int* rounds_out);

// view_sheet.hip: mvlm_render_view_sheet behind its MVLM_ENTER, for an entry point that has entered the context itself
int mvlm_view_sheet_draw(mvlm_ctx* ctx, const float* images_dev, int n_views, const float* maxima_dev, int n_lm, const double* rot_host,
                         const double* landmarks_host, const uint8_t* lm_rgb_host, const uint8_t* used_host, int background, int cols_in,
                         int scale, int gap, double marker_radius, uint8_t* out_dev);

// heat_sheet.hip: the launch of the kernel behind mvlm_heat_plane_peaks, for an entry point that holds the context
void mvlm_heat_launch_peaks(mvlm_ctx* ctx, const float* heat_dev, int n_planes, float* peaks_dev);

// conv_mfma.hip
constexpr long MVLM_KPARTS_MAX_TILES = 2048;  // output tiles of a launch that divides K over workgroups
constexpr long MVLM_KPARTS_MAX_PARTS = 4096;  // tiles x parts (4 KB of partial sums each)
int mvlm_conv_kparts_workspace(mvlm_ctx* ctx, float** ws, unsigned** cnt);
int mvlm_launch_conv(mvlm_ctx* ctx, const ConvArgs& a, int* variant_out);
bool mvlm_conv_in2_ok(const mvlm_ctx* ctx, const ConvArgs& a);  // this launch would run on the tile that can add ConvArgs::in2 on its load
bool mvlm_conv_can_pool(const mvlm_ctx* ctx, const ConvArgs& a);  // the variant this launch would use can also emit the 2x2 max-pooled tensor
int mvlm_conv_kind(const ConvArgs& a);
ConvKey mvlm_conv_key(const ConvArgs& a);
bool mvlm_conv_variant_can_pool(int variant);
bool mvlm_conv_variant_is_wino(int variant);   // an F(2,3) Winograd tile (reads ConvArgs::w_wino)
bool mvlm_conv_variant_is_wino4(int variant);  // the F(4,3) Winograd tile (reads ConvArgs::w_wino4)
// the Winograd variant this launch is routed to (overrides, mode and table of the context), or -1: the direct tiles
int mvlm_conv_wino_variant(const mvlm_ctx* ctx, const ConvArgs& a);
bool mvlm_conv_wino_serves_slot(int ksize, int cin_pad, int cout_pad);  // a Winograd variant exists for these channels
bool mvlm_conv_wino4_serves_slot(int ksize, int cin_pad, int cout_pad);  // the F(4,3) tile can serve these channels
// two independent convolutions in one grid (conv_tile.h: conv_pair_kernel)
constexpr int MVLM_CONV_PAIR_FLAG = 0x1000;  // variant code of a paired launch: flag | base id | lg(kparts0) << 8 | lg(kparts1) << 10
int mvlm_conv_pair_variant(const ConvArgs& a0, const ConvArgs& a1, int mode);
int mvlm_launch_conv_pair(mvlm_ctx* ctx, const ConvArgs& a0, const ConvArgs& a1, int pair_variant);
int mvlm_conv_amax_parts(int H, int W);  // partials per (image, channel) the argmax epilogue writes
const char* mvlm_conv_variant_name_impl(int v);

// conv_fast.hip (opt-in reduced-cost arithmetic)
// channel paddings of the opt-in bf16x3 kernel (its split weights are packed separately from the exact ones): 16-channel
// k-chunks, 64-channel tiles.  Served: 16..256 input channels, output padding waste of at most 1.6x (84 -> 128 yes, 32 -> 64 no).
inline int mvlm_fast_cin_pad(int cin) { return (cin + 15) / 16 * 16; }
inline int mvlm_fast_cout_pad(int cout) { return cout <= 32 ? 32 : (cout + 63) / 64 * 64; }  // (32: the f16x2 form's 32-channel tile)
inline bool mvlm_fast_channels_ok(int cin, int cout) {
    return cin >= 16 && cin <= 256 && cout > 0 && cout * 8 >= mvlm_fast_cout_pad(cout) * 5;
}
bool mvlm_conv_fast_ok(const ConvArgs& a, int splits);  // splits: 3 = bf16x3 ("fast"), 2 = f16x2 ("fast16")
int mvlm_launch_conv_fast(mvlm_ctx* ctx, const ConvArgs& a, const unsigned short* wq_dev, int splits = 3, float unscale = 1.f);
// the F(4,3) Winograd tile (conv3x3q_c32_t16x32): a code beyond the base ids and their K-part forms (0..1023) and below the pair
// flag - a row of the variant table like the others (conv_mfma.hip: decode_variant reads the code), and a bit of conv_attr_mask
constexpr int MVLM_CONV_VARIANT_WINO4 = 2048;
constexpr int MVLM_CONV_WINO4_ATTR_BIT = 41, MVLM_CONV_WINO4_WIDE_ATTR_BIT = 42, MVLM_CONV_FAST_ATTR_BIT0 = 54;
// The wide shape of that tile (conv_inst_q1.hip: 64 output channels x 8 rows x 32 pixels on one staged input tile) is no variant of
// its own: the dispatcher takes it for code 2048 where the context's switch is on and the layer's output channels come in 64s.  Everything
// else about the layer is what the 32 x 16 shape asks, so this is asked of launches already routed to code 2048.
inline bool mvlm_conv_wino4_wide_shape_ok(int cout_pad, int H) { return cout_pad > 0 && cout_pad % 64 == 0 && H % 16 == 0; }
// Does a 3x3 slot of these channels get padded F(4,3) weights: the tile would serve it but for cout_pad % 32 != 0?
inline bool mvlm_conv_wino4_pad_serves_slot(int ksize, int cin_pad, int cout_pad) {
    return cout_pad > 0 && cout_pad % 32 != 0 && mvlm_conv_wino4_serves_slot(ksize, cin_pad, mvlm_conv_wino4_padded_cout(cout_pad));
}
constexpr int MVLM_CONV_VARIANT_FAST = 62;    // id reported for launches of the bf16x3 kernel
constexpr int MVLM_CONV_VARIANT_FAST16 = 61;  // ... of the f16x2 kernel

// raster_view.hip: the launch set of mvlm_render_landmark_view (api.hip checks the arguments and holds the context); with
// vert_rgba_dev u8[V,4] (mvlm_render_landmark_view_colored) the tile kernel shades with those colours: no texture, shading 0
int mvlm_launch_landmark_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                              const float* frames_host, const double* landmarks_host, int n_lm, float radius,
                              const uint8_t* lm_rgb_host, uint8_t* out_dev, int32_t* lm_pixels_dev,
                              const uint8_t* vert_rgba_dev = nullptr);

// raster_rays.hip: the launch set of mvlm_render_ray_view (likewise)
int mvlm_launch_ray_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                         const float* frames_host, const double* landmarks_host, int n_lm, float radius, const uint8_t* lm_rgb_host,
                         const double* starts_dev, const double* ends_dev, int n_rays, float ray_radius, const uint8_t* ray_rgb_host,
                         uint8_t* out_dev, int32_t* lm_pixels_dev, int32_t* ray_pixels_dev);

// surface.hip: passes 0 and 1 of the surface snap (bound, de-indexed triangles, per-chunk winners in the context's scratch)
// for an entry point that holds the context; its final kernel follows (mvlm_project_to_surface, mvlm_surface_attach)
int mvlm_project_partials(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points, int* n_chunks_out,
                          const double** part_d_out, const int** part_t_out);

// surface_attach.hip: mvlm_surface_attach behind its MVLM_ENTER, for an entry point that holds the context (geodesic.hip)
int mvlm_launch_surface_attach(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points, double* snapped_dev,
                               int32_t* tri_dev, double* bary_dev, double* uv_dev);

// surface_points.hip: the snap of a point mesh (n_tris == 0) - the nearest point - for mvlm_project_to_surface, which holds the context
int mvlm_points_nearest(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* pts_dev, int n_points, double* out_dev);
// raster_points.hip: the automatic splat radius of a cloud (host only; exported, include/mvlm_hip.h)
extern "C" int mvlm_points_auto_radius(const float* verts, int n, double* r_out);

// api.hip: the buffer a cloud's normals go to, f32[V,3] - the mesh's own when it has normals already, else one from the mesh pool
// (recorded in cap[5] / waited[5]; the caller sets mesh->normals once the normals are on their way).  The caller holds ctx->mu.
float* mvlm_mesh_normals_buffer(mvlm_ctx* ctx, mvlm_mesh* mesh);

// small kernels (misc.hip)
int mvlm_launch_pack_input(mvlm_ctx* ctx, const float* images, int n, const int* sel4, int c, float* out);
int mvlm_launch_maxpool2(mvlm_ctx* ctx, const float* in, int planes, int H, int W, float* out);
int mvlm_launch_amax_final(mvlm_ctx* ctx, const float* val, const int* idx, int n_img, int view0, int n_views_total,
                           int nl, int parts, int size, float* maxima, int* best_idx = nullptr);
// "moment" refinement of the fused argmax's peaks from conv10's output (misc.hip: moment_refine_kernel)
// f16x2 precision: where *flag != 0 the pass's maxima scores (or the first heatmap value of every plane) become NaN
int mvlm_launch_fp16_poison(mvlm_ctx* ctx, const unsigned* flag, float* maxima, int n_img, int view0, int n_views_total, int nl,
                            float* heat);
int mvlm_launch_moment_refine(mvlm_ctx* ctx, const float* x10, int n_img, int nl, int cin_pad, int cout_pad, const float* const w_par[4],
                              const float* bias, const int* best_idx, int view0, int n_views_total, float* maxima);
