// Context and mesh upload of the C ABI (include/mvlm_hip.h); the single-convolution hooks are conv_hooks.hip.
#include <atomic>
#include <cstring>

#include <memory>

#include <cmath>

#include "common.h"
#include "raster_points_math.h"
#include "raster_view_math.h"

void* mvlm_ctx::get_scratch(const char* name, size_t bytes) {
    auto& e = scratch[name];
    if (e.second >= bytes && e.first) return e.first;
    if (e.first) {
        hipStreamSynchronize(stream);
        hipFree(e.first);
        e = {nullptr, 0};
    }
    void* p = nullptr;
    const size_t want = bytes + bytes / 4 + 256;  // headroom so growing view counts do not realloc every call
    if (hipMalloc(&p, want) != hipSuccess) return nullptr;
    e = {p, want};
    return p;
}

extern "C" const char* mvlm_build_arch(void) { return "gfx950"; }

extern "C" int mvlm_ctx_create(int device, mvlm_ctx** out) {
    if (!out) return 1;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return 2;
    if (hipSetDevice(device) != hipSuccess) return 3;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 4;
    auto* ctx = new mvlm_ctx();
    ctx->device = device;
    // the code objects in this library exist for gfx950 only - refuse anything else loudly
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        fprintf(stderr, "mvlm_hip: device %d is %s, this library is built for gfx950 (MI355X) only\n", device,
                prop.gcnArchName);
        delete ctx;
        return 5;
    }
    *out = ctx;
    return 0;
}

extern "C" void mvlm_ctx_destroy(mvlm_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->scratch)
        if (kv.second.first) hipFree(kv.second.first);
    if (ctx->cnn.blob) hipFree(ctx->cnn.blob);
    if (ctx->cnn.fast_blob) hipFree(ctx->cnn.fast_blob);
    if (ctx->cnn.fast16_blob) hipFree(ctx->cnn.fast16_blob);
    for (auto& ww : ctx->cnn.wino)
        if (ww.blob) hipFree(ww.blob);
    if (ctx->cnn.wino4_pad_blob) hipFree(ctx->cnn.wino4_pad_blob);
    if (ctx->cnn.fast16_flag) hipFree(ctx->cnn.fast16_flag);
    if (ctx->switch_event) hipEventDestroy(ctx->switch_event);
    for (int i = 0; i < 2; ++i) {
        if (ctx->kparts_ws[i]) hipFree(ctx->kparts_ws[i]);
        if (ctx->kparts_cnt[i]) hipFree(ctx->kparts_cnt[i]);
    }
    for (auto& e : ctx->mesh_pool) {
        hipFree(e.p);
        if (e.freed) hipEventDestroy(e.freed);
    }
    for (hipEvent_t e : ctx->event_free) hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (ctx->upload_stage[i]) hipHostFree(ctx->upload_stage[i]);
        if (ctx->upload_stage_done[i]) hipEventDestroy(ctx->upload_stage_done[i]);
    }
    if (ctx->upload_stream) hipStreamDestroy(ctx->upload_stream);
    if (ctx->jpeg_scratch) hipFree(ctx->jpeg_scratch);
    if (ctx->jpeg_flags_host) hipHostFree(ctx->jpeg_flags_host);
    if (ctx->render_overflow_host) hipHostFree(ctx->render_overflow_host);
    for (auto e : ctx->cnn.event_pool)
        if (e) hipEventDestroy(e);
    for (auto e : ctx->render_events)
        if (e) hipEventDestroy(e);
    for (auto e : ctx->cnn.sync_events)
        if (e) hipEventDestroy(e);
    ctx->cnn.drop_graphs();
    if (ctx->cnn.side_stream) hipStreamDestroy(ctx->cnn.side_stream);
    if (ctx->cnn.capture_stream) hipStreamDestroy(ctx->cnn.capture_stream);
    delete ctx;  // (and with it every feature's StageClock and its events: the device is current, above)
}

// The calling thread's last failure on this context (valid until that thread's next failing call); a thread without
// one of its own gets a private copy of the context's latest message - never a pointer into a string another thread
// may be reassigning.
extern "C" const char* mvlm_last_error(mvlm_ctx* ctx) {
    if (!ctx) return "null context";
    if (mvlm_thread_error_ctx() != ctx) {
        std::lock_guard<std::mutex> lock(ctx->err_mu);
        mvlm_thread_error() = ctx->err;
        mvlm_thread_error_ctx() = ctx;
    }
    return mvlm_thread_error().c_str();
}

// A context owns grow-only scratch (render bins and keys, transformed vertices, fusion staging) that its kernels reuse from
// call to call: safe while the calls are ordered on one stream.  Callers that move a context to ANOTHER stream (two
// pipelines of one device under different torch streams share the process-wide context) get that order kept for them: the
// new stream waits for everything the context enqueued before.  The event it waits for was recorded at the END of the
// previous entry points (MvlmOrderGuard), never here on the previous stream's handle - its owner may have destroyed that
// stream since.  Only the very first change records here: until then the context has lived on the stream it was created
// with, the null stream, which is never destroyed.
extern "C" int mvlm_set_stream(mvlm_ctx* ctx, void* hip_stream) {
    MVLM_ENTER(ctx);
    hipStream_t next = static_cast<hipStream_t>(hip_stream);
    if (next != ctx->stream) {
        if (!ctx->switch_event) MVLM_CHECK_HIP(ctx, hipEventCreateWithFlags(&ctx->switch_event, hipEventDisableTiming));
        if (!ctx->track_order) {
            MVLM_CHECK_HIP(ctx, hipEventRecord(ctx->switch_event, ctx->stream));  // (ctx->stream is still the null stream)
            ctx->order_recorded = true;
            ctx->track_order = true;
        }
        if (ctx->order_recorded) MVLM_CHECK_HIP(ctx, hipStreamWaitEvent(next, ctx->switch_event, 0));
    }
    ctx->stream = next;
    return 0;  // (the guard now records the event on the new stream: harmless, and it keeps "recorded" true)
}

extern "C" int mvlm_synchronize(mvlm_ctx* ctx) {
    MVLM_ENTER(ctx);
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// A device buffer for `room` bytes on the upload path (caller holds ctx->mu): the OLDEST pooled buffer that fits - its
// previous owner's work finished long ago, so the wait is a no-op and the copy really runs beside the current scan's
// kernels - or a new allocation.  `waited`: the previous owner's event (goes back to the event list with the new owner).
static bool take_upload_buffer(mvlm_ctx* ctx, size_t bytes, size_t room, void** p, size_t* cap, hipEvent_t* waited) {
    int pick = -1;
    for (int k = 0; k < int(ctx->mesh_pool.size()); ++k) {
        const size_t c = ctx->mesh_pool[size_t(k)].cap;
        if (c >= room && c <= 4 * bytes + (1u << 20)) {
            pick = k;
            break;
        }
    }
    if (pick >= 0) {
        const auto e = ctx->mesh_pool[size_t(pick)];
        ctx->mesh_pool.erase(ctx->mesh_pool.begin() + pick);
        ctx->mesh_pool_bytes -= e.cap;
        *p = e.p;
        *cap = e.cap;
        *waited = e.freed;
        return !(e.freed && hipStreamWaitEvent(ctx->upload_stream, e.freed, 0) != hipSuccess);
    }
    *cap = (room + 65535) / 65536 * 65536;
    if (hipMalloc(p, *cap) != hipSuccess) {
        *p = nullptr;
        *cap = 0;
        return false;
    }
    return true;
}

// a texture decoded ahead of its mesh (mvlm_texture_from_jpeg): the buffer a mesh upload takes over
struct mvlm_texture {
    uint8_t* dev = nullptr;
    size_t cap = 0;
    int h = 0, w = 0;
    hipEvent_t waited = nullptr;
};

// jpeg != null: the texture is decoded on the device from the staged JPEG (jpeg.hip) instead of copied from tex_host;
// pre != null: the texture is already on the device (mvlm_texture_from_jpeg) and its buffer becomes the mesh's;
// returns 2 (and no mesh) when the stream turns out not to decode - the caller then decodes on the host
static int mesh_upload_impl(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts, const int32_t* tris_host,
                            int n_tris, const uint8_t* tex_host, int tex_h, int tex_w, MvlmJpegPlan* jpeg,
                            const uint8_t* jpeg_bytes, size_t jpeg_n, mvlm_mesh** out, mvlm_texture* pre = nullptr) {
    // Called from reader threads while another thread launches kernels on this context.  The host work - index
    // validation (O(3T)), waiting for a staging slot, a possible hipHostMalloc, the 10-25 MB memcpy into pinned memory -
    // runs under the upload mutex only; the context mutex every launch entry point takes is held just for the pool
    // pick, the asynchronous copies and the event records.
    MVLM_REQUIRE(ctx, out, "mesh_upload: null output");
    *out = nullptr;
    // n_tris == 0 (tris_host may be null): a point mesh - the points alone, drawn as splats and snapped to the nearest point
    MVLM_REQUIRE(ctx, verts_host && n_verts > 0 && n_tris >= 0 && (tris_host || n_tris == 0), "mesh_upload: mesh does not contain any points");
    MVLM_REQUIRE(ctx, n_tris > 0 || !(jpeg || pre), "mesh_upload: a point cloud (n_tris == 0) takes no texture");
    if (n_tris == 0) {  // a texture or uvs on a faceless mesh are ignored
        uvs_host = nullptr;
        tex_host = nullptr;
    }
    MVLM_REQUIRE(ctx, !(tex_host || jpeg || pre) || (tex_h > 0 && tex_w > 0), "mesh_upload: bad texture size");
    for (long i = 0; i < 3l * n_tris; ++i)
        MVLM_REQUIRE(ctx, tris_host[i] >= 0 && tris_host[i] < n_verts, "mesh_upload: triangle index out of range");
    const bool with_tex = (tex_host || jpeg || pre) && uvs_host;
    if (!with_tex) jpeg = nullptr;
    if (!with_tex) pre = nullptr;  // (no texture coordinates: the texture is not used - utils3d.py:26; the caller keeps it)
    const void* src[4] = {verts_host, uvs_host, tris_host, with_tex && !jpeg && !pre ? tex_host : nullptr};
    const size_t bytes[4] = {size_t(n_verts) * 12, uvs_host ? size_t(n_verts) * 8 : 0, size_t(n_tris) * 12,
                             with_tex ? size_t(tex_h) * tex_w * 3 : 0};
    // the rasteriser fetches a texel with one 4-byte load at byte 3 * index: 4 spare bytes behind the texture
    const size_t room[4] = {bytes[0], bytes[1], bytes[2], bytes[3] ? bytes[3] + 4 : 0};
    size_t off[5], total = 0;
    for (int i = 0; i < 4; ++i) {
        off[i] = total;
        total += ((src[i] ? bytes[i] : 0) + 255) / 256 * 256;
    }
    off[4] = total;  // the JPEG's header, tables and unstuffed stream
    if (jpeg) total += mvlm_jpeg_stage_bytes(*jpeg, jpeg_n);

    std::lock_guard<std::mutex> upload_lock(ctx->upload_mu);
    MVLM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // the pinned staging slot (two slots alternate; a slot is reused once the copies out of it are done)
    if (!ctx->upload_stream) MVLM_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    const int slot = ctx->upload_stage_next;
    ctx->upload_stage_next ^= 1;
    if (ctx->upload_stage_done[slot]) MVLM_CHECK_HIP(ctx, hipEventSynchronize(ctx->upload_stage_done[slot]));
    if (ctx->upload_stage_cap[slot] < total) {
        if (ctx->upload_stage[slot]) (void)hipHostFree(ctx->upload_stage[slot]);
        ctx->upload_stage[slot] = nullptr;
        ctx->upload_stage_cap[slot] = 0;
        const size_t cap = (total + (size_t(4) << 20)) / (size_t(4) << 20) * (size_t(4) << 20);
        MVLM_CHECK_HIP(ctx, hipHostMalloc(&ctx->upload_stage[slot], cap, hipHostMallocDefault));
        ctx->upload_stage_cap[slot] = cap;
    }
    auto* stage = static_cast<unsigned char*>(ctx->upload_stage[slot]);
    for (int i = 0; i < 4; ++i)
        if (src[i] && bytes[i]) std::memcpy(stage + off[i], src[i], bytes[i]);
    std::string jpeg_why;
    if (jpeg && mvlm_jpeg_fill_stage(*jpeg, jpeg_bytes, jpeg_n, stage + off[4], jpeg_why) != 0) {
        ctx->fail("jpeg: " + jpeg_why);
        return 2;
    }

    auto* m = new mvlm_mesh();
    static std::atomic<unsigned long long> next_uid{1};
    m->uid = next_uid.fetch_add(1);
    m->n_verts = n_verts;
    m->n_tris = n_tris;
    if (n_tris == 0) {  // the automatic radius, from the points as uploaded
        (void)mvlm_points_auto_radius(verts_host, n_verts, &m->point_radius);
        (void)rp_radius_steps(m->point_radius, &m->point_R);  // (inside the admitted range by construction)
        m->point_c = rp_depth_coeff(m->point_radius, m->point_R);
    }
    void** dst[4] = {(void**)&m->verts, (void**)&m->uvs, (void**)&m->tris, (void**)&m->tex};
    bool ok = true;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);  // pool, event list: shared with the launch entry points
        for (int i = 0; i < 4 && ok; ++i) {
            if (!bytes[i]) continue;
            if (i == 3 && pre) {  // decoded ahead: the texture's buffer becomes the mesh's
                *dst[i] = pre->dev;
                m->cap[i] = pre->cap;
                m->waited[i] = pre->waited;
                continue;
            }
            if (!take_upload_buffer(ctx, bytes[i], room[i], dst[i], &m->cap[i], &m->waited[i])) ok = false;
            if (ok && src[i] && hipMemcpyAsync(*dst[i], stage + off[i], bytes[i], hipMemcpyHostToDevice, ctx->upload_stream) != hipSuccess) ok = false;
        }
        if (with_tex) {
            m->tex_h = tex_h;
            m->tex_w = tex_w;
        }
    }
    int jpeg_rc = 0;
    if (ok && jpeg) {
        // decode kernels on the upload stream; the host waits for that stream twice (jpeg.hip), with only the upload mutex
        // held - the launch thread keeps going
        jpeg_rc = mvlm_jpeg_run(ctx, *jpeg, stage + off[4], m->tex, ctx->upload_stream, jpeg_why, nullptr);
        if (jpeg_rc == 2) ctx->fail("jpeg: " + jpeg_why);
        if (jpeg_rc != 0) ok = false;
    }
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (ok) {
            if (!ctx->upload_stage_done[slot]) ctx->upload_stage_done[slot] = ctx->take_event();
            m->ready = ctx->take_event();
            ok = ctx->upload_stage_done[slot] && m->ready &&
                 hipEventRecord(ctx->upload_stage_done[slot], ctx->upload_stream) == hipSuccess &&
                 hipEventRecord(m->ready, ctx->upload_stream) == hipSuccess;
        }
    }
    if (!ok) {
        (void)hipStreamSynchronize(ctx->upload_stream);
        if (pre) {  // still the caller's
            m->tex = nullptr;
            m->waited[3] = nullptr;
        }
        mvlm_mesh_free(nullptr, m);
        if (jpeg_rc != 0) return jpeg_rc;  // (the message is set)
        return ctx->fail("mesh_upload: device allocation / copy failed");
    }
    if (pre) delete pre;  // consumed: buffer and event are the mesh's now
    *out = m;
    return 0;
}

extern "C" int mvlm_mesh_upload(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts,
                                const int32_t* tris_host, int n_tris, const uint8_t* tex_host, int tex_h, int tex_w,
                                mvlm_mesh** out) {
    return mesh_upload_impl(ctx, verts_host, uvs_host, n_verts, tris_host, n_tris, tex_host, tex_h, tex_w, nullptr, nullptr, 0, out);
}

// ---- JPEG textures decoded on the device (jpeg.hip) ------------------------------------------------------------------
extern "C" int mvlm_jpeg_info(const uint8_t* jpeg, size_t n_bytes, int* width, int* height, int* components, char* why, int why_len) {
    MvlmJpegPlan* plan = mvlm_jpeg_plan_new();
    std::string w;
    const int rc = mvlm_jpeg_plan_impl(jpeg, n_bytes, *plan, w);
    if (rc == 0) mvlm_jpeg_plan_dims(*plan, width, height, components);
    if (why && why_len > 0) {
        std::snprintf(why, size_t(why_len), "%s", w.c_str());
    }
    mvlm_jpeg_plan_delete(plan);
    return rc;
}

extern "C" int mvlm_mesh_upload_jpeg(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts,
                                     const int32_t* tris_host, int n_tris, const uint8_t* jpeg, size_t jpeg_bytes, mvlm_mesh** out) {
    MVLM_REQUIRE(ctx, out, "mesh_upload_jpeg: null output");
    *out = nullptr;
    MVLM_REQUIRE(ctx, n_tris != 0, "mesh_upload_jpeg: a point cloud (n_tris == 0) takes no texture");
    MVLM_REQUIRE(ctx, jpeg && jpeg_bytes > 0, "mesh_upload_jpeg: no JPEG");
    std::unique_ptr<MvlmJpegPlan, void (*)(MvlmJpegPlan*)> plan(mvlm_jpeg_plan_new(), mvlm_jpeg_plan_delete);
    std::string w;
    if (mvlm_jpeg_plan_impl(jpeg, jpeg_bytes, *plan, w) != 0) {
        ctx->fail("jpeg: " + w);
        return 2;
    }
    int tw = 0, th = 0, nc = 0;
    mvlm_jpeg_plan_dims(*plan, &tw, &th, &nc);
    return mesh_upload_impl(ctx, verts_host, uvs_host, n_verts, tris_host, n_tris, nullptr, th, tw, plan.get(), jpeg, jpeg_bytes, out);
}

// the decoder alone (tests, tools): rgb_dev [H, W, 3] is complete on return; rounds_out: synchronisation rounds it took
extern "C" int mvlm_jpeg_decode(mvlm_ctx* ctx, const uint8_t* jpeg, size_t jpeg_bytes, uint8_t* rgb_dev, int* rounds_out) {
    MVLM_REQUIRE(ctx, jpeg && jpeg_bytes > 0 && rgb_dev, "jpeg_decode: null pointer");
    std::unique_ptr<MvlmJpegPlan, void (*)(MvlmJpegPlan*)> plan(mvlm_jpeg_plan_new(), mvlm_jpeg_plan_delete);
    std::string w;
    if (mvlm_jpeg_plan_impl(jpeg, jpeg_bytes, *plan, w) != 0) {
        ctx->fail("jpeg: " + w);
        return 2;
    }
    std::lock_guard<std::mutex> upload_lock(ctx->upload_mu);
    MVLM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload_stream) MVLM_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    const size_t total = mvlm_jpeg_stage_bytes(*plan, jpeg_bytes);
    const int slot = ctx->upload_stage_next;
    ctx->upload_stage_next ^= 1;
    if (ctx->upload_stage_done[slot]) MVLM_CHECK_HIP(ctx, hipEventSynchronize(ctx->upload_stage_done[slot]));
    if (ctx->upload_stage_cap[slot] < total) {
        if (ctx->upload_stage[slot]) (void)hipHostFree(ctx->upload_stage[slot]);
        ctx->upload_stage[slot] = nullptr;
        ctx->upload_stage_cap[slot] = 0;
        const size_t cap = (total + (size_t(4) << 20)) / (size_t(4) << 20) * (size_t(4) << 20);
        MVLM_CHECK_HIP(ctx, hipHostMalloc(&ctx->upload_stage[slot], cap, hipHostMallocDefault));
        ctx->upload_stage_cap[slot] = cap;
    }
    auto* stage = static_cast<unsigned char*>(ctx->upload_stage[slot]);
    if (mvlm_jpeg_fill_stage(*plan, jpeg, jpeg_bytes, stage, w) != 0) {
        ctx->fail("jpeg: " + w);
        return 2;
    }
    // whatever the launch stream still does with rgb_dev comes first
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        hipEvent_t e = ctx->take_event();
        MVLM_REQUIRE(ctx, e, "jpeg_decode: no event");
        const bool ok = hipEventRecord(e, ctx->stream) == hipSuccess && hipStreamWaitEvent(ctx->upload_stream, e, 0) == hipSuccess;
        ctx->event_free.push_back(e);
        MVLM_REQUIRE(ctx, ok, "jpeg_decode: stream order");
    }
    const int rc = mvlm_jpeg_run(ctx, *plan, stage, rgb_dev, ctx->upload_stream, w, rounds_out);
    if (rc == 2) ctx->fail("jpeg: " + w);
    return rc;  // (mvlm_jpeg_run has waited for the stream: the staging slot is free, the image complete)
}

// The texture of a scan decoded AHEAD of its mesh, so that a caller can decode (GPU + this thread waiting for it) while
// another thread still parses the geometry: the JPEG goes through the decoder into a buffer of the mesh pool; the handle is
// consumed by mvlm_mesh_upload_texture or given back with mvlm_texture_free.  0 / 1 / 2 like mvlm_mesh_upload_jpeg.
extern "C" int mvlm_texture_from_jpeg(mvlm_ctx* ctx, const uint8_t* jpeg, size_t jpeg_bytes, mvlm_texture** out) {
    MVLM_REQUIRE(ctx, out, "texture_from_jpeg: null output");
    *out = nullptr;
    MVLM_REQUIRE(ctx, jpeg && jpeg_bytes > 0, "texture_from_jpeg: no JPEG");
    std::unique_ptr<MvlmJpegPlan, void (*)(MvlmJpegPlan*)> plan(mvlm_jpeg_plan_new(), mvlm_jpeg_plan_delete);
    std::string w;
    if (mvlm_jpeg_plan_impl(jpeg, jpeg_bytes, *plan, w) != 0) {
        ctx->fail("jpeg: " + w);
        return 2;
    }
    int tw = 0, th = 0, nc = 0;
    mvlm_jpeg_plan_dims(*plan, &tw, &th, &nc);
    std::lock_guard<std::mutex> upload_lock(ctx->upload_mu);
    MVLM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload_stream) MVLM_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    const size_t total = mvlm_jpeg_stage_bytes(*plan, jpeg_bytes);
    const int slot = ctx->upload_stage_next;
    ctx->upload_stage_next ^= 1;
    if (ctx->upload_stage_done[slot]) MVLM_CHECK_HIP(ctx, hipEventSynchronize(ctx->upload_stage_done[slot]));
    if (ctx->upload_stage_cap[slot] < total) {
        if (ctx->upload_stage[slot]) (void)hipHostFree(ctx->upload_stage[slot]);
        ctx->upload_stage[slot] = nullptr;
        ctx->upload_stage_cap[slot] = 0;
        const size_t cap = (total + (size_t(4) << 20)) / (size_t(4) << 20) * (size_t(4) << 20);
        MVLM_CHECK_HIP(ctx, hipHostMalloc(&ctx->upload_stage[slot], cap, hipHostMallocDefault));
        ctx->upload_stage_cap[slot] = cap;
    }
    auto* stage = static_cast<unsigned char*>(ctx->upload_stage[slot]);
    if (mvlm_jpeg_fill_stage(*plan, jpeg, jpeg_bytes, stage, w) != 0) {
        ctx->fail("jpeg: " + w);
        return 2;
    }
    std::unique_ptr<mvlm_texture> t(new mvlm_texture());
    t->h = th;
    t->w = tw;
    const size_t bytes = size_t(th) * tw * 3;
    bool ok;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        void* p = nullptr;
        ok = take_upload_buffer(ctx, bytes, bytes + 4, &p, &t->cap, &t->waited);  // (4 spare bytes: the rasteriser's texel load)
        t->dev = static_cast<uint8_t*>(p);
    }
    int rc = ok ? mvlm_jpeg_run(ctx, *plan, stage, t->dev, ctx->upload_stream, w, nullptr) : 1;
    if (rc != 0) {
        if (rc == 2) ctx->fail("jpeg: " + w);
        if (!ok) ctx->fail("texture_from_jpeg: device allocation failed");
        mvlm_texture_free(ctx, t.release());
        return rc;
    }
    *out = t.release();  // (mvlm_jpeg_run has waited for the stream: the pixels are there)
    return 0;
}

extern "C" void mvlm_texture_free(mvlm_ctx* ctx, mvlm_texture* t) {
    if (!t) return;
    if (ctx && t->dev) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        if (t->waited) ctx->event_free.push_back(t->waited);
        t->waited = nullptr;
        if (ctx->mesh_pool.size() < 32 && ctx->mesh_pool_bytes + t->cap <= (size_t(1) << 30)) {
            // only the upload stream has touched the buffer, and the decode waited for it: no event needed
            ctx->mesh_pool.push_back({t->dev, t->cap, nullptr});
            ctx->mesh_pool_bytes += t->cap;
            t->dev = nullptr;
        }
    }
    if (t->dev || t->waited) {
        if (t->waited) (void)hipEventDestroy(t->waited);
        if (t->dev) (void)hipFree(t->dev);
    }
    delete t;
}

extern "C" int mvlm_texture_size(const mvlm_texture* t, int* height, int* width) {
    if (!t) return 1;
    if (height) *height = t->h;
    if (width) *width = t->w;
    return 0;
}

// mvlm_mesh_upload with a texture that is on the device already; on success the handle is consumed (do not free it), on
// failure it is still the caller's.  Without texture coordinates the texture is not used and stays the caller's too.
extern "C" int mvlm_mesh_upload_texture(mvlm_ctx* ctx, const float* verts_host, const float* uvs_host, int n_verts,
                                        const int32_t* tris_host, int n_tris, mvlm_texture* tex, int* consumed, mvlm_mesh** out) {
    if (consumed) *consumed = 0;
    MVLM_REQUIRE(ctx, tex && tex->dev, "mesh_upload_texture: no texture");
    MVLM_REQUIRE(ctx, n_tris != 0, "mesh_upload_texture: a point cloud (n_tris == 0) takes no texture");
    const bool will_consume = uvs_host != nullptr;
    const int rc = mesh_upload_impl(ctx, verts_host, uvs_host, n_verts, tris_host, n_tris, nullptr, tex->h, tex->w, nullptr, nullptr, 0, out, tex);
    if (rc == 0 && will_consume && consumed) *consumed = 1;
    return rc;
}

// Per-vertex colours for a mesh that any of the upload entries above made: rgb_host u8[V,3] -> u8[V,4] (r g b 255) on the
// device, through the pinned staging and the upload stream like the mesh itself; the mesh's ready event is recorded again
// behind the copy, so whatever renders the mesh afterwards waits for the colours too.  May run on a reader thread.  The buffer
// comes from the mesh pool and is written in full - a recycled one keeps nothing of its previous owner - and a mesh that
// never had this call has no colours, whatever its buffers held before.  A second call replaces the colours.
extern "C" int mvlm_mesh_upload_colors(mvlm_ctx* ctx, mvlm_mesh* m, const uint8_t* rgb_host, int n_verts) {
    MVLM_REQUIRE(ctx, m && rgb_host, "mesh_upload_colors: null pointer");
    MVLM_REQUIRE(ctx, n_verts == m->n_verts, "mesh_upload_colors: " + std::to_string(n_verts) + " colours for a mesh of " +
                                                  std::to_string(m->n_verts) + " points");
    const size_t bytes = size_t(n_verts) * 4;
    std::lock_guard<std::mutex> upload_lock(ctx->upload_mu);
    MVLM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload_stream) MVLM_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    const int slot = ctx->upload_stage_next;
    ctx->upload_stage_next ^= 1;
    if (ctx->upload_stage_done[slot]) MVLM_CHECK_HIP(ctx, hipEventSynchronize(ctx->upload_stage_done[slot]));
    if (ctx->upload_stage_cap[slot] < bytes) {
        if (ctx->upload_stage[slot]) (void)hipHostFree(ctx->upload_stage[slot]);
        ctx->upload_stage[slot] = nullptr;
        ctx->upload_stage_cap[slot] = 0;
        const size_t cap = (bytes + (size_t(4) << 20)) / (size_t(4) << 20) * (size_t(4) << 20);
        MVLM_CHECK_HIP(ctx, hipHostMalloc(&ctx->upload_stage[slot], cap, hipHostMallocDefault));
        ctx->upload_stage_cap[slot] = cap;
    }
    auto* stage = static_cast<unsigned char*>(ctx->upload_stage[slot]);
    for (size_t i = 0; i < size_t(n_verts); ++i) {
        stage[4 * i] = rgb_host[3 * i];
        stage[4 * i + 1] = rgb_host[3 * i + 1];
        stage[4 * i + 2] = rgb_host[3 * i + 2];
        stage[4 * i + 3] = 255;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);  // pool, events, the mesh's fields: shared with the launch entry points
    bool ok = true;
    void* dst = m->colors;
    if (dst) {  // replacing: a render that was enqueued with the old colours reads them first
        hipEvent_t e = ctx->take_event();
        ok = e && hipEventRecord(e, ctx->stream) == hipSuccess && hipStreamWaitEvent(ctx->upload_stream, e, 0) == hipSuccess;
        if (e) ctx->event_free.push_back(e);
    } else {
        size_t cap = 0;
        hipEvent_t waited = nullptr;
        ok = take_upload_buffer(ctx, bytes, bytes, &dst, &cap, &waited);
        if (ok) {
            m->cap[4] = cap;
            m->waited[4] = waited;
        } else if (dst) {  // (the pool's buffer could not be waited for: back to the allocator)
            (void)hipFree(dst);
            if (waited) ctx->event_free.push_back(waited);
            dst = nullptr;
        }
    }
    ok = ok && hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, ctx->upload_stream) == hipSuccess;
    if (ok) {
        if (!ctx->upload_stage_done[slot]) ctx->upload_stage_done[slot] = ctx->take_event();
        if (!m->ready) m->ready = ctx->take_event();
        ok = ctx->upload_stage_done[slot] && m->ready &&
             hipEventRecord(ctx->upload_stage_done[slot], ctx->upload_stream) == hipSuccess &&
             hipEventRecord(m->ready, ctx->upload_stream) == hipSuccess;
    }
    if (!ok) (void)hipStreamSynchronize(ctx->upload_stream);  // (whatever was enqueued has left the staging slot)
    if (dst && !m->colors && !ok) {  // the new buffer stays out of the mesh
        (void)hipFree(dst);
        if (m->waited[4]) ctx->event_free.push_back(m->waited[4]);
        m->cap[4] = 0;
        m->waited[4] = nullptr;
        dst = nullptr;
    }
    if (ok) m->colors = static_cast<uint8_t*>(dst);
    MVLM_REQUIRE(ctx, ok, "mesh_upload_colors: device allocation / copy failed");
    return 0;
}

// The buffer a cloud's normals go to (declared in common.h; the caller holds ctx->mu): the mesh's own when it has normals, else
// one from the mesh pool, which stays the mesh's (normals_buf) and goes back with the others in mvlm_mesh_free.  The caller sets
// m->normals once the normals are on their way.
float* mvlm_mesh_normals_buffer(mvlm_ctx* ctx, mvlm_mesh* m) {
    if (m->normals_buf) return m->normals_buf;
    if (!ctx->upload_stream && hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
    const size_t bytes = size_t(m->n_verts) * 3 * sizeof(float);
    void* dst = nullptr;
    size_t cap = 0;
    hipEvent_t waited = nullptr;
    if (!take_upload_buffer(ctx, bytes, bytes, &dst, &cap, &waited)) {
        if (dst) (void)hipFree(dst);  // (the pool's buffer could not be waited for: back to the allocator)
        if (waited) ctx->event_free.push_back(waited);
        return nullptr;
    }
    // a pooled buffer's previous owner was made to precede the upload stream; the launch stream writes an estimate's normals
    if (waited && hipStreamWaitEvent(ctx->stream, waited, 0) != hipSuccess) {
        (void)hipFree(dst);
        ctx->event_free.push_back(waited);
        return nullptr;
    }
    m->cap[5] = cap;
    m->waited[5] = waited;
    m->normals_buf = static_cast<float*>(dst);
    return m->normals_buf;
}

// Per-point normals for a point mesh: normals_host f32[V,3] as a file gives them (any length; the shade divides by it) -> the
// device, through the pinned staging and the upload stream like the colours; the mesh's ready event is recorded again behind the
// copy.  May run on a reader thread.  A second call, or one after mvlm_mesh_estimate_normals, replaces the normals.
extern "C" int mvlm_mesh_upload_normals(mvlm_ctx* ctx, mvlm_mesh* m, const float* normals_host, int n_verts) {
    MVLM_REQUIRE(ctx, m && normals_host, "mesh_upload_normals: null pointer");
    MVLM_REQUIRE(ctx, m->n_tris == 0, "mesh_upload_normals: the mesh has triangles (normals belong to a point cloud)");
    MVLM_REQUIRE(ctx, n_verts == m->n_verts, "mesh_upload_normals: " + std::to_string(n_verts) + " normals for a mesh of " +
                                                  std::to_string(m->n_verts) + " points");
    const size_t bytes = size_t(n_verts) * 3 * sizeof(float);
    std::lock_guard<std::mutex> upload_lock(ctx->upload_mu);
    MVLM_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload_stream) MVLM_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    const int slot = ctx->upload_stage_next;
    ctx->upload_stage_next ^= 1;
    if (ctx->upload_stage_done[slot]) MVLM_CHECK_HIP(ctx, hipEventSynchronize(ctx->upload_stage_done[slot]));
    if (ctx->upload_stage_cap[slot] < bytes) {
        if (ctx->upload_stage[slot]) (void)hipHostFree(ctx->upload_stage[slot]);
        ctx->upload_stage[slot] = nullptr;
        ctx->upload_stage_cap[slot] = 0;
        const size_t cap = (bytes + (size_t(4) << 20)) / (size_t(4) << 20) * (size_t(4) << 20);
        MVLM_CHECK_HIP(ctx, hipHostMalloc(&ctx->upload_stage[slot], cap, hipHostMallocDefault));
        ctx->upload_stage_cap[slot] = cap;
    }
    std::memcpy(ctx->upload_stage[slot], normals_host, bytes);
    std::lock_guard<std::mutex> lock(ctx->mu);  // pool, events, the mesh's fields: shared with the launch entry points
    const bool replacing = m->normals_buf != nullptr;
    float* const dst = mvlm_mesh_normals_buffer(ctx, m);
    bool ok = dst != nullptr;
    if (ok && replacing) {  // a render that was enqueued with the old normals reads them first
        hipEvent_t e = ctx->take_event();
        ok = e && hipEventRecord(e, ctx->stream) == hipSuccess && hipStreamWaitEvent(ctx->upload_stream, e, 0) == hipSuccess;
        if (e) ctx->event_free.push_back(e);
    }
    ok = ok && hipMemcpyAsync(dst, ctx->upload_stage[slot], bytes, hipMemcpyHostToDevice, ctx->upload_stream) == hipSuccess;
    if (ok) {
        if (!ctx->upload_stage_done[slot]) ctx->upload_stage_done[slot] = ctx->take_event();
        if (!m->ready) m->ready = ctx->take_event();
        ok = ctx->upload_stage_done[slot] && m->ready &&
             hipEventRecord(ctx->upload_stage_done[slot], ctx->upload_stream) == hipSuccess &&
             hipEventRecord(m->ready, ctx->upload_stream) == hipSuccess;
    }
    if (!ok) (void)hipStreamSynchronize(ctx->upload_stream);  // (whatever was enqueued has left the staging slot)
    if (ok) m->normals = dst;
    MVLM_REQUIRE(ctx, ok, "mesh_upload_normals: device allocation / copy failed");
    return 0;
}

// The splat radius of a point mesh, in model units (raster_points_math.h): admitted from 0.75 to 8 pixels of the 256-pixel window
// that shows 300 units.  Renders enqueued before the call keep the radius they were launched with.
extern "C" int mvlm_mesh_set_point_radius(mvlm_ctx* ctx, mvlm_mesh* m, double r_model_units) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MVLM_REQUIRE(ctx, m, "mesh_set_point_radius: null mesh");
    MVLM_REQUIRE(ctx, m->n_tris == 0, "mesh_set_point_radius: the mesh has triangles (a radius belongs to a point cloud)");
    int32_t R = 0;
    MVLM_REQUIRE(ctx, rp_radius_steps(r_model_units, &R),
                 "mesh_set_point_radius: the radius must be 0.75 to 8 pixels, i.e. 0.87890625 to 9.375 model units (" +
                     std::to_string(r_model_units) + " given)");
    m->point_radius = r_model_units;
    m->point_R = R;
    m->point_c = rp_depth_coeff(r_model_units, R);
    return 0;
}

extern "C" int mvlm_mesh_point_radius(const mvlm_mesh* m, double* r_model_units) {
    if (!m || !r_model_units || m->n_tris != 0) return 1;
    *r_model_units = m->point_radius;
    return 0;
}

// Measuring hook (tools/points_bench.py): with counting on, a cloud's render runs the splat kernel's counting form;
// mvlm_points_get_stats waits for the stream and returns what the LAST such render counted - pixels that passed coverage and
// clip, and the atomics issued for them (the rest found a smaller key in place and skipped theirs).
extern "C" int mvlm_points_set_counting(mvlm_ctx* ctx, int enabled) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->points_counting = enabled != 0;
    return 0;
}

extern "C" int mvlm_points_get_stats(mvlm_ctx* ctx, unsigned long long* covered, unsigned long long* issued) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, covered && issued, "points_get_stats: null pointer");
    const auto it = ctx->scratch.find("points.stats");
    MVLM_REQUIRE(ctx, it != ctx->scratch.end() && it->second.first, "points_get_stats: no cloud has been rendered with counting on");
    unsigned long long host[2] = {0, 0};
    MVLM_CHECK_HIP(ctx, hipMemcpyAsync(host, it->second.first, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    MVLM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *covered = host[0];
    *issued = host[1];
    return 0;
}

// Milliseconds of the last cloud render's two kernels - splat, tile - while mvlm_render_set_profiling is on; waits for the stream.
extern "C" int mvlm_points_stage_ms(mvlm_ctx* ctx, float* ms2) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms2, "points_stage_ms: null pointer");
    return ctx->points_clock.read(ctx, 2, ms2, "points_stage_ms: no point cloud was rendered with render profiling on");
}

// Buffers go back to the context's pool together with an event on the launch stream: whatever was enqueued for this
// mesh before the free may still read them.  ctx == NULL (or a pool that is full): plain hipFree (which waits for the device).
extern "C" void mvlm_mesh_free(mvlm_ctx* ctx, mvlm_mesh* m) {
    if (!m) return;
    void* bufs[6] = {m->verts, m->uvs, m->tris, m->tex, m->colors, m->normals_buf};
    constexpr size_t POOL_MAX_BYTES = size_t(1) << 30;
    constexpr size_t POOL_MAX_ENTRIES = 32;
    hipEvent_t spare[7] = {m->ready, m->waited[0], m->waited[1], m->waited[2], m->waited[3], m->waited[4], m->waited[5]};
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        (void)hipSetDevice(ctx->device);
        for (int i = 0; i < 6; ++i)
            if (bufs[i] && m->cap[i] && ctx->mesh_pool.size() < POOL_MAX_ENTRIES &&
                ctx->mesh_pool_bytes + m->cap[i] <= POOL_MAX_BYTES) {
                hipEvent_t ev = ctx->take_event();
                if (!ev || hipEventRecord(ev, ctx->stream) != hipSuccess) {  // no event: keep the plain (synchronising) free
                    if (ev) ctx->event_free.push_back(ev);
                    continue;
                }
                ctx->mesh_pool.push_back({bufs[i], m->cap[i], ev});
                ctx->mesh_pool_bytes += m->cap[i];
                bufs[i] = nullptr;
            }
        for (hipEvent_t e : spare)
            if (e) ctx->event_free.push_back(e);
    } else {
        for (hipEvent_t e : spare)
            if (e) (void)hipEventDestroy(e);
    }
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete m;
}

// ---- landmark view (raster_view.hip; DESIGN.md 5.1, "Landmark view") and ray view (raster_rays.hip; "Ray view") -----------
// The checks of the arguments the two entry points share, under the entry's own name; fills the frames with k.
static int view_check_arguments(mvlm_ctx* ctx, const std::string& what, const mvlm_mesh* mesh, const double* rot_host, int n_views,
                                int size, const float* frame_host, const double* landmarks_host, int n_lm, float radius,
                                const uint8_t* out_dev, std::vector<float>& frames) {
    MVLM_REQUIRE(ctx, mesh && rot_host && frame_host && out_dev && n_views > 0, what + ": bad arguments");
    MVLM_REQUIRE(ctx, mesh->n_verts > 0, what + ": empty mesh");
    MVLM_REQUIRE(ctx, mesh->n_tris > 0, what + ": a point cloud is not supported here (the mesh has no triangles)");
    MVLM_REQUIRE(ctx, size >= RV_MIN_SIZE && size <= RV_MAX_SIZE && size % RM_TILE == 0,
                 what + ": size must be a multiple of 16 in 64..2048 (" + std::to_string(size) + " given)");
    MVLM_REQUIRE(ctx, n_views <= RV_MAX_VIEWS, what + ": at most 128 views per call (" + std::to_string(n_views) + " given)");
    MVLM_REQUIRE(ctx, (long long)n_views * size * size <= RV_MAX_PIXELS,
                 what + ": n_views * size * size exceeds 8 * 2048 * 2048 pixels per call");
    MVLM_REQUIRE(ctx, n_lm >= 0 && (n_lm == 0 || landmarks_host), what + ": landmarks missing");
    MVLM_REQUIRE(ctx, std::isfinite(radius) && radius >= 0.0f, what + ": the radius must be finite and >= 0");
    for (int k = 0; k < n_views * 9; ++k) MVLM_REQUIRE(ctx, std::isfinite(rot_host[k]), what + ": non-finite rotation");
    frames.assign(size_t(n_views) * 4, 0.0f);
    for (int v = 0; v < n_views; ++v) {
        const float cx = frame_host[3 * v], cy = frame_host[3 * v + 1], half = frame_host[3 * v + 2];
        MVLM_REQUIRE(ctx, std::isfinite(cx) && std::isfinite(cy) && std::isfinite(half) && half > 0.0f,
                     what + ": a frame needs finite cx, cy and half > 0");
        const float k = rv_scale(size, half);
        MVLM_REQUIRE(ctx, std::isfinite(k) && k > 0.0f, what + ": half is too small or too large for this size");
        frames[4 * v] = cx;
        frames[4 * v + 1] = cy;
        frames[4 * v + 2] = half;
        frames[4 * v + 3] = k;
    }
    for (int k = 0; k < n_lm * 3; ++k) MVLM_REQUIRE(ctx, std::isfinite(landmarks_host[k]), what + ": non-finite landmark");
    return 0;
}

// Checks the arguments - a bad one returns an error and launches nothing - and hands the launch set to raster_view.hip.
extern "C" int mvlm_render_landmark_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                                         const float* frame_host, const double* landmarks_host, int n_lm, float radius,
                                         const uint8_t* lm_rgb_host, uint8_t* out_dev, int32_t* lm_pixels_dev) {
    MVLM_ENTER(ctx);
    std::vector<float> frames;
    if (view_check_arguments(ctx, "landmark view", mesh, rot_host, n_views, size, frame_host, landmarks_host, n_lm, radius, out_dev,
                             frames))
        return 1;
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;  // the upload runs on a stream of its own
    return mvlm_launch_landmark_view(ctx, mesh, rot_host, n_views, size, frames.data(), landmarks_host, n_lm, radius, lm_rgb_host,
                                     out_dev, lm_pixels_dev);
}

// The landmark view with the caller's colour per vertex (the surface heat's, mvlm_surface_heat): the same checks and the same launch
// set, the tile kernel given those colours, no texture and shading 0.
extern "C" int mvlm_render_landmark_view_colored(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                                                 const float* frame_host, const double* landmarks_host, int n_lm, float radius,
                                                 const uint8_t* lm_rgb_host, uint8_t* out_dev, int32_t* lm_pixels_dev,
                                                 const uint8_t* vert_rgba_dev) {
    MVLM_ENTER(ctx);
    std::vector<float> frames;
    if (view_check_arguments(ctx, "landmark view", mesh, rot_host, n_views, size, frame_host, landmarks_host, n_lm, radius, out_dev,
                             frames))
        return 1;
    MVLM_REQUIRE(ctx, vert_rgba_dev && reinterpret_cast<uintptr_t>(vert_rgba_dev) % 4 == 0,
                 "landmark view: the vertex colours must be a 4-byte aligned device pointer");
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;
    return mvlm_launch_landmark_view(ctx, mesh, rot_host, n_views, size, frames.data(), landmarks_host, n_lm, radius, lm_rgb_host,
                                     out_dev, lm_pixels_dev, vert_rgba_dev);
}

// Bytes of the context's grow-only scratch whose names start with `prefix` ("backproject": the surface heat's; "": all of it).
extern "C" int mvlm_scratch_bytes(mvlm_ctx* ctx, const char* prefix, size_t* bytes) {
    if (!ctx) return 1;
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, prefix && bytes, "scratch_bytes: null pointer");
    size_t total = 0;
    for (const auto& kv : ctx->scratch)
        if (kv.first.rfind(prefix, 0) == 0 && kv.second.first) total += kv.second.second;
    *bytes = total;
    return 0;
}

// The same with the rays: the shared arguments are checked the same, the rays' own under "ray view:"; hands over to raster_rays.hip.
extern "C" int mvlm_render_ray_view(mvlm_ctx* ctx, const mvlm_mesh* mesh, const double* rot_host, int n_views, int size,
                                    const float* frame_host, const double* landmarks_host, int n_lm, float radius,
                                    const uint8_t* lm_rgb_host, const double* starts_dev, const double* ends_dev, int n_rays,
                                    float ray_radius, const uint8_t* ray_rgb_host, uint8_t* out_dev, int32_t* lm_pixels_dev,
                                    int32_t* ray_pixels_dev) {
    MVLM_ENTER(ctx);
    std::vector<float> frames;
    if (view_check_arguments(ctx, "ray view", mesh, rot_host, n_views, size, frame_host, landmarks_host, n_lm, radius, out_dev, frames))
        return 1;
    MVLM_REQUIRE(ctx, n_rays >= 0 && n_rays <= RV_MAX_RAYS,
                 "ray view: 0..65536 rays per call (" + std::to_string(n_rays) + " given)");
    MVLM_REQUIRE(ctx, (long long)n_views * n_rays <= RV_MAX_RAY_RECORDS,
                 "ray view: n_views * n_rays exceeds 1048576 records per call (" + std::to_string((long long)n_views * n_rays) + " asked)");
    MVLM_REQUIRE(ctx, n_rays == 0 || (starts_dev && ends_dev), "ray view: ray starts or ends missing");
    MVLM_REQUIRE(ctx, std::isfinite(ray_radius) && ray_radius >= 0.0f, "ray view: the ray radius must be finite and >= 0");
    if (mvlm_mesh_wait_ready(ctx, mesh, ctx->stream)) return 1;
    return mvlm_launch_ray_view(ctx, mesh, rot_host, n_views, size, frames.data(), landmarks_host, n_lm, radius, lm_rgb_host, starts_dev,
                                ends_dev, n_rays, ray_radius, ray_rgb_host, out_dev, lm_pixels_dev, ray_pixels_dev);
}

// Milliseconds of the last landmark view's stages (copies and fills - the key plane's among them -, transform, classify, scan,
// bin fill, landmark projection, tile) while
// mvlm_render_set_profiling is on; waits for the stream.
extern "C" int mvlm_landmark_view_stage_ms(mvlm_ctx* ctx, float* ms7) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms7, "landmark_view_stage_ms: null pointer");
    return ctx->view_clock.read(ctx, 7, ms7, "landmark_view_stage_ms: no landmark view was drawn with render profiling on");
}

// Likewise the last ray view's eight stages: the landmark view's first six, the ray projection, the tile kernel.
extern "C" int mvlm_ray_view_stage_ms(mvlm_ctx* ctx, float* ms8) {
    MVLM_ENTER(ctx);
    MVLM_REQUIRE(ctx, ms8, "ray_view_stage_ms: null pointer");
    return ctx->view_clock.read(ctx, 8, ms8, "ray_view_stage_ms: no ray view was drawn with render profiling on");
}
