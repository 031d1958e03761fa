// Context of the libtopaz_hip.so runtime: kernel registries, workspace pools, patch lanes, the batched-launch recorder, the
// HIP-event profiler, the ctx-level C entry points and the debug switches.
#include "rt_internal.h"

// ------------------------------------------------------------------------------------------------
// kernel registry
// ------------------------------------------------------------------------------------------------
namespace tpz {
namespace {
std::vector<ConvKernelInfo>& registry() {
    static std::vector<ConvKernelInfo> r;
    return r;
}
std::vector<SplitKernelInfo>& split_registry() {
    static std::vector<SplitKernelInfo> r;
    return r;
}
}  // namespace
void register_conv(const ConvKernelInfo& info) { registry().push_back(info); }
const ConvKernelInfo* find_conv(int dims, int K, int D, int MT, bool cin1, int epi) {
    for (const auto& k : registry())
        if (k.dims == dims && k.K == K && k.D == D && k.MT == MT && k.cin1 == (cin1 ? 1 : 0) && k.epi == epi) return &k;
    return nullptr;
}
void register_split(const SplitKernelInfo& info) { split_registry().push_back(info); }
const SplitKernelInfo* find_split(int K, int D, int MT, int epi, int KX, int sps) {
    if (KX <= 0) KX = K;
    // several instantiations of one shape may differ in the steps per stage: the most steps (fewest barriers) unless the
    // caller needs a particular form (sps > 0: the folded 1x1 projection exists for one-step stages only)
    const SplitKernelInfo* best = nullptr;
    for (const auto& k : split_registry())
        if (k.K == K && k.KX == KX && k.D == D && k.MT == MT && k.epi == epi && (sps <= 0 || k.SPS == sps) &&
            (!best || k.SPS > best->SPS)) best = &k;
    return best;
}
}  // namespace tpz

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
namespace tpz::rt {
namespace {
std::string g_last_error;
}  // namespace
const std::string& last_global_error() { return g_last_error; }
void restore_errors(tpz_ctx* ctx, const std::string& ctx_err, const std::string& global_err) {
    if (ctx) ctx->err = ctx_err;
    g_last_error = global_err;
}

// The ONE place the environment is read (see rt_internal.h): nothing is honoured without TPZ_DEBUG=1.
DebugEnv debug_env() {
    DebugEnv d;
    const char* on = getenv("TPZ_DEBUG");
    if (!on || !*on || !strcmp(on, "0")) return d;
    d.on = true;
    auto flag = [](const char* name) { const char* e = getenv(name); return e != nullptr && *e && strcmp(e, "0") != 0; };
    d.no_phase = flag("TPZ_NO_PHASE");
    d.exact_fp32 = flag("TPZ_EXACT_FP32");
    d.no_issuer = flag("TPZ_NO_ISSUER");
    d.no_lanes = flag("TPZ_NO_LANES");
    d.no_roi = flag("TPZ_NO_ROI");
    d.no_persist = flag("TPZ_NO_PERSIST");
    d.trace_host = flag("TPZ_TRACE_HOST");
    d.no_range = flag("TPZ_NO_RANGE");
    d.no_raster = flag("TPZ_NO_RASTER");
    d.no_srcmajor = flag("TPZ_NO_SRCMAJOR");
    d.no_valu_last = flag("TPZ_NO_VALU_LAST");
    d.no_rw = flag("TPZ_NO_RW");
    d.no_pool3d = flag("TPZ_NO_POOL3D");
    d.no_fold = flag("TPZ_NO_FOLD");
    d.no_widen = flag("TPZ_NO_WIDEN");
    d.poison = flag("TPZ_POISON");
    if (flag("TPZ_NO_BATCH")) d.batch = 0;
    else if (const char* e = getenv("TPZ_BATCH")) {
        const int n = atoi(e);
        d.batch = n < 0 ? 0 : n > (int)tpz::SPLIT_MULTI_MAX ? (int)tpz::SPLIT_MULTI_MAX : n;
    }
    if (const char* e = getenv("TPZ_LANES")) d.lanes = atoi(e);
    return d;
}

int fail(tpz_ctx* ctx, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (ctx) ctx->err = buf;
    return 1;
}

// a buffer of at least `bytes` from `pool`, marked used: the smallest cached one that fits, else a new one; *size: its whole size
static void* pool_alloc(tpz_ctx* ctx, std::vector<tpz_ctx::Buf>& pool, size_t bytes, size_t* size) {
    if (bytes == 0) bytes = 16;
    int best = -1;
    for (int i = 0; i < (int)pool.size(); ++i) {
        auto& b = pool[i];
        if (!b.used && b.bytes >= bytes && (best < 0 || b.bytes < pool[best].bytes)) best = i;
    }
    if (best >= 0) {
        pool[best].used = true;
        *size = pool[best].bytes;
        return pool[best].p;
    }
    void* p = nullptr;
    // round up so slightly larger requests can reuse the buffer
    size_t rounded = (bytes + (1u << 20) - 1) & ~((size_t)(1u << 20) - 1);
    if (hipMalloc(&p, rounded) != hipSuccess) {
        // drop unused cached buffers and retry: first this pool's, then those of EVERY pool of the ctx (the pools of a batched
        // pass -- up to lanes x 8 of them --, the lane pools, the ctx pool: a pass with other tile shapes, or a large frame on
        // the ctx stream after a batched pass filled the device, finds its memory cached elsewhere).
        // NOT the pools of a batch that is being RECORDED (rec_on): a buffer marked unused there may still be named by
        // launches that were recorded and not yet issued -- hipDeviceSynchronize() does not cover a launch that was never
        // made, and rec_flush would replay kernels on freed memory.  Those pools are left alone; the pass then fails cleanly.
        auto trim = [](std::vector<tpz_ctx::Buf>& pl) {
            for (auto it = pl.begin(); it != pl.end();) {
                if (!it->used) { (void)hipFree(it->p); it = pl.erase(it); }
                else ++it;
            }
        };
        auto recording = [&](const std::vector<tpz_ctx::Buf>* pl) {
            if (!ctx->rec_on) return false;
            for (const auto& rp : ctx->rec_pools[ctx->rec_lane])
                if (&rp == pl) return true;
            return false;
        };
        (void)hipGetLastError();
        if (!recording(&pool)) trim(pool);
        if (recording(&pool) || hipMalloc(&p, rounded) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();          // (buffers released by passes still in flight on the lanes)
            trim(ctx->pool);
            for (auto& ln : ctx->lanes) trim(ln.pool);
            for (auto& lane_pools : ctx->rec_pools)
                for (auto& pl : lane_pools)
                    if (!recording(&pl)) trim(pl);
            if (hipMalloc(&p, rounded) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        }
    }
    pool.push_back({p, rounded, true});
    *size = rounded;
    return p;
}
// tpz_ctx_set_poison: 0xFF over the whole buffer, ordered ahead of whatever the new holder launches -- on the current stream (the
// ctx stream or the lane's that lane_enter made current), or as a recorded op of the current image of a batched pass, which
// rec_flush replays in its place in that image's list.  Not a launch of the ledger (n_launches) and not timed by the profiler.
static void poison_fill(tpz_ctx* ctx, void* p, size_t size) {
    ++ctx->n_poison_fills;
    ctx->poison_bytes += (long long)size;
    if (ctx->rec_on) {
        RecOp op;
        op.fn = [=](hipStream_t st) { return hipMemsetAsync(p, 0xFF, size, st); };
        op.fill = true;
        ctx->rec[ctx->rec_cur].push_back(std::move(op));
        return;
    }
    (void)hipMemsetAsync(p, 0xFF, size, ctx->stream);
}
WorkBuf::WorkBuf(tpz_ctx* ctx, size_t bytes) : pool_(ctx->pool_cur) {
    size_t size = 0;
    p_ = pool_alloc(ctx, *pool_, bytes, &size);
    if (ctx->poison && p_) poison_fill(ctx, p_, size);
}
// (by device pointer, not by index: a trim of the pool erases entries)
void WorkBuf::release() {
    if (p_)
        for (auto& b : *pool_)
            if (b.p == p_) { b.used = false; break; }
    p_ = nullptr;
}

// ---- the overflow flag of a 2xf16 pass: cleared on the ctx stream before the pass, read back once the stream has drained
hipError_t flag_clear(tpz_ctx* ctx) { return hipMemsetAsync(ctx->d_flag, 0, sizeof(unsigned), ctx->stream); }
hipError_t flag_read(tpz_ctx* ctx, unsigned* flag, bool check_copy) {
    const hipError_t copied = hipMemcpyAsync(ctx->h_flag, ctx->d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t drained = hipStreamSynchronize(ctx->stream);
    *flag = *ctx->h_flag;
    return check_copy && copied != hipSuccess ? copied : drained;
}

float* next_nrm(tpz_ctx* ctx) {
    if (ctx->nrm_next >= NRM_RING) {
        if (ctx->lanes_on) (void)hipDeviceSynchronize();     // the other lane may still read blocks of this ring
        else (void)hipStreamSynchronize(ctx->stream);
        ctx->nrm_next = 0;
    }
    return ctx->d_nrm + 4 * (ctx->nrm_next++);
}

// ---- patch lanes (tpz_ctx::Lane)
int lanes_begin(tpz_ctx* ctx) {
    if (!ctx->lanes_enabled || ctx->lanes_on) return 0;
    if (!ctx->lanes_fork) {
        if (hipEventCreateWithFlags(&ctx->lanes_fork, hipEventDisableTiming) != hipSuccess) return fail(ctx, "hipEventCreate failed");
        for (auto& ln : ctx->lanes) {
            if (hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&ln.done, hipEventDisableTiming) != hipSuccess ||
                hipMalloc((void**)&ln.d_part, 2 * PART_BLOCKS * sizeof(double)) != hipSuccess)
                return fail(ctx, "patch lanes: stream / event / scratch creation failed");
        }
    }
    // the lanes start after everything already queued on the ctx stream (the input image, the cleared overflow flag)
    HIPCHK(ctx, hipEventRecord(ctx->lanes_fork, ctx->stream));
    for (auto& ln : ctx->lanes) HIPCHK(ctx, hipStreamWaitEvent(ln.stream, ctx->lanes_fork, 0));
    ctx->lanes_saved_stream = ctx->stream;
    ctx->lanes_saved_part = ctx->d_part;
    ctx->lanes_on = true;
    ctx->lanes_live = ctx->n_lanes;
    return 0;
}
void lane_enter(tpz_ctx* ctx, int k) {
    if (!ctx->lanes_on) return;
    tpz_ctx::Lane& ln = ctx->lanes[k % ctx->lanes_live];
    ctx->stream = ln.stream;
    ctx->pool_cur = &ln.pool;
    ctx->d_part = ln.d_part;
}
int lanes_end(tpz_ctx* ctx) {
    if (!ctx->lanes_on) return 0;
    ctx->stream = ctx->lanes_saved_stream;
    ctx->pool_cur = &ctx->pool;
    ctx->d_part = ctx->lanes_saved_part;
    ctx->lanes_on = false;
    for (auto& ln : ctx->lanes) {
        HIPCHK(ctx, hipEventRecord(ln.done, ln.stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ln.done, 0));
    }
    return 0;
}

// ---- profiling helpers
void prof_begin(tpz_ctx* ctx, int cls, double flops, const void* key, double bytes) {
    ctx->prof_open = false;
    if (!ctx->prof) return;
    if (ctx->prof == 2 && (cls != 0 || flops < 2e10)) return;
    ctx->prof_open = true;
    ProfRec r;
    r.cls = cls;
    r.flops = flops;
    r.bytes = bytes;
    r.key = key;
    auto get = [&]() {
        hipEvent_t e;
        if (!ctx->free_events.empty()) { e = ctx->free_events.back(); ctx->free_events.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    r.e0 = get();
    r.e1 = get();
    (void)hipEventRecord(r.e0, ctx->stream);
    ctx->recs.push_back(r);
}
void prof_end(tpz_ctx* ctx) {
    if (!ctx->prof_open || ctx->recs.empty()) return;
    ctx->prof_open = false;
    (void)hipEventRecord(ctx->recs.back().e1, ctx->stream);
}
void prof_flush(tpz_ctx* ctx) {
    if (ctx->recs.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& r : ctx->recs) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        ctx->acc_ms[r.cls] += ms;
        ctx->acc_n[r.cls] += 1;
        ctx->acc_flops[r.cls] += r.flops;
        if (r.key) {
            ProfAcc* a = nullptr;
            for (auto& kv : ctx->per_kernel)
                if (kv.first == r.key) a = &kv.second;
            if (!a) { ctx->per_kernel.push_back({r.key, ProfAcc()}); a = &ctx->per_kernel.back().second; }
            a->ms += ms; a->flops += r.flops; a->bytes += r.bytes; a->n += 1;
        }
        ctx->free_events.push_back(r.e0);
        ctx->free_events.push_back(r.e1);
    }
    ctx->recs.clear();
}

// `batch_no`: consecutive batches alternate on the patch lanes (lane_enter: the lane's stream and reduction scratch), so that
// one batch's elementwise launches and small grids run under the other's large ones -- batches of 8 images, two in flight
int rec_begin(tpz_ctx* ctx, int batch_no) {
    if (ctx->dbg.trace_host) ctx->rec_t0 = host_now_ms();
    for (auto& r : ctx->rec) r.clear();
    lane_enter(ctx, batch_no);                  // (no-op without lanes: everything on the ctx stream)
    ctx->rec_lane = ctx->lanes_on ? batch_no % ctx->lanes_live : 0;
    ctx->rec_on = true;
    ctx->rec_cur = 0;
    ctx->pool_cur = &ctx->rec_pools[ctx->rec_lane][0];
    return 0;
}
// image i of the batch: its launches are recorded in its own list, its tensors come from its own pool (the images of a batch
// run interleaved: nothing of one may alias anything of another)
void rec_select(tpz_ctx* ctx, int i) {
    ctx->rec_cur = i;
    ctx->pool_cur = &ctx->rec_pools[ctx->rec_lane][i];
}
// leaves a batched pass: whatever is still recorded (an error on the way) is dropped
void rec_abort(tpz_ctx* ctx) {
    ctx->rec_on = false;
    ctx->pool_cur = &ctx->pool;
    for (auto& r : ctx->rec) r.clear();
}
// Issue everything recorded.  Every list keeps its own order (the dependencies inside an image); across the lists the
// launches are independent, so each round first replays the non-convolution launches at the head of every list and then takes
// the conv_split launch at the head of the first unfinished list together with every other list's head that is the same
// kernel in the same mode with the same K-loop plan: one grid.
int rec_flush(tpz_ctx* ctx) {
    ctx->rec_on = false;
    ctx->pool_cur = &ctx->pool;
    const double t_flush0 = ctx->dbg.trace_host ? host_now_ms() : 0.0;
    long long n_issued = 0;
    const int n = (int)tpz::SPLIT_MULTI_MAX;
    size_t cur[tpz::SPLIT_MULTI_MAX] = {};
    int rc = 0;
    for (;;) {
        bool any = false;
        for (int i = 0; i < n && !rc; ++i) {
            auto& L = ctx->rec[i];
            while (cur[i] < L.size() && !L[cur[i]].ks && !rc) {
                RecOp& op = L[cur[i]++];
                if (op.fill) {                  // (a poison fill: no launch of the ledger)
                    if (op.fn(ctx->stream) != hipSuccess) rc = fail(ctx, "poison fill failed");
                    continue;
                }
                prof_begin(ctx, op.cls, op.flops, op.key, op.bytes);
                const hipError_t e = op.fn(ctx->stream);
                prof_end(ctx);
                ++ctx->n_launches;
                ++n_issued;
                if (e != hipSuccess) rc = fail(ctx, "launch failed: %s", hipGetErrorString(e));
            }
            if (cur[i] < L.size()) any = true;
        }
        if (rc || !any) break;
        int lead = -1;
        for (int i = 0; i < n; ++i)
            if (cur[i] < ctx->rec[i].size()) { lead = i; break; }
        const RecOp& o0 = ctx->rec[lead][cur[lead]];
        const SplitArgs* list[tpz::SPLIT_MULTI_MAX];
        int who[tpz::SPLIT_MULTI_MAX], m = 0;
        double flops = 0, bytes = 0;
        for (int i = lead; i < n; ++i) {
            if (cur[i] >= ctx->rec[i].size()) continue;
            const RecOp& o = ctx->rec[i][cur[i]];
            if (o.ks != o0.ks || o.a.plan != o0.a.plan || split_mode_of(o.a) != split_mode_of(o0.a)) continue;
            // only what conv_split_multi_kernel is instantiated for merges (modes 0 / 1 / 2 / 11): a plane-stacked two-source
            // launch whose chunks mix both tensors (MODE 3: odd widths of a user-trained 3-D U-Net, TPZ_NO_SRCMAJOR) goes alone
            if (i != lead && (!o0.ks->launch_multi || split_mode_of(o0.a) == 3)) continue;
            list[m] = &o.a; who[m++] = i;
            flops += o.flops; bytes += o.bytes;
        }
        prof_begin(ctx, 0, flops, o0.ks->name, bytes);
        hipError_t e;
        if (m == 1) {
            SplitArgs a1 = o0.a;
            a1.n_tiles = 0;                    // (a launch of its own: n_tiles > 0 would select the persistent kernel)
            e = o0.ks->launch(a1, o0.grid, ctx->stream);
        } else {
            e = o0.ks->launch_multi(list, m, ctx->stream);
        }
        prof_end(ctx);
        ++ctx->n_launches;
        ++ctx->n_walk[m == 1 ? WALK_PLAIN : WALK_MULTI];
        ++n_issued;
        if (e != hipSuccess) rc = fail(ctx, "conv_split launch failed: %s", hipGetErrorString(e));
        for (int k = 0; k < m; ++k) ++cur[who[k]];
    }
    if (ctx->dbg.trace_host) {
        size_t n_ops = 0;
        int n_img = 0;
        for (auto& r : ctx->rec) { n_ops += r.size(); n_img += r.empty() ? 0 : 1; }
        fprintf(stderr, "[tpz host] batch of %d images: %zu launches recorded in %.3f ms, issued as %lld in %.3f ms\n", n_img, n_ops,
                t_flush0 - ctx->rec_t0, n_issued, host_now_ms() - t_flush0);
    }
    for (auto& r : ctx->rec) r.clear();
    return rc;
}

}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_debug_switches(char* buf, int buf_len) {
    const DebugEnv d = debug_env();
    std::string s;
    int n = 0;
    auto add = [&](bool on, const char* name) { if (on) { if (!s.empty()) s += ' '; s += name; ++n; } };
    add(d.no_phase, "no_phase"); add(d.exact_fp32, "exact_fp32"); add(d.no_issuer, "no_issuer"); add(d.no_lanes, "no_lanes");
    add(d.no_roi, "no_roi"); add(d.no_persist, "no_persist"); add(d.trace_host, "trace_host"); add(d.no_range, "no_range");
    add(d.no_raster, "no_raster"); add(d.no_srcmajor, "no_srcmajor"); add(d.no_valu_last, "no_valu_last"); add(d.no_rw, "no_rw");
    add(d.no_pool3d, "no_pool3d"); add(d.no_fold, "no_fold"); add(d.no_widen, "no_widen"); add(d.batch >= 0, "batch");
    add(d.lanes != 0, "lanes"); add(d.poison, "poison");
    if (buf && buf_len > 0) snprintf(buf, (size_t)buf_len, "%s", s.c_str());
    return n;
}

const char* tpz_version(void) { return "topaz_hip 0.1 (gfx950)"; }

const char* tpz_last_error(tpz_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int tpz_ctx_create(int device_id, tpz_ctx** out) {
    if (!out) return fail(nullptr, "tpz_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, "tpz_ctx_create: no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, "tpz_ctx_create: device %d of %d", device_id, ndev);
    tpz_ctx* ctx = new tpz_ctx();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) { delete ctx; return fail(nullptr, "hipSetDevice(%d) failed", device_id); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            delete ctx;
            return fail(nullptr, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id,
                        prop.gcnArchName);
        }
        if (prop.multiProcessorCount > 0) ctx->n_cus = prop.multiProcessorCount;
    }
    // the debug switches (all off without TPZ_DEBUG=1) become this context's defaults; each has a tpz_ctx_set_* twin
    ctx->dbg = debug_env();
    ctx->lanes_enabled = !ctx->dbg.no_lanes;
    ctx->roi_enabled = !ctx->dbg.no_roi;
    ctx->persist_mode = ctx->dbg.no_persist ? 0 : 1;
    ctx->range_scaling = !ctx->dbg.no_range;
    ctx->raster = !ctx->dbg.no_raster;
    ctx->exact = ctx->dbg.exact_fp32;
    ctx->poison = ctx->dbg.poison;
    if (ctx->dbg.batch >= 0) ctx->batch = ctx->dbg.batch;
    if (ctx->dbg.lanes >= 2 && ctx->dbg.lanes <= N_LANES) ctx->n_lanes = ctx->dbg.lanes;
    if (hipStreamCreate(&ctx->own_stream) != hipSuccess) { delete ctx; return fail(nullptr, "hipStreamCreate failed"); }
    ctx->stream = ctx->own_stream;
    if (hipMalloc((void**)&ctx->d_part, 2 * PART_BLOCKS * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&ctx->d_nrm, 4 * NRM_RING * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&ctx->d_counters, NMS_COUNTERS * sizeof(unsigned int)) != hipSuccess ||
        hipMalloc((void**)&ctx->d_flag, 16) != hipSuccess || hipHostMalloc((void**)&ctx->h_flag, 16) != hipSuccess ||
        hipMalloc((void**)&ctx->d_absmax, 1024) != hipSuccess || hipMemset(ctx->d_absmax, 0, 1024) != hipSuccess ||
        hipMalloc((void**)&ctx->d_zeros, 256) != hipSuccess || hipMemset(ctx->d_zeros, 0, 256) != hipSuccess) {
        delete ctx;
        return fail(nullptr, "tpz_ctx_create: hipMalloc failed");
    }
    *out = ctx;
    return 0;
}

void tpz_ctx_destroy(tpz_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipDeviceSynchronize();
    if (ctx->io_stage) tpz_stage_free(ctx->io_stage);
    for (auto& b : ctx->pool) (void)hipFree(b.p);
    for (auto& lane_pools : ctx->rec_pools)
        for (auto& rp : lane_pools)
            for (auto& b : rp) (void)hipFree(b.p);
    for (auto& ln : ctx->lanes) {
        for (auto& b : ln.pool) (void)hipFree(b.p);
        if (ln.d_part) (void)hipFree(ln.d_part);
        if (ln.done) (void)hipEventDestroy(ln.done);
        if (ln.stream) (void)hipStreamDestroy(ln.stream);
    }
    if (ctx->lanes_fork) (void)hipEventDestroy(ctx->lanes_fork);
    (void)hipFree(ctx->d_part);
    (void)hipFree(ctx->d_nrm);
    (void)hipFree(ctx->d_counters);
    (void)hipFree(ctx->d_zeros);
    (void)hipFree(ctx->d_flag);
    (void)hipFree(ctx->d_absmax);
    (void)hipHostFree(ctx->h_flag);
    for (auto& e : ctx->split_plans) (void)hipFree(e.d);
    for (auto e : ctx->free_events) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int tpz_ctx_set_stream(tpz_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    (void)hipStreamSynchronize(ctx->stream);
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return 0;
}

int tpz_ctx_sync(tpz_ctx* ctx) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int tpz_ctx_set_lanes(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    if (on < 0 || on > N_LANES) return fail(ctx, "tpz_ctx_set_lanes: 0 (off), 1 (on, two lanes) or a lane count up to %d", (int)N_LANES);
    ctx->lanes_enabled = on != 0;
    if (on >= 1) ctx->n_lanes = on == 1 ? 2 : on;
    return 0;
}

int tpz_ctx_set_batch(tpz_ctx* ctx, int n) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    if (n < 0 || n > (int)SPLIT_MULTI_MAX) return fail(ctx, "tpz_ctx_set_batch: 0 (off) or up to %d images per launch", (int)SPLIT_MULTI_MAX);
    ctx->batch = n == 1 ? 0 : n;
    return 0;
}
int tpz_ctx_set_batch_memory(tpz_ctx* ctx, long long bytes) {
    if (!ctx || bytes < 0) return fail(ctx, "tpz_ctx_set_batch_memory: bytes >= 0 (0: 90 %% of the free device memory)");
    ctx->batch_mem = bytes;
    return 0;
}
long long tpz_prof_launches(tpz_ctx* ctx) { return ctx ? ctx->n_launches : 0; }
int tpz_ctx_pool_stats(tpz_ctx* ctx, long long* buffers, long long* bytes, long long* buffers_in_use) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    long long n = 0, b = 0, u = 0;
    auto add = [&](const std::vector<tpz_ctx::Buf>& pl) {
        for (const auto& e : pl) { ++n; b += (long long)e.bytes; u += e.used ? 1 : 0; }
    };
    add(ctx->pool);
    for (const auto& ln : ctx->lanes) add(ln.pool);
    for (const auto& lane_pools : ctx->rec_pools)
        for (const auto& pl : lane_pools) add(pl);
    if (buffers) *buffers = n;
    if (bytes) *bytes = b;
    if (buffers_in_use) *buffers_in_use = u;
    return 0;
}

int tpz_ctx_set_poison(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    ctx->poison = on != 0;
    return 0;
}
int tpz_ctx_poison_stats(tpz_ctx* ctx, int* on, long long* fills, long long* bytes) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    if (on) *on = ctx->poison ? 1 : 0;
    if (fills) *fills = ctx->n_poison_fills;
    if (bytes) *bytes = ctx->poison_bytes;
    return 0;
}
int tpz_ctx_walk_stats(tpz_ctx* ctx, long long out[5]) {
    if (!ctx || !out) return fail(ctx, "tpz_ctx_walk_stats: NULL argument");
    static_assert(N_WALKS == 5, "tpz_ctx_walk_stats reports five walks");
    for (int i = 0; i < N_WALKS; ++i) out[i] = ctx->n_walk[i];
    return 0;
}
int tpz_debug_workspace_peek(tpz_ctx* ctx, size_t bytes, void* host_out) {
    if (!ctx || !host_out) return fail(ctx, "tpz_debug_workspace_peek: NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (bytes == 0) bytes = 16;
    // every pool buffer is whole MiB: the copy covers the rounded request -- all of a new buffer, the head of a larger cached one
    const size_t rounded = (bytes + (1u << 20) - 1) & ~((size_t)(1u << 20) - 1);
    std::vector<tpz_ctx::Buf>* const saved = ctx->pool_cur;
    ctx->pool_cur = &ctx->pool;
    int rc = 0;
    {
        const WorkBuf buf(ctx, bytes);
        if (!buf) rc = fail(ctx, "out of device memory");
        else if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
                 hipMemcpy(host_out, buf.as<void>(), rounded, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, "tpz_debug_workspace_peek: copy failed");
    }
    ctx->pool_cur = saved;
    return rc;
}

int tpz_ctx_set_persist(tpz_ctx* ctx, int mode, int workgroups) {
    if (!ctx || mode < 0 || mode > 2 || workgroups < 0) return fail(ctx, "tpz_ctx_set_persist: bad arguments");
    ctx->persist_mode = mode;
    ctx->persist_wgs = workgroups;
    return 0;
}
int tpz_ctx_set_roi(tpz_ctx* ctx, int on) {
    if (!ctx) return 1;
    ctx->roi_enabled = on != 0;
    return 0;
}

int tpz_ctx_set_tiling(tpz_ctx* ctx, long long limit_px, int tile) {
    if (!ctx || limit_px < 1 || tile < 16) return fail(ctx, "tpz_ctx_set_tiling: limit_px >= 1, tile >= 16");
    ctx->tile_limit_px = limit_px;
    ctx->tile_size = tile;
    return 0;
}

int tpz_ctx_set_raster(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    ctx->raster = on != 0;
    return 0;
}

int tpz_ctx_set_rw(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    ctx->rw_enabled = on != 0;
    return 0;
}
int tpz_ctx_set_range(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    ctx->range_scaling = on != 0;
    return 0;
}

int tpz_ctx_set_exact(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    ctx->exact = (on != 0) || ctx->dbg.exact_fp32;
    return 0;
}

int tpz_model_split_stats(tpz_model* m, int* eligible, long long* split_runs, long long* fp32_reruns) {
    if (!m) return fail(nullptr, "model is NULL");
    if (eligible) *eligible = m->split_ok ? 1 : 0;
    if (split_runs) *split_runs = m->n_split;
    if (fp32_reruns) *fp32_reruns = m->n_fallback;
    return 0;
}

int tpz_model_split_layers(tpz_model* m, int* n_conv, int* n_split, char* off_path, int off_path_len) {
    if (!m) return fail(nullptr, "model is NULL");
    if (n_conv) *n_conv = m->n_conv;
    if (n_split) *n_split = m->n_conv_split;
    if (off_path && off_path_len > 0) snprintf(off_path, (size_t)off_path_len, "%s", m->off_path.c_str());
    return 0;
}

// ---- profiling -----------------------------------------------------------------------------------
int tpz_prof_enable(tpz_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    prof_flush(ctx);
    ctx->prof = on == 2 ? 2 : (on != 0 ? 1 : 0);
    return 0;
}
int tpz_prof_reset(tpz_ctx* ctx) {
    if (!ctx) return fail(nullptr, "ctx is NULL");
    prof_flush(ctx);
    for (int i = 0; i < 4; ++i) { ctx->acc_ms[i] = 0; ctx->acc_n[i] = 0; ctx->acc_flops[i] = 0; }
    ctx->per_kernel.clear();
    return 0;
}
int tpz_prof_get_kernel(tpz_ctx* ctx, int rank, double* ms, long long* launches, double* flops, char* name,
                        int name_len) {
    if (!ctx || rank < 0) return fail(ctx, "tpz_prof_get_kernel: bad arguments");
    prof_flush(ctx);
    std::vector<std::pair<const void*, ProfAcc>> order(ctx->per_kernel);
    std::stable_sort(order.begin(), order.end(),
                     [](const std::pair<const void*, ProfAcc>& x, const std::pair<const void*, ProfAcc>& y) {
                         return x.second.ms > y.second.ms;
                     });
    const bool have = rank < (int)order.size();
    const ProfAcc acc = have ? order[rank].second : ProfAcc();
    if (ms) *ms = acc.ms;
    if (launches) *launches = acc.n;
    if (flops) *flops = acc.flops;
    if (name && name_len > 0) {
        name[0] = 0;
        if (have) snprintf(name, name_len, "%s", (const char*)order[rank].first);
    }
    return 0;
}
int tpz_prof_get_kernel_bytes(tpz_ctx* ctx, int rank, double* bytes) {
    if (!ctx || rank < 0 || !bytes) return fail(ctx, "tpz_prof_get_kernel_bytes: bad arguments");
    prof_flush(ctx);
    std::vector<std::pair<const void*, ProfAcc>> order(ctx->per_kernel);
    std::stable_sort(order.begin(), order.end(),
                     [](const std::pair<const void*, ProfAcc>& x, const std::pair<const void*, ProfAcc>& y) {
                         return x.second.ms > y.second.ms;
                     });
    *bytes = rank < (int)order.size() ? order[rank].second.bytes : 0.0;
    return 0;
}
int tpz_prof_mfma_sustained(tpz_ctx* ctx, int ms, int zero_operands, double* tflops, double* clock_ratio) {
    if (!ctx || ms < 1 || ms > 5000 || !tflops) return fail(ctx, "tpz_prof_mfma_sustained: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int n_wg = 2 * prop.multiProcessorCount;           // two 4-wave workgroups per CU: two waves per SIMD
    const size_t n_src = 4096 * 8;
    std::vector<_Float16> h(n_src);
    unsigned lcg = 12345u;
    for (auto& v : h) {
        lcg = lcg * 1664525u + 1013904223u;
        v = zero_operands ? (_Float16)0.f : (_Float16)(((int)(lcg >> 8) % 2001 - 1000) * 1e-3f);
    }
    void* d_src = nullptr; float* d_out = nullptr; unsigned long long* d_ticks = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    auto run = [&](int iters, float* t_ms) {
        hipError_t e = hipEventRecord(e0, ctx->stream);
        if (e == hipSuccess) e = launch_mfma_spin(d_src, d_out, n_wg, iters, d_ticks, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(t_ms, e0, e1);
        return e;
    };
    hipError_t e = hipMalloc(&d_src, n_src * sizeof(_Float16));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, (size_t)n_wg * 256 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&d_ticks, 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpy(d_src, h.data(), n_src * sizeof(_Float16), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float t = 0.f;
    const int probe = 20000;
    if (e == hipSuccess) e = run(probe, &t);                 // sizes the loop (and is the first of the warm-up)
    if (e == hipSuccess) {
        const int iters = (int)std::min(2.0e9, std::max(1000.0, probe * (double)ms / std::max(t, 1e-3f)));
        e = run(iters, &t);                                  // the power management settles within this one
        if (e == hipSuccess) e = run(iters, &t);
        unsigned long long ticks[2] = {};
        if (e == hipSuccess) e = hipMemcpy(ticks, d_ticks, sizeof(ticks), hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
            const double flop = 8.0 * 16 * 16 * 32 * 2 * (double)iters * n_wg * 4;
            *tflops = flop / (t * 1e-3) * 1e-12;
            // s_memtime over s_memrealtime: proportional to the shader clock (both are read inside the loop's bracket)
            if (clock_ratio) *clock_ratio = ticks[1] ? (double)ticks[0] / (double)ticks[1] : 0.0;
        }
    }
    if (e != hipSuccess) rc = fail(ctx, "tpz_prof_mfma_sustained: %s", hipGetErrorString(e));
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d_src); (void)hipFree(d_out); (void)hipFree(d_ticks);
    return rc;
}
int tpz_prof_get_dominant(tpz_ctx* ctx, double* ms, long long* launches, double* flops, char* name, int name_len) {
    return tpz_prof_get_kernel(ctx, 0, ms, launches, flops, name, name_len);
}
int tpz_prof_get(tpz_ctx* ctx, int cls, double* ms, long long* launches, double* flops) {
    if (!ctx || cls < 0 || cls > 3) return fail(ctx, "tpz_prof_get: bad arguments");
    prof_flush(ctx);
    if (ms) *ms = ctx->acc_ms[cls];
    if (launches) *launches = ctx->acc_n[cls];
    if (flops) *flops = ctx->acc_flops[cls];
    return 0;
}
