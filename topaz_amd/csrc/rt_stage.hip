// Staging ring (pinned host buffer + device buffer + events per slot, one copy stream) and the host-pointer entry points.
#include "rt_internal.h"

// ---- staging ring: pinned host buffer + device buffer + events per slot, one copy stream ----------------------
struct tpz_stage {
    tpz_ctx* ctx = nullptr;
    size_t slot_bytes = 0;
    hipStream_t copy = nullptr;
    struct Slot {
        void* h = nullptr;
        void* d = nullptr;
        hipEvent_t ready = nullptr;       // last copy of this slot (either direction) finished
        hipEvent_t released = nullptr;    // kernels reading / writing the device buffer are done with it
        hipEvent_t produced = nullptr;    // the result to copy back exists
    };
    std::vector<Slot> slots;
};

namespace tpz::rt {
namespace {

tpz_stage::Slot* stage_slot(tpz_stage* st, int slot) {
    return (st && slot >= 0 && slot < (int)st->slots.size()) ? &st->slots[slot] : nullptr;
}

// tpz_stage_h2d_decode: the stored pixels of an n-pixel image lie behind its fp32 form, at the next multiple of 256 bytes
size_t stage_raw_offset(size_t n) { return (4 * n + 255) & ~(size_t)255; }
// tpz_stage_d2h_encode: the 8-byte overflow counter of a result lies behind its encoded pixels, at the next multiple of 256 bytes
size_t stage_counter_offset(size_t pixel_bytes) { return (pixel_bytes + 255) & ~(size_t)255; }

// host-pointer entry points: two slots of the ctx's own ring (input, output), grown on demand
int io_stage(tpz_ctx* ctx, size_t bytes, tpz_stage** out) {
    if (ctx->io_stage && ctx->io_stage->slot_bytes < bytes) { tpz_stage_free(ctx->io_stage); ctx->io_stage = nullptr; }
    if (!ctx->io_stage && tpz_stage_create(ctx, (bytes + (1u << 20) - 1) & ~((size_t)(1u << 20) - 1), 2, &ctx->io_stage)) return 1;
    *out = ctx->io_stage;
    return 0;
}

}  // namespace

}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_stage_create(tpz_ctx* ctx, size_t slot_bytes, int depth, tpz_stage** out) {
    if (!ctx || !out || slot_bytes == 0 || depth < 1 || depth > 64) return fail(ctx, "tpz_stage_create: bad arguments");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    tpz_stage* st = new tpz_stage();
    st->ctx = ctx;
    st->slot_bytes = slot_bytes;
    st->slots.resize(depth);
    bool ok = hipStreamCreateWithFlags(&st->copy, hipStreamNonBlocking) == hipSuccess;
    for (auto& sl : st->slots) {
        ok = ok && hipHostMalloc(&sl.h, slot_bytes) == hipSuccess && hipMalloc(&sl.d, slot_bytes) == hipSuccess &&
             hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.released, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.produced, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) { tpz_stage_free(st); return fail(ctx, "tpz_stage_create: allocation of %d x %zu bytes failed", depth, slot_bytes); }
    *out = st;
    return 0;
}
void tpz_stage_free(tpz_stage* st) {
    if (!st) return;
    (void)hipSetDevice(st->ctx->device);
    if (st->copy) (void)hipStreamSynchronize(st->copy);
    (void)hipStreamSynchronize(st->ctx->stream);
    for (auto& sl : st->slots) {
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.d) (void)hipFree(sl.d);
        if (sl.ready) (void)hipEventDestroy(sl.ready);
        if (sl.released) (void)hipEventDestroy(sl.released);
        if (sl.produced) (void)hipEventDestroy(sl.produced);
    }
    if (st->copy) (void)hipStreamDestroy(st->copy);
    delete st;
}
void* tpz_stage_host_ptr(tpz_stage* st, int slot) { auto* s = stage_slot(st, slot); return s ? s->h : nullptr; }
void* tpz_stage_device_ptr(tpz_stage* st, int slot) { auto* s = stage_slot(st, slot); return s ? s->d : nullptr; }
int tpz_stage_h2d(tpz_stage* st, int slot, const void* h_src, size_t bytes) {
    auto* sl = stage_slot(st, slot);
    if (!sl || bytes > st->slot_bytes) return fail(st ? st->ctx : nullptr, "tpz_stage_h2d: bad slot or size");
    tpz_ctx* ctx = st->ctx;
    if (h_src && h_src != sl->h) {
        // the pinned buffer may still be the source / target of this slot's previous copy
        HIPCHK(ctx, hipEventSynchronize(sl->ready));
        memcpy(sl->h, h_src, bytes);
    }
    HIPCHK(ctx, hipStreamWaitEvent(st->copy, sl->released, 0));      // kernels of the slot's previous use are done
    HIPCHK(ctx, hipMemcpyAsync(sl->d, sl->h, bytes, hipMemcpyHostToDevice, st->copy));
    HIPCHK(ctx, hipEventRecord(sl->ready, st->copy));
    return 0;
}
size_t tpz_stage_decode_bytes(int mrc_mode, size_t n) {
    const size_t item = stored_itemsize(mrc_mode);
    if (item == 0 || n > ((size_t)1 << 60)) return 0;
    return stage_raw_offset(n) + ((n * item + 255) & ~(size_t)255);
}
int tpz_stage_h2d_decode(tpz_stage* st, int slot, int mrc_mode, size_t n) {
    auto* sl = stage_slot(st, slot);
    tpz_ctx* ctx = st ? st->ctx : nullptr;
    if (!sl) return fail(ctx, "tpz_stage_h2d_decode: bad slot");
    const size_t item = stored_itemsize(mrc_mode), need = tpz_stage_decode_bytes(mrc_mode, n);
    if (item == 0) return fail(ctx, "tpz_stage_h2d_decode: MRC mode %d is not one of the stored real types 0, 1, 6, 12", mrc_mode);
    if (n > ((size_t)1 << 60) || need > st->slot_bytes)
        return fail(ctx, "tpz_stage_h2d_decode: %zu pixels of mode %d need a slot of %zu bytes, this ring has %zu", n, mrc_mode,
                    need, st->slot_bytes);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // stored pixels behind the fp32 image they decode into; the decode runs on the copy stream, between the copy and the event,
    // so `ready` means what it means after tpz_stage_h2d: an fp32 image at the start of the slot
    void* d_raw = (char*)sl->d + stage_raw_offset(n);
    HIPCHK(ctx, hipStreamWaitEvent(st->copy, sl->released, 0));      // kernels of the slot's previous use are done
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(d_raw, sl->h, n * item, hipMemcpyHostToDevice, st->copy));
        HIPCHK(ctx, launch_decode(d_raw, mrc_mode, n, (float*)sl->d, st->copy));
    }
    HIPCHK(ctx, hipEventRecord(sl->ready, st->copy));
    return 0;
}
int tpz_stage_acquire(tpz_stage* st, int slot) {
    auto* sl = stage_slot(st, slot);
    if (!sl) return fail(st ? st->ctx : nullptr, "tpz_stage_acquire: bad slot");
    HIPCHK(st->ctx, hipStreamWaitEvent(st->ctx->stream, sl->ready, 0));
    return 0;
}
int tpz_stage_release(tpz_stage* st, int slot) {
    auto* sl = stage_slot(st, slot);
    if (!sl) return fail(st ? st->ctx : nullptr, "tpz_stage_release: bad slot");
    HIPCHK(st->ctx, hipEventRecord(sl->released, st->ctx->stream));
    return 0;
}
int tpz_stage_d2h(tpz_stage* st, int slot, const void* d_src, size_t bytes) {
    auto* sl = stage_slot(st, slot);
    if (!sl || !d_src || bytes > st->slot_bytes) return fail(st ? st->ctx : nullptr, "tpz_stage_d2h: bad slot or size");
    tpz_ctx* ctx = st->ctx;
    HIPCHK(ctx, hipEventRecord(sl->produced, ctx->stream));           // everything queued so far produced d_src
    HIPCHK(ctx, hipStreamWaitEvent(st->copy, sl->produced, 0));
    HIPCHK(ctx, hipMemcpyAsync(sl->h, d_src, bytes, hipMemcpyDeviceToHost, st->copy));
    HIPCHK(ctx, hipEventRecord(sl->ready, st->copy));
    return 0;
}
size_t tpz_stage_encode_bytes(int enc, size_t n) {
    const size_t item = encoded_itemsize(enc);
    if (item == 0 || n > ((size_t)1 << 60)) return 0;
    return stage_counter_offset(n * item) + 256;
}
int tpz_stage_d2h_encode(tpz_stage* st, int slot, const float* d_src, size_t n, int enc, const float* params) {
    auto* sl = stage_slot(st, slot);
    tpz_ctx* ctx = st ? st->ctx : nullptr;
    if (!sl || !d_src) return fail(ctx, "tpz_stage_d2h_encode: bad slot or NULL source");
    const size_t item = encoded_itemsize(enc), need = tpz_stage_encode_bytes(enc, n);
    if (item == 0) return fail(ctx, "tpz_stage_d2h_encode: encoding %d is neither TPZ_ENC_F16 nor TPZ_ENC_U8", enc);
    if (enc == ENC_U8 && !params) return fail(ctx, "tpz_stage_d2h_encode: TPZ_ENC_U8 needs params = {mi, ma}");
    if (need == 0 || need > st->slot_bytes)
        return fail(ctx, "tpz_stage_d2h_encode: %zu pixels of encoding %d need a slot of %zu bytes, this ring has %zu", n, enc, need,
                    st->slot_bytes);
    if (((uintptr_t)d_src & 3) || ((const char*)d_src < (const char*)sl->d + st->slot_bytes &&
                                   (const char*)d_src + 4 * n > (const char*)sl->d))
        return fail(ctx, "tpz_stage_d2h_encode: d_src must be 4-byte aligned and lie outside the slot's device buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // encoded pixels at the start of the slot's device buffer, the overflow counter behind them; the encode runs on the copy
    // stream, between the `produced` event and the copy, so `ready` means: encoded pixels and counter are in the pinned slot
    const size_t off = stage_counter_offset(n * item);
    unsigned long long* d_count = (unsigned long long*)((char*)sl->d + off);
    const float mi = enc == ENC_U8 ? params[0] : 0.0f, ma = enc == ENC_U8 ? params[1] : 1.0f;
    HIPCHK(ctx, hipEventRecord(sl->produced, ctx->stream));           // everything queued so far produced d_src
    HIPCHK(ctx, hipStreamWaitEvent(st->copy, sl->produced, 0));
    HIPCHK(ctx, hipStreamWaitEvent(st->copy, sl->released, 0));      // kernels of the slot's previous use are done
    HIPCHK(ctx, hipMemsetAsync(d_count, 0, 8, st->copy));
    HIPCHK(ctx, launch_encode(d_src, enc, n, mi, ma, sl->d, d_count, st->copy));
    HIPCHK(ctx, hipMemcpyAsync(sl->h, sl->d, off + 8, hipMemcpyDeviceToHost, st->copy));
    HIPCHK(ctx, hipEventRecord(sl->ready, st->copy));
    return 0;
}
int tpz_stage_wait(tpz_stage* st, int slot) {
    auto* sl = stage_slot(st, slot);
    if (!sl) return fail(st ? st->ctx : nullptr, "tpz_stage_wait: bad slot");
    HIPCHK(st->ctx, hipEventSynchronize(sl->ready));
    return 0;
}

int tpz_score_2d_host(tpz_model* m, const float* h_in, int H, int W, float* h_out_logits) {
    if (!m || !h_in || !h_out_logits || H < 1 || W < 1) return fail(m ? m->ctx : nullptr, "tpz_score_2d_host: bad arguments");
    tpz_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int Do, Ho, Wo;
    tpz_model_out_shape(m, 1, H, W, &Do, &Ho, &Wo);
    if (Ho < 1 || Wo < 1) return fail(ctx, "input %dx%d too small for this model", H, W);
    const size_t nin = (size_t)H * W * sizeof(float), nout = (size_t)Ho * Wo * sizeof(float);
    tpz_stage* st;
    if (io_stage(ctx, std::max(nin, nout), &st)) return 1;
    if (tpz_stage_h2d(st, 0, h_in, nin) || tpz_stage_acquire(st, 0)) return 1;
    if (tpz_model_forward(m, (const float*)tpz_stage_device_ptr(st, 0), 1, 1, H, W, (float*)tpz_stage_device_ptr(st, 1))) return 1;
    if (tpz_stage_release(st, 0) || tpz_stage_d2h(st, 1, tpz_stage_device_ptr(st, 1), nout) || tpz_stage_wait(st, 1)) return 1;
    memcpy(h_out_logits, tpz_stage_host_ptr(st, 1), nout);
    return tpz_stage_release(st, 1);
}
int tpz_denoise_2d_host(tpz_model* m, const float* h_in, int H, int W, int patch, int pad, float* h_out) {
    if (!m || !h_in || !h_out || H < 1 || W < 1) return fail(m ? m->ctx : nullptr, "tpz_denoise_2d_host: bad arguments");
    tpz_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)H * W * sizeof(float);
    tpz_stage* st;
    if (io_stage(ctx, nb, &st)) return 1;
    if (tpz_stage_h2d(st, 0, h_in, nb) || tpz_stage_acquire(st, 0)) return 1;
    if (tpz_denoise_2d(m, (const float*)tpz_stage_device_ptr(st, 0), H, W, patch, pad, (float*)tpz_stage_device_ptr(st, 1))) return 1;
    if (tpz_stage_release(st, 0) || tpz_stage_d2h(st, 1, tpz_stage_device_ptr(st, 1), nb) || tpz_stage_wait(st, 1)) return 1;
    memcpy(h_out, tpz_stage_host_ptr(st, 1), nb);
    return tpz_stage_release(st, 1);
}
int tpz_resample_2d_host(tpz_resample* plan, const float* h_in, float* h_out) {
    tpz_ctx* ctx = resample_ctx(plan);
    if (!plan || !h_in || !h_out) return fail(ctx, "tpz_resample_2d_host: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int M, N, m, n;
    tpz_resample_shape(plan, &M, &N, &m, &n);
    const size_t nin = (size_t)M * N * sizeof(float), nout = (size_t)m * n * sizeof(float);
    tpz_stage* st;
    if (io_stage(ctx, nin, &st)) return 1;
    if (tpz_stage_h2d(st, 0, h_in, nin) || tpz_stage_acquire(st, 0)) return 1;
    if (tpz_resample_run(plan, (const float*)tpz_stage_device_ptr(st, 0), (float*)tpz_stage_device_ptr(st, 1))) return 1;
    if (tpz_stage_release(st, 0) || tpz_stage_d2h(st, 1, tpz_stage_device_ptr(st, 1), nout) || tpz_stage_wait(st, 1)) return 1;
    memcpy(h_out, tpz_stage_host_ptr(st, 1), nout);
    return tpz_stage_release(st, 1);
}
int tpz_nms_2d_host(tpz_ctx* ctx, const float* h_score, int H, int W, int r, float threshold, int32_t* h_coords,
                    float* h_scores, int cap, int* h_n) {
    if (!ctx || !h_score || !h_coords || !h_scores || H < 1 || W < 1 || cap < 0) return fail(ctx, "tpz_nms_2d_host: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)H * W * sizeof(float), ob = (size_t)std::max(cap, 1) * 3 * sizeof(float);
    tpz_stage* st;
    if (io_stage(ctx, std::max(nb, ob), &st)) return 1;
    if (tpz_stage_h2d(st, 0, h_score, nb) || tpz_stage_acquire(st, 0)) return 1;
    int32_t* d_coords = (int32_t*)tpz_stage_device_ptr(st, 1);
    float* d_scores = (float*)tpz_stage_device_ptr(st, 1) + (size_t)2 * std::max(cap, 1);
    int n = 0;
    const int rc = tpz_nms_2d(ctx, (const float*)tpz_stage_device_ptr(st, 0), H, W, r, threshold, d_coords, d_scores, cap, &n);
    if (h_n) *h_n = n;
    if (tpz_stage_release(st, 0)) return 1;
    if (rc) return rc;
    if (tpz_stage_d2h(st, 1, tpz_stage_device_ptr(st, 1), ob) || tpz_stage_wait(st, 1)) return 1;
    const size_t k = (size_t)std::min(n, cap);
    memcpy(h_coords, tpz_stage_host_ptr(st, 1), k * 2 * sizeof(int32_t));
    memcpy(h_scores, (const float*)tpz_stage_host_ptr(st, 1) + (size_t)2 * std::max(cap, 1), k * sizeof(float));
    return tpz_stage_release(st, 1);
}
