// Internal declarations of the libtopaz_hip.so runtime (NOT part of the C-ABI: include/topaz_hip.h is).  Everything here lives in
// namespace tpz::rt but the structs behind the C header's opaque handles (tpz_ctx, tpz_model), which the header declares at
// global scope.  The library exports the tpz_* functions only (libtopaz_hip.map); each runtime file keeps its own helpers in an
// anonymous namespace, defines the helpers other files share in tpz::rt and its tpz_* entry points last, at global scope.
// The runtime is split into translation units by concern:
//   rt_core.hip     kernel registries, the context (streams, workspace pools, patch lanes, the batched-launch recorder, the
//                   HIP-event profiler), its setters, the debug switches
//   rt_load.hip     model loading: the kernels each layer CAN run on and their weight packs (fp32 and 2xf16 forms, per-parity
//                   decoder forms, folded projections), zero-padded widths, the bias arena
//   rt_exec.hip     the layer-program executor: conv_plan() -- the one place that says which of those kernels a conv layer
//                   DOES run on, in which tensor formats (ConvForm / ConvPlan below) --, the launch window (launch_window, with
//                   its FLOP share and tile grid), launchers, per-layer drivers, the backward walk of the windows
//                   (need_regions), run_program with its slot helpers (make_dst, source_view)
//   rt_forward.hip  scoring drivers (range-scaled pass, internal tiling), the precision check of a loaded model
//                   (tpz_model_calibrate) and the single-op entry points
//   rt_denoise.hip  the patched 2-D and tiled 3-D denoising drivers (batched passes over the lanes)
//   rt_stats.hip    mean / std, GMM fit, affine, normalise, delta_stats
//   rt_preprocess.hip  the preprocess / normalize stream: radix-select order statistics, gather, the GMM fit with all
//                   initialisations per pass, the float64 normalise (kernels there too)
//   rt_stage.hip    the staging ring and the host-pointer entry points
//   rt_nms.hip      the NMS driver
//   rt_particles.hip  particle stacks: batched crop / standardise and frame resize (its kernels live there too)
//   rt_prefilter.hip  denoise pre-filters: fp64 low-pass GEMMs, tile covariances, the per-tile deconvolution filter (kernels there too)
//   rt_tiles.hip      score tiles: the zero-padded window cut, the all-zero flags of a tile grid, the cropped paste (kernels there too)
//   rt_resample.hip   the truncated-DFT resampler: plans with device-resident operators over the fp32-MFMA GEMM of resample_gemm.h
// Workspace ownership: temporary device memory is held by a WorkBuf (below), never by a bare pointer.  The handle takes its buffer
// from the pool that is current at that moment and remembers THAT pool, so its release -- scope exit, or release() where a
// buffer must go back earlier -- finds the buffer whatever lane_enter / rec_select have made current since.  A handle lives
// where the buffer is needed (per tile, per patch, per driver call) and no longer: the next request reuses what was released.
// Closures given to enqueue() capture the raw pointer (buf.as<T>() copied into a local), never the handle: in a batched pass
// they run at rec_flush, after the handle is gone, on a buffer nothing else takes from its per-image pool until then.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "../../include/topaz_hip.h"
#include "conv_registry.h"
#include "conv_split_registry.h"
#include "conv_rw.h"
#include "kernels_misc.h"

namespace tpz::rt {

// ---- debug / A-B switches ----------------------------------------------------------------------------------------------
// Every switch below changes how a job computes or is scheduled.  They exist for tools/ and tests/ (same-process A/B legs,
// bit-identity checks); a stray variable in a user's environment must not change a job, so the environment is consulted by ONE
// function, debug_env(), and only when TPZ_DEBUG=1 is set.  It is read when a context is created (the ctx keeps that copy:
// tpz_ctx::dbg) and again at every model load.  The settings that matter outside tests have a tpz_ctx_set_* entry point.
struct DebugEnv {
    bool on = false;             // TPZ_DEBUG=1
    bool no_phase = false;       // TPZ_NO_PHASE     keep the fused upsample+concat loader for every decoder layer
    bool exact_fp32 = false;     // TPZ_EXACT_FP32   every network on the fp32 MFMA kernels (tpz_ctx_set_exact)
    bool no_issuer = false;      // TPZ_NO_ISSUER    every wave issues its own share of the per-step LDS-DMA
    bool no_lanes = false;       // TPZ_NO_LANES     patches / tiles of an image on one stream only (tpz_ctx_set_lanes)
    bool no_roi = false;         // TPZ_NO_ROI       every layer of a patch computes its whole tensor (tpz_ctx_set_roi)
    bool no_persist = false;     // TPZ_NO_PERSIST   no persistent workgroups (tpz_ctx_set_persist)
    bool trace_host = false;     // TPZ_TRACE_HOST   host time of the recording / issuing phases of a batched pass, on stderr
    bool no_range = false;       // TPZ_NO_RANGE     no range-scaled scoring pass (tpz_ctx_set_range)
    bool no_raster = false;      // TPZ_NO_RASTER    row-major tile raster (tpz_ctx_set_raster)
    bool no_srcmajor = false;    // TPZ_NO_SRCMAJOR  plane-major virtual cells for two-source 3-D layers (MODE 3)
    bool no_valu_last = false;   // TPZ_NO_VALU_LAST the 1-output-channel last conv as a column kernel + shift-sum (round 4)
    bool no_rw = false;          // TPZ_NO_RW        no weights-resident kernel for the 3x3 32 -> 32 layers (tpz_ctx_set_rw)
    bool no_pool3d = false;      // TPZ_NO_POOL3D    no fused max-pool epilogue on 3-D encoder convs
    bool no_fold = false;        // TPZ_NO_FOLD      ResidA 1x1 projections as layers of their own
    bool no_widen = false;       // TPZ_NO_WIDEN     never load a program zero-padded to multiples of 16 channels
    bool poison = false;         // TPZ_POISON       every workspace buffer is filled with 0xFF bytes when it is taken (tpz_ctx_set_poison)
    int batch = -1;              // TPZ_BATCH=n / TPZ_NO_BATCH=1 (0)   images per batched pass (tpz_ctx_set_batch); -1: default
    int lanes = 0;               // TPZ_LANES=n      patch lanes in use (tpz_ctx_set_lanes); 0: default
};
DebugEnv debug_env();

static inline double host_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

#ifndef TPZ_N_LANES
#define TPZ_N_LANES 4
#endif
enum { N_LANES = TPZ_N_LANES };      // patch lanes: the most auxiliary streams the patches / tiles of an image alternate on
// the tile walk of a 2xf16 conv launch (tpz_ctx::n_walk): one workgroup per tile in row-major / XCD order, the patch raster
// (xcd_swizzle 2), persistent workgroups (MODE 4), the weights-resident kernel (conv_rw.h), the batched grid (conv_split_multi_kernel)
enum { WALK_PLAIN = 0, WALK_RASTER, WALK_PERSIST, WALK_RW, WALK_MULTI, N_WALKS };
enum { NMS_BATCH = 4, NMS_VER = 5, NMS_SNAP = 9, NMS_PICKS = 15, NMS_COUNTERS = 16 };

struct ProfRec {
    int cls;
    hipEvent_t e0, e1;
    double flops, bytes;  // algorithmic FLOP and HBM bytes of the launch (bytes: read inputs + weights once, write outputs once)
    const void* key;      // identity of the kernel instantiation (its registry name / a static label), nullptr for the rest
};
struct ProfAcc {
    double ms = 0, flops = 0, bytes = 0;
    long long n = 0;
};

// One deferred launch of a batched pass (tpz_ctx::rec): a conv_split launch (ks != nullptr: `a` complete but for the stream,
// a.n_tiles = the workgroups of `grid`) that rec_flush may merge with the same layer's launch of other images, or any other
// launch as a closure over its arguments.
struct RecOp {
    const SplitKernelInfo* ks = nullptr;
    SplitArgs a;
    dim3 grid;
    std::function<hipError_t(hipStream_t)> fn;
    int cls = 2;
    double flops = 0, bytes = 0;
    const void* key = nullptr;
    bool fill = false;           // a poison fill (WorkBuf): replayed in its place, counted neither as a launch nor by the profiler
};

}  // namespace tpz::rt

struct tpz_ctx {
    int device = 0;
    tpz::rt::DebugEnv dbg;        // the debug switches as they stood when the ctx was created (all off without TPZ_DEBUG=1)
    int n_cus = 256;              // compute units (persistent grids are sized from it)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    struct Buf {
        void* p;
        size_t bytes;
        bool used;
    };
    std::vector<Buf> pool;        // workspace of the ctx stream
    std::vector<Buf>* pool_cur = &pool;
    // Patch lanes: independent patches / tiles of one image are enqueued round-robin on N_LANES auxiliary streams, each
    // with its own workspace pool and reduction scratch, so that the small, latency-bound launches of one patch (the
    // deep U-Net levels: 16-tile grids on 256 CUs) run under the large ones of its neighbour (lanes_begin / lane_enter /
    // lanes_end).  One host thread enqueues everything; nothing synchronises with the host.
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        std::vector<Buf> pool;
        double* d_part = nullptr;
    };
    Lane lanes[tpz::rt::N_LANES];
    struct tpz_stage* io_stage = nullptr;     // ring behind the host-pointer entry points (created on first use)
    hipEvent_t lanes_fork = nullptr;
    hipStream_t lanes_saved_stream = nullptr;
    double* lanes_saved_part = nullptr;
    bool lanes_on = false;
    int lanes_live = 2;                       // ... of the lanes_begin in progress
    int n_lanes = 2;                          // lanes in use (<= N_LANES): tpz_ctx_set_lanes(ctx, n), TPZ_LANES
    bool lanes_enabled = true;                // tpz_ctx_set_lanes
    bool roi_enabled = true;                  // tpz_ctx_set_roi: patches compute only what their kept centre depends on
    int persist_mode = 1;                     // tpz_ctx_set_persist: 0 never, 1 large launches (default), 2 every eligible launch
    int persist_wgs = 0;                      // ... workgroups of a persistent grid (0: CUs x workgroups per CU)
    // Batched passes (rec_begin / rec_select / rec_flush): the launches of up to SPLIT_MULTI_MAX independent images (patches of
    // a micrograph, tiles of a tomogram) are RECORDED, image by image, each image on a workspace pool of its own, and then
    // issued layer by layer -- the conv_split launches of the same layer as ONE grid (conv_split_multi_kernel).  The deep
    // levels of a U-Net are 16-tile launches on a 256-CU chip; batched they are 8 x as large and 8 x fewer.
    int batch = (int)tpz::SPLIT_MULTI_MAX;    // images per batch (tpz_ctx_set_batch); 0: off (patch lanes)
    bool rec_on = false;
    double rec_t0 = 0;                        // (TPZ_TRACE_HOST)
    int rec_cur = 0;
    std::vector<tpz::rt::RecOp> rec[tpz::SPLIT_MULTI_MAX];
    std::vector<Buf> rec_pools[TPZ_N_LANES][tpz::SPLIT_MULTI_MAX];   // per lane (two batches are in flight at a time) and image
    int rec_lane = 0;
    long long batch_mem = 0;                  // tpz_ctx_set_batch_memory: device bytes a batched pass may take (0: what is free)
    long long n_launches = 0;                 // kernel launches issued (tpz_prof_launches)
    long long resample_upload_bytes = 0;      // operator bytes uploaded by tpz_resample_create (tpz_resample_upload_bytes)
    double* d_part = nullptr;     // reduction partials
    float* d_nrm = nullptr;       // ring of float[4] normalisation parameter blocks
    int nrm_next = 0;
    unsigned int* d_counters = nullptr;     // NMS_COUNTERS entries (nms_common)
    float* d_zeros = nullptr;     // 256 B of zeros: DMA source of padded / out-of-image elements
    // range-scaled scoring pass (tpz_model_forward): every bias-like vector is read `bias_shift` floats further on (the model's
    // scaled copy of its bias arena), the fused head adds no bias (the un-scaling pass does)
    ptrdiff_t bias_shift = 0;
    bool scaled_pass = false;
    unsigned* d_absmax = nullptr; // exponent histogram of launch_range_fit (256 words, kept zeroed)
    bool range_scaling = true;                // tpz_ctx_set_range
    bool raster = true;                       // tpz_ctx_set_raster: patch raster of the 8-wave tiles' grids
    bool rw_enabled = true;                   // tpz_ctx_set_rw: the weights-resident kernel for 3x3 32 -> 32 layers (conv_rw.h)
    // tpz_ctx_set_poison: a WorkBuf fills its whole pool buffer with 0xFF bytes when it takes it (every f16 / f32 / f64 a NaN, every
    // uint64_t the maximum, every int -1), so that a cell no kernel writes, or one read before it is written, shows in the result
    // instead of holding whatever the buffer's last tenant left -- often the right answer of the previous run
    bool poison = false;
    long long n_poison_fills = 0, poison_bytes = 0;      // tpz_ctx_poison_stats
    // conv launches by tile walk since the ctx was created (tpz_ctx_walk_stats)
    long long n_walk[tpz::rt::N_WALKS] = {0, 0, 0, 0, 0};
    // internal tiling of tpz_model_forward (run_image): 2-D images above tile_limit_px pixels are scored in tile_size^2 tiles
    long long tile_limit_px = 40LL << 20;
    int tile_size = 4096;
    unsigned* d_flag = nullptr;   // f16-range overflow flag of the 2xf16 path
    unsigned* h_flag = nullptr;   // pinned copy
    bool exact = false;           // fp32 kernels only (tpz_ctx_set_exact)
    // K-loop schedules of the 2xf16 kernels (conv_split.h SplitStep), built on first use per (kernel, layer shape) and kept
    // on the device for the life of the ctx: (kernel, key) -> device table
    struct SplitPlan {
        const tpz::SplitKernelInfo* ks;
        tpz::SplitPlanKey key;
        tpz::SplitStep* d;
        bool next_ok;             // holds a complete next-tile fetch: the persistent kernel may run this layer
    };
    std::vector<SplitPlan> split_plans;
    // profiling
    int prof = 0;                 // 0 off, 1 every launch, 2 conv launches of >= 20 GFLOP only (cheap enough for timed runs)
    bool prof_open = false;
    std::vector<tpz::rt::ProfRec> recs;
    std::vector<hipEvent_t> free_events;
    std::vector<std::pair<const void*, tpz::rt::ProfAcc>> per_kernel;   // conv_mfma instantiations
    double acc_ms[4] = {0, 0, 0, 0};
    long long acc_n[4] = {0, 0, 0, 0};
    double acc_flops[4] = {0, 0, 0, 0};
};

namespace tpz::rt {

static const int PART_BLOCKS = 1024;
static const int NRM_RING = 4096;

int fail(tpz_ctx* ctx, const char* fmt, ...);

#define HIPCHK(ctx, expr)                                                                        \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return ::tpz::rt::fail(ctx, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// ---- rt_core.hip
// A temporary device buffer from the workspace pool that is current when it is taken (*ctx->pool_cur), held for the handle's
// scope (ownership rule: the header comment above).  Move-only; an out-of-memory handle tests false.
// Under tpz_ctx_set_poison the constructor fills the whole pool buffer (its rounded size) with 0xFF bytes ahead of every consumer:
// on the stream that is current (a patch lane's included) or, in a batched pass, as a recorded op of the current image's list.
class WorkBuf {
public:
    WorkBuf() = default;
    WorkBuf(tpz_ctx* ctx, size_t bytes);
    WorkBuf(WorkBuf&& o) noexcept : pool_(o.pool_), p_(o.p_) { o.p_ = nullptr; }
    WorkBuf& operator=(WorkBuf&& o) noexcept {
        if (this != &o) { release(); pool_ = o.pool_; p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~WorkBuf() { release(); }
    void release();                                  // marks the buffer unused in the pool it came from; idempotent
    explicit operator bool() const { return p_ != nullptr; }
    template <class T>
    T* as() const { return static_cast<T*>(p_); }

private:
    std::vector<tpz_ctx::Buf>* pool_ = nullptr;      // (a member of the ctx: its address is stable)
    void* p_ = nullptr;
};
hipError_t flag_clear(tpz_ctx* ctx);       // the f16-range overflow flag of a 2xf16 pass (d_flag): zero it on the ctx stream ...
// ... copy it back, wait for the stream and return it in *flag.  The error is the copy's, else the wait's; check_copy = false: the
// wait's alone (tpz_conv_split_2d, which checks none of its launches)
hipError_t flag_read(tpz_ctx* ctx, unsigned* flag, bool check_copy = true);
float* next_nrm(tpz_ctx* ctx);
int lanes_begin(tpz_ctx* ctx);
void lane_enter(tpz_ctx* ctx, int k);
int lanes_end(tpz_ctx* ctx);
void prof_begin(tpz_ctx* ctx, int cls, double flops, const void* key = nullptr, double bytes = 0);
void prof_end(tpz_ctx* ctx);
void prof_flush(tpz_ctx* ctx);
int rec_begin(tpz_ctx* ctx, int batch_no = 0);
void rec_select(tpz_ctx* ctx, int i);
void rec_abort(tpz_ctx* ctx);
int rec_flush(tpz_ctx* ctx);
const std::string& last_global_error();
void restore_errors(tpz_ctx* ctx, const std::string& ctx_err, const std::string& global_err);

// ---- launches: issued at once on the ctx stream or, in a batched pass, recorded for rec_flush
// fn(stream) launches the kernel(s); cls / flops / key / bytes label it for the profiler
template <class F>
static hipError_t enqueue(tpz_ctx* ctx, int cls, double flops, const void* key, double bytes, F&& fn) {
    if (ctx->rec_on) {
        RecOp op;
        op.fn = std::forward<F>(fn);
        op.cls = cls; op.flops = flops; op.key = key; op.bytes = bytes;
        ctx->rec[ctx->rec_cur].push_back(std::move(op));
        return hipSuccess;
    }
    prof_begin(ctx, cls, flops, key, bytes);
    const hipError_t e = fn(ctx->stream);
    prof_end(ctx);
    ++ctx->n_launches;
    return e;
}
template <class F>
static hipError_t enqueue(tpz_ctx* ctx, F&& fn) { return enqueue(ctx, 2, 0.0, nullptr, 0.0, std::forward<F>(fn)); }

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------
struct LayerRT {
    tpz_layer L;
    const ConvKernelInfo* ki = nullptr;   // nullptr -> direct kernel
    int n_cog = 1, n_chunks = 1, cog_inner = 1;
    int c1 = 0, c2 = 0;                   // channels of the first / second source
    float* d_wpk = nullptr;               // packed (MFMA) or raw (direct) weights
    float* d_bias = nullptr;
    float* d_post_scale = nullptr;
    float* d_post_shift = nullptr;
    float* d_head_w = nullptr;
    float head_b = 0.f;
    float bias0 = 0.f;                    // bias of output channel 0 (host copy, for the 1-output-channel convs)
    // 2xf16 path (prepare_split): kernel, packed hi/lo weights, per-channel 2^-s; or the stem that feeds it
    const SplitKernelInfo* ks = nullptr;
    const ConvKernelInfo* ki_stem_split = nullptr;
    void* d_wsplit = nullptr;
    float* d_wscale = nullptr;
    int s_n_cog = 1, s_n_chunks = 1;
    // column-kernel forms (prepare_split): a 1-channel stem as an 8*ncell-channel conv over an x-shifted copy of the
    // image (kx taps as input channels), a 1-output-channel conv as k virtual output channels + a shifted sum
    const SplitKernelInfo* ks_stem = nullptr;
    const SplitKernelInfo* ks_last = nullptr;
    float* d_wlast = nullptr;                  // ... or (k = 3 / 5, few input channels) the vector-ALU stencil conv_cout1_split_kernel:
                                               // its weights [kz][cell][kx][ky][8] fp32
    // 3x3 32 -> 32 layers (dilation 1 / 2 / 4) of the 32-unit detectors: the weights-resident persistent kernel (conv_rw.h),
    // its weights packed with all 4 cells of a tap per step
    void* d_w_rw = nullptr;
    float* d_ws_rw = nullptr;
    const SplitKernelInfo* ks_pool = nullptr;  // twin of ks / ks_stem with the following 2x2 max-pool fused (EPI_POOL)
    // ResidA blocks that change width, y = [bn1](conv1(t) + proj(h)) (resnet.py:185-202): on the 2xf16 path the 1x1 projection is
    // FOLDED into conv1's K loop (SplitArgs::fold_cells) -- the projection layer is then skipped (folded_into = index of conv1)
    // and conv1 runs ks_fold (one-step stages, plain epilogue) over its own source + slot fold_src, eval-BN folded into weights
    int folded_into = -1;
    int fold_src = -1, fold_cells = 0, f_n_cog = 1, f_n_chunks = 1;
    const SplitKernelInfo* ks_fold = nullptr;
    void* d_wfold = nullptr;
    float* d_wscale_fold = nullptr;
    float* d_bias_fold = nullptr;
    // 2xf16 twin of the phase decomposition: the skip-source part runs first (stem kernel storing split cells
    // when the skip is the 1-channel image, else a plain split kernel), then one split kernel per output parity
    // adds itself in place through the residual epilogue and applies the activation
    struct SplitPhase {
        bool valid = false;
        const SplitKernelInfo* ks_low = nullptr;       // k1-tap kernel, EPI_RES, lattice output
        const SplitKernelInfo* ks_skip = nullptr;      // k-tap kernel over a multi-channel skip source, EPI_PLAIN
        const ConvKernelInfo* ki_skip_stem = nullptr;  // 1-channel skip source: fp32 CIN1 kernel, EPI_SPLIT
        int n_cog_low = 1, n_chunks_low = 1, n_cog_skip = 1, n_chunks_skip = 1;
        const SplitKernelInfo* ks_sub = nullptr;       // 5x5: all parities as 4*cout virtual channels of one 3x3 conv
        int n_cog_sub = 1;
        bool sub_with_skip = false;            // ... the 1-channel skip source folded in as 4 space-to-depth channels
        bool low_with_skip = false;            // 3x3(x3): the same fold into the per-parity kernels (one more cell)
        bool srcmajor = false;                 // ... in 3-D with the virtual cells ordered source-major (conv_split.h MODE 11)
        const SplitKernelInfo* ks_low_plain = nullptr;
        void* d_w_low = nullptr;               // the packs of all parities, w_phase_bytes apart
        float* d_ws_low = nullptr;             // [parity][cout]
        size_t w_phase_bytes = 0;
        void* d_w_skip = nullptr;
        float* d_ws_skip = nullptr;
    } sphase;
    // phase decomposition (prepare_phases): the first source arrives 2x nearest-upsampled
    struct Phase {
        bool valid = false;
        int c1 = 0, c2 = 0, k1 = 0;
        const ConvKernelInfo* ki_low = nullptr;    // k1-tap kernel over the low-resolution source, EPI_PLAIN
        const ConvKernelInfo* ki_skip = nullptr;   // k-tap kernel over the skip source, EPI_RES (in place)
        int n_cog_low = 1, n_chunks_low = 1, n_cog_skip = 1, n_chunks_skip = 1;
        float* d_w_low[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        float* d_w_skip = nullptr;
    } phase;
};

}  // namespace tpz::rt

struct tpz_model {
    tpz_ctx* ctx = nullptr;
    tpz::rt::DebugEnv dbg;                // the debug switches read when this model was loaded
    std::vector<tpz::rt::LayerRT> layers;
    int n_slots = 0;
    std::vector<int> last_use;
    std::vector<void*> dev_allocs;
    // bias-like vectors (conv biases, folded biases, eval-BN shifts) of all layers in one arena + a scratch copy of the same
    // size that a range-scaled pass fills with 2^-s times the originals (tpz_model_forward)
    float* d_bias_arena = nullptr;
    float* d_bias_scaled = nullptr;
    size_t n_bias_arena = 0;
    int n_conv = 0, n_conv_split = 0;     // convolution layers; those with a 2xf16 kernel (prepare_split)
    std::string off_path;                 // ... the others, "#layer KxK dD cin->cout, ..."
    bool split_ok = false;                // at least one layer has a 2xf16 kernel: the program runs in split mode
    bool widened = false;                 // the program was loaded with its widths zero-padded to multiples of 16 (widen_program)
    long long n_split = 0, n_fallback = 0;
    bool exact = false;                   // never tried on the 2xf16 path (tpz_model_set_exact, a tripped tpz_model_calibrate)
};

namespace tpz::rt {

// a rectangle of a 2-D tensor (planes [z0, z1) of a 3-D one: a box); on = false: the whole tensor
struct Rect {
    int y0 = 0, x0 = 0, y1 = 0, x1 = 0;
    bool on = false;
    int z0 = 0, z1 = 1;
    void unite(const Rect& r) {
        if (!r.on) return;
        if (!on) { *this = r; return; }
        y0 = std::min(y0, r.y0); x0 = std::min(x0, r.x0); y1 = std::max(y1, r.y1); x1 = std::max(x1, r.x1);
        z0 = std::min(z0, r.z0); z1 = std::max(z1, r.z1);
    }
    long long area() const { return (long long)(y1 - y0) * (x1 - x0); }
};

struct Slot {
    Rect need;                // the part of the tensor that anything reads (need_regions); the producer computes just that
    float* p = nullptr;
    int C = 0, D = 1, H = 0, W = 0;
    long long cs = 0, ps = 0;
    int pitch = 0;
    bool set = false;
    bool split = false;       // p holds split f16 cells (split_fmt.h) instead of fp32 planes
    bool pooled = false;      // the producing conv already applied the max-pool that follows it (EPI_POOL)
};

static void set_dense(Slot& s, float* p, int C, int D, int H, int W) {
    s.p = p; s.C = C; s.D = D; s.H = H; s.W = W;
    s.pitch = W; s.ps = (long long)H * W; s.cs = s.ps * D;
    s.set = true;
}

// a bias-like vector as the current pass reads it (the scaled copy in a range-scaled pass)
static inline const float* bias_view(const tpz_ctx* ctx, const float* p) { return p ? p + ctx->bias_shift : nullptr; }

// ---- which kernels run conv layer i, and in which tensor format: decided by conv_plan() and nowhere else ----------------------
// The loader (rt_load.hip prepare_split) equips a layer with the 2xf16 forms it has kernels for; conv_plan() picks the one a run
// takes from the shapes and formats it meets.  run_program dispatches on the result, need_regions asks form_windowable() about
// it, and the coverage count of the loader asks split_forms() whether there is any.
enum ConvForm {
    FORM_FP32,             // fp32 MFMA kernel (rt.ki; its per-parity form where the shapes allow, run_conv) or the direct kernel
    FORM_FP32_STEM_SPLIT,  // the fp32 1-channel stem storing split cells (rt.ki_stem_split)
    FORM_SPLIT,            // 2xf16 kernel (rt.ks; rt.ks_pool with fuse_pool; the weights-resident kernel where run_conv_split may)
    FORM_SPLIT_FOLD,       // 2xf16 kernel with a 1x1 projection folded into its K loop (rt.ks_fold)
    FORM_STEM,             // 1-channel stem as a column kernel over an x-shifted copy of the image (rt.ks_stem)
    FORM_LAST,             // 1-output-channel last conv (rt.ks_last): the vector-ALU stencil (rt.d_wlast) or column kernel + shift-sum
    FORM_PARITY,           // decoder conv over an exactly 2x upsampled + a skip source, by output parity (rt.sphase)
    FORM_FOLDED_AWAY,      // a 1x1 projection absorbed into the conv that adds it (rt.folded_into): nothing runs
};
struct ConvPlan {
    ConvForm form = FORM_FP32;
    bool fuse_pool = false;      // the 2x2 max-pool that follows runs in this conv's epilogue: the slot receives the pooled tensor
    bool split_dst = false;      // the destination holds split cells
    bool split1 = false, split2 = false, split_res = false;      // the format source 1, source 2 and the residual are read in
};
struct Dhw { int D = 1, H = 0, W = 0; };

// output size of a layer (conv, MAXPOOL, AVGPOOL, MAXPOOL2) from its geometry source: the second source of a conv that has one, else
// the first.  (A MAXPOOL of the pooled ResNets has pad = 0; the pools of a pooled BasicConv stack have pad = 1: topaz_hip.h.)
static inline Dhw layer_out_dhw(const tpz_layer& L, const Dhw& g) {
    if (L.op == TPZ_OP_MAXPOOL2) return {L.dims == 3 ? g.D / 2 : 1, g.H / 2, g.W / 2};
    const int grow = 2 * L.pad - L.dil * (L.k - 1);
    return {L.dims == 3 ? g.D + grow : 1, g.H + grow, g.W + grow};
}
// a pool with padding (pool_pad.hip): a program that holds one is neither tiled by run_image nor windowed by need_regions
static inline bool is_padded_pool(const tpz_layer& L) { return L.op == TPZ_OP_AVGPOOL || (L.op == TPZ_OP_MAXPOOL && L.pad > 0); }

// ---- cross-TU functions (defined in the file named)
// rt_load.hip
static inline size_t chan_pad(size_t n) { return (n + 127) / 128 * 128 + 128; }     // per-channel vectors: whole 128-channel tiles + one
static inline int phase_pad(int k, int p) { return (k / 2 - p + 1) / 2; }
int upload(tpz_ctx* ctx, tpz_model* m, const float* h, size_t n, float** out);
int upload_chan(tpz_ctx* ctx, tpz_model* m, const float* h, size_t n, float** out);
int upload_halfs(tpz_ctx* ctx, tpz_model* m, const std::vector<uint16_t>& h, void** out);      // packed f16 weights
void pack_weights_split(const SplitKernelInfo& ki, const float* w, int cout, int cin, int n_cog, int n_chunks,
                        std::vector<uint16_t>& out, std::vector<float>& wscale_inv, const float* wp = nullptr, int cin_b = 0,
                        const float* mul = nullptr);
const SplitKernelInfo* pick_split(int k, int dil, int cout, int epi, int kx = 0);
int model_load(tpz_ctx* ctx, const tpz_layer* layers, int n_layers, const float* h_blob, size_t n_floats,
               const std::vector<int>& preset_chan, tpz_model** out);
// rt_exec.hip
unsigned split_forms(const tpz_model* m, int i);       // the 2xf16 forms layer i was loaded with: bit (1 << ConvForm) each
// g1 / g2: D, H, W of the sources (g2 = nullptr: one source); split1: source 1 holds split cells; fold_set: rt.fold_src is set
ConvPlan conv_plan(const tpz_model* m, int i, bool split, const Dhw& g1, const Dhw* g2, bool split1, bool fold_set);
int run_conv_split(tpz_ctx* ctx, const LayerRT& rt, const Slot& s1, const Slot* sres, Slot& dst, const Slot* s2 = nullptr,
                   bool pooled = false, const Slot* fold = nullptr);
int run_program(tpz_model* m, std::vector<Slot>& slots, float* d_out, const float* d_nrm, bool split = false,
                const Rect* keep = nullptr);
// rt_resample.hip: the ctx a resampler plan belongs to (rt_stage.hip stages tpz_resample_2d_host through that ctx's ring)
tpz_ctx* resample_ctx(tpz_resample* plan);
// rt_stats.hip: launch_delta_stats on the ctx stream, its result copied to the host (synchronises)
int delta_stats(tpz_ctx* ctx, const float* d_a, const float* d_b, size_t n, tpz_delta* out);
// ---- the scalar steps of the 2-component mixture fit (topaz/stats.py:87-203), shared by tpz_gmm_fit (rt_stats.hip: one
// initialisation after the other) and tpz_gmm_fit_fused (rt_preprocess.hip: all of them per pass).  S / T are the seven sums of
// gmm_pass_kernel, N the number of pixels.
static inline double beta_logpdf(double x, double a, double b) {
    // scipy.stats.beta.logpdf: xlog1py(b-1, -x) + xlogy(a-1, x) - betaln(a, b)   (0 * log(0) = 0)
    const double t1 = (b - 1.0) == 0.0 ? 0.0 : (b - 1.0) * std::log1p(-x);
    const double t2 = (a - 1.0) == 0.0 ? 0.0 : (a - 1.0) * std::log(x);
    return t1 + t2 - (std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b));
}
struct GmmMoments { double mu_all, var_unbiased; };
// from the hard pass with split = +inf, which puts everything in component 0
static inline GmmMoments gmm_moments(const double* S, double N) {
    const double mu_all = S[3] / N;
    return {mu_all, (S[5] - 2.0 * mu_all * S[3] + mu_all * mu_all * N) / (N - 1.0)};   // torch .var()
}
// single-component model (stats.py:100-103): note the reference adds beta.PDF(1), not its logarithm
static inline void gmm_single_component(const GmmMoments& M, double N, double alpha, double beta, double scale, double& logp,
                                        double& mu, double& sd, double& pi) {
    const double pdf1 = beta == 1.0 ? std::exp(-(std::lgamma(alpha) + std::lgamma(beta) - std::lgamma(alpha + beta)))
                                    : (beta > 1.0 ? 0.0 : INFINITY);
    logp = scale * (-(N - 1.0) / 2.0 - N * 0.5 * std::log(2.0 * M_PI * M.var_unbiased)) + pdf1;
    mu = M.mu_all;
    sd = std::sqrt(M.var_unbiased);
    pi = 1.0;
}
static inline void gmm_m_step(const double* T, double N, double mu_all, double& mu0, double& mu1, double& var) {
    mu0 = T[1] > 0 ? T[3] / T[1] : mu_all;
    mu1 = T[2] > 0 ? T[4] / T[2] : mu_all;
    var = ((T[5] - 2.0 * mu0 * T[3] + mu0 * mu0 * T[1]) + (T[6] - 2.0 * mu1 * T[4] + mu1 * mu1 * T[2])) / N;
}
// MAP estimate of pi under the Beta prior from the assignments of the last E-step
static inline double gmm_map_pi(const double* S, double N, double alpha, double beta) {
    const double a_ = alpha + S[2], b_ = beta + N - S[2];
    return (a_ - 1.0) / (a_ + b_ - 2.0);
}
// the parameter block of an E-step pass (gmm_pass_kernel mode 1)
static inline void gmm_e_step_par(double mu0, double mu1, double var, double pi, double (&par)[6]) {
    par[0] = mu0; par[1] = mu1; par[2] = var; par[3] = var; par[4] = std::log1p(-pi); par[5] = std::log(pi);
}

// diag.hip: n_wg 4-wave workgroups each issue 8 * iters v_mfma_f32_16x16x32_f16 per wave on operands read from src (4096 x 16 B);
// ticks[0] = s_memtime, ticks[1] = s_memrealtime (100 MHz) ticks of wave 0's loop
hipError_t launch_mfma_spin(const void* src, float* out, int n_wg, int iters, unsigned long long* ticks, hipStream_t s);

}  // namespace tpz::rt
