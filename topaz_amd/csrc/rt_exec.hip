// The layer-program executor: launchers, per-layer drivers, windows (need_regions), run_program.
#include "rt_internal.h"

// ------------------------------------------------------------------------------------------------
// executor
// ------------------------------------------------------------------------------------------------
namespace tpz::rt {
namespace {

Dhw dhw(const Slot& s) { return {s.D, s.H, s.W}; }

// ---- the launch window: one rule for what a launch computes of its lattice, what that costs and the tiles that cover it
// planes [z0, z1), rows [y0, y1) and columns [x0, x1) of the lattice a launch computes (2-D: the one plane [0, 1))
struct Window { int z0, z1, y0, y1, x0, x1; };

// The window of a launch over the lattice `lat` from the part `need` of the layer's tensor that anything reads (need_regions; off:
// the whole lattice).  `scale` = 2: `lat` is the half-resolution lattice of a per-parity / sub-pixel launch; `align_x`: the left
// edge is rounded down to a multiple of it.  At least one plane, row and column: need_regions only hands out non-empty boxes
// inside the tensor (the kept pixels are one, and every step of its backward walk clips a grown, non-empty box to the tensor it
// lies in), so the guard changes no window it asks for.
Window launch_window(const Rect& need, const Dhw& lat, int scale = 1, int align_x = 1) {
    Window w = {0, std::max(lat.D, 1), 0, lat.H, 0, lat.W};
    if (!need.on) return w;
    w.y0 = need.y0 / scale; w.x0 = (need.x0 / scale) & ~(align_x - 1);
    w.y1 = std::max(w.y0 + 1, std::min(lat.H, (need.y1 + scale - 1) / scale));
    w.x1 = std::max(w.x0 + 1, std::min(lat.W, (need.x1 + scale - 1) / scale));
    if (lat.D > 1) {          // 3-D: the planes of the box
        w.z0 = std::min(lat.D - 1, need.z0 / scale);
        w.z1 = std::max(w.z0 + 1, std::min(lat.D, (need.z1 + scale - 1) / scale));
    }
    return w;
}
// (the two descriptors encode z differently: the fp32 kernels take the planes [wz0, wz1) of a.Dout, the plane-stacked 2xf16 kernels
// the first plane and, as a.Dout, the number of planes of a.Dlat)
void apply_window(ConvArgs& a, const Window& w) {
    a.wz0 = w.z0; a.wz1 = w.z1; a.wy0 = w.y0; a.wy1 = w.y1; a.wx0 = w.x0; a.wx1 = w.x1;
}
void apply_window(SplitArgs& a, const Window& w) {
    a.wy0 = w.y0; a.wy1 = w.y1; a.wx0 = w.x0; a.wx1 = w.x1;
    if (a.Dout > 1) { a.wz0 = w.z0; a.Dout = w.z1 - w.z0; }
}
// the share of the lattice that lies in the window: the FLOP a windowed launch executes of its layer's
double window_share(const Window& w, const Dhw& lat) {
    return (double)(w.y1 - w.y0) * (w.x1 - w.x0) / ((double)lat.H * lat.W) * ((double)(w.z1 - w.z0) / std::max(lat.D, 1));
}
// algorithmic FLOP of a conv layer over the output lattice `o`
double conv_flops(int cout, int cin, int k, int dims, const Dhw& o) {
    return 2.0 * cout * cin * std::pow((double)k, dims) * (double)o.D * o.H * o.W;
}
// tiles of `t` outputs that cover `n`, in whole groups of `d` (the tiles of a kernel of dilation d interleave: d of them share rows)
int tile_count(int n, int t, int d = 1) { return (n + t * d - 1) / (t * d) * d; }

// window, grid, XCD swizzle and phase stagger of one conv_mfma launch; a.Dout/Hout/Wout (the lattice), n_chunks, cog_inner are set
int launch_mfma(tpz_ctx* ctx, const ConvKernelInfo& ki, ConvArgs& a, int n_cog, double flops, const Window& w) {
    a.xcd_swizzle = 1;
    apply_window(a, w);
    flops *= window_share(w, {a.Dout, a.Hout, a.Wout});
    a.tiles_x = tile_count(w.x1 - w.x0, ki.TW);
    a.tiles_y = tile_count(w.y1 - w.y0, ki.TH, ki.D);
    a.tiles_z = ki.dims == 3 ? tile_count(w.z1 - w.z0, ki.TD, ki.D) : 1;
    a.stagger_first = a.stagger_sleeps = 0;
    // phase stagger of the two workgroups per CU (conv_mfma.h); only worth it for many generations
    if ((long long)a.tiles_x * a.tiles_y >= 4096) {
        a.stagger_first = 512;
        a.stagger_sleeps = (int)((long long)a.n_chunks * ki.SPG * ki.STEPS * (ki.MT / 16) *
                                 ((ki.TD * ki.TH / 4) * (ki.TW / 16)) * 32 / 8128 / 2);
    }
    if ((long long)a.tiles_y * a.tiles_z > 65535) return fail(ctx, "conv grid too large");
    // 32-bit LDS-DMA byte offsets relative to the first channel of a chunk
    if ((size_t)ki.NCH * (size_t)std::max(a.cs1, a.cs2) * 4 >= ((size_t)1 << 32))
        return fail(ctx, "image too large for one launch: process it in patches");
    dim3 grid(a.tiles_x, a.tiles_y * a.tiles_z, n_cog / a.cog_inner);
    const ConvKernelInfo* kip = &ki;
    const ConvArgs ac = a;
    hipError_t e = enqueue(ctx, 0, flops, ki.name, 0.0, [kip, ac, grid](hipStream_t st) { return kip->launch(ac, grid, st); });
    HIPCHK(ctx, e);
    return 0;
}

// The windows of the fp32 kernels start on a multiple of 4 pixels: the 16-byte granules of the MFMA kernels' loader stay aligned;
// the few extra columns are computed like any others.
enum { FP32_ALIGN_X = 4 };

// conv(cat(upsample2x(s1), s2)) by output parity (prepare_phases): 2^dims plain launches over s1 that write the
// strided output positions, then the skip-source launch over the full grid (its window: `full`) that adds itself in place.
int run_conv_phases(tpz_ctx* ctx, const LayerRT& rt, const ConvArgs& base, const Slot& s1, const Slot& s2, Slot& dst,
                    const Window& full) {
    const tpz_layer& L = rt.L;
    const LayerRT::Phase& ph = rt.phase;
    const int n_phase = 1 << L.dims;
    for (int p = 0; p < n_phase; ++p) {
        const int px = p & 1, py = (p >> 1) & 1, pz = L.dims == 3 ? (p >> 2) & 1 : 0;
        ConvArgs a = base;
        a.in2 = nullptr;
        a.wpk = ph.d_w_low[p];
        a.bias = nullptr;
        a.res = nullptr;
        a.nrm = nullptr;
        a.norm_out = 0;
        a.slope = 1.f;
        a.Cin = a.Cin1 = ph.c1;
        a.Din = a.D1 = s1.D; a.Hin = a.H1 = s1.H; a.Win = a.W1 = s1.W;
        a.Dout = s1.D; a.Hout = s1.H; a.Wout = s1.W;                  // the lattice of this parity
        a.pad_x = phase_pad(L.k, px); a.pad_y = phase_pad(L.k, py); a.pad_z = L.dims == 3 ? phase_pad(L.k, pz) : 0;
        a.pad = a.pad_x;
        a.os = 2; a.oox = px; a.ooy = py; a.ooz = pz;
        a.n_chunks = ph.n_chunks_low;
        a.cog_inner = 1;
        if (launch_mfma(ctx, *ph.ki_low, a, ph.n_cog_low, conv_flops(L.cout, ph.c1, ph.k1, L.dims, dhw(s1)),
                        launch_window(dst.need, dhw(s1), 2, FP32_ALIGN_X)))
            return 1;
    }
    ConvArgs a = base;
    a.in = s2.p;
    a.in2 = nullptr;
    a.wpk = ph.d_w_skip;
    a.res = dst.p;                                                     // in place: every thread reads what it writes
    a.Dres = dst.D; a.Hres = dst.H; a.Wres = dst.W; a.res_crop = 0;
    a.Cin = a.Cin1 = ph.c2;
    a.D1 = s2.D; a.H1 = s2.H; a.W1 = s2.W;
    a.cs1 = s2.cs; a.ps1 = s2.ps; a.pitch1 = s2.pitch;
    a.n_chunks = ph.n_chunks_skip;
    a.cog_inner = 1;
    return launch_mfma(ctx, *ph.ki_skip, a, ph.n_cog_skip, conv_flops(L.cout, ph.c2, L.k, L.dims, dhw(dst)), full);
}

int launch_split(tpz_ctx* ctx, const SplitKernelInfo& ks, SplitArgs& a, int n_cog, double flops, const Window& w);

// What every 2xf16 launch shares.  `in`: cells1 cells of g_in; the launch computes the lattice `lat` (kz taps along z, kz = 0: a 2-D
// launch; `pad` on every axis), element o of which is element o * os (+ the parity) of the full output tensor `full`.  The window is
// the whole lattice, Dlat its depth, until the launcher applies the launch's own.  The caller adds its operands, a second source and
// whatever else is particular to it.
SplitArgs split_args(tpz_ctx* ctx, const void* in, int cells1, const Dhw& g_in, int cout, const Dhw& lat, int os, const Dhw& full,
                     int kz, int pad, float slope) {
    SplitArgs a;
    memset(&a, 0, sizeof a);
    a.in = reinterpret_cast<const uint4*>(in);
    a.zeros = ctx->d_zeros;
    a.flag = ctx->d_flag;
    a.slope = slope;
    a.cells_in = a.cells_in1 = cells1;
    a.Hin = a.H1 = g_in.H; a.Win = a.W1 = g_in.W;
    a.Cout = cout; a.cells_out = (int)split_cells(cout);
    a.Hout = a.wy1 = lat.H; a.Wout = a.wx1 = lat.W;
    a.pad_x = a.pad_y = pad;
    a.os = os; a.Hfull = full.H; a.Wfull = full.W;
    a.cog_inner = 1;
    if (kz > 0) { a.KZ = kz; a.pad_z = pad; a.Din = g_in.D; a.Dout = a.Dlat = lat.D; a.Dfull = full.D; a.Dres = 1; }
    return a;
}
// the lattice of a 2xf16 launch as split_args left it
Dhw lattice(const SplitArgs& a) { return {a.Dout, a.Hout, a.Wout}; }

// the weights-resident kernel (conv_rw.h) for a 3x3 32 -> 32 layer: window and tile grid as launch_split, one persistent
// workgroup per CU
int launch_rw(tpz_ctx* ctx, SplitArgs& a, int dil, int epi, double flops, const Window& w) {
    static char names[3][3][96];
    const int di = dil == 1 ? 0 : dil == 2 ? 1 : 2;
    if (!names[di][epi][0])
        snprintf(names[di][epi], sizeof names[di][epi], "conv_split_rw_kernel<K=3x3,D=%d,MT=32,EPI=%d> (weights resident)", dil, epi);
    flops *= window_share(w, lattice(a));
    apply_window(a, w);
    a.tiles_x = tile_count(w.x1 - w.x0, 32);
    a.tiles_y = tile_count(w.y1 - w.y0, 8, dil);
    const long long nt = (long long)a.tiles_x * a.tiles_y;
    if (nt >= (1LL << 30)) return fail(ctx, "conv grid too large");
    a.n_tiles = (int)nt;
    if ((size_t)a.cells_in * a.Hin * a.Win * 16 >= ((size_t)1 << 32) - 16)
        return fail(ctx, "image too large for one launch (%d x %d): process it in patches", a.Hin, a.Win);
    // (the residual plane is addressed with 32-bit offsets too, and with res_crop > 0 it is larger than the input plane)
    if (a.res && (size_t)a.cells_out * a.Hres * a.Wres * 16 >= ((size_t)1 << 32) - 16)
        return fail(ctx, "residual tensor too large for one launch (%d x %d): process the image in patches", a.Hres, a.Wres);
    const int wgs = std::max(8, ctx->n_cus / 8 * 8);
    const double wy = a.wy1 - a.wy0, wx = a.wx1 - a.wx0, span = 2.0 * dil;
    double bytes = (double)a.cells_in * 32.0 * std::min((double)a.Hin, wy + span) * std::min((double)a.Win, wx + span) +
                   32.0 * a.cells_out * wy * wx * (a.res ? 2.0 : 1.0) + 36864.0;
    const SplitArgs ac = a;
    hipError_t e = enqueue(ctx, 0, flops, names[di][epi], bytes, [=](hipStream_t st) { return launch_conv_rw(ac, dil, epi, wgs, st); });
    if (e != hipSuccess) return fail(ctx, "conv_rw launch failed: %s", hipGetErrorString(e));
    ++ctx->n_walk[WALK_RW];          // (run_conv_split sends no layer here in a batched pass: the launch was issued)
    return 0;
}

}  // namespace

unsigned split_forms(const tpz_model* m, int i) {
    const LayerRT& rt = m->layers[i];
    if (rt.folded_into >= 0 && m->layers[rt.folded_into].ks_fold) return 1u << FORM_FOLDED_AWAY;
    return (rt.ks_stem ? 1u << FORM_STEM : 0) | (rt.ks_last ? 1u << FORM_LAST : 0) | (rt.sphase.valid ? 1u << FORM_PARITY : 0) |
           (rt.ks && rt.ks_fold ? 1u << FORM_SPLIT_FOLD : 0) | (rt.ks ? 1u << FORM_SPLIT : 0) |
           (rt.ki_stem_split ? 1u << FORM_FP32_STEM_SPLIT : 0);
}

// Which kernels run conv layer i of a pass (split: a 2xf16 pass), and in which format it reads and writes its tensors.  Of the forms
// the layer was loaded with, the first that this run's shapes and formats allow, in the order below.  (prepare_split gives a layer
// at most one of STEM / LAST / SPLIT-or-PARITY / FP32_STEM_SPLIT: they need a 1-channel source, no MFMA kernel, a multi-channel MFMA
// kernel and a 1-channel source without ks_stem; ks_fold needs a residual and ks_pool none, so a folded layer never fuses a pool.)
ConvPlan conv_plan(const tpz_model* m, int i, bool split, const Dhw& g1, const Dhw* g2, bool split1, bool fold_set) {
    const LayerRT& rt = m->layers[i];
    const tpz_layer& L = rt.L;
    const unsigned f = split ? split_forms(m, i) : 0;
    auto has = [&](ConvForm c) { return (f >> c & 1u) != 0; };
    // the per-parity form needs the skip source to be exactly twice the upsampled one
    const bool exact2x = g2 && g2->H == 2 * g1.H && g2->W == 2 * g1.W && (L.dims == 2 || g2->D == 2 * g1.D);
    ConvPlan p;
    if (has(FORM_FOLDED_AWAY)) p.form = FORM_FOLDED_AWAY;
    else if (has(FORM_STEM) && !split1) p.form = FORM_STEM;
    else if (has(FORM_LAST)) p.form = FORM_LAST;
    else if (has(FORM_PARITY) && exact2x) p.form = FORM_PARITY;
    else if (has(FORM_SPLIT_FOLD) && rt.fold_src >= 0 && fold_set) p.form = FORM_SPLIT_FOLD;
    else if (has(FORM_SPLIT)) p.form = FORM_SPLIT;
    else if (has(FORM_FP32_STEM_SPLIT)) p.form = FORM_FP32_STEM_SPLIT;
    const bool on_ks = p.form == FORM_SPLIT || p.form == FORM_SPLIT_FOLD;
    p.fuse_pool = rt.ks_pool && (p.form == FORM_STEM || (p.form == FORM_SPLIT && !g2)) && i + 1 < (int)m->layers.size();
    p.split_dst = p.form == FORM_PARITY || p.form == FORM_FP32_STEM_SPLIT || p.form == FORM_STEM ||
                  (on_ks && !L.head && rt.ks->epi != EPI_PLAIN_F32);
    p.split1 = p.form == FORM_PARITY || on_ks || p.form == FORM_LAST;
    p.split2 = p.form == FORM_PARITY ? !rt.sphase.ki_skip_stem : on_ks;       // (a 1-channel skip source is read as fp32)
    p.split_res = on_ks;
    return p;
}

// one conv layer on the 2xf16 path: split source (and residual), split output or fused fp32 head
// (fold: the input of a folded 1x1 projection, split cells -- the layer then runs ks_fold with the projection's channels
// appended to its K loop, no residual, eval-BN already inside weights and bias)
int run_conv_split(tpz_ctx* ctx, const LayerRT& rt, const Slot& s1, const Slot* sres, Slot& dst, const Slot* s2, bool pooled,
                   const Slot* fold) {
    const tpz_layer& L = rt.L;
    const SplitKernelInfo& ks = fold ? *rt.ks_fold : pooled ? *rt.ks_pool : *rt.ks;
    // (a pooled dst is the pooled tensor; the launch covers the un-pooled conv output)
    const Dhw lat = pooled ? layer_out_dhw(L, dhw(s2 ? *s2 : s1)) : dhw(dst);
    SplitArgs a = split_args(ctx, s1.p, (int)split_cells(s1.C), dhw(s1), L.cout, {dst.D, lat.H, lat.W}, 1, dhw(dst),
                             L.dims == 3 ? L.k : 0, L.pad, L.slope);
    a.wpk = reinterpret_cast<const uint4*>(fold ? rt.d_wfold : rt.d_wsplit);
    a.wscale = fold ? rt.d_wscale_fold : rt.d_wscale;
    a.bias = bias_view(ctx, fold ? rt.d_bias_fold : rt.d_bias);
    a.res = sres ? reinterpret_cast<const uint4*>(sres->p) : nullptr;
    a.post_scale = fold ? nullptr : rt.d_post_scale;
    a.post_shift = fold ? nullptr : bias_view(ctx, rt.d_post_shift);
    a.head_w = rt.d_head_w;
    a.head_b = ctx->scaled_pass ? 0.f : rt.head_b;
    if (L.head) a.head_out = dst.p;
    else if (ks.epi == EPI_PLAIN_F32) a.out_f32 = dst.p;
    else a.out = reinterpret_cast<uint4*>(dst.p);
    if (s2) {              // fused upsample + concat: s1 nearest-upsampled to the grid of s2
        a.in2 = reinterpret_cast<const uint4*>(s2->p);
        a.cells_in = a.cells_in1 + (int)split_cells(s2->C);
        a.Hin = s2->H; a.Win = s2->W;
    }
    if (sres) { a.Hres = sres->H; a.Wres = sres->W; a.res_crop = L.res_crop; }
    if (sres && L.dims == 3) a.Dres = sres->D;
    a.n_chunks = rt.s_n_chunks;
    a.cog_inner = L.head ? rt.s_n_cog : 1;
    double flops = conv_flops(L.cout, L.cin, L.k, L.dims, {dst.D, lat.H, lat.W});
    const Window w = launch_window(dst.need, lattice(a));      // (a pooled dst keeps its need in the coordinates of the un-pooled conv output)
    if (fold) {
        // out(y, x) += proj(h)(y + res_crop, x + res_crop); the centre tap of output y sits at tile-input row y - pad + (k/2) dil
        a.in2 = reinterpret_cast<const uint4*>(fold->p);
        a.fold_cells = rt.fold_cells;
        a.cells_in = a.cells_in1 + rt.fold_cells;
        a.fold_tap = (L.k * L.k) / 2;
        a.in2_H = fold->H; a.in2_W = fold->W;
        a.in2_oy = a.in2_ox = L.res_crop + L.pad - (L.k / 2) * L.dil;
        a.n_chunks = rt.f_n_chunks;
        flops += 2.0 * L.cout * (8.0 * rt.fold_cells) * (double)a.Hout * a.Wout;
        return launch_split(ctx, ks, a, rt.f_n_cog, flops, w);
    }
    if (rt.d_w_rw && !pooled && !s2 && !ctx->rec_on && ks.epi <= EPI_RES_POST && L.dims == 2 && ctx->rw_enabled) {
        a.wpk = reinterpret_cast<const uint4*>(rt.d_w_rw);
        a.wscale = rt.d_ws_rw;
        return launch_rw(ctx, a, L.dil, ks.epi, flops, w);
    }
    return launch_split(ctx, ks, a, rt.s_n_cog, flops, w);
}

namespace {

// the K-loop schedule of this launch (SplitArgs::plan): tile-invariant, so one table per (kernel, cells, sources) serves every
// launch of the layer; the first launch builds and uploads it (a blocking copy, once)
const SplitStep* split_plan(tpz_ctx* ctx, const SplitKernelInfo& ks, const SplitArgs& a, bool* next_ok) {
    SplitPlanKey k;
    memset(&k, 0, sizeof k);
    k.cells_in = a.cells_in; k.cells_in1 = a.cells_in1; k.n_chunks = a.n_chunks; k.has_in2 = a.in2 != nullptr;
    k.vol = (a.KZ > 1 || a.Din > 1) ? 1 : 0; k.KZ = a.KZ; k.fold_cells = a.fold_cells; k.fold_tap = a.fold_tap;
    k.srcmajor = (k.vol && a.in2) ? a.vol_srcmajor : 0;
    for (auto& e : ctx->split_plans)
        if (e.ks == &ks && memcmp(&e.key, &k, sizeof k) == 0) { *next_ok = e.next_ok; return e.d; }
    std::vector<SplitStep> h;
    ks.make_plan(k, h);
    *next_ok = (h[0].dma & SPLIT_DMA_NEXT) != 0;
    SplitStep* d = nullptr;
    if (hipMalloc(&d, h.size() * sizeof(SplitStep)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), h.size() * sizeof(SplitStep), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    ctx->split_plans.push_back({&ks, k, d, *next_ok});
    return d;
}

int launch_split(tpz_ctx* ctx, const SplitKernelInfo& ks, SplitArgs& a, int n_cog, double flops, const Window& w) {
    flops *= window_share(w, lattice(a));
    apply_window(a, w);
    a.tiles_x = tile_count(w.x1 - w.x0, ks.TW);
    a.tiles_y = tile_count(w.y1 - w.y0, ks.TH, ks.D);
    a.xcd_swizzle = 1;
    a.issuer_half = ks.WAVES == 8 && ks.MT >= 96 && !ctx->dbg.no_issuer;   // -3 .. -4 % on the 128-channel tiles, nothing at 64 (tools/split_ablate.hip)
    if (a.KZ < 1) { a.KZ = 1; a.pad_z = 0; a.Din = a.Dout = a.Dfull = a.Dres = 1; a.ooz = 0; }     // 2-D launch
    if (a.Dres < 1) a.Dres = 1;
    a.ncz = n_cog / a.cog_inner;
    const long long gz = (long long)a.ncz * a.Dout * std::max(a.nphase, 1);
    if (a.tiles_y > 65535 || gz > 65535) return fail(ctx, "conv grid too large");
    // the LDS-DMA addresses are 32-bit byte offsets from a wave-uniform base: a chunk of cells (2-D) or one half of the
    // whole tensor (plane-stacked 3-D) must stay below 4 GiB
    if (a.Din > 1 && (size_t)a.cells_in * a.Din * a.Hin * a.Win * 16 >= ((size_t)1 << 32) - 16)
        return fail(ctx, "3-D tensor too large for the plane-stacked 2xf16 kernel (tile the volume)");
    if ((size_t)ks.CC * std::max((size_t)a.Hin * a.Win, (size_t)a.H1 * a.W1) * 16 >= ((size_t)1 << 32) - 16)
        return fail(ctx, "image too large for one launch (%d x %d): process it in patches", a.Hin, a.Win);
    // ... and so are the epilogue's buffer offsets: the two cell planes of a channel fragment, of the output and of the residual
    if (ks.epi != EPI_HEAD && ks.epi != EPI_PLAIN_F32 &&
        2 * std::max((size_t)a.Dfull * a.Hfull * a.Wfull, (size_t)a.Dres * a.Hres * a.Wres) * 16 >= ((size_t)1 << 32) - 16)
        return fail(ctx, "tensor too large for one launch (%d x %d x %d): process it in patches", a.Dfull, a.Hfull, a.Wfull);
    dim3 grid(a.tiles_x, a.tiles_y, (unsigned)gz);
    bool next_ok = false;
    a.plan = split_plan(ctx, ks, a, &next_ok);
    if (!a.plan) return fail(ctx, "out of device memory (K-loop plan)");
    // Persistent workgroups (conv_split.h MODE 4): a few per CU, each walking its share of the tiles and prefetching its next
    // tile's first chunk during the current tile's last -- for plain single-source layers with several tiles per workgroup.
    // Not under the patch lanes: a persistent grid holds every CU until it ends, and the lanes live on the small launches of one
    // patch slipping in beside the large ones of its neighbour.
    a.n_tiles = 0;
    {
        const long long nt = (long long)a.tiles_x * a.tiles_y * gz;
        const int slots = ctx->n_cus * (ks.WAVES == 8 ? 1 : 2);
        const bool plain = !a.in2 && a.KZ <= 1 && a.Din <= 1;
        const bool eligible = next_ok && plain && ks.epi != EPI_HEAD && a.cog_inner == 1 && nt < (1LL << 30);
        // (measured, profiles/r03_persistent_ab.txt: +5 .. +60 % on the tiles of up to 96 channels, whose prologue is 10 - 20 % of
        // a tile; +-0 on the 128-channel 8-wave tiles, where the longer scalar state costs the K loop what the prologue gave)
        const bool want = ctx->persist_mode == 2 || (ctx->persist_mode == 1 && !ctx->lanes_on && nt >= 2LL * slots && ks.MT <= 96);
        if (eligible && want && !ctx->rec_on) {
            const int wgs = ctx->persist_wgs > 0 ? ctx->persist_wgs : slots;
            a.n_tiles = (int)nt;
            grid = dim3((unsigned)std::max(8, wgs / 8 * 8), 1, 1);
        }
    }
    // algorithmic HBM bytes of the launch: the input window (with its halo) of every source once, the weights once, the output
    // window once (+ the residual it adds); 4 bytes per element in either format
    double bytes = 0;
    {
        const double wy = a.wy1 - a.wy0, wx = a.wx1 - a.wx0, span = (double)ks.D * (ks.K - 1), spanx = (double)ks.D * (ks.KX - 1);
        const double planes = (double)a.Dout * std::max(a.nphase, 1);
        bytes += (double)a.cells_in * 32.0 * std::min((double)a.Hin, wy + span) * std::min((double)a.Win, wx + spanx) * (a.Din > 1 ? a.Din : 1);
        const double outpx = wy * wx * planes * (a.os > 1 && a.nphase == 0 && a.subpix_cout > 0 ? 4.0 : 1.0);
        bytes += (a.out_f32 ? 4.0 * a.Cout : a.head_out ? 4.0 : 32.0 * a.cells_out) * outpx;
        if (a.res) bytes += 32.0 * a.cells_out * outpx;
        bytes += (double)n_cog * ks.stages(a.cells_in * std::max(a.KZ, 1)) * ks.W_STEP_BYTES * std::max(a.nphase, 1);
    }
    // patch raster (conv_split.h, xcd_swizzle 2) for the one-workgroup-per-CU tiles of a launch of its own: the grid is padded to
    // whole 8 x 4 blocks of tiles
    if (ctx->raster && !ctx->rec_on && a.n_tiles == 0 && ks.WAVES == 8 && (long long)a.tiles_x * a.tiles_y >= 512) {
        a.xcd_swizzle = 2;
        grid = dim3((unsigned)((a.tiles_x + 7) / 8 * 8), (unsigned)((a.tiles_y + 3) / 4 * 4), (unsigned)gz);
    }
    if (ctx->rec_on) {
        // a batched pass: recorded; rec_flush issues it together with the same layer's launch of the other images
        RecOp op;
        op.ks = &ks;
        op.a = a;
        op.a.n_tiles = (int)std::min<long long>((long long)a.tiles_x * a.tiles_y * gz, 0x7fffffff);
        op.grid = grid;
        op.cls = 0; op.flops = flops; op.bytes = bytes; op.key = ks.name;
        ctx->rec[ctx->rec_cur].push_back(std::move(op));
        return 0;
    }
    prof_begin(ctx, 0, flops, ks.name, bytes);
    hipError_t e = ks.launch(a, grid, ctx->stream);
    prof_end(ctx);
    ++ctx->n_launches;
    ++ctx->n_walk[a.n_tiles > 0 ? WALK_PERSIST : a.xcd_swizzle == 2 ? WALK_RASTER : WALK_PLAIN];
    HIPCHK(ctx, e);
    return 0;
}

// conv(cat(upsample2x(s1), s2)) on the 2xf16 path (prepare_split_phases).  s1: split; s2: fp32 when it is the
// 1-channel image (stem kernel), else split; dst: split.
int run_conv_split_phases(tpz_ctx* ctx, const LayerRT& rt, const Slot& s1, const Slot& s2, Slot& dst) {
    const tpz_layer& L = rt.L;
    const LayerRT::SplitPhase& sp = rt.sphase;
    const LayerRT::Phase& ph = rt.phase;
    if (sp.sub_with_skip) {
        // one plain sub-pixel launch: low-resolution source + the space-to-depth copy of the 1-channel skip source
        if (s2.pitch != s2.W || s2.ps != (long long)s2.H * s2.W) return fail(ctx, "2xf16 decoder needs a dense skip source");
        const WorkBuf Xb(ctx, (size_t)8 * s1.H * s1.W * sizeof(float));
        if (!Xb) return fail(ctx, "out of device memory");
        float* X = Xb.as<float>();
        hipError_t e;
        {
            const float* sp_ = s2.p; unsigned* fl_ = ctx->d_flag;
            const int h1 = s1.H, w1 = s1.W, h2 = s2.H, w2 = s2.W;
            e = enqueue(ctx, [=](hipStream_t st) { return launch_s2d_split(sp_, X, 1, h1, w1, h2, w2, 2, fl_, st); });
        }
        if (e != hipSuccess) return fail(ctx, "s2d failed: %s", hipGetErrorString(e));
        SplitArgs a = split_args(ctx, s1.p, (int)split_cells(s1.C), dhw(s1), L.cout, dhw(s1), 2, dhw(dst), 0, 1, L.slope);
        a.in2 = reinterpret_cast<const uint4*>(X);
        a.cells_in = a.cells_in1 + 1;
        a.wpk = reinterpret_cast<const uint4*>(sp.d_w_low);
        a.wscale = sp.d_ws_low;
        a.bias = bias_view(ctx, rt.d_bias);
        a.subpix_cout = L.cout;
        a.out = reinterpret_cast<uint4*>(dst.p);
        a.n_chunks = sp.n_chunks_low;
        const double fl = 2.0 * L.cout * (ph.c1 * 9.0 * 4.0 + 25.0 * 4.0) * (double)s1.H * s1.W;
        return launch_split(ctx, *sp.ks_sub, a, sp.n_cog_sub, fl, launch_window(dst.need, lattice(a), 2));
    }
    // ---- skip-source part over the full grid: bias, no activation
    WorkBuf Xb;
    float* Xs2d = nullptr;
    if (sp.low_with_skip) {
        if (s2.pitch != s2.W || s2.ps != (long long)s2.H * s2.W) return fail(ctx, "2xf16 decoder needs a dense skip source");
        Xb = WorkBuf(ctx, (size_t)8 * s1.D * s1.H * s1.W * sizeof(float));
        if (!Xb) return fail(ctx, "out of device memory");
        Xs2d = Xb.as<float>();
        hipError_t e;
        {
            const float* sp_ = s2.p; unsigned* fl_ = ctx->d_flag;
            const int d1 = s1.D, h1 = s1.H, w1 = s1.W, h2 = s2.H, w2 = s2.W, dims = L.dims;
            e = enqueue(ctx, [=](hipStream_t st) { return launch_s2d_split(sp_, Xs2d, d1, h1, w1, h2, w2, dims, fl_, st); });
        }
        if (e != hipSuccess) return fail(ctx, "s2d failed: %s", hipGetErrorString(e));
    } else if (sp.ki_skip_stem) {
        ConvArgs a;
        memset(&a, 0, sizeof a);
        a.in = s2.p;
        a.wpk = ph.d_w_skip;
        a.bias = bias_view(ctx, rt.d_bias);
        a.out = dst.p;
        a.zeros = ctx->d_zeros;
        a.flag = ctx->d_flag;
        a.Cin = a.Cin1 = 1;
        a.Din = a.D1 = s2.D; a.Hin = a.H1 = s2.H; a.Win = a.W1 = s2.W;
        a.cs1 = s2.cs; a.ps1 = s2.ps; a.pitch1 = s2.pitch;
        a.Cout = L.cout;
        a.Dout = dst.D; a.Hout = dst.H; a.Wout = dst.W;
        a.pad = a.pad_x = a.pad_y = a.pad_z = L.pad;
        a.os = 1;
        a.Dfull = dst.D; a.Hfull = dst.H; a.Wfull = dst.W;
        a.slope = 1.f;
        a.n_chunks = 1;
        a.cog_inner = 1;
        // (over the whole grid, whatever is needed of it)
        if (launch_mfma(ctx, *sp.ki_skip_stem, a, 1, conv_flops(L.cout, 1, L.k, L.dims, dhw(dst)), launch_window(Rect(), dhw(dst)))) return 1;
    } else {
        SplitArgs a = split_args(ctx, s2.p, (int)split_cells(s2.C), dhw(s2), L.cout, dhw(dst), 1, dhw(dst), L.dims == 3 ? L.k : 0,
                                 L.pad, 1.f);
        a.wpk = reinterpret_cast<const uint4*>(sp.d_w_skip);
        a.wscale = sp.d_ws_skip;
        a.bias = bias_view(ctx, rt.d_bias);
        a.out = reinterpret_cast<uint4*>(dst.p);
        a.n_chunks = sp.n_chunks_skip;
        // (the window is even-aligned by need_regions: the parity launch below adds itself in place)
        if (launch_split(ctx, *sp.ks_skip, a, sp.n_cog_skip, conv_flops(L.cout, ph.c2, L.k, L.dims, dhw(dst)),
                         launch_window(dst.need, lattice(a))))
            return 1;
    }
    // ---- every output parity over the low-resolution source in one launch, added in place, then the activation
    {
        // (the lattice of one parity; with nphase set the kernel takes pads and lattice offsets from the parity)
        SplitArgs a = split_args(ctx, s1.p, (int)split_cells(s1.C), dhw(s1), L.cout, dhw(s1), 2, dhw(dst), L.dims == 3 ? ph.k1 : 0,
                                 sp.ks_sub ? 1 : 0, L.slope);
        a.wpk = reinterpret_cast<const uint4*>(sp.d_w_low);
        a.wscale = sp.d_ws_low;
        if (sp.ks_sub) {
            a.subpix_cout = L.cout;
        } else {
            a.nphase = 1 << L.dims;
            a.phase_k = L.k;
            a.w_phase_bytes = sp.w_phase_bytes;
            a.ws_phase_stride = (int)chan_pad(L.cout);
        }
        a.out = reinterpret_cast<uint4*>(dst.p);
        a.res = reinterpret_cast<const uint4*>(dst.p);
        if (sp.low_with_skip) {                       // + the space-to-depth cell of the skip source; plain epilogue
            a.in2 = reinterpret_cast<const uint4*>(Xs2d);
            a.cells_in = a.cells_in1 + 1;
            a.res = nullptr;
            a.bias = bias_view(ctx, rt.d_bias);
            a.vol_srcmajor = sp.srcmajor ? 1 : 0;
        }
        a.Hres = dst.H; a.Wres = dst.W;
        if (L.dims == 3) a.Dres = dst.D;
        a.n_chunks = sp.n_chunks_low;
        const double fl = conv_flops(L.cout, ph.c1, ph.k1, L.dims, dhw(s1)) * (1 << L.dims);
        const SplitKernelInfo& kk = sp.ks_sub ? *sp.ks_sub : (sp.low_with_skip ? *sp.ks_low_plain : *sp.ks_low);
        if (launch_split(ctx, kk, a, sp.ks_sub ? sp.n_cog_sub : sp.n_cog_low, fl, launch_window(dst.need, lattice(a), 2))) return 1;
    }
    return 0;
}

// 1-channel stem on the 2xf16 path: x-shifted copy of the image (kx taps as channels), then a k x 1 column kernel
int run_stem_split(tpz_ctx* ctx, const LayerRT& rt, const Slot& s1, Slot& dst, bool pooled = false) {
    const tpz_layer& L = rt.L;
    const SplitKernelInfo& ks = pooled ? *rt.ks_pool : *rt.ks_stem;
    if (s1.pitch != s1.W || s1.ps != (long long)s1.H * s1.W) return fail(ctx, "2xf16 stem needs a dense input");
    const int ncell = (L.k + 7) / 8;
    const size_t rows = (size_t)s1.D * s1.H;
    // conv output geometry (dst is the pooled tensor when the max-pool is fused)
    const int Hc = layer_out_dhw(L, dhw(s1)).H, Wc = layer_out_dhw(L, dhw(s1)).W;      // (dilation 1: prepare_split)
    const WorkBuf Xb(ctx, (size_t)ncell * 8 * rows * Wc * sizeof(float));
    if (!Xb) return fail(ctx, "out of device memory");
    float* X = Xb.as<float>();
    // the window of the conv (dst.need: in the coordinates of the conv output, also when the max-pool is fused)
    const Window w = launch_window(dst.need, {dst.D, Hc, Wc});
    // (2-D with a window: only the rows and columns the windowed conv reads -- output row y reads input rows y - pad .. y + pad)
    hipError_t e;
    {
        const float* sp_ = s1.p; unsigned* fl_ = ctx->d_flag;
        const int k = L.k, pad = L.pad, W1 = s1.W;
        if (dst.need.on && L.dims == 2) {
            const size_t r0 = (size_t)std::max(0, w.y0 - L.pad), r1 = (size_t)std::min(s1.H, w.y1 + L.pad);
            const int c0 = w.x0, c1 = std::min(Wc, (w.x1 + 1) & ~1);
            e = enqueue(ctx, [=](hipStream_t st) { return launch_shiftx_split(sp_, X, k, pad, rows, W1, Wc, fl_, st, r0, r1, c0, c1); });
        } else {
            e = enqueue(ctx, [=](hipStream_t st) { return launch_shiftx_split(sp_, X, k, pad, rows, W1, Wc, fl_, st); });
        }
    }
    if (e != hipSuccess) return fail(ctx, "shiftx failed: %s", hipGetErrorString(e));
    SplitArgs a = split_args(ctx, X, ncell, {s1.D, s1.H, Wc}, L.cout, {dst.D, Hc, Wc}, 1, dhw(dst), L.dims == 3 ? L.k : 0, L.pad,
                             L.slope);
    a.pad_x = 0;                       // (the kx taps are channels of X)
    a.wpk = reinterpret_cast<const uint4*>(rt.d_wsplit);
    a.wscale = rt.d_wscale;
    a.bias = bias_view(ctx, rt.d_bias);
    a.out = reinterpret_cast<uint4*>(dst.p);
    a.n_chunks = rt.s_n_chunks;
    return launch_split(ctx, ks, a, rt.s_n_cog, conv_flops(L.cout, 1, L.k, L.dims, {dst.D, Hc, Wc}), w);
}

// 1-output-channel last conv on the 2xf16 path: k virtual output channels (one per kx tap) over W + 2*pad columns
// by a k x 1 column kernel storing fp32, then out[x] = sum_v Y[v][x + v] + bias (and the un-normalisation)
int run_last_split(tpz_ctx* ctx, const LayerRT& rt, const Slot& s1, Slot& dst, const float* d_nrm, int norm_out,
                   const Slot* sres = nullptr) {
    const tpz_layer& L = rt.L;
    const Window w = launch_window(dst.need, dhw(dst));       // what is needed of the output
    if (rt.d_wlast) {
        // one pass: stencil + bias + residual + un-normalisation (conv_cout1_split_kernel)
        const int z0 = w.z0, z1 = w.z1, y0 = w.y0, y1 = w.y1, x0 = w.x0, x1 = w.x1;
        const double vox = (double)(z1 - z0) * (y1 - y0) * (x1 - x0);
        const double taps = std::pow((double)L.k, L.dims);
        const double fl = conv_flops(1, L.cin, L.k, L.dims, {z1 - z0, y1 - y0, x1 - x0});
        // algorithmic bytes: the input box (with its halo) once, the output (and the residual) once, the weights once
        const double by = 32.0 * split_cells(s1.C) * (double)std::min(dst.D, z1 - z0 + (L.dims == 3 ? 2 * L.pad : 0)) *
                              std::min(dst.H, y1 - y0 + 2 * L.pad) * std::min(dst.W, x1 - x0 + 2 * L.pad) +
                          4.0 * vox * (sres ? 2 : 1) + 4.0 * L.cin * taps;
        const void* ip = s1.p; const float* wp_ = rt.d_wlast; float* op = dst.p;
        const float* resp = sres ? sres->p : nullptr;
        const float b0 = L.b_off >= 0 ? rt.bias0 : 0.f;
        const int cells = (int)split_cells(s1.C), k = L.k, kz = L.dims == 3 ? L.k : 1, Dd = dst.D, Hd = dst.H, Wd = dst.W;
        hipError_t e = enqueue(ctx, 0, fl, "conv_cout1_split_kernel (last conv: fp32 stencil on the vector ALUs + bias + un-normalisation)",
                               by, [=](hipStream_t st) {
                                   return launch_conv_cout1_split(ip, wp_, op, resp, d_nrm, norm_out, b0, cells, k, kz, Dd, Hd, Wd, z0, z1,
                                                                  y0, y1, x0, x1, st);
                               });
        if (e != hipSuccess) return fail(ctx, "conv_cout1_split failed: %s", hipGetErrorString(e));
        return 0;
    }
    const SplitKernelInfo& ks = *rt.ks_last;
    const int Wp = dst.W + 2 * L.pad;
    const size_t rows = (size_t)dst.D * dst.H;
    const WorkBuf Yb(ctx, (size_t)L.k * rows * Wp * sizeof(float));
    if (!Yb) return fail(ctx, "out of device memory");
    float* Y = Yb.as<float>();
    const Dhw lat = {dst.D, dst.H, Wp};
    SplitArgs a = split_args(ctx, s1.p, (int)split_cells(s1.C), dhw(s1), L.k, lat, 1, lat, L.dims == 3 ? L.k : 0, L.pad, 1.f);
    a.cells_out = 1;
    a.wpk = reinterpret_cast<const uint4*>(rt.d_wsplit);
    a.wscale = rt.d_wscale;
    a.out_f32 = Y;
    a.n_chunks = rt.s_n_chunks;
    Window wy = w;
    wy.x1 += 2 * L.pad;                   // Y columns x .. x + k - 1 feed output column x
    int rc = launch_split(ctx, ks, a, rt.s_n_cog, conv_flops(1, L.cin, L.k, L.dims, dhw(dst)), wy);
    if (!rc) {
        // (labelled: an HBM-bound kernel whose bandwidth bench.py reports -- reads k planes of Wp columns, writes one of W)
        const double ss_rows = (double)(w.y1 - w.y0) * (w.z1 - w.z0), ss_cols = (double)(w.x1 - w.x0);
        // (a residual of the output's own size -- UDenoiseNet3: x - dec1(h), weights negated -- is added here, in fp32)
        const float* resp = sres ? sres->p : nullptr;
        float* dp_ = dst.p;
        const int k = L.k, Wd = dst.W;
        const float b0 = L.b_off >= 0 ? rt.bias0 : 0.f;
        const size_t r0 = (size_t)w.y0, r1 = (size_t)w.y1;
        const int c0 = w.x0, c1 = w.x1, Hp = dst.H, z0 = w.z0, z1 = w.z1;
        hipError_t e = enqueue(ctx, 2, 0.0, "shiftsum (last conv: sum of the k column-kernel planes + bias + un-normalisation)",
                               4.0 * ss_rows * ((double)L.k * (ss_cols + 2 * L.pad) + ss_cols), [=](hipStream_t st) {
                                   return launch_shiftsum(Y, dp_, k, rows, Wd, Wp, b0, d_nrm, norm_out, st, r0, r1, c0, c1, resp, Hp, z0, z1);
                               });
        if (e != hipSuccess) rc = fail(ctx, "shiftsum failed: %s", hipGetErrorString(e));
    }
    return rc;
}

// the buffers of the workspace pool behind a slot (a Slot is a view and is copied freely): run_program holds one per slot
struct SlotBufs {
    WorkBuf own;      // the tensor the producing layer wrote (none: the caller's input or output)
    WorkBuf alt;      // the same tensor converted to the other format for a consumer that needs it
};

// the slot's 2-D tensor in the wanted format: the producer's own buffer, or a converted copy made once
float* slot_as(tpz_ctx* ctx, const Slot& s, SlotBufs& b, bool want_split) {
    if (s.split == want_split) return s.p;
    if (b.alt) return b.alt.as<float>();
    if (s.pitch != s.W || s.ps != (long long)s.H * s.W || s.cs != s.ps * s.D) return nullptr;
    const size_t c_alloc = want_split ? split_cells(s.C) * 8 : (size_t)s.C;
    WorkBuf qb(ctx, c_alloc * s.D * s.H * s.W * sizeof(float));
    if (!qb) return nullptr;
    float* q = qb.as<float>();
    // cells are [c/8][D*H*W]: a volume converts as an image of D*H rows
    hipError_t e;
    {
        const float* sp_ = s.p; unsigned* fl_ = ctx->d_flag;
        const int C = s.C, R = s.D * s.H, W = s.W;
        e = enqueue(ctx, [=](hipStream_t st) {
            return want_split ? launch_to_split(sp_, q, C, R, W, fl_, st) : launch_from_split(sp_, q, C, R, W, st);
        });
    }
    if (e != hipSuccess) return nullptr;
    b.alt = std::move(qb);
    return q;
}
// ... the slot as a source in that format; .p == nullptr: the conversion failed
Slot source_view(tpz_ctx* ctx, const Slot& s, SlotBufs& b, bool want_split) {
    Slot v = s;
    v.p = slot_as(ctx, s, b, want_split);
    v.split = want_split;
    return v;
}

// Gives layer i its destination: C channels of `o` voxels as fp32 planes or (split) as split cells, which take the bytes of fp32
// with the channels rounded up to whole 8-channel cells -- d_out for the last layer, else a buffer of the workspace pool that
// `b` then owns (whatever it held before goes back).  `need`: the part of the tensor anything reads.
int make_dst(tpz_ctx* ctx, Slot& dst, SlotBufs& b, int i, bool last, float* d_out, int C, bool split, const Dhw& o, const Rect& need) {
    const size_t c_alloc = split ? split_cells(C) * 8 : (size_t)C;
    WorkBuf nb = last ? WorkBuf() : WorkBuf(ctx, c_alloc * o.D * o.H * o.W * sizeof(float));
    float* p = last ? d_out : nb.as<float>();
    if (!p) return fail(ctx, "out of device memory (layer %d)", i);
    set_dense(dst, p, C, o.D, o.H, o.W);
    dst.need = need;
    dst.split = split;
    dst.pooled = false;
    b.own = std::move(nb);
    b.alt.release();
    return 0;
}

int run_conv(tpz_ctx* ctx, const LayerRT& rt, const Slot& s1, const Slot* s2, const Slot* sres, Slot& dst,
             const float* d_nrm, int norm_out, bool split_out = false) {
    const tpz_layer& L = rt.L;
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.in = s1.p;
    a.in2 = s2 ? s2->p : nullptr;
    a.wpk = rt.d_wpk;
    a.bias = bias_view(ctx, rt.d_bias);
    a.res = sres ? sres->p : nullptr;
    a.post_scale = rt.d_post_scale;
    a.post_shift = bias_view(ctx, rt.d_post_shift);
    a.head_w = rt.d_head_w;
    a.head_b = ctx->scaled_pass ? 0.f : rt.head_b;
    a.nrm = d_nrm;
    a.zeros = ctx->d_zeros;
    a.norm_out = d_nrm ? norm_out : 0;
    a.Cin = L.cin;
    a.Cin1 = s1.C;
    const Slot& geo = s2 ? *s2 : s1;
    a.Din = geo.D; a.Hin = geo.H; a.Win = geo.W;
    a.D1 = s1.D; a.H1 = s1.H; a.W1 = s1.W;
    a.cs1 = s1.cs; a.ps1 = s1.ps; a.pitch1 = s1.pitch;
    if (s2) { a.cs2 = s2->cs; a.ps2 = s2->ps; a.pitch2 = s2->pitch; }
    a.Cout = L.cout;
    a.Dout = dst.D; a.Hout = dst.H; a.Wout = dst.W;
    a.pad = L.pad;
    a.pad_x = a.pad_y = a.pad_z = L.pad;
    a.os = 1;
    a.Dfull = dst.D; a.Hfull = dst.H; a.Wfull = dst.W;
    if (sres) { a.Dres = sres->D; a.Hres = sres->H; a.Wres = sres->W; a.res_crop = L.res_crop; }
    a.slope = L.slope;
    if (L.head) { a.head_out = dst.p; a.out = nullptr; }
    else a.out = dst.p;
    // patched / tiled denoise: only what the kept centre depends on (need_regions)
    const Window w = launch_window(dst.need, dhw(dst), 1, FP32_ALIGN_X);
    const double flops = conv_flops(L.cout, L.cin, L.k, L.dims, dhw(dst));
    if (rt.ki) {
        const ConvKernelInfo& ki = split_out ? *rt.ki_stem_split : *rt.ki;    // same tile and weight packing
        a.flag = ctx->d_flag;
        const LayerRT::Phase& ph = rt.phase;
        if (ph.valid && s2 && s1.C == ph.c1 && s2->C == ph.c2 && s2->H == 2 * s1.H && s2->W == 2 * s1.W &&
            (L.dims == 2 || s2->D == 2 * s1.D))
            return run_conv_phases(ctx, rt, a, s1, *s2, dst, w);
        if (s2 && (s1.C % ki.NCH) != 0)
            return fail(ctx, "fused concat needs the first source's channels (%d) to be a multiple of %d", s1.C, ki.NCH);
        a.n_chunks = rt.n_chunks;
        a.cog_inner = rt.cog_inner;
        if (launch_mfma(ctx, ki, a, rt.n_cog, flops, w)) return 1;
    } else {
        if (s1.D != geo.D || s1.H != geo.H || s1.W != geo.W) return fail(ctx, "direct conv cannot upsample");
        apply_window(a, w);
        const ConvArgs ac = a;
        const float* wp_ = rt.d_wpk;
        const int k = L.k, kz = L.dims == 3 ? L.k : 1, dil = L.dil;
        hipError_t e = enqueue(ctx, 1, flops * window_share(w, dhw(dst)), nullptr, 0.0,
                               [=](hipStream_t st) { return launch_conv_direct(ac, wp_, k, kz, dil, st); });
        HIPCHK(ctx, e);
    }
    return 0;
}

// runs the layer program.  `slots` holds preset external slots (at least slot 0); the dst of the last
// layer is written to d_out (dense).  d_nrm != nullptr: slot 0 is normalised on load wherever it is read
// and the output is un-normalised (Denoise._denoise, topaz/denoise.py:283-295).
// PyTorch 'nearest' source index exactly as the kernels compute it (conv_mfma.h nearest_src)
int nearest_src_host(int dst, int in_sz, int out_sz) {
    if (in_sz == out_sz) return dst;
    const float scale = (float)in_sz / (float)out_sz;
    const int v = (int)floorf((float)dst * scale);
    return v < in_sz - 1 ? v : in_sz - 1;
}

// May a layer that conv_plan gives this form compute just a window of its tensor in a 2xf16 pass?  The 2xf16 forms may.  The fp32
// forms may not: the format conversions either side of them read whole tensors, and what a windowed producer did not write may
// hold any bit pattern (the overflow flag).  Three named conditions depart from that rule; each is an open question, not a design:
bool form_windowable(ConvForm form, const LayerRT& rt, int dims) {
    // a column-kernel stem that reads a 1-channel tensor other than the input leaves its program whole (no model of the
    // package has one; the form itself windows like any other)
    const bool stem_off_input = form == FORM_STEM && rt.L.src != 0;
    // so does a 2-D per-parity layer with a 1-channel skip source that has no fused-loader kernel (rt.ks) beside it -- although
    // every launch of the form covers its window or the whole grid, and the same form is windowed in 3-D
    const bool parity_2d_image_skip = form == FORM_PARITY && dims == 2 && rt.sphase.ki_skip_stem && !rt.ks;
    // a 2-D decoder layer with per-parity kernels over a multi-channel skip source whose shapes are not exactly 2x and which has
    // no rt.ks runs on its fp32 kernel, between format conversions, and its program IS windowed: the case the rule above forbids
    const bool inexact_2d_decoder_on_fp32 = form == FORM_FP32 && dims == 2 && rt.sphase.valid && !rt.sphase.ki_skip_stem;
    if (stem_off_input || parity_2d_image_skip) return false;
    return form == FORM_SPLIT || form == FORM_SPLIT_FOLD || form == FORM_STEM || form == FORM_LAST || form == FORM_PARITY ||
           inexact_2d_decoder_on_fp32;
}

// Which part of every slot's tensor do the pixels `keep` of the program's output depend on?  (2-D programs, on the 2xf16
// kernels or -- exact mode -- on the fp32 kernels, whose launches take the same windows: ConvArgs::wy0..wx1.)  A patched denoise keeps only the centre of each patch (denoise.py:299-323: patch_size pixels of a patch_size +
// 2*padding tile; CLI default 1024 of 2024), and the U-Net's receptive field (~230 pixels) is far smaller than the default
// padding (500): most of what the full-size layers of a patch compute is thrown away.  Walking the layer list backwards from
// `keep` -- a conv needs its window grown by the padding, a 2x2 max-pool twice the window, a nearest-upsampled source the
// window mapped through the same index formula the kernel uses -- gives every layer the rectangle it has to produce; the
// launches cover just that (SplitArgs::wy0..wx1).  Nothing else changes: the tensors keep their full-size layout and
// coordinates, every kept pixel is computed by the same instructions on the same operands as before (bit-identical output,
// tests/test_gpu_denoise.py), the statistics of the normalisation are still those of the whole padded patch.
// 3-D programs (the tiles of Denoise3D.denoise, denoise.py:340-377: patch_size^3 voxels kept of a (patch_size + 2*padding)^3
// tile -- 1/8 of the tile at the CLI's 96 / 48) are windowed the same way with boxes instead of rectangles, on the 2xf16
// kernels only: the plane-stacked launches take the planes of the box (SplitArgs::wz0, Dout) besides its rectangle.
// Returns an empty vector when the program cannot be windowed (a 3-D program on the fp32 kernels, a 2xf16 program with a layer
// left on an fp32 kernel, an op it does not know).
std::vector<Rect> need_regions(const tpz_model* m, int D0, int H0, int W0, const Rect& keep, bool split) {
    const int nl = (int)m->layers.size();
    std::vector<Rect> need;
    // (TPZ_TRACE_HOST=1 says which check left a program whole)
    auto bail = [&](int why) {
        if (m->ctx->dbg.trace_host) fprintf(stderr, "[tpz host] need_regions: program left whole (check %d)\n", why);
        need.clear();
        return need;
    };
    if (!keep.on || !m->ctx->roi_enabled || nl == 0) return need;
    const int dims = D0 > 1 ? 3 : 2;
    // (round 5: the fp32 kernels of a 3-D program take boxes as well -- ConvArgs::wz0 / wz1 -- so exact mode and an overflow
    // re-run of a tiled tomogram no longer compute every tile in full)
    // shapes of all slots
    std::vector<int> Ds(m->n_slots, 1), Hs(m->n_slots, 0), Ws(m->n_slots, 0);
    std::vector<char> fmt(m->n_slots, 0), set(m->n_slots, 0);      // ... their format (1: split cells), as run_program will leave it
    Ds[0] = D0; Hs[0] = H0; Ws[0] = W0; set[0] = 1;
    auto shape = [&](int s) { return Dhw{Ds[s], Hs[s], Ws[s]}; };
    for (int i = 0; i < nl; ++i) {
        const LayerRT& rt = m->layers[i];
        const tpz_layer& L = rt.L;
        if (L.dims != dims) return bail(2);
        const int g = (L.op == TPZ_OP_CONV && L.src2 >= 0) ? L.src2 : L.src;
        if (L.op == TPZ_OP_CONV) {
            const Dhw g2 = shape(g);
            const ConvPlan pl = conv_plan(m, i, split, shape(L.src), L.src2 >= 0 ? &g2 : nullptr, fmt[L.src] != 0,
                                          rt.fold_src >= 0 && set[rt.fold_src]);
            if (pl.form == FORM_FOLDED_AWAY) return bail(2);
            if (split && !form_windowable(pl.form, rt, dims)) return bail(3);
            fmt[L.dst] = pl.split_dst;
        } else if (L.op == TPZ_OP_MAXPOOL2 || (L.op == TPZ_OP_MAXPOOL && L.pad == 0)) {      // (a padded pool: bail(4), not windowed)
            fmt[L.dst] = fmt[L.src] && i != nl - 1;                // pooled in the format the source has
        } else {
            return bail(4);
        }
        const Dhw o = layer_out_dhw(L, shape(g));
        Ds[L.dst] = o.D; Hs[L.dst] = o.H; Ws[L.dst] = o.W; set[L.dst] = 1;
        if (o.D < 1 || o.H < 1 || o.W < 1) return bail(5);
    }
    need.assign(m->n_slots, Rect());
    // (2-D: every box is the one plane [0, 1))
    auto clip = [&](Rect r, int slot) {
        r.y0 = std::max(0, r.y0); r.x0 = std::max(0, r.x0);
        r.y1 = std::min(Hs[slot], r.y1); r.x1 = std::min(Ws[slot], r.x1);
        if (dims == 3) { r.z0 = std::max(0, r.z0); r.z1 = std::min(Ds[slot], r.z1); }
        else { r.z0 = 0; r.z1 = 1; }
        r.on = true;
        return r;
    };
    need[m->layers[nl - 1].L.dst] = clip(keep, m->layers[nl - 1].L.dst);
    for (int i = nl - 1; i >= 0; --i) {
        const tpz_layer& L = m->layers[i].L;
        Rect R = need[L.dst];
        if (!R.on) { return bail(6); }            // a tensor nobody reads: leave the program alone
        if (L.op == TPZ_OP_CONV) {
            // launch windows start and end on even pixels: the per-parity kernels work on the half-resolution lattice, a
            // fused max-pool pairs rows and columns
            R.y0 &= ~1; R.x0 &= ~1;
            R.y1 = std::min(Hs[L.dst], (R.y1 + 1) & ~1); R.x1 = std::min(Ws[L.dst], (R.x1 + 1) & ~1);
            if (dims == 3) { R.z0 &= ~1; R.z1 = std::min(Ds[L.dst], (R.z1 + 1) & ~1); }
            need[L.dst] = R;
            const int g = L.src2 >= 0 ? L.src2 : L.src, span = L.dil * (L.k - 1);
            Rect G;                                           // in the coordinates of the (upsampled) input grid
            G.y0 = R.y0 - L.pad; G.x0 = R.x0 - L.pad; G.y1 = R.y1 - L.pad + span; G.x1 = R.x1 - L.pad + span;
            if (dims == 3) { G.z0 = R.z0 - L.pad; G.z1 = R.z1 - L.pad + span; }
            G = clip(G, g);
            if (L.src2 >= 0) {
                need[L.src2].unite(G);
                Rect S;                                       // the first source, nearest-upsampled to the grid of the second
                S.y0 = nearest_src_host(G.y0, Hs[L.src], Hs[g]); S.y1 = nearest_src_host(G.y1 - 1, Hs[L.src], Hs[g]) + 1;
                S.x0 = nearest_src_host(G.x0, Ws[L.src], Ws[g]); S.x1 = nearest_src_host(G.x1 - 1, Ws[L.src], Ws[g]) + 1;
                if (dims == 3) { S.z0 = nearest_src_host(G.z0, Ds[L.src], Ds[g]); S.z1 = nearest_src_host(G.z1 - 1, Ds[L.src], Ds[g]) + 1; }
                need[L.src].unite(clip(S, L.src));
            } else {
                need[L.src].unite(G);
            }
            if (L.res >= 0) {
                Rect Q = R;
                Q.y0 += L.res_crop; Q.y1 += L.res_crop; Q.x0 += L.res_crop; Q.x1 += L.res_crop;
                if (dims == 3) { Q.z0 += L.res_crop; Q.z1 += L.res_crop; }
                need[L.res].unite(clip(Q, L.res));
            }
        } else if (L.op == TPZ_OP_MAXPOOL2) {
            Rect Q;
            Q.y0 = 2 * R.y0; Q.x0 = 2 * R.x0; Q.y1 = 2 * R.y1; Q.x1 = 2 * R.x1;
            if (dims == 3) { Q.z0 = 2 * R.z0; Q.z1 = 2 * R.z1; }
            need[L.src].unite(clip(Q, L.src));
        } else {
            Rect Q = R;
            Q.y1 += L.dil * (L.k - 1); Q.x1 += L.dil * (L.k - 1);
            if (dims == 3) Q.z1 += L.dil * (L.k - 1);
            need[L.src].unite(clip(Q, L.src));
        }
    }
    if (m->ctx->dbg.trace_host)
        for (int i = 0; i < nl; ++i) {
            const tpz_layer& L = m->layers[i].L;
            const Rect& r = need[L.dst];
            fprintf(stderr, "[tpz host] need_regions: layer %d op %d -> slot %d: z [%d, %d) of %d, y [%d, %d) of %d, x [%d, %d) of %d\n", i,
                    (int)L.op, L.dst, r.z0, r.z1, Ds[L.dst], r.y0, r.y1, Hs[L.dst], r.x0, r.x1, Ws[L.dst]);
        }
    return need;
}

}  // namespace

int run_program(tpz_model* m, std::vector<Slot>& slots, float* d_out, const float* d_nrm, bool split, const Rect* keep) {
    tpz_ctx* ctx = m->ctx;
    const int nl = (int)m->layers.size();
    slots.resize(std::max<size_t>(slots.size(), (size_t)m->n_slots));
    std::vector<Rect> need;
    if (keep && slots[0].set) need = need_regions(m, slots[0].D, slots[0].H, slots[0].W, *keep, split);
    auto need_of = [&](int slot) { return need.empty() ? Rect() : need[slot]; };
    std::vector<SlotBufs> bufs(slots.size());      // what the slots own: back in the pool when this returns, if not before
    int rc = 0;
    for (int i = 0; i < nl && rc == 0; ++i) {
        const LayerRT& rt = m->layers[i];
        const tpz_layer& L = rt.L;
        const Slot& s1 = slots[L.src];
        if (!s1.set) { rc = fail(ctx, "layer %d reads unset slot %d", i, L.src); break; }
        Slot& dst = slots[L.dst];
        const bool last = i == nl - 1;
        const Slot* s2 = (L.op == TPZ_OP_CONV && L.src2 >= 0) ? &slots[L.src2] : nullptr;
        const Dhw g2 = s2 ? dhw(*s2) : Dhw();
        // which kernels run a conv layer, and in which formats: conv_plan's decision, dispatched below
        const ConvPlan pl = L.op == TPZ_OP_CONV ? conv_plan(m, i, split, dhw(s1), s2 ? &g2 : nullptr, s1.split,
                                                            rt.fold_src >= 0 && slots[rt.fold_src].set) : ConvPlan();
        if (pl.form == FORM_FOLDED_AWAY) {
            // a 1x1 projection folded into the conv that adds it (prepare_split): nothing to run, its slot stays unset
        } else if (L.op == TPZ_OP_CONV) {
            const Slot* sres = (L.res >= 0 && pl.form != FORM_SPLIT_FOLD) ? &slots[L.res] : nullptr;
            if ((s2 && !s2->set) || (sres && !sres->set)) { rc = fail(ctx, "layer %d reads an unset slot", i); break; }
            const Slot& geo = s2 ? *s2 : s1;
            if (s1.C + (s2 ? s2->C : 0) != L.cin) {
                rc = fail(ctx, "layer %d: cin %d != channels of its sources (%d)", i, L.cin, s1.C + (s2 ? s2->C : 0));
                break;
            }
            const Dhw o = layer_out_dhw(L, dhw(geo));
            if (o.D < 1 || o.H < 1 || o.W < 1) { rc = fail(ctx, "layer %d: input %dx%dx%d too small", i, geo.D, geo.H, geo.W); break; }
            const int Co = L.head ? 1 : L.cout;
            if (sres && (sres->H - 2 * L.res_crop != o.H || sres->W - 2 * L.res_crop != o.W || sres->C != L.cout)) {
                rc = fail(ctx, "layer %d: residual geometry mismatch", i);
                break;
            }
            // a fused max-pool: the slot receives the pooled tensor (and keeps its need in the coordinates of the conv output)
            const Dhw od = {o.D, pl.fuse_pool ? o.H / 2 : o.H, pl.fuse_pool ? o.W / 2 : o.W};
            if (pl.fuse_pool && (od.H < 1 || od.W < 1)) { rc = fail(ctx, "layer %d: input too small to pool", i + 1); break; }
            if ((rc = make_dst(ctx, dst, bufs[L.dst], i, last, d_out, Co, pl.split_dst, od, need_of(L.dst)))) break;
            dst.pooled = pl.fuse_pool;
            if (pl.split_dst && last) { rc = fail(ctx, "layer %d: the result must leave as fp32", i); break; }
            // sources in the format the chosen kernels read (converted once if the producer wrote the other one)
            const Slot v1 = source_view(ctx, slots[L.src], bufs[L.src], pl.split1);
            const Slot v2 = s2 ? source_view(ctx, slots[L.src2], bufs[L.src2], pl.split2) : Slot();
            const Slot vres = sres ? source_view(ctx, slots[L.res], bufs[L.res], pl.split_res) : Slot();
            if (!v1.p || (s2 && !v2.p) || (sres && !vres.p)) { rc = fail(ctx, "layer %d: tensor format conversion failed", i); break; }
            // slot 0 arrives already normalised (denoise_region); only the last layer un-normalises
            const int norm_out = (d_nrm && last) ? 1 : 0;
            switch (pl.form) {
            case FORM_STEM: rc = run_stem_split(ctx, rt, v1, dst, pl.fuse_pool); break;
            case FORM_LAST: rc = run_last_split(ctx, rt, v1, dst, d_nrm, norm_out, sres ? &vres : nullptr); break;
            case FORM_PARITY: rc = run_conv_split_phases(ctx, rt, v1, v2, dst); break;
            case FORM_SPLIT_FOLD: {
                const Slot vf = source_view(ctx, slots[rt.fold_src], bufs[rt.fold_src], true);
                if (!vf.p) rc = fail(ctx, "layer %d: tensor format conversion failed", i);
                else rc = run_conv_split(ctx, rt, v1, nullptr, dst, nullptr, false, &vf);
                break;
            }
            case FORM_SPLIT: rc = run_conv_split(ctx, rt, v1, sres ? &vres : nullptr, dst, s2 ? &v2 : nullptr, pl.fuse_pool); break;
            default: rc = run_conv(ctx, rt, v1, s2 ? &v2 : nullptr, sres ? &vres : nullptr, dst, d_nrm, norm_out,
                                   pl.form == FORM_FP32_STEM_SPLIT);
            }
        } else if (L.op == TPZ_OP_MAXPOOL2 && s1.pooled && L.dims == 3) {
            // pooled in-plane by the producing conv: the z pairs remain
            const Slot src = s1;
            if (src.D / 2 < 1) { rc = fail(ctx, "layer %d: input too small to pool", i); break; }
            if ((rc = make_dst(ctx, dst, bufs[L.dst], i, last, d_out, src.C, true, {src.D / 2, src.H, src.W}, need_of(L.dst)))) break;
            hipError_t e;
            {
                const float* sp_ = src.p; float* dp_ = dst.p;
                const int C = src.C, Dd = src.D, Hh = src.H, Ww = src.W;
                e = enqueue(ctx, [=](hipStream_t st) { return launch_maxpoolz_split(sp_, dp_, C, Dd, Hh, Ww, st); });
            }
            if (e != hipSuccess) rc = fail(ctx, "maxpool launch failed: %s", hipGetErrorString(e));
        } else if (L.op == TPZ_OP_MAXPOOL2 && s1.pooled) {
            // already pooled by the producing conv: the slot changes hands
            dst = s1;
            dst.need = need_of(L.dst);
            dst.pooled = false;
            bufs[L.dst] = std::move(bufs[L.src]);
        } else if (L.op == TPZ_OP_MAXPOOL2 || L.op == TPZ_OP_MAXPOOL || L.op == TPZ_OP_AVGPOOL) {
            if (s1.pitch != s1.W || s1.ps != (long long)s1.H * s1.W) { rc = fail(ctx, "maxpool needs a dense input"); break; }
            const Dhw o = layer_out_dhw(L, dhw(s1));
            if (o.D < 1 || o.H < 1 || o.W < 1) { rc = fail(ctx, "layer %d: input too small to pool", i); break; }
            const bool sp = s1.split && !last;                // pooled in the format the source has
            const float* src_p = s1.p;
            if (s1.split && !sp) { src_p = slot_as(ctx, slots[L.src], bufs[L.src], false); if (!src_p) { rc = fail(ctx, "conversion failed"); break; } }
            const int Cs = s1.C, Ds = s1.D, Hs = s1.H, Ws = s1.W;
            if ((rc = make_dst(ctx, dst, bufs[L.dst], i, last, d_out, Cs, sp, o, need_of(L.dst)))) break;
            float* dp_ = dst.p;
            const int k = L.k, dil = L.dil, dims = L.dims, pad = L.pad;
            const bool by2 = L.op == TPZ_OP_MAXPOOL2, padded = is_padded_pool(L), mean = L.op == TPZ_OP_AVGPOOL;
            const hipError_t e = enqueue(ctx, [=](hipStream_t st) {
                if (padded) return launch_pool_pad(src_p, dp_, Cs, Ds, Hs, Ws, dil, pad, dims, mean, sp, st);   // (pad = 0: the kernel below, as before)
                if (!by2) return launch_maxpoolk(src_p, dp_, Cs, Ds, Hs, Ws, k, dil, dims, sp, st);
                return sp ? launch_maxpool2_split(src_p, dp_, Cs, Ds, Hs, Ws, dims, st) : launch_maxpool2(src_p, dp_, Cs, Ds, Hs, Ws, dims, st);
            });
            if (e != hipSuccess) rc = fail(ctx, "maxpool launch failed: %s", hipGetErrorString(e));
        } else {
            rc = fail(ctx, "layer %d: unknown op %d", i, L.op);
        }
        // release intermediates whose last reader was this layer
        for (int s = 0; s < m->n_slots; ++s)
            if (slots[s].set && m->last_use[s] == i) { bufs[s].own.release(); bufs[s].alt.release(); }
    }
    return rc;
}

}  // namespace tpz::rt
