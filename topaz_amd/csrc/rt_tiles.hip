// Score tiles cut and stitched on the device: the zero-padded window of get_patches without the padded copy of the
// image (tpz_tile_cut), the all-zero test of every tile of the grid in one launch (tpz_tile_flags) and the cropped paste into the
// stitched map (tpz_tile_paste).  Three bandwidth kernels, here with their entry points: grid-stride loops over groups of four
// consecutive x of one row, no LDS, no atomics.  A group moves as one 16-byte access wherever its side of the copy is 16-byte
// aligned and whole, element by element otherwise -- decided per group, so a tensor view at an odd float offset, a width that is
// no multiple of four and a window that straddles an edge take the same kernel.  Pixels move as 32-bit words: nothing here can
// touch a NaN payload, a signed zero or a subnormal.
#include "rt_internal.h"

namespace tpz::rt {
namespace {

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct TileGeom {
    int D, H, W;        // the tensor
    int td, th, tw;     // the window / tile
};

// the four words of window row (sz, sy) from x = sx on; 0 outside the tensor
__device__ __forceinline__ uint4 window_quad(const unsigned* __restrict__ src, const TileGeom& g, int sz, int sy, int sx) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (sz < 0 || sz >= g.D || sy < 0 || sy >= g.H || sx + 3 < 0 || sx >= g.W) return v;
    const unsigned* r = src + ((long long)sz * g.H + sy) * g.W;             // an in-tensor row
    if (sx >= 0 && sx + 4 <= g.W && aligned16(r + sx)) return *reinterpret_cast<const uint4*>(r + sx);
    if (sx >= 0) v.x = r[sx];
    if (sx + 1 >= 0 && sx + 1 < g.W) v.y = r[sx + 1];
    if (sx + 2 >= 0 && sx + 2 < g.W) v.z = r[sx + 2];
    if (sx + 3 < g.W) v.w = r[sx + 3];
    return v;
}

// (a window has fewer than 2^31 elements -- the entry points refuse more --, so the walk over its groups is 32-bit arithmetic)
__global__ __launch_bounds__(256) void tile_cut_kernel(const unsigned* __restrict__ src, TileGeom g, int z0, int y0, int x0,
                                                       unsigned* __restrict__ dst) {
    const unsigned qw = (unsigned)(g.tw + 3) >> 2;
    const unsigned nq = (unsigned)g.td * g.th * qw;
    for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int xq = (int)(q % qw) * 4;
        const unsigned row = q / qw;
        const int y = (int)(row % g.th), z = (int)(row / g.th);
        const uint4 v = window_quad(src, g, z0 + z, y0 + y, x0 + xq);
        unsigned* d = dst + (size_t)row * g.tw + xq;
        const int rem = g.tw - xq;
        if (rem >= 4 && aligned16(d)) {
            *reinterpret_cast<uint4*>(d) = v;
        } else {
            d[0] = v.x;
            if (rem > 1) d[1] = v.y;
            if (rem > 2) d[2] = v.z;
            if (rem > 3) d[3] = v.w;
        }
    }
}

// flag[t] = 1 when window t holds an in-tensor element other than +-0 (torch's ne(0): NaN counts).  Every thread that sees one
// stores the constant 1: the stores race to the same value, nothing is read back in the kernel.  blockIdx.y strides the windows.
__global__ __launch_bounds__(256) void tile_flags_kernel(const unsigned* __restrict__ src, TileGeom g,
                                                         const int* __restrict__ origins, unsigned n, unsigned* __restrict__ flags) {
    const unsigned qw = (unsigned)(g.tw + 3) >> 2;
    const unsigned nq = (unsigned)g.td * g.th * qw;
    for (unsigned t = blockIdx.y; t < n; t += gridDim.y) {
        const int z0 = origins[3 * (size_t)t], y0 = origins[3 * (size_t)t + 1], x0 = origins[3 * (size_t)t + 2];
        bool any = false;
        for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
            const int xq = (int)(q % qw) * 4;
            const unsigned row = q / qw;
            const int y = (int)(row % g.th), z = (int)(row / g.th);
            uint4 v = window_quad(src, g, z0 + z, y0 + y, x0 + xq);
            const int rem = g.tw - xq;                  // (a last group reaches past the window: those words are not its own)
            if (rem < 4) v.w = 0u;
            if (rem < 3) v.z = 0u;
            if (rem < 2) v.y = 0u;
            any |= ((v.x | v.y | v.z | v.w) & 0x7fffffffu) != 0u;
        }
        if (any) flags[t] = 1u;
    }
}

struct PasteGeom {
    int th, tw;             // rows and row length of the tile
    int cz, cy, cx;         // the first element of the box in the tile
    int nz, ny, nx;         // the box
    int D, H, W;            // the canvas
    int z, y, x;            // where the box goes
};

// words [lo, hi) of v to row[dx + lo .. dx + hi): 0 <= lo < hi <= 4 and those elements are in the row
__device__ __forceinline__ void store_quad(float* row, int dx, uint4 v, int lo, int hi) {
    if (lo == 0 && hi == 4 && aligned16(row + dx)) {
        *reinterpret_cast<uint4*>(row + dx) = v;
        return;
    }
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= lo && j < hi) reinterpret_cast<unsigned*>(row)[dx + j] = w[j];
}

__device__ __forceinline__ void store_quad(double* row, int dx, uint4 v, int lo, int hi) {
    const double w[4] = {(double)__uint_as_float(v.x), (double)__uint_as_float(v.y), (double)__uint_as_float(v.z),
                         (double)__uint_as_float(v.w)};
    if (lo == 0 && hi == 4 && aligned16(row + dx)) {
        reinterpret_cast<double2*>(row + dx)[0] = make_double2(w[0], w[1]);
        reinterpret_cast<double2*>(row + dx)[1] = make_double2(w[2], w[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= lo && j < hi) row[dx + j] = w[j];
}

template <class T>
__global__ __launch_bounds__(256) void tile_paste_kernel(const unsigned* __restrict__ tile, PasteGeom g, T* __restrict__ canvas) {
    const unsigned qw = (unsigned)(g.nx + 3) >> 2;
    const unsigned nq = (unsigned)g.nz * g.ny * qw;
    for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int bx = (int)(q % qw) * 4;
        const unsigned row = q / qw;
        const int by = (int)(row % g.ny), bz = (int)(row / g.ny);
        const int dz = g.z + bz, dy = g.y + by, dx = g.x + bx;
        if (dz < 0 || dz >= g.D || dy < 0 || dy >= g.H) continue;
        // the group's elements [lo, hi) are in the box and in the canvas row
        const int have = g.nx - bx < 4 ? g.nx - bx : 4;
        const int lo = dx < 0 ? (dx < -4 ? 4 : -dx) : 0;
        const int hi = dx >= g.W ? 0 : (dx + have > g.W ? g.W - dx : have);
        if (lo >= hi) continue;
        const unsigned* s = tile + ((size_t)(g.cz + bz) * g.th + (g.cy + by)) * g.tw + g.cx + bx;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (have == 4 && aligned16(s)) {
            v = *reinterpret_cast<const uint4*>(s);
        } else {                                        // (s[j] for j < have is in the box, hence in the tile)
            v.x = s[0];
            if (have > 1) v.y = s[1];
            if (have > 2) v.z = s[2];
            if (have > 3) v.w = s[3];
        }
        store_quad(canvas + ((long long)dz * g.H + dy) * g.W, dx, v, lo, hi);
    }
}

// the extents of a tile / window / box the kernels walk with 32-bit arithmetic, and the origins they add them to
inline bool extents_ok(int a, int b, int c) {
    return a <= (1 << 30) && b <= (1 << 30) && c <= (1 << 30) && (unsigned long long)a * b * c < (1ull << 31);
}
inline bool origin_ok(int v) { return v >= -(1 << 29) && v <= (1 << 29); }

inline int quad_grid(size_t nq) { return (int)std::min<size_t>((nq + 255) / 256, 8192); }

}  // namespace
}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_tile_cut(tpz_ctx* ctx, const float* d_x, int D, int H, int W, int z0, int y0, int x0, int td, int th, int tw,
                 float* d_tile) {
    if (!ctx || !d_x || !d_tile) return fail(ctx, "tpz_tile_cut: bad arguments");
    if (D < 1 || H < 1 || W < 1 || td < 1 || th < 1 || tw < 1)
        return fail(ctx, "tpz_tile_cut: tensor %d x %d x %d and tile %d x %d x %d must be positive", D, H, W, td, th, tw);
    if (((uintptr_t)d_x & 3) || ((uintptr_t)d_tile & 3)) return fail(ctx, "tpz_tile_cut: d_x and d_tile must be 4-byte aligned");
    if (!extents_ok(td, th, tw))
        return fail(ctx, "tpz_tile_cut: a tile of %d x %d x %d has 2^31 elements or more", td, th, tw);
    if (!origin_ok(z0) || !origin_ok(y0) || !origin_ok(x0))      // (window coordinates are formed as origin + offset in int)
        return fail(ctx, "tpz_tile_cut: origin (%d, %d, %d) is beyond +-2^29", z0, y0, x0);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const TileGeom g{D, H, W, td, th, tw};
    const size_t nq = (size_t)td * th * ((tw + 3) / 4);
    const unsigned* src = reinterpret_cast<const unsigned*>(d_x);
    unsigned* dst = reinterpret_cast<unsigned*>(d_tile);
    HIPCHK(ctx, enqueue(ctx, 2, 0.0, nullptr, 8.0 * td * th * tw, [=](hipStream_t st) {
        hipLaunchKernelGGL(tile_cut_kernel, dim3(quad_grid(nq)), dim3(256), 0, st, src, g, z0, y0, x0, dst);
        return hipGetLastError();
    }));
    return 0;
}

int tpz_tile_flags(tpz_ctx* ctx, const float* d_x, int D, int H, int W, const int* h_origins, size_t n, int td, int th, int tw,
                   unsigned* d_flags) {
    if (!ctx || !d_x || (n && (!h_origins || !d_flags))) return fail(ctx, "tpz_tile_flags: bad arguments");
    if (D < 1 || H < 1 || W < 1 || td < 1 || th < 1 || tw < 1)
        return fail(ctx, "tpz_tile_flags: tensor %d x %d x %d and window %d x %d x %d must be positive", D, H, W, td, th, tw);
    if (((uintptr_t)d_x & 3) || ((uintptr_t)d_flags & 3)) return fail(ctx, "tpz_tile_flags: d_x and d_flags must be 4-byte aligned");
    if (!extents_ok(td, th, tw))
        return fail(ctx, "tpz_tile_flags: a window of %d x %d x %d has 2^31 elements or more", td, th, tw);
    if (n >= ((size_t)1 << 31)) return fail(ctx, "tpz_tile_flags: %zu windows: 2^31 or more", n);
    for (size_t i = 0; i < 3 * n; ++i)
        if (!origin_ok(h_origins[i]))
            return fail(ctx, "tpz_tile_flags: origin %d (window %zu) is beyond +-2^29", h_origins[i], i / 3);
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (the origins go back to the pool of this stream: whatever takes the buffer next is queued behind the kernel)
    const WorkBuf org_b(ctx, 3 * n * sizeof(int));
    int* d_org = org_b.as<int>();
    if (!d_org) return fail(ctx, "tpz_tile_flags: workspace allocation failed");
    HIPCHK(ctx, hipMemcpyAsync(d_org, h_origins, 3 * n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, n * sizeof(unsigned), ctx->stream));
    const TileGeom g{D, H, W, td, th, tw};
    // blocks: x over the groups of one window, y over the windows, about 16 K in all
    const int gx = (int)std::min<size_t>(((size_t)td * th * ((tw + 3) / 4) + 255) / 256, 1024);
    const int gy = (int)std::min<size_t>(n, (size_t)std::max(1, 16384 / gx));
    const unsigned* src = reinterpret_cast<const unsigned*>(d_x);
    HIPCHK(ctx, enqueue(ctx, 2, 0.0, nullptr, 4.0 * td * th * tw * n, [=](hipStream_t st) {
        hipLaunchKernelGGL(tile_flags_kernel, dim3(gx, gy), dim3(256), 0, st, src, g, (const int*)d_org, (unsigned)n, d_flags);
        return hipGetLastError();
    }));
    return 0;
}

int tpz_tile_paste(tpz_ctx* ctx, const float* d_tile, int td, int th, int tw, int cz, int cy, int cx, int nz, int ny, int nx,
                   void* d_canvas, int canvas_f64, int D, int H, int W, int z, int y, int x) {
    if (!ctx || !d_tile || !d_canvas) return fail(ctx, "tpz_tile_paste: bad arguments");
    if (D < 1 || H < 1 || W < 1 || td < 1 || th < 1 || tw < 1 || nz < 1 || ny < 1 || nx < 1)
        return fail(ctx, "tpz_tile_paste: canvas %d x %d x %d, tile %d x %d x %d and box %d x %d x %d must be positive", D, H, W,
                    td, th, tw, nz, ny, nx);
    if (cz < 0 || cy < 0 || cx < 0 || (long long)cz + nz > td || (long long)cy + ny > th || (long long)cx + nx > tw)
        return fail(ctx, "tpz_tile_paste: the box [%d, %d) x [%d, %d) x [%d, %d) is not inside the tile %d x %d x %d", cz,
                    cz + nz, cy, cy + ny, cx, cx + nx, td, th, tw);
    if (((uintptr_t)d_tile & 3) || ((uintptr_t)d_canvas & (canvas_f64 ? 7 : 3)))
        return fail(ctx, "tpz_tile_paste: d_tile must be 4-byte aligned and d_canvas aligned to its element");
    if (!extents_ok(td, th, tw))
        return fail(ctx, "tpz_tile_paste: a tile of %d x %d x %d has 2^31 elements or more", td, th, tw);
    if (!origin_ok(z) || !origin_ok(y) || !origin_ok(x))
        return fail(ctx, "tpz_tile_paste: position (%d, %d, %d) is beyond +-2^29", z, y, x);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const PasteGeom g{th, tw, cz, cy, cx, nz, ny, nx, D, H, W, z, y, x};
    const size_t nq = (size_t)nz * ny * ((nx + 3) / 4);
    const unsigned* src = reinterpret_cast<const unsigned*>(d_tile);
    HIPCHK(ctx, enqueue(ctx, 2, 0.0, nullptr, (canvas_f64 ? 12.0 : 8.0) * nz * ny * nx, [=](hipStream_t st) {
        if (canvas_f64)
            hipLaunchKernelGGL(tile_paste_kernel<double>, dim3(quad_grid(nq)), dim3(256), 0, st, src, g, (double*)d_canvas);
        else
            hipLaunchKernelGGL(tile_paste_kernel<float>, dim3(quad_grid(nq)), dim3(256), 0, st, src, g, (float*)d_canvas);
        return hipGetLastError();
    }));
    return 0;
}
