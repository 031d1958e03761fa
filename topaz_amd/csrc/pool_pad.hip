// Padded 3^dims pools, stride 1: the FILLED form of the pooling(3, stride = 2, padding = 1) layers of a BasicConv stack trained
// with `topaz train -m conv31|conv63|conv127 --pooling max|avg` (topaz/model/features/basic.py:33-39,54-56,81-89).  fill() sets
// every stride to 1, gives the modules that have a `dilation` attribute -- MaxPool, not AvgPool -- the accumulated stride as their
// dilation, and leaves padding = 1 as it is:
//   max   window of 3 taps per axis, `dil` apart, one element of -inf padding: n -> n + 2 - 2 * dil per axis
//   mean  plain 3^dims window (dilation 1), one element of zero padding, divisor 3^dims always (count_include_pad): n -> n
// Both are upstream quirks (the max map shrinks, the mean ignores the accumulated stride); upstream's `extract` scores with them.
// One pass, HBM-bound: grid-stride over output elements, every tap bounds-checked, no LDS.  fp32 planes and split cells
// (split_fmt.h: a hi and a lo plane of 16-byte cells of 8 channels).  The unpadded dilated max of the pooled ResNets stays in
// kernels_misc.hip (maxpoolk_kernel).
#include <hip/hip_runtime.h>
#include "kernels_misc.h"
#include "split_fmt.h"

namespace tpz {
namespace {

struct PoolGeo {
    int D, H, W, Do, Ho, Wo;
    int dil, pad;
    int kz;          // taps along z: 3 in 3-D, 1 in 2-D (D = Do = 1)
};

// element i of [c][Do][Ho][Wo] -> (c, z, y, x)
__device__ __forceinline__ void out_coords(size_t i, const PoolGeo& g, size_t& c, int& z, int& y, int& x) {
    x = (int)(i % g.Wo);
    size_t t = i / g.Wo;
    y = (int)(t % g.Ho);
    t /= g.Ho;
    z = (int)(t % g.Do);
    c = t / g.Do;
}

// Max.  Padding taps are skipped: they hold -inf and never win; the centre tap (offset dil - pad >= 0 from the output element) is
// always inside the tensor, so the running maximum -inf is replaced unless every tap IS -inf.  Taps in window row-major order,
// `v > m || v != v` as torch's max_pool: the first of equal values stays, a NaN propagates.
__global__ __launch_bounds__(256) void maxpool_pad_kernel(const float* __restrict__ in, float* __restrict__ out, size_t C,
                                                          const PoolGeo g) {
    const size_t n = C * g.Do * g.Ho * g.Wo;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        size_t c; int z, y, x;
        out_coords(i, g, c, z, y, x);
        const float* base = in + c * g.D * g.H * g.W;
        float m = -INFINITY;
        for (int kz = 0; kz < g.kz; ++kz) {
            const int gz = g.kz > 1 ? z - g.pad + kz * g.dil : 0;
            if ((unsigned)gz >= (unsigned)g.D) continue;
            for (int ky = 0; ky < 3; ++ky) {
                const int gy = y - g.pad + ky * g.dil;
                if ((unsigned)gy >= (unsigned)g.H) continue;
                const float* row = base + ((size_t)gz * g.H + gy) * g.W;
                for (int kx = 0; kx < 3; ++kx) {
                    const int gx = x - g.pad + kx * g.dil;
                    if ((unsigned)gx >= (unsigned)g.W) continue;
                    const float v = row[gx];
                    m = (v > m || v != v) ? v : m;
                }
            }
        }
        out[i] = m;
    }
}

// ... on split cells: hi + lo compares as the fp32 value it stands for and the winning (hi, lo) pair is carried, so the result
// equals the pooled fp32 value exactly
__global__ __launch_bounds__(256) void maxpool_pad_split_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                                size_t cells, const PoolGeo g) {
    const size_t n = cells * g.Do * g.Ho * g.Wo;
    const size_t plane_in = cells * g.D * g.H * g.W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        size_t c; int z, y, x;
        out_coords(i, g, c, z, y, x);
        const size_t base = c * g.D * g.H * g.W;
        f16x8 bh, bl;
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { bh[j] = (_Float16)(-INFINITY); bl[j] = (_Float16)0.f; m[j] = -INFINITY; }
        for (int kz = 0; kz < g.kz; ++kz) {
            const int gz = g.kz > 1 ? z - g.pad + kz * g.dil : 0;
            if ((unsigned)gz >= (unsigned)g.D) continue;
            for (int ky = 0; ky < 3; ++ky) {
                const int gy = y - g.pad + ky * g.dil;
                if ((unsigned)gy >= (unsigned)g.H) continue;
                const size_t row = base + ((size_t)gz * g.H + gy) * g.W;
                for (int kx = 0; kx < 3; ++kx) {
                    const int gx = x - g.pad + kx * g.dil;
                    if ((unsigned)gx >= (unsigned)g.W) continue;
                    const f16x8 h = __builtin_bit_cast(f16x8, in[row + gx]), l = __builtin_bit_cast(f16x8, in[plane_in + row + gx]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float v = (float)h[j] + (float)l[j];
                        if (v > m[j] || v != v) { m[j] = v; bh[j] = h[j]; bl[j] = l[j]; }
                    }
                }
            }
        }
        out[i] = __builtin_bit_cast(uint4, bh);
        out[n + i] = __builtin_bit_cast(uint4, bl);
    }
}

// Mean.  The in-bounds taps are summed in fp32 in window row-major order (the zero padding adds nothing) and the sum is divided by
// the full window, 9 or 27, wherever the window lies: torch's AvgPool with count_include_pad.
__global__ __launch_bounds__(256) void avgpool_pad_kernel(const float* __restrict__ in, float* __restrict__ out, size_t C,
                                                          const PoolGeo g, float div) {
    const size_t n = C * g.Do * g.Ho * g.Wo;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        size_t c; int z, y, x;
        out_coords(i, g, c, z, y, x);
        const float* base = in + c * g.D * g.H * g.W;
        float s = 0.f;
        for (int kz = 0; kz < g.kz; ++kz) {
            const int gz = g.kz > 1 ? z - g.pad + kz * g.dil : 0;
            if ((unsigned)gz >= (unsigned)g.D) continue;
            for (int ky = 0; ky < 3; ++ky) {
                const int gy = y - g.pad + ky * g.dil;
                if ((unsigned)gy >= (unsigned)g.H) continue;
                const float* row = base + ((size_t)gz * g.H + gy) * g.W;
                for (int kx = 0; kx < 3; ++kx) {
                    const int gx = x - g.pad + kx * g.dil;
                    if ((unsigned)gx < (unsigned)g.W) s += row[gx];
                }
            }
        }
        out[i] = s / div;
    }
}

// ... on split cells: each channel's taps joined to fp32 (hi + lo), summed and divided as above, the result split again as
// split_fmt.h forms the halves (hi = f16(v), lo = f16(v - hi)).  A mean of values inside the f16 range stays inside it.
__global__ __launch_bounds__(256) void avgpool_pad_split_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                                size_t cells, const PoolGeo g, float div) {
    const size_t n = cells * g.Do * g.Ho * g.Wo;
    const size_t plane_in = cells * g.D * g.H * g.W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        size_t c; int z, y, x;
        out_coords(i, g, c, z, y, x);
        const size_t base = c * g.D * g.H * g.W;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int kz = 0; kz < g.kz; ++kz) {
            const int gz = g.kz > 1 ? z - g.pad + kz * g.dil : 0;
            if ((unsigned)gz >= (unsigned)g.D) continue;
            for (int ky = 0; ky < 3; ++ky) {
                const int gy = y - g.pad + ky * g.dil;
                if ((unsigned)gy >= (unsigned)g.H) continue;
                const size_t row = base + ((size_t)gz * g.H + gy) * g.W;
                for (int kx = 0; kx < 3; ++kx) {
                    const int gx = x - g.pad + kx * g.dil;
                    if ((unsigned)gx >= (unsigned)g.W) continue;
                    const f16x8 h = __builtin_bit_cast(f16x8, in[row + gx]), l = __builtin_bit_cast(f16x8, in[plane_in + row + gx]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) s[j] += (float)h[j] + (float)l[j];
                }
            }
        }
        const float a[4] = {s[0] / div, s[1] / div, s[2] / div, s[3] / div}, b[4] = {s[4] / div, s[5] / div, s[6] / div, s[7] / div};
        uint2 h0, l0, h1, l1;
        split4(a, h0, l0);
        split4(b, h1, l1);
        out[i] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        out[n + i] = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
}

}  // namespace

// in [C][D][H][W] (split: cells of 8 channels, hi plane then lo plane) -> out [C][Do][Ho][Wo], Xo = X + 2 * pad - 2 * dil.
// The caller has checked 0 <= pad <= dil (the centre tap lies inside the tensor) and that the output is not empty.
hipError_t launch_pool_pad(const void* in, void* out, int C, int D, int H, int W, int dil, int pad, int dims, bool mean, bool split,
                           hipStream_t s) {
    if (pad < 0 || pad > dil || dil < 1) return hipErrorInvalidValue;
    PoolGeo g;
    const int grow = 2 * pad - 2 * dil;
    g.D = dims == 3 ? D : 1; g.H = H; g.W = W;
    g.Do = dims == 3 ? D + grow : 1; g.Ho = H + grow; g.Wo = W + grow;
    g.dil = dil; g.pad = pad; g.kz = dims == 3 ? 3 : 1;
    if (g.Do < 1 || g.Ho < 1 || g.Wo < 1) return hipErrorInvalidValue;
    const size_t cc = split ? split_cells(C) : (size_t)C;
    const size_t n = cc * g.Do * g.Ho * g.Wo;
    if (n == 0) return hipSuccess;
    const int blocks = (int)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535);
    const float div = dims == 3 ? 27.0f : 9.0f;
    if (mean && split)
        hipLaunchKernelGGL(avgpool_pad_split_kernel, dim3(blocks), dim3(256), 0, s, (const uint4*)in, (uint4*)out, cc, g, div);
    else if (mean)
        hipLaunchKernelGGL(avgpool_pad_kernel, dim3(blocks), dim3(256), 0, s, (const float*)in, (float*)out, cc, g, div);
    else if (split)
        hipLaunchKernelGGL(maxpool_pad_split_kernel, dim3(blocks), dim3(256), 0, s, (const uint4*)in, (uint4*)out, cc, g);
    else
        hipLaunchKernelGGL(maxpool_pad_kernel, dim3(blocks), dim3(256), 0, s, (const float*)in, (float*)out, cc, g);
    return hipGetLastError();
}

}  // namespace tpz
