// Particle stacks (topaz particle_stack, topaz/utils/picks.py:71-197): batched crop + standardise of the boxes around the
// picks of one micrograph, and the optional truncated-DFT resize of every frame followed by a second standardisation.
#include "rt_internal.h"

namespace tpz::rt {
namespace {

constexpr int PS_THREADS = 256;     // 4 waves
constexpr int GM_TILE = 64, GM_K = 16;

// sum over the workgroup, in a fixed order (the same value in every thread, independent of the launch)
__device__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                   // red may still be read by the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per particle.  xy != nullptr: the box of size S centred on pick p of the [mz][H][W] image `img`
// (left = x - S/2, upper = y - S/2), written to out[p] ([mz][S][S]); xy == nullptr: out[p] itself is the box (H = W = S),
// standardised in place.  The in-bounds pixels of all mz frames are standardised as numpy evaluates (c - c.mean()) / c.std()
// in float32 (picks.py:148): mean and population std rounded to fp32 -- both sums accumulated in fp64, the variance over the
// fp32 differences x - mean --, then an fp32 subtraction and an IEEE division.  Out-of-image pixels are 0 (picks.py:149-152);
// a box without in-bounds pixels is all zeros, one with zero variance NaN.
__global__ __launch_bounds__(PS_THREADS) void particle_std_kernel(const float* img, int mz, int H, int W, const int* __restrict__ xy,
                                                                   int S, float* out) {
    __shared__ double red[PS_THREADS / 64];
    const int p = blockIdx.x;
    float* dst = out + (size_t)p * mz * S * S;
    const float* src = xy ? img : dst;
    const int left = xy ? xy[2 * p] - S / 2 : 0, upper = xy ? xy[2 * p + 1] - S / 2 : 0;
    const size_t fs = (size_t)H * W;
    const int y0 = max(0, upper), y1 = min(H, upper + S), x0 = max(0, left), x1 = min(W, left + S);
    const int h = max(0, y1 - y0), w = max(0, x1 - x0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long count = (long long)mz * h * w;
    float mean = 0.f, sd = 0.f;
    if (count > 0) {
        double s = 0.0;
        for (int r = wave; r < mz * h; r += PS_THREADS / 64) {
            const float* row = src + (r / h) * fs + (size_t)(y0 + r % h) * W + x0;
            for (int c = lane; c < w; c += 64) s += (double)row[c];
        }
        mean = (float)(block_sum(s, red) / (double)count);
        double q = 0.0;
        for (int r = wave; r < mz * h; r += PS_THREADS / 64) {
            const float* row = src + (r / h) * fs + (size_t)(y0 + r % h) * W + x0;
            for (int c = lane; c < w; c += 64) {
                const double d = (double)__fsub_rn(row[c], mean);
                q = fma(d, d, q);
            }
        }
        sd = (float)sqrt(block_sum(q, red) / (double)count);
    }
    for (int r = wave; r < mz * S; r += PS_THREADS / 64) {
        const int z = r / S, yy = upper + r % S;
        const bool row_in = count > 0 && yy >= 0 && yy < H;
        const float* row = src + z * fs + (size_t)(row_in ? yy : 0) * W;
        float* o = dst + (size_t)r * S;
        for (int c = lane; c < S; c += 64) {
            const int xx = left + c;
            o[c] = row_in && xx >= 0 && xx < W ? __fdiv_rn(__fsub_rn(row[xx], mean), sd) : 0.f;
        }
    }
}

// Batched fp32 GEMM, C[b] (M x N) = A[b] (M x K) . B[b] (K x N), all row-major, with A[b] = A + (b >> a_shift) * a_stride and
// B[b] = B + (b & b_mask) * b_stride, C[b] = C + b * M * N.  64 x 64 tiles, 16-deep K steps through the LDS, 4 x 4 outputs per
// thread; every product is a plain fp32 FMA.  The flat grid walks batch-major: (b, tile row, tile column).
__global__ __launch_bounds__(256) void particle_gemm_kernel(const float* __restrict__ A, long long a_stride, int a_shift,
                                                            const float* __restrict__ B, long long b_stride, unsigned b_mask,
                                                            float* __restrict__ C, int M, int N, int K, int tiles_m, int tiles_n) {
    __shared__ float As[GM_K][GM_TILE + 4];
    __shared__ float Bs[GM_K][GM_TILE + 4];
    const int per_b = tiles_m * tiles_n;
    const int b = blockIdx.x / per_b, t = blockIdx.x % per_b;
    const int m0 = (t / tiles_n) * GM_TILE, n0 = (t % tiles_n) * GM_TILE;
    const float* a = A + (size_t)(b >> a_shift) * a_stride;
    const float* bm = B + (size_t)(b & b_mask) * b_stride;
    float* c = C + (size_t)b * M * N;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += GM_K) {
        for (int l = threadIdx.x; l < GM_TILE * GM_K; l += 256) {
            const int am = l / GM_K, ak = l % GM_K;                      // A: consecutive threads along k
            const int gm = m0 + am, gk = k0 + ak;
            As[ak][am] = gm < M && gk < K ? a[(size_t)gm * K + gk] : 0.f;
            const int bk = l / GM_TILE, bn = l % GM_TILE;                // B: consecutive threads along n
            const int hk = k0 + bk, gn = n0 + bn;
            Bs[bk][bn] = hk < K && gn < N ? bm[(size_t)hk * N + gn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GM_K; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[kk][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Bs[kk][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty + 16 * i;
        if (gm >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx + 16 * j;
            if (gn < N) c[(size_t)gm * N + gn] = acc[i][j];
        }
    }
}

hipError_t launch_particle_gemm(const float* A, long long a_stride, int a_shift, const float* B, long long b_stride, unsigned b_mask,
                                float* C, int batch, int M, int N, int K, hipStream_t s) {
    const int tm = (M + GM_TILE - 1) / GM_TILE, tn = (N + GM_TILE - 1) / GM_TILE;
    hipLaunchKernelGGL(particle_gemm_kernel, dim3((unsigned)batch * tm * tn), dim3(256), 0, s, A, a_stride, a_shift, B, b_stride,
                       b_mask, C, M, N, K, tm, tn);
    return hipGetLastError();
}

}  // namespace
}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_particle_stack(tpz_ctx* ctx, const float* d_img, int mz, int H, int W, const int32_t* h_xy, int n, int size, int resize,
                       const float* h_ops, float* d_out) {
    if (!ctx || !d_img || !h_xy || !d_out || mz < 1 || H < 1 || W < 1 || n < 0 || size < 1)
        return fail(ctx, "tpz_particle_stack: bad arguments");
    const int S = size, R = resize > 0 ? resize : size;
    const bool rs = R != S;
    if (rs && (!h_ops || R > S)) return fail(ctx, "tpz_particle_stack: resize needs the operators and resize <= size");
    if ((long long)mz * S * S >= (1LL << 31) || (long long)n * mz * 2 * (S / GM_TILE + 1) * (R / GM_TILE + 1) >= (1LL << 31))
        return fail(ctx, "tpz_particle_stack: chunk too large (split the picks into smaller chunks)");
    // a box wholly left of / above the image: the reference's negative slice end counts from the far edge and its assignment
    // fails (picks.py:146-152); refused before anything is launched
    for (int i = 0; i < n; ++i) {
        const long long left = (long long)h_xy[2 * i] - S / 2, upper = (long long)h_xy[2 * i + 1] - S / 2;
        if (left + S < 0 || upper + S < 0)
            return fail(ctx, "tpz_particle_stack: pick %d at (%d, %d): the %d-pixel box lies wholly outside the low edge", i,
                        h_xy[2 * i], h_xy[2 * i + 1], S);
    }
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t frame_s = (size_t)S * S, frames = (size_t)n * mz;
    const WorkBuf xy_b(ctx, (size_t)n * 2 * sizeof(int));
    WorkBuf ops_b, crop_b, p_b;
    if (rs) {
        ops_b = WorkBuf(ctx, (size_t)4 * S * R * sizeof(float));
        crop_b = WorkBuf(ctx, frames * frame_s * sizeof(float));
        p_b = WorkBuf(ctx, frames * 2 * S * R * sizeof(float));
    }
    int* d_xy = xy_b.as<int>();
    float *d_ops = ops_b.as<float>(), *d_crop = crop_b.as<float>(), *d_p = p_b.as<float>();
    if (!d_xy || (rs && (!d_ops || !d_crop || !d_p)))
        return fail(ctx, "tpz_particle_stack: out of device memory for %d particles", n);
    hipError_t e = hipMemcpyAsync(d_xy, h_xy, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && rs) e = hipMemcpyAsync(d_ops, h_ops, (size_t)4 * S * R * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    // 1. crop + standardise: reads the in-bounds boxes twice and writes them once
    float* boxes = rs ? d_crop : d_out;
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 0.0, "particle_crop_std", 4.0 * frames * frame_s * 2, [&](hipStream_t s) {
            hipLaunchKernelGGL(particle_std_kernel, dim3(n), dim3(PS_THREADS), 0, s, d_img, mz, H, W, d_xy, S, boxes);
            return hipGetLastError();
        });
    if (e == hipSuccess && rs) {
        // 2. P = X . [R1 | R2] per frame, stored [2][S][R] (h_ops: [2][S][R] column operators, then the [R][2S] row operator
        //    [Re Lc | Im Lc]); 3. y = [Re Lc | Im Lc] . [P1; P2]: the separable truncated DFT of topaz_amd/utils/image.py
        const double f1 = 2.0 * 2 * frames * S * S * R, f2 = 2.0 * frames * R * 2 * S * R;
        e = enqueue(ctx, 2, f1, "particle_resize_cols", 4.0 * frames * (frame_s + 2.0 * S * R), [&](hipStream_t s) {
            return launch_particle_gemm(d_crop, (long long)frame_s, 1, d_ops, (long long)S * R, 1u, d_p, (int)(2 * frames), S, R, S, s);
        });
        if (e == hipSuccess)
            e = enqueue(ctx, 2, f2, "particle_resize_rows", 4.0 * frames * (2.0 * S * R + (double)R * R), [&](hipStream_t s) {
                return launch_particle_gemm(d_ops + 2 * (size_t)S * R, 0, 0, d_p, 2LL * S * R, ~0u, d_out, (int)frames, R, R, 2 * S, s);
            });
        // 4. re-standardise each particle over its mz * R * R pixels (picks.py:158), in place
        if (e == hipSuccess)
            e = enqueue(ctx, 2, 0.0, "particle_restd", 4.0 * frames * R * R * 3, [&](hipStream_t s) {
                hipLaunchKernelGGL(particle_std_kernel, dim3(n), dim3(PS_THREADS), 0, s, (const float*)d_out, mz, R, R, (const int*)nullptr,
                                   R, d_out);
                return hipGetLastError();
            });
    }
    HIPCHK(ctx, e);
    return 0;
}
