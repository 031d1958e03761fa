// Pre-filters of `topaz denoise` (topaz/denoise.py:382-416): the hard low-pass (`--lowpass F`, denoise.py:174-197) as four fp64
// GEMMs with the separable projection operators, and the covariance deconvolution (`--deconvolve [--deconv-patch P]`,
// denoise.py:22-75, 129-172): lag covariances of all tiles, then one zero-padded filter over the whole image with per-tile
// weights.  The launch count of every entry point is independent of the image size and of P.
#include "rt_internal.h"

namespace tpz::rt {
namespace {

constexpr int LP_TILE = 64, LP_K = 16;
constexpr int CV_THREADS = 256, CV_ROWS = 8;   // covariance partials: rows of the tile centre per workgroup
constexpr int CV_WIDTH = 11;                   // the reference's filter width (correct_spatial_covariance(width=11))
constexpr int CV_LAGS = CV_WIDTH * CV_WIDTH;
constexpr int TF_TILE = 16;                    // tiled filter: 16 x 16 outputs per workgroup

// C (M x N, row-major, leading dimension N) = A (M x K) . B (K x N) with A(m, k) = A[m * a_rs + k * a_cs] and
// B(k, n) = B[k * b_rs + n * b_cs] (either operand may be a transposed view).  Operands are widened to fp64 as they enter the
// LDS, every product is an fp64 FMA and C is rounded to TC once.  64 x 64 tiles, 16-deep K steps, 4 x 4 outputs per thread.
template <class TA, class TB, class TC>
__global__ __launch_bounds__(256) void lp_gemm_kernel(const TA* __restrict__ A, long long a_rs, long long a_cs,
                                                      const TB* __restrict__ B, long long b_rs, long long b_cs,
                                                      TC* __restrict__ C, int M, int N, int K, int tiles_n) {
    __shared__ double As[LP_K][LP_TILE + 1];
    __shared__ double Bs[LP_K][LP_TILE + 1];
    const int m0 = (blockIdx.x / tiles_n) * LP_TILE, n0 = (blockIdx.x % tiles_n) * LP_TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const bool a_k_fast = a_cs == 1, b_n_fast = b_cs == 1;     // consecutive threads along the contiguous index
    double acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += LP_K) {
        for (int l = threadIdx.x; l < LP_TILE * LP_K; l += 256) {
            const int am = a_k_fast ? l / LP_K : l % LP_TILE, ak = a_k_fast ? l % LP_K : l / LP_TILE;
            const int gm = m0 + am, gk = k0 + ak;
            As[ak][am] = gm < M && gk < K ? (double)A[(size_t)gm * a_rs + (size_t)gk * a_cs] : 0.0;
            const int bn = b_n_fast ? l % LP_TILE : l / LP_K, bk = b_n_fast ? l / LP_TILE : l % LP_K;
            const int hk = k0 + bk, gn = n0 + bn;
            Bs[bk][bn] = hk < K && gn < N ? (double)B[(size_t)hk * b_rs + (size_t)gn * b_cs] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < LP_K; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[kk][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Bs[kk][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
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
            if (gn < N) C[(size_t)gm * N + gn] = (TC)acc[i][j];
        }
    }
}

template <class TA, class TB, class TC>
hipError_t launch_lp_gemm(const TA* A, long long a_rs, long long a_cs, const TB* B, long long b_rs, long long b_cs, TC* C, int M,
                          int N, int K, hipStream_t s) {
    const int tm = (M + LP_TILE - 1) / LP_TILE, tn = (N + LP_TILE - 1) / LP_TILE;
    hipLaunchKernelGGL((lp_gemm_kernel<TA, TB, TC>), dim3((unsigned)tm * tn), dim3(256), 0, s, A, a_rs, a_cs, B, b_rs, b_cs, C, M, N,
                       K, tn);
    return hipGetLastError();
}

// Tile t of P along an axis of length n (correct_spatial_covariance, denoise.py:137-142): the first n % P tiles are one longer.
struct Span {
    int start, len;
};
__host__ __device__ inline Span tile_span(int n, int P, int t) {
    const int q = n / P, r = n % P;
    return {t * q + (t < r ? t : r), q + (t < r ? 1 : 0)};
}
// the tile a coordinate belongs to
__device__ inline int tile_of(int v, int n, int P) {
    const int q = n / P, r = n % P, big = r * (q + 1);
    return v < big ? v / (q + 1) : r + (v - big) / q;
}
// the tile extended by the halo p, clipped to [0, n) (denoise.py:150-154)
__host__ __device__ inline Span halo_span(int n, int P, int t, int p) {
    const Span s = tile_span(n, P, t);
    const int a = s.start - p > 0 ? s.start - p : 0, b = s.start + s.len + p < n ? s.start + s.len + p : n;
    return {a, b - a};
}

// One workgroup per (tile, block of CV_ROWS rows of the tile centre x_c = xt[p:-p, p:-p]) of the halo'd tile xt: the partial
// sums over those rows of all 121 lags, cov[a][b] = sum_ij xt[a + i][b + j] * xt[p + i][p + j] (spatial_covariance, denoise.py:45-46:
// a valid cross-correlation of xt with x_c).  fp32 products are exact in fp64 and are accumulated in fp64; the order is fixed by
// the launch geometry, which depends on (H, W, P) only.  part: [P * P * nrb][121].
__global__ __launch_bounds__(CV_THREADS) void cov_partial_kernel(const float* __restrict__ x, int H, int W, int P, int nrb,
                                                                 double* __restrict__ part) {
    __shared__ double red[CV_THREADS / 64][CV_WIDTH];
    constexpr int p = CV_WIDTH / 2;
    const int tile = blockIdx.x / nrb, rb = blockIdx.x % nrb;
    const Span ry = halo_span(H, P, tile / P, p), rx = halo_span(W, P, tile % P, p);
    const int ch = ry.len - 2 * p, cw = rx.len - 2 * p;
    const int i0 = rb * CV_ROWS, i1 = min(ch, i0 + CV_ROWS);
    const float* xt = x + (size_t)ry.start * W + rx.start;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* out = part + (size_t)blockIdx.x * CV_LAGS;
    for (int a = 0; a < CV_WIDTH; ++a) {
        double acc[CV_WIDTH];
#pragma unroll
        for (int b = 0; b < CV_WIDTH; ++b) acc[b] = 0.0;
        for (int i = i0; i < i1; ++i) {
            const float* rc = xt + (size_t)(i + p) * W + p;      // row i of x_c
            const float* rl = xt + (size_t)(i + a) * W;          // row i + a of xt
            for (int j = threadIdx.x; j < cw; j += CV_THREADS) {
                const double c = (double)rc[j];
#pragma unroll
                for (int b = 0; b < CV_WIDTH; ++b) acc[b] = fma((double)rl[j + b], c, acc[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < CV_WIDTH; ++b) {
            double v = acc[b];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) red[wave][b] = v;
        }
        __syncthreads();
        if (threadIdx.x < CV_WIDTH)
            out[a * CV_WIDTH + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        __syncthreads();
    }
}

// cov[t][lag] = (sum over the row blocks of tile t, in block order) / |x_c| (denoise.py:47)
__global__ __launch_bounds__(256) void cov_reduce_kernel(const double* __restrict__ part, int H, int W, int P, int nrb,
                                                         double* __restrict__ cov) {
    constexpr int p = CV_WIDTH / 2;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P * P * CV_LAGS) return;
    const int tile = g / CV_LAGS, lag = g % CV_LAGS;
    const Span ry = halo_span(H, P, tile / P, p), rx = halo_span(W, P, tile % P, p);
    const double* src = part + (size_t)tile * nrb * CV_LAGS + lag;
    double s = 0.0;
    for (int r = 0; r < nrb; ++r) s += src[(size_t)r * CV_LAGS];
    cov[g] = s / ((double)(ry.len - 2 * p) * (double)(rx.len - 2 * p));
}

// y[i][j] = sum_ab w_t[a][b] * x[i + a - p][j + b - p], zero outside the image, w_t the fp32 weights of the tile that holds (i, j):
// AffineFilter (filters.py:28-37, Conv2d with padding p, bias 0) on each halo'd tile, keeping its centre (denoise.py:156-158) --
// the halo makes every kept pixel see its true neighbours or the image's zero padding.  fp64 accumulation, one rounding.
__global__ __launch_bounds__(TF_TILE * TF_TILE) void tile_filter_kernel(const float* __restrict__ x, int H, int W, int P,
                                                                        const float* __restrict__ w, float* __restrict__ y) {
    constexpr int p = CV_WIDTH / 2, S = TF_TILE + 2 * p;
    __shared__ float xs[S][S + 1];
    const int by = blockIdx.y * TF_TILE, bx = blockIdx.x * TF_TILE;
    for (int l = threadIdx.x; l < S * S; l += TF_TILE * TF_TILE) {
        const int yy = by - p + l / S, xx = bx - p + l % S;
        xs[l / S][l % S] = yy >= 0 && yy < H && xx >= 0 && xx < W ? x[(size_t)yy * W + xx] : 0.f;
    }
    __syncthreads();
    const int ly = threadIdx.x / TF_TILE, lx = threadIdx.x % TF_TILE;
    const int gy = by + ly, gx = bx + lx;
    if (gy >= H || gx >= W) return;
    const float* wt = w + (size_t)(tile_of(gy, H, P) * P + tile_of(gx, W, P)) * CV_LAGS;
    double acc = 0.0;
    for (int a = 0; a < CV_WIDTH; ++a)
#pragma unroll
        for (int b = 0; b < CV_WIDTH; ++b) acc = fma((double)wt[a * CV_WIDTH + b], (double)xs[ly + a][lx + b], acc);
    y[(size_t)gy * W + gx] = (float)acc;
}

// the reference fails inside conv2d when a halo'd tile is narrower than the filter; refused here before anything runs
int check_tiles(tpz_ctx* ctx, const char* fn, int H, int W, int P, int width) {
    if (width != CV_WIDTH) return fail(ctx, "%s: width %d (only the reference's width %d is implemented)", fn, width, CV_WIDTH);
    if (P < 1) return fail(ctx, "%s: patch count %d < 1", fn, P);
    for (int t = 0; t < P; ++t) {
        const Span ry = halo_span(H, P, t, width / 2), rx = halo_span(W, P, t, width / 2);
        if (ry.len < width || rx.len < width)
            return fail(ctx, "%s: the %d x %d image in %d x %d tiles gives a %d x %d halo'd tile, smaller than the %d x %d filter", fn,
                        H, W, P, P, ry.len, rx.len, width, width);
    }
    return 0;
}

}  // namespace
}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_lowpass_2d(tpz_ctx* ctx, const float* d_in, int H, int W, const double* h_qh, int rh, const double* h_qw, int rw,
                   float* d_out) {
    if (!ctx || !d_in || !h_qh || !h_qw || !d_out || H < 1 || W < 1 || rh < 1 || rw < 1 || rh > H || rw > W)
        return fail(ctx, "tpz_lowpass_2d: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nqh = (size_t)H * rh, nqw = (size_t)W * rw;
    const WorkBuf qh_b(ctx, nqh * sizeof(double)), qw_b(ctx, nqw * sizeof(double)), t1_b(ctx, (size_t)rh * W * sizeof(double)),
        t2_b(ctx, (size_t)rh * rw * sizeof(double)), t3_b(ctx, (size_t)H * rw * sizeof(double));
    double *d_qh = qh_b.as<double>(), *d_qw = qw_b.as<double>(), *d_t1 = t1_b.as<double>(), *d_t2 = t2_b.as<double>(),
           *d_t3 = t3_b.as<double>();
    if (!d_qh || !d_qw || !d_t1 || !d_t2 || !d_t3)
        return fail(ctx, "tpz_lowpass_2d: out of device memory for a %d x %d image", H, W);
    hipError_t e = hipMemcpyAsync(d_qh, h_qh, nqh * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qw, h_qw, nqw * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    // y = Qh (Qh^T x Qw) Qw^T: 1. T1 = Qh^T x  2. T2 = T1 Qw  3. T3 = Qh T2  4. y = T3 Qw^T (rounded to fp32)
    const double h = H, w = W;
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 2.0 * rh * h * w, "lowpass_gemm", 8.0 * (nqh + (double)rh * w) + 4.0 * h * w, [&](hipStream_t s) {
            return launch_lp_gemm(d_qh, 1, rh, d_in, W, 1, d_t1, rh, W, H, s);
        });
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 2.0 * rh * w * rw, "lowpass_gemm", 8.0 * ((double)rh * w + nqw + (double)rh * rw), [&](hipStream_t s) {
            return launch_lp_gemm((const double*)d_t1, W, 1, (const double*)d_qw, rw, 1, d_t2, rh, rw, W, s);
        });
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 2.0 * h * rh * rw, "lowpass_gemm", 8.0 * (nqh + (double)rh * rw + h * rw), [&](hipStream_t s) {
            return launch_lp_gemm((const double*)d_qh, rh, 1, (const double*)d_t2, rw, 1, d_t3, H, rw, rh, s);
        });
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 2.0 * h * rw * w, "lowpass_gemm", 8.0 * (h * rw + nqw) + 4.0 * h * w, [&](hipStream_t s) {
            return launch_lp_gemm((const double*)d_t3, rw, 1, (const double*)d_qw, 1, rw, d_out, H, W, rw, s);
        });
    HIPCHK(ctx, e);
    return 0;
}

int tpz_spatial_cov_2d(tpz_ctx* ctx, const float* d_x, int H, int W, int P, int width, double* h_cov) {
    if (!ctx || !d_x || !h_cov || H < 1 || W < 1) return fail(ctx, "tpz_spatial_cov_2d: bad arguments");
    if (int rc = check_tiles(ctx, "tpz_spatial_cov_2d", H, W, P, width)) return rc;
    if ((long long)P * P * CV_LAGS >= (1LL << 31)) return fail(ctx, "tpz_spatial_cov_2d: too many tiles (%d)", P);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // row blocks per tile: enough for the tallest tile centre; blocks past a shorter centre write zeros
    int ch_max = 0;
    for (int t = 0; t < P; ++t) ch_max = std::max(ch_max, halo_span(H, P, t, width / 2).len - 2 * (width / 2));
    const int nrb = (ch_max + CV_ROWS - 1) / CV_ROWS;
    const long long nblk = (long long)P * P * nrb;
    if (nblk >= (1LL << 31)) return fail(ctx, "tpz_spatial_cov_2d: image too large");
    const WorkBuf part_b(ctx, (size_t)nblk * CV_LAGS * sizeof(double)), cov_b(ctx, (size_t)P * P * CV_LAGS * sizeof(double));
    double *d_part = part_b.as<double>(), *d_cov = cov_b.as<double>();
    if (!d_part || !d_cov) return fail(ctx, "tpz_spatial_cov_2d: out of device memory");
    hipError_t e = enqueue(ctx, 2, 2.0 * CV_LAGS * H * W, "spatial_cov_partial", 4.0 * H * W, [&](hipStream_t s) {
        hipLaunchKernelGGL(cov_partial_kernel, dim3((unsigned)nblk), dim3(CV_THREADS), 0, s, d_x, H, W, P, nrb, d_part);
        return hipGetLastError();
    });
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 0.0, "spatial_cov_reduce", 8.0 * nblk * CV_LAGS, [&](hipStream_t s) {
            hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)((P * P * CV_LAGS + 255) / 256)), dim3(256), 0, s, (const double*)d_part,
                               H, W, P, nrb, d_cov);
            return hipGetLastError();
        });
    if (e == hipSuccess) e = hipMemcpyAsync(h_cov, d_cov, (size_t)P * P * CV_LAGS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    HIPCHK(ctx, e);
    return 0;
}

int tpz_tile_filter_2d(tpz_ctx* ctx, const float* d_x, int H, int W, int P, int width, const float* h_w, float* d_out) {
    if (!ctx || !d_x || !h_w || !d_out || H < 1 || W < 1) return fail(ctx, "tpz_tile_filter_2d: bad arguments");
    if (int rc = check_tiles(ctx, "tpz_tile_filter_2d", H, W, P, width)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nw = (size_t)P * P * CV_LAGS;
    const WorkBuf w_b(ctx, nw * sizeof(float));
    float* d_w = w_b.as<float>();
    if (!d_w) return fail(ctx, "tpz_tile_filter_2d: out of device memory");
    hipError_t e = hipMemcpyAsync(d_w, h_w, nw * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 2.0 * CV_LAGS * H * W, "tile_filter", 8.0 * H * W, [&](hipStream_t s) {
            const dim3 grid((unsigned)((W + TF_TILE - 1) / TF_TILE), (unsigned)((H + TF_TILE - 1) / TF_TILE));
            hipLaunchKernelGGL(tile_filter_kernel, grid, dim3(TF_TILE * TF_TILE), 0, s, d_x, H, W, P, (const float*)d_w, d_out);
            return hipGetLastError();
        });
    HIPCHK(ctx, e);
    return 0;
}
