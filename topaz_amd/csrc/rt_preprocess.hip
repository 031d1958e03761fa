// Device side of the `topaz preprocess` / `topaz normalize` stream (topaz_amd/stats.py normalize_device): exact order
// statistics by radix select, a gather of sampled pixels, the mixture fit with every initialisation advanced by ONE pass over
// the pixels per EM iteration, and the float64 (x - mu) / std.  The kernels live here with their entry points.
#include "rt_internal.h"

namespace tpz::rt {
namespace {

// ------------------------------------------------------------------------------------------
// Order statistics: the ranks[j]-th smallest of n floats, exactly, for up to OS_MAX_RANKS ranks at once.
// Radix select on the order-preserving 32-bit key of a float (all bits of a negative flipped, the sign bit of the rest), four
// digits of 8 bits from the top.  One launch per digit: every workgroup counts into an LDS histogram [prefix][256] (32 prefixes
// x 256 bins x 4 B = 32 KB) and merges it into the global one with 64-bit integer atomics -- integer sums, so the counts do not
// depend on the schedule.  The first digit has one histogram shared by all ranks; a later digit counts only the elements whose
// higher bits equal one of the (distinct) prefixes the host found for the ranks.  NaNs are counted alongside the first digit.
// ------------------------------------------------------------------------------------------
enum { OS_MAX_RANKS = 32, OS_BINS = 256, OS_BLOCKS = 1024 };

struct OsPrefixes {
    unsigned v[OS_MAX_RANKS];      // the key bits above this digit, right-aligned, one per distinct prefix
    int n;                         // prefixes in use (1 for the first digit)
    int shift;                     // bit position of this digit: 24, 16, 8, 0
};

__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

float key_value(unsigned key) {
    const unsigned u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}

// hist[0] = number of NaNs (first digit only), hist[1 + p * 256 + d] = elements under prefix p whose digit is d
__global__ __launch_bounds__(256) void order_hist_kernel(const float* __restrict__ x, size_t n, OsPrefixes P,
                                                         unsigned long long* __restrict__ hist) {
    __shared__ unsigned sh[OS_MAX_RANKS * OS_BINS];
    __shared__ unsigned sh_nan;
    const int cells = P.n * OS_BINS;
    for (int i = threadIdx.x; i < cells; i += 256) sh[i] = 0;
    if (threadIdx.x == 0) sh_nan = 0;
    __syncthreads();
    const int shift = P.shift;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float f = x[i];
        const unsigned key = order_key(f);
        const unsigned digit = (key >> shift) & 0xFFu;
        if (shift == 24) {
            atomicAdd(&sh[digit], 1u);
            if (f != f) atomicAdd(&sh_nan, 1u);
        } else {
            const unsigned hi = key >> (shift + 8);
            for (int p = 0; p < P.n; ++p)
                if (P.v[p] == hi) { atomicAdd(&sh[p * OS_BINS + digit], 1u); break; }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 256) {
        const unsigned c = sh[i];
        if (c) atomicAdd(&hist[1 + i], (unsigned long long)c);
    }
    if (threadIdx.x == 0 && sh_nan) atomicAdd(&hist[0], (unsigned long long)sh_nan);
}

// ------------------------------------------------------------------------------------------
// out[i] = x[idx[i]]
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ x, const long long* __restrict__ idx, size_t m,
                                                     float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (size_t)gridDim.x * 256) out[i] = x[idx[i]];
}

// ------------------------------------------------------------------------------------------
// y = (float)(((double)x - mean) / std): numpy's `(x - mu) / std` for a float32 image and np.float64 scalars
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normalize_f64_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n,
                                                            double mu, double sd) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        y[i] = (float)(((double)x[i] - mu) / sd);
}

// ------------------------------------------------------------------------------------------
// One pass of the mixture fit for up to GMM_G initialisations at once: gmm_pass_kernel (kernels_misc.hip) with the element
// loop's body repeated per initialisation, so x is read once per pass instead of once per initialisation.  For every
// initialisation the sums are formed in the order of gmm_pass_kernel + gmm_final_kernel -- the same grid (launch_gmm_pass's
// block count), the same grid stride, so each thread adds the same elements in the same sequence, the same expressions per
// element, wave_sum, the sum of the four waves' partials left to right, then a serial sum over the blocks -- which makes the
// fp64 results equal bit for bit, not merely close.
// par[j] = {split | mu0, mu1, var0, var1, ln(1-pi), ln(pi)} of initialisation j, all of them in the same mode.
// ------------------------------------------------------------------------------------------
enum { GMM_G = 11, GMM_BLOCKS = 256 };

struct GmmGroupPar {
    double p[GMM_G][6];
    int n;                        // initialisations in this launch (<= GMM_G)
    int mode;
};

__global__ __launch_bounds__(256) void gmm_fused_pass_kernel(const float* __restrict__ x, size_t n, GmmGroupPar P,
                                                             double* __restrict__ part) {
    __shared__ double sh[4][GMM_G * 7];
    double acc[GMM_G][7];
    double c0[GMM_G], c1[GMM_G];
    const int mode = P.mode;
#pragma unroll
    for (int j = 0; j < GMM_G; ++j) {
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[j][k] = 0;
        const double p2_ = P.p[j][2], p3_ = P.p[j][3], p4_ = P.p[j][4], p5_ = P.p[j][5];
        c0[j] = mode ? -0.5 * log(2.0 * 3.14159265358979323846 * p2_) + p4_ : 0.0;
        c1[j] = mode ? -0.5 * log(2.0 * 3.14159265358979323846 * p3_) + p5_ : 0.0;
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double v = (double)x[i];
#pragma unroll
        for (int j = 0; j < GMM_G; ++j) {
            if (j < P.n) {
                const double p0_ = P.p[j][0], p1_ = P.p[j][1], p2_ = P.p[j][2], p3_ = P.p[j][3];
                double q0, q1, Z = 0.0;
                if (mode == 0) {
                    q0 = v <= p0_ ? 1.0 : 0.0;
                    q1 = 1.0 - q0;
                } else {
                    const double l0 = -(v - p0_) * (v - p0_) / 2.0 / p2_ + c0[j];
                    const double l1 = -(v - p1_) * (v - p1_) / 2.0 / p3_ + c1[j];
                    const double ma = l0 > l1 ? l0 : l1;
                    Z = ma + log(exp(l0 - ma) + exp(l1 - ma));
                    q0 = exp(l0 - Z);
                    q1 = exp(l1 - Z);
                }
                acc[j][0] += Z; acc[j][1] += q0; acc[j][2] += q1;
                acc[j][3] += q0 * v; acc[j][4] += q1 * v;
                acc[j][5] += q0 * v * v; acc[j][6] += q1 * v * v;
            }
        }
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < GMM_G; ++j) {
        if (j < P.n) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const double s = wave_sum(acc[j][k]);
                if ((threadIdx.x & 63) == 0) sh[wv][j * 7 + k] = s;
            }
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < P.n * 7) part[(size_t)blockIdx.x * (GMM_G * 7) + t] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
}

// out[j * 7 + k] = the partials of the blocks summed in block order (gmm_final_kernel)
__global__ void gmm_fused_final_kernel(const double* __restrict__ part, int blocks, int n_init, double* __restrict__ out) {
    const int t = threadIdx.x;
    if (t < n_init * 7) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += part[(size_t)b * (GMM_G * 7) + t];
        out[t] = s;
    }
}

int grid_1d(size_t n, int cap) {
    const size_t b = (n + 255) / 256;
    return (int)(b < (size_t)cap ? (b < 1 ? 1 : b) : (size_t)cap);
}

}  // namespace
}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_order_stats(tpz_ctx* ctx, const float* d_x, size_t n, const long long* h_ranks, int k, float* h_out) {
    if (!ctx || !d_x || !h_ranks || !h_out || n == 0 || k < 1 || k > OS_MAX_RANKS || n > ((size_t)1 << 40))
        return fail(ctx, "tpz_order_stats: bad arguments (1 <= k <= %d ranks, 1 <= n <= 2^40)", (int)OS_MAX_RANKS);
    for (int j = 0; j < k; ++j)
        if (h_ranks[j] < 0 || (unsigned long long)h_ranks[j] >= n)
            return fail(ctx, "tpz_order_stats: rank %lld is outside [0, %zu)", h_ranks[j], n);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t hist_words = 1 + (size_t)OS_MAX_RANKS * OS_BINS;
    const WorkBuf hist_b(ctx, hist_words * sizeof(unsigned long long));
    unsigned long long* d_hist = hist_b.as<unsigned long long>();
    if (!d_hist) return fail(ctx, "tpz_order_stats: workspace allocation failed");
    std::vector<unsigned long long> h(hist_words);
    unsigned prefix[OS_MAX_RANKS];
    unsigned long long rem[OS_MAX_RANKS];
    int slot[OS_MAX_RANKS];
    for (int j = 0; j < k; ++j) { prefix[j] = 0; rem[j] = (unsigned long long)h_ranks[j]; }
    const int blocks = grid_1d(n, OS_BLOCKS);
    hipError_t e = hipSuccess;
    bool has_nan = false;
    for (int level = 0; level < 4 && e == hipSuccess && !has_nan; ++level) {
        OsPrefixes P;
        memset(&P, 0, sizeof(P));
        P.shift = 24 - 8 * level;
        for (int j = 0; j < k; ++j) {                    // the distinct prefixes of the ranks (all ranks share the first digit)
            int s = 0;
            while (s < P.n && P.v[s] != prefix[j]) ++s;
            if (s == P.n) P.v[P.n++] = prefix[j];
            slot[j] = s;
        }
        const size_t words = 1 + (size_t)P.n * OS_BINS;
        e = hipMemsetAsync(d_hist, 0, words * sizeof(unsigned long long), ctx->stream);
        if (e != hipSuccess) break;
        prof_begin(ctx, 2, 0);
        hipLaunchKernelGGL(order_hist_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_x, n, P, d_hist);
        e = hipGetLastError();
        prof_end(ctx);
        if (e != hipSuccess) break;
        e = hipMemcpyAsync(h.data(), d_hist, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) break;
        if (level == 0 && h[0] > 0) { has_nan = true; break; }
        for (int j = 0; j < k; ++j) {
            const unsigned long long* bins = h.data() + 1 + (size_t)slot[j] * OS_BINS;
            int b = 0;
            while (b < OS_BINS - 1 && rem[j] >= bins[b]) rem[j] -= bins[b++];
            prefix[j] = (prefix[j] << 8) | (unsigned)b;
        }
    }
    HIPCHK(ctx, e);
    for (int j = 0; j < k; ++j) h_out[j] = has_nan ? NAN : key_value(prefix[j]);
    return 0;
}

int tpz_gather_f32(tpz_ctx* ctx, const float* d_x, size_t n, const long long* h_idx, size_t m, float* d_out) {
    if (!ctx || !d_x || (m && (!h_idx || !d_out))) return fail(ctx, "tpz_gather_f32: bad arguments");
    for (size_t i = 0; i < m; ++i)
        if (h_idx[i] < 0 || (unsigned long long)h_idx[i] >= n)
            return fail(ctx, "tpz_gather_f32: index %lld (position %zu) is outside [0, %zu)", h_idx[i], i, n);
    if (m == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (the index buffer goes back to the pool of this stream: whatever takes it next is queued behind the gather)
    const WorkBuf idx_b(ctx, m * sizeof(long long));
    long long* d_idx = idx_b.as<long long>();
    if (!d_idx) return fail(ctx, "tpz_gather_f32: workspace allocation failed");
    hipError_t e = hipMemcpyAsync(d_idx, h_idx, m * sizeof(long long), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        prof_begin(ctx, 2, 0);
        hipLaunchKernelGGL(gather_kernel, dim3(grid_1d(m, 8192)), dim3(256), 0, ctx->stream, d_x, d_idx, m, d_out);
        e = hipGetLastError();
        prof_end(ctx);
    }
    HIPCHK(ctx, e);
    return 0;
}

int tpz_normalize_f64(tpz_ctx* ctx, const float* d_x, size_t n, double mean, double std, float* d_y) {
    if (!ctx || !d_x || !d_y) return fail(ctx, "tpz_normalize_f64: bad arguments");
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    prof_begin(ctx, 2, 0);
    hipLaunchKernelGGL(normalize_f64_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, ctx->stream, d_x, d_y, n, mean, std);
    const hipError_t e = hipGetLastError();
    prof_end(ctx);
    HIPCHK(ctx, e);
    return 0;
}

// tpz_gmm_fit (rt_stats.hip) with the initialisations advanced together: pass 1 the global moments (the very launch of
// tpz_gmm_fit), pass 2 the hard split of every two-component initialisation, pass 3 their first E-step, then one pass per EM
// iteration over those that have not converged.  The scalar steps between the passes are the functions tpz_gmm_fit calls.
int tpz_gmm_fit_fused(tpz_ctx* ctx, const float* d_x, size_t n, const double* pis, const double* splits, int n_init,
                      double alpha, double beta, double scale, int num_iters, double tol, double* mus, double* stds,
                      double* pis_out, double* logps, int* n_passes) {
    if (!ctx || !d_x || !pis || !splits || !mus || !stds || !pis_out || !logps || n < 2 || n_init < 1)
        return fail(ctx, "tpz_gmm_fit_fused: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_passes) *n_passes = 0;
    struct Fit {
        int i;
        double pi, mu0, mu1, var, logp, logp_cur;
        int it;
    };
    std::vector<Fit> fits;
    for (int i = 0; i < n_init; ++i)
        if (pis[i] != 1.0) fits.push_back(Fit{i, pis[i], 0, 0, 0, 0, 0, 0});
    const int blocks = grid_1d(n, GMM_BLOCKS);
    const size_t n_groups = (fits.size() + GMM_G - 1) / GMM_G;
    const size_t part_words = std::max<size_t>(n_groups, 1) * GMM_BLOCKS * GMM_G * 7, out_words = std::max<size_t>(fits.size(), 1) * 7;
    const WorkBuf buf_b(ctx, (part_words + out_words + 8) * sizeof(double));
    double* d_buf = buf_b.as<double>();
    if (!d_buf) return fail(ctx, "tpz_gmm_fit_fused: workspace allocation failed");
    double *d_part = d_buf, *d_out = d_buf + part_words, *d_par = d_out + out_words;
    std::vector<double> S(out_words);
    int passes = 0;
    const double N = (double)n;

    // global moments: the hard pass of tpz_gmm_fit with split = +inf
    double S0[7];
    hipError_t e;
    {
        const double par[6] = {INFINITY, 0, 0, 0, 0, 0};
        e = hipMemcpyAsync(d_par, par, sizeof(par), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            prof_begin(ctx, 2, 0);
            e = launch_gmm_pass(d_x, n, 0, d_par, ctx->d_part, 256, d_out, ctx->stream);
            prof_end(ctx);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(S0, d_out, sizeof(S0), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        ++passes;
    }
    // one pass over x for the fits listed in `act`: S[a * 7 ..] receives the sums of act[a]
    auto pass = [&](const std::vector<int>& act, const std::vector<GmmGroupPar>& groups) -> hipError_t {
        prof_begin(ctx, 2, 0);
        for (size_t g = 0; g < groups.size(); ++g) {
            double* part = d_part + g * GMM_BLOCKS * GMM_G * 7;
            hipLaunchKernelGGL(gmm_fused_pass_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_x, n, groups[g], part);
            hipLaunchKernelGGL(gmm_fused_final_kernel, dim3(1), dim3(128), 0, ctx->stream, part, blocks, groups[g].n,
                               d_out + g * GMM_G * 7);
        }
        hipError_t err = hipGetLastError();
        prof_end(ctx);
        if (err != hipSuccess) return err;
        err = hipMemcpyAsync(S.data(), d_out, act.size() * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (err != hipSuccess) return err;
        ++passes;
        return hipStreamSynchronize(ctx->stream);
    };
    auto pack = [&](int mode, const std::vector<int>& act, const std::function<void(const Fit&, double (&)[6])>& fill) {
        std::vector<GmmGroupPar> groups((act.size() + GMM_G - 1) / GMM_G);
        for (auto& g : groups) { memset(&g, 0, sizeof(g)); g.mode = mode; }
        for (size_t a = 0; a < act.size(); ++a) {
            GmmGroupPar& g = groups[a / GMM_G];
            fill(fits[act[a]], g.p[g.n++]);
        }
        return groups;
    };
    if (e == hipSuccess) {
        const GmmMoments M = gmm_moments(S0, N);
        for (int i = 0; i < n_init; ++i)
            if (pis[i] == 1.0) gmm_single_component(M, N, alpha, beta, scale, logps[i], mus[i], stds[i], pis_out[i]);
        std::vector<int> act(fits.size());
        for (size_t a = 0; a < act.size(); ++a) act[a] = (int)a;
        if (!act.empty()) {
            // hard split, then the M-step from it
            e = pass(act, pack(0, act, [&](const Fit& f, double (&par)[6]) {
                         par[0] = splits[f.i]; par[1] = par[2] = par[3] = par[4] = par[5] = 0; }));
            for (size_t a = 0; a < act.size() && e == hipSuccess; ++a) {
                Fit& f = fits[act[a]];
                gmm_m_step(&S[a * 7], N, M.mu_all, f.mu0, f.mu1, f.var);
            }
            // first E-step
            if (e == hipSuccess)
                e = pass(act, pack(1, act, [&](const Fit& f, double (&par)[6]) { gmm_e_step_par(f.mu0, f.mu1, f.var, f.pi, par); }));
            std::vector<double> T(S);      // the sums of the last E-step per fit, by position in `fits`
            for (size_t a = 0; a < act.size() && e == hipSuccess; ++a) {
                Fit& f = fits[act[a]];
                f.logp = scale * S[a * 7] + beta_logpdf(f.pi, alpha, beta);
                f.logp_cur = f.logp;
                f.it = 1;
            }
            if (num_iters < 1) act.clear();
            while (!act.empty() && e == hipSuccess) {
                // M-step from the assignments of the last E-step, MAP estimate of pi under the Beta prior; next E-step
                for (int a : act) {
                    Fit& f = fits[a];
                    f.pi = gmm_map_pi(&T[(size_t)a * 7], N, alpha, beta);
                    gmm_m_step(&T[(size_t)a * 7], N, M.mu_all, f.mu0, f.mu1, f.var);
                }
                e = pass(act, pack(1, act, [&](const Fit& f, double (&par)[6]) { gmm_e_step_par(f.mu0, f.mu1, f.var, f.pi, par); }));
                if (e != hipSuccess) break;
                std::vector<int> next;
                for (size_t a = 0; a < act.size(); ++a) {
                    Fit& f = fits[act[a]];
                    memcpy(&T[(size_t)act[a] * 7], &S[a * 7], 7 * sizeof(double));
                    f.logp = scale * S[a * 7] + beta_logpdf(f.pi, alpha, beta);
                    if (f.logp - f.logp_cur <= tol) continue;                 // converged: out of the later passes
                    f.logp_cur = f.logp;
                    if (++f.it <= num_iters) next.push_back(act[a]);
                }
                act.swap(next);
            }
        }
        for (const Fit& f : fits) {
            logps[f.i] = f.logp;
            mus[f.i] = f.mu1;
            stds[f.i] = std::sqrt(f.var);
            pis_out[f.i] = f.pi;
        }
    }
    if (n_passes) *n_passes = passes;
    if (e != hipSuccess) return fail(ctx, "tpz_gmm_fit_fused: device pass failed: %s", hipGetErrorString(e));
    return 0;
}
