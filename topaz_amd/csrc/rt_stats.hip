// Statistics and elementwise entry points: mean / std, GMM fit (topaz normalize), affine, normalise, stored-type decode.
#include <cstddef>
#include "rt_internal.h"

namespace tpz::rt {

static_assert(sizeof(tpz_delta) == sizeof(DeltaStats) && offsetof(tpz_delta, argmax) == offsetof(DeltaStats, argmax) &&
                  offsetof(tpz_delta, sum_sq) == offsetof(DeltaStats, sum_sq),
              "tpz_delta is what delta_final_kernel writes");
static_assert(DELTA_SCRATCH_BYTES + sizeof(DeltaStats) <= 2 * PART_BLOCKS * sizeof(double), "delta_stats works in tpz_ctx::d_part");

// the partials and, behind them, the result live in the reduction scratch of the ctx stream
int delta_stats(tpz_ctx* ctx, const float* d_a, const float* d_b, size_t n, tpz_delta* out) {
    DeltaStats* d_res = (DeltaStats*)((char*)ctx->d_part + DELTA_SCRATCH_BYTES);
    HIPCHK(ctx, enqueue(ctx, [=](hipStream_t st) { return launch_delta_stats(d_a, d_b, n, ctx->d_part, d_res, st); }));
    HIPCHK(ctx, hipMemcpyAsync(out, d_res, sizeof(tpz_delta), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_delta_stats(tpz_ctx* ctx, const float* d_a, const float* d_b, size_t n, tpz_delta* out) {
    if (!ctx || !d_a || !d_b || !out) return fail(ctx, "tpz_delta_stats: NULL argument");
    if (n == 0) return fail(ctx, "tpz_delta_stats: n = 0: nothing to compare");
    if (n > ((size_t)1 << 40)) return fail(ctx, "tpz_delta_stats: n = %zu is above 2^40", n);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return delta_stats(ctx, d_a, d_b, n, out);
}

int tpz_mean_std(tpz_ctx* ctx, const float* d_x, size_t n, int unbiased, float* h_mean_std) {
    if (!ctx || !d_x || !h_mean_std || n == 0) return fail(ctx, "tpz_mean_std: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float* out = next_nrm(ctx);
    // present the vector as rows of <= 2^20 elements so int geometry cannot overflow
    const int Wv = (int)std::min<size_t>(n, (size_t)1 << 20);
    const size_t rows = n / Wv;
    if (rows * (size_t)Wv != n) {
        // fall back to a single row when n is not a multiple (n < 2^31 required)
        if (n >= ((size_t)1 << 31)) return fail(ctx, "tpz_mean_std: n too large for a ragged vector");
        HIPCHK(ctx, launch_meanstd(d_x, 1, 1, (int)n, 0, (int)n, unbiased, 0, nullptr, ctx->d_part, PART_BLOCKS, out, ctx->stream));
    } else {
        HIPCHK(ctx, launch_meanstd(d_x, 1, (int)rows, Wv, 0, Wv, unbiased, 0, nullptr, ctx->d_part, PART_BLOCKS, out, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(h_mean_std, out, 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- 2-component Gaussian mixture fit (topaz normalize) ---------------------------------------------------
// topaz/stats.py:87-117 norm_fit + :120-203 gmm_fit (share_var = True), evaluated in fp64 from the sufficient
// statistics of gmm_pass_kernel: one device pass per EM iteration, the scalar M-step on the host.
int tpz_gmm_fit(tpz_ctx* ctx, const float* d_x, size_t n, const double* pis, const double* splits, int n_init,
                double alpha, double beta, double scale, int num_iters, double tol, double* mus, double* stds,
                double* pis_out, double* logps) {
    if (!ctx || !d_x || !pis || !splits || !mus || !stds || !pis_out || !logps || n < 2 || n_init < 1)
        return fail(ctx, "tpz_gmm_fit: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const WorkBuf par_b(ctx, 8 * sizeof(double)), out_b(ctx, 8 * sizeof(double));
    double *d_par = par_b.as<double>(), *d_out = out_b.as<double>();
    if (!d_par || !d_out) return fail(ctx, "tpz_gmm_fit: workspace allocation failed");
    int rc = 0;
    const double N = (double)n;
    auto pass = [&](int mode, const double (&par)[6], double (&S)[7]) -> int {
        if (hipMemcpyAsync(d_par, par, 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return 1;
        prof_begin(ctx, 2, 0);
        hipError_t e = launch_gmm_pass(d_x, n, mode, d_par, ctx->d_part, 256, d_out, ctx->stream);
        prof_end(ctx);
        if (e != hipSuccess) return 1;
        if (hipMemcpyAsync(S, d_out, 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return 1;
        return hipStreamSynchronize(ctx->stream) != hipSuccess;
    };
    // global moments: hard pass with split = +inf puts everything in component 0
    double S[7];
    {
        const double par[6] = {INFINITY, 0, 0, 0, 0, 0};
        if (pass(0, par, S)) rc = fail(ctx, "tpz_gmm_fit: device pass failed");
    }
    const GmmMoments M = gmm_moments(S, N);
    for (int i = 0; i < n_init && !rc; ++i) {
        double pi = pis[i];
        if (pi == 1.0) {
            gmm_single_component(M, N, alpha, beta, scale, logps[i], mus[i], stds[i], pis_out[i]);
            continue;
        }
        double mu0, mu1, var;
        {
            const double par[6] = {splits[i], 0, 0, 0, 0, 0};
            if (pass(0, par, S)) { rc = fail(ctx, "tpz_gmm_fit: device pass failed"); break; }
        }
        gmm_m_step(S, N, M.mu_all, mu0, mu1, var);
        auto e_step = [&](double (&T)[7]) -> int {
            double par[6];
            gmm_e_step_par(mu0, mu1, var, pi, par);
            return pass(1, par, T);
        };
        if (e_step(S)) { rc = fail(ctx, "tpz_gmm_fit: device pass failed"); break; }
        double logp = scale * S[0] + beta_logpdf(pi, alpha, beta);
        double logp_cur = logp;
        for (int it = 1; it <= num_iters; ++it) {
            // M-step from the assignments of the last E-step (S), MAP estimate of pi under the Beta prior
            pi = gmm_map_pi(S, N, alpha, beta);
            gmm_m_step(S, N, M.mu_all, mu0, mu1, var);
            if (e_step(S)) { rc = fail(ctx, "tpz_gmm_fit: device pass failed"); break; }
            logp = scale * S[0] + beta_logpdf(pi, alpha, beta);
            if (logp - logp_cur <= tol) break;
            logp_cur = logp;
        }
        logps[i] = logp;
        mus[i] = mu1;
        stds[i] = std::sqrt(var);
        pis_out[i] = pi;
    }
    return rc;
}

int tpz_affine(tpz_ctx* ctx, const float* d_x, size_t n, float scale, float shift, float* d_y) {
    if (!ctx || !d_x || !d_y) return fail(ctx, "tpz_affine: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    prof_begin(ctx, 2, 0);
    hipError_t e = launch_affine(d_x, d_y, n, scale, shift, ctx->stream);
    prof_end(ctx);
    HIPCHK(ctx, e);
    return 0;
}

int tpz_normalize(tpz_ctx* ctx, const float* d_x, size_t n, float mean, float std, float* d_y) {
    if (!ctx || !d_x || !d_y) return fail(ctx, "tpz_normalize: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    prof_begin(ctx, 2, 0);
    hipError_t e = launch_normalize(d_x, d_y, n, mean, std, ctx->stream);
    prof_end(ctx);
    HIPCHK(ctx, e);
    return 0;
}

int tpz_normalize_cutoff(tpz_ctx* ctx, const float* d_x, size_t n, float mean, float std, float cutoff, float* d_y) {
    if (!ctx || !d_x || !d_y) return fail(ctx, "tpz_normalize_cutoff: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    prof_begin(ctx, 2, 0);
    hipError_t e = launch_normalize_cutoff(d_x, d_y, n, mean, std, cutoff, ctx->stream);
    prof_end(ctx);
    HIPCHK(ctx, e);
    return 0;
}

int tpz_decode(tpz_ctx* ctx, const void* d_raw, int mrc_mode, size_t n, float* d_out) {
    if (!ctx || !d_raw || !d_out) return fail(ctx, "tpz_decode: bad arguments");
    const size_t item = stored_itemsize(mrc_mode);
    if (item == 0) return fail(ctx, "tpz_decode: MRC mode %d is not one of the stored real types 0, 1, 6, 12", mrc_mode);
    if (n == 0) return 0;
    if (((uintptr_t)d_raw & 15) || ((uintptr_t)d_out & 3))
        return fail(ctx, "tpz_decode: d_raw must be 16-byte aligned (and d_out 4-byte)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, enqueue(ctx, 2, 0.0, nullptr, (double)n * (item + 4),
                        [=](hipStream_t st) { return launch_decode(d_raw, mrc_mode, n, d_out, st); }));
    return 0;
}

int tpz_encode(tpz_ctx* ctx, const float* d_in, size_t n, int enc, const float* params, void* d_out,
               unsigned long long* d_overflow) {
    if (!ctx || !d_in || !d_out) return fail(ctx, "tpz_encode: bad arguments");
    const size_t item = encoded_itemsize(enc);
    if (item == 0) return fail(ctx, "tpz_encode: encoding %d is neither TPZ_ENC_F16 nor TPZ_ENC_U8", enc);
    if (enc == ENC_U8 && !params) return fail(ctx, "tpz_encode: TPZ_ENC_U8 needs params = {mi, ma}");
    if (n == 0) return 0;
    if (((uintptr_t)d_in & 3) || ((uintptr_t)d_out & (item - 1)) || ((uintptr_t)d_overflow & 7))
        return fail(ctx, "tpz_encode: d_in must be 4-byte aligned, d_out aligned to its pixel, d_overflow 8-byte");
    const float mi = enc == ENC_U8 ? params[0] : 0.0f, ma = enc == ENC_U8 ? params[1] : 1.0f;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, enqueue(ctx, 2, 0.0, nullptr, (double)n * (item + 4),
                        [=](hipStream_t st) { return launch_encode(d_in, enc, n, mi, ma, d_out, d_overflow, st); }));
    return 0;
}
