// The truncated-DFT resampler with its operators resident on the device (tpz_resample_*): `downsample` of
// topaz/utils/image.py:38-61 (rfft2 -> keep the low-frequency block -> irfft2) as the real-linear map it is,
//     U = [Re Lc; Im Lc] . x   (2m x N),      y = Re(U) . R1 + Im(U) . R2   (m x n),
// two launches of resample_gemm_kernel on the ctx stream.  A plan owns the two operators (uploaded once, at create, with their
// rows padded to multiples of 4 floats and R transposed to [2N][n] so that both stages read row-major K x Q operands); a run
// takes its intermediate U from the ctx workspace pool and enqueues: no host packing, no upload, no synchronise.
#include "rt_internal.h"
#include "resample_gemm.h"

struct tpz_resample {
    tpz_ctx* ctx = nullptr;
    int M = 0, N = 0, m = 0, n = 0;
    float* d_L = nullptr;         // [2m][ldl]: Re Lc over Im Lc
    float* d_Rt = nullptr;        // [2N][ldr]: R1 over R2
    long long ldl = 0, ldr = 0, ldu = 0;
};

namespace tpz::rt {
namespace {

inline long long pad4(long long v) { return (v + 3) & ~3LL; }
inline int vec_ok(const float* p, long long ld) { return ((uintptr_t)p & 15) == 0 && (ld & 3) == 0; }

hipError_t launch_resample_gemm(RsArgs a, hipStream_t s) {
    const long long tp = (a.P + RS_TILE - 1) / RS_TILE, tq = (a.Q + RS_TILE - 1) / RS_TILE;
    a.tiles_q = (int)tq;
    a.fast_ok = 1;
    for (int i = 0; i < a.n_seg; ++i)
        a.fast_ok &= a.seg[i].K % RS_KS == 0 && vec_ok(a.seg[i].A, a.lda) && vec_ok(a.seg[i].B, a.ldb);
    hipLaunchKernelGGL(resample_gemm_kernel, dim3((unsigned)(tp * tq)), dim3(RS_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace

tpz_ctx* resample_ctx(tpz_resample* plan) { return plan ? plan->ctx : nullptr; }

}  // namespace tpz::rt

using namespace tpz;
using namespace tpz::rt;

int tpz_resample_create(tpz_ctx* ctx, int M, int N, int m, int n, const float* h_L, const float* h_R, tpz_resample** out) {
    if (out) *out = nullptr;
    if (!ctx || !h_L || !h_R || !out) return fail(ctx, "tpz_resample_create: NULL argument");
    if (M < 1 || N < 1 || m < 1 || n < 1 || m > M || n > N)
        return fail(ctx, "tpz_resample_create: %d x %d -> %d x %d is not a reduction of a non-empty image", M, N, m, n);
    // one workgroup per 128 x 128 outputs, 32-bit tile counts
    if ((2LL * m + RS_TILE - 1) / RS_TILE * ((N + RS_TILE - 1LL) / RS_TILE) >= (1LL << 31))
        return fail(ctx, "tpz_resample_create: image too large");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    tpz_resample* pl = new tpz_resample;
    pl->ctx = ctx; pl->M = M; pl->N = N; pl->m = m; pl->n = n;
    pl->ldl = pad4(M); pl->ldr = pad4(n); pl->ldu = pad4(N);
    const size_t nl = (size_t)2 * m * pl->ldl, nr = (size_t)2 * N * pl->ldr;
    // h_R is [n][2N] = [R1; R2]^T: transposed here, once, into the [2N][n] the second stage reads as its K x Q operand
    std::vector<float> packed(std::max(nl, nr), 0.f);
    hipError_t e = hipMalloc((void**)&pl->d_L, nl * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&pl->d_Rt, nr * sizeof(float));
    if (e == hipSuccess) {
        for (int r = 0; r < 2 * m; ++r) memcpy(&packed[(size_t)r * pl->ldl], h_L + (size_t)r * M, (size_t)M * sizeof(float));
        e = hipMemcpy(pl->d_L, packed.data(), nl * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        std::fill(packed.begin(), packed.end(), 0.f);
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < 2 * N; ++k) packed[(size_t)k * pl->ldr + j] = h_R[(size_t)j * 2 * N + k];
        e = hipMemcpy(pl->d_Rt, packed.data(), nr * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        tpz_resample_free(pl);
        return fail(ctx, "tpz_resample_create: %s (%d x %d -> %d x %d)", hipGetErrorString(e), M, N, m, n);
    }
    ctx->resample_upload_bytes += (long long)((nl + nr) * sizeof(float));
    *out = pl;
    return 0;
}

int tpz_resample_run(tpz_resample* pl, const float* d_in, float* d_out) {
    if (!pl || !d_in || !d_out) return fail(pl ? pl->ctx : nullptr, "tpz_resample_run: NULL argument");
    tpz_ctx* ctx = pl->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int M = pl->M, N = pl->N, m = pl->m, n = pl->n;
    const WorkBuf u_b(ctx, (size_t)2 * m * pl->ldu * sizeof(float));       // (re-used only by later work on the same stream)
    float* d_u = u_b.as<float>();
    if (!d_u) return fail(ctx, "tpz_resample_run: out of device memory for the %d x %d intermediate", 2 * m, N);
    RsArgs s1{};
    s1.seg[0].A = pl->d_L; s1.seg[0].B = d_in; s1.seg[0].K = M;
    s1.n_seg = 1; s1.lda = pl->ldl; s1.ldb = N; s1.ldc = pl->ldu; s1.C = d_u; s1.P = 2 * m; s1.Q = N;
    RsArgs s2{};
    s2.seg[0].A = d_u; s2.seg[0].B = pl->d_Rt; s2.seg[0].K = N;
    s2.seg[1].A = d_u + (size_t)m * pl->ldu; s2.seg[1].B = pl->d_Rt + (size_t)N * pl->ldr; s2.seg[1].K = N;
    s2.n_seg = 2; s2.lda = pl->ldu; s2.ldb = pl->ldr; s2.ldc = n; s2.C = d_out; s2.P = m; s2.Q = n;
    const double dm = m, dn = n, dM = M, dN = N;
    hipError_t e = enqueue(ctx, 2, 2.0 * 2.0 * dm * dM * dN, "resample_gemm", 4.0 * (2.0 * dm * dM + dM * dN + 2.0 * dm * dN),
                           [s1](hipStream_t s) { return launch_resample_gemm(s1, s); });
    if (e == hipSuccess)
        e = enqueue(ctx, 2, 2.0 * dm * 2.0 * dN * dn, "resample_gemm", 4.0 * (2.0 * dm * dN + 2.0 * dN * dn + dm * dn),
                    [s2](hipStream_t s) { return launch_resample_gemm(s2, s); });
    HIPCHK(ctx, e);
    return 0;
}

void tpz_resample_free(tpz_resample* pl) {
    if (!pl) return;
    if (pl->ctx) {
        (void)hipSetDevice(pl->ctx->device);
        (void)hipStreamSynchronize(pl->ctx->stream);      // runs already enqueued still read the operators
    }
    if (pl->d_L) (void)hipFree(pl->d_L);
    if (pl->d_Rt) (void)hipFree(pl->d_Rt);
    delete pl;
}

int tpz_resample_shape(tpz_resample* pl, int* M, int* N, int* m, int* n) {
    if (!pl) return fail(nullptr, "tpz_resample_shape: NULL plan");
    if (M) *M = pl->M;
    if (N) *N = pl->N;
    if (m) *m = pl->m;
    if (n) *n = pl->n;
    return 0;
}

long long tpz_resample_upload_bytes(tpz_ctx* ctx) { return ctx ? ctx->resample_upload_bytes : 0; }
