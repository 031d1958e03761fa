// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32) behind the truncated-DFT resampler (rt_resample.hip):
//
//     C[P x Q] = sum over the segments s of  A_s[P x K_s] . B_s[K_s x Q]
//
// Row-major operands with leading dimensions (lda / ldb shared by the segments, ldc).  One or two (A, B) segments are walked by
// ONE K loop, so y = Re(U) R1 + Im(U) R2 is a single launch that never forms [Re(U) | Im(U)] side by side.
//
// Tile: RS_TILE x RS_TILE outputs per 256-thread workgroup, 2 x 2 waves of 64 x 64, each 2 x 2 MFMA blocks of 32 x 32; RS_KS-deep K
// steps staged through the LDS in two buffers: the global loads of step s + 1 are issued before the MFMAs of step s and stored
// after them, one barrier per step.  A is stored k-major (As[k][row]) so that both fragment reads are 32 consecutive words per
// half-wave (ds_read_b32 banks in half-waves: conflict-free); the row pitch RS_LD = RS_TILE + 4 keeps the float4 stores of B
// aligned and the transposing stores of A at most 2-way conflicted (free for ds_write_b32).
//
// Any P, Q, K >= 1: elements outside a matrix enter the LDS as zeros and every store of C is predicated.  The K loop exists
// twice (rs_k_loop<FAST>), and a workgroup picks one for its whole tile:
//   FAST   the tile lies wholly inside C, every K_s is a multiple of RS_KS and every operand allows 16-byte loads (base and
//          leading dimension multiples of 4 floats -- the runtime pads what it owns): float4 loads, nothing else.
//   else   single loads from addresses CLAMPED into the matrix (always a valid read); which elements lie outside is kept as
//          a bit mask and applied when the registers go to the LDS, behind the MFMAs.
// Either way nothing touches a loaded value between its load and the MFMAs of the current step, so the loads stay in flight
// under them.  (One loop with both paths inside did not: hipcc merged a conditional fetch and store into one block BEHIND the
// MFMAs, turned `ok ? v : 0` on a loaded value back into a branch around the load, and drained vmcnt at the joins.)
//
// Arithmetic: fp32 operands, fp32 accumulation.  An MFMA accumulates as a k-ordered fmaf chain; a chain over thousands of
// detector counts (all positive: the partial sums grow linearly) would carry the rounding of a long running sum, so the chain is
// cut every RS_FOLD steps (RS_FOLD * RS_KS = 64 products) into a second accumulator -- the blocking a CPU sgemm has in its K
// panels, 64 vector adds per 128 MFMAs.  (Emulated on the host for Poisson(5000) counts, 515 x 387 / 4: one unbroken chain is
// 2.3 x the error of a CPU fp32 sgemm against float64, chains of 64 are 0.55 x.)  The order is fixed by (P, Q, K) alone and is
// the same in both loops: results are bit-identical run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpz {

constexpr int RS_TILE = 128;      // outputs per workgroup in P and in Q
constexpr int RS_KS = 16;         // K step
constexpr int RS_FOLD = 4;        // K steps per inner accumulation chain
constexpr int RS_THREADS = 256;
constexpr int RS_LD = RS_TILE + 4;

struct RsSeg {
    const float* A;               // [P][K], leading dimension lda
    const float* B;               // [K][Q], leading dimension ldb
    int K;
};
struct RsArgs {
    RsSeg seg[2];
    int n_seg;
    int fast_ok;                  // every K a multiple of RS_KS, every A and B 16-byte loadable (set by the launcher)
    long long lda, ldb, ldc;
    float* C;
    int P, Q, tiles_q;
};

typedef float rs_f32x16 __attribute__((ext_vector_type(16)));
typedef float (*rs_lds_t)[RS_KS][RS_LD];

template <bool FAST>
__device__ __forceinline__ void rs_k_loop(const RsArgs& a, rs_lds_t As, rs_lds_t Bs, int p0, int q0, rs_f32x16 (&tot)[2][2]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wp = (wave >> 1) * 64, wq = (wave & 1) * 64;
    // loader coordinates: A 128 rows x 4 chunks of 4 k (two rows per thread), B 16 k x 32 chunks of 4 columns (two k per thread)
    const int a_row = tid >> 2, a_k4 = (tid & 3) * 4;
    const int b_k = tid >> 5, b_c4 = (tid & 31) * 4;
    const int steps0 = (a.seg[0].K + RS_KS - 1) / RS_KS;
    const int steps = steps0 + (a.n_seg > 1 ? (a.seg[1].K + RS_KS - 1) / RS_KS : 0);

    float ra[2][4], rb[2][4];
    unsigned in_a = 0xffu, in_b = 0xffu;         // bit 4 * i + j: ra[i][j] / rb[i][j] is an element of its matrix
    auto fetch = [&](int step) {
        const RsSeg& sg = step < steps0 ? a.seg[0] : a.seg[1];
        const int k0 = (step < steps0 ? step : step - steps0) * RS_KS;
        if constexpr (FAST) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 v = *reinterpret_cast<const float4*>(sg.A + (size_t)(p0 + a_row + 64 * i) * a.lda + k0 + a_k4);
                ra[i][0] = v.x; ra[i][1] = v.y; ra[i][2] = v.z; ra[i][3] = v.w;
                const float4 w = *reinterpret_cast<const float4*>(sg.B + (size_t)(k0 + b_k + 8 * i) * a.ldb + q0 + b_c4);
                rb[i][0] = w.x; rb[i][1] = w.y; rb[i][2] = w.z; rb[i][3] = w.w;
            }
        } else {
            in_a = in_b = 0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int p = p0 + a_row + 64 * i, kb = k0 + b_k + 8 * i;
                const float* arow = sg.A + (size_t)min(p, a.P - 1) * a.lda;
                const float* brow = sg.B + (size_t)min(kb, sg.K - 1) * a.ldb;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = k0 + a_k4 + j, q = q0 + b_c4 + j;
                    ra[i][j] = arow[min(k, sg.K - 1)];
                    rb[i][j] = brow[min(q, a.Q - 1)];
                    in_a |= (p < a.P && k < sg.K ? 1u : 0u) << (4 * i + j);
                    in_b |= (kb < sg.K && q < a.Q ? 1u : 0u) << (4 * i + j);
                }
            }
        }
    };
    // (a bit mask, not a select: see the note on the two loops above)
    auto keep = [](float v, unsigned bits, int bit) {
        return FAST ? v : __uint_as_float(__float_as_uint(v) & (0u - ((bits >> bit) & 1u)));
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) As[buf][a_k4 + j][a_row + 64 * i] = keep(ra[i][j], in_a, 4 * i + j);
            *reinterpret_cast<float4*>(&Bs[buf][b_k + 8 * i][b_c4]) =
                make_float4(keep(rb[i][0], in_b, 4 * i), keep(rb[i][1], in_b, 4 * i + 1), keep(rb[i][2], in_b, 4 * i + 2),
                            keep(rb[i][3], in_b, 4 * i + 3));
        }
    };

    rs_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; tot[i][j][r] = 0.f; }

    fetch(0);
    stash(0);
    __syncthreads();
    const int fr = lane & 31, fk = lane >> 5;      // fragment maps of 32x32x2: A[i = lane & 31][k = lane >> 5], B[k][j = lane & 31]
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        // (the last step fetches and stores its own chunk once more, into the buffer nobody reads again: unconditional, so that
        // fetch -> MFMAs -> store stays in that order)
        fetch(min(s + 1, steps - 1));
        __builtin_amdgcn_sched_barrier(0);       // (the scheduler otherwise sinks the loads to the last few MFMAs of the step)
#pragma unroll
        for (int kk = 0; kk < RS_KS; kk += 2) {
            const float a0 = As[buf][kk + fk][wp + fr], a1 = As[buf][kk + fk][wp + 32 + fr];
            const float b0 = Bs[buf][kk + fk][wq + fr], b1 = Bs[buf][kk + fk][wq + 32 + fr];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if ((s + 1) % RS_FOLD == 0 || s + 1 == steps) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { tot[i][j][r] += acc[i][j][r]; acc[i][j][r] = 0.f; }
        }
        stash(buf ^ 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(RS_THREADS) void resample_gemm_kernel(RsArgs a) {
    __shared__ __attribute__((aligned(16))) float As[2][RS_KS][RS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][RS_KS][RS_LD];
    const int p0 = ((int)blockIdx.x / a.tiles_q) * RS_TILE, q0 = ((int)blockIdx.x % a.tiles_q) * RS_TILE;
    rs_f32x16 tot[2][2];
    if (a.fast_ok && p0 + RS_TILE <= a.P && q0 + RS_TILE <= a.Q) rs_k_loop<true>(a, As, Bs, p0, q0, tot);
    else rs_k_loop<false>(a, As, Bs, p0, q0, tot);
    // C / D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wp = (wave >> 1) * 64, wq = (wave & 1) * 64, fr = lane & 31, fk = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + wq + 32 * j + fr;
            if (q >= a.Q) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + wp + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fk;
                if (p < a.P) a.C[(size_t)p * a.ldc + q] = tot[i][j][r];
            }
        }
}

}  // namespace tpz
