// launch helpers implemented in kernels_misc.hip and nms.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.h"

namespace tpz {

// sum of v over the 64 lanes of a wave, in every lane: the butterfly the fp64 reductions share (mean / std, the mixture fit)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

hipError_t launch_conv_direct(const ConvArgs& a, const float* d_w, int K, int KZ, int dil, hipStream_t s);
hipError_t launch_maxpool2(const float* in, float* out, int C, int D, int H, int W, int dims, hipStream_t s);
hipError_t launch_meanstd(const float* x, int D, int H, int W, long long ps, int pitch, int unbiased, int mode,
                          const float* d_g, double* d_part, int part_blocks, float* d_out, hipStream_t s);
hipError_t launch_gmm_pass(const float* x, size_t n, int mode, const double* d_par, double* d_part, int part_blocks,
                           double* d_out, hipStream_t s);
hipError_t launch_affine(const float* x, float* y, size_t n, float scale, float shift, hipStream_t s);
hipError_t launch_normalize(const float* x, float* y, size_t n, float mu, float sd, hipStream_t s);     // y = (x - mu) / sd
// y = (x - mu) / sd, then 0 where y < -c or y > c (fp32 comparisons; NaN passes); c <= 0: launch_normalize
hipError_t launch_normalize_cutoff(const float* x, float* y, size_t n, float mu, float sd, float c, hipStream_t s);
hipError_t launch_affine_dev(const float* x, int D, int H, int W, long long ps, int pitch, const float* d_p, float* y,
                             hipStream_t s);

// Stored MRC pixel types -> fp32 (decode_kernel).  Bytes per pixel of the real scalar modes the library decodes on the device
// (0 int8, 1 int16, 6 uint16, 12 float16); 0 for every other mode.
static inline size_t stored_itemsize(int mrc_mode) {
    return mrc_mode == 0 ? 1 : (mrc_mode == 1 || mrc_mode == 6 || mrc_mode == 12) ? 2 : 0;
}
// The fp32 bits of a binary16 value, by integer operations only: what numpy's astype(float32) gives for all 65 536 patterns --
// the 2 046 subnormals become the normal fp32 value m * 2^-24 (an exact int -> float conversion and an exact scaling by a power
// of two, so no float mode of the device, denormal flushing included, can touch it), zeros and infinities keep their sign, a NaN
// keeps sign and payload.
__host__ __device__ static inline unsigned f16_bits_to_f32_bits(unsigned h) {
    const unsigned sign = (h & 0x8000u) << 16, em = h & 0x7fffu;
    if (em >= 0x7c00u) return sign | 0x7f800000u | ((em & 0x3ffu) << 13);      // inf / NaN
    if (em >= 0x0400u) return sign | ((em << 13) + (112u << 23));              // normal: exponent rebias 15 -> 127
    return sign | __builtin_bit_cast(unsigned, (float)(int)em * 0x1p-24f);     // zero / subnormal
}
// out[i] = (float)raw[i] for n pixels of MRC mode 0 / 1 / 6 / 12 (any other mode: hipErrorInvalidValue).  raw must be 16-byte
// aligned; out 4-byte (16-byte for the vector body, otherwise every pixel takes the scalar loop).  One launch; n == 0: none.
hipError_t launch_decode(const void* raw, int mrc_mode, size_t n, float* out, hipStream_t s);

// fp32 -> stored pixels (encode_kernel).  The encodings of tpz_encode (topaz_hip.h: TPZ_ENC_F16, TPZ_ENC_U8) and their bytes per
// pixel; 0 for anything else.
enum { ENC_F16 = 12, ENC_U8 = 8 };
static inline size_t encoded_itemsize(int enc) { return enc == ENC_F16 ? 2 : enc == ENC_U8 ? 1 : 0; }
// The binary16 bits of an fp32 value, by integer operations only: what numpy's astype(np.float16) gives for every one of the 2^32
// patterns (npy_floatbits_to_halfbits) -- round to nearest, ties to even, at the 13 dropped mantissa bits of a half normal and at
// the 14..24 dropped bits of a half subnormal (a carry walks into the exponent, up to the smallest normal and up to infinity, by
// itself); |x| >= 65520 (the midpoint of 65504 and 2^16) is +-inf; below 2^-25, fp32 subnormals included, +-0; a NaN keeps its sign
// and the top 10 payload bits, with bit 0 set when those are all zero.
__host__ __device__ static inline unsigned f32_bits_to_f16_bits(unsigned f) {
    const unsigned sign = (f >> 16) & 0x8000u, a = f & 0x7fffffffu;
    if (a >= 0x7f800000u) {                                                    // inf / NaN
        if (a == 0x7f800000u) return sign | 0x7c00u;
        const unsigned m = 0x7c00u + ((a & 0x007fffffu) >> 13);
        return sign | (m == 0x7c00u ? 0x7c01u : m);
    }
    if (a >= 0x477ff000u) return sign | 0x7c00u;                               // >= 65520: rounds to infinity
    const unsigned e = a >> 23;
    if (e >= 113u) {                                                           // half normal: exponent rebias 127 -> 15
        const unsigned h = (a - (112u << 23)) >> 13, rem = a & 0x1fffu;
        return sign | (h + ((rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ? 1u : 0u));
    }
    if (e < 102u) return sign;                                                 // below 2^-25: zero
    // half subnormal: the 24-bit significand in units of 2^(e - 150), stored in units of 2^-24
    const unsigned m = (a & 0x007fffffu) | 0x00800000u, shift = 126u - e;      // 14 .. 24
    const unsigned h = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    return sign | (h + ((rem > half || (rem == half && (h & 1u))) ? 1u : 0u));
}
// out[i] = encoded in[i] for n pixels; enc ENC_F16 (2 bytes per pixel) or ENC_U8 (1 byte, with mi and ma of quantize); any other
// enc: hipErrorInvalidValue.  in must be 4-byte aligned, out aligned to its pixel; both 16-byte aligned for the vector body,
// otherwise every pixel takes the scalar loop.  overflow (ENC_F16; may be null): += finite inputs stored as +-inf.  One launch;
// n == 0: none.
hipError_t launch_encode(const float* in, int enc, size_t n, float mi, float ma, void* out, unsigned long long* overflow,
                         hipStream_t s);
hipError_t launch_transpose(const float* in, float* out, int R, int Cc, hipStream_t s);
hipError_t launch_maxpool2_split(const void* in, void* out, int C, int D, int H, int W, int dims, hipStream_t s);
hipError_t launch_maxpoolz_split(const float* in, float* out, int C, int D, int H, int W, hipStream_t s);   // z pairs only (split cells)
hipError_t launch_maxpoolk(const void* in, void* out, int C, int D, int H, int W, int k, int dil, int dims, bool split,
                           hipStream_t s);
// padded 3^dims pools, stride 1 (pool_pad.hip): dilated max with -inf padding / plain mean with zero padding and divisor 3^dims;
// out is X + 2 * pad - 2 * dil per axis; 0 <= pad <= dil
hipError_t launch_pool_pad(const void* in, void* out, int C, int D, int H, int W, int dil, int pad, int dims, bool mean, bool split,
                           hipStream_t s);
hipError_t launch_shiftx_split(const float* in, void* out, int K, int pad, size_t rows, int W, int Wo, unsigned* flag,
                               hipStream_t s, size_t r0 = 0, size_t r1 = (size_t)-1, int x0 = 0, int x1 = 0x7fffffff);
hipError_t launch_shiftsum(const float* Y, float* out, int K, size_t rows, int W, int Wp, float bias, const float* nrm,
                           int norm_out, hipStream_t s, size_t y0 = 0, size_t y1 = (size_t)-1, int x0 = 0, int x1 = 0x7fffffff,
                           const float* res = nullptr, int Hp = 0, int z0 = 0, int z1 = 1);   // Hp > 0: planes [z0, z1) of Hp rows
// 1-output-channel k^dims conv over split cells on the vector ALUs (K = 3 or 5; KZ = K for a 3-D conv, else 1), fused with bias,
// same-size residual and un-normalisation; wt = [KZ][cells][kx][ky][8] fp32
hipError_t launch_conv_cout1_split(const void* in, const float* wt, float* out, const float* res, const float* nrm, int norm_out,
                                   float bias, int cells, int K, int KZ, int D, int H, int W, int z0, int z1, int y0, int y1,
                                   int x0, int x1, hipStream_t s);
hipError_t launch_s2d_split(const float* in, void* out, int d, int h, int w, int H, int W, int dims, unsigned* flag,
                            hipStream_t s);
hipError_t launch_to_split(const float* in, void* out, int C, int H, int W, unsigned* flag, hipStream_t s);
hipError_t launch_from_split(const void* in, float* out, int C, int H, int W, hipStream_t s);
hipError_t launch_copy_box(const float* src, long long sps, int spitch, float* dst, long long dps, int dpitch, int bd,
                           int bh, int bw, hipStream_t s);
// Range scaling of a scoring pass (rt_forward.hip tpz_model_forward): rng[0] = 2^-s, rng[1] = 0, rng[2] = 2^s, rng[3] = s with s >= 0
// chosen from the exponent histogram of the image (its 99.9 % quantile of |x| brought to ~2^3); dst[i] = src[i] * 2^-s for the
// model's bias-like vectors.  `hist` = 256 zeroed words (left zeroed).
hipError_t launch_range_fit(const float* x, size_t n, unsigned* hist, float* rng, const float* src, float* dst, size_t n_vec,
                            hipStream_t s);
// y[i] = y[i] * rng[2] + add (skipped on the device when that is the identity)
hipError_t launch_unscale(float* y, size_t n, const float* rng, float add, hipStream_t s);
hipError_t launch_extract_tile3d(const float* tomo, int D, int H, int W, int i0, int j0, int k0, int d,
                                 const float* d_g, float* tile, hipStream_t s);

// delta_stats: max |a - b| (non-finite differences count as +inf) with the first index that attains it, max |b| (NaN: +inf) and
// the fp64 sum of (a - b)^2 over n >= 1 elements, into *out on the device (the layout of tpz_delta, topaz_hip.h).  16-byte loads
// when both pointers are 16-byte aligned, dword loads otherwise.  delta_stats_grid(n) workgroups -- a function of n alone -- leave
// one partial each in `scratch` (DELTA_SCRATCH_BYTES) and one more workgroup folds them in order: two runs are bit-identical.
struct DeltaStats {
    float max_abs_delta, max_abs_ref;
    long long argmax;
    double sum_sq;
};
enum { DELTA_MAX_BLOCKS = 512, DELTA_SCRATCH_BYTES = 24 * DELTA_MAX_BLOCKS };
int delta_stats_grid(size_t n);
hipError_t launch_delta_stats(const float* a, const float* b, size_t n, void* scratch, DeltaStats* out, hipStream_t s);

hipError_t nms_mark(const float* score, size_t n, float thr, uint8_t* status, uint32_t* cand, unsigned int* counters,
                    hipStream_t s);
hipError_t nms2d_sweep(const float* score, int H, int W, const int* near_cells, int n_near, const int* cells, int ncells,
                       uint8_t* status, const uint32_t* list_in, uint32_t* list_out, uint32_t* list_ver, unsigned int* cnt,
                       unsigned int* cnt_ver, unsigned int* snap, uint64_t* keys, unsigned int* npicks, size_t hint,
                       hipStream_t s);
hipError_t nms3d_sweep(const float* score, long long n, const int* near_deltas, int n_near, const int* deltas, int ndelta,
                       uint8_t* status, const uint32_t* list_in, uint32_t* list_out, uint32_t* list_ver, unsigned int* cnt,
                       unsigned int* cnt_ver, unsigned int* snap, uint64_t* keys, unsigned int* npicks, size_t hint,
                       hipStream_t s);
hipError_t fill_u64(uint64_t* p, size_t lo, size_t hi, uint64_t v, hipStream_t s);
hipError_t bitonic_sort_desc(uint64_t* keys, size_t npow2, hipStream_t s);
hipError_t nms_write(const uint64_t* keys, unsigned int n, const float* score, int H, int W, int dims,
                     int32_t* coords, float* out_scores, hipStream_t s);

}  // namespace tpz
