/* libtopaz_hip.so -- C-ABI of the MI355X (gfx950) hot path of tbepler/topaz.
 *
 * The reference has no FFI layer: its boundary is the Python callable
 *     model(x: Tensor[N,1,H,W]) -> Tensor[N,1,H,W]          (nn.Module.__call__)
 * invoked from topaz/extract.py:249, topaz/model/utils.py:122, topaz/predict.py:26,
 * topaz/denoise.py:293, plus the pure functions non_maximum_suppression
 * (topaz/algorithms.py:25) / non_maximum_suppression_3d (:66) and Denoise.denoise
 * (topaz/denoise.py:328) / Denoise3D.denoise (:340).  Each entry point below names the
 * reference interface it replaces.  The Python package topaz_amd binds these with ctypes
 * (topaz_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; tpz_last_error(ctx) gives the text.
 *   - plain pointers and sizes only.  Pointers named d_* are DEVICE pointers (HBM of the
 *     ctx's GPU); h_* are host pointers.  fp32 everywhere, tensors are dense, C-order
 *     [C][D][H][W] (D omitted in 2-D), batch entries are processed one after another.
 *   - one ctx per process/GPU; calls on a ctx are serialised on its HIP stream
 *     (tpz_ctx_set_stream lets the caller supply e.g. torch's current stream).
 *     Calls are asynchronous w.r.t. the host unless stated; tpz_ctx_sync waits.
 *   - the library owns its workspaces (grow-only), the caller owns in/out buffers.
 */
#ifndef TOPAZ_HIP_H
#define TOPAZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tpz_ctx tpz_ctx;
typedef struct tpz_model tpz_model;

/* ---- layer program: the manifest a model is loaded from ------------------------------
 * A model is a list of ops over tensor "slots".  Slot 0 is the network input (1 channel);
 * the dst slot of the last layer is the network output.  The host packer
 * (topaz_amd/model/pack.py) emits this from a state_dict / unpickled module; it mirrors
 * the module graphs of topaz/model/features/resnet.py:243-251,185-202,
 * topaz/model/features/basic.py:98-111, topaz/model/classifier.py:64-66 and
 * topaz/denoising/models.py:130-175,515-562.                                              */
enum {
    TPZ_OP_CONV = 1,
    TPZ_OP_MAXPOOL2 = 2,     /* MaxPool(2) with floor (the U-Net encoders, denoising/models.py:81-97) */
    TPZ_OP_MAXPOOL = 3,      /* k^dims max over a window dilated by `dil`, stride 1, `pad` elements of -inf padding per side
                                (output n + 2 * pad - dil * (k - 1)): the FILLED form of a max-pool with stride 2.
                                pad = 0: MaxPool(3, stride = 2) of ResNet6 and the --pooling max ResNets (resnet.py:10-47,254-339).
                                pad = 1 (k = 3, pad <= dil): MaxPool(3, stride = 2, padding = 1) of a conv31/63/127 stack trained
                                with --pooling max (basic.py:33-39,54-56,81-89) -- its score map is 2 * (dil - 1) smaller per pool */
    TPZ_OP_AVGPOOL = 4       /* 3^dims mean, stride 1, k = 3, dil = 1, pad = 1: zero padding, divisor 3^dims everywhere
                                (count_include_pad).  The FILLED form of AvgPool(3, stride = 2, padding = 1) of a conv31/63/127
                                stack trained with --pooling avg: fill() sets its stride to 1 and, the module having no
                                `dilation`, nothing else (basic.py:81-89); it preserves the size */
};

typedef struct tpz_layer {
    int32_t op;        /* TPZ_OP_* */
    int32_t dims;      /* 2 or 3 */
    int32_t src;       /* input slot */
    int32_t src2;      /* -1, or slot concatenated AFTER src on the channel axis; src is first
                          nearest-upsampled to src2's size (F.interpolate(mode='nearest') + torch.cat,
                          denoising/models.py:140-171) */
    int32_t dst;       /* output slot */
    int32_t cin;       /* total input channels (src [+ src2]) */
    int32_t cout;
    int32_t k;         /* cubic kernel size */
    int32_t dil;       /* dilation (the "filled" stride->dilation rewrite, resnet.py:87-92,153-164) */
    int32_t pad;       /* padding on every side: zeros (CONV, AVGPOOL), -inf (MAXPOOL) */
    float slope;       /* activation y = v > 0 ? v : slope*v : 0 = ReLU, 0.1 = LeakyReLU, 1 = none, else PReLU */
    int64_t w_off;     /* offset (floats) of the [cout][cin][k(][k)][k] weights in the blob */
    int64_t b_off;     /* offset of the [cout] bias, -1 = none */
    int32_t res;       /* -1, or slot added before the activation (ResidA skip, resnet.py:185-202) */
    int32_t res_crop;  /* the skip is centre-cropped by this many pixels per side */
    int64_t post_scale_off; /* -1, or [cout] scale of the eval-BN affine applied AFTER the add (bn1) */
    int64_t post_shift_off;
    int32_t head;      /* 1: fuse a following 1x1 conv cout->1 (classifier.py:29,65); dst then has 1 channel */
    int32_t reserved;
    int64_t head_w_off;/* [cout] */
    int64_t head_b_off;/* [1] */
} tpz_layer;

/* ---- context ------------------------------------------------------------------------- */
/* replaces topaz/cuda.py:16-32 set_device (no CPU fallback: errors are reported, never hidden).
 * Threading: a context, with the models loaded into it, is driven by ONE host thread at a time -- the staging ring is the
 * exception: its producer side (the h2d call and the pinned buffers) may run on a reader thread, as the CLI does.  One
 * process per GPU with one ctx is the tested configuration (topaz --gpus N); several contexts on one device driven by
 * several threads at once are not. */
int tpz_ctx_create(int device_id, tpz_ctx** out);
void tpz_ctx_destroy(tpz_ctx* ctx);
const char* tpz_last_error(tpz_ctx* ctx);            /* ctx may be NULL: last global error */
int tpz_ctx_set_stream(tpz_ctx* ctx, void* hip_stream); /* NULL = the ctx's own stream */
int tpz_ctx_sync(tpz_ctx* ctx);
const char* tpz_version(void);

/* ---- models -------------------------------------------------------------------------- */
/* replaces topaz/model/factory.py:33-64 load_model + model.eval(); model.fill(); model.cuda()
 * (extract.py:227-232) and topaz/denoising/models.py:581-625 load_model + .cuda() (denoise.py:248-262):
 * weights are packed into MFMA fragment order and copied to the device; the model owns them. */
int tpz_model_load(tpz_ctx* ctx, const tpz_layer* layers, int n_layers, const float* h_blob,
                   size_t n_floats, tpz_model** out);
void tpz_model_free(tpz_model* m);

/* replaces model(x) -- LinearClassifier.forward (classifier.py:48-66), UDenoiseNet.forward
 * (denoising/models.py:130-175), UDenoiseNet3D.forward (:515-562).
 * d_in [n][1][D][H][W] -> d_out [n][1][Do][Ho][Wo]; D = 1 for 2-D models.
 * Arithmetic path per image: the 2xf16 kernels where the model has them, re-run on the fp32 kernels when an activation left
 * the f16 range; a 3-D volume whose widest activation exceeds 4 GiB per split half (32-bit offsets of the plane-stacked
 * kernels: e.g. 128 channels x more than 256^3 voxels) goes to the fp32 kernels directly -- or is tiled by the caller, as
 * classify_patches does.  A 2-D image above ~11 500^2 pixels is refused with a message: process it in patches. */
int tpz_model_forward(tpz_model* m, const float* d_in, int n, int D, int H, int W, float* d_out);
/* output size of the model for a given input size */
int tpz_model_out_shape(tpz_model* m, int D, int H, int W, int* Do, int* Ho, int* Wo);
/* channels of the model output (1 for every network of the reference; >1 only for partial programs) */
int tpz_model_out_channels(tpz_model* m, int* C);

/* ---- denoising ----------------------------------------------------------------------- */
/* replaces Denoise.denoise / denoise_patches / _denoise (topaz/denoise.py:274-332):
 * patch grid range(0,H,patch) x range(0,W,patch), each crop [i-pad, i+patch+pad) clipped to the
 * image is normalised by ITS OWN mean / unbiased std (torch.std), run through the net,
 * un-normalised and its centre pasted.  patch <= 0 or patch+pad >= max(H,W): whole image. */
int tpz_denoise_2d(tpz_model* m, const float* d_in, int H, int W, int patch, int pad, float* d_out);
/* replaces Denoise3D.denoise + PatchDataset (topaz/denoise.py:340-377,
 * topaz/denoising/datasets.py:412-468): global mean / population std (numpy), zero-filled
 * (patch+2*pad)^3 tiles normalised globally then per tile (unbiased), stitched.
 * patch < 1: the whole volume goes through _denoise. */
int tpz_denoise_3d(tpz_model* m, const float* d_in, int D, int H, int W, int patch, int pad, float* d_out);
/* One rank's share of a tomogram: only the tiles whose index (z-major over the ceil(n / patch)^3 grid, the order of
 * PatchDataset) is == shard (mod n_shards) are denoised and pasted; the rest of d_out is left untouched (zero it first
 * and sum the ranks' volumes).  The global mean / std are computed over the whole input by every rank -- a deterministic
 * reduction, so all ranks normalise identically without exchanging anything. */
int tpz_denoise_3d_shard(tpz_model* m, const float* d_in, int D, int H, int W, int patch, int pad, int shard, int n_shards,
                         float* d_out);
/* mean and std of n floats; unbiased != 0 -> divide by n-1 (torch.std), else by n (numpy.std)
 * (topaz/denoise.py:283,343,388).  h_mean_std[2] on the host; synchronises. */
int tpz_mean_std(tpz_ctx* ctx, const float* d_x, size_t n, int unbiased, float* h_mean_std);
/* 2-component Gaussian-mixture fit of pixel values, the model behind `topaz normalize` (topaz/stats.py:87-203
 * norm_fit + gmm_fit with a shared variance and a Beta(alpha, beta) prior on the mixing proportion): for each of
 * the n_init initialisations (mixing proportion pis[i], hard split at splits[i] = quantile(x, 1 - pis[i]);
 * pis[i] == 1 selects the single-Gaussian model) runs EM for at most num_iters iterations or until the
 * log-likelihood gains <= tol, and returns mean / std of the upper component, the MAP proportion and the final
 * log-likelihood (x scale, the sub-sampling factor).  d_x: n device floats.  One device pass per EM iteration,
 * statistics in fp64. */
int tpz_gmm_fit(tpz_ctx* ctx, const float* d_x, size_t n, const double* pis, const double* splits, int n_init,
                double alpha, double beta, double scale, int num_iters, double tol, double* mus, double* stds,
                double* pis_out, double* logps);
/* tpz_gmm_fit with all initialisations advanced together: one pass over the pixels per EM iteration serves every
 * initialisation that has not converged yet (one launch pair, one download, one synchronise), instead of one pass per
 * initialisation and iteration.  Every initialisation's sums are accumulated in the order tpz_gmm_fit accumulates them, so the
 * four output arrays equal tpz_gmm_fit's bit for bit.  *n_passes (may be NULL) receives the number of passes over d_x:
 * at most num_iters + 3 (moments, hard split, first E-step, the EM iterations). */
int tpz_gmm_fit_fused(tpz_ctx* ctx, const float* d_x, size_t n, const double* pis, const double* splits, int n_init,
                      double alpha, double beta, double scale, int num_iters, double tol, double* mus, double* stds,
                      double* pis_out, double* logps, int* n_passes);
/* Exact order statistics: h_out[j] = the h_ranks[j]-th smallest (0-based) of the n device floats d_x, for 1 <= k <= 32 ranks in
 * one call -- what np.partition / np.quantile's bracketing elements are.  Radix select on the order-preserving integer key of a
 * float, four 8-bit digits, integer counts (independent of scheduling); -0 sorts before +0.  If any input is NaN every output
 * is NaN (np.quantile).  A rank outside [0, n) is an error.  h_ranks / h_out on the host; synchronises. */
int tpz_order_stats(tpz_ctx* ctx, const float* d_x, size_t n, const long long* h_ranks, int k, float* h_out);
/* d_out[i] = d_x[h_idx[i]], i < m: the sub-sample of `topaz normalize --sample`.  The m indices are on the host and uploaded by
 * the call; one outside [0, n) is an error, raised before anything is launched.  Asynchronous. */
int tpz_gather_f32(tpz_ctx* ctx, const float* d_x, size_t n, const long long* h_idx, size_t m, float* d_out);
/* y = (float)(((double)x - mean) / std): `(x - mu) / std` as numpy evaluates it for a float32 image and np.float64 scalars (the
 * mixture fit's mu and std) -- the float64 counterpart of tpz_normalize; std == 0 yields inf / nan.  Asynchronous. */
int tpz_normalize_f64(tpz_ctx* ctx, const float* d_x, size_t n, double mean, double std, float* d_y);
/* y = x*scale + shift  (the (x-mu)/std and std*y+mu steps of topaz/denoise.py:389,414) */
int tpz_affine(tpz_ctx* ctx, const float* d_x, size_t n, float scale, float shift, float* d_y);
/* y = (x - mean) / std evaluated as numpy does in `(mic - mu) / std` (topaz/denoise.py:389, :412 and commands/normalize):
 * fp32 subtraction, then an IEEE fp32 division -- exact low bits on raw-count micrographs (|mean| >> std); std == 0 yields the
 * reference's inf / nan. */
int tpz_normalize(tpz_ctx* ctx, const float* d_x, size_t n, float mean, float std, float* d_y);
/* tpz_normalize with the pixel cutoff of denoise_image fused (topaz/denoise.py:389-391): v = (x - mean) / std rounded as
 * tpz_normalize rounds it, then v = 0 where v < -cutoff or v > cutoff, compared in fp32 (what numpy >= 2 does for a float32
 * array and a Python float).  NaN passes through unchanged, +-inf (std == 0) is zeroed.  cutoff <= 0: no cutoff, the bytes of
 * tpz_normalize.  Asynchronous; one launch. */
int tpz_normalize_cutoff(tpz_ctx* ctx, const float* d_x, size_t n, float mean, float std, float cutoff, float* d_y);
/* d_out[i] = (float)d_raw[i] for n pixels in the type an MRC file of mode mrc_mode stores them in: 0 int8, 1 int16, 6 uint16,
 * 12 float16 (any other mode is an error).  All four conversions are exact: the result is the bits of numpy's
 * astype(np.float32), for float16 over all 65 536 patterns (subnormals become normal fp32 values, zeros and infinities keep
 * their sign, a NaN stays a NaN) whatever the float mode of the device, because it is done in integer arithmetic.  d_raw must be
 * 16-byte aligned (one 16-byte load per lane), d_out 4-byte (16-byte for the vector stores; otherwise a slower scalar loop).
 * n == 0 does nothing.  The buffers must not overlap.  Asynchronous; one launch. */
int tpz_decode(tpz_ctx* ctx, const void* d_raw, int mrc_mode, size_t n, float* d_out);
/* The other direction: n fp32 pixels at d_in become the pixels a file stores, at d_out, on the ctx stream.
 *   TPZ_ENC_F16  binary16 (MRC mode 12), 2 bytes per pixel: the bits of numpy's astype(np.float16) for EVERY fp32 input -- round
 *                to nearest, ties to even; half subnormals are produced, not flushed; |x| >= 65520 becomes +-inf; infinities and
 *                signed zeros are kept; a NaN becomes sign | (0x7c00 + (mantissa >> 13)), plus 1 where that would read as an
 *                infinity (npy_floatbits_to_halfbits).  Integer arithmetic on the bits, so no float mode of the device enters.
 *                params is ignored (may be NULL).  d_overflow: NULL, or a device unsigned long long to which the number of FINITE
 *                inputs stored as +-inf is ADDED (the caller zeroes it).
 *   TPZ_ENC_U8   one byte per pixel, params = {mi, ma} on the host: the bytes of numpy's
 *                round(clip(255 * (x - mi) / (ma - mi), 0, 255)).astype(uint8) on a float32 array -- every fp32 operation rounded
 *                on its own, in that order, IEEE division, ties to even; ma - mi is formed in fp32 from the fp32 params, so
 *                these are numpy's bytes when mi, ma and ma - mi are exact in fp32 (-3, 3: the pair of save_image).  NaN is
 *                stored as 0.  d_overflow is ignored.
 * Any other enc is an error.  d_in must be 4-byte aligned and d_out aligned to its pixel; when both are 16-byte aligned a lane
 * takes 16-byte loads and writes one 16-byte store (8 / 16 pixels), otherwise every pixel goes through a scalar loop.  Nothing
 * at d_out beyond n pixels is written.  n == 0 does nothing.  The buffers must not overlap.  Asynchronous; one launch. */
enum { TPZ_ENC_F16 = 12, TPZ_ENC_U8 = 8 };
int tpz_encode(tpz_ctx* ctx, const float* d_in, size_t n, int enc, const float* params, void* d_out,
               unsigned long long* d_overflow);
/* ---- score tiles: cut, test, paste (predict_in_patches on the device) ------- */
/* d_tile[z][y][x] = d_x[z0 + z][y0 + y][x0 + x] for the dense [td][th][tw] window of the dense fp32 tensor d_x[D][H][W] at origin
 * (z0, y0, x0); elements outside the tensor are written as +0.  D = td = 1, z0 = 0 for an image.  The origin may be negative and
 * the window may reach past the far faces or lie wholly outside (an all-zero tile): this is the zero padding of get_patches
 * (topaz/model/utils.py:133-169) without the padded copy of the tensor.  The pixels move as 32-bit words (NaN payloads, signed
 * zeros and subnormals are kept).  Groups of four x take one 16-byte load where the source address is 16-byte aligned and the
 * group lies inside the row, one 16-byte store where the tile address is; otherwise element by element -- any 4-byte aligned
 * pointers and any sizes are served.  Nothing outside the td * th * tw floats of d_tile is written.  Refused before anything
 * is launched: a null pointer, a size < 1, a tile of 2^31 elements or more (or a side above 2^30), an origin beyond +-2^29.
 * Asynchronous; one launch. */
int tpz_tile_cut(tpz_ctx* ctx, const float* d_x, int D, int H, int W, int z0, int y0, int x0, int td, int th, int tw,
                 float* d_tile);
/* d_flags[t] = 1 when the [td][th][tw] window of d_x[D][H][W] at origin h_origins[3 t .. 3 t + 2] = (z, y, x) holds an element
 * INSIDE the tensor that is != 0.0f, else 0, for t < n: torch's ne(0).any() of every tile of a grid at once (a NaN counts, -0.0
 * and what lies outside the tensor do not; a subnormal counts whatever the float mode, the test is on the bits).  The n origins
 * are on the host and uploaded by the call.  No atomics: whoever sees a non-zero element stores the constant 1.  n == 0 does
 * nothing.  Refusals as tpz_tile_cut's, and n >= 2^31.  Asynchronous (read d_flags after the stream); one launch. */
int tpz_tile_flags(tpz_ctx* ctx, const float* d_x, int D, int H, int W, const int* h_origins, size_t n, int td, int th, int tw,
                   unsigned* d_flags);
/* canvas[z + k][y + j][x + i] = d_tile[cz + k][cy + j][cx + i] for k < nz, j < ny, i < nx: the box [c, c + n) per axis of the dense
 * fp32 tile [td][th][tw] pasted into the dense canvas [D][H][W] at (z, y, x), clipped to the canvas (elements that would land
 * outside it are dropped; the position may be negative).  canvas_f64 == 0: an fp32 canvas, the words are copied; != 0: an fp64
 * canvas, each value converted (exactly).  16-byte accesses as in tpz_tile_cut, per group of four.  Nothing outside the pasted
 * box is written.  Refused before anything is launched: a null pointer, a size < 1, a box that is not inside the tile, a tile
 * of 2^31 elements or more, a position beyond +-2^29.  Asynchronous; one launch. */
int tpz_tile_paste(tpz_ctx* ctx, const float* d_tile, int td, int th, int tw, int cz, int cy, int cx, int nz, int ny, int nx,
                   void* d_canvas, int canvas_f64, int D, int H, int W, int z, int y, int x);
/* 1->1 channel 2-D filter with zero "same" padding: GaussianDenoise / InvGaussianFilter /
 * AffineFilter.forward (topaz/filters.py:28-96).  h_w is the [k][k] kernel on the host. */
int tpz_filter_2d(tpz_ctx* ctx, const float* d_in, int H, int W, const float* h_w, int k, float bias,
                  float* d_out);

/* ---- denoise pre-filters ---------------------------------------------------------------- */
/* lowpass(x, factor) of topaz/denoise.py:174-197 (2-D) as y = Qh (Qh^T x Qw) Qw^T: h_qh [H][rh] and h_qw [W][rw] (host, float64,
 * row-major) are orthonormal bases of the kept 1-D frequencies (topaz_amd/denoise.py builds them from the reference's masks).
 * Four GEMMs with fp64 operands and fp64 accumulation; y is rounded to fp32 once.  Asynchronous; four launches. */
int tpz_lowpass_2d(tpz_ctx* ctx, const float* d_in, int H, int W, const double* h_qh, int rh, const double* h_qw, int rw,
                   float* d_out);
/* spatial_covariance (topaz/denoise.py:22-49) of each of the P x P tiles of correct_spatial_covariance (:129-172; the first H % P
 * tile rows and W % P tile columns are one pixel longer, each tile is extended by a width/2 halo clipped at the image): h_cov
 * [P*P][width][width] float64, the lag products summed in fp64 in a fixed order (bit-identical run to run) and divided by the
 * size of the tile centre.  width must be 11 and every halo'd tile at least width x width.  Two launches; synchronises. */
int tpz_spatial_cov_2d(tpz_ctx* ctx, const float* d_x, int H, int W, int P, int width, double* h_cov);
/* the AffineFilter step of correct_spatial_covariance for all tiles at once: a zero-padded width x width cross-correlation of the
 * whole image where each pixel uses the fp32 weights h_w [P*P][width][width] (host) of its own tile; fp64 accumulation, one
 * rounding.  Same tile rules as tpz_spatial_cov_2d.  Asynchronous; one launch. */
int tpz_tile_filter_2d(tpz_ctx* ctx, const float* d_x, int H, int W, int P, int width, const float* h_w, float* d_out);

/* ---- particle stacks ------------------------------------------------------------------- */
/* replaces the per-particle loop of create_particle_stack (topaz/utils/picks.py:132-163) for the n picks of one micrograph:
 * d_img [mz][H][W], h_xy [n][2] int32 (x, y) on the host, d_out [n][mz][R][R] with R = resize (resize <= 0 or == size: R = size).
 * Each box (left = x - size/2, upper = y - size/2) is standardised over its in-bounds pixels of all mz frames as numpy's float32
 * (c - c.mean()) / c.std() (population std); pixels outside the image are 0, a box with zero variance is NaN, one that misses the
 * image on the high side all zeros.  A box with left + size < 0 or upper + size < 0 is refused before anything runs.
 * resize < size: every frame is resized by the separable truncated DFT and each particle standardised again over mz*R*R pixels;
 * h_ops (host, fp32) holds [2][size][R] column operators followed by the [R][2*size] row operator (topaz_amd/utils/picks.py
 * builds them from the float64 operators of utils/image.py).  Asynchronous; one launch per call (four with resize). */
int tpz_particle_stack(tpz_ctx* ctx, const float* d_img, int mz, int H, int W, const int32_t* h_xy, int n, int size, int resize,
                       const float* h_ops, float* d_out);

/* ---- non-maximum suppression ----------------------------------------------------------- */
/* replaces non_maximum_suppression(x, r, threshold) (topaz/algorithms.py:25-63), bit-identical
 * to the greedy loop including the clip-to-W quirk (offsets past the right edge suppress
 * column 0 of the next row).  Ties between equal scores are ordered by DESCENDING flat index
 * (what a stable argsort reversed gives; numpy's default argsort leaves tie order undefined).
 * Outputs (device): d_coords [cap][2] int32 (x, y), d_scores [cap] fp32, in descending score order.
 * *h_n receives the number of picks found (may exceed cap: then only cap rows were written
 * and the return code is non-zero).  Synchronises. */
int tpz_nms_2d(tpz_ctx* ctx, const float* d_score, int H, int W, int r, float threshold,
               int32_t* d_coords, float* d_scores, int cap, int* h_n);
/* replaces non_maximum_suppression_3d(x, r, scale, threshold) (topaz/algorithms.py:66-103):
 * flat-index deltas, no clipping (they wrap across rows/planes); d_coords [cap][3] (x, y, z). */
int tpz_nms_3d(tpz_ctx* ctx, const float* d_score, int D, int H, int W, int r, double scale,
               float threshold, int32_t* d_coords, float* d_scores, int cap, int* h_n);
/* (scale is a double: the reference forms r = scale * r in Python floats, and a lattice point at distance exactly r
 *  must stay inside the ball -- 0.7f * 10 is 6.9999998, 0.7 * 10 is 7.0.  The threshold is compared with fp32 scores
 *  as fp32, like numpy does for a float32 map.) */

/* ---- host buffers: staging ring and host-pointer entry points ----------------------------------------------
 * The reference's callers own numpy images (extract.py:234-251 loads one, scores it, hands the map on; denoise.py:463-488
 * likewise).  A tpz_stage is a ring of `depth` slots -- pinned host buffer + device buffer + events -- with its own copy
 * stream: the H2D copy of image i+1 and the D2H copy of result i-1 run under the kernels of image i.
 *   producer:  p = tpz_stage_host_ptr(st, k);  fill p (e.g. read the file into it);  tpz_stage_h2d(st, k, NULL, bytes)
 *              (or tpz_stage_h2d(st, k, h_src, bytes): h_src is first copied into the pinned buffer)
 *   consumer:  tpz_stage_acquire(st, k)  -- the ctx stream waits for the copy (no host wait);
 *              ... kernels reading tpz_stage_device_ptr(st, k) ...;  tpz_stage_release(st, k)
 *   results:   tpz_stage_d2h(st, k, d_src, bytes) queues device -> pinned slot k after the work already on the ctx stream;
 *              tpz_stage_wait(st, k) blocks the host until slot k's last copy has finished.
 * A slot is reused only after the kernels that read it were released (h2d waits for the release event). */
typedef struct tpz_stage tpz_stage;
int tpz_stage_create(tpz_ctx* ctx, size_t slot_bytes, int depth, tpz_stage** out);
void tpz_stage_free(tpz_stage* st);
void* tpz_stage_host_ptr(tpz_stage* st, int slot);
void* tpz_stage_device_ptr(tpz_stage* st, int slot);
int tpz_stage_h2d(tpz_stage* st, int slot, const void* h_src, size_t bytes);
int tpz_stage_acquire(tpz_stage* st, int slot);
int tpz_stage_release(tpz_stage* st, int slot);
int tpz_stage_d2h(tpz_stage* st, int slot, const void* d_src, size_t bytes);
int tpz_stage_wait(tpz_stage* st, int slot);
/* tpz_stage_h2d for an image whose pixels lie in the slot's pinned buffer in the type the file stores them in (mrc_mode 0, 1, 6
 * or 12: see tpz_decode): the n * itemsize stored bytes are copied to a raw region of the slot's device buffer, BEHIND the fp32
 * image (at the next multiple of 256 bytes after 4 * n), decoded into the start of the slot by tpz_decode's kernel on the copy
 * stream, and only then is the slot's copy event recorded.  tpz_stage_acquire / tpz_stage_device_ptr and every consumer see
 * what they see after tpz_stage_h2d -- n fp32 pixels at the start of the slot -- while a quarter or half of the bytes crossed
 * the bus and the host converted nothing.  The slot must hold tpz_stage_decode_bytes(mrc_mode, n) bytes (4 * n rounded up to
 * 256, plus the stored bytes rounded up to 256; 0 for a mode that is not decoded).  The launch is not counted by
 * tpz_prof_launches (it is not on the ctx stream). */
size_t tpz_stage_decode_bytes(int mrc_mode, size_t n);
int tpz_stage_h2d_decode(tpz_stage* st, int slot, int mrc_mode, size_t n);
/* The mirror image on the way out: tpz_stage_d2h for a result that is stored as float16 or as bytes (enc, params: tpz_encode).
 * `produced` is recorded on the ctx stream; the copy stream waits for it, clears the slot's 8-byte overflow counter, encodes the
 * n fp32 pixels at d_src into the slot's DEVICE buffer -- encoded pixels at its start, the counter (unsigned long long) at the
 * next multiple of 256 bytes -- and brings pixels and counter into the pinned buffer with one copy, at the same offsets; then
 * the slot's copy event is recorded.  After tpz_stage_wait the pinned slot holds the encoded pixels and the counter: half or a
 * quarter of the bytes crossed the bus and the host converted nothing.  The slot must hold tpz_stage_encode_bytes(enc, n) bytes
 * (the pixels rounded up to 256, plus 256; 0 for an unknown enc).  An unknown enc, a slot that is too small or a NULL pointer
 * is an error and queues nothing.  The launch is not counted by tpz_prof_launches (it is not on the ctx stream). */
size_t tpz_stage_encode_bytes(int enc, size_t n);
int tpz_stage_d2h_encode(tpz_stage* st, int slot, const float* d_src, size_t n, int enc, const float* params);
/* Host-pointer forms of the three calls of the path (synchronous; plain pageable or pinned memory), the signatures
 * SURVEY.md 8(b) sketches: model(x) on a numpy image (extract.py:247-249), Denoise.denoise (denoise.py:327-332),
 * non_maximum_suppression (algorithms.py:25-63).  Each stages through an internal ring owned by the ctx. */
int tpz_score_2d_host(tpz_model* m, const float* h_in, int H, int W, float* h_out_logits);
int tpz_denoise_2d_host(tpz_model* m, const float* h_in, int H, int W, int patch, int pad, float* h_out);
int tpz_nms_2d_host(tpz_ctx* ctx, const float* h_score, int H, int W, int r, float threshold, int32_t* h_coords,
                    float* h_scores, int cap, int* h_n);

/* ---- single ops (unit tests and the host-side pipelines) --------------------------------- */
/* one fused convolution: the op the layer program is made of.  h_w [cout][cin][k..], h_b [cout] or NULL.
 * d_in2 / d_res / h_post_* may be NULL.  in is [cin1][D1][H1][W1]; when d_in2 != NULL it is
 * nearest-upsampled to in2's [cin-cin1][D][H][W] and concatenated. */
int tpz_conv(tpz_ctx* ctx, int dims, const float* d_in, int cin1, int D1, int H1, int W1, const float* d_in2,
             int cin, int D, int H, int W, const float* h_w, const float* h_b, int cout, int k, int dil,
             int pad, float slope, const float* d_res, int res_crop, const float* h_post_scale,
             const float* h_post_shift, const float* h_head_w, float head_b, float* d_out);
int tpz_maxpool2(tpz_ctx* ctx, int dims, const float* d_in, int C, int D, int H, int W, float* d_out);
/* one padded 3^dims pool as the layer program runs it: op = TPZ_OP_MAXPOOL (window dilated by dil, pad <= dil elements of -inf
 * padding) or TPZ_OP_AVGPOOL (dil = 1, pad = 1).  d_in [C][D][H][W] -> d_out [C][Do][Ho][Wo], Xo = X + 2 * pad - 2 * dil.
 * split = 0: the fp32-plane kernel; split = 1: d_in is converted to split f16 cells, pooled by the split-cell kernel and converted
 * back (values beyond the f16 range do not survive that: *overflow = 1, may be NULL).  Synchronises. */
int tpz_pool(tpz_ctx* ctx, int op, int dims, const float* d_in, int C, int D, int H, int W, int dil, int pad, int split,
             float* d_out, int* overflow);
/* d_out[cols][rows] = d_in[rows][cols] (the truncated-DFT downsample that once ran as two tpz_conv GEMMs around it is
 * tpz_resample_* now) */
int tpz_transpose_2d(tpz_ctx* ctx, const float* d_in, int rows, int cols, float* d_out);

/* ---- truncated-DFT resampler ---------------------------------------------------------------- */
/* replaces downsample(x, factor, shape) (topaz/utils/image.py:38-61: rfft2 -> keep the m x (n/2+1) low-frequency block -> scale ->
 * irfft2), the first half of `topaz preprocess`.  That is a real-linear, separable map of the M x N image:
 *     U = L x  (2m x N; L = [Re Lc; Im Lc], Lc the complex m x M row operator),   y = Re(U) R1 + Im(U) R2  (m x n),
 * two fp32 GEMMs on the matrix cores (fp32 operands, fp32 accumulation: micrographs are detector counts).  A plan keeps the two
 * operators of one shape on the device:
 *   create  h_L [2m][M] and h_R [n][2N] (= [R1; R2] transposed) on the host, fp32, row-major (topaz_amd/utils/image.py builds
 *           them in float64 with numpy's own FFT); packed and uploaded once.  1 <= m <= M, 1 <= n <= N.  Synchronous.
 *   run     d_in [M][N] -> d_out [m][n], dense device arrays that must not overlap; two launches on the ctx stream, the
 *           intermediate from the ctx workspace: no host packing, no operator upload, no synchronise.  Bit-identical run to run.
 *   free    waits for the ctx stream (runs already enqueued still read the operators), then releases the plan.  A plan must be
 *           freed before its ctx is destroyed.
 * tpz_resample_2d_host: run on host arrays h_in [M][N] -> h_out [m][n] through the ctx's staging ring (synchronous).
 * tpz_resample_upload_bytes: operator bytes this ctx has uploaded in all its tpz_resample_create calls so far -- a run on an
 * existing plan leaves it unchanged. */
typedef struct tpz_resample tpz_resample;
int tpz_resample_create(tpz_ctx* ctx, int M, int N, int m, int n, const float* h_L, const float* h_R, tpz_resample** out);
int tpz_resample_run(tpz_resample* plan, const float* d_in, float* d_out);
void tpz_resample_free(tpz_resample* plan);
int tpz_resample_shape(tpz_resample* plan, int* M, int* N, int* m, int* n);
int tpz_resample_2d_host(tpz_resample* plan, const float* h_in, float* h_out);
long long tpz_resample_upload_bytes(tpz_ctx* ctx);

/* ---- introspection / measurement --------------------------------------------------------- */
/* ---- 2xf16 path.  Every convolution with a conv_split kernel -- the scoring networks (stem as a column kernel, dilated
 * 3x3 / 5x5 layers, folded 1x1 projections, fused head), the 2-D U-Nets / FCNN (encoders with fused max-pool, per-parity and
 * sub-pixel decoders, the 1-output-channel last conv as a column kernel) and the 3-D U-Net (plane-stacked) -- runs by default on
 * the f16 matrix cores with every fp32 operand carried as two f16 halves and three exact products accumulated in fp32
 * (topaz_amd/csrc/conv_split.h): fp32-level accuracy at several times the fp32-MFMA rate.  The rule per layer: it takes the 2xf16
 * path when a conv_split kernel exists for its shape (2-D and plane-stacked 3-D alike: the 3-D scoring networks run there too),
 * otherwise it stays on its fp32-MFMA kernel; layers with a PReLU slope > 1 always do.  An activation beyond the f16 range is detected on the device and that
 * image is re-run on the fp32 kernels, so results never depend on the range.  tpz_ctx_set_exact(ctx, 1) pins the
 * fp32 kernels.
 * tpz_model_split_stats: whether the model is eligible, images finished on the 2xf16 path, images re-run in fp32. */
int tpz_ctx_set_exact(tpz_ctx* ctx, int on);
/* Debug switches.  The library's A/B switches (TPZ_NO_ROI, TPZ_EXACT_FP32, TPZ_NO_LANES, ... -- the list is the DebugEnv struct of
 * topaz_amd/csrc/rt_internal.h) exist for tools/ and tests/; a variable left in a user's environment must not change how a job
 * computes, so the library reads them in ONE function and only when TPZ_DEBUG=1 is set as well.  tpz_debug_switches writes the
 * space-separated names of the switches that are in effect right now into buf ("" when none: always so without TPZ_DEBUG=1)
 * and returns their number.  Needs no device. */
int tpz_debug_switches(char* buf, int buf_len);
/* Range scaling of the scoring pass (tpz_model_forward of a program that ends in the linear head), on by default
 * (on = 0: off).  `topaz extract` scores micrographs as they come (topaz/extract.py:234-249 does not normalise), and
 * a raw-count image (mean 10^3 .. 10^4) would leave the f16 range in the very first layer and send the whole image to the fp32
 * kernels.  A scoring network is positively homogeneous in (input, biases) jointly -- convolutions, PReLU / ReLU, max-pools,
 * residual adds, eval-BN affines, the linear head --, so it is run on x * 2^-s with every bias-like vector scaled by 2^-s and its
 * logits multiplied by 2^s: exact (powers of two).  s >= 0 brings the 99.9 % quantile of |x| (from an exponent histogram taken on
 * the device, no host round trip) to ~8: the bulk of the image decides, so a hot pixel cannot push the rest towards the f16
 * subnormals -- it either still fits the f16 range or trips the overflow flag and the image is re-run in fp32.  A normalised image
 * has s = 0 and runs unchanged, bit for bit. */
int tpz_ctx_set_range(tpz_ctx* ctx, int on);
/* Patch lanes: tpz_denoise_2d / _3d enqueue the independent patches / tiles of an image alternately on two auxiliary
 * streams (own workspace each), so that one patch's small, latency-bound launches run under its neighbour's large ones.
 * On by default (on = 0 here: everything on the ctx stream, e.g. to time kernels in
 * isolation).  on = 2 .. 4: that many lanes; more than two measured no gain on the 4096^2 pipeline
 * (profiles/r03_lanes.txt).  Results are bit-identical either way. */
int tpz_ctx_set_lanes(tpz_ctx* ctx, int on);
/* Batched patches (2xf16 path): tpz_denoise_2d / _3d record the launches of up to n (<= 8) independent patches / tiles and issue
 * them layer by layer, the same layer of all n as ONE grid (conv_split_multi_kernel): the deep levels of a U-Net are 16-tile
 * launches on a 256-CU chip, ~400 of them per micrograph (denoise.py:299-323 runs the patches one after another).  Consecutive
 * batches alternate on the patch lanes above (a batch's elementwise launches and small grids run under the other batch's large
 * ones: profiles/r04_batch_lanes_ab.txt).  Default n = 8; n = 0: off -- single
 * patches then alternate on the lanes, as do the fp32 kernels (exact mode, overflow re-run) always.  Results are bit-identical
 * either way.
 * Every image of a batch has a workspace of its own and two batches are in flight: the batch is cut to what fits 90 % of the
 * free device memory (tpz_ctx_set_batch_memory(ctx, bytes): that many bytes instead; 0 = automatic), below 2 the pass falls
 * back to single patches on the lanes -- a large tile costs launches, not an out-of-memory error.
 * tpz_prof_launches: kernel launches the library has issued on this context (convolutions, elementwise, NMS sweeps excluded).
 * tpz_ctx_pool_stats: the workspace buffers all pools of the context cache (the ctx pool, the patch lanes', those of the batched
 * passes), their bytes, and how many are marked in use -- 0 between calls; any out pointer may be NULL. */
int tpz_ctx_set_batch(tpz_ctx* ctx, int n);
int tpz_ctx_set_batch_memory(tpz_ctx* ctx, long long bytes);
long long tpz_prof_launches(tpz_ctx* ctx);
int tpz_ctx_pool_stats(tpz_ctx* ctx, long long* buffers, long long* bytes, long long* buffers_in_use);
/* Poisoned workspace, for tests (default off; with TPZ_DEBUG=1: TPZ_POISON=1).  The workspace pools hand the same buffers to the
 * same sequence of requests and never clear them, so a cell that a kernel fails to write reads back as what the previous run left
 * there.  on = 1: every temporary buffer the library takes is filled whole (its size in the pool, whole MiB) with 0xFF bytes before
 * anything can touch it -- every f16 / f32 / f64 a NaN, every 64-bit key the maximum, every int -1 --, ordered on the stream (or in
 * the recorded batch) that orders the consumer's launches.  The fills count neither in tpz_prof_launches nor in the profiler.
 * tpz_ctx_poison_stats: whether the switch is on, the fills made and the bytes filled since the context was created; any out
 *   pointer may be NULL.
 * tpz_ctx_walk_stats: the 2xf16 conv launches issued since the context was created, by tile walk: out[0] one workgroup per tile
 *   in row-major / XCD order, [1] the patch raster, [2] persistent workgroups, [3] the weights-resident kernel, [4] the batched grid
 *   of several images.
 * tpz_debug_workspace_peek: takes a temporary buffer of `bytes` from the context's pool as a driver would, waits for the stream,
 *   copies the buffer's first `bytes` rounded up to a whole MiB to host_out (which must have that much room) and gives the buffer
 *   back: what a kernel would find there. */
int tpz_ctx_set_poison(tpz_ctx* ctx, int on);
int tpz_ctx_poison_stats(tpz_ctx* ctx, int* on, long long* fills, long long* bytes);
int tpz_ctx_walk_stats(tpz_ctx* ctx, long long out[5]);
int tpz_debug_workspace_peek(tpz_ctx* ctx, size_t bytes, void* host_out);
/* Patch windows: a patch of tpz_denoise_2d keeps only its centre (topaz/denoise.py:299-323: patch_size pixels of a
 * patch_size + 2*padding tile), so each layer computes only the rectangle of its tensor that those pixels depend on (the
 * U-Net's receptive field is ~230 pixels, the CLI's default padding 500).  The statistics of the normalisation are still the
 * whole padded patch's; every kept pixel is computed exactly as before -- the output is bit-identical with the switch off
 * (on = 0 here).  Both paths: the 2xf16 kernels and, under tpz_ctx_set_exact, the fp32 ones.
 * The tiles of tpz_denoise_3d (denoise.py:340-377: patch^3 voxels kept of a (patch + 2*padding)^3 tile, 1/8 at the CLI's 96 / 48)
 * are windowed the same way with boxes, on the 2xf16 kernels and (round 5) on the fp32 kernels of exact mode / an overflow
 * re-run: 3.5x on a 512x512x256 tomogram, bit-identical. */
int tpz_ctx_set_roi(tpz_ctx* ctx, int on);
/* The 3x3 32 -> 32 layers of the 32-unit detectors (resnet8_u32 / resnet16_u32: topaz/model/features/resnet.py:108-204 filled)
 * run on a persistent kernel that keeps the layer's packed weights in the LDS (csrc/conv_rw.h); on = 0 (with TPZ_DEBUG=1: TPZ_NO_RW=1 at load
 * time) sends them to the general 2xf16 tile again.  Same tensors either side; results agree to rounding (another summation
 * order), each within 1e-4 of the reference. */
int tpz_ctx_set_rw(tpz_ctx* ctx, int on);
/* Persistent workgroups of the 2xf16 convolutions (conv_split.h, MODE 4): a plain single-source layer with several tiles per
 * workgroup slot is launched as CUs x workgroups-per-CU workgroups that walk the tiles and fetch the first chunk of their next
 * tile under the last chunk of the current one.  mode 0: never, 1: large launches outside the patch lanes
 * (default), 2: every eligible launch, with `workgroups` of them (0: one grid slot each) -- the form the tests use to run
 * small images through many tiles per workgroup.  Results are bit-identical in every mode. */
int tpz_ctx_set_persist(tpz_ctx* ctx, int mode, int workgroups);
/* Patch raster of the large 8-wave launches (conv_split.h, xcd_swizzle 2): the 32 tiles an XCD's CUs hold at a time form an
 * 8 x 4 block of neighbouring tiles (rows taken phase-major for dilated layers), so that their halos overlap in that XCD's L2,
 * instead of a row-major run that shares columns only.  On by default (on = 0: row-major runs).  Same
 * arithmetic per tile: results are bit-identical. */
int tpz_ctx_set_raster(tpz_ctx* ctx, int on);
/* Internal tiling of tpz_model_forward: a 2-D image of more than limit_px pixels (default 40 Mi: beyond a 6400^2 frame) through a
 * size-preserving scoring network is scored in tile x tile tiles (default 4096), each computed on the tile grown by the network's
 * receptive halo and stitched -- where the reference scores any image that fits memory (topaz/extract.py:247-249), the kernels
 * address 32-bit byte offsets per chunk of cells (< ~11 500^2 pixels) and a whole-image pass would hold every activation at full
 * size (an 11 520 x 8 184 super-resolution frame: 146 GB).  Bit-identical to the whole-image pass. */
int tpz_ctx_set_tiling(tpz_ctx* ctx, long long limit_px, int tile);
int tpz_model_split_stats(tpz_model* m, int* eligible, long long* split_runs, long long* fp32_reruns);
/* ---- precision check of a loaded model.  The 2xf16 path multiplies 22-bit operands; how far that leaves a given model from its
 * own fp32 result depends on its weights, and a user-trained model is untested by construction.
 * tpz_delta_stats: one streaming pass over two fp32 device arrays of n >= 1 elements (n = 0 is an error): max_abs_delta = max
 *   |a[i] - b[i]| in fp32 with every non-finite difference (a NaN either side, inf - inf) counted as +inf, argmax = the smallest
 *   flat index that attains it, max_abs_ref = max |b[i]| (NaN: +inf), sum_sq = the fp64 sum of (a[i] - b[i])^2.  Deterministic
 *   (fixed reduction order, a grid chosen from n alone).  Synchronises.
 * tpz_model_calibrate: one image d_in [D][H][W] (D = 1 in 2-D) through the model twice -- on the 2xf16 path exactly as
 *   tpz_model_forward would run it (range scaling included), then on the fp32 kernels as under tpz_ctx_set_exact -- and
 *   tpz_delta_stats of (2xf16 output, fp32 output) in d, rms_delta = sqrt(sum_sq / n).  eligible = 0 (and zeros) for a model
 *   without a 2xf16 path; overflow = 1 (and no comparison) when the image left the f16 range, which the runtime re-runs in fp32
 *   anyway.  With bar > 0, a max_abs_delta above it (or not finite) sets the model's exact flag and tripped = 1; bar <= 0 only
 *   measures.  The counters of tpz_model_split_stats, the context's exact flag and its workspace are left as they were.  Never
 *   called implicitly.
 * tpz_model_set_exact: the per-model twin of tpz_ctx_set_exact -- the model is never tried on the 2xf16 path (scoring and
 *   denoising alike; neither counter of tpz_model_split_stats moves); other models of the context are unaffected. */
typedef struct tpz_delta { float max_abs_delta, max_abs_ref; long long argmax; double sum_sq; } tpz_delta;
typedef struct tpz_calibration { int eligible, overflow, tripped; tpz_delta d; double rms_delta; } tpz_calibration;
int tpz_delta_stats(tpz_ctx* ctx, const float* d_a, const float* d_b, size_t n, tpz_delta* out);
int tpz_model_calibrate(tpz_model* m, const float* d_in, int D, int H, int W, float bar, tpz_calibration* out);
int tpz_model_set_exact(tpz_model* m, int on);
int tpz_model_get_exact(tpz_model* m, int* on);
/* Coverage of the 2xf16 path: convolution layers of the model, how many of them have a 2xf16 kernel, and the others as text
 * ("#layer KxK dD cin->cout, ...").  `eligible` above is true as soon as ONE layer has: the rest of a mixed program runs on its
 * fp32 kernels (correct, converted either side, several times slower) -- topaz_amd warns once per model when that happens. */
int tpz_model_split_layers(tpz_model* m, int* n_conv, int* n_split, char* off_path, int off_path_len);
/* One 2-D convolution on the 2xf16 kernels with fp32 [C][H][W] tensors at the boundary (converted on the device):
 * unit-test / interop entry; arguments as tpz_conv (single source).  *overflow = 1 when a result left the f16 range. */
int tpz_conv_split_2d(tpz_ctx* ctx, const float* d_in, int cin, int H, int W, const float* h_w, const float* h_b,
                      int cout, int k, int dil, int pad, float slope, const float* d_res, int res_crop,
                      const float* h_post_scale, const float* h_post_shift, const float* h_head_w, float head_b,
                      float* d_out, int* overflow);

/* time (ms, HIP events on the ctx stream) and launch count of the kernels of one class since
 * the last reset.  cls: 0 = conv_mfma, 1 = conv_direct, 2 = elementwise, 3 = nms.
 * Timing is only collected while enabled (it adds two event records per timed launch): on = 1 times every launch,
 * on = 2 only the convolution launches of >= 20 GFLOP (cheap enough to stay enabled during a benchmark's timed steps). */
int tpz_prof_enable(tpz_ctx* ctx, int on);
int tpz_prof_reset(tpz_ctx* ctx);
int tpz_prof_get(tpz_ctx* ctx, int cls, double* ms, long long* launches, double* flops);
/* the conv_mfma instantiation with the largest accumulated time since the last reset: total ms, launch count,
 * algorithmic FLOP of those launches and its template parameters as text (matches the rocprofv3 kernel name) */
int tpz_prof_get_dominant(tpz_ctx* ctx, double* ms, long long* launches, double* flops, char* name, int name_len);
/* the same for the rank-th instantiation by accumulated time (rank 0 = the dominant one); an empty name and zeros
 * once rank runs past the instantiations that were launched */
int tpz_prof_get_kernel(tpz_ctx* ctx, int rank, double* ms, long long* launches, double* flops, char* name,
                        int name_len);
/* algorithmic HBM bytes (inputs with halo + weights read once, outputs written once) of the launches behind
 * tpz_prof_get_kernel(rank): the bandwidth of the kernels that are HBM-bound rather than MFMA-bound */
int tpz_prof_get_kernel_bytes(tpz_ctx* ctx, int rank, double* bytes);
/* The matrix-pipe rate this board sustains (diagnostic, no reference counterpart): a register-resident loop of
 * v_mfma_f32_16x16x32_f16 -- the instruction of the 2xf16 kernels -- on every SIMD for about `ms` milliseconds, operands
 * uniform in [-1, 1] (zero_operands = 0) or all zero (1).  *tflops = dense f16 TFLOP/s (3 such products make one fp32-equivalent
 * multiply-add on the 2xf16 path); *clock_ratio = s_memtime / s_memrealtime ticks over the loop (proportional to the shader
 * clock; may be NULL).  With full-entropy operands the power management holds the clock well below the 2.4 GHz the dense peak
 * is quoted at: bench.py reports the dominant kernel against both. */
int tpz_prof_mfma_sustained(tpz_ctx* ctx, int ms, int zero_operands, double* tflops, double* clock_ratio);

/* ---- pick-table text (host only) ------------------------------------------------------------------------------------
 * replaces the per-pick f-string of topaz/extract.py:341-354: n rows `image_name \t x \t y [\t z] \t score \n` into `out`
 * (capacity `cap` bytes; strlen(image_name) + 80 per row is always enough).  coords: int32, `coord_stride` ints per row of
 * which the first `dims` are written; a float32 score prints as Python prints float(score): the shortest digits that
 * round-trip the float64 value (repr).  Returns the bytes written, -1 on bad arguments, -2 when `out` is too small. */
long long tpz_format_picks(const char* image_name, const int32_t* coords, int coord_stride, int dims, const float* scores,
                           long long n, char* out, long long cap);

#ifdef __cplusplus
}
#endif
#endif /* TOPAZ_HIP_H */
