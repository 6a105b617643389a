/*
 * ipdm.h -- C ABI of libipdm.so: the MI355X (gfx950) kernels of the Annealed-Langevin-Dynamics
 * reconstruction hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 * a parameter is documented as host.  All launches are asynchronous on `stream` (a hipStream_t cast
 * to void*; NULL = the default stream), allocate nothing and never synchronise, so a caller may
 * capture any sequence of them into a hipGraph.
 *
 * Return value: 0 on success; a positive hipError_t if the runtime rejected a launch; a negative
 * IPDM_E* code if the arguments were rejected before anything was launched.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the ctypes / pybind stub a reference maintainer would add.
 *
 * Layouts: images are NCHW planar, row-major, float32.  Complex data is interleaved (re, im)
 * float32 pairs ("c64"), the memory layout of torch.complex64 / numpy.complex64.
 *
 * Alignment: every tensor argument may be any contiguous buffer on its element's natural boundary (4 bytes for float32, 8 for
 * c64 and int64 / double, 2 for half); 16-byte alignment only selects faster kernel forms, never a different result beyond
 * rounding order.  No entry answers a misaligned tensor with IPDM_EINVAL.  Exceptions, answered with IPDM_EUNSUPPORTED (the
 * caller takes its other path, as for an unsupported shape): ipdm_conv3x3_thin_f32 and the 1-D Winograd entries
 * (ipdm_conv2d_wino1d_*, ipdm_conv3d_wino1d_f32) need `x` on 16 bytes; the Winograd entries whose epilogue moves pairs of columns
 * (ipdm_conv2d_wino_f32, ipdm_conv2d_wino_{bx3,hx2}_f32 and _stats_f32 -- the pooled form included, for one rule per entry --
 * and the 1-D ones) need `residual`, `out` and `out_act` on 8 bytes; the split-K entries (ipdm_conv2d_wino_*_splitk_f32) finish
 * in a scalar reduction and take them at any alignment.  Packed weight blobs come from the pack functions into 16-byte aligned
 * buffers and are not covered by the relaxation.
 */
#ifndef IPDM_H
#define IPDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPDM_OK 0
#define IPDM_EINVAL (-1)       /* bad size / NULL pointer / unsupported combination            */
#define IPDM_EUNSUPPORTED (-2) /* valid request this build has no kernel for (size limits)     */

/* activation codes used by the fused normalisation / convolution prologues */
#define IPDM_ACT_NONE 0
#define IPDM_ACT_ELU 1
#define IPDM_ACT_RELU 2
#define IPDM_ACT_LRELU02 3
#define IPDM_ACT_SWISH 4
#define IPDM_ACT_COPY 5           /* identity, as an `act_out` code: "produce the second output without an activation" (with
                                     ipdm_conv_ext_t.res_second: out = conv, out_act = conv + residual) */

/* "maxima vectors": per-image max |x| of an activation tensor (or an upper bound of it), what the f16x2 convolutions take as
 * `in_amax` (dynamic range) and what producers hand over (`out_amax`, `act_amax`, `amax_out`, `amax_bound` below).  Layout:
 * [B][IPDM_AMAX_SLOT] floats, 8 ways per image at a stride of 16 floats (one 64-byte line each: memory-side atomics serialise per
 * line); the value of an image is the max over its ways.  Atomic producers need the whole vector ZEROED by the caller;
 * ipdm_absmax_f32 and the coefficient kernels write every way themselves. */
#define IPDM_AMAX_WAYS 8
#define IPDM_AMAX_SLOT 128

/* library identification: returns IPDM_ABI_VERSION, writes the gfx arch string the kernels were built for */
#define IPDM_ABI_VERSION 4
int ipdm_abi_version(void);
const char* ipdm_build_arch(void);

/* ------------------------------------------------------------------------------------------------
 * StyleGAN2 resampling ops (reference: op/upfirdn2d.cpp:12-23 `upfirdn2d`, kernels
 * op/upfirdn2d_kernel.cu:49-369; op/fused_bias_act.cpp:11-21 `fused_bias_act`, kernel
 * op/fused_bias_act_kernel.cu:19-99).
 * ---------------------------------------------------------------------------------------------- */

/* in [major][in_h][in_w][minor] -> out [major][out_h][out_w][minor],
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kernel_h)/down_y + 1 (likewise out_w); zero-insert upsample,
 * pad (negative pad crops), correlate with the FLIPPED kernel, decimate.  kernel [kernel_h][kernel_w]. */
int ipdm_upfirdn2d_f32(const float* in, const float* kernel, float* out,
                       int major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                       int up_x, int up_y, int down_x, int down_y,
                       int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* the other storage types of the reference's dispatch (AT_DISPATCH_FLOATING_TYPES_AND_HALF, op/upfirdn2d_kernel.cu:311):
 * IEEE half (2-byte elements behind the void pointers; fp32 arithmetic, one rounding at the store) and double */
int ipdm_upfirdn2d_f16(const void* in, const void* kernel, void* out,
                       int major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                       int up_x, int up_y, int down_x, int down_y,
                       int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
int ipdm_upfirdn2d_f64(const double* in, const double* kernel, double* out,
                       int major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                       int up_x, int up_y, int down_x, int down_y,
                       int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* y[i] = act(x[i] + b[(i / step_b) % size_b]) * scale;  act*10+grad as in the reference kernel:
 * 10/11 linear, 12 zero, 30 leaky-relu(alpha), 31 leaky-relu gradient gated by ref, 32 zero.
 * b == NULL or size_b == 0: no bias.  ref == NULL: treated as zeros. */
int ipdm_fused_bias_act_f32(const float* x, const float* b, const float* ref, float* y,
                            int64_t n, int step_b, int size_b, int act, int grad,
                            float alpha, float scale, void* stream);
/* half / double storage (op/fused_bias_act_kernel.cu:79 dispatches the same three types) */
int ipdm_fused_bias_act_f16(const void* x, const void* b, const void* ref, void* y,
                            int64_t n, int step_b, int size_b, int act, int grad,
                            float alpha, float scale, void* stream);
int ipdm_fused_bias_act_f64(const double* x, const double* b, const double* ref, double* y,
                            int64_t n, int step_b, int size_b, int act, int grad,
                            float alpha, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * k-space operators (reference: ncsn/linear_transforms/__init__.py:36-57 i2k_complex/k2i_complex;
 * ncsn/linear_transforms/undersampling_fourier.py:77-97 RandomUndersamplingFourier,
 * :140-170 SENSE.__call__/conj_op/SSOS; ncsn/models/proximal_op.py:19-51 L2Penalty, :72-94 SingleCoil).
 * mask is uint8 [mask_t][W] (1 = sampled k-space column); mask_t == 1 broadcasts over the batch,
 * otherwise image b uses row b % mask_t (the reference's (T,1,1,W) broadcast against a (T,1,H,W) stack).
 * A NEGATIVE mask_t = -T announces a 2-D mask, uint8 [T][H][W] (1 = sampled k-space sample: variable-density
 * (ky, kz) patterns, partial Fourier, elliptical shutters, ...; the reference's (T,1,H,W) mask); T == 1 broadcasts
 * over the batch, otherwise image b uses plane b % T.  Every entry point below that takes (mask, mask_t) accepts
 * both layouts (ipdm_mask_layouts() & IPDM_MASK_2D; older builds return IPDM_EINVAL for mask_t < 0); mask_t == 0 is
 * invalid.  A mask only selects samples: no arithmetic, normalisation included, depends on the layout.
 * sens maps are float32 [n_coils][H][W] (real, as the reference's "exp" maps).
 * ---------------------------------------------------------------------------------------------- */

/* centred orthonormal 2-D DFT of `batch` images [H][W] c64; inverse != 0 -> k2i_complex.  Any H, W
 * in [1, 1024] (this entry point's own limit: a served side above 1024 is IPDM_EINVAL here, though the SENSE operators
 * take it); served sizes (ipdm_kspace_size_class) take the FFT kernels, the rest an O(N^2) direct DFT. in may equal out. */
int ipdm_fft2c_c64(const float* in, float* out, int batch, int H, int W, int inverse,
                   float* workspace /* batch*H*W c64, only for the non-LDS path; may be NULL otherwise */,
                   void* stream);
/* bytes of workspace ipdm_fft2c_c64 needs for (batch,H,W); 0 for a served size (the direct DFT is not used) */
int64_t ipdm_fft2c_workspace_bytes(int batch, int H, int W);

/* mask layouts the (mask, mask_t) entry points accept: IPDM_MASK_LINES | IPDM_MASK_2D */
#define IPDM_MASK_LINES 1 /* mask_t > 0: uint8 [mask_t][W] */
#define IPDM_MASK_2D 2    /* mask_t < 0: uint8 [-mask_t][H][W] */
int ipdm_mask_layouts(void);

/* Image sizes the k-space kernels serve.  A side N is served when it is a power of two from 4, or N = 2^a 3^b 5^c with
 * a >= 4 (a multiple of 16) and 16 <= N <= 2048; a pair (H, W) may mix served sides freely (one exception: 8x2000 and
 * 2000x8 have no kernel).
 *   IPDM_KSPACE_LDS     H*W <= 16384: the whole image in one CU's LDS
 *   IPDM_KSPACE_STRIPS  larger, sides up to 2048: row / column FFT passes over strips
 *   IPDM_KSPACE_NONE    no kernel: the SENSE / single-coil / CG entry points return IPDM_EUNSUPPORTED (odd sides, a factor
 *                       7 or larger, multiples of 8 that are not multiples of 16), ipdm_fft2c_c64 falls back to a direct DFT */
#define IPDM_KSPACE_NONE 0
#define IPDM_KSPACE_LDS 1
#define IPDM_KSPACE_STRIPS 2
int ipdm_kspace_size_class(int H, int W);

/* y[c][b] = mask * fft2c(S_c * x[b])        x [B][H][W] c64 -> y [n_coils][B][H][W] c64 */
/* (sens == NULL with n_coils == 1: the single-coil operator RandomUndersamplingFourier.__call__, y = M F x,
 *  undersampling_fourier.py:77-82) */
int ipdm_sense_forward_c64(const float* x, const float* sens, const uint8_t* mask, int mask_t,
                           float* y, int B, int n_coils, int H, int W, void* stream);
/* Scratch the SENSE / single-coil operators below need for (B, n_coils, H, W):
 *   IPDM_KSPACE_LDS sizes (up to 128x128; image resident in LDS): n_coils*B*H*W*8 bytes for the proximal operators (one
 *   plane per (sample, coil): the coils of a sample run in parallel workgroups), nothing for forward / adjoint / SSOS;
 *   IPDM_KSPACE_STRIPS sizes (e.g. the reference's 256x256 ACDC slices, helpers/load_data.py:274; row / column FFT
 *   passes): n_coils*B*H*W*8 bytes for every operator except ipdm_sense_forward_c64 (single-coil: n_coils = 1). */
int64_t ipdm_sense_workspace_bytes(int B, int n_coils, int H, int W);
/* x[b] = sum_c S_c * ifft2c(mask? mask*s : s)    apply_mask == 0 reproduces SENSE.conj_op; workspace: see above
 * (may be NULL up to 128x128) */
int ipdm_sense_adjoint_c64(const float* s, const float* sens, const uint8_t* mask, int mask_t,
                           int apply_mask, float* x, float* workspace, int B, int n_coils, int H, int W, void* stream);
/* out[b] = sqrt(sum_c |ifft2c(s[c][b])|^2)    float32 [B][H][W] */
int ipdm_sense_ssos_c64(const float* s, float* out, float* workspace, int B, int n_coils, int H, int W, void* stream);

/* L2Penalty with a SENSE operator, closed form of its one SGD step:
 *   x = z - coef * A^H(A z - y),   coef = 0.05 * (alpha/lamda) / (n_coils * W)  (computed by the caller)
 * z given as planar real / imaginary float32 [B][H][W] (the sampler's x_mod_real / x_mod_imag), result
 * written planar to out_re / out_im (may alias z_re / z_im). */
int ipdm_sense_l2prox_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                          const uint8_t* mask, int mask_t, float coef, float* out_re, float* out_im,
                          float* work /* ipdm_sense_workspace_bytes(B, n_coils, H, W) */, int B, int n_coils, int H, int W,
                          void* stream);

/* Per-iteration scalars held in DEVICE memory, so that a captured hipGraph of one iteration can be
 * replayed for every noise level without re-instantiation: the host (or a tiny kernel) rewrites the
 * struct between replays. */
typedef struct ipdm_sched_t {
  float step;        /* step_lr * (sigma / sigma_L)^2                       */
  float noise_scale; /* sqrt(2 * step)                                      */
  float coef;        /* proximal coefficient (see ipdm_sense_l2prox_f32)    */
  float sigma;       /* current noise level (informational)                 */
  int64_t step_id;   /* global iteration counter: Philox key                */
  float seg_scale;   /* segmentation-likelihood weight lh_weight / sigma (ALD_optimizers.py:283) */
  float reserved;    /* keeps the struct 32 bytes                            */
} ipdm_sched_t;

/* One fused Annealed-Langevin iteration tail for the SENSE sampler (reference:
 * ncsn/models/ALD_optimizers.py:238-247 + :288-327 + proximal_op.py:19-51):
 *   x_re += step*g_re + sqrt(2*step)*n_re ; x_im likewise ; x = L2prox(x_re + i x_im)
 * noise_re/noise_im NULL -> counter-based Philox4x32-10 normals keyed by (seed, sample id, step_id),
 * sample id = sample_offset + b, so results do not depend on how samples are sharded over GPUs. */
int ipdm_ald_sense_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                            const float* noise_re, const float* noise_im,
                            float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                            const ipdm_sched_t* dev_sched /* device; non-NULL overrides step/noise_scale/coef/step_id */,
                            const float* y, const float* sens, const uint8_t* mask, int mask_t, float coef,
                            float* work /* ipdm_sense_workspace_bytes(B, n_coils, H, W) */, int B, int n_coils, int H, int W,
                            void* stream);

/* The four operators above for COMPLEX coil sensitivity maps (measured maps: ESPIRiT, body-coil division, simulation).
 * Same argument lists and return codes; `sens` is interleaved complex64 [n_coils][H][W] (2 floats per element, must not
 * be NULL: IPDM_EINVAL).  Forward multiplies by S_c, adjoint and proximal tail by conj(S_c).  Maps with a zero imaginary
 * part give the values of the real-map entry points exactly (only the sign of a zero may differ); workspace sizes are
 * unchanged (ipdm_sense_workspace_bytes). */
int ipdm_sense_forward_csm_c64(const float* x, const float* sens, const uint8_t* mask, int mask_t,
                               float* y, int B, int n_coils, int H, int W, void* stream);
int ipdm_sense_adjoint_csm_c64(const float* s, const float* sens, const uint8_t* mask, int mask_t,
                               int apply_mask, float* x, float* workspace, int B, int n_coils, int H, int W, void* stream);
int ipdm_sense_l2prox_csm_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                              const uint8_t* mask, int mask_t, float coef, float* out_re, float* out_im,
                              float* work, int B, int n_coils, int H, int W, void* stream);
int ipdm_ald_sense_step_csm_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                const float* noise_re, const float* noise_im,
                                float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                const ipdm_sched_t* dev_sched, const float* y, const float* sens, const uint8_t* mask,
                                int mask_t, float coef, float* work, int B, int n_coils, int H, int W, void* stream);

/* Exact multi-coil proximal by conjugate gradients (the argmin that L2Penalty's docstring states and its
 * check_solution tests, proximal_op.py:19-69; the one-step operators above miss it by orders of magnitude):
 *   x = argmin 1/2 |x - z|^2 + a/2 |A x - y|^2   <=>   (I + a A^H A) x = z + a A^H y,   a = alpha/lamda (by the caller)
 * Plain CG per sample on complex vectors with real dot products, warm start x0 = z.  Sample b stops when
 * |r| <= tol * |b|, b = z + a A^H y, or after max_iter iterations; a stopped sample is frozen (its x no longer changes)
 * and samples never interact, so a sample's result does not depend on its batch.  tol == 0 runs max_iter iterations;
 * a sample whose <r,r> or <p,Np> is not positive is frozen instead of divided by (z = 0, y = 0 returns exactly 0);
 * a == 0 returns z bit for bit.  max_iter < 1, tol < 0 or not finite: IPDM_EINVAL.
 *   z_re / z_im -> out_re / out_im   planar float32 [B][H][W], may alias
 *   ahy         optional A^H y, complex64 [B][H][W] (constant over a sampler run); NULL: formed into the workspace
 *   iters_out   optional device int32 [B]: CG iterations each sample ran
 *   work        ipdm_sense_cg_workspace_bytes(B, n_coils, H, W)
 * Sizes as the other SENSE operators (ipdm_kspace_size_class: up to 128x128 in LDS, up to 2048 by row / column passes),
 * anything else IPDM_EUNSUPPORTED.  The launch sequence is fixed by (max_iter, size) alone -- it does not depend on
 * convergence -- and the calls are asynchronous, allocation-free and hipGraph-capturable.  Deterministic (no atomics). */
int64_t ipdm_sense_cg_workspace_bytes(int B, int n_coils, int H, int W);
int ipdm_sense_cgprox_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                          const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter, float tol,
                          float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils, int H, int W,
                          void* stream);
/* the same with complex coil maps (interleaved complex64 [n_coils][H][W]) */
int ipdm_sense_cgprox_csm_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                              const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter, float tol,
                              float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils, int H, int W,
                              void* stream);
/* ipdm_ald_sense_step_f32 with the CG proximal as its data-consistency operator: Langevin update of both planes (same
 * scalars, noise and Philox keying), then x = the solution above with z the updated state.  `coef` (dev_sched->coef
 * when a device schedule is given) carries a = alpha/lamda, as for the SingleCoil closed form; ahy, max_iter, tol,
 * iters_out and work as ipdm_sense_cgprox_f32. */
int ipdm_ald_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                               const float* noise_re, const float* noise_im,
                               float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                               const ipdm_sched_t* dev_sched, const float* y, const float* sens, const uint8_t* mask,
                               int mask_t, float coef, float* work, const float* ahy, int max_iter, float tol,
                               int32_t* iters_out, int B, int n_coils, int H, int W, void* stream);
int ipdm_ald_sense_cg_step_csm_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                   const float* noise_re, const float* noise_im,
                                   float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                   const ipdm_sched_t* dev_sched, const float* y, const float* sens, const uint8_t* mask,
                                   int mask_t, float coef, float* work, const float* ahy, int max_iter, float tol,
                                   int32_t* iters_out, int B, int n_coils, int H, int W, void* stream);

/* One set of coil maps per slice: a stack of slices reconstructed in one batch.
 *   sens          [sens_sets][n_coils][H][W], float32 (sens_complex == 0) or interleaved complex64 (sens_complex != 0)
 *   image b       reads set b % sens_sets -- the rule mask planes follow (b % T).  The two indices are independent:
 *                 sens_sets = 2 with a 3-plane mask is legal and means (set b % 2, plane b % 3).
 * A batch that holds n samples of each of S slices is laid out sample-major, b = sample * S + slice; y stays
 * [n_coils][B][H][W] and the Philox key stays sample_offset + b.  Every other argument, the arithmetic, the return codes
 * and the workspace sizes (ipdm_sense_workspace_bytes, ipdm_sense_cg_workspace_bytes) are those of the entry points
 * above, which are the sens_sets == 1 case of the same kernels: one set gives their results bit for bit, and rows
 * b % S == s of a multi-set call equal the single-set call on those rows with set s.  sens_sets < 1 or sens == NULL:
 * IPDM_EINVAL (there is no single-coil shortcut here).  B need not be a multiple of sens_sets. */
int ipdm_sense_forward_sets_c64(const float* x, const float* sens, int sens_complex, int sens_sets, const uint8_t* mask,
                                int mask_t, float* y, int B, int n_coils, int H, int W, void* stream);
int ipdm_sense_adjoint_sets_c64(const float* s, const float* sens, int sens_complex, int sens_sets, const uint8_t* mask,
                                int mask_t, int apply_mask, float* x, float* workspace, int B, int n_coils, int H, int W,
                                void* stream);
int ipdm_sense_l2prox_sets_f32(const float* z_re, const float* z_im, const float* y, const float* sens, int sens_complex,
                               int sens_sets, const uint8_t* mask, int mask_t, float coef, float* out_re, float* out_im,
                               float* work, int B, int n_coils, int H, int W, void* stream);
int ipdm_ald_sense_step_sets_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                 const float* noise_re, const float* noise_im,
                                 float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                 const ipdm_sched_t* dev_sched, const float* y, const float* sens, int sens_complex,
                                 int sens_sets, const uint8_t* mask, int mask_t, float coef, float* work, int B, int n_coils,
                                 int H, int W, void* stream);
int ipdm_sense_cgprox_sets_f32(const float* z_re, const float* z_im, const float* y, const float* sens, int sens_complex,
                               int sens_sets, const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter,
                               float tol, float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils,
                               int H, int W, void* stream);
int ipdm_ald_sense_cg_step_sets_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                    const float* noise_re, const float* noise_im,
                                    float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                    const ipdm_sched_t* dev_sched, const float* y, const float* sens, int sens_complex,
                                    int sens_sets, const uint8_t* mask, int mask_t, float coef, float* work,
                                    const float* ahy, int max_iter, float tol, int32_t* iters_out, int B, int n_coils,
                                    int H, int W, void* stream);

/* Coil sensitivity maps estimated from the fully sampled calibration region of the measurement itself (Walsh's adaptive
 * estimator on low-resolution calibration images; the reference only synthesises maps, undersampling_fourier.py:124-138).
 *   y [n_coils][B][H][W] c64, the measurement layout of the SENSE operators (centred, orthonormal scale)
 *   (ah, aw)   half-widths of the calibration box [H/2-ah, H/2+ah] x [W/2-aw, W/2+aw], inside the image
 *   calibration images  c_j = ifft2c(w_H (x) w_W . y_j),  w(k) = 0.5 + 0.5 cos(pi (k - N/2) / (a + 1)) in the box, 0 outside
 *   support    rss(x) = sqrt(sum_j |c_j(x)|^2) > thresh * rss_max[b]   (strict; rss_max[b] the maximum over image b)
 *   maps       the dominant eigenvector of R(x) = sum over the (2 radius + 1)^2 neighbourhood of c(x') c(x')^H (neighbours
 *              outside the image contribute zero), by power iteration from v0 = normalise(R(x) 1) and power_iters further
 *              applications v <- normalise(R(x) v); normalise divides by the 2-norm over the coils (by 1 where it is 0);
 *              then rotated so that coil 0 is real and non-negative; 0 outside the support.
 * radius 1..4, n_coils 1..32, sizes of ipdm_kspace_size_class LDS / STRIPS with sides up to 1024 (ipdm_fft2c_c64's limit)
 * and n_coils * B <= 65535; otherwise IPDM_EUNSUPPORTED (ipdm_csm_supported tells, without a GPU).  IPDM_EINVAL: a box
 * outside the image, radius outside 1..4, power_iters < 0, thresh negative or NaN, a NULL tensor.  fp32 arithmetic;
 * asynchronous, allocation-free and hipGraph-capturable (rss_max is zeroed by a memset node of the call, then raised by one
 * atomic max per wave on the bit pattern: exact, order-independent); an image's maps do not depend on its batch.  Every
 * tensor may sit on any 8-byte boundary (rss, rss_max: 4). */
size_t ipdm_csm_workspace_bytes(int B, int n_coils, int H, int W);   /* calibration images + rss plane; 0 when unserved */
int ipdm_csm_supported(int n_coils, int radius, int H, int W);       /* 1 / 0, no GPU needed */
/* the calibration images alone: calib [n_coils][B][H][W] c64, must not alias y */
int ipdm_csm_calib_images_c64(const float* y, int ah, int aw, float* calib, int B, int n_coils, int H, int W, void* stream);
int ipdm_csm_walsh_c64(const float* y, int ah, int aw, int radius, int power_iters, float thresh,
                       float* maps /* [n_coils][B][H][W] c64 */, float* rss /* [B][H][W] or NULL */,
                       float* rss_max /* [B] */, float* work /* ipdm_csm_workspace_bytes(B, n_coils, H, W) */, int B,
                       int n_coils, int H, int W, void* stream);

/* Coil compression and noise prewhitening of a multi-coil measurement (software coil compression by PCA of the calibration
 * data; not in the reference, which synthesises 4 maps).  y [n_coils][B][H][W] c64 and the calibration box (ah, aw) as above.
 *   gram    G_b[i][j] = sum over the box of y_i(b,k) conj(y_j(b,k)), no window: [B][n_coils][n_coils] c64, exactly
 *           Hermitian with a real diagonal (summed in double, rounded once)
 *   matrix  with noise_cov psi [n_coils][n_coils] c64 (Hermitian positive definite, shared by the batch; NULL: none):
 *           psi = L L^H, G <- L^-1 G L^-H.  G = U diag(eig) U^H by cyclic Hermitian Jacobi (12 sweeps, fixed: the
 *           launch never depends on the data), eigenvalues descending, equal ones in their original order.  A_b = U[:, :n_virtual]^H (times
 *           L^-1), [B][n_virtual][n_coils] c64, each row turned by a unit phase so that A_b[v][0] is real and non-negative
 *           (left alone where it is exactly zero).  eig [B][n_coils] or NULL.  status [B] int32: 0, or 1 where a Cholesky
 *           pivot of psi is not positive; that image's A and eig are then zeros, never NaN.
 *   apply   out_v(b,p) = sum_c A[v][c] y_c(b,p): y [n_coils][B][P], out [n_virtual][B][P] c64 for any pixel count P per
 *           image (maps [n_coils][1][H*W] compress the same way); A per image ([B][n_virtual][n_coils], per_image != 0) or
 *           one [n_virtual][n_coils] for the whole batch.  out may not overlap y (IPDM_EINVAL).
 *   compress  the three in one call, A per image; work: ipdm_coilcomp_workspace_bytes(B, n_coils) bytes (the Gram matrices).
 * n_coils 1..64, n_virtual 1..min(n_coils, 32), B <= 65535, otherwise IPDM_EUNSUPPORTED (ipdm_coilcomp_supported tells,
 * without a GPU); IPDM_EINVAL: a box outside the image, a NULL tensor, overlapping y and out.  fp32 arithmetic; asynchronous,
 * allocation-free, hipGraph-capturable, no atomics: deterministic, an image's results do not depend on its batch.  Every
 * tensor may sit on any 8-byte boundary (eig, status: 4). */
int ipdm_coilcomp_supported(int n_coils, int n_virtual);             /* 1 / 0, no GPU needed */
size_t ipdm_coilcomp_workspace_bytes(int B, int n_coils);            /* 0 when unserved */
int ipdm_coil_gram_c64(const float* y, int ah, int aw, float* gram, int B, int n_coils, int H, int W, void* stream);
int ipdm_coilcomp_matrix_c64(const float* gram, const float* noise_cov, int n_virtual, float* A, float* eig, int32_t* status,
                             int B, int n_coils, void* stream);
int ipdm_coil_apply_c64(const float* y, const float* A, int per_image, float* out, int B, int n_coils, int n_virtual,
                        int64_t P, void* stream);
int ipdm_coil_compress_c64(const float* y, int ah, int aw, int n_virtual, const float* noise_cov, float* A, float* eig,
                           int32_t* status, float* out, float* work, int B, int n_coils, int H, int W, void* stream);

/* Geometric coil compression along the fully sampled readout axis H (Zhang et al. 2013): one matrix per readout position.
 *   readout_fft  centred orthonormal DFT (inverse != 0: inverse DFT) along H of every column of `planes` [H][W] c64 planes,
 *                fft2c's centring, so that row x of the inverse transform of k-space is image row x.  H a power of two from
 *                4 or a multiple of 16 of the form 2^a 3^b 5^c, at most 2048 (else IPDM_EUNSUPPORTED); any W.  out == in is
 *                allowed, a partial overlap is IPDM_EINVAL.
 *   gram         h [n_coils][B][H][W] c64 (hybrid space): G_{b,x}[i][j] = sum over the rows [x-win, x+win] clipped to the
 *                image, ascending, and the columns [W/2-aw, W/2+aw], ascending, of h_i conj(h_j), summed in double and
 *                rounded once: [B][H][n_coils][n_coils] c64, exactly Hermitian.  win 0..8.
 *   align        Ahat [B][H][n_virtual][n_coils] c64 (the matrix stage on every G_{b,x}) -> A of the same shape: row H/2
 *                is copied; outward in both directions A_x = P_x Ahat_x with P_x the unitary polar factor that makes
 *                P_x (Ahat_x psi A_p^H) Hermitian positive semidefinite (30 Newton-Schulz iterations), p the nearest
 *                position on the centre side that was not degenerate.  A position whose iterate X has an entry of
 *                X^H X - I above 1e-3 (real or imaginary part) is degenerate: it keeps Ahat_x.  status [B] int32: the count
 *                of degenerate positions.  noise_cov psi [n_coils][n_coils] c64 or NULL (identity).  work: 2 * B int32.
 *                A may not overlap Ahat.
 *   apply_rows   out_v(b,x,c) = sum_k A[b][x][v][k] y_k(b,x,c): y [n_coils][B][H][W], out [n_virtual][B][H][W] c64; A per
 *                image [B][H][n_virtual][n_coils] (per_image != 0) or one [H][n_virtual][n_coils] for the batch.
 *   compress     the whole chain y -> y' [n_virtual][B][H][W] with A [B][H][n_virtual][n_coils], eig [B][H][n_coils] (or
 *                NULL) and status [B]: the degenerate count, or -1 (and zero matrices) where a Cholesky pivot of psi was not
 *                positive.  work: ipdm_gcc_workspace_bytes(B, n_coils, n_virtual, H, W) bytes, overlapping neither y nor out.
 * Coil counts and B as above; ipdm_gcc_supported tells without a GPU.  Asynchronous, no atomics, capturable in a hipGraph. */
int ipdm_gcc_supported(int n_coils, int n_virtual, int H, int W, int win);              /* 1 / 0, no GPU needed */
size_t ipdm_gcc_workspace_bytes(int B, int n_coils, int n_virtual, int H, int W);        /* 0 when unserved */
int ipdm_readout_fft_c64(const float* in, float* out, int inverse, int64_t planes, int H, int W, void* stream);
int ipdm_gcc_gram_c64(const float* h, int aw, int win, float* gram, int B, int n_coils, int H, int W, void* stream);
int ipdm_gcc_align_c64(const float* Ahat, const float* noise_cov, float* A, int32_t* status, int32_t* work, int B, int H,
                       int n_coils, int n_virtual, void* stream);
int ipdm_coil_apply_rows_c64(const float* y, const float* A, int per_image, float* out, int B, int n_coils, int n_virtual, int H,
                             int W, void* stream);
int ipdm_gcc_compress_c64(const float* y, int aw, int win, int n_virtual, const float* noise_cov, float* A, float* eig,
                          int32_t* status, float* out, float* work, int B, int n_coils, int H, int W, void* stream);

/* ESPIRiT coil sensitivity maps from the calibration region (Uecker et al. 2014; one map set).  y [n_coils][B][H][W] c64 and
 * the calibration box (ah, aw) as above; ksize the side k of the k-space kernels, M = n_coils k^2.
 *   gram     Gm_b[i][j] = sum over the (2ah+2-k)(2aw+2-k) patch positions p of conj(a_p[i]) a_p[j], a_p[(c, ty, tx)] =
 *            y_c(H/2-ah+py+ty, W/2-aw+px+tx), columns in the order (coil, ty, tx): [B][M][M] complex double (re, im),
 *            products and sums in double, exactly Hermitian with a real diagonal
 *   kernels  gram, then Gm = V diag(lam) V^H by cyclic two-sided Hermitian Jacobi in double (round-robin ordering; stops
 *            when a sweep met off(G) <= 1e-12 ||G||_F, at most 60 sweeps), lam [B][M] descending, rank[b] =
 *            #{sqrt(max(lam_i, 0)) > sv_thresh sqrt(max(lam_0, 0))}, decided on the device, and the kernel correlation
 *            K [B][n][n][2k-1][2k-1] c64, K[c][c'][dy][dx] = sum over t - t' = (dy-(k-1), dx-(k-1)) of P[(c,t)][(c',t')],
 *            P the projector onto the first rank[b] eigenvectors (summed in double, rounded once).  status [B] int32: 0, or 1
 *            where the sweeps did not converge or a value is not finite; that image's lam, rank, K and maps are zeros.
 *            sweeps [B] int32 (or NULL): the sweeps made.  work: ipdm_espirit_workspace_bytes(B, n_coils, ksize) bytes.
 *   pixel    G(x)[c][c'] = (1/k^2) sum_d K[c][c'][d] exp(-2 pi i (dy (xr - H/2) / H + dx (xc - W/2) / W)), a direct DFT of
 *            the taps (every H, W up to 1024, also sizes without an FFT kernel); u = normalise(G(x) 1), power_iters further
 *            applications u <- normalise(G(x) u) (normalise divides by the 2-norm, by 1 where it is 0); eigval [B][H][W]
 *            (or NULL) = Re(u^H G(x) u); maps [n_coils][B][H][W] c64 = conj(u) turned so that coil 0 is real and
 *            non-negative where eigval > crop, exactly 0 elsewhere.  fp32.  status [B] (or NULL: every image is computed).
 *   espirit  kernels, then pixel.
 * n_coils 1..16, ksize 3..8, M <= 432, H, W <= 1024, B <= 65535, otherwise IPDM_EUNSUPPORTED (ipdm_espirit_supported tells,
 * without a GPU).  IPDM_EINVAL: a box outside the image or with a side below ksize, sv_thresh outside [0, 1) or NaN, crop
 * NaN, power_iters < 0, a NULL tensor.  Asynchronous, allocation-free, hipGraph-capturable, no atomics and no host
 * synchronisation: an image's results do not depend on its batch.  y, K, maps on any 8-byte boundary, the others on their
 * element's. */
int ipdm_espirit_supported(int n_coils, int ksize, int H, int W);    /* 1 / 0, no GPU needed */
size_t ipdm_espirit_workspace_bytes(int B, int n_coils, int ksize);  /* Gm and V; 0 when unserved */
int ipdm_espirit_gram_c64(const float* y, int ah, int aw, int ksize, double* gram, int B, int n_coils, int H, int W, void* stream);
int ipdm_espirit_kernels_c64(const float* y, int ah, int aw, int ksize, double sv_thresh, float* K, double* lam, int32_t* rank,
                             int32_t* status, int32_t* sweeps, double* work, int B, int n_coils, int H, int W, void* stream);
int ipdm_espirit_pixel_c64(const float* K, const int32_t* status, int ksize, float crop, int power_iters, float* maps,
                           float* eigval, int B, int n_coils, int H, int W, void* stream);
int ipdm_espirit_c64(const float* y, int ah, int aw, int ksize, double sv_thresh, float crop, int power_iters, float* maps,
                     float* eigval, float* K, double* lam, int32_t* rank, int32_t* status, double* work, int B, int n_coils,
                     int H, int W, void* stream);

/* Mask-weighted time average of 2D+time multi-coil k-space: the composite a cine acquisition is calibrated from (its
 * interleaved per-frame patterns together sample the centre fully; maps and compression matrix come from the composite
 * and are shared by the frames).  y [n_coils][B][T][H][W] c64 (the cine measurement (n, B, T, 1, H, W)); mask / mask_t as
 * for the SENSE operators, frame t of image b using plane (b*T + t) % |mask_t| -- what those operators apply to the
 * flattened (B*T) stack.  count [B][H][W] int32 (or NULL): the number of frames that sampled the pixel; ybar
 * [n_coils][B][H][W] c64: the sum of y over those frames, in frame order, divided by count -- summed and divided in double,
 * rounded once -- and exactly 0 where count == 0.  y is read at sampled positions only (a NaN elsewhere never reaches the
 * output).  Any H, W, n_coils, B >= 1 (B == 0: IPDM_OK, nothing launched; B above 65535 is folded), 1 <= T <= 4096
 * (above: IPDM_EUNSUPPORTED); IPDM_EINVAL: a non-positive size, mask_t == 0, a NULL y / mask / ybar, ybar overlapping y.
 * Asynchronous, allocation-free, hipGraph-capturable, no atomics: a pixel's result depends on its own frames alone.  y and
 * ybar may sit on any 8-byte boundary (count: 4). */
int ipdm_kspace_tavg_c64(const float* y, const uint8_t* mask, int mask_t, float* ybar, int32_t* count, int B, int T,
                         int n_coils, int H, int W, void* stream);

/* Single-coil data-consistency operators (A = M F, RandomUndersamplingFourier, no coil maps) on planar real/imag
 * float32 [B][H][W], y [B][H][W] complex64; out may alias z.  mode:
 *   0  L2Penalty on a single-coil operator (proximal_op.py:19-51): x = z - coef * F^-1[M (M F z - y)],
 *      coef = 0.05 * (alpha/lamda) / B  (the .mean() of the reference's loss runs over the batch; computed by the caller)
 *   1  SingleCoil closed form (proximal_op.py:72-94): x = F^-1[(F z + coef*y) / (1 + coef*M)], coef = alpha/lamda
 *   2  RandomUndersamplingFourier.projection (undersampling_fourier.py:89-97) = Constrained.__call__ (proximal_op.py:62-69):
 *      x = F^-1[coef*y + (1-coef) M F z + (1-M) F z], coef = lamda */
int ipdm_singlecoil_prox_f32(const float* z_re, const float* z_im, const float* y, const uint8_t* mask, int mask_t,
                             float coef, int mode, float* out_re, float* out_im,
                             float* workspace /* ipdm_sense_workspace_bytes(B, 1, H, W); NULL allowed up to 128x128 */,
                             int B, int H, int W, void* stream);

/* One fused Annealed-Langevin iteration tail for the single-coil samplers (the reference's
 * scripts/acdc_inv_seg_sampling_keep_center_prox_real_imag.py:79-89 and cine_inv_sampling_keep_center_prox_real_imag.py:78-88
 * build ALDInvSegProximalRealImag on RandomUndersamplingFourier + get_proximal(...)): Langevin update of both planes,
 * then ipdm_singlecoil_prox_f32's operator `mode`, in place; scalars / noise as ipdm_ald_sense_step_f32. */
int ipdm_ald_singlecoil_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                 const float* noise_re, const float* noise_im,
                                 float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                 const ipdm_sched_t* dev_sched, const float* y, const uint8_t* mask, int mask_t,
                                 float coef, int mode, float* workspace /* as ipdm_singlecoil_prox_f32 */, int B, int H,
                                 int W, void* stream);

/* Predictor-corrector sampling with data consistency (sde/inverse.py): one schedule record PER SAMPLE.
 *
 * ipdm_pc_langevin_coef_f32 forms the Langevin corrector's step of each complex sample on the device (score_sde's
 * LangevinCorrector, sampling.py, with its two batch means replaced by per-sample norms, so that a sample does not
 * depend on its batch or on sharding).  For sample b of the planar score g_re / g_im [B][sample_elems]:
 *   ng = sqrt(sum g_re^2 + sum g_im^2),  nz = the same norm of the noise z the following tail applies to sample b:
 *        noise_re / noise_im when given, else the Philox normals of (seed, sample_offset + b, step_id, plane 0 / 1),
 *        regenerated here (no noise tensor exists in memory)
 *   sample_sched[b] = { step = 2 alpha (snr nz / ng)^2, noise_scale = sqrt(2 step), coef, sigma, step_id, seg_scale = 0 }
 * coef, sigma and step_id come from *dev_sched when it is non-NULL (a shared device record), else from the arguments.
 * Sums are accumulated in double in a fixed order without atomics (bit-reproducible; independent of B), the
 * coefficients formed in double and rounded once.  ng == 0: step = noise_scale = 0 (the tail then only applies data
 * consistency); a NaN or infinite norm: NaN in that sample's record only.
 * work: ipdm_pc_langevin_coef_workspace_bytes(B) bytes of device memory.  B <= 65535, 0 < sample_elems <= 2^31. */
int64_t ipdm_pc_langevin_coef_workspace_bytes(int B);
int ipdm_pc_langevin_coef_f32(const float* g_re, const float* g_im, const float* noise_re, const float* noise_im,
                              double snr, double alpha, uint64_t seed, int64_t sample_offset, int64_t step_id,
                              const ipdm_sched_t* dev_sched, float coef, float sigma, ipdm_sched_t* sample_sched,
                              double* work, int B, int64_t sample_elems, void* stream);
/* The fused tails ipdm_ald_sense_step_sets_f32, ipdm_ald_sense_cg_step_sets_f32 and ipdm_ald_singlecoil_step_f32 with
 * sched_stride records between consecutive samples: 0 is those entry points (one shared record or the host scalars;
 * the same kernels, the same bits), 1 makes sample b read dev_sched[b] (step, noise_scale, coef and step_id; B
 * records, dev_sched non-NULL).  Any other stride: IPDM_EINVAL.  Every other argument as in those entry points. */
int ipdm_pc_sense_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                           const float* noise_re, const float* noise_im,
                           float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                           const ipdm_sched_t* dev_sched, int sched_stride, const float* y, const float* sens,
                           int sens_complex, int sens_sets, const uint8_t* mask, int mask_t, float coef, float* work, int B,
                           int n_coils, int H, int W, void* stream);
int ipdm_pc_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                              const float* noise_re, const float* noise_im,
                              float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                              const ipdm_sched_t* dev_sched, int sched_stride, const float* y, const float* sens,
                              int sens_complex, int sens_sets, const uint8_t* mask, int mask_t, float coef, float* work,
                              const float* ahy, int max_iter, float tol, int32_t* iters_out, int B, int n_coils, int H,
                              int W, void* stream);
int ipdm_pc_singlecoil_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                const float* noise_re, const float* noise_im,
                                float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                const ipdm_sched_t* dev_sched, int sched_stride, const float* y, const uint8_t* mask,
                                int mask_t, float coef, int mode, float* workspace, int B, int H, int W, void* stream);

/* Non-Cartesian SENSE: samples at arbitrary k-space positions (radial, spiral, ...), DESIGN.md 4.4l.
 *   traj      device float64 [M][2] = (k_y, k_x) in cycles per field of view, |k_y| <= H/2, |k_x| <= W/2 (by the caller)
 *   weights   device float32 [M], w_m >= 0; NULL: 1 (the likelihood of i.i.d. noise; density compensation is for the
 *             zero-filled image alone)
 *   sens      interleaved complex64 [n_coils][H][W]; NULL: S = 1 (see each entry point)
 *   forward   y[c,b,m] = (HW)^-1/2 sum_{r,col} S_c[r,col] x[b,r,col] exp(-2 pi i (k_y,m (r - H/2)/H + k_x,m (col - W/2)/W))
 *             -- the package's centred orthonormal convention: a sample on the integer grid point (k_y, k_x) is
 *             ipdm_fft2c_c64's value at index (k_y + H/2, k_x + W/2) --, adjoint its conjugate transpose after w.
 * The transforms are exact direct sums (no gridding, no interpolation), accumulated in double in a fixed order, and
 * are meant to run once per reconstruction.  The per-iteration operator A^H W A is Toeplitz:
 *   T[dr + H, dc + W] = sum_m w_m exp(2 pi i (k_y,m dr/H + k_x,m dc/W)), |dr| < H, |dc| < W (row 0 / column 0: zero),
 *   psf = centred unnormalised DFT of T, over HW: real, float32 [2H][2W], may be negative
 *   A^H W A v = sum_c conj(S_c) crop(F^-1(psf . F(pad(S_c v)))),  v at rows [H/2, H/2 + H), columns [W/2, W/2 + W) of 2H x 2W.
 * Sizes: every (H, W) whose padded grid 2H x 2W is a size of ipdm_kspace_size_class (ipdm_nc_supported tells, without a
 * GPU), B and n_coils <= 65535 (n_coils * B <= 65535 for the two transforms); otherwise IPDM_EUNSUPPORTED.  IPDM_EINVAL:
 * a non-positive size, a NULL operand.  All calls are asynchronous, allocation-free and deterministic. */
int ipdm_nc_supported(int H, int W);
/* x: complex64 [B][H][W] with sens, else the coil images [n_coils][B][H][W]; y: complex64 [n_coils][B][M] */
int64_t ipdm_ndft_workspace_bytes(int M, int H, int W);
int ipdm_ndft_forward_c64(const float* x, const float* sens, const double* traj, float* y,
                          float* work /* ipdm_ndft_workspace_bytes */, int B, int n_coils, int M, int H, int W, void* stream);
/* x: with sens the combined image sum_c conj(S_c)(.) [B][H][W], else the coil images [n_coils][B][H][W] */
int ipdm_ndft_adjoint_c64(const float* y, const float* sens, const double* traj, const float* weights, float* x,
                          float* work /* ipdm_ndft_workspace_bytes */, int B, int n_coils, int M, int H, int W, void* stream);
int64_t ipdm_toeplitz_psf_workspace_bytes(int M, int H, int W);
int ipdm_toeplitz_psf_f32(const double* traj, const float* weights, float* psf,
                          float* work /* ipdm_toeplitz_psf_workspace_bytes */, int M, int H, int W, void* stream);
/* out = A^H W A v; v, out complex64 [B][H][W], out != v; sens NULL needs n_coils == 1 */
int64_t ipdm_toeplitz_workspace_bytes(int B, int n_coils, int H, int W);
int ipdm_toeplitz_normal_c64(const float* v, const float* sens, const float* psf, float* out,
                             float* work /* ipdm_toeplitz_workspace_bytes */, int B, int n_coils, int H, int W, void* stream);
/* ipdm_sense_cgprox_f32 and ipdm_pc_sense_cg_step_f32 (sched_stride 0: ipdm_ald_sense_cg_step_f32) for the operator
 * above: (I + a A^H W A) x = z + a ahy with ahy = A^H W y REQUIRED (ipdm_ndft_adjoint_c64; the iterations never apply
 * A).  Same solver kernels, stopping rule, per-sample freezing, iters_out, schedule records and fixed launch sequence
 * (3 + 4 max_iter launches, + 1 with a Langevin update): one captured hipGraph serves every noise level. */
int64_t ipdm_nc_sense_cg_workspace_bytes(int B, int n_coils, int H, int W);
int ipdm_nc_sense_cgprox_f32(const float* z_re, const float* z_im, const float* sens, const float* psf, float a,
                             const float* ahy, int max_iter, float tol, float* out_re, float* out_im, float* work,
                             int32_t* iters_out, int B, int n_coils, int H, int W, void* stream);
int ipdm_ald_nc_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                  const float* noise_re, const float* noise_im,
                                  float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                  const ipdm_sched_t* dev_sched, int sched_stride, const float* sens, const float* psf,
                                  float coef, float* work, const float* ahy, int max_iter, float tol, int32_t* iters_out,
                                  int B, int n_coils, int H, int W, void* stream);
/* Frame sets (radial cine): one trajectory per frame, the ipdm_*_sets_* rule a third time.
 *   traj      device float64 [T][M][2], T = traj_sets >= 1 frames of M samples each (frames of unequal length: pad to one M
 *             and give the padding weight 0)
 *   weights   device float32 [T][M] or NULL
 *   psf       float32 [T][2H][2W], set t from trajectory t (and weights t); T = psf_sets
 * Image row b of every operand ([B][H][W], [n_coils][B][M], ahy, iters_out, the schedule records) reads set b % T, so a
 * (posterior sample, frame) batch flattened frame-fastest is served as it lies in memory.  B % T != 0, T < 1: IPDM_EINVAL.
 * T * M beyond INT32_MAX: IPDM_EUNSUPPORTED.  The two transforms need ipdm_ndft_workspace_bytes(T * M, H, W) -- the phasor
 * tables cover all T * M samples --, the psf call ipdm_toeplitz_psf_workspace_bytes(M, H, W) (the sets are formed one
 * after another through it), the others the workspace of their one-set form.  Every sum of row b runs in the order the
 * one-set entry point has for trajectory b % T: its rows equal, bit for bit, the rows of that call on the same batch.
 * The iteration path gains no launch: the column pass offsets its psf read by (b % T) * 4HW, a workgroup-uniform value.
 * The entry points above are these with T = 1. */
int ipdm_ndft_forward_sets_c64(const float* x, const float* sens, const double* traj, int traj_sets, float* y, float* work,
                               int B, int n_coils, int M, int H, int W, void* stream);
int ipdm_ndft_adjoint_sets_c64(const float* y, const float* sens, const double* traj, int traj_sets, const float* weights,
                               float* x, float* work, int B, int n_coils, int M, int H, int W, void* stream);
int ipdm_toeplitz_psf_sets_f32(const double* traj, int traj_sets, const float* weights, float* psf, float* work, int M, int H,
                               int W, void* stream);
int ipdm_toeplitz_normal_sets_c64(const float* v, const float* sens, const float* psf, int psf_sets, float* out, float* work,
                                  int B, int n_coils, int H, int W, void* stream);
int ipdm_nc_sense_cgprox_sets_f32(const float* z_re, const float* z_im, const float* sens, const float* psf, int psf_sets,
                                  float a, const float* ahy, int max_iter, float tol, float* out_re, float* out_im,
                                  float* work, int32_t* iters_out, int B, int n_coils, int H, int W, void* stream);
int ipdm_ald_nc_sense_cg_step_sets_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                       const float* noise_re, const float* noise_im,
                                       float step, float noise_scale, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                       const ipdm_sched_t* dev_sched, int sched_stride, const float* sens, const float* psf,
                                       int psf_sets, float coef, float* work, const float* ahy, int max_iter, float tol,
                                       int32_t* iters_out, int B, int n_coils, int H, int W, void* stream);

/* Non-Cartesian self-calibration (csrc/nc_calib.hip): the weighted Gram matrix of the samples themselves, for coil
 * compression before calibration images exist.  y [n_coils][B][M] complex64 (the layout of the ndft_* operands), weights
 * [M] float32 >= 0 (NULL: 1; the calibration window of the trajectory), gram [B][n_coils][n_coils] complex64:
 *   G_b[i][j] = sum_m w_m y[i][b][m] conj(y[j][b][m])
 * Double products and sums over chunks of a fixed length, the chunks added in order, one rounding to float32, no atomics:
 * G is exactly Hermitian with a real diagonal, independent of the batch, and reproducible bit for bit.  y is read only
 * where w_m > 0, so a NaN at a zero-weight sample does not reach G.  work: ipdm_nc_coil_gram_workspace_bytes (the double
 * partial sums; 16-byte aligned; 0 for a shape the call refuses).  n_coils 1..64 and B <= 65535, otherwise
 * IPDM_EUNSUPPORTED; M < 1, n_coils < 1 or NULL tensors: IPDM_EINVAL; B == 0 returns IPDM_OK.  The result feeds
 * ipdm_coilcomp_matrix_c64 / ipdm_coil_apply_c64 as ipdm_coil_gram_c64's does. */
size_t ipdm_nc_coil_gram_workspace_bytes(int B, int n_coils, int M);
int ipdm_nc_coil_gram_c64(const float* y, const float* weights, float* gram, float* work, int B, int n_coils, int M, void* stream);

/* Langevin update alone (ALD_optimizers.py:117): x += step*g + noise_scale*noise ; noise NULL -> Philox. */
int ipdm_langevin_step_f32(float* x, const float* g, const float* noise, float step, float noise_scale,
                           uint64_t seed, int64_t sample_offset, int64_t step_id, const ipdm_sched_t* dev_sched,
                           int64_t n_samples, int64_t sample_elems, void* stream);

/* Philox normals exactly as the fused kernels draw them, for tests: out [n_samples][sample_elems] */
int ipdm_philox_normal_f32(float* out, uint64_t seed, int64_t sample_offset, int64_t step_id, int plane,
                           int64_t n_samples, int64_t sample_elems, void* stream);

/* HOST function (no GPU): the 128 random bits behind elements 4*quad..4*quad+3 of (seed, sample, step_id, plane).
 * key = seed, counter = (quad, step, sample, plane): distinct seeds / steps / samples never share a block
 * (replaces torch.randn_like's device generator, ALD_optimizers.py:238-241, by a sharding-invariant stream). */
int ipdm_philox_block_host(uint64_t seed, int64_t sample, int64_t step_id, int plane, uint32_t quad, uint32_t* out4);

/* ------------------------------------------------------------------------------------------------
 * Score-network glue (reference: ncsn/models/normalization.py:150-176 InstanceNorm2dPlus;
 * ncsn/models/layers.py:11-23 get_act, :62-83 CRPBlock max-pool, :165-184 MSFBlock bilinear sum,
 * :291-313 ConvMeanPool mean; ncsn/models/ncsnv2.py:270-271 input rescale, :295-297 sigma division).
 * ---------------------------------------------------------------------------------------------- */

/* per (b,c) plane statistics -> coef [B][C][3] = (mu, scale, shift) such that
 *   InstanceNorm2dPlus(x)[b,c,:,:] = (x - mu) * scale + shift
 * gamma/alpha/beta are the module's parameters ([C] each; beta may be NULL). Two launches. */
int ipdm_instnorm_plus_coef_f32(const float* x, const float* alpha, const float* gamma, const float* beta,
                                float* coef, int B, int C, int HW,
                                float* amax_bound /* NULL, or a maxima vector: an upper bound of max |normalised value| per image, from the
                                                     coefficients alone (|x - mu| * rstd < sqrt(HW)) -- the in_amax of the f16x2
                                                     convolution that reads the normalised tensor, at no pass over it */,
                                void* stream);
/* ConditionalInstanceNorm2dPlus (ncsn/models/normalization.py:179-208): the same coef [B][C][3] (and amax_bound), with gamma,
 * alpha, beta taken from row labels[b] of the embedding table embed [num_classes][row], row = [gamma | alpha | beta] (3C) or,
 * bias == 0, [gamma | alpha] (2C).  labels: int64 [B] in device memory, read by the kernel (a captured graph follows labels
 * written in place); a label outside [0, num_classes) gives NaN coefficients and a NaN bound for that image.  Two launches. */
int ipdm_cond_instnorm_plus_coef_f32(const float* x, const float* embed, const int64_t* labels, int num_classes, int bias,
                                     float* coef, int B, int C, int HW, float* amax_bound, void* stream);
/* y = act((x - mu) * scale + shift) with coef from above; x may equal y */
int ipdm_affine_act_f32(const float* x, const float* coef, float* y, int B, int C, int HW, int act, void* stream);
/* y = act(x) elementwise */
int ipdm_act_f32(const float* x, float* y, int64_t n, int act, void* stream);
/* y = a*x + b (scalar a, b) */
int ipdm_scale_shift_f32(const float* x, float* y, int64_t n, float a, float b, void* stream);
/* out = x + y (out may alias either) */
int ipdm_add_f32(const float* x, const float* y, float* out, int64_t n, void* stream);
/* out[b,...] = x[b,...] / sigmas[labels[b]];  labels == NULL: out[b,...] = x[b,...] / sigmas[b] */
int ipdm_div_sigma_f32(const float* x, const float* sigmas, const int64_t* labels, float* out,
                       int B, int64_t sample_elems, void* stream);
/* 3x3 'same' convolution (stride 1, dilation 1, zero padding) with at most three input OR at most three output channels:
 * the first / last layer of every score network (nn.Conv2d begin_conv / end_conv, ncsn/models/ncsnv2.py:40,45; conv3x3 of
 * models/ncsnpp.py:143,226).  Streaming fp32 kernels on the vector ALU (the matrix-core kernels pad the thin side to an
 * MFMA operand): w is the reference's own layout [Cout][Cin][3][3], bias may be NULL; W % 4 == 0, 16-byte aligned x / out.
 * ipdm_conv3x3_thin_supported tells whether a shape is served (else IPDM_EUNSUPPORTED). */
int ipdm_conv3x3_thin_supported(int Cin, int Cout, int H, int W);
int ipdm_conv3x3_thin_f32(const float* x, const float* w, const float* bias,
                          const float* coef /* NULL, or [B][Cin][3] = (c0, c1, c2): the input is (x - c0) * c1 + c2 inside the
                                               image (few-input-channel form only: `h = 2x - 1`, ncsnv2.py:64) */,
                          float* out, int B, int Cin, int Cout, int H, int W, void* stream);
/* The few-input-channel form with the statistics epilogue of the Winograd entries (ipdm_conv2d_wino1d_stats_f32): part
 * [B][Cout][P][3] = (count, mean, sum of squared deviations) of the stored values per group of 64 quads of a plane, P =
 * ipdm_conv3x3_thin_stats_partials (0: this shape has no such epilogue, the _stats entry answers IPDM_EUNSUPPORTED) -- what
 * ipdm_instnorm_plus_coef_partials_f32 takes instead of a pass over the tensor.  `out` has the bits of ipdm_conv3x3_thin_f32. */
int ipdm_conv3x3_thin_stats_partials(int Cin, int Cout, int H, int W);
int ipdm_conv3x3_thin_stats_f32(const float* x, const float* w, const float* bias, const float* coef, float* out, float* part,
                                int B, int Cin, int Cout, int H, int W, void* stream);
/* The few-output-channel form (Cout <= 3) on act(InstanceNorm++(x)) given as the RAW x and coef [B][Cin][3] (mu, scale, shift
 * from ipdm_instnorm_plus_coef_*): end_conv(act(normalizer(x))) of ncsn/models/ncsnv2.py:270-271 in one pass over x.  act:
 * IPDM_ACT_ELU only (else IPDM_EUNSUPPORTED).  The result equals ipdm_affine_act_f32 followed by ipdm_conv3x3_thin_f32 bit
 * for bit.  W % 4 == 0, 16-byte aligned x / out (else IPDM_EUNSUPPORTED). */
int ipdm_conv3x3_fewout_fin_supported(int Cin, int Cout, int H, int W);
int ipdm_conv3x3_fewout_fin_f32(const float* x, const float* w, const float* bias, const float* coef, int act, float* out,
                                int B, int Cin, int Cout, int H, int W, void* stream);
/* MaxPool2d(kernel 5, stride 1, padding 2) on [planes][H][W] */
int ipdm_maxpool5_f32(const float* x, float* y, int planes, int H, int W, void* stream);
/* CondCRPBlock's norm + AvgPool2d(5, stride 1, padding 2) (ncsn/models/layers.py:86-110) in one pass:
 * y = avg_pool(((x - mu) * scale + shift), 5, 1, 2, count_include_pad) per plane, coef [planes][3]; the padding is zero in the
 * normalised domain and every window divides by 25.  Any H, W; y != x. */
int ipdm_affine_avgpool5_f32(const float* x, const float* coef, float* y, int planes, int H, int W, void* stream);
/* 2x2 mean pooling (ConvMeanPool's tail) [planes][H][W] -> [planes][H/2][W/2]; H, W even */
int ipdm_meanpool2_f32(const float* x, float* y, int planes, int H, int W, void* stream);
/* bilinear resize, align_corners=True: out = act(resize(x) [+ out]); accumulate != 0 adds the previous out */
int ipdm_bilinear_f32(const float* x, float* out, int planes, int in_h, int in_w, int out_h, int out_w,
                      int accumulate, int act /* applied to the value written */,
                      int planes_per_image, float* amax_out /* NULL, or a maxima vector ([planes / planes_per_image] images) zeroed by the
                                                               caller: per-image max |value written| (atomic max), see ipdm_conv_ext_t */,
                      void* stream);
/* trilinear resize, align_corners=True, of [planes][D][H][W] volumes (the 3-D MSF block's F.interpolate,
 * ncsn/models/layers3d.py:185,214); same accumulate / act convention */
int ipdm_trilinear_f32(const float* x, float* out, int planes, int in_d, int in_h, int in_w, int out_d, int out_h,
                       int out_w, int accumulate, int act, int planes_per_image, float* amax_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * NCSN++ / predictor-corrector extras (reference: torch.nn.GroupNorm(eps 1e-6) in models/layerspp.py:66,219
 * and models/ncsnpp.py:194; torch.nn.Linear models/ncsnpp.py:85-90; AttnBlockpp.forward models/layerspp.py:75-91;
 * skip_rescale (x + h)/sqrt(2) models/layerspp.py:88-91,271-274; ReverseDiffusionPredictor / LangevinCorrector
 * update arithmetic sde/sampling.py:200-205, 267-287).
 * ---------------------------------------------------------------------------------------------- */
/* GroupNorm as per-(b,c) coefficients (mu, weight*rstd, bias) for ipdm_affine_act_f32 / the conv prologue */
int ipdm_groupnorm_coef_f32(const float* x, const float* weight, const float* bias, float* coef,
                            int B, int C, int HW, int G, float eps,
                            float* plane_amax /* may be NULL; [B][C]: max |x| per plane from the same pass (single-read
                                                 plane kernels only, IPDM_EUNSUPPORTED otherwise) */,
                            void* stream);
/* GroupNorm (+ activation) of torch.cat([x1, x2], dim=1) WITHOUT the concatenation (the up path of NCSN++ feeds every block
 * `torch.cat([h, hs.pop()], dim=1)`, models/ncsnpp.py:351): coefficients [B][C1+C2][3] from the two tensors' planes, then one
 * pass that writes the normalised, activated, concatenated tensor.  IPDM_EUNSUPPORTED outside the single-read plane kernels
 * (HW % 4 != 0, HW > 65536, more than 65535 planes): concatenate and use the one-tensor calls. */
/* ... from the statistics partials of the convolution(s) that produced the tensor(s) (the _stats_f32 convolution calls: [B][C][P][3]
 * = count, mean, sum of squared deviations per pixel block): the tensor is not read.  part2 / C2 (may be NULL / 0): the channels
 * >= C1 of torch.cat([x1, x2], dim=1). */
int ipdm_groupnorm_coef_partials_f32(const float* part1, int C1, const float* part2, int C2, int P, const float* weight,
                                     const float* bias, float* coef /* [B][C1+C2][3] */, int B, int G, float eps, void* stream);
int ipdm_groupnorm_coef_cat_f32(const float* x1, int C1, const float* x2, int C2, const float* weight, const float* bias,
                                float* coef, int B, int HW, int G, float eps, float* plane_amax /* may be NULL; [B][C1+C2] */,
                                void* stream);
int ipdm_affine_act_cat_f32(const float* x1, int C1, const float* x2, int C2, const float* coef, float* y, int B, int HW,
                            int act, void* stream);
/* y[b][o] = bias[o] + sum_i act(x[b][i]) * W[o][i]   (torch.nn.Linear weight layout [Out][In]) */
int ipdm_linear_f32(const float* x, const float* W, const float* bias, float* y, int B, int In, int Out,
                    int act, void* stream);
/* out[b,:,i] = sum_j softmax_j(scale * q[b,:,i].k[b,:,j]) v[b,:,j]   q,k,v,out [B][C][N] */
int ipdm_attention_f32(const float* q, const float* k, const float* v, float* out, int B, int C, int N,
                       float scale, void* stream);
/* out = a*x + b*y */
int ipdm_axpby_f32(const float* x, const float* y, float* out, int64_t n, float a, float b, void* stream);
/* out[s] = x[s] + a[s]*y[s] + c[s]*z[s] with per-sample device coefficients a, c [n_samples]; z/c may be NULL */
int ipdm_sample_axpy2_f32(const float* x, const float* y, const float* z, const float* a, const float* c,
                          float* out, int n_samples, int64_t sample_elems, void* stream);
/* norms[s] = ||x[s]||_2 */
int ipdm_sample_norm_f32(const float* x, float* norms, int n_samples, int64_t sample_elems, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense 3x3 / 1x1 convolution, float32 MFMA implicit GEMM (reference: torch.nn.Conv2d call sites in
 * ncsn/models/layers.py:28-60 conv1x1 / conv3x3 / dilated_conv3x3, stride 1, padding = dilation*(k/2)).
 *   out[b,co] = bias[co] + sum_ci W[co,ci] * pre(x[b,ci])  (+ residual[b,co])
 *   pre(v) = act((v - mu)*scale + shift) when coef != NULL (fused InstanceNorm2dPlus), else act(v)
 * wt is the weight repacked by ipdm_conv_pack_weight_f32: [k*k][Cin][Cout].
 * out_act (optional) receives act_out(out): the activated copy the NEXT convolution consumes (RCU / CRP chains
 * apply the non-linearity before every conv; producing it once in the epilogue is cheaper than activating in
 * each consumer's prologue).  out may be NULL when only the activated copy is needed.
 * pool2 != 0 additionally applies the 2x2 mean (ConvMeanPool) in the epilogue: out is [B][Cout][H/2][W/2].
 * ---------------------------------------------------------------------------------------------- */
int ipdm_conv_pack_weight_f32(const float* w /* [Cout][Cin][k][k] */, float* wt, int Cout, int Cin, int k, void* stream);
int ipdm_conv2d_f32(const float* x, const float* wt, const float* bias, const float* coef, int act,
                    const float* residual, float* out, float* out_act, int act_out,
                    int B, int Cin, int Cout, int H, int W, int k, int dilation, int pool2, void* stream);

/* Winograd F(2x2,3x3) variant of the 3x3 / dilation-1 convolution: 16 multiply-adds per 4 outputs instead of 36
 * (2.25x fewer MFMA cycles), exact-fp32 fma chains in the transformed domain.  U = G g G^T is produced once per
 * layer by ipdm_conv_wino_weight_f32 ([16][Cin][Cout]).  ipdm_conv2d_wino_supported tells whether a shape is
 * eligible (Cin % 8 == 0, Cout % 64 == 0; wide images: even H, W, dilation 1; small or dilated images: H and W
 * divisible by 2*dilation -- a dilated convolution is run as dilation^2 interleaved undilated ones); otherwise use
 * ipdm_conv2d_f32. */
int ipdm_conv_wino_weight_f32(const float* w /* [Cout][Cin][3][3] */, float* U, int Cout, int Cin, void* stream);
int ipdm_conv2d_wino_supported(int Cin, int Cout, int H, int W, int dilation);
int ipdm_conv2d_wino_f32(const float* x, const float* U, const float* bias, const float* residual, float* out,
                         float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                         void* stream);

/* tuning aid: when set (device buffer of 4*n_blocks uint64), the Winograd kernel's workgroups write s_memtime stamps
 * (start, loop start, loop end, end); NULL (default) disables it */
int ipdm_debug_set_stamp_buffer(void* buf);
/* how many times the library has raised a kernel's dynamic-LDS limit (hipFuncSetAttribute) in this process: once per kernel
 * instantiation, device and size above what was granted before -- steady-state launches add nothing */
int64_t ipdm_debug_lds_optin_count(void);

/* 3-D variant for the temporal prior (reference: nn.Conv3d(k=3, padding=dilation, dilation) call sites in
 * ncsn/models/layers3d.py and ncsn/models/ncsn3d.py:137,141): x [B][Cin][D][H][W], weights packed by
 * ipdm_conv_pack_weight_f32(k = 27) to [27][Cin][Cout] (k == 1: [1][Cin][Cout]).  Each depth slice is an
 * (H x W) image of the 2-D kernel; the three depth taps are three more passes over the K loop. */
int ipdm_conv3d_f32(const float* x, const float* wt, const float* bias, const float* coef, int act,
                    const float* residual, float* out, float* out_act, int act_out,
                    int B, int Cin, int Cout, int D, int H, int W, int k, int dilation, void* stream);

/* MaxPool3d(kernel 5, stride 1, padding 2) on [planes][D][H][W] (volumes up to 8192 voxels) */
int ipdm_maxpool3d5_f32(const float* x, float* y, int planes, int D, int H, int W, void* stream);
/* tap gather for the temporal (1,1,4)/stride-2 convolutions of NCSN3DShallow: x [planes][S][T_in] ->
 * out [planes][4][S][T_out]; mode 0 = strided conv (T_out = T_in/2), mode 1 = transposed conv (T_out = 2*T_in).
 * A 1x1 ipdm_conv2d_f32 over the 4*C gathered channels then IS the temporal convolution. */
int ipdm_temporal_taps_f32(const float* x, float* out, int planes, int S, int T_in, int T_out, int mode, void* stream);

/* Optional extras of the split-operand convolution calls below (`ext` may be NULL = all defaults).  A HOST struct, read when
 * the call is made (its device pointer member is dereferenced by the kernel):
 *   in_amax       f16x2 calls only: maxima vector of the input (ipdm_absmax_f32, or a producer's out_amax / act_amax / amax_out /
 *                 amax_bound) -> dynamic range, see the f16x2 note; NULL = static
 *   bias_bstride  bias index = image * bias_bstride + channel: Cout gives one bias ROW PER IMAGE (the reference's
 *                 `h += Dense_0(act(temb))[:, :, None, None]` after a convolution, models/layerspp.py:252-254, folded into the
 *                 epilogue); 0 = the usual per-channel bias
 *   out_amax / act_amax   see the struct
 *   out_scale     result = (conv + bias + residual) * out_scale -- the skip_rescale of the score_sde blocks,
 *                 (x + h) / sqrt(2) (models/layerspp.py:271-274), folded into the epilogue; 0 is read as 1 */
typedef struct {
  const float* in_amax;
  int bias_bstride;
  float out_scale;
  int res_second;    /* != 0: the residual enters the SECOND output only -- out = (conv + bias) * out_scale, out_act =          */
                     /* act_out((conv + bias + residual) * out_scale).  CRPBlock's `path = conv(pool(path)); x = path + x`          */
                     /* (ncsn/models/layers.py:76-83) as one launch: `path` and the running sum leave the same epilogue           */
  float* out_amax;   /* maxima vector ZEROED by the caller, or NULL: per-image max |out| of what the call stores, accumulated with  */
  float* act_amax;   /* atomic max (exact, order-independent) -- likewise for out_act.  What the NEXT f16x2 convolution takes as   */
                     /* in_amax: the dynamic range then costs no pass over the tensor (the reference has no counterpart: fp32)      */
} ipdm_conv_ext_t;

/* ---- fp32 convolution on the bf16 matrix cores ("bf16x3": exact three-way operand split, six
 * v_mfma_f32_32x32x16_bf16 per k-step, fp32 accumulation; fp32-faithful results at 2.67x the fp32 MFMA rate) ----
 * Same call sites, arguments and fused input / output options as ipdm_conv2d_f32 / ipdm_conv3d_f32; only the
 * packed-weight format differs: an opaque blob of ipdm_conv_bx3_weight_bytes(Cout, Cin, k) bytes written by
 * ipdm_conv_bx3_pack_weight (k = 1, 3, or 27 for a 3x3x3 kernel), valid for every batch / image size. */
int64_t ipdm_conv_bx3_weight_bytes(int Cout, int Cin, int k);
int ipdm_conv_bx3_pack_weight(const float* w /* [Cout][Cin][k][k] or [Cout][Cin][3][3][3] */, void* packed, int Cout,
                              int Cin, int k, void* stream);
int ipdm_conv2d_bx3_f32(const float* x, const void* packed, const float* bias, const float* coef, int act,
                        const float* residual, float* out, float* out_act, int act_out,
                        int B, int Cin, int Cout, int H, int W, int k, int dilation, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_conv3d_bx3_f32(const float* x, const void* packed, const float* bias, const float* coef, int act,
                        const float* residual, float* out, float* out_act, int act_out,
                        int B, int Cin, int Cout, int D, int H, int W, int k, int dilation, const ipdm_conv_ext_t* ext, void* stream);

/* Split-K form of the two calls above for shapes whose tiles alone leave most of the chip idle (small images at
 * small batch): ipdm_conv_bx3_splitk returns how many K parts pay (1 = use the plain call); with ksplit > 1 the parts
 * write raw partial sums to `work` (ksplit * B * Cout * D * H * W floats) and a second pass adds them in fixed order
 * (deterministic) together with bias / residual / activation.  volume: 0 = 2-D weights (D = 1), 1 = 3-D weights. */
int ipdm_conv_bx3_splitk(int B, int D, int Cin, int Cout, int H, int W, int k, int dilation);
int ipdm_conv_bx3_splitk_f32(const float* x, const void* packed, const float* bias, const float* coef, int act,
                             const float* residual, float* out, float* out_act, int act_out,
                             int B, int Cin, int Cout, int D, int H, int W, int k, int dilation, int volume, int ksplit,
                             float* work, const ipdm_conv_ext_t* ext, void* stream);

/* One torch.optim.Adam step (no weight decay / amsgrad) in place on x along the ASCENT direction g, i.e. with
 * param.grad = -g as the reference's MAP optimizers hand it over (ncsn/models/MAP_optimizers.py:72-74,103-105);
 * m, v: first / second moment buffers (zero-initialised by the caller), step = 1, 2, ... */
int ipdm_adam_ascent_f32(float* x, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                         float eps, int step, void* stream);

/* Winograd F(2x2,3x3) with split-bf16 operands (3x3, Cin % 16 == 0, Cout % 64 == 0, see ..._supported): the same
 * call sites and output options as ipdm_conv2d_wino_f32; weights transformed, split and laid out once per layer into
 * a blob of ipdm_conv_wino_bx3_weight_bytes(Cout, Cin) bytes. */
int64_t ipdm_conv_wino_bx3_weight_bytes(int Cout, int Cin);
int ipdm_conv_wino_bx3_pack_weight(const float* w /* [Cout][Cin][3][3] */, void* U, int Cout, int Cin, void* stream);
int ipdm_conv2d_wino_bx3_supported(int Cin, int Cout, int H, int W, int dilation);
/* pool2 != 0 (wide images, dilation 1): ConvMeanPool (layers.py:291-313) in one launch -- out / out_act / residual are
 * [B][Cout][H/2][W/2] and hold the 2x2 mean of the convolution (+ residual, activation); IPDM_EUNSUPPORTED where the
 * pooled epilogue is not built (the caller then runs the convolution and ipdm_meanpool2_f32 separately) */
int ipdm_conv2d_wino_bx3_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                             float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                             int pool2, const ipdm_conv_ext_t* ext, void* stream);
/* The same launch with the statistics epilogue: besides the result it writes, per (image, output channel), P partials
 * (count, mean, sum of squared deviations about that mean) of the stored result -- one per (tile block, tile group), a
 * function of the image geometry only -- to stats [B][Cout][P][3]; ipdm_instnorm_plus_coef_partials_f32 turns them into the
 * InstanceNorm++ coefficients of the FOLLOWING normalisation (normalization.py:163-176) without reading the tensor again.
 * ipdm_conv2d_wino_bx3_stats_partials returns P for a layer shape, 0 where the epilogue does not exist (small / dilated
 * images, W % 4 != 0): callers then use ipdm_instnorm_plus_coef_f32 on the tensor as before. */
/* Split-K form of the Winograd launch for 16-pixel layers with fewer than 512 output channels, whose (image, channel tile)
 * pairs alone leave most of the chip idle: ipdm_conv2d_wino_bx3_splitk returns the number of K parts for a layer shape (1: use
 * the plain call; a function of the shape only, never of the batch); with ksplit > 1 the parts write raw partial results to
 * `work` (ksplit * B * Cout * H * W floats) and a second pass adds them in fixed order with bias / residual / activation. */
int ipdm_conv2d_wino_bx3_splitk(int Cin, int Cout, int H, int W, int dilation);
int ipdm_conv2d_wino_bx3_splitk_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                                    float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                                    int ksplit, float* work, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_conv2d_wino_bx3_stats_partials(int Cin, int Cout, int H, int W, int dilation, int pool2);
int ipdm_conv2d_wino_bx3_stats_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                                   float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                                   int pool2, float* stats, const ipdm_conv_ext_t* ext, void* stream);
/* ---- "f16x2": the split-operand kernels above with TWO fp16 pieces per fp32 operand and THREE v_mfma_f32_32x32x16_f16 per
 * product (fp32 accumulation) -- half the matrix-core work and two thirds of the weight bytes of the three-way bf16 split.
 * fp32-faithful (error against float64 at or below the bf16 split's and the exact-fp32 kernel's on the networks' layer
 * shapes) under a RANGE contract: weights are scaled per output channel by a power of two at pack time (the inverse scale
 * rides in the blob); activations must satisfy |x| < 65504 (the Winograd calls pre-scale their input transform to keep that bound) -- beyond that the result
 * is NaN / inf (never a wrong finite number); the bx3 calls keep the whole fp32 exponent range.  DYNAMIC RANGE: `ext->in_amax`
 * (NULL = the static contract above) is the maxima vector of the input (ipdm_absmax_f32 measures one; producers hand theirs
 * over, see ipdm_conv_ext_t); the kernels
 * then scale every image by the power of two that puts its maximum in [2^14, 2^15) and undo it in the epilogue (both exact), so
 * ANY fp32 input is in range and values down to 2^-17 of an image's maximum keep all 22 bits.  (Ignored -- pass NULL -- when the
 * call fuses an input normalisation / activation: the normalised values are what is split.)  Same other arguments, semantics
 * and replaced reference interface (torch.nn.Conv2d / Conv3d inside ncsn/models/layers.py:28-60) as their bx3 twins; the
 * shape rules (ipdm_conv_bx3_splitk, ipdm_conv2d_wino_bx3_supported / _splitk / _stats_partials) are shared. */
int ipdm_absmax_f32(const float* x, float* amax /* maxima vector [n_images][IPDM_AMAX_SLOT], zeroed by the call */, int n_images,
                    int64_t per_image, void* stream);
int64_t ipdm_conv_hx2_weight_bytes(int Cout, int Cin, int k);
int ipdm_conv_hx2_pack_weight(const float* w /* [Cout][Cin][k][k] or [Cout][Cin][3][3][3] */, void* packed, int Cout,
                              int Cin, int k, void* stream);
int ipdm_conv2d_hx2_f32(const float* x, const void* packed, const float* bias, const float* coef, int act,
                        const float* residual, float* out, float* out_act, int act_out,
                        int B, int Cin, int Cout, int H, int W, int k, int dilation, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_conv3d_hx2_f32(const float* x, const void* packed, const float* bias, const float* coef, int act,
                        const float* residual, float* out, float* out_act, int act_out,
                        int B, int Cin, int Cout, int D, int H, int W, int k, int dilation, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_conv_hx2_splitk_f32(const float* x, const void* packed, const float* bias, const float* coef, int act,
                             const float* residual, float* out, float* out_act, int act_out,
                             int B, int Cin, int Cout, int D, int H, int W, int k, int dilation, int volume, int ksplit,
                             float* work, const ipdm_conv_ext_t* ext, void* stream);
int64_t ipdm_conv_wino_hx2_weight_bytes(int Cout, int Cin);
int ipdm_conv_wino_hx2_pack_weight(const float* w /* [Cout][Cin][3][3] */, void* U, int Cout, int Cin, void* stream);
int ipdm_conv2d_wino_hx2_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                             float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                             int pool2, const ipdm_conv_ext_t* ext, void* stream);
/* Which instantiation of the persistent 2-D Winograd kernel ipdm_conv2d_wino_hx2_f32 runs for a layer shape (a function of the
 * shape and of the IPDM_WBX3_* environment switches, never of the batch); IPDM_EUNSUPPORTED where the kernel does not apply.
 * CO32: (image, 32 output channels) workgroups; HALF: (image, upper / lower eight rows, 64 channels) workgroups -- both for
 * undilated <= 16-pixel layers with fewer than 512 output channels, HALF for the 16 x 16 ones; POLY: dilated 16 x 16 layers. */
#define IPDM_WINO_FORM_OTHER 0
#define IPDM_WINO_FORM_CO32 1
#define IPDM_WINO_FORM_HALF 2
#define IPDM_WINO_FORM_POLY 3
int ipdm_conv2d_wino_hx2_form(int Cin, int Cout, int H, int W, int dilation);
/* 1-D Winograd form of the same 3x3 convolution on f16x2 operands (conv_wino1d.hip): F(2,3) along x, the filter's three rows as
 * K -- 4 positions instead of 16, 128 output channels per workgroup, 12 instead of 16 weight values per (co, ci) and 1.5x the
 * matrix instructions.  Same arguments as ipdm_conv2d_wino_hx2_f32 without the dilation (undilated launches; Cin % 32 == 0,
 * Cout % 128 == 0, W % 4 == 0 and >= 32, H even and >= 8: ipdm_conv2d_wino1d_supported; activated copy: ELU or
 * IPDM_ACT_COPY); its own weight blob. */
int64_t ipdm_conv_wino1d_weight_bytes(int Cout, int Cin);
int ipdm_conv_wino1d_pack_weight(const float* w /* [Cout][Cin][3][3] */, void* U, int Cout, int Cin, void* stream);
int ipdm_conv2d_wino1d_supported(int Cin, int Cout, int H, int W);
/* The folded ConvMeanPool blob of the same kernel: the 2x2 mean's two rows summed (in fp32) into a 4-row filter g'[0] = g[0],
 * g'[1] = g[0] + g[1], g'[2] = g[1] + g[2], g'[3] = g[2] -- 16 positions, the same layout and scale table.  A pooled row is then
 * one contraction over four input rows: 16 instead of 24 multiply-adds per pooling window and (co, ci).  Only for
 * ipdm_conv2d_wino1d_f32 / _stats_f32 with pool2 = 2 and coef = NULL (a fused input: IPDM_EUNSUPPORTED); results agree with
 * the pool2 = 1 launch of the 12-position blob to fp32 rounding, not bit for bit. */
int64_t ipdm_conv_wino1d_pool_weight_bytes(int Cout, int Cin);
int ipdm_conv_wino1d_pack_weight_pool(const float* w /* [Cout][Cin][3][3] */, void* U, int Cout, int Cin, void* stream);
/* 3x3x3 convolution of volumes [B][C][D][H][W] on the same kernel: the depth taps are further K chunks (36 weight positions; blob
 * from ipdm_conv_wino1d_pack_weight3d, w [Cout][Cin][3][3][3]); planes of 12 pixels or less go two depth slices per row block.
 * Undilated, Cin % 32 == 0, Cout % 128 == 0, W % 4 == 0 and (W <= 12 or W >= 16): ipdm_conv3d_wino1d_supported. */
int64_t ipdm_conv_wino1d_weight_bytes3d(int Cout, int Cin);
int ipdm_conv_wino1d_pack_weight3d(const float* w, void* U, int Cout, int Cin, void* stream);
int ipdm_conv3d_wino1d_supported(int Cin, int Cout, int D, int H, int W);
int ipdm_conv3d_wino1d_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                           float* out_act, int act_out, int B, int Cin, int Cout, int D, int H, int W,
                           const ipdm_conv_ext_t* ext, void* stream);
/* coef != NULL: the input is act(InstanceNorm++(x)) -- coef [B][Cin][3] from ipdm_instnorm_plus_coef_f32, act = IPDM_ACT_ELU --
 * applied inside the kernel (as ipdm_conv2d_hx2_f32's fused input); ext->in_amax is then the coefficient kernel's bound.
 * pool2: 0 = the convolution, 1 = its 2x2 mean [B][Cout][H/2][W/2] from the 12-position blob, 2 = the same mean from the folded
 * blob of ipdm_conv_wino1d_pack_weight_pool (U must be that blob). */
int ipdm_conv2d_wino1d_f32(const float* x, const void* U, const float* bias, const float* coef, int act,
                           const float* residual, float* out, float* out_act, int act_out, int B, int Cin, int Cout, int H,
                           int W, int pool2, const ipdm_conv_ext_t* ext, void* stream);
/* ... with the statistics epilogue (as ipdm_conv2d_wino_hx2_stats_f32): stats[B][Cout][P][3] = (count, mean, sum of squared
 * deviations) of `out` per 8 x 32 pixel block, P = ipdm_conv2d_wino1d_stats_partials (0: not served) */
int ipdm_conv2d_wino1d_stats_partials(int Cin, int Cout, int H, int W);
int ipdm_conv2d_wino1d_stats_f32(const float* x, const void* U, const float* bias, const float* coef, int act,
                                 const float* residual, float* out, float* out_act, int act_out, int B, int Cin, int Cout,
                                 int H, int W, int pool2, float* stats, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_conv2d_wino_hx2_splitk_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                                    float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                                    int ksplit, float* work, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_conv2d_wino_hx2_stats_f32(const float* x, const void* U, const float* bias, const float* residual, float* out,
                                   float* out_act, int act_out, int B, int Cin, int Cout, int H, int W, int dilation,
                                   int pool2, float* stats, const ipdm_conv_ext_t* ext, void* stream);
int ipdm_instnorm_plus_coef_partials_f32(const float* partials, int P, const float* alpha, const float* gamma,
                                         const float* beta /* may be NULL */, float* coef /* [B][C][3] */, int B, int C,
                                         int HW /* elements per plane: only the bound needs it */, float* amax_bound /* as above */,
                                         void* stream);

/* conditional form of the above: embed / labels / num_classes / bias as in ipdm_cond_instnorm_plus_coef_f32 */
int ipdm_cond_instnorm_plus_coef_partials_f32(const float* partials, int P, const float* embed, const int64_t* labels,
                                              int num_classes, int bias, float* coef, int B, int C, int HW, float* amax_bound,
                                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * 1-D convolution of [N][C][L] sequences on the f16x2 arithmetic (conv1d.hip) -- the temporal score networks NCSN1D*
 * (reference: ncsn/models/layers1d.py:28-60 conv1x1 / conv3x3 / dilated_conv3x3 as nn.Conv1d, :63-84 CRPBlock, :113-135
 * RCUBlock, :166-187 MSFBlock, :296-324 ConvMeanPool, :415-470 ResidualBlock; ncsn/models/ncsn1d.py:53-56 begin / end
 * convolutions).  y[n][co][t] = bias[co] + sum_{ci,j} w[co][ci][j] x[n][ci][t + (j - k/2) * dilation], zero padding, k = 1 or 3,
 * dilation 1 / 2 / 4.  Served shapes (ipdm_conv1d_hx2_supported; IPDM_EUNSUPPORTED otherwise -- the caller then runs the
 * (N, C, 1, L) view on ipdm_conv2d_hx2_f32 with the filter in the middle row of a 3 x 3 one, which is the same convolution):
 * Cin % 16 == 0, Cout % 64 == 0, L >= 12 dividing 96.  x, residual, out, out_act at any 4-byte alignment.
 *   ext->in_amax: maxima vector with one slot per SEQUENCE (dynamic range: one power-of-two input scale per sequence);
 *   ext->out_amax / act_amax: per-sequence maxima of what is stored; ext->res_second as in ipdm_conv_ext_t; bias_bstride and
 *   out_scale are not served.  pool2 != 0: ConvMeanPool (layers1d.py:319-324) in one launch -- out / out_act / residual are
 *   [N][Cout][L/2] and hold (y[2j] + y[2j+1]) / 2 (+ residual, activation).  A sequence's result does not depend on N or on
 *   its position in the batch. */
int ipdm_conv1d_hx2_supported(int Cin, int Cout, int L, int k, int dilation);
int64_t ipdm_conv1d_hx2_weight_bytes(int Cout, int Cin, int k);
int ipdm_conv1d_hx2_pack_weight(const float* w /* [Cout][Cin][k] */, void* packed, int Cout, int Cin, int k, void* stream);
int ipdm_conv1d_hx2_f32(const float* x, const void* packed, const float* bias, const float* residual, float* out,
                        float* out_act, int act_out, int N, int Cin, int Cout, int L, int k, int dilation, int pool2,
                        const ipdm_conv_ext_t* ext, void* stream);
/* the pair mean on its own (layers1d.py:324; the kernel_size = 1 shortcut pools before its convolution):
 * y[row][j] = (x[row][2j] + x[row][2j+1]) / 2, L even */
int ipdm_meanpool1d2_f32(const float* x, float* y, int rows, int L, void* stream);
/* y = a * x + b with the per-image maxima of y (amax_out: a maxima vector ZEROED by the caller) -- the input rescale
 * `2 * x - 1` of ncsn/models/ncsn1d.py:104-108 as a producer of the first convolution's in_amax */
int ipdm_scale_shift_amax_f32(const float* x, float* y, float* amax_out, int n_images, int64_t per_image, float a, float b,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segmentation-likelihood guidance (reference: ncsn/models/__init__.py:197-215 compute_seg_grad through a MONAI UNet --
 * stride-2 Convolution / transposed Convolution blocks with InstanceNorm + PReLU --, ALD_optimizers.py:272-286).
 * The strided (transposed) convolutions and their input-gradients run on ipdm_conv2d_bx3_f32 between these:
 * ---------------------------------------------------------------------------------------------- */

/* out [planes][2H][2W]: out[2i][2j] = x[i][j], zero elsewhere */
int ipdm_zero_insert2_f32(const float* x, float* out, int planes, int H, int W, void* stream);
/* out [planes][Ho][Wo] = x[2i + oy][2j + ox]: a stride-2 convolution is the stride-1 one sampled at (oy, ox) + 2(i, j) */
int ipdm_subsample2_f32(const float* x, float* out, int planes, int H, int W, int oy, int ox, int Ho, int Wo, void* stream);
/* per-plane InstanceNorm (biased variance, eps, no affine) + PReLU with one slope (slope NULL: identity):
 * xhat = (x - mean) * rstd, y = prelu(xhat); rstd [planes] and xhat are what the backward needs */
int ipdm_in_prelu_fwd_f32(const float* x, const float* slope, float* xhat, float* y, float* rstd, int planes, int HW,
                          float eps, void* stream);
/* input-gradient of ipdm_in_prelu_fwd_f32 */
int ipdm_in_prelu_bwd_f32(const float* gy, const float* xhat, const float* rstd, const float* slope, float* gx, int planes,
                          int HW, void* stream);
/* the same with the forward's eps (> 0): at HW = 2, where the gradient is eps rstd^2 of the terms of its formula and the fp32 xhat
 * no longer holds it, the closed form gx = +-eps rstd^3 (g_h0 - g_h1) / 2 is taken; every other HW is ipdm_in_prelu_bwd_f32 */
int ipdm_in_prelu_bwd_eps_f32(const float* gy, const float* xhat, const float* rstd, const float* slope, float* gx, int planes,
                              int HW, float eps, void* stream);
/* g = d/dlogits sum log softmax(logits)[label]: g[b][c][p] = [c == label[b][p]] - softmax_c; logits [B][C][HW], label int64 */
int ipdm_seg_loglh_grad_f32(const float* logits, const int64_t* label, float* g, int B, int C, int64_t HW, void* stream);
/* y += scale * x (* mask[i % mask_period], the "FG" mode); scale = dev_sched->seg_scale when dev_sched is non-NULL */
int ipdm_axpy_sched_f32(float* y, const float* x, const int64_t* mask, int64_t mask_period, const ipdm_sched_t* dev_sched,
                        float scale, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device reporting (reference: helpers/metrics.py:21-102, helpers/visualizations.py:93,117,121).  Deterministic
 * float64 reductions; metrics are per image (one result per image in `out`, device float64).
 * ---------------------------------------------------------------------------------------------- */

/* out[i] = |x[i]| */
int ipdm_magnitude_c64(const float* x /* n complex64 */, float* out, int64_t n, void* stream);
/* samples [n_samples][HW] complex64 -> planes [7][HW] float64: sum |x|, sum |x|^2, sum angle, sum angle^2, sum Re,
 * sum Im, sum |angle| over the samples (compute_mean_and_std, helpers/metrics.py:77-92, as partial sums a shard can
 * all-reduce; the reference's phase std is np.std(np.abs(angle)), hence the last plane) */
int ipdm_posterior_moments_c64(const float* samples, double* planes, int n_samples, int64_t HW, void* stream);
/* NRMSE_wrapper (helpers/metrics.py:70-74): skimage normalized_root_mse(img, ref, "euclidean") = ||img - ref|| / ||img||,
 * img [n_images][elems]; ref [n_images][elems] or one [elems] image shared by all (ref_broadcast) */
int ipdm_nrmse_f32(const float* img, const float* ref, double* out, int n_images, int64_t elems, int ref_broadcast,
                   void* stream);
/* SSIM_wrapper (helpers/metrics.py:55-67) on single-channel [H][W] images: skimage structural_similarity defaults
 * (7x7 uniform window, K1 0.01, K2 0.03, sample covariance, mean over the valid interior) with an explicit data_range */
int ipdm_ssim_f32(const float* img, const float* ref, double* out, int n_images, int H, int W, int ref_broadcast,
                  double data_range, void* stream);

/* Total-variation baseline (reference: scripts/acdc_SENSE_TV.py:76-83 + ncsn/models/MAP_optimizers.py:26-52 MAPModel with
 * kornia.losses.TotalVariation): x, g complex64 [n_images][H][W] (interleaved re/im).
 * ipdm_tv_c64: out[b] = sum |x[i+1,j]-x[i,j]| + sum |x[i,j+1]-x[i,j]| (float64);
 * ipdm_tv_grad_c64: the gradient autograd gives for the complex parameter (unit difference vectors, 0 at a zero difference). */
int ipdm_tv_c64(const float* x, double* out, int n_images, int H, int W, void* stream);
int ipdm_tv_grad_c64(const float* x, float* g, int n_images, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IPDM_H */
