// k-space side of the ALD step on gfx950: centred orthonormal 2-D FFT held entirely in one CU's LDS
// (128x128 complex64 = 128 KiB of the 160 KiB), multi-coil SENSE forward / adjoint / SSOS, the
// closed form of the reference's one-SGD-step L2Penalty proximal, and the fused Langevin + proximal
// iteration tail.  One 1024-thread workgroup owns one image; coils are looped inside the workgroup so
// the coil sum is deterministic (no atomics).  All of this is launch/latency-bound work (~1 MiB of
// algorithmic traffic per sample per step) that rides beside the score network.
//
// The fftshift/ifftshift pairs of i2k_complex / k2i_complex (ncsn/linear_transforms/__init__.py:36-57)
// are folded into (-1)^(r+c) sign flips before and after an ordinary FFT (exact for sizes % 4 == 0);
// sizes without an FFT kernel (ipdm_kspace_size_class) go through a direct centred DFT with an exact integer phase index.
#include "kspace_fft.h"

namespace {

using namespace ipdm_kspace;

// ---------------------------------------------------------------------------------------------
// MIXED (every FFT kernel here): sides with factors 3 or 5, kspace_fft.h; chosen at launch by fft_dispatch
template <bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void fft2c_lds_kernel(const float2* in, float2* out,
                                                                int H, int W, int inverse) {
  FFT_LDS_SETUP(H, W, MIXED)
  const int HW = H * W;
  const float2* src = in + (size_t)blockIdx.x * HW;
  float2* dst = out + (size_t)blockIdx.x * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float s = sign_rc(r, c);
    float2 v = src[e];
    L.buf[e] = make_float2(v.x * s, v.y * s);
  }
  __syncthreads();
  fft2_lds<MIXED>(L, H, W, inverse != 0);
  const float scale = rsqrtf((float)HW);
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float s = sign_rc(r, c) * scale;
    float2 v = L.buf[e];
    dst[e] = make_float2(v.x * s, v.y * s);
  }
}

// direct centred DFT along the last axis, output transposed: in [batch][R][N] -> out [batch][N][R]
__global__ __launch_bounds__(256) void dft_rows_transposed_kernel(const float2* __restrict__ in,
                                                                  float2* __restrict__ out, int R, int N, int inverse) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float2* row = reinterpret_cast<float2*>(smem_raw);
  float2* tw = row + N;
  const int b = blockIdx.y, r = blockIdx.x;
  const float2* src = in + ((size_t)b * R + r) * N;
  const double sgn = inverse ? 2.0 : -2.0;
  const float scale = (float)(1.0 / sqrt((double)N));
  for (int q = threadIdx.x; q < N; q += blockDim.x) {
    double s, c;
    sincospi(sgn * (double)q / (double)N, &s, &c);
    tw[q] = make_float2((float)c * scale, (float)s * scale);
    row[q] = src[q];
  }
  __syncthreads();
  const int cshift = N / 2;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    int dk = ((k - cshift) % N + N) % N;
    int p = (int)(((int64_t)(N - cshift) * dk) % N);     // (m - c)(k - c) mod N at m = 0
    float2 acc = make_float2(0.f, 0.f);
    for (int m = 0; m < N; ++m) {
      float2 w = tw[p], x = row[m];
      acc.x += x.x * w.x - x.y * w.y;
      acc.y += x.x * w.y + x.y * w.x;
      p += dk;
      if (p >= N) p -= N;
    }
    out[((size_t)b * N + k) * R + r] = acc;
  }
}

// ---------------------------------------------------------------------------------------------

// SensT (here and below): the coil maps' element type, float or float2 (interleaved complex64); the products are
// sens_mul / sens_mul_conj of kspace_fft.h
template <typename SensT, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void sense_forward_kernel(const float2* __restrict__ x,
                                                                    const SensT* __restrict__ sens, int sens_sets,
                                                                    const uint8_t* __restrict__ mask, int mask_t,
                                                                    float2* __restrict__ y, int B, int H, int W) {
  FFT_LDS_SETUP(H, W, MIXED)
  const int HW = H * W;
  const int b = blockIdx.x, coil = blockIdx.y;
  const float2* src = x + (size_t)b * HW;
  const SensT* set = sens_at(sens, sens_sets, b, (size_t)gridDim.y * HW);      // gridDim.y: n_coils
  const SensT* sm = set ? set + (size_t)coil * HW : nullptr;        // NULL: single coil, S = 1
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float s = sign_rc(r, c);
    float2 v = src[e];
    L.buf[e] = sm ? sens_mul(v, s, sm[e]) : make_float2(v.x * s, v.y * s);
  }
  __syncthreads();
  fft2_lds<MIXED>(L, H, W, false);
  const float scale = rsqrtf((float)HW);
  float2* dst = y + ((size_t)coil * B + b) * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float2 v = L.buf[e];
    float s = mask_at(mask, mask_t, b, H, W, r, c) ? sign_rc(r, c) * scale : 0.f;
    dst[e] = make_float2(v.x * s, v.y * s);
  }
}

// s [n_coils][B][H][W] -> out[b] = sum_c S_c * ifft2c(s[c][b])  (or root-sum-of-squares for SSOS).
// The coil sum is accumulated in the (L2-resident) output image, coil by coil in index order, like the
// reference's `X_out += ...` loop: no accumulator registers live across the FFT, deterministic.
template <bool SSOS, typename SensT, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void sense_adjoint_kernel(const float2* __restrict__ s,
                                                                    const SensT* __restrict__ sens, int sens_sets,
                                                                    const uint8_t* __restrict__ mask, int mask_t,
                                                                    int apply_mask, float* out, int B,
                                                                    int n_coils, int H, int W) {
  FFT_LDS_SETUP(H, W, MIXED)
  const int HW = H * W;
  const int b = blockIdx.x;
  const float scale = rsqrtf((float)HW);
  const SensT* set = sens_at(sens, sens_sets, b, (size_t)n_coils * HW);
  for (int coil = 0; coil < n_coils; ++coil) {
    const float2* src = s + ((size_t)coil * B + b) * HW;
    for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
      int r = e / W, c = e - r * W;
      float sg = sign_rc(r, c);
      if (apply_mask && !mask_at(mask, mask_t, b, H, W, r, c)) sg = 0.f;
      float2 v = src[e];
      L.buf[e] = make_float2(v.x * sg, v.y * sg);
    }
    __syncthreads();
    fft2_lds<MIXED>(L, H, W, true);
    const bool last = coil == n_coils - 1;
    for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
      float2 v = L.buf[e];
      size_t gi = (size_t)b * HW + e;
      if constexpr (SSOS) {
        float a = (v.x * v.x + v.y * v.y) * (scale * scale);
        if (coil > 0) a += out[gi];
        out[gi] = last ? sqrtf(a) : a;
      } else {
        int r = e / W, c = e - r * W;
        float2 a = sens_mul_conj(v, sign_rc(r, c) * scale, set[(size_t)coil * HW + e]);
        float2* o = reinterpret_cast<float2*>(out) + gi;
        if (coil > 0) {
          float2 prev = *o;
          a.x += prev.x;
          a.y += prev.y;
        }
        *o = a;
      }
    }
    __syncthreads();
  }
}

// Langevin update of one sample's two planes, in place (the first phase of the fused iteration tails): x = langevin_value
__device__ __forceinline__ void langevin_phase(float* xr, float* xi, const LangevinArgs& lg, int b, int HW) {
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    float zr, zi;
    langevin_value(xr, xi, lg, b, HW, e, zr, zi);
    xr[e] = zr;
    xi[e] = zi;
  }
}

// Langevin update (optional) + L2Penalty closed form, planar real/imag, in place.
//   phase 0: z = x + step*g + noise_scale*n           -> stored back to x (global, L2-resident)
//   per coil: LDS = S_c z ; FFT ; residual on sampled columns ; IFFT ; work += S_c * (.)
//   final:   x = z - coef * work
// `work` ([B][H][W] c64) carries the coil sum so that no accumulator registers live across the FFTs.
template <bool LANGEVIN, typename SensT, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void ald_sense_step_kernel(float* x_re, float* x_im, LangevinArgs lg,
                                                                     const SenseProblem<SensT> pb, float coef, float2* work) {
  const int B = pb.B, n_coils = pb.n_coils, H = pb.H, W = pb.W, mask_t = pb.mask_t;
  const float2* __restrict__ y = pb.y;
  const uint8_t* __restrict__ mask = pb.mask;
  FFT_LDS_SETUP(H, W, MIXED)
  const int HW = H * W;
  const int b = blockIdx.x;
  coef = sched_override(lg, b, coef);
  const SensT* __restrict__ sens = sens_at(pb.sens, pb.sens_sets, b, (size_t)n_coils * HW);
  const float scale = rsqrtf((float)HW);
  float* xr = x_re + (size_t)b * HW;
  float* xi = x_im + (size_t)b * HW;
  float2* wk = work + (size_t)b * HW;
  if constexpr (LANGEVIN) langevin_phase(xr, xi, lg, b, HW);
  if (coef == 0.f) return;
  // pass 2c: forward transform of S_c z ; pass 2c+1: inverse transform of the masked residual
  for (int pass = 0; pass < 2 * n_coils; ++pass) {
    const int coil = pass >> 1;
    const bool inv = pass & 1;
    const SensT* sm = sens + (size_t)coil * HW;
    if (!inv) {
      for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
        int r = e / W, c = e - r * W;
        L.buf[e] = sens_mul(make_float2(xr[e], xi[e]), sign_rc(r, c), sm[e]);
      }
    }
    __syncthreads();
    fft2_lds<MIXED>(L, H, W, inv);
    if (!inv) {
      const float2* yc = y + ((size_t)coil * B + b) * HW;
      for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
        int r = e / W, c = e - r * W;
        float2 v = L.buf[e];
        L.buf[e] = masked_residual(mask_at(mask, mask_t, b, H, W, r, c), make_float2(v.x * scale, v.y * scale), sign_rc(r, c),
                                   yc + e);
      }
    } else {
      const bool last = coil == n_coils - 1;
      for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
        int r = e / W, c = e - r * W;
        float2 v = L.buf[e];
        float2 a = sens_mul_conj(v, sign_rc(r, c) * scale, sm[e]);
        if (coil > 0) {
          float2 prev = wk[e];
          a.x += prev.x;
          a.y += prev.y;
        }
        if (last) {
          xr[e] = xr[e] - coef * a.x;
          xi[e] = xi[e] - coef * a.y;
        } else {
          wk[e] = a;
        }
      }
    }
  }
}

// The normal operator with the coils in parallel (launch_normal_coils, kspace_fft.h), the first half of the coil-parallel
// iteration tail and of every conjugate-gradient step.  A rank's batch is 13-14 samples, i.e. 14 of 256 CUs busy for four
// dependent (FFT, inverse FFT) pairs in the one-workgroup-per-sample kernel above.  Here workgroup (coil, b) forms its input
// v in registers (MODE 2: every coil workgroup of a sample computes the same Langevin update z: the noise is injected or a
// pure function of (seed, sample, step, element)), does ITS coil's transform pair and writes
// r_c = conj(S_c) F^-1[M (F S_c v - y_c)] to planes[b][coil]: 56 workgroups instead of 14, one transform pair deep instead
// of four.
template <int MODE, typename SensT, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void sense_normal_coil_kernel(const float* x_re, const float* x_im, LangevinArgs lg,
                                                                        float coef, const float2* __restrict__ p,
                                                                        const CgState* __restrict__ state,
                                                                        const SenseProblem<SensT> pb, float2* __restrict__ planes) {
  const int B = pb.B, n_coils = pb.n_coils, H = pb.H, W = pb.W, mask_t = pb.mask_t;
  const uint8_t* __restrict__ mask = pb.mask;
  const int coil = blockIdx.x, b = blockIdx.y;
  if constexpr (MODE == 0) {
    if (state[b].frozen) return;
  } else {
    // the tail's combine pass then only applies the Langevin update; the CG init pass leaves x = z and freezes the sample
    if (sched_override(lg, b, coef) == 0.f) return;
  }
  FFT_LDS_SETUP(H, W, MIXED)
  const int HW = H * W;
  const float scale = rsqrtf((float)HW);
  const SensT* __restrict__ sm = sens_at(pb.sens, pb.sens_sets, b, (size_t)n_coils * HW) + (size_t)coil * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    float2 v;
    if constexpr (MODE == 0) {
      v = p[(size_t)b * HW + e];
    } else {
      const float* xr = x_re + (size_t)b * HW;
      const float* xi = x_im + (size_t)b * HW;
      v = make_float2(xr[e], xi[e]);
      if constexpr (MODE == 2) langevin_value(xr, xi, lg, b, HW, e, v.x, v.y);
    }
    const int r = e / W, c = e - r * W;
    L.buf[e] = sens_mul(v, sign_rc(r, c), sm[e]);
  }
  __syncthreads();
  fft2_lds<MIXED>(L, H, W, false);
  const float2* __restrict__ yc = MODE == 0 ? nullptr : pb.y + ((size_t)coil * B + b) * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    const int r = e / W, c = e - r * W;
    const float2 v = L.buf[e];
    L.buf[e] = masked_residual(mask_at(mask, mask_t, b, H, W, r, c), make_float2(v.x * scale, v.y * scale), sign_rc(r, c),
                               MODE == 0 ? nullptr : yc + e);
  }
  __syncthreads();
  fft2_lds<MIXED>(L, H, W, true);
  float2* wk = planes + ((size_t)b * n_coils + coil) * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    const int r = e / W, c = e - r * W;
    wk[e] = sens_mul_conj(L.buf[e], sign_rc(r, c) * scale, sm[e]);
  }
}

// Second half of the coil-parallel tail: forms z once more and x = z - coef * (((r_0 + r_1) + r_2) + ...), the sequential
// kernel's order: bit-identical results.
template <bool LANGEVIN>
__global__ __launch_bounds__(256) void ald_sense_combine_kernel(float* x_re, float* x_im, LangevinArgs lg, float coef,
                                                                const float2* __restrict__ work, int n_coils, int HW) {
  const int b = blockIdx.y;
  coef = sched_override(lg, b, coef);
  float* xr = x_re + (size_t)b * HW;
  float* xi = x_im + (size_t)b * HW;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += gridDim.x * 256) {
    float zr = xr[e], zi = xi[e];
    if constexpr (LANGEVIN) langevin_value(xr, xi, lg, b, HW, e, zr, zi);
    if (coef != 0.f) {
      const float2 a = plane_sum(work + (size_t)b * n_coils * HW, n_coils, HW, e);
      zr = zr - coef * a.x;
      zi = zi - coef * a.y;
    }
    xr[e] = zr;
    xi[e] = zi;
  }
}

// Single-coil iteration tail (RandomUndersamplingFourier: A = M F, no coil maps), planar real/imag, in place:
// Langevin update (optional) + one of the reference's three single-coil data-consistency operators
//   mode 0  L2Penalty   x = z - coef * F^-1[ M (M F z - y) ]               (proximal_op.py:19-51, coef = 0.05 a/(l K), K = B)
//   mode 1  SingleCoil  x = F^-1[ (F z + coef*y) / (1 + coef*M) ]          (proximal_op.py:72-94, coef = alpha/lamda)
//   mode 2  projection  x = F^-1[ coef*y + (1-coef) M F z + (1-M) F z ]   (undersampling_fourier.py:89-97, coef = lamda)
// The image stays in LDS between the two transforms; z is re-read from x (L2-resident) for mode 0.  pb.sens is not used.
template <bool LANGEVIN, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void ald_singlecoil_step_kernel(float* x_re, float* x_im, LangevinArgs lg,
                                                                          const SenseProblem<float> pb, float coef, int mode) {
  const int H = pb.H, W = pb.W, mask_t = pb.mask_t;
  const float2* __restrict__ y = pb.y;
  const uint8_t* __restrict__ mask = pb.mask;
  FFT_LDS_SETUP(H, W, MIXED)
  const int HW = H * W;
  const int b = blockIdx.x;
  coef = sched_override(lg, b, coef);
  const float scale = rsqrtf((float)HW);
  float* xr = x_re + (size_t)b * HW;
  float* xi = x_im + (size_t)b * HW;
  if constexpr (LANGEVIN) langevin_phase(xr, xi, lg, b, HW);
  if (mode == 0 && coef == 0.f) return;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float sg = sign_rc(r, c);
    L.buf[e] = make_float2(xr[e] * sg, xi[e] * sg);
  }
  __syncthreads();
  fft2_lds<MIXED>(L, H, W, false);
  // k-space value K = sg*scale*v; the inverse transform wants sg*K' -> every formula is written on scale*v and sg*y
  const float2* yb = y + (size_t)b * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float2 v = L.buf[e];
    v.x *= scale;
    v.y *= scale;
    const bool m = mask_at(mask, mask_t, b, H, W, r, c);
    float2 o;
    if (mode == 0) {
      o = masked_residual(m, v, sign_rc(r, c), yb + e);
    } else if (mode == 1) {
      float sg = sign_rc(r, c) * coef;
      float2 yy = yb[e];
      float inv = m ? 1.f / (1.f + coef) : 1.f;
      o = make_float2((v.x + sg * yy.x) * inv, (v.y + sg * yy.y) * inv);
    } else {
      float sg = sign_rc(r, c) * coef;
      float2 yy = yb[e];
      float keep = m ? 1.f - coef : 1.f;
      o = make_float2(sg * yy.x + keep * v.x, sg * yy.y + keep * v.y);
    }
    L.buf[e] = o;
  }
  __syncthreads();
  fft2_lds<MIXED>(L, H, W, true);
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    int r = e / W, c = e - r * W;
    float2 v = L.buf[e];
    float w = sign_rc(r, c) * scale;
    if (mode == 0) {
      xr[e] = xr[e] - coef * (v.x * w);
      xi[e] = xi[e] - coef * (v.y * w);
    } else {
      xr[e] = v.x * w;
      xi[e] = v.y * w;
    }
  }
}

template <int MODE, typename SensT>
static int launch_normal_coils_mode(const float* x_re, const float* x_im, const LangevinArgs& lg, float coef, const float2* p,
                                    const CgState* state, const SenseProblem<SensT>& pb, float2* planes, hipStream_t st) {
  const size_t lds = lds_bytes(pb.H, pb.W);
  return fft_dispatch(fft_mixed(pb.H, pb.W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    const int rc = ipdm_lds_optin(sense_normal_coil_kernel<MODE, SensT, MIXED>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((sense_normal_coil_kernel<MODE, SensT, MIXED>), dim3(pb.n_coils, pb.B), dim3(FFT_THREADS), lds, st, x_re,
                       x_im, lg, coef, p, state, pb, planes);
    return ipdm_launch_status();
  });
}

// the coil-parallel iteration tail: normal operator per coil, then the combine pass
template <typename SensT>
static int launch_sense_step_coils(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb, float coef,
                                   float2* work, hipStream_t st) {
  if (pb.B > 65535) return IPDM_EUNSUPPORTED;
  const int rc = launch_normal_coils(lg.g_re ? 2 : 1, x_re, x_im, lg, coef, nullptr, nullptr, pb, work, st);
  if (rc) return rc;
  const int HW = pb.H * pb.W;
  int gx = (HW + 255) / 256;
  if (gx > 64) gx = 64;
  if (lg.g_re)
    hipLaunchKernelGGL(ald_sense_combine_kernel<true>, dim3(gx, pb.B), dim3(256), 0, st, x_re, x_im, lg, coef, work, pb.n_coils, HW);
  else
    hipLaunchKernelGGL(ald_sense_combine_kernel<false>, dim3(gx, pb.B), dim3(256), 0, st, x_re, x_im, lg, coef, work, pb.n_coils, HW);
  return ipdm_launch_status();
}

}  // namespace

template <typename SensT>
int ipdm_kspace::launch_normal_coils(int mode, const float* x_re, const float* x_im, const LangevinArgs& lg, float coef,
                                     const float2* p, const CgState* state, const SenseProblem<SensT>& pb, float2* planes,
                                     hipStream_t st) {
  if (mode == 0) return launch_normal_coils_mode<0>(x_re, x_im, lg, coef, p, state, pb, planes, st);
  if (mode == 1) return launch_normal_coils_mode<1>(x_re, x_im, lg, coef, p, state, pb, planes, st);
  return launch_normal_coils_mode<2>(x_re, x_im, lg, coef, p, state, pb, planes, st);
}
template int ipdm_kspace::launch_normal_coils(int, const float*, const float*, const LangevinArgs&, float, const float2*,
                                              const CgState*, const SenseProblem<float>&, float2*, hipStream_t);
template int ipdm_kspace::launch_normal_coils(int, const float*, const float*, const LangevinArgs&, float, const float2*,
                                              const CgState*, const SenseProblem<float2>&, float2*, hipStream_t);

extern "C" int ipdm_kspace_size_class(int H, int W) {
  if (H <= 0 || W <= 0) return IPDM_KSPACE_NONE;
  if (lds_fft_ok(H, W)) return IPDM_KSPACE_LDS;
  return ipdm_kspace_large::large_ok(H, W) ? IPDM_KSPACE_STRIPS : IPDM_KSPACE_NONE;
}

extern "C" int64_t ipdm_fft2c_workspace_bytes(int batch, int H, int W) {
  if (batch <= 0 || H <= 0 || W <= 0) return 0;
  return (lds_fft_ok(H, W) || ipdm_kspace_large::large_ok(H, W)) ? 0 : (int64_t)batch * H * W * 8;
}

// IPDM_SENSE_COILS=0: the one-workgroup-per-sample kernel (tuning / comparison; same bits)
static int sense_coil_parallel() {
  static const int v = ipdm_env_int("IPDM_SENSE_COILS", 1);
  return v;
}

extern "C" int64_t ipdm_sense_workspace_bytes(int B, int n_coils, int H, int W) {
  if (B <= 0 || n_coils <= 0 || H <= 0 || W <= 0) return 0;
  if (lds_fft_ok(H, W)) return (int64_t)B * n_coils * H * W * 8;   // one plane per (sample, coil): the coil-parallel path
  return ipdm_kspace_large::workspace_bytes(B, n_coils, H, W);
}

extern "C" int ipdm_fft2c_c64(const float* in, float* out, int batch, int H, int W, int inverse, float* workspace,
                              void* stream) {
  IPDM_REQUIRE(batch >= 0 && H > 0 && W > 0 && H <= 1024 && W <= 1024);
  if (batch == 0) return IPDM_OK;
  IPDM_REQUIRE(in && out);
  hipStream_t s = ipdm_stream(stream);
  if (lds_fft_ok(H, W)) {
    size_t lds = lds_bytes(H, W);
    return fft_dispatch(fft_mixed(H, W), [&](auto mixed) {
      constexpr bool MIXED = decltype(mixed)::value;
      int rc = ipdm_lds_optin(fft2c_lds_kernel<MIXED>, lds);
      if (rc) return rc;
      hipLaunchKernelGGL(fft2c_lds_kernel<MIXED>, dim3(batch), dim3(FFT_THREADS), lds, s, reinterpret_cast<const float2*>(in),
                         reinterpret_cast<float2*>(out), H, W, inverse);
      return ipdm_launch_status();
    });
  }
  if (ipdm_kspace_large::large_ok(H, W))
    return ipdm_kspace_large::fft2c(reinterpret_cast<const float2*>(in), reinterpret_cast<float2*>(out), batch, H, W,
                                    inverse, s);
  IPDM_REQUIRE(workspace);
  // pass 1: DFT along W, [b][H][W] -> ws [b][W][H]; pass 2: DFT along H, ws -> out [b][H][W]
  hipLaunchKernelGGL(dft_rows_transposed_kernel, dim3(H, batch), dim3(256), (size_t)2 * W * sizeof(float2), s,
                     reinterpret_cast<const float2*>(in), reinterpret_cast<float2*>(workspace), H, W, inverse);
  hipLaunchKernelGGL(dft_rows_transposed_kernel, dim3(W, batch), dim3(256), (size_t)2 * H * sizeof(float2), s,
                     reinterpret_cast<const float2*>(workspace), reinterpret_cast<float2*>(out), W, H, inverse);
  return ipdm_launch_status();
}

template <typename SensT>
static int sense_forward_impl(const float* x, const SenseProblem<SensT>& pb, float* y, void* stream) {
  IPDM_REQUIRE(dims_ok(pb));
  if (pb.B == 0) return IPDM_OK;
  IPDM_REQUIRE(x && pb.mask && y && (pb.sens || pb.n_coils == 1));
  if (ipdm_kspace_large::large_ok(pb.H, pb.W))
    return ipdm_kspace_large::sense_forward(reinterpret_cast<const float2*>(x), pb, reinterpret_cast<float2*>(y),
                                            ipdm_stream(stream));
  if (!lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  size_t lds = lds_bytes(pb.H, pb.W);
  return fft_dispatch(fft_mixed(pb.H, pb.W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    int rc = ipdm_lds_optin(sense_forward_kernel<SensT, MIXED>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((sense_forward_kernel<SensT, MIXED>), dim3(pb.B, pb.n_coils), dim3(FFT_THREADS), lds, ipdm_stream(stream),
                       reinterpret_cast<const float2*>(x), pb.sens, pb.sens_sets, pb.mask, pb.mask_t, reinterpret_cast<float2*>(y),
                       pb.B, pb.H, pb.W);
    return ipdm_launch_status();
  });
}

// pb.y: the coil images s; pb.mask_t is looked at only with apply_mask
template <typename SensT>
static int sense_adjoint_impl(SenseProblem<SensT> pb, int apply_mask, float* x, float* workspace, void* stream) {
  IPDM_REQUIRE(pb.B >= 0 && pb.n_coils > 0 && pb.H > 0 && pb.W > 0 && pb.sens_sets >= 1);
  if (pb.B == 0) return IPDM_OK;
  IPDM_REQUIRE(pb.y && pb.sens && x);
  if (apply_mask) IPDM_REQUIRE(pb.mask && mask_t_ok(pb.mask_t));
  else pb.mask_t = 1;
  if (ipdm_kspace_large::large_ok(pb.H, pb.W)) {
    IPDM_REQUIRE(workspace);
    return ipdm_kspace_large::sense_adjoint(pb, apply_mask, reinterpret_cast<float2*>(x), nullptr,
                                            reinterpret_cast<float2*>(workspace), ipdm_stream(stream));
  }
  if (!lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  size_t lds = lds_bytes(pb.H, pb.W);
  return fft_dispatch(fft_mixed(pb.H, pb.W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    int rc = ipdm_lds_optin(sense_adjoint_kernel<false, SensT, MIXED>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((sense_adjoint_kernel<false, SensT, MIXED>), dim3(pb.B), dim3(FFT_THREADS), lds, ipdm_stream(stream), pb.y,
                       pb.sens, pb.sens_sets, pb.mask, pb.mask_t, apply_mask, x, pb.B, pb.n_coils, pb.H, pb.W);
    return ipdm_launch_status();
  });
}

extern "C" int ipdm_sense_forward_c64(const float* x, const float* sens, const uint8_t* mask, int mask_t, float* y,
                                      int B, int n_coils, int H, int W, void* stream) {
  return sense_forward_impl(x, sense_problem<float>(nullptr, sens, mask, mask_t, B, n_coils, H, W), y, stream);
}

extern "C" int ipdm_sense_forward_csm_c64(const float* x, const float* sens, const uint8_t* mask, int mask_t, float* y,
                                          int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(sens || B == 0);                                 // no single-coil shortcut here: complex maps are required
  return sense_forward_impl(x, sense_problem<float2>(nullptr, sens, mask, mask_t, B, n_coils, H, W), y, stream);
}

extern "C" int ipdm_sense_adjoint_c64(const float* s, const float* sens, const uint8_t* mask, int mask_t,
                                      int apply_mask, float* x, float* workspace, int B, int n_coils, int H, int W,
                                      void* stream) {
  return sense_adjoint_impl(sense_problem<float>(s, sens, mask, mask_t, B, n_coils, H, W), apply_mask, x, workspace, stream);
}

extern "C" int ipdm_sense_adjoint_csm_c64(const float* s, const float* sens, const uint8_t* mask, int mask_t,
                                          int apply_mask, float* x, float* workspace, int B, int n_coils, int H, int W,
                                          void* stream) {
  return sense_adjoint_impl(sense_problem<float2>(s, sens, mask, mask_t, B, n_coils, H, W), apply_mask, x, workspace, stream);
}

extern "C" int ipdm_sense_ssos_c64(const float* s, float* out, float* workspace, int B, int n_coils, int H, int W,
                                   void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && H > 0 && W > 0);
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(s && out);
  if (ipdm_kspace_large::large_ok(H, W)) {
    IPDM_REQUIRE(workspace);
    return ipdm_kspace_large::sense_adjoint(sense_problem<float>(s, nullptr, nullptr, 1, B, n_coils, H, W), 0, nullptr, out,
                                            reinterpret_cast<float2*>(workspace), ipdm_stream(stream));
  }
  if (!lds_fft_ok(H, W)) return IPDM_EUNSUPPORTED;
  size_t lds = lds_bytes(H, W);
  return fft_dispatch(fft_mixed(H, W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    int rc = ipdm_lds_optin(sense_adjoint_kernel<true, float, MIXED>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((sense_adjoint_kernel<true, float, MIXED>), dim3(B), dim3(FFT_THREADS), lds, ipdm_stream(stream),
                       reinterpret_cast<const float2*>(s), static_cast<const float*>(nullptr), 1, nullptr, 1, 0, out, B, n_coils,
                       H, W);
    return ipdm_launch_status();
  });
}

// x_re / x_im hold z (Langevin pending when lg.g_re) and receive the proximal
template <typename SensT>
static int sense_step(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb, float coef, float* work,
                      hipStream_t st) {
  float2* wk = reinterpret_cast<float2*>(work);
  if (ipdm_kspace_large::large_ok(pb.H, pb.W)) return ipdm_kspace_large::prox_step(x_re, x_im, lg, pb, coef, 0, wk, st);
  if (!lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  if (sense_coil_parallel()) return launch_sense_step_coils(x_re, x_im, lg, pb, coef, wk, st);
  const size_t lds = lds_bytes(pb.H, pb.W);
  return fft_dispatch(fft_mixed(pb.H, pb.W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    if (lg.g_re) {
      int rc = ipdm_lds_optin(ald_sense_step_kernel<true, SensT, MIXED>, lds);
      if (rc) return rc;
      hipLaunchKernelGGL((ald_sense_step_kernel<true, SensT, MIXED>), dim3(pb.B), dim3(FFT_THREADS), lds, st, x_re, x_im, lg, pb,
                         coef, wk);
    } else {
      int rc = ipdm_lds_optin(ald_sense_step_kernel<false, SensT, MIXED>, lds);
      if (rc) return rc;
      hipLaunchKernelGGL((ald_sense_step_kernel<false, SensT, MIXED>), dim3(pb.B), dim3(FFT_THREADS), lds, st, x_re, x_im, lg, pb,
                         coef, wk);
    }
    return ipdm_launch_status();
  });
}

template <typename SensT>
static int sense_l2prox_impl(const float* z_re, const float* z_im, const SenseProblem<SensT>& pb, float coef, float* out_re,
                             float* out_im, float* work, void* stream) {
  IPDM_REQUIRE(dims_ok(pb));
  if (pb.B == 0) return IPDM_OK;
  IPDM_REQUIRE(z_re && z_im && pb.y && pb.sens && pb.mask && out_re && out_im && work);
  if (!ipdm_kspace_large::large_ok(pb.H, pb.W) && !lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  hipStream_t st = ipdm_stream(stream);
  const int rc = copy_planes(out_re, out_im, z_re, z_im, (size_t)pb.B * pb.H * pb.W, st);
  return rc ? rc : sense_step(out_re, out_im, NO_LANGEVIN, pb, coef, work, st);
}

template <typename SensT>
static int ald_sense_step_impl(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb, float coef,
                               float* work, void* stream) {
  IPDM_REQUIRE(dims_ok(pb));
  if (pb.B == 0) return IPDM_OK;
  IPDM_REQUIRE(step_ptrs_ok(x_re, x_im, lg, pb) && pb.sens && work);
  return sense_step(x_re, x_im, lg, pb, coef, work, ipdm_stream(stream));
}

extern "C" int ipdm_sense_l2prox_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                     const uint8_t* mask, int mask_t, float coef, float* out_re, float* out_im,
                                     float* work, int B, int n_coils, int H, int W, void* stream) {
  return sense_l2prox_impl(z_re, z_im, sense_problem<float>(y, sens, mask, mask_t, B, n_coils, H, W), coef, out_re, out_im, work,
                           stream);
}

extern "C" int ipdm_sense_l2prox_csm_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                         const uint8_t* mask, int mask_t, float coef, float* out_re, float* out_im,
                                         float* work, int B, int n_coils, int H, int W, void* stream) {
  return sense_l2prox_impl(z_re, z_im, sense_problem<float2>(y, sens, mask, mask_t, B, n_coils, H, W), coef, out_re, out_im, work,
                           stream);
}

extern "C" int ipdm_ald_sense_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                       const float* noise_re, const float* noise_im, float step, float noise_scale,
                                       uint64_t seed, int64_t sample_offset, int64_t step_id,
                                       const ipdm_sched_t* dev_sched, const float* y, const float* sens, const uint8_t* mask,
                                       int mask_t, float coef, float* work, int B, int n_coils, int H, int W, void* stream) {
  return ald_sense_step_impl(x_re, x_im, {g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched},
                             sense_problem<float>(y, sens, mask, mask_t, B, n_coils, H, W), coef, work, stream);
}

extern "C" int ipdm_ald_sense_step_csm_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                           const float* noise_re, const float* noise_im, float step, float noise_scale,
                                           uint64_t seed, int64_t sample_offset, int64_t step_id,
                                           const ipdm_sched_t* dev_sched, const float* y, const float* sens,
                                           const uint8_t* mask, int mask_t, float coef, float* work, int B, int n_coils, int H,
                                           int W, void* stream) {
  return ald_sense_step_impl(x_re, x_im, {g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched},
                             sense_problem<float2>(y, sens, mask, mask_t, B, n_coils, H, W), coef, work, stream);
}

// ---- one map set per slice: sens [sens_sets][n_coils][H][W], image b reads set b % sens_sets (sens_at, kspace_fft.h) --------
// The entry points above are the sens_sets = 1 case of the same implementations.
extern "C" int ipdm_sense_forward_sets_c64(const float* x, const float* sens, int sens_complex, int sens_sets,
                                           const uint8_t* mask, int mask_t, float* y, int B, int n_coils, int H, int W,
                                           void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1);
  return sens_dispatch(sens_complex, nullptr, sens, mask, mask_t, B, n_coils, H, W, sens_sets,
                       [&](const auto& pb) { return sense_forward_impl(x, pb, y, stream); });
}

extern "C" int ipdm_sense_adjoint_sets_c64(const float* s, const float* sens, int sens_complex, int sens_sets,
                                           const uint8_t* mask, int mask_t, int apply_mask, float* x, float* workspace, int B,
                                           int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1);
  return sens_dispatch(sens_complex, s, sens, mask, mask_t, B, n_coils, H, W, sens_sets,
                       [&](const auto& pb) { return sense_adjoint_impl(pb, apply_mask, x, workspace, stream); });
}

extern "C" int ipdm_sense_l2prox_sets_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                          int sens_complex, int sens_sets, const uint8_t* mask, int mask_t, float coef,
                                          float* out_re, float* out_im, float* work, int B, int n_coils, int H, int W,
                                          void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1);
  return sens_dispatch(sens_complex, y, sens, mask, mask_t, B, n_coils, H, W, sens_sets, [&](const auto& pb) {
    return sense_l2prox_impl(z_re, z_im, pb, coef, out_re, out_im, work, stream);
  });
}

extern "C" int ipdm_ald_sense_step_sets_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                            const float* noise_re, const float* noise_im, float step, float noise_scale,
                                            uint64_t seed, int64_t sample_offset, int64_t step_id,
                                            const ipdm_sched_t* dev_sched, const float* y, const float* sens, int sens_complex,
                                            int sens_sets, const uint8_t* mask, int mask_t, float coef, float* work, int B,
                                            int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1);
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched};
  return sens_dispatch(sens_complex, y, sens, mask, mask_t, B, n_coils, H, W, sens_sets,
                       [&](const auto& pb) { return ald_sense_step_impl(x_re, x_im, lg, pb, coef, work, stream); });
}

// x_re / x_im hold z (Langevin pending when lg.g_re) and receive the single-coil operator's result
static int singlecoil_step(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<float>& pb, float coef, int mode,
                           float* workspace, hipStream_t st) {
  if (ipdm_kspace_large::large_ok(pb.H, pb.W)) {
    IPDM_REQUIRE(workspace);
    return ipdm_kspace_large::prox_step(x_re, x_im, lg, pb, coef, mode, reinterpret_cast<float2*>(workspace), st);
  }
  if (!lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  const size_t lds = lds_bytes(pb.H, pb.W);
  return fft_dispatch(fft_mixed(pb.H, pb.W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    if (lg.g_re) {
      int rc = ipdm_lds_optin(ald_singlecoil_step_kernel<true, MIXED>, lds);
      if (rc) return rc;
      hipLaunchKernelGGL((ald_singlecoil_step_kernel<true, MIXED>), dim3(pb.B), dim3(FFT_THREADS), lds, st, x_re, x_im, lg, pb, coef,
                         mode);
    } else {
      int rc = ipdm_lds_optin(ald_singlecoil_step_kernel<false, MIXED>, lds);
      if (rc) return rc;
      hipLaunchKernelGGL((ald_singlecoil_step_kernel<false, MIXED>), dim3(pb.B), dim3(FFT_THREADS), lds, st, x_re, x_im, lg, pb, coef,
                         mode);
    }
    return ipdm_launch_status();
  });
}

extern "C" int ipdm_singlecoil_prox_f32(const float* z_re, const float* z_im, const float* y, const uint8_t* mask,
                                        int mask_t, float coef, int mode, float* out_re, float* out_im, float* workspace,
                                        int B, int H, int W, void* stream) {
  const SenseProblem<float> pb = sense_problem<float>(y, nullptr, mask, mask_t, B, 1, H, W);
  IPDM_REQUIRE(dims_ok(pb) && mode >= 0 && mode <= 2);
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(z_re && z_im && y && mask && out_re && out_im);
  if (!ipdm_kspace_large::large_ok(H, W) && !lds_fft_ok(H, W)) return IPDM_EUNSUPPORTED;
  hipStream_t st = ipdm_stream(stream);
  const int rc = copy_planes(out_re, out_im, z_re, z_im, (size_t)B * H * W, st);
  return rc ? rc : singlecoil_step(out_re, out_im, NO_LANGEVIN, pb, coef, mode, workspace, st);
}

extern "C" int ipdm_ald_singlecoil_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                            const float* noise_re, const float* noise_im, float step, float noise_scale,
                                            uint64_t seed, int64_t sample_offset, int64_t step_id,
                                            const ipdm_sched_t* dev_sched, const float* y, const uint8_t* mask, int mask_t,
                                            float coef, int mode, float* workspace, int B, int H, int W, void* stream) {
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched};
  const SenseProblem<float> pb = sense_problem<float>(y, nullptr, mask, mask_t, B, 1, H, W);
  IPDM_REQUIRE(dims_ok(pb) && mode >= 0 && mode <= 2);
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(step_ptrs_ok(x_re, x_im, lg, pb));
  return singlecoil_step(x_re, x_im, lg, pb, coef, mode, workspace, ipdm_stream(stream));
}

// ---- one schedule record per sample (the predictor-corrector samplers: a step per sample, pc_coef.hip) ----------------------
// The `_sets_` / single-coil tails above with sched_stride records between consecutive samples: 0 is their shared record
// (same kernels, same bits), 1 lets sample b read dev_sched[b].
extern "C" int ipdm_pc_sense_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im, const float* noise_re,
                                      const float* noise_im, float step, float noise_scale, uint64_t seed,
                                      int64_t sample_offset, int64_t step_id, const ipdm_sched_t* dev_sched, int sched_stride,
                                      const float* y, const float* sens, int sens_complex, int sens_sets, const uint8_t* mask,
                                      int mask_t, float coef, float* work, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1 && sched_stride_ok(dev_sched, sched_stride));
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched, sched_stride};
  return sens_dispatch(sens_complex, y, sens, mask, mask_t, B, n_coils, H, W, sens_sets,
                       [&](const auto& pb) { return ald_sense_step_impl(x_re, x_im, lg, pb, coef, work, stream); });
}

extern "C" int ipdm_pc_singlecoil_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                           const float* noise_re, const float* noise_im, float step, float noise_scale,
                                           uint64_t seed, int64_t sample_offset, int64_t step_id,
                                           const ipdm_sched_t* dev_sched, int sched_stride, const float* y, const uint8_t* mask,
                                           int mask_t, float coef, int mode, float* workspace, int B, int H, int W,
                                           void* stream) {
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched, sched_stride};
  const SenseProblem<float> pb = sense_problem<float>(y, nullptr, mask, mask_t, B, 1, H, W);
  IPDM_REQUIRE(dims_ok(pb) && mode >= 0 && mode <= 2 && sched_stride_ok(dev_sched, sched_stride));
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(step_ptrs_ok(x_re, x_im, lg, pb));
  return singlecoil_step(x_re, x_im, lg, pb, coef, mode, workspace, ipdm_stream(stream));
}
