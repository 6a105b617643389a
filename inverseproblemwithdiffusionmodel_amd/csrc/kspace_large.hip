// k-space operators for images that do not fit one CU's LDS (served sides, kspace_fft.h, above 16384 pixels, e.g. the 256x256 ACDC
// slices of the reference's real-data front end, helpers/load_data.py:274): the centred 2-D FFT runs as a ROW pass and a
// COLUMN pass over 64 KiB strips held in LDS, with the operator's elementwise work fused into the loads / stores of the
// passes and -- for the proximal operators -- the forward and the inverse column transform of a strip back to back in
// one kernel (the masked residual never leaves LDS; column strips without a sampled line skip both transforms, which at
// R = 40 is most of them).  The multi-coil proximal / Langevin step becomes four launches
//     Langevin update (planar, in place)  ->  rows forward, all coils  ->  columns forward + residual + columns inverse
//     ->  rows inverse + S_c-weighted coil sum (registers, coil order: deterministic) + update
// through a workspace of n_coils x B images (ipdm_sense_workspace_bytes).  Same arithmetic conventions as kspace.hip:
// fftshift / ifftshift folded into (-1)^(r+c) sign flips, orthonormal scale 1/sqrt(HW) applied once per 2-D transform.
#include "kspace_fft.h"

namespace ipdm_kspace_large {

using namespace ipdm_kspace;

constexpr int STRIP_ELEMS = 8192;                    // complex elements per workgroup strip (64 KiB)
constexpr int EPT = STRIP_ELEMS / FFT_THREADS;       // 8 elements per thread

bool large_ok(int H, int W) {
  return fft_side_ok(H) && fft_side_ok(W) && H <= FFT_MAX_SIDE && W <= FFT_MAX_SIDE && (int64_t)H * W > FFT_MAX_ELEMS;
}
// Lines per strip: the largest divisor of `lines` with at most STRIP_ELEMS elements, so every strip is full and the grid is
// lines / strip_lines exactly (no ragged last strip).  Powers of two: min(lines, STRIP_ELEMS / len), which divides.  Other
// served sides are multiples of 16 and len <= 2048, so a divisor >= 4 always fits (80x240: 20 rows of 34 that would fit;
// 48x512: 128 columns of 170).  The kernels and their launches both call this; MIXED = false (both sides powers of two)
// leaves the search out of the kernels that never need it.
template <bool MIXED = true>
__host__ __device__ __forceinline__ int strip_lines(int lines, int len) {
  int s = lines < STRIP_ELEMS / len ? lines : STRIP_ELEMS / len;
  if constexpr (MIXED)
    while (lines % s) --s;
  return s;
}
static inline size_t strip_lds_bytes(int n) { return ((size_t)STRIP_ELEMS + (size_t)n) * sizeof(float2); }

#define STRIP_LDS_SETUP(N)                                    \
  extern __shared__ __align__(16) unsigned char smem_raw[];  \
  FftLds L;                                                   \
  L.buf = reinterpret_cast<float2*>(smem_raw);               \
  L.tw = L.buf + STRIP_ELEMS;                                \
  L.twN = (N);                                               \
  fft_make_twiddles(L);

// ---- generic passes ---------------------------------------------------------------------------------------------
// F: load(b, coil, r, c) -> float2 and store(b, coil, r, c, v); rows [r0, r0 + RS) of image (b, coil)
// MIXED (all three strip kernels): a side with factors 3 or 5, kspace_fft.h; chosen at launch by fft_dispatch
template <class F, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void rows_kernel(F f0, int H, int W, int inverse) {
  STRIP_LDS_SETUP(W)
  const int RS = strip_lines<MIXED>(H, W);
  const int r0 = blockIdx.x * RS, b = blockIdx.y, coil = blockIdx.z;
  const F f = f0.for_image(b);
  const int n = RS * W;
  for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
    const int lr = e / W, c = e - lr * W;
    L.buf[e] = f.load(b, coil, r0 + lr, c);
  }
  __syncthreads();
  fft_lines<MIXED>(L, W, 1, W, RS, false, inverse != 0);
  for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
    const int lr = e / W, c = e - lr * W;
    f.store(b, coil, r0 + lr, c, L.buf[e]);
  }
}

// columns [c0, c0 + CS) of image (b, coil); LDS layout buf[r * CS + lc].  With TWO_WAY the strip is transformed forward,
// F::mid is applied in place, and it is transformed back (inverse) before the store; F::skip lets a strip whose mid()
// is identically zero bypass both transforms.
template <class F, bool TWO_WAY, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void cols_kernel(F f, int H, int W, int inverse) {
  STRIP_LDS_SETUP(H)
  const int CS = strip_lines<MIXED>(W, H);
  const int c0 = blockIdx.x * CS, b = blockIdx.y, coil = blockIdx.z;
  const int n = H * CS;
  if constexpr (TWO_WAY) {
    if (f.skip(b, c0, CS)) {                                   // uniform over the workgroup
      for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
        const int r = e / CS, lc = e - r * CS;
        f.store(b, coil, r, c0 + lc, make_float2(0.f, 0.f));
      }
      return;
    }
  }
  for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
    const int r = e / CS, lc = e - r * CS;
    L.buf[e] = f.load(b, coil, r, c0 + lc);
  }
  __syncthreads();
  fft_lines<MIXED>(L, H, CS, 1, CS, true, TWO_WAY ? false : inverse != 0);
  if constexpr (TWO_WAY) {
    for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
      const int r = e / CS, lc = e - r * CS;
      L.buf[e] = f.mid(b, coil, r, c0 + lc, L.buf[e]);
    }
    __syncthreads();
    fft_lines<MIXED>(L, H, CS, 1, CS, true, true);
  }
  for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
    const int r = e / CS, lc = e - r * CS;
    f.store(b, coil, r, c0 + lc, L.buf[e]);
  }
}

// ---- functors ---------------------------------------------------------------------------------------------------
struct ImgGeo {
  int B, H, W;
  __device__ __forceinline__ size_t at(int b, int r, int c) const { return ((size_t)b * H + r) * W + c; }
  __device__ __forceinline__ size_t at(int coil, int b, int r, int c) const {
    return (((size_t)coil * B + b) * H + r) * W + c;
  }
};

// rows of sign * S_c * x -> tmp[coil][b]      (x complex64 or planar; sens NULL: S = 1; SensT float or float2 maps)
template <typename SensT>
struct RowsFwd {
  ImgGeo g;
  const float2* x;                 // complex input, or NULL ->
  const float *xr, *xi;            // planar input
  const SensT* sens;               // [sens_sets][coils][H][W]; after for_image(): image b's set
  float2* dst;                     // [coil][b][H][W]
  int sens_sets, n_coils;
  // the functor of image b's workgroup: the map set is chosen here, once, not in load()
  __device__ __forceinline__ RowsFwd for_image(int b) const {
    RowsFwd f = *this;
    f.sens = sens_at(sens, sens_sets, b, (size_t)n_coils * g.H * g.W);
    return f;
  }
  __device__ __forceinline__ float2 load(int b, int coil, int r, int c) const {
    float2 v;
    if (x) v = x[g.at(b, r, c)];
    else v = make_float2(xr[g.at(b, r, c)], xi[g.at(b, r, c)]);
    const float s = sign_rc(r, c);
    if (sens) return sens_mul(v, s, sens[((size_t)coil * g.H + r) * g.W + c]);
    return make_float2(v.x * s, v.y * s);
  }
  __device__ __forceinline__ void store(int b, int coil, int r, int c, float2 v) const { dst[g.at(coil, b, r, c)] = v; }
};

// in-place columns on y[coil][b]: y = mask ? sign * scale * v : 0     (second half of SENSE.__call__ / i2k_complex)
struct ColsFwdMask {
  ImgGeo g;
  float2* y;
  const uint8_t* mask;             // NULL: no mask (plain centred transform)
  int mask_t;
  float scale;
  __device__ __forceinline__ float2 load(int b, int coil, int r, int c) const { return y[g.at(coil, b, r, c)]; }
  __device__ __forceinline__ void store(int b, int coil, int r, int c, float2 v) const {
    const float s = (!mask || mask_at(mask, mask_t, b, g.H, g.W, r, c)) ? sign_rc(r, c) * scale : 0.f;
    y[g.at(coil, b, r, c)] = make_float2(v.x * s, v.y * s);
  }
  __device__ __forceinline__ bool skip(int, int, int) const { return false; }
  __device__ __forceinline__ float2 mid(int, int, int, int, float2 v) const { return v; }
};

// columns of sign * (mask?) s[coil][b] -> tmp[coil][b]   (first half of the adjoint; inverse transform)
struct ColsInvFromS {
  ImgGeo g;
  const float2* s;
  float2* dst;
  const uint8_t* mask;
  int mask_t, apply_mask;
  __device__ __forceinline__ float2 load(int b, int coil, int r, int c) const {
    float sg = sign_rc(r, c);
    if (apply_mask && !mask_at(mask, mask_t, b, g.H, g.W, r, c)) sg = 0.f;
    const float2 v = s[g.at(coil, b, r, c)];
    return make_float2(v.x * sg, v.y * sg);
  }
  __device__ __forceinline__ void store(int b, int coil, int r, int c, float2 v) const { dst[g.at(coil, b, r, c)] = v; }
  __device__ __forceinline__ bool skip(int, int, int) const { return false; }
  __device__ __forceinline__ float2 mid(int, int, int, int, float2 v) const { return v; }
};

// in-place columns on tmp[coil][b]: forward, data-consistency operator in k-space, inverse.
//   mode < 0  SENSE / single-coil L2Penalty residual:  m ? (scale*v - sign*y) : 0
//   mode 1    SingleCoil closed form:                  (scale*v + coef*sign*y) / (1 + coef*m)
//   mode 2    projection:                              coef*sign*y + (m ? 1 - coef : 1) * scale*v
struct ColsProx {
  ImgGeo g;
  float2* tmp;
  const float2* y;                 // [coil][b][H][W]; NULL (mode <= 0 only): y = 0, the normal operator A^H A alone
  const uint8_t* mask;
  int mask_t, mode;
  float scale, coef_host;
  const ipdm_sched_t* sched;       // device schedule: overrides coef_host (modes 1, 2 use it in k-space)
  int sched_stride;                // sched_coef()
  __device__ __forceinline__ float2 load(int b, int coil, int r, int c) const { return tmp[g.at(coil, b, r, c)]; }
  __device__ __forceinline__ void store(int b, int coil, int r, int c, float2 v) const { tmp[g.at(coil, b, r, c)] = v; }
  // Called by every thread of the workgroup, before any divergence; the answer is the same in all of them.
  //   line mask: each thread scans the strip's cs column bytes (the same bytes, hence the same answer);
  //   2-D mask:  the strip is skippable only if none of its H x cs points is sampled -- the threads share the scan and
  //              __syncthreads_or makes the verdict uniform by construction (mask_t and mode are kernel arguments, so
  //              all threads take this branch together and all reach the barrier).
  __device__ __forceinline__ bool skip(int b, int c0, int cs) const {
    if (mode > 0) return false;
    if (mask_t > 0) {
      for (int c = c0; c < c0 + cs; ++c)
        if (mask_at(mask, mask_t, b, g.H, g.W, 0, c)) return false;
      return true;
    }
    int any = 0;
    for (int e = threadIdx.x; e < g.H * cs; e += FFT_THREADS) {
      const int r = e / cs, lc = e - r * cs;
      any |= mask_at(mask, mask_t, b, g.H, g.W, r, c0 + lc);
    }
    return !__syncthreads_or(any);
  }
  __device__ __forceinline__ float2 mid(int b, int coil, int r, int c, float2 v) const {
    v.x *= scale;
    v.y *= scale;
    const bool m = mask_at(mask, mask_t, b, g.H, g.W, r, c);
    const float2 yy = y ? y[g.at(coil, b, r, c)] : make_float2(0.f, 0.f);
    const float sg = sign_rc(r, c);
    if (mode <= 0) return masked_residual(m, v, sg, yy);
    const float coef = sched_coef(sched, sched_stride, b, coef_host);
    if (mode == 1) {
      const float inv = m ? 1.f / (1.f + coef) : 1.f;
      return make_float2((v.x + coef * sg * yy.x) * inv, (v.y + coef * sg * yy.y) * inv);
    }
    const float keep = m ? 1.f - coef : 1.f;
    return make_float2(coef * sg * yy.x + keep * v.x, coef * sg * yy.y + keep * v.y);
  }
};

// ---- rows inverse + coil sum + final operation ------------------------------------------------------------------------
enum { FIN_ADJOINT = 0, FIN_SSOS = 1, FIN_L2 = 2, FIN_REPLACE = 3 };

// tmp[coil][b] rows -> inverse row FFT -> acc += sign*scale*S_c * v  (coil order) ->
//   FIN_ADJOINT: out_c[b] = acc        FIN_SSOS: out_f[b] = sqrt(sum |scale*v|^2)
//   FIN_L2: x = x - coef*acc (planar, in place)      FIN_REPLACE: x = acc (planar)
template <int FIN, typename SensT, bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void rows_inv_accum_kernel(const float2* __restrict__ tmp,
                                                                     const SensT* __restrict__ sens_all, int sens_sets,
                                                                     float2* out_c, float* out_f, float* x_re, float* x_im,
                                                                     const ipdm_sched_t* __restrict__ sched, int sched_stride,
                                                                     float coef, int B, int n_coils, int H, int W) {
  STRIP_LDS_SETUP(W)
  const ImgGeo g{B, H, W};
  const int RS = strip_lines<MIXED>(H, W);
  const int r0 = blockIdx.x * RS, b = blockIdx.y;
  coef = sched_coef(sched, sched_stride, b, coef);
  const SensT* __restrict__ sens = sens_at(sens_all, sens_sets, b, (size_t)n_coils * H * W);
  const int n = RS * W;
  const float scale = rsqrtf((float)H * (float)W);
  float2 acc[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) acc[k] = make_float2(0.f, 0.f);
  for (int coil = 0; coil < n_coils; ++coil) {
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = threadIdx.x + k * FFT_THREADS;
      if (e < n) {
        const int lr = e / W, c = e - lr * W;
        L.buf[e] = tmp[g.at(coil, b, r0 + lr, c)];
      }
    }
    __syncthreads();
    fft_lines<MIXED>(L, W, 1, W, RS, false, true);
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = threadIdx.x + k * FFT_THREADS;
      if (e < n) {
        const int lr = e / W, c = e - lr * W;
        const float2 v = L.buf[e];
        if constexpr (FIN == FIN_SSOS) {
          acc[k].x += (v.x * v.x + v.y * v.y) * (scale * scale);
        } else {
          const float w = sign_rc(r0 + lr, c) * scale;
          const float2 t = sens ? sens_mul_conj(v, w, sens[((size_t)coil * H + r0) * W + e])   // (r0 + lr) * W + c = r0 * W + e
                                : make_float2(v.x * w, v.y * w);
          acc[k].x += t.x;
          acc[k].y += t.y;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = threadIdx.x + k * FFT_THREADS;
    if (e < n) {
      const int lr = e / W, c = e - lr * W;
      const size_t gi = g.at(b, r0 + lr, c);
      if constexpr (FIN == FIN_ADJOINT) out_c[gi] = acc[k];
      else if constexpr (FIN == FIN_SSOS) out_f[gi] = sqrtf(acc[k].x);
      else if constexpr (FIN == FIN_L2) {
        x_re[gi] = x_re[gi] - coef * acc[k].x;
        x_im[gi] = x_im[gi] - coef * acc[k].y;
      } else {
        x_re[gi] = acc[k].x;
        x_im[gi] = acc[k].y;
      }
    }
  }
}

// Langevin update of both planes in place, a quad of elements per thread: the update and the Philox keying are
// langevin_update / langevin_quad of kspace_fft.h, as in the fused 128x128 kernels
__global__ __launch_bounds__(256) void langevin_planes_kernel(float* x_re, float* x_im, LangevinArgs lg, int HW) {
  const float* __restrict__ g_re = lg.g_re;
  const float* __restrict__ g_im = lg.g_im;
  const float* __restrict__ n_re = lg.n_re;
  const float* __restrict__ n_im = lg.n_im;
  const int b = blockIdx.y;
  (void)sched_override(lg, b, 0.f);                            // the Langevin scalars only: no coefficient here
  const int quads = HW / 4;                                    // HW is a multiple of 4 (of 16, for every served size)
  // float4 access only where all the caller's planes sit on 16-byte boundaries; otherwise element by element (same
  // arithmetic, same Philox quad per four elements)
  const bool aligned = ((reinterpret_cast<uintptr_t>(x_re) | reinterpret_cast<uintptr_t>(x_im) | reinterpret_cast<uintptr_t>(g_re) |
                         reinterpret_cast<uintptr_t>(g_im) | reinterpret_cast<uintptr_t>(n_re) | reinterpret_cast<uintptr_t>(n_im)) & 15) == 0;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
    const size_t gi = (size_t)b * HW + 4 * (size_t)q;
    float nr[4], ni[4];
    if (!n_re) {
      langevin_quad(lg, b, 0, (uint32_t)q, nr);
      langevin_quad(lg, b, 1, (uint32_t)q, ni);
    }
    if (!aligned) {
      for (int j = 0; j < 4; ++j) {
        const float a = n_re ? n_re[gi + j] : nr[j], c = n_re ? n_im[gi + j] : ni[j];
        x_re[gi + j] = langevin_update(lg, x_re[gi + j], g_re[gi + j], a);
        x_im[gi + j] = langevin_update(lg, x_im[gi + j], g_im[gi + j], c);
      }
      continue;
    }
    if (n_re) {
      const float4 a = *reinterpret_cast<const float4*>(n_re + gi), c = *reinterpret_cast<const float4*>(n_im + gi);
      nr[0] = a.x; nr[1] = a.y; nr[2] = a.z; nr[3] = a.w;
      ni[0] = c.x; ni[1] = c.y; ni[2] = c.z; ni[3] = c.w;
    }
    float4 xr = *reinterpret_cast<float4*>(x_re + gi), xi = *reinterpret_cast<float4*>(x_im + gi);
    const float4 gr = *reinterpret_cast<const float4*>(g_re + gi), gim = *reinterpret_cast<const float4*>(g_im + gi);
    xr.x = langevin_update(lg, xr.x, gr.x, nr[0]); xr.y = langevin_update(lg, xr.y, gr.y, nr[1]);
    xr.z = langevin_update(lg, xr.z, gr.z, nr[2]); xr.w = langevin_update(lg, xr.w, gr.w, nr[3]);
    xi.x = langevin_update(lg, xi.x, gim.x, ni[0]); xi.y = langevin_update(lg, xi.y, gim.y, ni[1]);
    xi.z = langevin_update(lg, xi.z, gim.z, ni[2]); xi.w = langevin_update(lg, xi.w, gim.w, ni[3]);
    *reinterpret_cast<float4*>(x_re + gi) = xr;
    *reinterpret_cast<float4*>(x_im + gi) = xi;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
template <class F>
static int launch_rows(const F& f, int B, int coils, int H, int W, int inverse, hipStream_t s) {
  const size_t lds = strip_lds_bytes(W);
  const int RS = strip_lines(H, W);
  return fft_dispatch(fft_mixed(H, W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    int rc = ipdm_lds_optin(rows_kernel<F, MIXED>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((rows_kernel<F, MIXED>), dim3(H / RS, B, coils), dim3(FFT_THREADS), lds, s, f, H, W, inverse);
    return ipdm_launch_status();
  });
}

template <class F, bool TWO_WAY>
static int launch_cols(const F& f, int B, int coils, int H, int W, int inverse, hipStream_t s) {
  const size_t lds = strip_lds_bytes(H);
  const int CS = strip_lines(W, H);
  return fft_dispatch(fft_mixed(H, W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    int rc = ipdm_lds_optin((cols_kernel<F, TWO_WAY, MIXED>), lds);
    if (rc) return rc;
    hipLaunchKernelGGL((cols_kernel<F, TWO_WAY, MIXED>), dim3(W / CS, B, coils), dim3(FFT_THREADS), lds, s, f, H, W, inverse);
    return ipdm_launch_status();
  });
}

// tmp: pb.n_coils * pb.B column-transformed images; the coil sum weighted by pb.sens (NULL: unweighted)
template <int FIN, typename SensT>
static int launch_accum(const float2* tmp, const SenseProblem<SensT>& pb, float2* out_c, float* out_f, float* x_re, float* x_im,
                        const ipdm_sched_t* sched, int sched_stride, float coef, hipStream_t s) {
  const size_t lds = strip_lds_bytes(pb.W);
  const int RS = strip_lines(pb.H, pb.W);
  return fft_dispatch(fft_mixed(pb.H, pb.W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    int rc = ipdm_lds_optin((rows_inv_accum_kernel<FIN, SensT, MIXED>), lds);
    if (rc) return rc;
    hipLaunchKernelGGL((rows_inv_accum_kernel<FIN, SensT, MIXED>), dim3(pb.H / RS, pb.B), dim3(FFT_THREADS), lds, s, tmp, pb.sens,
                       pb.sens_sets, out_c, out_f, x_re, x_im, sched, sched_stride, coef, pb.B, pb.n_coils, pb.H, pb.W);
    return ipdm_launch_status();
  });
}

int64_t workspace_bytes(int B, int n_coils, int H, int W) {
  return large_ok(H, W) ? (int64_t)n_coils * B * H * W * (int64_t)sizeof(float2) : 0;
}

// centred orthonormal 2-D (i)FFT, out may alias in: rows into `out`, columns in place on `out`
int fft2c(const float2* in, float2* out, int batch, int H, int W, int inverse, hipStream_t s) {
  const ImgGeo g{batch, H, W};
  RowsFwd<float> rf{g, in, nullptr, nullptr, nullptr, out, 1, 1};
  int rc = launch_rows(rf, batch, 1, H, W, inverse, s);
  if (rc) return rc;
  ColsFwdMask cf{g, out, nullptr, 1, 1.f / sqrtf((float)H * (float)W)};
  return launch_cols<ColsFwdMask, false>(cf, batch, 1, H, W, inverse, s);
}

template <typename SensT>
int sense_forward(const float2* x, const SenseProblem<SensT>& pb, float2* y, hipStream_t s) {
  const int B = pb.B, n_coils = pb.n_coils, H = pb.H, W = pb.W;
  const ImgGeo g{B, H, W};
  RowsFwd<SensT> rf{g, x, nullptr, nullptr, pb.sens, y, pb.sens_sets, n_coils};
  int rc = launch_rows(rf, B, n_coils, H, W, 0, s);
  if (rc) return rc;
  ColsFwdMask cf{g, y, pb.mask, pb.mask_t, 1.f / sqrtf((float)H * (float)W)};
  return launch_cols<ColsFwdMask, false>(cf, B, n_coils, H, W, 0, s);
}
template int sense_forward(const float2*, const SenseProblem<float>&, float2*, hipStream_t);
template int sense_forward(const float2*, const SenseProblem<float2>&, float2*, hipStream_t);

template <typename SensT>
int sense_adjoint(const SenseProblem<SensT>& pb, int apply_mask, float2* x_out, float* ssos_out, float2* ws, hipStream_t s) {
  const ImgGeo g{pb.B, pb.H, pb.W};
  ColsInvFromS ci{g, pb.y, ws, pb.mask, pb.mask_t, apply_mask};
  int rc = launch_cols<ColsInvFromS, false>(ci, pb.B, pb.n_coils, pb.H, pb.W, 1, s);
  if (rc) return rc;
  if (ssos_out) {                                              // no maps in a sum of squares: one kernel for both SensT
    const SenseProblem<float> np{nullptr, nullptr, nullptr, 1, pb.B, pb.n_coils, pb.H, pb.W, 1};
    return launch_accum<FIN_SSOS>(ws, np, nullptr, ssos_out, nullptr, nullptr, nullptr, 0, 0.f, s);
  }
  return launch_accum<FIN_ADJOINT>(ws, pb, x_out, nullptr, nullptr, nullptr, nullptr, 0, 0.f, s);
}
template int sense_adjoint(const SenseProblem<float>&, int, float2*, float*, float2*, hipStream_t);
template int sense_adjoint(const SenseProblem<float2>&, int, float2*, float*, float2*, hipStream_t);

int langevin(float* x_re, float* x_im, const LangevinArgs& lg, int B, int H, int W, hipStream_t s) {
  int gx = (H * W / 4 + 255) / 256;
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(langevin_planes_kernel, dim3(gx, B), dim3(256), 0, s, x_re, x_im, lg, H * W);
  return ipdm_launch_status();
}

// forward rows, then columns forward + data-consistency operator + columns inverse, in place on ws[coil][b]
template <typename SensT>
static int rows_cols_prox(const float2* xc, const float* x_re, const float* x_im, const SenseProblem<SensT>& pb, int mode,
                          float coef, const ipdm_sched_t* sched, int sched_stride, float2* ws, hipStream_t s) {
  const ImgGeo g{pb.B, pb.H, pb.W};
  RowsFwd<SensT> rf{g, xc, x_re, x_im, pb.sens, ws, pb.sens_sets, pb.n_coils};
  int rc = launch_rows(rf, pb.B, pb.n_coils, pb.H, pb.W, 0, s);
  if (rc) return rc;
  ColsProx cp{g, ws, pb.y, pb.mask, pb.mask_t, mode, 1.f / sqrtf((float)pb.H * (float)pb.W), coef, sched,
              sched_stride};
  return launch_cols<ColsProx, true>(cp, pb.B, pb.n_coils, pb.H, pb.W, 0, s);
}

// out[b] = A^H (A v - y): the proximal chain's three passes with the coil sum stored instead of applied
template <typename SensT>
int normal_op(const float2* xc, const float* x_re, const float* x_im, const SenseProblem<SensT>& pb, float2* out, float2* ws,
              hipStream_t s) {
  int rc = rows_cols_prox(xc, x_re, x_im, pb, 0, 0.f, nullptr, 0, ws, s);
  if (rc) return rc;
  return launch_accum<FIN_ADJOINT>(ws, pb, out, nullptr, nullptr, nullptr, nullptr, 0, 0.f, s);
}
template int normal_op(const float2*, const float*, const float*, const SenseProblem<float>&, float2*, float2*, hipStream_t);
template int normal_op(const float2*, const float*, const float*, const SenseProblem<float2>&, float2*, float2*, hipStream_t);

template <typename SensT>
int prox_step(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb, float coef, int mode, float2* ws,
              hipStream_t s) {
  if (lg.g_re) {
    int rc = langevin(x_re, x_im, lg, pb.B, pb.H, pb.W, s);
    if (rc) return rc;
  }
  // (the 128x128 kernel returns early when coef == 0; here the schedule value lives on the device, so the chain always
  //  runs -- with coef == 0 it adds exactly zero for the L2 modes)
  int rc = rows_cols_prox(nullptr, x_re, x_im, pb, mode, coef, lg.sched, lg.sched_stride, ws, s);
  if (rc) return rc;
  if (mode <= 0)
    return launch_accum<FIN_L2>(ws, pb, nullptr, nullptr, x_re, x_im, lg.sched, lg.sched_stride, coef, s);
  return launch_accum<FIN_REPLACE>(ws, pb, nullptr, nullptr, x_re, x_im, nullptr, 0, 0.f, s);
}
template int prox_step(float*, float*, const LangevinArgs&, const SenseProblem<float>&, float, int, float2*, hipStream_t);
template int prox_step(float*, float*, const LangevinArgs&, const SenseProblem<float2>&, float, int, float2*, hipStream_t);

// ---- Toeplitz normal operator of a non-Cartesian trajectory ---------------------------------------------
// The H x W image sits at rows [H/2, H/2 + H), columns [W/2, W/2 + W) of a zero 2H x 2W grid that is never stored: the row
// passes run over the H rows that hold data (length 2W), the two-way column pass over all 2W columns (length 2H) with zeros
// loaded outside the H stored rows and only those rows stored.  ws[coil][b][H][2W].  Signs: the centring flips of the forward
// transform's output and of the inverse transform's input cancel around the real factor psf, so the column pass applies
// psf / (4HW) alone; the flips of the padded grid's index (r + H/2, c) remain at the two ends.
struct ToepGeo {
  int B, H, W;                     // image size
  __device__ __forceinline__ size_t ws_at(int coil, int b, int r, int c) const {     // c on the 2W grid
    return (((size_t)coil * B + b) * H + r) * (2 * (size_t)W) + c;
  }
};

// rows of pad(sign * S_c * v) -> ws[coil][b]      (v complex64 or planar; sens NULL: S = 1)
struct ToepRowsFwd {
  ToepGeo g;
  const float2* x;
  const float *xr, *xi;
  const float2* sens;
  float2* dst;
  __device__ __forceinline__ ToepRowsFwd for_image(int) const { return *this; }
  __device__ __forceinline__ float2 load(int b, int coil, int r, int c) const {
    const int c2 = c - g.W / 2;
    if ((unsigned)c2 >= (unsigned)g.W) return make_float2(0.f, 0.f);
    const size_t i = ((size_t)b * g.H + r) * g.W + c2;
    const float2 v = x ? x[i] : make_float2(xr[i], xi[i]);
    const float s = sign_rc(r + g.H / 2, c);
    if (sens) return sens_mul(v, s, sens[((size_t)coil * g.H + r) * g.W + c2]);
    return make_float2(v.x * s, v.y * s);
  }
  __device__ __forceinline__ void store(int b, int coil, int r, int c, float2 v) const { dst[g.ws_at(coil, b, r, c)] = v; }
};

// in-place columns on ws[coil][b], the 2H-long columns of the padded grid: forward, times psf / (4HW), inverse
struct ToepCols {
  ToepGeo g;
  float2* ws;
  const float* psf;                // [psf_sets][2H][2W]
  float scale2;                    // 1 / (4HW): the orthonormal pair's two factors
  int psf_sets;                    // image row b reads set b % psf_sets (b is the workgroup's: a scalar offset)
  __device__ __forceinline__ float2 load(int b, int coil, int r, int c) const {
    const int r2 = r - g.H / 2;
    return (unsigned)r2 < (unsigned)g.H ? ws[g.ws_at(coil, b, r2, c)] : make_float2(0.f, 0.f);
  }
  __device__ __forceinline__ void store(int b, int coil, int r, int c, float2 v) const {
    const int r2 = r - g.H / 2;
    if ((unsigned)r2 < (unsigned)g.H) ws[g.ws_at(coil, b, r2, c)] = v;
  }
  __device__ __forceinline__ bool skip(int, int, int) const { return false; }
  __device__ __forceinline__ float2 mid(int b, int, int r, int c, float2 v) const {
    const float* __restrict__ ps = psf + (size_t)(b % psf_sets) * (4 * (size_t)g.H * g.W);
    const float p = ps[(size_t)r * (2 * (size_t)g.W) + c] * scale2;
    return make_float2(v.x * p, v.y * p);
  }
};

// ws[coil][b] rows -> inverse row FFT (length 2W) -> crop -> acc += sign * conj(S_c) * v (registers, coil order) ->
// out[b] = acc - sub[b]    (sub NULL: nothing subtracted)
template <bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void toep_rows_inv_accum_kernel(const float2* __restrict__ ws,
                                                                          const float2* __restrict__ sens,
                                                                          const float2* __restrict__ sub, float2* out, int B,
                                                                          int n_coils, int H, int W) {
  const int W2 = 2 * W;
  STRIP_LDS_SETUP(W2)
  const ToepGeo g{B, H, W};
  const int RS = strip_lines<MIXED>(H, W2);
  const int r0 = blockIdx.x * RS, b = blockIdx.y;
  const int n = RS * W2;
  float2 acc[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) acc[k] = make_float2(0.f, 0.f);
  for (int coil = 0; coil < n_coils; ++coil) {
    const float2* __restrict__ src = ws + g.ws_at(coil, b, r0, 0);       // the strip's rows are contiguous
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = threadIdx.x + k * FFT_THREADS;
      if (e < n) L.buf[e] = src[e];
    }
    __syncthreads();
    fft_lines<MIXED>(L, W2, 1, W2, RS, false, true);
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = threadIdx.x + k * FFT_THREADS;
      if (e < n) {
        const int lr = e / W2, c = e - lr * W2, c2 = c - W / 2;
        if ((unsigned)c2 < (unsigned)W) {
          const float2 v = L.buf[e];
          const float sg = sign_rc(r0 + lr + H / 2, c);
          const float2 t = sens ? sens_mul_conj(v, sg, sens[((size_t)coil * H + r0 + lr) * W + c2])
                                : make_float2(v.x * sg, v.y * sg);
          acc[k].x += t.x;
          acc[k].y += t.y;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = threadIdx.x + k * FFT_THREADS;
    if (e < n) {
      const int lr = e / W2, c = e - lr * W2, c2 = c - W / 2;
      if ((unsigned)c2 < (unsigned)W) {
        const size_t gi = ((size_t)b * H + r0 + lr) * W + c2;
        float2 o = acc[k];
        if (sub) {
          const float2 h = sub[gi];
          o = make_float2(o.x - h.x, o.y - h.y);
        }
        out[gi] = o;
      }
    }
  }
}

bool toeplitz_ok(int H, int W) {
  if (H <= 0 || W <= 0 || H > FFT_MAX_SIDE / 2 || W > FFT_MAX_SIDE / 2) return false;
  return lds_fft_ok(2 * H, 2 * W) || large_ok(2 * H, 2 * W);
}

int toeplitz_normal(const float2* vc, const float* v_re, const float* v_im, const ToepProblem& tp, const float2* sub, float2* out,
                    float2* ws, hipStream_t s) {
  const int B = tp.B, n = tp.n_coils, H = tp.H, W = tp.W;
  const ToepGeo g{B, H, W};
  ToepRowsFwd rf{g, vc, v_re, v_im, tp.sens, ws};
  int rc = launch_rows(rf, B, n, H, 2 * W, 0, s);
  if (rc) return rc;
  ToepCols tc{g, ws, tp.psf, 0.25f / ((float)H * (float)W), tp.psf_sets};
  rc = launch_cols<ToepCols, true>(tc, B, n, 2 * H, 2 * W, 0, s);
  if (rc) return rc;
  const size_t lds = strip_lds_bytes(2 * W);
  const int RS = strip_lines(H, 2 * W);
  return fft_dispatch(fft_mixed(H, 2 * W), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    rc = ipdm_lds_optin(toep_rows_inv_accum_kernel<MIXED>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(toep_rows_inv_accum_kernel<MIXED>, dim3(H / RS, B), dim3(FFT_THREADS), lds, s, ws, tp.sens, sub, out, B, n,
                       H, W);
    return ipdm_launch_status();
  });
}

}  // namespace ipdm_kspace_large
