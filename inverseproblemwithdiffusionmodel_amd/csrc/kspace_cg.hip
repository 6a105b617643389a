// Exact multi-coil proximal of the SENSE sampler by conjugate gradients:
//     x = argmin 1/2 |x - z|^2 + a/2 |A x - y|^2      <=>      (I + a A^H A) x = z + a A^H y,      a = alpha / lamda
// N = I + a A^H A is Hermitian with every eigenvalue in [1, 1 + a] (RSS-normalised maps), so plain CG on complex vectors
// with real dot products Re<u, v> converges like ((sqrt(k) - 1) / (sqrt(k) + 1))^it, k <= 1 + a, and |x - x*| <= |b - N x|.
// Warm start x0 = z: r0 = -a A^H (A z - y), the quantity the one-step tail's coil kernel forms per coil.
//
// Launch sequence (fixed: it does not depend on convergence, so one captured hipGraph serves every noise level):
//     [A^H y, only when the caller does not pass it]
//     normal operator on z, coils in parallel   ->   init: x = z, r = p = r0, <r,r>, |b|^2, per-sample state
//     max_iter x ( normal operator on p, coils in parallel   ->   per-sample update )
// i.e. 2 + 2 max_iter launches for images held in LDS.  Every sample carries its own state {<r,r>, |b|^2, iterations,
// frozen} in device memory; a sample stops (is frozen: both kernels return at once for it, workgroup-uniformly) when
// |r| <= tol |b|, or when <r,r> or <p,Np> is not positive -- fp32 CG run past convergence underflows <r,r> and the
// textbook recursion then divides by zero.  Samples never interact: no batch-wide norm, no shared flag.
// Reductions: per-thread partial in element order, wave shuffles, then the 16 wave sums added in fixed order by every
// thread (no atomics: deterministic, and the result is uniform over the workgroup without a broadcast).
// Images beyond the LDS get the same solver by composition: the strip passes of kspace_large.hip apply the normal operator
// (coil sum included: one plane per sample instead of one per coil) and the update kernels grid-stride over the image.
#include "kspace_fft.h"

namespace {

using namespace ipdm_kspace;

struct CgState {
  float rr;        // <r, r>
  float bb;        // |b|^2, b = z + a A^H y
  int iters;       // CG iterations done
  int frozen;      // 1: x is final
};

struct CgWork {    // the caller's workspace, carved up (float2 units; ipdm_sense_cg_workspace_bytes)
  float2 *planes, *nout, *r, *p, *ahy;
  CgState* state;
};

static inline CgWork carve(float* work, int B, int n_coils, int H, int W) {
  const size_t img = (size_t)B * H * W;
  CgWork w;
  w.planes = reinterpret_cast<float2*>(work);      // [B][n_coils] coil planes (LDS path) / the strip passes' n_coils*B images
  w.nout = w.planes + img * n_coils;               // strip path: A^H(A v - y), coil sum done
  w.r = w.nout + img;
  w.p = w.r + img;
  w.ahy = w.p + img;
  w.state = reinterpret_cast<CgState*>(w.ahy + img);
  return w;
}

// every thread gets the workgroup's sum; red: FFT_THREADS / 64 floats of LDS, not in use by another reduction in flight
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = ipdm_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < FFT_THREADS / 64; ++w) s += red[w];
  return s;
}

// (((w_0 + w_1) + w_2) + ...) over the planes of one sample at element e, fixed order
__device__ __forceinline__ float2 plane_sum(const float2* __restrict__ pl, int n_planes, int HW, int e) {
  float2 a = pl[e];
  for (int c = 1; c < n_planes; ++c) {
    const float2 w = pl[(size_t)c * HW + e];
    a = make_float2(a.x + w.x, a.y + w.y);
  }
  return a;
}

// Normal operator, workgroup (coil, b): planes[b][coil] = conj(S_c) F^-1 M (F S_c v - y_c)
//   MODE 0: v = p[b], y = 0, skipped for a frozen sample;  MODE 1: v = z = x;  MODE 2: v = z = x + step*g + noise_scale*n
template <int MODE, typename SensT>
__global__ __launch_bounds__(FFT_THREADS) void cg_normal_coil_kernel(
    const float* x_re, const float* x_im, const float* __restrict__ g_re, const float* __restrict__ g_im,
    const float* __restrict__ n_re, const float* __restrict__ n_im, float step, float noise_scale, uint64_t seed,
    int64_t sample_offset, int64_t step_id, const ipdm_sched_t* __restrict__ sched, float a, const float2* __restrict__ p,
    const float2* __restrict__ y, const SensT* __restrict__ sens, const uint8_t* __restrict__ mask, int mask_t,
    const CgState* __restrict__ state, float2* planes, int B, int n_coils, int H, int W) {
  const int coil = blockIdx.x, b = blockIdx.y;
  if (sched) {
    step = sched->step;
    noise_scale = sched->noise_scale;
    a = sched->coef;
    step_id = sched->step_id;
  }
  if constexpr (MODE == 0) {
    if (state[b].frozen) return;
  } else {
    if (a == 0.f) return;                                      // the init pass then leaves x = z and freezes the sample
  }
  FFT_LDS_SETUP(H, W)
  const int HW = H * W;
  const float scale = rsqrtf((float)HW);
  const SensT* sm = sens + (size_t)coil * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    float2 v;
    if constexpr (MODE == 0) {
      v = p[(size_t)b * HW + e];
    } else {
      const float* xr = x_re + (size_t)b * HW;
      const float* xi = x_im + (size_t)b * HW;
      v = make_float2(xr[e], xi[e]);
      if constexpr (MODE == 2)
        langevin_value(xr, xi, g_re, g_im, n_re, n_im, step, noise_scale, seed, sample_offset, step_id, b, HW, e, v.x, v.y);
    }
    const int r = e / W, c = e - r * W;
    L.buf[e] = sens_mul(v, sign_rc(r, c), sm[e]);
  }
  __syncthreads();
  fft2_lds(L, H, W, false);
  // masked k-space value, re-modulated for the inverse transform: sign*(sign*scale*v - y) = scale*v - sign*y
  const float2* yc = MODE == 0 ? nullptr : y + ((size_t)coil * B + b) * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    const int r = e / W, c = e - r * W;
    const float2 v = L.buf[e];
    float2 res = make_float2(0.f, 0.f);
    if (mask_at(mask, mask_t, b, H, W, r, c)) {
      res = make_float2(v.x * scale, v.y * scale);
      if constexpr (MODE != 0) {
        const float sg = sign_rc(r, c);
        const float2 yy = yc[e];
        res = make_float2(res.x - sg * yy.x, res.y - sg * yy.y);
      }
    }
    L.buf[e] = res;
  }
  __syncthreads();
  fft2_lds(L, H, W, true);
  float2* wk = planes + ((size_t)b * n_coils + coil) * HW;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    const int r = e / W, c = e - r * W;
    wk[e] = sens_mul_conj(L.buf[e], sign_rc(r, c) * scale, sm[e]);
  }
}

// Init, one workgroup per sample: x = z (Langevin update applied here when LANGEVIN), r = p = -a * sum_c planes,
// <r,r>, |b|^2 = |z + a A^H y|^2, state.  a == 0: x = z exactly, frozen at 0 iterations.
template <bool LANGEVIN>
__global__ __launch_bounds__(FFT_THREADS) void cg_init_kernel(
    float* x_re, float* x_im, const float* __restrict__ g_re, const float* __restrict__ g_im,
    const float* __restrict__ n_re, const float* __restrict__ n_im, float step, float noise_scale, uint64_t seed,
    int64_t sample_offset, int64_t step_id, const ipdm_sched_t* __restrict__ sched, float a, float tol,
    const float2* __restrict__ planes, int n_planes, const float2* __restrict__ ahy, float2* r, float2* p, CgState* state,
    int32_t* iters_out, int HW) {
  __shared__ float red[2][FFT_THREADS / 64];
  if (sched) {
    step = sched->step;
    noise_scale = sched->noise_scale;
    a = sched->coef;
    step_id = sched->step_id;
  }
  const int b = blockIdx.x;
  float* xr = x_re + (size_t)b * HW;
  float* xi = x_im + (size_t)b * HW;
  const float2* pl = planes + (size_t)b * n_planes * HW;
  const float2* ab = ahy + (size_t)b * HW;
  float2* rb = r + (size_t)b * HW;
  float2* pb = p + (size_t)b * HW;
  float rr = 0.f, bb = 0.f;
  for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
    float zr = xr[e], zi = xi[e];
    if constexpr (LANGEVIN) {
      langevin_value(xr, xi, g_re, g_im, n_re, n_im, step, noise_scale, seed, sample_offset, step_id, b, HW, e, zr, zi);
      xr[e] = zr;
      xi[e] = zi;
    }
    if (a != 0.f) {
      const float2 w = plane_sum(pl, n_planes, HW, e);
      const float2 r0 = make_float2(-a * w.x, -a * w.y);
      rb[e] = r0;
      pb[e] = r0;
      rr += r0.x * r0.x + r0.y * r0.y;
      const float2 h = ab[e];
      const float br = zr + a * h.x, bi = zi + a * h.y;
      bb += br * br + bi * bi;
    }
  }
  rr = block_sum(rr, red[0]);
  bb = block_sum(bb, red[1]);
  if (threadIdx.x == 0) {
    CgState s;
    s.rr = rr;
    s.bb = bb;
    s.iters = 0;
    s.frozen = (a == 0.f || !(rr > 0.f) || rr <= tol * tol * bb) ? 1 : 0;
    state[b] = s;
    if (iters_out) iters_out[b] = 0;
  }
}

// One CG iteration of one sample, one workgroup:
//   q = p + a * sum_c planes ; alpha = <r,r> / <p,q> ; x += alpha p ; r -= alpha q ; beta = <r,r>' / <r,r> ; p = r + beta p
// REG: the image fits FFT_EPT elements per thread and q stays in registers; otherwise q is formed twice from the planes.
template <bool REG>
__global__ __launch_bounds__(FFT_THREADS) void cg_update_kernel(float* x_re, float* x_im, const ipdm_sched_t* __restrict__ sched,
                                                                float a, float tol, const float2* __restrict__ planes,
                                                                int n_planes, float2* r, float2* p, CgState* state,
                                                                int32_t* iters_out, int HW) {
  __shared__ float red[2][FFT_THREADS / 64];
  const int b = blockIdx.x;
  const CgState s = state[b];
  if (s.frozen) return;                                        // uniform over the workgroup
  if (sched) a = sched->coef;
  float* xr = x_re + (size_t)b * HW;
  float* xi = x_im + (size_t)b * HW;
  const float2* pl = planes + (size_t)b * n_planes * HW;
  float2* rb = r + (size_t)b * HW;
  float2* pb = p + (size_t)b * HW;
  float2 q[REG ? FFT_EPT : 1];
  float pq = 0.f;
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < FFT_EPT; ++k) {
      const int e = threadIdx.x + k * FFT_THREADS;
      if (e < HW) {
        const float2 pv = pb[e], w = plane_sum(pl, n_planes, HW, e);
        q[k] = make_float2(pv.x + a * w.x, pv.y + a * w.y);
        pq += pv.x * q[k].x + pv.y * q[k].y;
      }
    }
  } else {
    for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
      const float2 pv = pb[e], w = plane_sum(pl, n_planes, HW, e);
      pq += pv.x * (pv.x + a * w.x) + pv.y * (pv.y + a * w.y);
    }
  }
  pq = block_sum(pq, red[0]);
  if (!(pq > 0.f)) {                                           // also NaN: never divided by
    if (threadIdx.x == 0) state[b].frozen = 1;
    return;
  }
  const float alpha = s.rr / pq;
  float rr = 0.f;
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < FFT_EPT; ++k) {
      const int e = threadIdx.x + k * FFT_THREADS;
      if (e < HW) {
        const float2 pv = pb[e];
        float2 rv = rb[e];
        xr[e] = xr[e] + alpha * pv.x;
        xi[e] = xi[e] + alpha * pv.y;
        rv = make_float2(rv.x - alpha * q[k].x, rv.y - alpha * q[k].y);
        rb[e] = rv;
        rr += rv.x * rv.x + rv.y * rv.y;
      }
    }
  } else {
    for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {
      const float2 pv = pb[e], w = plane_sum(pl, n_planes, HW, e);
      float2 rv = rb[e];
      xr[e] = xr[e] + alpha * pv.x;
      xi[e] = xi[e] + alpha * pv.y;
      rv = make_float2(rv.x - alpha * (pv.x + a * w.x), rv.y - alpha * (pv.y + a * w.y));
      rb[e] = rv;
      rr += rv.x * rv.x + rv.y * rv.y;
    }
  }
  rr = block_sum(rr, red[1]);
  const bool dead = !(rr > 0.f);
  if (!dead) {
    const float beta = rr / s.rr;
    for (int e = threadIdx.x; e < HW; e += FFT_THREADS) {      // each thread re-reads the r it has just written
      const float2 rv = rb[e], pv = pb[e];
      pb[e] = make_float2(rv.x + beta * pv.x, rv.y + beta * pv.y);
    }
  }
  if (threadIdx.x == 0) {
    CgState o;
    o.rr = rr;
    o.bb = s.bb;
    o.iters = s.iters + 1;
    o.frozen = (dead || rr <= tol * tol * s.bb) ? 1 : 0;
    state[b] = o;
    if (iters_out) iters_out[b] = o.iters;
  }
}

struct Langevin {  // the fused tail's first phase; g_re NULL: none (the plain proximal)
  const float *g_re, *g_im, *n_re, *n_im;
  float step, noise_scale;
  uint64_t seed;
  int64_t sample_offset, step_id;
  const ipdm_sched_t* sched;
};

template <int MODE, typename SensT>
static int launch_normal_coils(float* x_re, float* x_im, const Langevin& lg, float a, const float2* p, const float2* y,
                               const SensT* sens, const uint8_t* mask, int mask_t, const CgWork& w, int B, int n_coils, int H,
                               int W, hipStream_t st) {
  const size_t lds = lds_bytes(H, W);
  const int rc = set_lds_limit(cg_normal_coil_kernel<MODE, SensT>, lds);
  if (rc) return rc;
  hipLaunchKernelGGL((cg_normal_coil_kernel<MODE, SensT>), dim3(n_coils, B), dim3(FFT_THREADS), lds, st, x_re, x_im, lg.g_re,
                     lg.g_im, lg.n_re, lg.n_im, lg.step, lg.noise_scale, lg.seed, (long long)lg.sample_offset,
                     (long long)lg.step_id, lg.sched, a, p, y, sens, mask, mask_t, w.state, w.planes, B, n_coils, H, W);
  return ipdm_launch_status();
}

// x_re / x_im hold x (Langevin pending when lg.g_re) and receive the solution
template <typename SensT>
static int cg_solve(float* x_re, float* x_im, const Langevin& lg, float a, const float2* y, const SensT* sens,
                    const uint8_t* mask, int mask_t, const float2* ahy, int max_iter, float tol, float* work,
                    int32_t* iters_out, int B, int n_coils, int H, int W, hipStream_t st) {
  const bool large = ipdm_kspace_large::large_ok(H, W);
  if (!large && !lds_fft_ok(H, W)) return IPDM_EUNSUPPORTED;
  if (B > 65535) return IPDM_EUNSUPPORTED;
  const CgWork w = carve(work, B, n_coils, H, W);
  const int HW = H * W;
  const bool lang = lg.g_re != nullptr;
  int rc;
  if (!ahy) {                                                  // A^H y = SENSE adjoint of the masked measurement
    if constexpr (sizeof(SensT) == sizeof(float2))
      rc = ipdm_sense_adjoint_csm_c64(reinterpret_cast<const float*>(y), reinterpret_cast<const float*>(sens), mask, mask_t, 1,
                                      reinterpret_cast<float*>(w.ahy), reinterpret_cast<float*>(w.planes), B, n_coils, H, W, st);
    else
      rc = ipdm_sense_adjoint_c64(reinterpret_cast<const float*>(y), reinterpret_cast<const float*>(sens), mask, mask_t, 1,
                                  reinterpret_cast<float*>(w.ahy), reinterpret_cast<float*>(w.planes), B, n_coils, H, W, st);
    if (rc) return rc;
    ahy = w.ahy;
  }
  const float2* planes = large ? w.nout : w.planes;
  const int n_planes = large ? 1 : n_coils;
  if (large) {
    if (lang) {
      rc = ipdm_kspace_large::langevin(x_re, x_im, lg.g_re, lg.g_im, lg.n_re, lg.n_im, lg.step, lg.noise_scale, lg.seed,
                                       lg.sample_offset, lg.step_id, lg.sched, B, H, W, st);
      if (rc) return rc;
    }
    rc = ipdm_kspace_large::normal_op<SensT>(nullptr, x_re, x_im, y, sens, mask, mask_t, w.nout, w.planes, B, n_coils, H, W, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cg_init_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, nullptr, nullptr, nullptr, nullptr,
                       0.f, 0.f, 0ull, 0ll, 0ll, lg.sched, a, tol, planes, n_planes, ahy, w.r, w.p, w.state, iters_out, HW);
  } else if (lang) {
    rc = launch_normal_coils<2>(x_re, x_im, lg, a, nullptr, y, sens, mask, mask_t, w, B, n_coils, H, W, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cg_init_kernel<true>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg.g_re, lg.g_im, lg.n_re, lg.n_im,
                       lg.step, lg.noise_scale, lg.seed, (long long)lg.sample_offset, (long long)lg.step_id, lg.sched, a, tol,
                       planes, n_planes, ahy, w.r, w.p, w.state, iters_out, HW);
  } else {
    rc = launch_normal_coils<1>(x_re, x_im, lg, a, nullptr, y, sens, mask, mask_t, w, B, n_coils, H, W, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cg_init_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, nullptr, nullptr, nullptr, nullptr,
                       0.f, 0.f, 0ull, 0ll, 0ll, lg.sched, a, tol, planes, n_planes, ahy, w.r, w.p, w.state, iters_out, HW);
  }
  rc = ipdm_launch_status();
  if (rc) return rc;
  for (int it = 0; it < max_iter; ++it) {
    if (large) {
      // (the strip passes have no per-sample exit: a frozen sample's planes are computed and ignored)
      rc = ipdm_kspace_large::normal_op<SensT>(w.p, nullptr, nullptr, nullptr, sens, mask, mask_t, w.nout, w.planes, B, n_coils,
                                               H, W, st);
      if (rc) return rc;
      hipLaunchKernelGGL(cg_update_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg.sched, a, tol, planes,
                         n_planes, w.r, w.p, w.state, iters_out, HW);
    } else {
      rc = launch_normal_coils<0>(x_re, x_im, lg, a, w.p, nullptr, sens, mask, mask_t, w, B, n_coils, H, W, st);
      if (rc) return rc;
      hipLaunchKernelGGL(cg_update_kernel<true>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg.sched, a, tol, planes,
                         n_planes, w.r, w.p, w.state, iters_out, HW);
    }
    rc = ipdm_launch_status();
    if (rc) return rc;
  }
  return IPDM_OK;
}

template <typename SensT>
static int cgprox_impl(const float* z_re, const float* z_im, const float* y, const SensT* sens, const uint8_t* mask, int mask_t,
                       float a, const float* ahy, int max_iter, float tol, float* out_re, float* out_im, float* work,
                       int32_t* iters_out, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && H > 0 && W > 0 && mask_t_ok(mask_t) && max_iter >= 1 && tol >= 0.f && tol < INFINITY);
  if (B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::large_ok(H, W) && !lds_fft_ok(H, W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(z_re && z_im && y && sens && mask && out_re && out_im && work);
  hipStream_t st = ipdm_stream(stream);
  const size_t bytes = (size_t)B * H * W * sizeof(float);
  if (out_re != z_re && hipMemcpyAsync(out_re, z_re, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
  if (out_im != z_im && hipMemcpyAsync(out_im, z_im, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
  const Langevin none{nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0ull, 0, 0, nullptr};
  return cg_solve(out_re, out_im, none, a, reinterpret_cast<const float2*>(y), sens, mask, mask_t,
                  reinterpret_cast<const float2*>(ahy), max_iter, tol, work, iters_out, B, n_coils, H, W, st);
}

template <typename SensT>
static int cg_step_impl(float* x_re, float* x_im, const float* g_re, const float* g_im, const float* noise_re,
                        const float* noise_im, float step, float noise_scale, uint64_t seed, int64_t sample_offset,
                        int64_t step_id, const ipdm_sched_t* dev_sched, const float* y, const SensT* sens, const uint8_t* mask,
                        int mask_t, float coef, float* work, const float* ahy, int max_iter, float tol, int32_t* iters_out, int B,
                        int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && H > 0 && W > 0 && mask_t_ok(mask_t) && max_iter >= 1 && tol >= 0.f && tol < INFINITY);
  if (B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::large_ok(H, W) && !lds_fft_ok(H, W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(x_re && x_im && g_re && g_im && y && sens && mask && work);
  IPDM_REQUIRE((noise_re == nullptr) == (noise_im == nullptr));
  const Langevin lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched};
  return cg_solve(x_re, x_im, lg, coef, reinterpret_cast<const float2*>(y), sens, mask, mask_t,
                  reinterpret_cast<const float2*>(ahy), max_iter, tol, work, iters_out, B, n_coils, H, W, ipdm_stream(stream));
}

}  // namespace

extern "C" int64_t ipdm_sense_cg_workspace_bytes(int B, int n_coils, int H, int W) {
  if (B <= 0 || n_coils <= 0 || H <= 0 || W <= 0) return 0;
  if (!lds_fft_ok(H, W) && !ipdm_kspace_large::large_ok(H, W)) return 0;
  return ((int64_t)n_coils + 4) * B * H * W * (int64_t)sizeof(float2) + (int64_t)B * (int64_t)sizeof(CgState);
}

extern "C" int ipdm_sense_cgprox_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                     const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter, float tol,
                                     float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils, int H,
                                     int W, void* stream) {
  return cgprox_impl(z_re, z_im, y, sens, mask, mask_t, a, ahy, max_iter, tol, out_re, out_im, work, iters_out, B, n_coils, H, W,
                     stream);
}

extern "C" int ipdm_sense_cgprox_csm_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                         const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter, float tol,
                                         float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils,
                                         int H, int W, void* stream) {
  return cgprox_impl(z_re, z_im, y, reinterpret_cast<const float2*>(sens), mask, mask_t, a, ahy, max_iter, tol, out_re, out_im,
                     work, iters_out, B, n_coils, H, W, stream);
}

extern "C" int ipdm_ald_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                          const float* noise_re, const float* noise_im, float step, float noise_scale,
                                          uint64_t seed, int64_t sample_offset, int64_t step_id, const ipdm_sched_t* dev_sched,
                                          const float* y, const float* sens, const uint8_t* mask, int mask_t, float coef,
                                          float* work, const float* ahy, int max_iter, float tol, int32_t* iters_out, int B,
                                          int n_coils, int H, int W, void* stream) {
  return cg_step_impl(x_re, x_im, g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched, y,
                      sens, mask, mask_t, coef, work, ahy, max_iter, tol, iters_out, B, n_coils, H, W, stream);
}

extern "C" int ipdm_ald_sense_cg_step_csm_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                              const float* noise_re, const float* noise_im, float step, float noise_scale,
                                              uint64_t seed, int64_t sample_offset, int64_t step_id,
                                              const ipdm_sched_t* dev_sched, const float* y, const float* sens,
                                              const uint8_t* mask, int mask_t, float coef, float* work, const float* ahy,
                                              int max_iter, float tol, int32_t* iters_out, int B, int n_coils, int H, int W,
                                              void* stream) {
  return cg_step_impl(x_re, x_im, g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched, y,
                      reinterpret_cast<const float2*>(sens), mask, mask_t, coef, work, ahy, max_iter, tol, iters_out, B, n_coils,
                      H, W, stream);
}
