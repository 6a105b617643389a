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

// Init, one workgroup per sample: x = z (Langevin update applied here when LANGEVIN), r = p = -a * sum_c planes,
// <r,r>, |b|^2 = |z + a A^H y|^2, state.  a == 0: x = z exactly, frozen at 0 iterations.
template <bool LANGEVIN>
__global__ __launch_bounds__(FFT_THREADS) void cg_init_kernel(float* x_re, float* x_im, LangevinArgs lg, float a, float tol,
                                                              const float2* __restrict__ planes, int n_planes,
                                                              const float2* __restrict__ ahy, float2* r, float2* p,
                                                              CgState* state, int32_t* iters_out, int HW) {
  __shared__ float red[2][FFT_THREADS / 64];
  const int b = blockIdx.x;
  a = sched_override(lg, b, a);
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
      langevin_value(xr, xi, lg, b, HW, e, zr, zi);
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
                                                                int sched_stride, float a, float tol, const float2* __restrict__ planes,
                                                                int n_planes, float2* r, float2* p, CgState* state,
                                                                int32_t* iters_out, int HW) {
  __shared__ float red[2][FFT_THREADS / 64];
  const int b = blockIdx.x;
  const CgState s = state[b];
  if (s.frozen) return;                                        // uniform over the workgroup
  a = sched_coef(sched, sched_stride, b, a);
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

// x_re / x_im hold x (Langevin pending when lg.g_re) and receive the solution
template <typename SensT>
static int cg_solve(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb, float a, const float2* ahy,
                    int max_iter, float tol, float* work, int32_t* iters_out, hipStream_t st) {
  const int B = pb.B, H = pb.H, W = pb.W;
  const bool large = ipdm_kspace_large::large_ok(H, W);
  if (!large && !lds_fft_ok(H, W)) return IPDM_EUNSUPPORTED;
  if (B > 65535) return IPDM_EUNSUPPORTED;
  const CgWork w = carve(work, B, pb.n_coils, H, W);
  const int HW = H * W;
  const bool lang = lg.g_re != nullptr;
  int rc;
  if (!ahy) {                                                  // A^H y = SENSE adjoint of the masked measurement
    rc = ipdm_sense_adjoint_sets_c64(reinterpret_cast<const float*>(pb.y), reinterpret_cast<const float*>(pb.sens),
                                     sizeof(SensT) == sizeof(float2), pb.sens_sets, pb.mask, pb.mask_t, 1,
                                     reinterpret_cast<float*>(w.ahy), reinterpret_cast<float*>(w.planes), B, pb.n_coils, H, W,
                                     st);
    if (rc) return rc;
    ahy = w.ahy;
  }
  SenseProblem<SensT> no_y = pb;                               // the iterations apply A^H A alone
  no_y.y = nullptr;
  const float2* planes = large ? w.nout : w.planes;
  const int n_planes = large ? 1 : pb.n_coils;
  if (large) {
    if (lang) {
      rc = ipdm_kspace_large::langevin(x_re, x_im, lg, B, H, W, st);
      if (rc) return rc;
    }
    rc = ipdm_kspace_large::normal_op(nullptr, x_re, x_im, pb, w.nout, w.planes, st);
  } else {
    rc = launch_normal_coils(lang ? 2 : 1, x_re, x_im, lg, a, nullptr, nullptr, pb, w.planes, st);
  }
  if (rc) return rc;
  if (lang && !large)
    hipLaunchKernelGGL(cg_init_kernel<true>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg, a, tol, planes, n_planes, ahy, w.r,
                       w.p, w.state, iters_out, HW);
  else                                                         // no update, or (strips) already applied: only lg.sched is read
    hipLaunchKernelGGL(cg_init_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg, a, tol, planes, n_planes, ahy,
                       w.r, w.p, w.state, iters_out, HW);
  rc = ipdm_launch_status();
  if (rc) return rc;
  for (int it = 0; it < max_iter; ++it) {
    if (large) {
      // (the strip passes have no per-sample exit: a frozen sample's planes are computed and ignored)
      rc = ipdm_kspace_large::normal_op(w.p, nullptr, nullptr, no_y, w.nout, w.planes, st);
      if (rc) return rc;
      hipLaunchKernelGGL(cg_update_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg.sched, lg.sched_stride, a, tol,
                         planes, n_planes, w.r, w.p, w.state, iters_out, HW);
    } else {
      rc = launch_normal_coils(0, x_re, x_im, lg, a, w.p, w.state, no_y, w.planes, st);
      if (rc) return rc;
      hipLaunchKernelGGL(cg_update_kernel<true>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg.sched, lg.sched_stride, a, tol,
                         planes, n_planes, w.r, w.p, w.state, iters_out, HW);
    }
    rc = ipdm_launch_status();
    if (rc) return rc;
  }
  return IPDM_OK;
}

static inline bool cg_scalars_ok(int max_iter, float tol) { return max_iter >= 1 && tol >= 0.f && tol < INFINITY; }

template <typename SensT>
static int cgprox_impl(const float* z_re, const float* z_im, const SenseProblem<SensT>& pb, float a, const float* ahy, int max_iter,
                       float tol, float* out_re, float* out_im, float* work, int32_t* iters_out, void* stream) {
  IPDM_REQUIRE(dims_ok(pb) && cg_scalars_ok(max_iter, tol));
  if (pb.B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::large_ok(pb.H, pb.W) && !lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(z_re && z_im && pb.y && pb.sens && pb.mask && out_re && out_im && work);
  hipStream_t st = ipdm_stream(stream);
  const int rc = copy_planes(out_re, out_im, z_re, z_im, (size_t)pb.B * pb.H * pb.W, st);
  return rc ? rc : cg_solve(out_re, out_im, NO_LANGEVIN, pb, a, reinterpret_cast<const float2*>(ahy), max_iter, tol, work,
                            iters_out, st);
}

template <typename SensT>
static int cg_step_impl(float* x_re, float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb, float coef, float* work,
                        const float* ahy, int max_iter, float tol, int32_t* iters_out, void* stream) {
  IPDM_REQUIRE(dims_ok(pb) && cg_scalars_ok(max_iter, tol));
  if (pb.B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::large_ok(pb.H, pb.W) && !lds_fft_ok(pb.H, pb.W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(step_ptrs_ok(x_re, x_im, lg, pb) && pb.sens && work);
  return cg_solve(x_re, x_im, lg, pb, coef, reinterpret_cast<const float2*>(ahy), max_iter, tol, work, iters_out,
                  ipdm_stream(stream));
}

// ---- non-Cartesian SENSE: the same solver with the Toeplitz normal operator ----------------------------------
// N = I + a A^H W A, A^H W A applied by ipdm_kspace_large::toeplitz_normal; A^H W y is always the caller's (the hot path never
// applies A).  The strip form of cg_solve for every size: one plane per sample, the update kernels grid-stride.
//     [Langevin]  ->  T x - A^H y  ->  init  ->  max_iter x ( T p  ->  update )
struct NcCgWork {
  float2 *ws, *nout, *r, *p;
  CgState* state;
};
static inline NcCgWork nc_carve(float* work, int B, int n_coils, int H, int W) {
  const size_t img = (size_t)B * H * W;
  NcCgWork w;
  w.ws = reinterpret_cast<float2*>(work);          // the Toeplitz chain's n_coils * B * H * 2W values
  w.nout = w.ws + 2 * img * n_coils;
  w.r = w.nout + img;
  w.p = w.r + img;
  w.state = reinterpret_cast<CgState*>(w.p + img);
  return w;
}

static int nc_cg_solve(float* x_re, float* x_im, const LangevinArgs& lg, const ToepProblem& tp, float a, const float2* ahy,
                       int max_iter, float tol, float* work, int32_t* iters_out, hipStream_t st) {
  const int B = tp.B, H = tp.H, W = tp.W, HW = H * W;
  const NcCgWork w = nc_carve(work, B, tp.n_coils, H, W);
  int rc;
  if (lg.g_re) {
    rc = ipdm_kspace_large::langevin(x_re, x_im, lg, B, H, W, st);
    if (rc) return rc;
  }
  rc = ipdm_kspace_large::toeplitz_normal(nullptr, x_re, x_im, tp, ahy, w.nout, w.ws, st);
  if (rc) return rc;
  hipLaunchKernelGGL(cg_init_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg, a, tol, w.nout, 1, ahy, w.r, w.p,
                     w.state, iters_out, HW);
  rc = ipdm_launch_status();
  if (rc) return rc;
  for (int it = 0; it < max_iter; ++it) {
    rc = ipdm_kspace_large::toeplitz_normal(w.p, nullptr, nullptr, tp, nullptr, w.nout, w.ws, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cg_update_kernel<false>, dim3(B), dim3(FFT_THREADS), 0, st, x_re, x_im, lg.sched, lg.sched_stride, a, tol,
                       w.nout, 1, w.r, w.p, w.state, iters_out, HW);
    rc = ipdm_launch_status();
    if (rc) return rc;
  }
  return IPDM_OK;
}

static inline bool nc_cg_dims_ok(int B, int n_coils, int H, int W) { return B >= 0 && n_coils > 0 && H > 0 && W > 0; }
static inline bool nc_cg_served(int B, int n_coils, int H, int W) {
  return ipdm_kspace_large::toeplitz_ok(H, W) && B <= 65535 && n_coils <= 65535;
}

}  // namespace

extern "C" int64_t ipdm_nc_sense_cg_workspace_bytes(int B, int n_coils, int H, int W) {
  if (B <= 0 || n_coils <= 0 || !ipdm_kspace_large::toeplitz_ok(H, W)) return 0;
  return (2 * (int64_t)n_coils + 3) * B * H * W * (int64_t)sizeof(float2) + (int64_t)B * (int64_t)sizeof(CgState);
}

// psf [psf_sets][2H][2W]: image row b solves with set b % psf_sets (frames); the launch sequence is the same
extern "C" int ipdm_nc_sense_cgprox_sets_f32(const float* z_re, const float* z_im, const float* sens, const float* psf,
                                             int psf_sets, float a, const float* ahy, int max_iter, float tol, float* out_re,
                                             float* out_im, float* work, int32_t* iters_out, int B, int n_coils, int H, int W,
                                             void* stream) {
  IPDM_REQUIRE(nc_cg_dims_ok(B, n_coils, H, W) && cg_scalars_ok(max_iter, tol) && (sens || n_coils == 1) && psf_sets >= 1 &&
               B % psf_sets == 0);
  if (B == 0) return IPDM_OK;
  if (!nc_cg_served(B, n_coils, H, W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(z_re && z_im && psf && ahy && out_re && out_im && work);
  hipStream_t st = ipdm_stream(stream);
  const int rc = copy_planes(out_re, out_im, z_re, z_im, (size_t)B * H * W, st);
  const ToepProblem tp{reinterpret_cast<const float2*>(sens), psf, B, n_coils, H, W, psf_sets};
  return rc ? rc : nc_cg_solve(out_re, out_im, NO_LANGEVIN, tp, a, reinterpret_cast<const float2*>(ahy), max_iter, tol, work,
                               iters_out, st);
}

extern "C" int ipdm_nc_sense_cgprox_f32(const float* z_re, const float* z_im, const float* sens, const float* psf, float a,
                                        const float* ahy, int max_iter, float tol, float* out_re, float* out_im, float* work,
                                        int32_t* iters_out, int B, int n_coils, int H, int W, void* stream) {
  return ipdm_nc_sense_cgprox_sets_f32(z_re, z_im, sens, psf, 1, a, ahy, max_iter, tol, out_re, out_im, work, iters_out, B,
                                       n_coils, H, W, stream);
}

extern "C" int ipdm_ald_nc_sense_cg_step_sets_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                                  const float* noise_re, const float* noise_im, float step, float noise_scale,
                                                  uint64_t seed, int64_t sample_offset, int64_t step_id,
                                                  const ipdm_sched_t* dev_sched, int sched_stride, const float* sens,
                                                  const float* psf, int psf_sets, float coef, float* work, const float* ahy,
                                                  int max_iter, float tol, int32_t* iters_out, int B, int n_coils, int H, int W,
                                                  void* stream) {
  IPDM_REQUIRE(nc_cg_dims_ok(B, n_coils, H, W) && cg_scalars_ok(max_iter, tol) && (sens || n_coils == 1) &&
               sched_stride_ok(dev_sched, sched_stride) && psf_sets >= 1 && B % psf_sets == 0);
  if (B == 0) return IPDM_OK;
  if (!nc_cg_served(B, n_coils, H, W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(x_re && x_im && g_re && g_im && (noise_re == nullptr) == (noise_im == nullptr) && psf && ahy && work);
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched, sched_stride};
  const ToepProblem tp{reinterpret_cast<const float2*>(sens), psf, B, n_coils, H, W, psf_sets};
  return nc_cg_solve(x_re, x_im, lg, tp, coef, reinterpret_cast<const float2*>(ahy), max_iter, tol, work, iters_out,
                     ipdm_stream(stream));
}

extern "C" int ipdm_ald_nc_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                             const float* noise_re, const float* noise_im, float step, float noise_scale,
                                             uint64_t seed, int64_t sample_offset, int64_t step_id,
                                             const ipdm_sched_t* dev_sched, int sched_stride, const float* sens,
                                             const float* psf, float coef, float* work, const float* ahy, int max_iter, float tol,
                                             int32_t* iters_out, int B, int n_coils, int H, int W, void* stream) {
  return ipdm_ald_nc_sense_cg_step_sets_f32(x_re, x_im, g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset,
                                            step_id, dev_sched, sched_stride, sens, psf, 1, coef, work, ahy, max_iter, tol,
                                            iters_out, B, n_coils, H, W, stream);
}

extern "C" int64_t ipdm_sense_cg_workspace_bytes(int B, int n_coils, int H, int W) {
  if (B <= 0 || n_coils <= 0 || H <= 0 || W <= 0) return 0;
  if (!lds_fft_ok(H, W) && !ipdm_kspace_large::large_ok(H, W)) return 0;
  return ((int64_t)n_coils + 4) * B * H * W * (int64_t)sizeof(float2) + (int64_t)B * (int64_t)sizeof(CgState);
}

extern "C" int ipdm_sense_cgprox_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                     const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter, float tol,
                                     float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils, int H,
                                     int W, void* stream) {
  return cgprox_impl(z_re, z_im, sense_problem<float>(y, sens, mask, mask_t, B, n_coils, H, W), a, ahy, max_iter, tol, out_re,
                     out_im, work, iters_out, stream);
}

extern "C" int ipdm_sense_cgprox_csm_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                         const uint8_t* mask, int mask_t, float a, const float* ahy, int max_iter, float tol,
                                         float* out_re, float* out_im, float* work, int32_t* iters_out, int B, int n_coils,
                                         int H, int W, void* stream) {
  return cgprox_impl(z_re, z_im, sense_problem<float2>(y, sens, mask, mask_t, B, n_coils, H, W), a, ahy, max_iter, tol, out_re,
                     out_im, work, iters_out, stream);
}

extern "C" int ipdm_ald_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                          const float* noise_re, const float* noise_im, float step, float noise_scale,
                                          uint64_t seed, int64_t sample_offset, int64_t step_id, const ipdm_sched_t* dev_sched,
                                          const float* y, const float* sens, const uint8_t* mask, int mask_t, float coef,
                                          float* work, const float* ahy, int max_iter, float tol, int32_t* iters_out, int B,
                                          int n_coils, int H, int W, void* stream) {
  return cg_step_impl(x_re, x_im, {g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched},
                      sense_problem<float>(y, sens, mask, mask_t, B, n_coils, H, W), coef, work, ahy, max_iter, tol, iters_out,
                      stream);
}

extern "C" int ipdm_ald_sense_cg_step_csm_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                              const float* noise_re, const float* noise_im, float step, float noise_scale,
                                              uint64_t seed, int64_t sample_offset, int64_t step_id,
                                              const ipdm_sched_t* dev_sched, const float* y, const float* sens,
                                              const uint8_t* mask, int mask_t, float coef, float* work, const float* ahy,
                                              int max_iter, float tol, int32_t* iters_out, int B, int n_coils, int H, int W,
                                              void* stream) {
  return cg_step_impl(x_re, x_im, {g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched},
                      sense_problem<float2>(y, sens, mask, mask_t, B, n_coils, H, W), coef, work, ahy, max_iter, tol, iters_out,
                      stream);
}

// one map set per slice (sens_at, kspace_fft.h); the entry points above are the sens_sets = 1 case
extern "C" int ipdm_sense_cgprox_sets_f32(const float* z_re, const float* z_im, const float* y, const float* sens,
                                          int sens_complex, int sens_sets, const uint8_t* mask, int mask_t, float a,
                                          const float* ahy, int max_iter, float tol, float* out_re, float* out_im, float* work,
                                          int32_t* iters_out, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1);
  return sens_dispatch(sens_complex, y, sens, mask, mask_t, B, n_coils, H, W, sens_sets, [&](const auto& pb) {
    return cgprox_impl(z_re, z_im, pb, a, ahy, max_iter, tol, out_re, out_im, work, iters_out, stream);
  });
}

extern "C" int ipdm_ald_sense_cg_step_sets_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                               const float* noise_re, const float* noise_im, float step, float noise_scale,
                                               uint64_t seed, int64_t sample_offset, int64_t step_id,
                                               const ipdm_sched_t* dev_sched, const float* y, const float* sens,
                                               int sens_complex, int sens_sets, const uint8_t* mask, int mask_t, float coef,
                                               float* work, const float* ahy, int max_iter, float tol, int32_t* iters_out,
                                               int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1);
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched};
  return sens_dispatch(sens_complex, y, sens, mask, mask_t, B, n_coils, H, W, sens_sets, [&](const auto& pb) {
    return cg_step_impl(x_re, x_im, lg, pb, coef, work, ahy, max_iter, tol, iters_out, stream);
  });
}

// one schedule record per sample: sched_stride as ipdm_pc_sense_step_f32 (kspace.hip); 0 is the entry point above
extern "C" int ipdm_pc_sense_cg_step_f32(float* x_re, float* x_im, const float* g_re, const float* g_im,
                                         const float* noise_re, const float* noise_im, float step, float noise_scale,
                                         uint64_t seed, int64_t sample_offset, int64_t step_id, const ipdm_sched_t* dev_sched,
                                         int sched_stride, const float* y, const float* sens, int sens_complex, int sens_sets,
                                         const uint8_t* mask, int mask_t, float coef, float* work, const float* ahy,
                                         int max_iter, float tol, int32_t* iters_out, int B, int n_coils, int H, int W,
                                         void* stream) {
  IPDM_REQUIRE(sens && sens_sets >= 1 && sched_stride_ok(dev_sched, sched_stride));
  const LangevinArgs lg{g_re, g_im, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id, dev_sched, sched_stride};
  return sens_dispatch(sens_complex, y, sens, mask, mask_t, B, n_coils, H, W, sens_sets, [&](const auto& pb) {
    return cg_step_impl(x_re, x_im, lg, pb, coef, work, ahy, max_iter, tol, iters_out, stream);
  });
}
