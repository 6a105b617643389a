// Per-sample Langevin-corrector step of the predictor-corrector samplers (score_sde's LangevinCorrector,
// sampling.py, with the two batch means replaced by the norms of each complex sample):
//     step_b = 2 alpha (snr |z_b| / |g_b|)^2,   noise_scale_b = sqrt(2 step_b)
// g the score, z the noise the following fused tail applies to sample b: injected planes, or the Philox normals that tail
// will draw (ipdm_philox_normal4 with the tail's keys; nothing is written to HBM but the records).
// Two launches, no atomics:
//   1. workgroup (k, b) of a (G, B) grid sums |g|^2 and |z|^2 over its quads of sample b: per thread in double, quads
//      q = k*256 + t, + G*256, ... in that order (whole quads: a Philox block is drawn once), then the xor butterfly
//      over the wave and the 4 wave sums in wave order -> partial[b][k]
//   2. one thread per sample adds partial[b][0..G) in index order, forms the coefficients in double, rounds once and
//      writes record b.
// G depends on sample_elems alone, so a sample's record does not depend on its batch.
#include "ipdm_common.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_MAX_BLOCKS = 64;                              // 256x256: 16384 quads, one per thread

inline int pc_blocks(int64_t sample_elems) {
  const int64_t quads = (sample_elems + 3) / 4;
  const int64_t g = (quads + PC_THREADS - 1) / PC_THREADS;
  return (int)(g > PC_MAX_BLOCKS ? PC_MAX_BLOCKS : g);
}

template <bool PHILOX>
__global__ __launch_bounds__(PC_THREADS) void pc_norms_kernel(const float* __restrict__ g_re, const float* __restrict__ g_im,
                                                              const float* __restrict__ n_re, const float* __restrict__ n_im,
                                                              uint64_t seed, int64_t sample_offset, int64_t step_id,
                                                              const ipdm_sched_t* __restrict__ sched, int64_t sample_elems,
                                                              double* __restrict__ partial) {
  __shared__ double red[2][PC_THREADS / 64];
  if (sched) step_id = sched->step_id;
  const int b = blockIdx.y;
  const int64_t quads = (sample_elems + 3) / 4;
  const int64_t off = (int64_t)b * sample_elems;
  // float4 loads where every plane read is on a 16-byte boundary at this sample; otherwise element by element
  const bool aligned = (((reinterpret_cast<uintptr_t>(g_re) | reinterpret_cast<uintptr_t>(g_im) |
                          (PHILOX ? uintptr_t(0) : (reinterpret_cast<uintptr_t>(n_re) | reinterpret_cast<uintptr_t>(n_im)))) & 15) == 0) &&
                       ((off & 3) == 0);
  double sg = 0.0, sz = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * PC_THREADS) {
    const int64_t base = off + q * 4;
    const int64_t left = sample_elems - q * 4;
    const int cnt = left < 4 ? (int)left : 4;
    float gr[4] = {0.f, 0.f, 0.f, 0.f}, gi[4] = {0.f, 0.f, 0.f, 0.f}, zr[4] = {0.f, 0.f, 0.f, 0.f}, zi[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PHILOX) {
      ipdm_philox_normal4(seed, sample_offset + b, step_id, 0, (uint32_t)q, zr);
      ipdm_philox_normal4(seed, sample_offset + b, step_id, 1, (uint32_t)q, zi);
    }
    if (aligned && cnt == 4) {
      const float4 a = *reinterpret_cast<const float4*>(g_re + base), c = *reinterpret_cast<const float4*>(g_im + base);
      gr[0] = a.x; gr[1] = a.y; gr[2] = a.z; gr[3] = a.w;
      gi[0] = c.x; gi[1] = c.y; gi[2] = c.z; gi[3] = c.w;
      if constexpr (!PHILOX) {
        const float4 u = *reinterpret_cast<const float4*>(n_re + base), v = *reinterpret_cast<const float4*>(n_im + base);
        zr[0] = u.x; zr[1] = u.y; zr[2] = u.z; zr[3] = u.w;
        zi[0] = v.x; zi[1] = v.y; zi[2] = v.z; zi[3] = v.w;
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        gr[j] = g_re[base + j];
        gi[j] = g_im[base + j];
        if constexpr (!PHILOX) {
          zr[j] = n_re[base + j];
          zi[j] = n_im[base + j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {                                           // elements past the sample's end carry no score and no noise
        sg += (double)gr[j] * (double)gr[j];
        sg += (double)gi[j] * (double)gi[j];
        sz += (double)zr[j] * (double)zr[j];
        sz += (double)zi[j] * (double)zi[j];
      }
    }
  }
  sg = ipdm_wave_sum(sg);
  sz = ipdm_wave_sum(sz);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sg;
    red[1][threadIdx.x >> 6] = sz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0][0], c = red[1][0];
#pragma unroll
    for (int w = 1; w < PC_THREADS / 64; ++w) {
      a += red[0][w];
      c += red[1][w];
    }
    double* o = partial + 2 * ((size_t)b * gridDim.x + blockIdx.x);
    o[0] = a;
    o[1] = c;
  }
}

__global__ __launch_bounds__(64) void pc_coef_kernel(const double* __restrict__ partial, int n_partial, double snr, double alpha,
                                                     const ipdm_sched_t* __restrict__ sched, float coef, float sigma,
                                                     int64_t step_id, ipdm_sched_t* __restrict__ out, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (sched) {
    coef = sched->coef;
    sigma = sched->sigma;
    step_id = sched->step_id;
  }
  double sg = 0.0, sz = 0.0;
  for (int k = 0; k < n_partial; ++k) {
    sg += partial[2 * ((size_t)b * n_partial + k)];
    sz += partial[2 * ((size_t)b * n_partial + k) + 1];
  }
  double step, scale;
  if (sg == 0.0) {                                             // no score: the sample only receives data consistency
    step = 0.0;
    scale = 0.0;
  } else if (!(sg < INFINITY) || !(sz < INFINITY)) {           // NaN or infinite norm: never a wrong finite value
    step = scale = __builtin_nan("");
  } else {
    const double r = snr * sqrt(sz) / sqrt(sg);
    step = 2.0 * alpha * r * r;
    scale = sqrt(2.0 * step);
  }
  ipdm_sched_t rec;
  rec.step = (float)step;
  rec.noise_scale = (float)scale;
  rec.coef = coef;
  rec.sigma = sigma;
  rec.step_id = step_id;
  rec.seg_scale = 0.f;
  rec.reserved = 0.f;
  out[b] = rec;
}

}  // namespace

extern "C" int64_t ipdm_pc_langevin_coef_workspace_bytes(int B) {
  return B <= 0 ? 0 : (int64_t)B * PC_MAX_BLOCKS * 2 * (int64_t)sizeof(double);
}

extern "C" int ipdm_pc_langevin_coef_f32(const float* g_re, const float* g_im, const float* noise_re, const float* noise_im,
                                         double snr, double alpha, uint64_t seed, int64_t sample_offset, int64_t step_id,
                                         const ipdm_sched_t* dev_sched, float coef, float sigma, ipdm_sched_t* sample_sched,
                                         double* work, int B, int64_t sample_elems, void* stream) {
  IPDM_REQUIRE(B >= 0 && B <= 65535 && sample_elems > 0 && sample_elems <= ((int64_t)1 << 31));
  IPDM_REQUIRE((noise_re == nullptr) == (noise_im == nullptr));
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(g_re && g_im && sample_sched && work);
  const int G = pc_blocks(sample_elems);
  hipStream_t st = ipdm_stream(stream);
  if (noise_re)
    hipLaunchKernelGGL(pc_norms_kernel<false>, dim3(G, B), dim3(PC_THREADS), 0, st, g_re, g_im, noise_re, noise_im, seed,
                       (long long)sample_offset, (long long)step_id, dev_sched, (long long)sample_elems, work);
  else
    hipLaunchKernelGGL(pc_norms_kernel<true>, dim3(G, B), dim3(PC_THREADS), 0, st, g_re, g_im, noise_re, noise_im, seed,
                       (long long)sample_offset, (long long)step_id, dev_sched, (long long)sample_elems, work);
  int rc = ipdm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(pc_coef_kernel, dim3((B + 63) / 64), dim3(64), 0, st, work, G, snr, alpha, dev_sched, coef, sigma,
                     (long long)step_id, sample_sched, B);
  return ipdm_launch_status();
}
