// Non-Cartesian self-calibration: the one kernel pair the calibration chain lacked -- the weighted Gram
// matrix of the samples themselves, for coil compression before the calibration images exist.
//     G_b[i][j] = sum_m w_m y[i][b][m] conj(y[j][b][m]),   y [n][B][M] (the layout of the ndft_* operands), w [M] >= 0 (NULL: 1)
// The sample axis is cut into chunks of NCG_CHUNK samples.  nc_gram_partial_kernel, workgroup (chunk, pair tile, b), stages its
// chunk NCG_STAGE samples at a time for all coils through LDS and writes the double partial sums of its 256 pairs of the upper
// triangle to work[b][chunk][pair]; nc_gram_reduce_kernel adds the chunks in chunk order, rounds once to float32 and
// mirrors.  Products and sums are double, every order is fixed by (n, M) alone, no atomics: G is exactly Hermitian with a
// real diagonal, an image's result does not depend on its batch, and two runs give the same bits.  y is read only where
// w_m > 0 (the time average reads sampled positions only, in the same way): whatever lies at a zero-weight sample, a NaN
// included, never reaches G.
#include "launch.h"

namespace {

constexpr int NCG_MAX_COILS = 64;               // the range of ipdm_coilcomp_supported
constexpr int NCG_THREADS = 256;
constexpr int NCG_CHUNK = 1024;                 // samples per workgroup: the unit of the partial sums
constexpr int NCG_STAGE = 32;                   // samples staged per pass ([coil][NCG_STAGE + 1] float2: 16.5 KiB at 64 coils)
static_assert(NCG_CHUNK % NCG_STAGE == 0, "a chunk is a whole number of stages");

static inline int ncg_chunks(int M) { return (M - 1) / NCG_CHUNK + 1; }
static inline int ncg_pairs(int n) { return n * (n + 1) / 2; }

// pair t of the upper triangle, row by row: (0,0) (0,1) ... (0,n-1) (1,1) ...
__device__ __forceinline__ void ncg_pair(int t, int n, int& i, int& j) {
  i = 0;
  int rem = t;
  while (rem >= n - i) {
    rem -= n - i;
    ++i;
  }
  j = i + rem;
}

__global__ __launch_bounds__(NCG_THREADS) void nc_gram_partial_kernel(const float2* __restrict__ y, const float* __restrict__ wgt,
                                                                      double2* __restrict__ work, int B, int n, int M) {
  __shared__ float2 smp[NCG_MAX_COILS * (NCG_STAGE + 1)];
  __shared__ float wsm[NCG_STAGE];
  const int chunk = blockIdx.x, b = blockIdx.z;
  const int npairs = n * (n + 1) / 2;
  const int t = blockIdx.y * NCG_THREADS + threadIdx.x;
  int i = 0, j = 0;
  if (t < npairs) ncg_pair(t, n, i, j);
  const int m_lo = chunk * NCG_CHUNK;
  const int m_hi = M - m_lo < NCG_CHUNK ? M : m_lo + NCG_CHUNK;  // (no overflow: m_lo + NCG_CHUNK only when it is <= M)
  double acc_re = 0.0, acc_im = 0.0;
  for (int m0 = m_lo; m0 < m_hi; m0 += NCG_STAGE) {
    for (int idx = threadIdx.x; idx < n * NCG_STAGE; idx += NCG_THREADS) {
      const int c = idx / NCG_STAGE, s = idx - c * NCG_STAGE;
      const int m = m0 + s;
      float w = 0.f;
      if (m < m_hi) w = wgt ? wgt[m] : 1.f;
      float2 v = make_float2(0.f, 0.f);
      if (w > 0.f) v = y[((size_t)c * B + b) * M + m];           // the only read of y: a zero-weight sample is never touched
      else w = 0.f;                                              // (a negative or NaN weight counts as zero)
      smp[c * (NCG_STAGE + 1) + s] = v;
      if (c == 0) wsm[s] = w;
    }
    __syncthreads();
    if (t < npairs) {
      const float2* pi = smp + i * (NCG_STAGE + 1);
      const float2* pj = smp + j * (NCG_STAGE + 1);
#pragma unroll 4
      for (int s = 0; s < NCG_STAGE; ++s) {                      // samples past the chunk are zeros of weight zero
        const float2 a = pi[s], c = pj[s];
        const double w = (double)wsm[s];
        acc_re += w * ((double)a.x * (double)c.x + (double)a.y * (double)c.y);
        acc_im += w * ((double)a.y * (double)c.x - (double)a.x * (double)c.y);
      }
    }
    __syncthreads();
  }
  if (t < npairs) work[((size_t)b * gridDim.x + chunk) * npairs + t] = make_double2(acc_re, acc_im);
}

// workgroup (pair tile, b): the chunks in chunk order, one rounding, the mirror image
__global__ __launch_bounds__(NCG_THREADS) void nc_gram_reduce_kernel(const double2* __restrict__ work, float2* __restrict__ gram,
                                                                     int n, int chunks) {
  const int b = blockIdx.y;
  const int npairs = n * (n + 1) / 2;
  const int t = blockIdx.x * NCG_THREADS + threadIdx.x;
  if (t >= npairs) return;
  int i, j;
  ncg_pair(t, n, i, j);
  double re = 0.0, im = 0.0;
  for (int k = 0; k < chunks; ++k) {
    const double2 p = work[((size_t)b * chunks + k) * npairs + t];
    re += p.x;
    im += p.y;
  }
  float2* g = gram + (size_t)b * n * n;
  const float fr = (float)re, fi = i == j ? 0.f : (float)im;
  g[i * n + j] = make_float2(fr, fi);
  if (i != j) g[j * n + i] = make_float2(fr, -fi);
}

}  // namespace

// double2 partials [B][chunks][pairs of the upper triangle]
extern "C" size_t ipdm_nc_coil_gram_workspace_bytes(int B, int n_coils, int M) {
  if (B <= 0 || n_coils < 1 || n_coils > NCG_MAX_COILS || M < 1 || B > 65535) return 0;
  return (size_t)B * ncg_chunks(M) * ncg_pairs(n_coils) * sizeof(double2);
}

extern "C" int ipdm_nc_coil_gram_c64(const float* y, const float* weights, float* gram, float* work, int B, int n_coils, int M,
                                     void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && M >= 1);
  if (n_coils > NCG_MAX_COILS || B > 65535) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && gram && work);
  hipStream_t st = ipdm_stream(stream);
  const int chunks = ncg_chunks(M), tiles = (ncg_pairs(n_coils) + NCG_THREADS - 1) / NCG_THREADS;
  double2* part = reinterpret_cast<double2*>(work);
  hipLaunchKernelGGL(nc_gram_partial_kernel, dim3(chunks, tiles, B), dim3(NCG_THREADS), 0, st, reinterpret_cast<const float2*>(y),
                     weights, part, B, n_coils, M);
  const int rc = ipdm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(nc_gram_reduce_kernel, dim3(tiles, B), dim3(NCG_THREADS), 0, st, part, reinterpret_cast<float2*>(gram), n_coils,
                     chunks);
  return ipdm_launch_status();
}
