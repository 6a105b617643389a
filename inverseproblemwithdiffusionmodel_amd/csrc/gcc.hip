// Geometric coil compression along the fully sampled readout axis H (Zhang, Pauly, Vasanawala, Lustig, MRM 2013;
// DESIGN.md 4.4j).  One compression matrix per readout position x instead of one per image:
//     h = R^-1 y (centred inverse DFT along H, a strip pass over the columns of every coil plane)
//     ->  G_{b,x}: Gram matrix of the calibration columns over the rows [x - win, x + win] of h  (double sums, one rounding)
//     ->  the eigen-stage of coilcomp.hip over the B*H matrices  ->  alignment of the matrices along x
//     ->  h'_v(x, c) = sum_k A_{b,x}[v][k] h_k(x, c)  ->  y' = R h'
// The alignment is a chain in x: one workgroup per (image, direction) walks outward from the centre row with the matrices
// in LDS and turns each position onto its neighbour by the unitary polar factor of C = A^_x psi A_p^H (Newton-Schulz on
// nv x nv matrices).  No atomics, no host synchronisation: an image's results do not depend on its batch.
#include "kspace_fft.h"

// the eigen-stage of coilcomp.hip over any count of matrices (the public entry point keeps its 65535 limit)
namespace ipdm_coilcomp {
int matrix_many(const float2* gram, const float2* psi, int nv, float2* A, float* eig, int32_t* status, int64_t count, int n,
                hipStream_t s);
}

namespace {

using namespace ipdm_kspace;

constexpr int GCC_MAX_COILS = 64;
constexpr int GCC_MAX_VIRTUAL = 32;
constexpr int GCC_MAX_WIN = 8;
constexpr int GCC_THREADS = 256;
constexpr int GCC_GRAM_CHUNK = 32;              // window samples staged per pass
constexpr int GCC_NS_ITERS = 30;                // Newton-Schulz iterations of the polar factor
constexpr float GCC_NS_TOL = 1.0e-3f;           // |X^H X - I| above it (either component of any entry): a degenerate position
constexpr int RO_STRIP_ELEMS = 4096;            // complex elements of a readout strip (32 KiB): two columns at H = 2048
constexpr int RO_MAX_SIDE = 2048;

__device__ __forceinline__ float2 g_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 g_mulc(float2 a, float2 b) {           // a conj(b)
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ float2 g_cmul(float2 a, float2 b) {           // conj(a) b
  return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

// ---- the readout transform -------------------------------------------------------------------------------------------------
// Workgroup blockIdx.x = plane * nstrips + strip: columns [c0, c0 + CS) of one [H][W] plane, LDS layout buf[r * CS + lc] as
// cols_kernel of kspace_large.hip.  CS = min(W, RO_STRIP_ELEMS / H); the last strip of a plane may be ragged: its missing
// columns are zeros in LDS and are not stored.  Centring as fft2c: (-1)^r on the way in and on the way out (H is a multiple
// of 4), 1 / sqrt(H) on the way out.  A column's arithmetic does not depend on its strip or plane.
template <bool MIXED>
__global__ __launch_bounds__(FFT_THREADS) void readout_fft_kernel(const float2* __restrict__ in, float2* __restrict__ out, int H,
                                                                  int W, int CS, int nstrips, int inverse, float scale) {
  extern __shared__ __align__(16) unsigned char ro_smem[];
  FftLds L;
  L.buf = reinterpret_cast<float2*>(ro_smem);
  L.tw = L.buf + RO_STRIP_ELEMS;
  L.twN = H;
  fft_make_twiddles(L);
  const int64_t plane = blockIdx.x / nstrips;
  const int c0 = (int)(blockIdx.x - plane * nstrips) * CS;
  const float2* src = in + (size_t)plane * H * W;
  float2* dst = out + (size_t)plane * H * W;
  const int n = H * CS;
  for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
    const int r = e / CS, lc = e - r * CS;
    float2 v = make_float2(0.f, 0.f);
    if (c0 + lc < W) {
      v = src[(size_t)r * W + c0 + lc];
      const float s = (r & 1) ? -1.f : 1.f;
      v = make_float2(v.x * s, v.y * s);
    }
    L.buf[e] = v;
  }
  __syncthreads();
  fft_lines<MIXED>(L, H, CS, 1, CS, true, inverse != 0);
  for (int e = threadIdx.x; e < n; e += FFT_THREADS) {
    const int r = e / CS, lc = e - r * CS;
    if (c0 + lc < W) {
      const float s = (r & 1) ? -scale : scale;
      const float2 v = L.buf[e];
      dst[(size_t)r * W + c0 + lc] = make_float2(v.x * s, v.y * s);
    }
  }
}

// ---- windowed Gram matrices ------------------------------------------------------------------------------------------------
// Workgroup (blockIdx.x, x, b): pairs t = blockIdx.x * 256 + tid of the upper triangle of G_{b,x}, coil_gram_kernel's form
// with the box replaced by the rows [x - win, x + win] (clipped to the image) of the calibration columns: samples staged
// GCC_GRAM_CHUNK at a time for all coils, rows ascending then columns ascending, products and sums in double.
__global__ __launch_bounds__(GCC_THREADS) void gcc_gram_kernel(const float2* __restrict__ h, float2* __restrict__ gram, int B, int n,
                                                               int H, int W, int aw, int win) {
  __shared__ float2 smp[GCC_MAX_COILS * (GCC_GRAM_CHUNK + 1)];
  const int x = blockIdx.y, b = blockIdx.z;
  const int bw = 2 * aw + 1;
  const int r0 = x - win < 0 ? 0 : x - win, r1 = x + win > H - 1 ? H - 1 : x + win;
  const int nbox = (r1 - r0 + 1) * bw;
  const int c0 = W / 2 - aw;
  const size_t HW = (size_t)H * W;
  const int npairs = n * (n + 1) / 2;
  const int t = blockIdx.x * GCC_THREADS + threadIdx.x;
  int i = 0, j = 0;
  if (t < npairs) {
    int rem = t;
    while (rem >= n - i) { rem -= n - i; ++i; }
    j = i + rem;
  }
  double acc_re = 0.0, acc_im = 0.0;
  for (int k0 = 0; k0 < nbox; k0 += GCC_GRAM_CHUNK) {
    for (int idx = threadIdx.x; idx < n * GCC_GRAM_CHUNK; idx += GCC_THREADS) {
      const int c = idx / GCC_GRAM_CHUNK, s = idx - c * GCC_GRAM_CHUNK;
      const int k = k0 + s;
      float2 v = make_float2(0.f, 0.f);
      if (k < nbox) {
        const int r = k / bw, cc = k - r * bw;
        v = h[((size_t)c * B + b) * HW + (size_t)(r0 + r) * W + (c0 + cc)];
      }
      smp[c * (GCC_GRAM_CHUNK + 1) + s] = v;
    }
    __syncthreads();
    if (t < npairs) {
      const float2* pi = smp + i * (GCC_GRAM_CHUNK + 1);
      const float2* pj = smp + j * (GCC_GRAM_CHUNK + 1);
#pragma unroll 4
      for (int s = 0; s < GCC_GRAM_CHUNK; ++s) {                 // samples past the window are zeros: they add exactly nothing
        const float2 a = pi[s], c = pj[s];
        acc_re += (double)a.x * (double)c.x + (double)a.y * (double)c.y;
        acc_im += (double)a.y * (double)c.x - (double)a.x * (double)c.y;
      }
    }
    __syncthreads();
  }
  if (t < npairs) {
    float2* g = gram + ((size_t)b * H + x) * n * n;
    const float re = (float)acc_re, im = i == j ? 0.f : (float)acc_im;
    g[i * n + j] = make_float2(re, im);
    if (i != j) g[j * n + i] = make_float2(re, -im);
  }
}

// ---- alignment along x -------------------------------------------------------------------------------------------------------
// Workgroup (dir, b): dir 0 walks x0 - 1 .. 0 (and copies the centre row x0 = H / 2), dir 1 walks x0 + 1 .. H - 1.  Per
// position:  W = A^_x psi (psi NULL: W = A^_x),  C = W A_p^H,  X <- 1.5 X - 0.5 X (X^H X) from X = C, GCC_NS_ITERS times,
// A_x = X^H A^_x.  A_p is the last aligned position on the centre side that was not degenerate; a degenerate position
// (some entry of X^H X - I above GCC_NS_TOL in either component, NaN included) keeps A^_x and is counted.  Every sum runs
// over its index ascending, products and sums rounded one by one (tests/gcc_helpers.py restates them).
// LDS: psi [n][ldn], A^_x, W, A_p [nv][ldn], three [nv][ldv] squares; ldn = n | 1, ldv = nv | 1 (105 KiB at 64 -> 32).
__global__ __launch_bounds__(GCC_THREADS) void gcc_align_kernel(const float2* __restrict__ Ahat, const float2* __restrict__ psi,
                                                                float2* __restrict__ A, const int32_t* __restrict__ mstat,
                                                                int32_t* __restrict__ dstat, int H, int n, int nv) {
  extern __shared__ __align__(16) unsigned char al_smem[];
  __shared__ int degen;
  const int ldn = n | 1, ldv = nv | 1;
  float2* Ax = reinterpret_cast<float2*>(al_smem);
  float2* Ap = Ax + nv * ldn;
  float2* X = Ap + nv * ldn;
  float2* Y = X + nv * ldv;
  float2* Z = Y + nv * ldv;
  float2* Wx = psi ? Z + nv * ldv : Ax;
  float2* Ps = Wx + nv * ldn;                    // only with psi
  const int dir = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int x0 = H / 2;
  const size_t mat = (size_t)nv * n;
  const float2* Ab = Ahat + (size_t)b * H * mat;
  float2* Ob = A + (size_t)b * H * mat;

  if (mstat && mstat[(size_t)b * H + x0] != 0) {   // the eigen-stage refused psi (uniform): zero matrices, status -1
    const int xa = dir == 0 ? 0 : x0 + 1, xb = dir == 0 ? x0 + 1 : H;
    for (size_t e = (size_t)xa * mat + tid; e < (size_t)xb * mat; e += GCC_THREADS) Ob[e] = make_float2(0.f, 0.f);
    if (tid == 0) dstat[b * 2 + dir] = -1;
    return;
  }
  for (int e = tid; e < nv * n; e += GCC_THREADS) {
    const int i = e / n, k = e - i * n;
    const float2 v = Ab[(size_t)x0 * mat + e];
    Ap[i * ldn + k] = v;
    if (dir == 0) Ob[(size_t)x0 * mat + e] = v;
  }
  if (psi)
    for (int e = tid; e < n * n; e += GCC_THREADS) {
      const int i = e / n, k = e - i * n;
      Ps[i * ldn + k] = psi[e];
    }
  int count = 0;
  const int step = dir == 0 ? -1 : 1;
  for (int x = x0 + step; x >= 0 && x < H; x += step) {
    __syncthreads();                               // A_p (and psi) complete; the previous position's reads are over
    for (int e = tid; e < nv * n; e += GCC_THREADS) {
      const int i = e / n, k = e - i * n;
      Ax[i * ldn + k] = Ab[(size_t)x * mat + e];
    }
    if (tid == 0) degen = 0;
    __syncthreads();
    if (psi) {
      for (int e = tid; e < nv * n; e += GCC_THREADS) {
        const int i = e / n, k = e - i * n;
        float2 a = make_float2(0.f, 0.f);
        for (int j = 0; j < n; ++j) {
          const float2 t = g_mul(Ax[i * ldn + j], Ps[j * ldn + k]);
          a = make_float2(a.x + t.x, a.y + t.y);
        }
        Wx[i * ldn + k] = a;
      }
      __syncthreads();
    }
    for (int e = tid; e < nv * nv; e += GCC_THREADS) {
      const int i = e / nv, j = e - i * nv;
      float2 a = make_float2(0.f, 0.f);
      for (int k = 0; k < n; ++k) {
        const float2 t = g_mulc(Wx[i * ldn + k], Ap[j * ldn + k]);
        a = make_float2(a.x + t.x, a.y + t.y);
      }
      X[i * ldv + j] = a;
    }
    __syncthreads();
    for (int it = 0; it <= GCC_NS_ITERS; ++it) {
      for (int e = tid; e < nv * nv; e += GCC_THREADS) {         // Y = X^H X
        const int i = e / nv, j = e - i * nv;
        float2 a = make_float2(0.f, 0.f);
        for (int k = 0; k < nv; ++k) {
          const float2 t = g_cmul(X[k * ldv + i], X[k * ldv + j]);
          a = make_float2(a.x + t.x, a.y + t.y);
        }
        Y[i * ldv + j] = a;
      }
      __syncthreads();
      if (it == GCC_NS_ITERS) break;                             // the last pass only measures X^H X
      for (int e = tid; e < nv * nv; e += GCC_THREADS) {         // Z = 1.5 X - 0.5 X Y
        const int i = e / nv, j = e - i * nv;
        float2 a = make_float2(0.f, 0.f);
        for (int k = 0; k < nv; ++k) {
          const float2 t = g_mul(X[i * ldv + k], Y[k * ldv + j]);
          a = make_float2(a.x + t.x, a.y + t.y);
        }
        const float2 v = X[i * ldv + j];
        Z[i * ldv + j] = make_float2(1.5f * v.x - 0.5f * a.x, 1.5f * v.y - 0.5f * a.y);
      }
      __syncthreads();
      float2* sw = X;
      X = Z;
      Z = sw;
    }
    for (int e = tid; e < nv * nv; e += GCC_THREADS) {
      const int i = e / nv, j = e - i * nv;
      const float2 v = Y[i * ldv + j];
      const float dr = fabsf(v.x - (i == j ? 1.f : 0.f)), di = fabsf(v.y);
      if (!(dr <= GCC_NS_TOL) || !(di <= GCC_NS_TOL)) degen = 1;
    }
    __syncthreads();
    const bool bad = degen != 0;                                 // (uniform: read after the barrier)
    if (bad) ++count;
    for (int e = tid; e < nv * n; e += GCC_THREADS) {
      const int i = e / n, k = e - i * n;
      float2 a;
      if (bad) {
        a = Ax[i * ldn + k];
      } else {
        a = make_float2(0.f, 0.f);
        for (int j = 0; j < nv; ++j) {                           // (X^H A^_x)[i][k]
          const float2 t = g_cmul(X[j * ldv + i], Ax[j * ldn + k]);
          a = make_float2(a.x + t.x, a.y + t.y);
        }
        Ap[i * ldn + k] = a;                                     // a degenerate position is no reference for the next one
      }
      Ob[(size_t)x * mat + e] = a;
    }
  }
  if (tid == 0) dstat[b * 2 + dir] = count;
}

__global__ void gcc_status_kernel(const int32_t* __restrict__ dstat, int32_t* __restrict__ status, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    const int a = dstat[2 * b], c = dstat[2 * b + 1];
    status[b] = (a < 0 || c < 0) ? -1 : a + c;
  }
}

// ---- h'_v(x, c) = sum_k A_{b,x}[v][k] h_k(x, c) ------------------------------------------------------------------------------
// coil_apply_kernel<NV> of coilcomp.hip with the matrix chosen by row: workgroup (x, b) reloads the LDS matrix [coil][NV] for
// its row and walks the row's W pixels, one per thread and pass.  Four fused multiply-adds per product, coils in order.
template <int NV>
__global__ __launch_bounds__(GCC_THREADS) void coil_apply_rows_kernel(const float2* __restrict__ y, const float2* __restrict__ A,
                                                                      float2* __restrict__ out, int B, int n, int nv, int H, int W,
                                                                      int per_image) {
  __shared__ __align__(16) float2 mat[GCC_MAX_COILS * NV];
  const int x = blockIdx.x, b = blockIdx.y;
  const float2* Ax = A + ((per_image ? (size_t)b * H : 0) + x) * nv * n;
  for (int e = threadIdx.x; e < n * NV; e += GCC_THREADS) {
    const int c = e / NV, v = e - c * NV;
    mat[e] = v < nv ? Ax[v * n + c] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const size_t plane = (size_t)B * H * W;
  const size_t row = ((size_t)b * H + x) * W;
  for (int e = threadIdx.x; e < W; e += GCC_THREADS) {
    const float2* src = y + row + e;
    float2 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int c = 0; c < n; ++c) {
      const float2 s = src[(size_t)c * plane];
      const float2* mr = mat + c * NV;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float2 a = mr[v];
        acc[v].x = __builtin_fmaf(a.x, s.x, acc[v].x);
        acc[v].x = __builtin_fmaf(-a.y, s.y, acc[v].x);
        acc[v].y = __builtin_fmaf(a.x, s.y, acc[v].y);
        acc[v].y = __builtin_fmaf(a.y, s.x, acc[v].y);
      }
    }
    float2* dst = out + row + e;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (v < nv) dst[(size_t)v * plane] = acc[v];
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static inline bool readout_ok(int H) { return fft_side_ok(H) && H <= RO_MAX_SIDE; }
static inline bool counts_ok(int n, int nv) { return n >= 1 && n <= GCC_MAX_COILS && nv >= 1 && nv <= n && nv <= GCC_MAX_VIRTUAL; }
static inline bool cols_ok(int aw, int W) { return aw >= 0 && W / 2 - aw >= 0 && W / 2 + aw <= W - 1; }
static inline int padded(int nv) { return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : nv <= 16 ? 16 : 32; }
static inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

static int readout_launch(const float2* in, float2* out, int inverse, int64_t planes, int H, int W, hipStream_t s) {
  const int CS = W < RO_STRIP_ELEMS / H ? W : RO_STRIP_ELEMS / H;
  const int nstrips = (W + CS - 1) / CS;
  if (planes * nstrips > 0x7fffffffLL) return IPDM_EUNSUPPORTED;
  const size_t lds = ((size_t)RO_STRIP_ELEMS + (size_t)H) * sizeof(float2);
  const float scale = 1.f / sqrtf((float)H);
  const dim3 grid((unsigned)(planes * nstrips));
  return fft_dispatch(!is_pow2(H), [&](auto mixed) {
    constexpr bool MIXED = decltype(mixed)::value;
    return ipdm_launch_lds(readout_fft_kernel<MIXED>, grid, dim3(FFT_THREADS), lds, s, in, out, H, W, CS, nstrips, inverse, scale);
  });
}

static int gram_launch(const float2* h, int aw, int win, float2* gram, int B, int n, int H, int W, hipStream_t s) {
  const int npairs = n * (n + 1) / 2;
  hipLaunchKernelGGL(gcc_gram_kernel, dim3((npairs + GCC_THREADS - 1) / GCC_THREADS, H, B), dim3(GCC_THREADS), 0, s, h, gram, B, n, H, W,
                     aw, win);
  return ipdm_launch_status();
}

static size_t align_lds(int n, int nv, bool psi) {
  const size_t ldn = n | 1, ldv = nv | 1;
  return ((psi ? 3 : 2) * nv * ldn + 3 * nv * ldv + (psi ? n * ldn : 0)) * sizeof(float2);
}

static int align_launch(const float2* Ahat, const float2* psi, float2* A, const int32_t* mstat, int32_t* dstat, int32_t* status,
                        int B, int H, int n, int nv, hipStream_t s) {
  int rc = ipdm_launch_lds(gcc_align_kernel, dim3(2, B), dim3(GCC_THREADS), align_lds(n, nv, psi != nullptr), s, Ahat, psi, A, mstat,
                           dstat, H, n, nv);
  if (rc) return rc;
  hipLaunchKernelGGL(gcc_status_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const int32_t*)dstat, status, B);
  return ipdm_launch_status();
}

template <int NV>
static int launch_rows(const float2* y, const float2* A, float2* out, int B, int n, int nv, int H, int W, int per_image, hipStream_t s) {
  hipLaunchKernelGGL(coil_apply_rows_kernel<NV>, dim3(H, B), dim3(GCC_THREADS), 0, s, y, A, out, B, n, nv, H, W, per_image);
  return ipdm_launch_status();
}
static int rows_launch(const float2* y, const float2* A, int per_image, float2* out, int B, int n, int nv, int H, int W, hipStream_t s) {
  switch (padded(nv)) {
    case 1: return launch_rows<1>(y, A, out, B, n, nv, H, W, per_image, s);
    case 2: return launch_rows<2>(y, A, out, B, n, nv, H, W, per_image, s);
    case 4: return launch_rows<4>(y, A, out, B, n, nv, H, W, per_image, s);
    case 8: return launch_rows<8>(y, A, out, B, n, nv, H, W, per_image, s);
    case 16: return launch_rows<16>(y, A, out, B, n, nv, H, W, per_image, s);
    default: return launch_rows<32>(y, A, out, B, n, nv, H, W, per_image, s);
  }
}

// workspace of the whole chain, in this order; every part starts on a multiple of 16 bytes
struct GccWork {
  size_t hybrid, gram, ahat, mstat, dstat, total;
};
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static GccWork gcc_work(int B, int n, int nv, int H, int W) {
  GccWork w;
  size_t at = 0;
  w.hybrid = at;
  at += up16((size_t)n * B * H * W * sizeof(float2));
  w.gram = at;
  at += up16((size_t)B * H * n * n * sizeof(float2));
  w.ahat = at;
  at += up16((size_t)B * H * nv * n * sizeof(float2));
  w.mstat = at;
  at += up16((size_t)B * H * sizeof(int32_t));
  w.dstat = at;
  at += up16((size_t)B * 2 * sizeof(int32_t));
  w.total = at;
  return w;
}

}  // namespace

extern "C" int ipdm_gcc_supported(int n_coils, int n_virtual, int H, int W, int win) {
  return counts_ok(n_coils, n_virtual) && readout_ok(H) && W >= 1 && win >= 0 && win <= GCC_MAX_WIN;
}

extern "C" size_t ipdm_gcc_workspace_bytes(int B, int n_coils, int n_virtual, int H, int W) {
  if (B <= 0 || B > 65535 || !ipdm_gcc_supported(n_coils, n_virtual, H, W, 0)) return 0;
  return gcc_work(B, n_coils, n_virtual, H, W).total;
}

extern "C" int ipdm_readout_fft_c64(const float* in, float* out, int inverse, int64_t planes, int H, int W, void* stream) {
  IPDM_REQUIRE(planes >= 0 && H > 0 && W > 0);
  if (!readout_ok(H)) return IPDM_EUNSUPPORTED;
  if (planes == 0) return IPDM_OK;
  IPDM_REQUIRE(in && out);
  const size_t bytes = (size_t)planes * H * W * sizeof(float2);
  IPDM_REQUIRE(in == out || !overlaps(in, bytes, out, bytes));   // in place is fine: a strip is read whole before it is stored
  return readout_launch(reinterpret_cast<const float2*>(in), reinterpret_cast<float2*>(out), inverse != 0, planes, H, W,
                        ipdm_stream(stream));
}

extern "C" int ipdm_gcc_gram_c64(const float* h, int aw, int win, float* gram, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && H > 0 && W > 0 && cols_ok(aw, W) && win >= 0);
  if (n_coils > GCC_MAX_COILS || B > 65535 || H > 65535 || win > GCC_MAX_WIN) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(h && gram);
  return gram_launch(reinterpret_cast<const float2*>(h), aw, win, reinterpret_cast<float2*>(gram), B, n_coils, H, W, ipdm_stream(stream));
}

extern "C" int ipdm_gcc_align_c64(const float* Ahat, const float* noise_cov, float* A, int32_t* status, int32_t* work, int B, int H,
                                  int n_coils, int n_virtual, void* stream) {
  IPDM_REQUIRE(B >= 0 && H > 0 && n_coils > 0 && n_virtual > 0);
  if (!counts_ok(n_coils, n_virtual) || B > 65535) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(Ahat && A && status && work);
  const size_t bytes = (size_t)B * H * n_virtual * n_coils * sizeof(float2);
  IPDM_REQUIRE(!overlaps(Ahat, bytes, A, bytes));
  return align_launch(reinterpret_cast<const float2*>(Ahat), reinterpret_cast<const float2*>(noise_cov), reinterpret_cast<float2*>(A),
                      nullptr, work, status, B, H, n_coils, n_virtual, ipdm_stream(stream));
}

extern "C" int ipdm_coil_apply_rows_c64(const float* y, const float* A, int per_image, float* out, int B, int n_coils, int n_virtual,
                                        int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && n_virtual > 0 && H > 0 && W > 0);
  if (!counts_ok(n_coils, n_virtual) || B > 65535) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && A && out);
  const size_t P = (size_t)B * H * W * sizeof(float2);
  IPDM_REQUIRE(!overlaps(y, n_coils * P, out, n_virtual * P));
  return rows_launch(reinterpret_cast<const float2*>(y), reinterpret_cast<const float2*>(A), per_image != 0,
                     reinterpret_cast<float2*>(out), B, n_coils, n_virtual, H, W, ipdm_stream(stream));
}

extern "C" int ipdm_gcc_compress_c64(const float* y, int aw, int win, int n_virtual, const float* noise_cov, float* A, float* eig,
                                     int32_t* status, float* out, float* work, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && n_virtual > 0 && H > 0 && W > 0 && cols_ok(aw, W) && win >= 0);
  if (!ipdm_gcc_supported(n_coils, n_virtual, H, W, win) || B > 65535) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && A && status && out && work);
  const size_t P = (size_t)B * H * W * sizeof(float2);
  const GccWork w = gcc_work(B, n_coils, n_virtual, H, W);
  IPDM_REQUIRE(!overlaps(y, n_coils * P, out, n_virtual * P) && !overlaps(work, w.total, y, n_coils * P) &&
               !overlaps(work, w.total, out, n_virtual * P));
  hipStream_t s = ipdm_stream(stream);
  unsigned char* base = reinterpret_cast<unsigned char*>(work);
  float2* hyb = reinterpret_cast<float2*>(base + w.hybrid);
  float2* gram = reinterpret_cast<float2*>(base + w.gram);
  float2* ahat = reinterpret_cast<float2*>(base + w.ahat);
  int32_t* mstat = reinterpret_cast<int32_t*>(base + w.mstat);
  int32_t* dstat = reinterpret_cast<int32_t*>(base + w.dstat);
  const float2* psi = reinterpret_cast<const float2*>(noise_cov);
  float2* o = reinterpret_cast<float2*>(out);
  int rc = readout_launch(reinterpret_cast<const float2*>(y), hyb, 1, (int64_t)n_coils * B, H, W, s);
  if (rc) return rc;
  rc = gram_launch(hyb, aw, win, gram, B, n_coils, H, W, s);
  if (rc) return rc;
  rc = ipdm_coilcomp::matrix_many(gram, psi, n_virtual, ahat, eig, mstat, (int64_t)B * H, n_coils, s);
  if (rc) return rc;
  rc = align_launch(ahat, psi, reinterpret_cast<float2*>(A), mstat, dstat, status, B, H, n_coils, n_virtual, s);
  if (rc) return rc;
  rc = rows_launch(hyb, reinterpret_cast<const float2*>(A), 1, o, B, n_coils, n_virtual, H, W, s);
  if (rc) return rc;
  return readout_launch(o, o, 0, (int64_t)n_virtual * B, H, W, s);
}
