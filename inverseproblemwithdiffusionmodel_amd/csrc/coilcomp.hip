// Coil compression and noise prewhitening of measured multi-coil k-space (software coil compression by PCA of the
// calibration data, Buehrer 2007 / Huang 2008).  Three launches, all asynchronous:
//     Gram matrix of the calibration box, per image  ->  whitening, eigendecomposition, sort and gauge -> A [nv][nc]
//     ->  y'_v = sum_c A[v][c] y_c on every pixel (the streaming kernel)
// coil_gram_kernel sums in double (exact products of floats, one rounding at the end); coil_eig_kernel is a cyclic
// two-sided Hermitian Jacobi in LDS with the round-robin pair ordering, fp32, every rounding in a fixed order that
// tests/coilcomp_helpers.py restates operation by operation; coil_apply_kernel<NV> keeps NV complex accumulators per pixel
// in registers and walks the input coils once, the matrix broadcast from LDS.  No atomics anywhere: an image's results do
// not depend on its batch.
#include "launch.h"

namespace {

constexpr int CC_MAX_COILS = 64;
constexpr int CC_MAX_VIRTUAL = 32;
constexpr int CC_SWEEPS = 12;                   // Jacobi sweeps (every test case converged after 8)
constexpr int CC_THREADS = 256;
constexpr int CC_GRAM_CHUNK = 32;               // calibration samples staged per pass
constexpr float CC_TAU_BIG = 1.0e8f;            // beyond it sqrt(1 + tau^2) == |tau| in fp32 and tau^2 may overflow

__device__ __forceinline__ float2 cc_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cc_mulc(float2 a, float2 b) {          // a conj(b)
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// ---- Gram matrix of the calibration box ----------------------------------------------------------------------------------
// Workgroup (blockIdx.x, b): pairs t = blockIdx.x * 256 + tid of the upper triangle (i <= j) of image b.  The box is staged
// CC_GRAM_CHUNK samples at a time for all coils ([coil][CC_GRAM_CHUNK + 1] float2 of LDS, 16.5 KiB at 64 coils); y is read
// inside the box only.  Samples run in box order, products and sums in double: G is the float64 result rounded once.
__global__ __launch_bounds__(CC_THREADS) void coil_gram_kernel(const float2* __restrict__ y, float2* __restrict__ gram, int B,
                                                               int n, int H, int W, int ah, int aw) {
  __shared__ float2 smp[CC_MAX_COILS * (CC_GRAM_CHUNK + 1)];
  const int b = blockIdx.y;
  const int bw = 2 * aw + 1, nbox = (2 * ah + 1) * bw;
  const int r0 = H / 2 - ah, c0 = W / 2 - aw;
  const size_t HW = (size_t)H * W;
  const int npairs = n * (n + 1) / 2;
  const int t = blockIdx.x * CC_THREADS + threadIdx.x;
  int i = 0, j = 0;
  if (t < npairs) {
    int rem = t;
    while (rem >= n - i) { rem -= n - i; ++i; }
    j = i + rem;
  }
  double acc_re = 0.0, acc_im = 0.0;
  for (int k0 = 0; k0 < nbox; k0 += CC_GRAM_CHUNK) {
    for (int idx = threadIdx.x; idx < n * CC_GRAM_CHUNK; idx += CC_THREADS) {
      const int c = idx / CC_GRAM_CHUNK, s = idx - c * CC_GRAM_CHUNK;
      const int k = k0 + s;
      float2 v = make_float2(0.f, 0.f);
      if (k < nbox) {
        const int r = k / bw, cc = k - r * bw;
        v = y[((size_t)c * B + b) * HW + (size_t)(r0 + r) * W + (c0 + cc)];
      }
      smp[c * (CC_GRAM_CHUNK + 1) + s] = v;
    }
    __syncthreads();
    if (t < npairs) {
      const float2* pi = smp + i * (CC_GRAM_CHUNK + 1);
      const float2* pj = smp + j * (CC_GRAM_CHUNK + 1);
#pragma unroll 4
      for (int s = 0; s < CC_GRAM_CHUNK; ++s) {                  // samples past the box are zeros: they add exactly nothing
        const float2 a = pi[s], c = pj[s];
        acc_re += (double)a.x * (double)c.x + (double)a.y * (double)c.y;
        acc_im += (double)a.y * (double)c.x - (double)a.x * (double)c.y;
      }
    }
    __syncthreads();
  }
  if (t < npairs) {
    float2* g = gram + (size_t)b * n * n;
    const float re = (float)acc_re, im = i == j ? 0.f : (float)acc_im;
    g[i * n + j] = make_float2(re, im);
    if (i != j) g[j * n + i] = make_float2(re, -im);
  }
}

// ---- whitening, eigendecomposition, sort, gauge ----------------------------------------------------------------------------
// One workgroup per image.  LDS: G, V (and L, X = L^-1 with a noise covariance) as [n][ld] float2, ld = n | 1 so that a column
// walk of 32 lanes touches 32 different banks; at 64 coils 2 (4) x 33 280 bytes.
struct CcRot { float c; float2 s; };            // J = [[c, s], [-conj(s), c]] on the (p, q) plane

__device__ __forceinline__ void cc_pair(int m, int r, int k, int& p, int& q) {   // round-robin: m players (even), round r, table k
  int a, c;
  if (k == 0) {
    a = m - 1;
    c = r;
  } else {
    a = (r + k) % (m - 1);
    c = (r - k + (m - 1)) % (m - 1);
  }
  p = a < c ? a : c;
  q = a < c ? c : a;
}

__global__ __launch_bounds__(CC_THREADS) void coil_eig_kernel(const float2* __restrict__ gram, const float2* __restrict__ psi,
                                                              float2* __restrict__ A_out, float* __restrict__ eig_out,
                                                              int32_t* __restrict__ status, int n, int nv) {
  extern __shared__ __align__(16) unsigned char cc_smem[];
  __shared__ CcRot rot[CC_MAX_COILS / 2];
  __shared__ int2 pq[CC_MAX_COILS / 2];
  __shared__ float lam[CC_MAX_COILS];
  __shared__ int perm[CC_MAX_COILS];
  __shared__ float red[CC_THREADS / 64];
  __shared__ int bad;
  const int ld = n | 1;
  float2* G = reinterpret_cast<float2*>(cc_smem);
  float2* V = G + n * ld;
  float2* L = V + n * ld;                        // only with psi
  float2* X = L + n * ld;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float2* g_in = gram + (size_t)b * n * n;
  float2* A = A_out + (size_t)b * nv * n;
  float* eig = eig_out ? eig_out + (size_t)b * n : nullptr;

  // G <- gram / 2^e, 2^e the power of two at or above the largest diagonal entry: an exact scaling, undone on the eigenvalues
  float dmax = 0.f;
  for (int i = tid; i < n; i += CC_THREADS) dmax = fmaxf(dmax, fabsf(g_in[i * n + i].x));
  dmax = ipdm_wave_max(dmax);
  if ((tid & 63) == 0) red[tid >> 6] = dmax;
  if (tid == 0) bad = 0;
  __syncthreads();
  dmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int ex = 0;
  if (dmax > 0.f && dmax < INFINITY) frexpf(dmax, &ex);
  ex = ex < -120 ? -120 : ex > 120 ? 120 : ex;
  const float down = ldexpf(1.f, -ex), up = ldexpf(1.f, ex);
  for (int e = tid; e < n * n; e += CC_THREADS) {
    const int i = e / n, j = e - i * n;
    const float2 v = g_in[e];
    G[i * ld + j] = make_float2(v.x * down, v.y * down);
    V[i * ld + j] = make_float2(i == j ? 1.f : 0.f, 0.f);
  }
  __syncthreads();

  if (psi) {
    // Cholesky psi = L L^H, column by column; a pivot that is not positive (NaN included) stops the image
    for (int e = tid; e < n * n; e += CC_THREADS) {
      const int i = e / n, j = e - i * n;
      L[i * ld + j] = i >= j ? psi[e] : make_float2(0.f, 0.f);
      X[i * ld + j] = make_float2(0.f, 0.f);
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      if (tid == 0) {
        float d = L[j * ld + j].x;
        for (int k = 0; k < j; ++k) {
          const float2 l = L[j * ld + k];
          d = d - (l.x * l.x + l.y * l.y);
        }
        if (!(d > 0.f) || !(d < INFINITY)) {
          bad = 1;
          d = 1.f;
        }
        L[j * ld + j] = make_float2(sqrtf(d), 0.f);
      }
      __syncthreads();
      const float piv = L[j * ld + j].x;
      for (int i = j + 1 + tid; i < n; i += CC_THREADS) {
        float2 a = L[i * ld + j];
        for (int k = 0; k < j; ++k) {
          const float2 t = cc_mulc(L[i * ld + k], L[j * ld + k]);
          a = make_float2(a.x - t.x, a.y - t.y);
        }
        L[i * ld + j] = make_float2(a.x / piv, a.y / piv);
      }
      __syncthreads();
    }
    if (bad) {                                   // (uniform: read after the barrier)
      for (int e = tid; e < nv * n; e += CC_THREADS) A[e] = make_float2(0.f, 0.f);
      if (eig)
        for (int i = tid; i < n; i += CC_THREADS) eig[i] = 0.f;
      if (tid == 0) status[b] = 1;
      return;
    }
    // X = L^-1 by forward substitution, one column per thread
    for (int j = tid; j < n; j += CC_THREADS) {
      X[j * ld + j] = make_float2(1.f / L[j * ld + j].x, 0.f);
      for (int i = j + 1; i < n; ++i) {
        float2 a = make_float2(0.f, 0.f);
        for (int k = j; k < i; ++k) {
          const float2 t = cc_mul(L[i * ld + k], X[k * ld + j]);
          a = make_float2(a.x + t.x, a.y + t.y);
        }
        const float d = L[i * ld + i].x;
        X[i * ld + j] = make_float2(-a.x / d, -a.y / d);
      }
    }
    __syncthreads();
    // T = X G (into L, no longer needed), then G = upper triangle of T X^H, mirrored
    for (int e = tid; e < n * n; e += CC_THREADS) {
      const int j = e / n, i = e - j * n;       // i fastest: X walks a column, G broadcasts
      float2 a = make_float2(0.f, 0.f);
      for (int k = 0; k < n; ++k) {
        const float2 t = cc_mul(X[i * ld + k], G[k * ld + j]);
        a = make_float2(a.x + t.x, a.y + t.y);
      }
      L[i * ld + j] = a;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += CC_THREADS) {
      const int i = e / n, j = e - i * n;
      if (i > j) continue;
      float2 a = make_float2(0.f, 0.f);
      for (int k = 0; k < n; ++k) {
        const float2 t = cc_mulc(L[i * ld + k], X[j * ld + k]);
        a = make_float2(a.x + t.x, a.y + t.y);
      }
      if (i == j) a.y = 0.f;
      G[i * ld + j] = a;
      if (i != j) G[j * ld + i] = make_float2(a.x, -a.y);
    }
    __syncthreads();
  }

  // cyclic Jacobi, round-robin ordering: m - 1 rounds of m / 2 disjoint rotations per sweep.  A thread's work items
  // e = tid, tid + 256, ... of a phase are (table k, line i) = (e / n, e % n), stepped without a division.
  const int m = n + (n & 1), half = m / 2;
  const int dk = CC_THREADS / n, di = CC_THREADS - dk * n;
  const int k0 = tid / n, i0 = tid - k0 * n;
  for (int sw = 0; sw < CC_SWEEPS && n > 1; ++sw) {
    for (int r = 0; r < m - 1; ++r) {
      if (tid < half) {
        int p, q;
        cc_pair(m, r, tid, p, q);
        CcRot R;
        R.c = 1.f;
        R.s = make_float2(0.f, 0.f);
        if (q < n) {
          const float2 g = G[p * ld + q];
          const float mag = sqrtf(g.x * g.x + g.y * g.y);
          if (mag > 0.f) {                       // exactly zero (rank-deficient Grams, underflow): no rotation
            const float gap = G[q * ld + q].x - G[p * ld + p].x;
            const float tau = gap / (2.f * mag);
            float t;
            if (fabsf(tau) > CC_TAU_BIG) t = 0.5f / tau;
            else t = (tau >= 0.f ? 1.f : -1.f) / (fabsf(tau) + sqrtf(1.f + tau * tau));
            R.c = 1.f / sqrtf(1.f + t * t);
            const float s = t * R.c;
            R.s = make_float2(s * (g.x / mag), s * (g.y / mag));
          }
        }
        rot[tid] = R;                            // the phantom player's pair (q == n) keeps the identity: skipped below
        pq[tid] = make_int2(p, q);
      }
      __syncthreads();
      // columns: G <- G J, V <- V J
      for (int k = k0, i = i0; k < half;) {
        const CcRot R = rot[k];
        if (R.s.x != 0.f || R.s.y != 0.f) {
          const int p = pq[k].x, q = pq[k].y;
          const float2 gp = G[i * ld + p], gq = G[i * ld + q];
          float2 t = cc_mulc(gq, R.s);
          G[i * ld + p] = make_float2(R.c * gp.x - t.x, R.c * gp.y - t.y);
          t = cc_mul(gp, R.s);
          G[i * ld + q] = make_float2(t.x + R.c * gq.x, t.y + R.c * gq.y);
          const float2 vp = V[i * ld + p], vq = V[i * ld + q];
          t = cc_mulc(vq, R.s);
          V[i * ld + p] = make_float2(R.c * vp.x - t.x, R.c * vp.y - t.y);
          t = cc_mul(vp, R.s);
          V[i * ld + q] = make_float2(t.x + R.c * vq.x, t.y + R.c * vq.y);
        }
        k += dk;
        i += di;
        if (i >= n) {
          i -= n;
          ++k;
        }
      }
      __syncthreads();
      // rows: G <- J^H G; the rotated pair is zero by construction and the diagonal real
      for (int k = k0, j = i0; k < half;) {
        const CcRot R = rot[k];
        if (R.s.x != 0.f || R.s.y != 0.f) {
          const int p = pq[k].x, q = pq[k].y;
          const float2 gp = G[p * ld + j], gq = G[q * ld + j];
          float2 t = cc_mul(R.s, gq);
          float2 np_ = make_float2(R.c * gp.x - t.x, R.c * gp.y - t.y);
          t = cc_mulc(gp, R.s);
          float2 nq = make_float2(t.x + R.c * gq.x, t.y + R.c * gq.y);
          if (j == p) {
            np_.y = 0.f;
            nq = make_float2(0.f, 0.f);
          }
          if (j == q) {
            nq.y = 0.f;
            np_ = make_float2(0.f, 0.f);
          }
          G[p * ld + j] = np_;
          G[q * ld + j] = nq;
        }
        k += dk;
        j += di;
        if (j >= n) {
          j -= n;
          ++k;
        }
      }
      __syncthreads();
    }
  }

  // sort: descending, equal eigenvalues keep the lower original index first
  if (tid < n) {
    lam[tid] = G[tid * ld + tid].x;
    perm[tid] = tid;                             // NaN eigenvalues rank alike: every entry stays a valid column
  }
  __syncthreads();
  if (tid < n) {
    const float mine = lam[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float o = lam[j];
      rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
    }
    perm[rank] = tid;
    if (eig) eig[rank] = mine * up;
  }
  __syncthreads();
  // rows of A before the gauge, into G: conj(V[:, perm[v]]) (times L^-1)
  for (int e = tid; e < nv * n; e += CC_THREADS) {
    const int v = e / n, c = e - v * n;
    const int col = perm[v];
    float2 a;
    if (psi) {
      a = make_float2(0.f, 0.f);
      for (int k = 0; k < n; ++k) {              // conj(V[k][col]) X[k][c]
        const float2 u = V[k * ld + col], x = X[k * ld + c];
        const float2 t = make_float2(u.x * x.x + u.y * x.y, u.x * x.y - u.y * x.x);
        a = make_float2(a.x + t.x, a.y + t.y);
      }
    } else {
      const float2 u = V[c * ld + col];
      a = make_float2(u.x, -u.y);
    }
    G[v * ld + c] = a;
  }
  __syncthreads();
  for (int e = tid; e < nv * n; e += CC_THREADS) {
    const int v = e / n, c = e - v * n;
    const float2 ref = G[v * ld];
    const float mag = sqrtf(ref.x * ref.x + ref.y * ref.y);
    float2 a = G[v * ld + c];
    if (mag > 0.f) a = c == 0 ? make_float2(mag, 0.f) : cc_mulc(a, make_float2(ref.x / mag, ref.y / mag));
    A[e] = a;
  }
  if (tid == 0) status[b] = 0;
}

// ---- y' = A y, the streaming kernel -----------------------------------------------------------------------------------------
// Workgroup (blockIdx.x, b): pixels blockIdx.x * 256 + tid (grid stride) of image b, one pixel per thread and pass, NV complex
// accumulators in registers.  The matrix sits in LDS as [coil][NV] (rows past n_virtual are zeros), read as a broadcast; the
// coil planes are read once, 512 contiguous bytes per wave instruction.  Four fused multiply-adds per complex product, coils
// in order: the helper restates the same roundings.
template <int NV>
__global__ __launch_bounds__(CC_THREADS) void coil_apply_kernel(const float2* __restrict__ y, const float2* __restrict__ A,
                                                                float2* __restrict__ out, int B, int n, int nv, int64_t P,
                                                                int per_image) {
  __shared__ __align__(16) float2 mat[CC_MAX_COILS * NV];
  const int b = blockIdx.y;
  const float2* Ab = A + (per_image ? (size_t)b * nv * n : 0);
  for (int e = threadIdx.x; e < n * NV; e += CC_THREADS) {
    const int c = e / NV, v = e - c * NV;
    mat[e] = v < nv ? Ab[v * n + c] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const size_t plane = (size_t)B * P;
  for (int64_t e = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; e < P; e += (int64_t)gridDim.x * CC_THREADS) {
    const float2* src = y + (size_t)b * P + e;
    float2 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int c = 0; c < n; ++c) {
      const float2 s = src[(size_t)c * plane];
      const float2* row = mat + c * NV;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float2 a = row[v];
        acc[v].x = __builtin_fmaf(a.x, s.x, acc[v].x);
        acc[v].x = __builtin_fmaf(-a.y, s.y, acc[v].x);
        acc[v].y = __builtin_fmaf(a.x, s.y, acc[v].y);
        acc[v].y = __builtin_fmaf(a.y, s.x, acc[v].y);
      }
    }
    float2* dst = out + (size_t)b * P + e;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (v < nv) dst[(size_t)v * plane] = acc[v];
  }
}

static inline bool cc_box_ok(int a, int N) { return a >= 0 && N / 2 - a >= 0 && N / 2 + a <= N - 1; }
static inline int cc_padded(int nv) { return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : nv <= 16 ? 16 : 32; }

template <int NV>
static int launch_apply(const float2* y, const float2* A, float2* out, int B, int n, int nv, int64_t P, int per_image, hipStream_t s) {
  int64_t gx = (P + CC_THREADS - 1) / CC_THREADS;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(coil_apply_kernel<NV>, dim3((unsigned)gx, B), dim3(CC_THREADS), 0, s, y, A, out, B, n, nv, P, per_image);
  return ipdm_launch_status();
}

static int gram_launch(const float2* y, int ah, int aw, float2* gram, int B, int n, int H, int W, hipStream_t s) {
  const int npairs = n * (n + 1) / 2;
  hipLaunchKernelGGL(coil_gram_kernel, dim3((npairs + CC_THREADS - 1) / CC_THREADS, B), dim3(CC_THREADS), 0, s, y, gram, B, n, H, W, ah,
                     aw);
  return ipdm_launch_status();
}

static int matrix_launch(const float2* gram, const float2* psi, int nv, float2* A, float* eig, int32_t* status, int B, int n,
                         hipStream_t s) {
  const int ld = n | 1;
  const size_t lds = (size_t)(psi ? 4 : 2) * n * ld * sizeof(float2);         // 64 coils: 65 KiB, whitened 130 KiB
  return ipdm_launch_lds(coil_eig_kernel, dim3(B), dim3(CC_THREADS), lds, s, gram, psi, A, eig, status, n, nv);
}

static int apply_launch(const float2* y, const float2* A, int per_image, float2* out, int B, int n, int nv, int64_t P, hipStream_t s) {
  switch (cc_padded(nv)) {
    case 1: return launch_apply<1>(y, A, out, B, n, nv, P, per_image, s);
    case 2: return launch_apply<2>(y, A, out, B, n, nv, P, per_image, s);
    case 4: return launch_apply<4>(y, A, out, B, n, nv, P, per_image, s);
    case 8: return launch_apply<8>(y, A, out, B, n, nv, P, per_image, s);
    case 16: return launch_apply<16>(y, A, out, B, n, nv, P, per_image, s);
    default: return launch_apply<32>(y, A, out, B, n, nv, P, per_image, s);
  }
}

static inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

static int gram_check(int ah, int aw, int B, int n, int H, int W) {
  IPDM_REQUIRE(B >= 0 && n > 0 && H > 0 && W > 0 && cc_box_ok(ah, H) && cc_box_ok(aw, W));
  if (n > CC_MAX_COILS || B > 65535) return IPDM_EUNSUPPORTED;
  return IPDM_OK;
}
static int apply_check(int B, int n, int nv, int64_t P) {
  IPDM_REQUIRE(B >= 0 && n > 0 && nv > 0 && P >= 0);
  if (!ipdm_coilcomp_supported(n, nv) || B > 65535) return IPDM_EUNSUPPORTED;
  return IPDM_OK;
}

}  // namespace

// the eigen-stage over any count of matrices, for gcc.hip (one matrix per readout position): the grid is one-dimensional,
// so nothing but the public entry point's contract stops at 65535
namespace ipdm_coilcomp {
int matrix_many(const float2* gram, const float2* psi, int nv, float2* A, float* eig, int32_t* status, int64_t count, int n,
                hipStream_t s) {
  if (count > 0x7fffffffLL) return IPDM_EUNSUPPORTED;
  return matrix_launch(gram, psi, nv, A, eig, status, (int)count, n, s);
}
}  // namespace ipdm_coilcomp

extern "C" int ipdm_coilcomp_supported(int n_coils, int n_virtual) {
  return n_coils >= 1 && n_coils <= CC_MAX_COILS && n_virtual >= 1 && n_virtual <= n_coils && n_virtual <= CC_MAX_VIRTUAL;
}

extern "C" size_t ipdm_coilcomp_workspace_bytes(int B, int n_coils) {
  if (B <= 0 || n_coils < 1 || n_coils > CC_MAX_COILS || B > 65535) return 0;
  return (size_t)B * n_coils * n_coils * sizeof(float2);
}

extern "C" int ipdm_coil_gram_c64(const float* y, int ah, int aw, float* gram, int B, int n_coils, int H, int W, void* stream) {
  const int rc = gram_check(ah, aw, B, n_coils, H, W);
  if (rc) return rc;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && gram);
  return gram_launch(reinterpret_cast<const float2*>(y), ah, aw, reinterpret_cast<float2*>(gram), B, n_coils, H, W, ipdm_stream(stream));
}

extern "C" int ipdm_coilcomp_matrix_c64(const float* gram, const float* noise_cov, int n_virtual, float* A, float* eig,
                                        int32_t* status, int B, int n_coils, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && n_virtual > 0);
  if (!ipdm_coilcomp_supported(n_coils, n_virtual) || B > 65535) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(gram && A && status);
  return matrix_launch(reinterpret_cast<const float2*>(gram), reinterpret_cast<const float2*>(noise_cov), n_virtual,
                       reinterpret_cast<float2*>(A), eig, status, B, n_coils, ipdm_stream(stream));
}

extern "C" int ipdm_coil_apply_c64(const float* y, const float* A, int per_image, float* out, int B, int n_coils, int n_virtual,
                                   int64_t P, void* stream) {
  const int rc = apply_check(B, n_coils, n_virtual, P);
  if (rc) return rc;
  if (B == 0 || P == 0) return IPDM_OK;
  IPDM_REQUIRE(y && A && out);
  IPDM_REQUIRE(!overlaps(y, (size_t)n_coils * B * P * sizeof(float2), out, (size_t)n_virtual * B * P * sizeof(float2)));
  return apply_launch(reinterpret_cast<const float2*>(y), reinterpret_cast<const float2*>(A), per_image != 0,
                      reinterpret_cast<float2*>(out), B, n_coils, n_virtual, P, ipdm_stream(stream));
}

extern "C" int ipdm_coil_compress_c64(const float* y, int ah, int aw, int n_virtual, const float* noise_cov, float* A, float* eig,
                                      int32_t* status, float* out, float* work, int B, int n_coils, int H, int W, void* stream) {
  int rc = gram_check(ah, aw, B, n_coils, H, W);
  if (rc) return rc;
  IPDM_REQUIRE(n_virtual > 0);
  if (!ipdm_coilcomp_supported(n_coils, n_virtual)) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && A && status && out && work);
  const int64_t P = (int64_t)H * W;
  IPDM_REQUIRE(!overlaps(y, (size_t)n_coils * B * P * sizeof(float2), out, (size_t)n_virtual * B * P * sizeof(float2)));
  hipStream_t s = ipdm_stream(stream);
  const float2* yy = reinterpret_cast<const float2*>(y);
  float2* gram = reinterpret_cast<float2*>(work);
  rc = gram_launch(yy, ah, aw, gram, B, n_coils, H, W, s);
  if (rc) return rc;
  rc = matrix_launch(gram, reinterpret_cast<const float2*>(noise_cov), n_virtual, reinterpret_cast<float2*>(A), eig, status, B, n_coils,
                     s);
  if (rc) return rc;
  return apply_launch(yy, reinterpret_cast<const float2*>(A), 1, reinterpret_cast<float2*>(out), B, n_coils, n_virtual, P, s);
}
