// Shared device code of the k-space kernels (kspace.hip: whole image in one CU's LDS; kspace_large.hip: row / column
// passes for images beyond the LDS): mixed-radix (4/2, then 3, then 5) Stockham FFT over lines held in LDS, the served
// sizes, sign and mask helpers.
#pragma once
#include <type_traits>
#include "launch.h"

namespace ipdm_kspace {

constexpr int FFT_THREADS = 1024;
constexpr int FFT_MAX_ELEMS = 16384;           // 128 KiB of float2
constexpr int FFT_EPT = FFT_MAX_ELEMS / FFT_THREADS;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// LDS image + twiddle table.  tw[q] = exp(-2*pi*i*q/twN); twN is a common multiple of every line length transformed with
// the table: lcm(H, W) for a whole image (max(H, W) when one side divides the other, as with powers of two), the line
// length for a strip.  A stage's phase k*t/(Ns*R) is then the exact table index k*t*twN/(Ns*R): Ns*R divides the line
// length, and k < Ns, t < R keeps the index below twN.
struct FftLds {
  float2* buf;
  float2* tw;
  int twN;
};

__device__ __forceinline__ void fft_make_twiddles(const FftLds& L) {
  for (int q = threadIdx.x; q < L.twN; q += blockDim.x) {
    double s, c;
    sincospi(-2.0 * (double)q / (double)L.twN, &s, &c);
    L.tw[q] = make_float2((float)c, (float)s);
  }
}

// One in-place Stockham stage of radix R over `nlines` lines of length N.
//   element (line, n) lives at buf[line*ls + n*es];  lines_fast: consecutive threads -> consecutive lines.
// Every thread reads all its butterflies, the workgroup barriers, then everyone writes.
// MIXED (here and below): the line length may hold factors 3 and 5.  It is a template flag, chosen at launch, because the
// power-of-two kernels must keep their code: with the radix-3 / 5 stages behind a run-time branch they took 6 to 10 more
// VGPRs and the kernels at the 128-VGPR cap three times the scratch.  MIXED = false is the code they always had.
template <int R, bool MIXED>
__device__ __forceinline__ void fft_stage(const FftLds& L, int N, int Ns, int es, int ls, int nlines, bool lines_fast,
                                          bool inverse) {
  constexpr int BPT = FFT_EPT / R;             // butterflies per thread at the largest image
  const int nb = N / R;                        // butterflies per line
  const int total = nb * nlines;
  const int twstep = L.twN / (Ns * R);
  float2 v[BPT][R];
  int dst[BPT];
#pragma unroll
  for (int u = 0; u < BPT; ++u) {
    int i = threadIdx.x + u * FFT_THREADS;
    dst[u] = -1;
    if (i < total) {
      int line, j;
      if (lines_fast) { j = i / nlines; line = i - j * nlines; }
      else { line = i / nb; j = i - line * nb; }
      int k;                                     // j mod Ns; Ns is a power of two while the radix-4 / 2 stages run
      if constexpr (R == 2 || R == 4) k = j & (Ns - 1);
      else k = j % Ns;
      const int kt = k * twstep;                 // MIXED: the phase index of t = 1; k < Ns, so kt * t < twN (not a power of two)
      int base = line * ls;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        float2 x = L.buf[base + (j + t * nb) * es];
        if (t > 0) {
          float2 w = L.tw[MIXED ? kt * t : (k * t * twstep) & (L.twN - 1)];
          if (inverse) w.y = -w.y;
          x = cmul(x, w);
        }
        v[u][t] = x;
      }
      dst[u] = base + (((j - k) * R) + k) * es;
      if constexpr (R == 2) {
        float2 a = v[u][0], b = v[u][1];
        v[u][0] = make_float2(a.x + b.x, a.y + b.y);
        v[u][1] = make_float2(a.x - b.x, a.y - b.y);
      } else if constexpr (R == 3) {
        // X0 = a + (b + c);  X1, X2 = a - (b + c)/2 -+ i*sin(2pi/3)*(b - c)   (forward; the inverse swaps the two)
        constexpr float S3 = 0.86602540378443864676f;            // sqrt(3)/2
        float2 a = v[u][0], b = v[u][1], c = v[u][2];
        float2 t1 = make_float2(b.x + c.x, b.y + c.y);
        float2 t2 = make_float2(a.x - 0.5f * t1.x, a.y - 0.5f * t1.y);
        float2 t3 = make_float2(S3 * (b.x - c.x), S3 * (b.y - c.y));
        // forward: -i*t3 = (t3.y, -t3.x); inverse: +i*t3
        float2 jt = inverse ? make_float2(-t3.y, t3.x) : make_float2(t3.y, -t3.x);
        v[u][0] = make_float2(a.x + t1.x, a.y + t1.y);
        v[u][1] = make_float2(t2.x + jt.x, t2.y + jt.y);
        v[u][2] = make_float2(t2.x - jt.x, t2.y - jt.y);
      } else if constexpr (R == 5) {
        // with w = exp(-2pi*i/5):  X1, X4 = m1 -+ i*n1,  X2, X3 = m2 -+ i*n2   (forward; the inverse swaps each pair)
        constexpr float C1 = 0.30901699437494742410f;            // cos(2pi/5)
        constexpr float C2 = -0.80901699437494742410f;           // cos(4pi/5)
        constexpr float S1 = 0.95105651629515357212f;            // sin(2pi/5)
        constexpr float S2 = 0.58778525229247312917f;            // sin(4pi/5)
        float2 a = v[u][0], b = v[u][1], c = v[u][2], d = v[u][3], e = v[u][4];
        float2 t1 = make_float2(b.x + e.x, b.y + e.y), t3 = make_float2(b.x - e.x, b.y - e.y);
        float2 t2 = make_float2(c.x + d.x, c.y + d.y), t4 = make_float2(c.x - d.x, c.y - d.y);
        float2 m1 = make_float2(a.x + C1 * t1.x + C2 * t2.x, a.y + C1 * t1.y + C2 * t2.y);
        float2 m2 = make_float2(a.x + C2 * t1.x + C1 * t2.x, a.y + C2 * t1.y + C1 * t2.y);
        float2 n1 = make_float2(S1 * t3.x + S2 * t4.x, S1 * t3.y + S2 * t4.y);
        float2 n2 = make_float2(S2 * t3.x - S1 * t4.x, S2 * t3.y - S1 * t4.y);
        float2 j1 = inverse ? make_float2(-n1.y, n1.x) : make_float2(n1.y, -n1.x);
        float2 j2 = inverse ? make_float2(-n2.y, n2.x) : make_float2(n2.y, -n2.x);
        v[u][0] = make_float2(a.x + t1.x + t2.x, a.y + t1.y + t2.y);
        v[u][1] = make_float2(m1.x + j1.x, m1.y + j1.y);
        v[u][2] = make_float2(m2.x + j2.x, m2.y + j2.y);
        v[u][3] = make_float2(m2.x - j2.x, m2.y - j2.y);
        v[u][4] = make_float2(m1.x - j1.x, m1.y - j1.y);
      } else {
        float2 a = v[u][0], b = v[u][1], c = v[u][2], d = v[u][3];
        float2 apc = make_float2(a.x + c.x, a.y + c.y), amc = make_float2(a.x - c.x, a.y - c.y);
        float2 bpd = make_float2(b.x + d.x, b.y + d.y), bmd = make_float2(b.x - d.x, b.y - d.y);
        // forward: -i*(b-d) = (bmd.y, -bmd.x); inverse: +i*(b-d) = (-bmd.y, bmd.x)
        float2 jb = inverse ? make_float2(-bmd.y, bmd.x) : make_float2(bmd.y, -bmd.x);
        v[u][0] = make_float2(apc.x + bpd.x, apc.y + bpd.y);
        v[u][1] = make_float2(amc.x + jb.x, amc.y + jb.y);
        v[u][2] = make_float2(apc.x - bpd.x, apc.y - bpd.y);
        v[u][3] = make_float2(amc.x - jb.x, amc.y - jb.y);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < BPT; ++u) {
    if (dst[u] >= 0) {
#pragma unroll
      for (int t = 0; t < R; ++t) L.buf[dst[u] + t * Ns * es] = v[u][t];
    }
  }
  __syncthreads();
}

template <bool MIXED>
__device__ __forceinline__ void fft_lines(const FftLds& L, int N, int es, int ls, int nlines, bool lines_fast,
                                          bool inverse) {
  int Ns = 1;
  if constexpr (!MIXED) {
    while (Ns * 4 <= N) {
      fft_stage<4, false>(L, N, Ns, es, ls, nlines, lines_fast, inverse);
      Ns *= 4;
    }
    if (Ns < N) fft_stage<2, false>(L, N, Ns, es, ls, nlines, lines_fast, inverse);
  } else {
    // N = 2^a 3^b 5^c, factored here.  The radix-4 / 2 stages run first, so Ns is a power of two for all of them and their
    // index arithmetic is that of a power-of-two line; the radix-3 and radix-5 stages follow with Ns = 2^a 3^i (5^j).
    const int p2 = N & -N;                       // 2^a
    while (Ns * 4 <= p2) {
      fft_stage<4, true>(L, N, Ns, es, ls, nlines, lines_fast, inverse);
      Ns *= 4;
    }
    if (Ns < p2) {
      fft_stage<2, true>(L, N, Ns, es, ls, nlines, lines_fast, inverse);
      Ns *= 2;
    }
    while ((N / Ns) % 3 == 0) {
      fft_stage<3, true>(L, N, Ns, es, ls, nlines, lines_fast, inverse);
      Ns *= 3;
    }
    while (Ns < N) {
      fft_stage<5, true>(L, N, Ns, es, ls, nlines, lines_fast, inverse);
      Ns *= 5;
    }
  }
}

// plain (uncentred, unnormalised) 2-D FFT of buf[H][W]; caller applies the (-1)^(r+c) flips and 1/sqrt(HW).
template <bool MIXED>
__device__ __forceinline__ void fft2_lds(const FftLds& L, int H, int W, bool inverse) {
  fft_lines<MIXED>(L, W, 1, W, H, false, inverse);   // along rows
  fft_lines<MIXED>(L, H, W, 1, W, true, inverse);    // along columns
}

__device__ __forceinline__ float sign_rc(int r, int c) { return ((r + c) & 1) ? -1.f : 1.f; }

// Coil-map products, the only place they are written.  A map element is `float` (real maps, the reference's synthetic
// "exp" maps) or `float2` (interleaved complex64, measured maps); `g` is the real factor folded in with the map: the
// centring sign +-1 in sens_mul, sign / sqrt(HW) in sens_mul_conj.
//   sens_mul(v, g, S)      = (g S) v          forward:  S_c x
//   sens_mul_conj(v, g, S) = (g conj(S)) v    adjoint and proximal tail:  conj(S_c) F^-1[...]
// The real forms are the expressions the kernels have always used.  The complex forms fix the operation order (one
// rounded product, one fma per component), so every kernel form rounds alike whatever the compiler's contraction
// setting; with a zero imaginary part they give the real form's bits.
__device__ __forceinline__ float2 sens_mul(float2 v, float g, float s) {
  const float w = g * s;
  return make_float2(v.x * w, v.y * w);
}
__device__ __forceinline__ float2 sens_mul_conj(float2 v, float g, float s) {
  const float w = g * s;
  return make_float2(v.x * w, v.y * w);
}
__device__ __forceinline__ float2 sens_mul(float2 v, float g, float2 s) {
  const float wx = __fmul_rn(g, s.x), wy = __fmul_rn(g, s.y);
  return make_float2(fmaf(v.x, wx, -__fmul_rn(v.y, wy)), fmaf(v.x, wy, __fmul_rn(v.y, wx)));
}
__device__ __forceinline__ float2 sens_mul_conj(float2 v, float g, float2 s) {
  const float wx = __fmul_rn(g, s.x), wy = __fmul_rn(g, s.y);
  return make_float2(fmaf(v.x, wx, __fmul_rn(v.y, wy)), fmaf(v.y, wx, -__fmul_rn(v.x, wy)));
}

__host__ __device__ __forceinline__ bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// A side the FFT serves: a power of two from 4, or 2^a 3^b 5^c with a >= 4 (a multiple of 16: the (-1)^(r+c) folding of
// fftshift needs a multiple of 4, the score networks halve the image three times) between 16 and FFT_MAX_SIDE.
constexpr int FFT_MAX_SIDE = 2048;
__host__ __device__ __forceinline__ bool fft_side_ok(int n) {
  if (n < 4) return false;
  if (is_pow2(n)) return true;
  if (n % 16 != 0 || n > FFT_MAX_SIDE) return false;
  while (n % 2 == 0) n /= 2;
  while (n % 3 == 0) n /= 3;
  while (n % 5 == 0) n /= 5;
  return n == 1;
}
// length of the whole-image twiddle table: lcm(H, W)
__host__ __device__ __forceinline__ int fft_tw_len(int H, int W) {
  int a = H, b = W;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return H / a * W;
}
// fft_stage<R> gives a thread FFT_EPT / R butterflies, rounded down: 4 of radix 4, 8 of radix 2, 5 of radix 3, 3 of radix 5,
// i.e. 16384 elements per stage for the radix-4 / 2 stages and 15360 for the radix-3 / 5 ones.  An image of two sides that
// are multiples of 16 and that runs a radix-3 or radix-5 stage has H*W = 256 * m with m <= 64 holding a factor 3 or 5, so
// m <= 60 and H*W <= 15360: covered, with nothing to spare at 96x160.  A power-of-two side of 4 or 8 beside a mixed side
// escapes that argument in one pair, 8x2000 / 2000x8 (16000 pixels): lds_fft_ok refuses it, and as it is no larger than
// 16384 pixels large_ok does too -- the one pair of served sides without a kernel.  (A strip of the row / column path
// holds at most 8192 elements.)
constexpr int FFT_MAX_ELEMS_R35 = (FFT_EPT / 3) * 3 * FFT_THREADS;
static_assert(FFT_MAX_ELEMS_R35 == (FFT_EPT / 5) * 5 * FFT_THREADS && FFT_MAX_ELEMS_R35 == 15360, "radix-3 / 5 stage capacity");
// launch-time choice of the MIXED instantiation: f(std::false_type) for power-of-two lines, f(std::true_type) otherwise
template <class Fn>
static inline int fft_dispatch(bool mixed, Fn&& f) {
  return mixed ? f(std::true_type{}) : f(std::false_type{});
}
static inline bool fft_mixed(int H, int W) { return !(is_pow2(H) && is_pow2(W)); }
static inline size_t lds_bytes(int H, int W) { return ((size_t)H * W + (size_t)fft_tw_len(H, W)) * sizeof(float2); }
static inline bool lds_fft_ok(int H, int W) {
  if (!fft_side_ok(H) || !fft_side_ok(W) || (int64_t)H * W > FFT_MAX_ELEMS) return false;
  if (is_pow2(H) && is_pow2(W)) return true;
  // the first fails for 8x2000 / 2000x8 alone; the second holds for every pair (the most: 8x1920, 15360 + 1920 values, 135 KiB)
  return H * W <= FFT_MAX_ELEMS_R35 && lds_bytes(H, W) <= 160 * 1024;
}


// Sampling mask at k-space point (r, c) of image b, the only place the two layouts are told apart:
//   mask_t > 0   line mask  uint8 [mask_t][W]     (sampled columns; row r is not looked at)
//   mask_t < 0   2-D mask   uint8 [T][H][W], T = -mask_t
// One plane broadcasts over the batch, otherwise image b uses plane b % T.  A mask only selects: no arithmetic depends
// on the layout.
static inline bool mask_t_ok(int mask_t) { return mask_t != 0 && mask_t > -0x7fffffff; }
__device__ __forceinline__ bool mask_at(const uint8_t* mask, int mask_t, int b, int H, int W, int r, int c) {
  if (mask_t > 0) return mask[(size_t)(mask_t == 1 ? 0 : b % mask_t) * W + c] != 0;
  const int T = -mask_t;
  return mask[((size_t)(T == 1 ? 0 : b % T) * H + r) * W + c] != 0;
}

// whole-image LDS kernels (kspace.hip, kspace_cg.hip): the image followed by the twiddle table in dynamic LDS
#define FFT_LDS_SETUP(H, W, MIXED)                            \
  extern __shared__ __align__(16) unsigned char smem_raw[];  \
  FftLds L;                                                   \
  L.buf = reinterpret_cast<float2*>(smem_raw);               \
  L.tw = L.buf + (size_t)(H) * (W);                          \
  L.twN = (MIXED) ? fft_tw_len((H), (W)) : ((H) > (W) ? (H) : (W)); \
  fft_make_twiddles(L);

// ---- argument bundles, passed to kernels by value (like ConvArgs and the strip functors) ----------------------------------
// The fused tails' first phase.  g_re NULL: no Langevin phase (the plain proximals); n_re NULL: Philox noise.
struct LangevinArgs {
  const float *g_re, *g_im, *n_re, *n_im;
  float step, noise_scale;
  uint64_t seed;
  int64_t sample_offset, step_id;
  const ipdm_sched_t* sched;       // device schedule: overrides step / noise_scale / step_id and the coefficient
  int sched_stride;                // records between consecutive samples: 0 one shared record, 1 sample b reads sched[b]
};
constexpr LangevinArgs NO_LANGEVIN{};

// The measurement model.  SensT: the coil maps' element type, float or float2 (interleaved complex64).
template <typename SensT>
struct SenseProblem {
  const float2* y;                 // k-space data [n_coils][B][H][W]
  const SensT* sens;               // [sens_sets][n_coils][H][W], sens_at()
  const uint8_t* mask;             // mask_at()
  int mask_t, B, n_coils, H, W;
  int sens_sets;                   // S >= 1 map sets; image b reads set b % S (a stack of slices in one batch)
};
template <typename SensT>
static inline SenseProblem<SensT> sense_problem(const float* y, const float* sens, const uint8_t* mask, int mask_t, int B,
                                                int n_coils, int H, int W, int sens_sets = 1) {
  return {reinterpret_cast<const float2*>(y), reinterpret_cast<const SensT*>(sens), mask, mask_t, B, n_coils, H, W, sens_sets};
}
// The `_sets_` entry points take the maps' element type as a flag: f(SenseProblem<float2>) for complex64 maps, else <float>.
template <class Fn>
static inline int sens_dispatch(int sens_complex, const float* y, const float* sens, const uint8_t* mask, int mask_t, int B,
                                int n_coils, int H, int W, int sens_sets, Fn&& f) {
  return sens_complex ? f(sense_problem<float2>(y, sens, mask, mask_t, B, n_coils, H, W, sens_sets))
                      : f(sense_problem<float>(y, sens, mask, mask_t, B, n_coils, H, W, sens_sets));
}

// Coil maps of image b, the only place a map set is chosen: set b % sens_sets of [sens_sets][n_coils][H][W], the rule
// mask_at uses for mask planes (the two indices are independent).  One set serves every image with no modulo and the
// pointer unchanged.  b is a block index in every kernel, so this is uniform over the workgroup: it is taken once at the
// top of a kernel, never per element.  set_elems = n_coils * H * W.  sens NULL (single coil) stays NULL.
template <typename SensT>
__device__ __forceinline__ const SensT* sens_at(const SensT* sens, int sens_sets, int b, size_t set_elems) {
  return (sens_sets == 1 || !sens) ? sens : sens + (size_t)(b % sens_sets) * set_elems;
}

// The device schedule, the only place it is read: the coefficient alone, or with the Langevin scalars as well.  Sample b
// reads record b * stride (stride 0: one record shared by the batch).  b is a block index in every kernel, so the record's
// address is uniform over the workgroup and the reads stay scalar loads.
__device__ __forceinline__ float sched_coef(const ipdm_sched_t* __restrict__ sched, int stride, int b, float coef) {
  return sched ? sched[(size_t)b * stride].coef : coef;
}
__device__ __forceinline__ float sched_override(LangevinArgs& lg, int b, float coef) {
  const ipdm_sched_t* __restrict__ sched = lg.sched;
  if (sched) {
    sched += (size_t)b * lg.sched_stride;
    lg.step = sched->step;
    lg.noise_scale = sched->noise_scale;
    lg.step_id = sched->step_id;
    return sched->coef;
  }
  return coef;
}

// ---- the Langevin update, the only place it is written ---------------------------------------------------------------------
// Philox normals of quad q (elements 4q .. 4q+3) of sample b, keyed by (seed, global sample id, step, plane); plane 0 is
// the real part, plane 1 the imaginary part
__device__ __forceinline__ void langevin_quad(const LangevinArgs& lg, int b, int plane, uint32_t q, float (&n)[4]) {
  ipdm_philox_normal4(lg.seed, lg.sample_offset + b, lg.step_id, plane, q, n);
}
__device__ __forceinline__ float langevin_update(const LangevinArgs& lg, float x, float g, float n) {
  return x + lg.step * g + n * lg.noise_scale;
}
// z at element e of sample b, in registers: noise injected (n_re / n_im) or Philox.  Every workgroup of a sample forms the
// same z, which is what lets the coil-parallel tails recompute it instead of exchanging it.
__device__ __forceinline__ void langevin_value(const float* xr, const float* xi, const LangevinArgs& lg, int b, int HW, int e,
                                               float& zr, float& zi) {
  const float* __restrict__ g_re = lg.g_re;
  const float* __restrict__ g_im = lg.g_im;
  const float* __restrict__ n_re = lg.n_re;
  const float* __restrict__ n_im = lg.n_im;
  const size_t gi = (size_t)b * HW + e;
  float nr, ni;
  if (n_re) {
    nr = n_re[gi];
    ni = n_im[gi];
  } else {
    float q[4];
    langevin_quad(lg, b, 0, (uint32_t)(e >> 2), q);
    const int lane4 = e & 3;                                   // (selects written out: as a function they cost the packed math)
    nr = lane4 == 0 ? q[0] : lane4 == 1 ? q[1] : lane4 == 2 ? q[2] : q[3];
    langevin_quad(lg, b, 1, (uint32_t)(e >> 2), q);
    ni = lane4 == 0 ? q[0] : lane4 == 1 ? q[1] : lane4 == 2 ? q[2] : q[3];
  }
  zr = langevin_update(lg, xr[e], g_re[gi], nr);
  zi = langevin_update(lg, xi[e], g_im[gi], ni);
}

// masked k-space residual, re-modulated for the inverse transform: sign*(sign*scale*v - y) = scale*v - sign*y on the sampled
// points, 0 elsewhere.  sv = scale * v.  The pointer form reads y only where sampled; y NULL: y = 0, nothing is subtracted.
__device__ __forceinline__ float2 masked_residual(bool m, float2 sv, float sg, float2 yy) {
  return m ? make_float2(sv.x - sg * yy.x, sv.y - sg * yy.y) : make_float2(0.f, 0.f);
}
__device__ __forceinline__ float2 masked_residual(bool m, float2 sv, float sg, const float2* __restrict__ y) {
  if (!m) return make_float2(0.f, 0.f);
  return y ? masked_residual(true, sv, sg, *y) : sv;
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

// per-sample state of the conjugate-gradient proximal (kspace_cg.hip)
struct CgState {
  float rr;        // <r, r>
  float bb;        // |b|^2, b = z + a A^H y
  int iters;       // CG iterations done
  int frozen;      // 1: x is final
};

// Coil-parallel normal operator on images held in LDS (kspace.hip), workgroup (coil, b):
//     planes[b][coil] = conj(S_c) F^-1 M (F S_c v - y_c)
//   mode 0: v = p[b], y = 0, skipped for a sample with state[b].frozen;  mode 1: v = x;  mode 2: v = x + Langevin update
// Modes 1 and 2 return at once on a zero coefficient (planes are then not written).  planes overlaps no operand.
template <typename SensT>
int launch_normal_coils(int mode, const float* x_re, const float* x_im, const LangevinArgs& lg, float coef, const float2* p,
                        const CgState* state, const SenseProblem<SensT>& pb, float2* planes, hipStream_t st);

// argument checks shared by the entry points: sizes, then (after the B == 0 exit) the fused tails' pointers
template <typename SensT>
static inline bool dims_ok(const SenseProblem<SensT>& pb) {
  return pb.B >= 0 && pb.n_coils > 0 && pb.H > 0 && pb.W > 0 && mask_t_ok(pb.mask_t) && pb.sens_sets >= 1;
}
template <typename SensT>
static inline bool step_ptrs_ok(const float* x_re, const float* x_im, const LangevinArgs& lg, const SenseProblem<SensT>& pb) {
  return x_re && x_im && lg.g_re && lg.g_im && pb.y && pb.mask && (lg.n_re == nullptr) == (lg.n_im == nullptr);
}

// a record per sample needs records to read
static inline bool sched_stride_ok(const ipdm_sched_t* sched, int stride) { return stride == 0 || (stride == 1 && sched); }

// out-of-place entry points: z -> out, plane by plane, unless the caller passed the same plane
static inline int copy_planes(float* out_re, float* out_im, const float* z_re, const float* z_im, size_t n, hipStream_t st) {
  if (out_re != z_re && hipMemcpyAsync(out_re, z_re, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return (int)hipGetLastError();
  if (out_im != z_im && hipMemcpyAsync(out_im, z_im, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return (int)hipGetLastError();
  return IPDM_OK;
}

// Non-Cartesian SENSE: A^H W A is the Toeplitz operator of the real spectrum psf on the 2H x 2W grid.
struct ToepProblem {
  const float2* sens;              // complex64 [n_coils][H][W]; NULL (n_coils == 1): S = 1
  const float* psf;                // float32 [psf_sets][2H][2W]
  int B, n_coils, H, W;
  int psf_sets = 1;                // frames: image row b reads set b % psf_sets
};

}  // namespace ipdm_kspace

// row / column-pass operators for images of served sides beyond the LDS (kspace_large.hip)
namespace ipdm_kspace_large {
bool large_ok(int H, int W);
int64_t workspace_bytes(int B, int n_coils, int H, int W);
int fft2c(const float2* in, float2* out, int batch, int H, int W, int inverse, hipStream_t s);
// SensT: float (real maps) or float2 (interleaved complex64 maps); both are instantiated in kspace_large.hip
template <typename SensT>
int sense_forward(const float2* x, const ipdm_kspace::SenseProblem<SensT>& pb, float2* y, hipStream_t s);
// adjoint of pb.y (masked first when apply_mask) into x_out, or its root-sum-of-squares into ssos_out
template <typename SensT>
int sense_adjoint(const ipdm_kspace::SenseProblem<SensT>& pb, int apply_mask, float2* x_out, float* ssos_out, float2* ws,
                  hipStream_t s);
// Langevin (optional: lg.g_re) + data-consistency operator on planar x, in place.  pb.sens NULL: single coil; mode as ColsProx.
template <typename SensT>
int prox_step(float* x_re, float* x_im, const ipdm_kspace::LangevinArgs& lg, const ipdm_kspace::SenseProblem<SensT>& pb,
              float coef, int mode, float2* ws, hipStream_t s);
// the conjugate-gradient proximal's pieces (kspace_cg.hip).  langevin: the planar update x += step*g + noise_scale*n alone.
// normal_op: out[b] = A^H (A v - y) with v complex (xc) or planar (x_re, x_im; xc NULL) and pb.y NULL for A^H A v alone;
// ws holds n_coils*B images and out must not overlap it.
int langevin(float* x_re, float* x_im, const ipdm_kspace::LangevinArgs& lg, int B, int H, int W, hipStream_t s);
template <typename SensT>
int normal_op(const float2* xc, const float* x_re, const float* x_im, const ipdm_kspace::SenseProblem<SensT>& pb, float2* out,
              float2* ws, hipStream_t s);
// Toeplitz normal operator of a non-Cartesian trajectory on the strip passes, every served size (toeplitz_ok: the padded
// 2H x 2W grid is a size of ipdm_kspace_size_class):
//   out[b] = sum_c conj(S_c) crop(F^-1(psf . F(pad(S_c v))))  [- sub[b] when sub is given]
// v complex (vc) or planar (v_re, v_im; vc NULL); ws holds n_coils * B * H * 2W values and out must not overlap it.
bool toeplitz_ok(int H, int W);
int toeplitz_normal(const float2* vc, const float* v_re, const float* v_im, const ipdm_kspace::ToepProblem& tp, const float2* sub,
                    float2* out, float2* ws, hipStream_t s);
}  // namespace ipdm_kspace_large
