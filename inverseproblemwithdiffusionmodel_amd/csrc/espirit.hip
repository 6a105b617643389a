// ESPIRiT coil sensitivity maps from the fully sampled calibration region of multi-coil k-space (Uecker 2014; DESIGN.md
// 4.4i).  Four launches, all asynchronous, no atomics (an image's bits do not depend on its batch):
//     Gram matrix of the calibration matrix (every k x k patch of the box, all coils), double  ->  eigendecomposition by
//     cyclic Hermitian Jacobi in double, sort, rank  ->  kernel correlation K [n][n][2k-1][2k-1] of the row space
//     ->  per pixel: G(x) = DFT of K's taps, power iteration, Rayleigh quotient, conj, coil-0 gauge, crop
// The M x M matrices (M = n k^2 up to 432) live in the global workspace: one workgroup of 1024 threads per image works
// on them in place, a round of the round-robin ordering being M / 2 disjoint rotations whose 2 x 2 blocks of G and column
// pairs of V each belong to one thread.  The pixel kernel is templated on a PADDED coil count (4, 8, 16) like
// csm_walsh_kernel: padded coils are zero rows and columns of G, every coil loop unrolls, no per-thread array is indexed at
// run time.  G(x) is the direct DFT of at most 15 x 15 taps, so the kernel serves every image size up to 1024 x 1024,
// whether or not the FFT kernels do.
#include "launch.h"

namespace {

constexpr int ESP_MAX_COILS = 16;
constexpr int ESP_MIN_K = 3, ESP_MAX_K = 8;
constexpr int ESP_MAX_M = 432;                  // n k^2: 12 coils at k = 6, 16 at k = 5 (the Jacobi stage grows as M^3: DESIGN.md 4.4i)
constexpr int ESP_MAX_SIDE = 1024;
constexpr int ESP_GRAM_THREADS = 256;
constexpr int ESP_GRAM_CHUNK = 8;               // patches staged per pass: [M][CHUNK + 1] float2, 30.4 KiB at M = 432
constexpr int ESP_EIG_THREADS = 1024;
constexpr int ESP_BLK_ILP = 2, ESP_COL_ILP = 2;    // items of a Jacobi round whose loads a thread keeps in flight
constexpr int ESP_SWEEPS = 60;                  // sweep cap (the test cases converge after 9..25)
constexpr double ESP_OFF_TOL2 = 1.0e-24;        // stop when a sweep met off(G)^2 <= tol^2 ||G||_F^2, tol = 1e-12
constexpr double ESP_ROT_SKIP = 2.0e-16;        // |g_pq| of the matrix scaled to a largest diagonal entry in [0.5, 1): rounding
                                                // noise, no rotation (all M^2 / 2 of them move an eigenvalue by < 2e-13 lam_0)
constexpr int ESP_TILE = 8;                     // pixel tile side: 64 pixels, their G(x) in LDS
constexpr int ESP_PIX_THREADS = 256;
constexpr int ESP_MAX_TAPS = 2 * ESP_MAX_K - 1;
constexpr size_t ESP_LDS_MAX = 160 * 1024;
static_assert((size_t)ESP_TILE * ESP_TILE * (ESP_MAX_COILS * ESP_MAX_COILS + 1) * sizeof(float2) <= ESP_LDS_MAX - 4096,
              "the 16-coil tile of G(x) must fit one CU's LDS beside the twiddles");

struct cd { double x, y; };                     // complex double, 8-byte aligned

__device__ __forceinline__ cd cd_make(double x, double y) { cd r; r.x = x; r.y = y; return r; }
__device__ __forceinline__ cd cd_mul(cd a, cd b) { return cd_make(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cd cd_mulc(cd a, cd b) { return cd_make(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ float2 esp_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// ---- Gram matrix of the calibration matrix ---------------------------------------------------------------------------------
// Workgroup (blockIdx.x, b): pairs t = blockIdx.x * 256 + tid of the upper triangle (i <= j) of image b.  Column (c, ty, tx)
// of patch (py, px) is y_c(r0 + py + ty, c0 + px + tx); ESP_GRAM_CHUNK patches are staged at a time, consecutive patches
// (consecutive px) read consecutive k-space samples.  Patches run in order, products and sums in double.
__global__ __launch_bounds__(ESP_GRAM_THREADS) void espirit_gram_kernel(const float2* __restrict__ y, cd* __restrict__ gram, int B,
                                                                        int n, int k, int H, int W, int ah, int aw) {
  __shared__ float2 smp[ESP_MAX_M * (ESP_GRAM_CHUNK + 1)];
  const int b = blockIdx.y;
  const int kk = k * k, M = n * kk;
  const int pw = 2 * aw + 1 - k + 1, np = (2 * ah + 1 - k + 1) * pw;
  const int r0 = H / 2 - ah, c0 = W / 2 - aw;
  const size_t HW = (size_t)H * W;
  const int npairs = M * (M + 1) / 2;
  const int t = blockIdx.x * ESP_GRAM_THREADS + threadIdx.x;
  int i = 0, j = 0;
  if (t < npairs) {
    int rem = t;
    while (rem >= M - i) { rem -= M - i; ++i; }
    j = i + rem;
  }
  double acc_re = 0.0, acc_im = 0.0;
  for (int p0 = 0; p0 < np; p0 += ESP_GRAM_CHUNK) {
    for (int idx = threadIdx.x; idx < M * ESP_GRAM_CHUNK; idx += ESP_GRAM_THREADS) {
      const int col = idx / ESP_GRAM_CHUNK, s = idx - col * ESP_GRAM_CHUNK;
      const int p = p0 + s;
      float2 v = make_float2(0.f, 0.f);
      if (p < np) {
        const int py = p / pw, px = p - py * pw;
        const int c = col / kk, rem = col - c * kk;
        const int ty = rem / k, tx = rem - ty * k;
        v = y[((size_t)c * B + b) * HW + (size_t)(r0 + py + ty) * W + (c0 + px + tx)];
      }
      smp[col * (ESP_GRAM_CHUNK + 1) + s] = v;
    }
    __syncthreads();
    if (t < npairs) {
      const float2* pi = smp + i * (ESP_GRAM_CHUNK + 1);
      const float2* pj = smp + j * (ESP_GRAM_CHUNK + 1);
#pragma unroll
      for (int s = 0; s < ESP_GRAM_CHUNK; ++s) {                 // patches past the last are zeros: they add exactly nothing
        const float2 a = pi[s], c = pj[s];                       // conj(a) c
        acc_re += (double)a.x * (double)c.x + (double)a.y * (double)c.y;
        acc_im += (double)a.x * (double)c.y - (double)a.y * (double)c.x;
      }
    }
    __syncthreads();
  }
  if (t < npairs) {
    cd* g = gram + (size_t)b * M * M;
    const double im = i == j ? 0.0 : acc_im;
    g[(size_t)i * M + j] = cd_make(acc_re, im);
    if (i != j) g[(size_t)j * M + i] = cd_make(acc_re, -im);
  }
}

// ---- eigendecomposition, sort, rank -------------------------------------------------------------------------------------------
struct EspRot { double c, sx, sy; int p, q; };   // J = [[c, s], [-conj(s), c]] on the (p, q) plane; s == 0: the identity

__device__ __forceinline__ void esp_pair(int m, int r, int k, int& p, int& q) {   // round-robin: m players (even), round r, table k
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

// one 2 x 2 block of G <- J^H G J: rows (p, q) of rotation k, columns (p, q) of rotation l
struct EspBlk { cd a, b, c, d; int k, l; bool act; };

__device__ __forceinline__ bool esp_identity(const EspRot& R) { return R.sx == 0.0 && R.sy == 0.0; }

__device__ __forceinline__ void esp_blk_load(const cd* G, const EspRot* rot, int e, int half, int M, EspBlk& w) {
  w.act = false;
  if (e >= half * half) return;
  w.k = e / half;
  w.l = e - w.k * half;
  const int kp = rot[w.k].p, kq = rot[w.k].q, lp = rot[w.l].p, lq = rot[w.l].q;
  if (esp_identity(rot[w.k]) && esp_identity(rot[w.l])) return;
  w.act = true;
  const cd z = cd_make(0.0, 0.0);
  const bool qk = kq < M, ql = lq < M;                           // the phantom player has no row and no column
  const size_t rp = (size_t)kp * M, rq = (size_t)kq * M;
  w.a = G[rp + lp];
  w.b = ql ? G[rp + lq] : z;
  w.c = qk ? G[rq + lp] : z;
  w.d = (qk && ql) ? G[rq + lq] : z;
}

__device__ __forceinline__ void esp_blk_finish(cd* G, const EspRot* rot, int M, const EspBlk& w) {
  if (!w.act) return;
  const EspRot Rk = rot[w.k], Rl = rot[w.l];
  const cd z = cd_make(0.0, 0.0);
  const cd sk = cd_make(Rk.sx, Rk.sy), sl = cd_make(Rl.sx, Rl.sy);
  // rows: new_p = c_k row_p - s_k row_q, new_q = conj(s_k) row_p + c_k row_q
  cd t0 = cd_mul(sk, w.c), t1 = cd_mul(sk, w.d);
  const cd a1 = cd_make(Rk.c * w.a.x - t0.x, Rk.c * w.a.y - t0.y), b1 = cd_make(Rk.c * w.b.x - t1.x, Rk.c * w.b.y - t1.y);
  t0 = cd_mulc(w.a, sk);
  t1 = cd_mulc(w.b, sk);
  const cd c1 = cd_make(t0.x + Rk.c * w.c.x, t0.y + Rk.c * w.c.y), d1 = cd_make(t1.x + Rk.c * w.d.x, t1.y + Rk.c * w.d.y);
  // columns: new_p = c_l col_p - col_q conj(s_l), new_q = col_p s_l + c_l col_q
  t0 = cd_mulc(b1, sl);
  t1 = cd_mulc(d1, sl);
  cd a = cd_make(Rl.c * a1.x - t0.x, Rl.c * a1.y - t0.y);
  cd c = cd_make(Rl.c * c1.x - t1.x, Rl.c * c1.y - t1.y);
  t0 = cd_mul(a1, sl);
  t1 = cd_mul(c1, sl);
  cd bb = cd_make(t0.x + Rl.c * b1.x, t0.y + Rl.c * b1.y);
  cd d = cd_make(t1.x + Rl.c * d1.x, t1.y + Rl.c * d1.y);
  if (w.k == w.l) {                                              // the rotated pair is zero by construction, the diagonal real
    a.y = 0.0;
    d.y = 0.0;
    bb = z;
    c = z;
  }
  const bool qk = Rk.q < M, ql = Rl.q < M;
  const size_t rp = (size_t)Rk.p * M, rq = (size_t)Rk.q * M;
  G[rp + Rl.p] = a;
  if (ql) G[rp + Rl.q] = bb;
  if (qk) G[rq + Rl.p] = c;
  if (qk && ql) G[rq + Rl.q] = d;
}

// one row of V <- V J for one rotation (a rotation that is not the identity has a real q)
struct EspCol { cd vp, vq; int i, k; bool act; };

__device__ __forceinline__ void esp_col_load(const cd* V, const EspRot* rot, int e, int half, int M, EspCol& w) {
  w.act = false;
  if (e >= M * half) return;
  w.i = e / half;
  w.k = e - w.i * half;
  if (esp_identity(rot[w.k])) return;
  w.act = true;
  const size_t row = (size_t)w.i * M;
  w.vp = V[row + rot[w.k].p];
  w.vq = V[row + rot[w.k].q];
}

__device__ __forceinline__ void esp_col_finish(cd* V, const EspRot* rot, int M, const EspCol& w) {
  if (!w.act) return;
  const EspRot R = rot[w.k];
  const cd s = cd_make(R.sx, R.sy);
  const size_t row = (size_t)w.i * M;
  cd t = cd_mulc(w.vq, s);
  V[row + R.p] = cd_make(R.c * w.vp.x - t.x, R.c * w.vp.y - t.y);
  t = cd_mul(w.vp, s);
  V[row + R.q] = cd_make(t.x + R.c * w.vq.x, t.y + R.c * w.vq.y);
}

// sum / maximum over the workgroup, the same value (added in the same order) in every thread
__device__ __forceinline__ double esp_block_sum(double v, double* red) {
  v = ipdm_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < ESP_EIG_THREADS / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double esp_block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < ESP_EIG_THREADS / 64; ++w) s = fmax(s, red[w]);
  __syncthreads();
  return s;
}

// One workgroup per image.  G (the Gram matrix on entry) and V are [M][M] complex double in global memory, written and read
// by this workgroup alone, a barrier between every phase.  On exit the first `rank` rows of G hold the kept eigenvectors
// TRANSPOSED and sorted, Vs[i][row] = V[row][perm[i]]: what espirit_corr_kernel walks.
__global__ __launch_bounds__(ESP_EIG_THREADS) void espirit_eig_kernel(cd* gram, cd* vws, double* __restrict__ lam_out,
                                                                      int32_t* __restrict__ rank_out, int32_t* __restrict__ status_out,
                                                                      int32_t* __restrict__ sweeps_out, int M, double sv_thresh) {
  __shared__ EspRot rot[ESP_MAX_M / 2];
  __shared__ double lam[ESP_MAX_M];
  __shared__ double lams[ESP_MAX_M];
  __shared__ int perm[ESP_MAX_M];
  __shared__ double red[ESP_EIG_THREADS / 64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int MM = M * M;
  cd* G = gram + (size_t)b * MM;
  cd* V = vws + (size_t)b * MM;

  // G <- G / 2^e, 2^e the power of two at or above the largest diagonal entry: an exact scaling, undone on the eigenvalues
  double dmax = 0.0, nonfinite = 0.0;
  for (int e = tid; e < MM; e += ESP_EIG_THREADS) {
    const cd v = G[e];
    if (!(fabs(v.x) < INFINITY) || !(fabs(v.y) < INFINITY)) nonfinite += 1.0;
    const int i = e / M;
    if (e - i * M == i) dmax = fmax(dmax, fabs(v.x));
  }
  dmax = esp_block_max(dmax, red);
  nonfinite = esp_block_sum(nonfinite, red);
  int ex = 0;
  if (dmax > 0.0 && dmax < INFINITY) frexp(dmax, &ex);
  ex = ex < -1000 ? -1000 : ex > 1000 ? 1000 : ex;
  const double down = ldexp(1.0, -ex);
  double fro2 = 0.0;
  for (int e = tid; e < MM; e += ESP_EIG_THREADS) {
    const int i = e / M, j = e - i * M;
    const cd v = G[e];
    const cd w = cd_make(v.x * down, v.y * down);
    fro2 += w.x * w.x + w.y * w.y;
    G[e] = w;
    V[e] = cd_make(i == j ? 1.0 : 0.0, 0.0);
  }
  fro2 = esp_block_sum(fro2, red);                               // (its barriers order the stores above before the first round)

  // cyclic Jacobi, round-robin ordering: m - 1 rounds of m / 2 disjoint rotations per sweep
  const int m = M + (M & 1), half = m / 2;
  bool converged = !(nonfinite > 0.0) && !(fro2 > 0.0);          // the zero matrix is its own decomposition
  int sweeps = 0;
  if (!(nonfinite > 0.0) && fro2 > 0.0 && fro2 < INFINITY) {
    for (int sw = 0; sw < ESP_SWEEPS && !converged; ++sw) {
      double off2 = 0.0;
      for (int r = 0; r < m - 1; ++r) {
        if (tid < half) {
          EspRot R;
          esp_pair(m, r, tid, R.p, R.q);
          R.c = 1.0;
          R.sx = 0.0;
          R.sy = 0.0;
          if (R.q < M) {                                         // the phantom player's pair keeps the identity
            const cd g = G[(size_t)R.p * M + R.q];
            const double mag = sqrt(g.x * g.x + g.y * g.y);
            off2 += 2.0 * mag * mag;
            if (mag > ESP_ROT_SKIP) {
              const double gap = G[(size_t)R.q * M + R.q].x - G[(size_t)R.p * M + R.p].x;
              const double tau = gap / (2.0 * mag);
              double t;
              if (fabs(tau) > 1.0e150) t = 0.5 / tau;
              else t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
              R.c = 1.0 / sqrt(1.0 + t * t);
              const double s = t * R.c;
              R.sx = s * (g.x / mag);
              R.sy = s * (g.y / mag);
            }
          }
          rot[tid] = R;
        }
        __syncthreads();
        // G <- J^H G J, one 2 x 2 block (rows of rotation k, columns of rotation l) per item; V <- V J, one row and rotation
        // per item.  The loads of ESP_BLK_ILP (ESP_COL_ILP) items are issued before the first is finished; the stage is
        // bound by what one CU moves through L2 all the same (82 GB/s with one item or two in flight).
        for (int e0 = tid; e0 < half * half; e0 += ESP_BLK_ILP * ESP_EIG_THREADS) {
          EspBlk w[ESP_BLK_ILP];
#pragma unroll
          for (int u = 0; u < ESP_BLK_ILP; ++u) esp_blk_load(G, rot, e0 + u * ESP_EIG_THREADS, half, M, w[u]);
#pragma unroll
          for (int u = 0; u < ESP_BLK_ILP; ++u) esp_blk_finish(G, rot, M, w[u]);
        }
        for (int e0 = tid; e0 < M * half; e0 += ESP_COL_ILP * ESP_EIG_THREADS) {
          EspCol w[ESP_COL_ILP];
#pragma unroll
          for (int u = 0; u < ESP_COL_ILP; ++u) esp_col_load(V, rot, e0 + u * ESP_EIG_THREADS, half, M, w[u]);
#pragma unroll
          for (int u = 0; u < ESP_COL_ILP; ++u) esp_col_finish(V, rot, M, w[u]);
        }
        __syncthreads();
      }
      off2 = esp_block_sum(off2, red);                           // the same sum in every thread: the test is uniform
      sweeps = sw + 1;
      converged = off2 <= ESP_OFF_TOL2 * fro2;
    }
  }

  // sort: descending, equal eigenvalues keep the lower original index first
  double mine = 0.0;
  if (tid < M) {
    mine = G[(size_t)tid * M + tid].x;
    lam[tid] = mine;
  }
  const double notfinite = esp_block_sum(tid < M && !(fabs(mine) < INFINITY) ? 1.0 : 0.0, red);
  const bool ok = converged && !(notfinite > 0.0);               // uniform
  if (!ok) {                                                     // K and the maps of this image are zeros
    for (int i = tid; i < M; i += ESP_EIG_THREADS) lam_out[(size_t)b * M + i] = 0.0;
    if (tid == 0) {
      rank_out[b] = 0;
      status_out[b] = 1;
      if (sweeps_out) sweeps_out[b] = sweeps;
    }
    return;
  }
  if (tid < M) {
    int rank = 0;
    for (int j = 0; j < M; ++j) {
      const double o = lam[j];
      rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
    }
    perm[rank] = tid;
    const double l = ldexp(mine, ex);
    lams[rank] = l;
    lam_out[(size_t)b * M + rank] = l;
  }
  __syncthreads();
  // rank = #{sigma_i > sv_thresh sigma_0}, sigma = sqrt(max(lambda, 0))
  const double s0 = sqrt(fmax(lams[0], 0.0));
  const double kept = esp_block_sum(tid < M && sqrt(fmax(lams[tid], 0.0)) > sv_thresh * s0 ? 1.0 : 0.0, red);
  const int rank = (int)kept;
  for (int e = tid; e < rank * M; e += ESP_EIG_THREADS) {        // (the diagonal of G was read before the barriers above)
    const int i = e / M, row = e - i * M;
    G[e] = V[(size_t)row * M + perm[i]];
  }
  if (tid == 0) {
    rank_out[b] = rank;
    status_out[b] = 0;
    if (sweeps_out) sweeps_out[b] = sweeps;
  }
}

// ---- kernel correlation ---------------------------------------------------------------------------------------------------------
// K[c][c2][dy][dx] = sum over t - t2 = d of P[(c, t)][(c2, t2)], P = sum_{i < rank} v_i v_i^H, formed from the rows of Vs
// without P.  One output per thread, dx fastest, so neighbouring threads read neighbouring entries of a row of Vs.  Sums in
// double (columns outermost, taps in (ty, tx) order), rounded once.
__global__ __launch_bounds__(256) void espirit_corr_kernel(const cd* __restrict__ vs, const int32_t* __restrict__ rank,
                                                           const int32_t* __restrict__ status, float2* __restrict__ K, int n, int k) {
  const int b = blockIdx.y;
  const int side = 2 * k - 1, kk = k * k, M = n * kk;
  const int total = n * n * side * side;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  float2 out = make_float2(0.f, 0.f);
  if (status[b] == 0) {
    const int dx = o % side, dy = (o / side) % side;
    const int c2 = (o / (side * side)) % n, c = o / (side * side * n);
    const int ddy = dy - (k - 1), ddx = dx - (k - 1);            // t - t2
    const int ty0 = ddy > 0 ? ddy : 0, ty1 = ddy < 0 ? k + ddy : k;
    const int tx0 = ddx > 0 ? ddx : 0, tx1 = ddx < 0 ? k + ddx : k;
    const cd* V = vs + (size_t)b * M * M;
    const int r = rank[b];
    double re = 0.0, im = 0.0;
    for (int i = 0; i < r; ++i) {
      const cd* row = V + (size_t)i * M;
      for (int ty = ty0; ty < ty1; ++ty) {
        for (int tx = tx0; tx < tx1; ++tx) {
          const cd a = row[c * kk + ty * k + tx], bq = row[c2 * kk + (ty - ddy) * k + (tx - ddx)];
          re += a.x * bq.x + a.y * bq.y;                         // a conj(bq)
          im += a.y * bq.x - a.x * bq.y;
        }
      }
    }
    out = make_float2((float)re, (float)im);
  }
  K[(size_t)b * total + o] = out;
}

// ---- per pixel ----------------------------------------------------------------------------------------------------------------
// One workgroup: one 8 x 8 tile of image b.  Phase 1, all 256 threads: G(x)[c][c2] = (1 / k^2) sum_d K[c][c2][d] Ey[xr][dy]
// Ex[xc][dx] for the 64 pixels, separably -- a thread owns a pair (c, c2) and XCP of the tile's columns, reads each tap once,
// keeps t[xc] = sum_dx K Ex and the 8 x XCP results in registers (compile-time indices only); the twiddles of the tile's 8
// rows and 8 columns sit in LDS and are read as broadcasts.  G goes to LDS as [pixel][NC * NC + 1] float2: the odd stride
// spreads the 64 pixels of phase 2 over the banks.  Phase 2, one thread per pixel: power iteration with u in registers.
template <int NC>
__global__ __launch_bounds__(ESP_PIX_THREADS) void espirit_pixel_kernel(const float2* __restrict__ K, const int32_t* __restrict__ status,
                                                                        float2* __restrict__ maps, float* __restrict__ eigval, int B,
                                                                        int n, int k, int H, int W, int power_iters, float crop,
                                                                        int tiles_w) {
  extern __shared__ __align__(16) unsigned char esp_smem[];
  __shared__ float2 Ey[ESP_TILE * ESP_MAX_TAPS], Ex[ESP_TILE * ESP_MAX_TAPS];
  constexpr int PAIRS = NC * NC, LD = PAIRS + 1;
  constexpr int XCP = NC == 16 ? 4 : NC == 8 ? 2 : 1, SLICES = ESP_TILE / XCP;
  float2* Gt = reinterpret_cast<float2*>(esp_smem);
  const int b = blockIdx.y;
  const int th = blockIdx.x / tiles_w, tw = blockIdx.x - th * tiles_w;
  const int r0 = th * ESP_TILE, c0 = tw * ESP_TILE;
  const int side = 2 * k - 1;
  const size_t HW = (size_t)H * W;
  const int tid = threadIdx.x;
  const int ly = tid / ESP_TILE, lx = tid - ly * ESP_TILE;
  const int pr = r0 + ly, pc = c0 + lx;
  const bool mine = tid < ESP_TILE * ESP_TILE && pr < H && pc < W;
  if (status != nullptr && status[b] != 0) {                     // (uniform) a failed decomposition: zeros
    if (mine) {
      const size_t e = (size_t)pr * W + pc;
      for (int j = 0; j < n; ++j) maps[((size_t)j * B + b) * HW + e] = make_float2(0.f, 0.f);
      if (eigval) eigval[(size_t)b * HW + e] = 0.f;
    }
    return;
  }
  // exp(-2 pi i d (x - N/2) / N), the product reduced mod N in integers
  for (int i = tid; i < 2 * ESP_TILE * side; i += ESP_PIX_THREADS) {
    const int which = i / (ESP_TILE * side), rem = i - which * (ESP_TILE * side);
    const int x = rem / side, d = rem - x * side - (k - 1);
    const int N = which ? W : H, pos = (which ? c0 : r0) + x;
    int mth = (d * (pos - N / 2)) % N;
    if (mth < 0) mth += N;
    float s, c;
    sincospif(2.f * ((float)mth / (float)N), &s, &c);
    (which ? Ex : Ey)[x * side + (d + k - 1)] = make_float2(c, -s);
  }
  __syncthreads();
  const float scale = (float)(k * k);
  for (int item = tid; item < PAIRS * SLICES; item += ESP_PIX_THREADS) {
    const int sl = item / PAIRS, pair = item - sl * PAIRS;
    const int c = pair / NC, c2 = pair - c * NC;
    float2 acc[ESP_TILE][XCP];
#pragma unroll
    for (int xr = 0; xr < ESP_TILE; ++xr)
#pragma unroll
      for (int j = 0; j < XCP; ++j) acc[xr][j] = make_float2(0.f, 0.f);
    if (c < n && c2 < n) {                                       // padded coils: zero rows and columns
      const float2* Kp = K + (((size_t)b * n + c) * n + c2) * side * side;
      const float2* ex = Ex + sl * XCP * side;
      for (int dy = 0; dy < side; ++dy) {
        float2 t[XCP];
#pragma unroll
        for (int j = 0; j < XCP; ++j) t[j] = make_float2(0.f, 0.f);
        for (int dx = 0; dx < side; ++dx) {
          const float2 kv = Kp[dy * side + dx];
#pragma unroll
          for (int j = 0; j < XCP; ++j) {
            const float2 p = esp_mul(kv, ex[j * side + dx]);
            t[j] = make_float2(t[j].x + p.x, t[j].y + p.y);
          }
        }
#pragma unroll
        for (int xr = 0; xr < ESP_TILE; ++xr) {
          const float2 ey = Ey[xr * side + dy];
#pragma unroll
          for (int j = 0; j < XCP; ++j) {
            const float2 p = esp_mul(ey, t[j]);
            acc[xr][j] = make_float2(acc[xr][j].x + p.x, acc[xr][j].y + p.y);
          }
        }
      }
    }
#pragma unroll
    for (int xr = 0; xr < ESP_TILE; ++xr)
#pragma unroll
      for (int j = 0; j < XCP; ++j)
        Gt[(xr * ESP_TILE + sl * XCP + j) * LD + pair] = make_float2(acc[xr][j].x / scale, acc[xr][j].y / scale);
  }
  __syncthreads();
  if (!mine) return;                                             // (no barrier follows)
  const float2* Gp = Gt + tid * LD;
  float2 u[NC], acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) u[j] = make_float2(1.f, 0.f);
  for (int it = 0; it <= power_iters + 1; ++it) {                // u0 = normalise(G 1), power_iters more, then G u once more
    asm volatile("" ::: "memory");                               // G is re-read from LDS every pass: 2 NC^2 registers would spill
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      float2 a = make_float2(0.f, 0.f);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const float2 p = esp_mul(Gp[i * NC + j], u[j]);
        a = make_float2(a.x + p.x, a.y + p.y);
      }
      acc[i] = a;
    }
    if (it == power_iters + 1) break;                            // acc = G u of the final u: the Rayleigh quotient's
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) s += acc[j].x * acc[j].x + acc[j].y * acc[j].y;
    const float nrm = sqrtf(s);
    const float inv = nrm > 0.f ? 1.f / nrm : 1.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) u[j] = make_float2(acc[j].x * inv, acc[j].y * inv);
  }
  float ev = 0.f;                                                // Re(u^H G u)
#pragma unroll
  for (int j = 0; j < NC; ++j) ev += u[j].x * acc[j].x + u[j].y * acc[j].y;
  const size_t e = (size_t)pr * W + pc;
  if (eigval) eigval[(size_t)b * HW + e] = ev;
  const bool keep = ev > crop;
  // map = conj(u), turned so that coil 0 is real and non-negative: conj(u_j) u_0 / |u_0|
  const float mag = sqrtf(u[0].x * u[0].x + u[0].y * u[0].y);
  float2 ph = make_float2(1.f, 0.f);
  if (mag > 0.f) ph = make_float2(u[0].x / mag, u[0].y / mag);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    if (j < n) {
      float2 v = make_float2(0.f, 0.f);
      if (keep) v = (j == 0 && mag > 0.f) ? make_float2(mag, 0.f) : esp_mul(make_float2(u[j].x, -u[j].y), ph);
      maps[((size_t)j * B + b) * HW + e] = v;
    }
  }
}

static inline bool esp_box_ok(int a, int N) { return a >= 0 && N / 2 - a >= 0 && N / 2 + a <= N - 1; }
static inline int esp_padded(int n_coils) { return n_coils <= 4 ? 4 : n_coils <= 8 ? 8 : 16; }
static inline bool esp_kernel_ok(int n_coils, int ksize) {
  return n_coils >= 1 && n_coils <= ESP_MAX_COILS && ksize >= ESP_MIN_K && ksize <= ESP_MAX_K && n_coils * ksize * ksize <= ESP_MAX_M;
}

// the checks of the entries that read y: IPDM_EINVAL first, then the sizes without a kernel
static int esp_check(int ah, int aw, int ksize, int B, int n_coils, int H, int W) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && ksize > 0 && H > 0 && W > 0 && esp_box_ok(ah, H) && esp_box_ok(aw, W));
  IPDM_REQUIRE(2 * ah + 1 >= ksize && 2 * aw + 1 >= ksize);
  if (!ipdm_espirit_supported(n_coils, ksize, H, W) || B > 65535) return IPDM_EUNSUPPORTED;
  return IPDM_OK;
}

static int gram_launch(const float2* y, int ah, int aw, int ksize, cd* gram, int B, int n, int H, int W, hipStream_t s) {
  const int M = n * ksize * ksize, npairs = M * (M + 1) / 2;
  hipLaunchKernelGGL(espirit_gram_kernel, dim3((npairs + ESP_GRAM_THREADS - 1) / ESP_GRAM_THREADS, B), dim3(ESP_GRAM_THREADS), 0, s, y,
                     gram, B, n, ksize, H, W, ah, aw);
  return ipdm_launch_status();
}

static int kernels_launch(cd* gram, cd* vws, int ksize, double sv_thresh, float2* K, double* lam, int32_t* rank, int32_t* status,
                          int32_t* sweeps, int B, int n, hipStream_t s) {
  const int M = n * ksize * ksize, side = 2 * ksize - 1;
  hipLaunchKernelGGL(espirit_eig_kernel, dim3(B), dim3(ESP_EIG_THREADS), 0, s, gram, vws, lam, rank, status, sweeps, M, sv_thresh);
  int rc = ipdm_launch_status();
  if (rc) return rc;
  const int total = n * n * side * side;
  hipLaunchKernelGGL(espirit_corr_kernel, dim3((total + 255) / 256, B), dim3(256), 0, s, gram, rank, status, K, n, ksize);
  return ipdm_launch_status();
}

template <int NC>
static int launch_pixel(const float2* K, const int32_t* status, float2* maps, float* eigval, int B, int n, int ksize, int H, int W,
                        int power_iters, float crop, hipStream_t s) {
  const size_t lds = (size_t)ESP_TILE * ESP_TILE * (NC * NC + 1) * sizeof(float2);
  const int tiles_h = (H + ESP_TILE - 1) / ESP_TILE, tiles_w = (W + ESP_TILE - 1) / ESP_TILE;
  return ipdm_launch_lds(espirit_pixel_kernel<NC>, dim3(tiles_h * tiles_w, B), dim3(ESP_PIX_THREADS), lds, s, K, status, maps, eigval, B,
                         n, ksize, H, W, power_iters, crop, tiles_w);
}

static int pixel_launch(const float2* K, const int32_t* status, float2* maps, float* eigval, int B, int n, int ksize, int H, int W,
                        int power_iters, float crop, hipStream_t s) {
  switch (esp_padded(n)) {
    case 4: return launch_pixel<4>(K, status, maps, eigval, B, n, ksize, H, W, power_iters, crop, s);
    case 8: return launch_pixel<8>(K, status, maps, eigval, B, n, ksize, H, W, power_iters, crop, s);
    default: return launch_pixel<16>(K, status, maps, eigval, B, n, ksize, H, W, power_iters, crop, s);
  }
}

}  // namespace

extern "C" int ipdm_espirit_supported(int n_coils, int ksize, int H, int W) {
  return esp_kernel_ok(n_coils, ksize) && H >= 1 && W >= 1 && H <= ESP_MAX_SIDE && W <= ESP_MAX_SIDE;
}

extern "C" size_t ipdm_espirit_workspace_bytes(int B, int n_coils, int ksize) {
  if (B <= 0 || B > 65535 || !esp_kernel_ok(n_coils, ksize)) return 0;
  const size_t M = (size_t)n_coils * ksize * ksize;
  return (size_t)B * 2 * M * M * sizeof(cd);
}

extern "C" int ipdm_espirit_gram_c64(const float* y, int ah, int aw, int ksize, double* gram, int B, int n_coils, int H, int W,
                                     void* stream) {
  const int rc = esp_check(ah, aw, ksize, B, n_coils, H, W);
  if (rc) return rc;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && gram);
  return gram_launch(reinterpret_cast<const float2*>(y), ah, aw, ksize, reinterpret_cast<cd*>(gram), B, n_coils, H, W, ipdm_stream(stream));
}

extern "C" int ipdm_espirit_kernels_c64(const float* y, int ah, int aw, int ksize, double sv_thresh, float* K, double* lam,
                                        int32_t* rank, int32_t* status, int32_t* sweeps, double* work, int B, int n_coils, int H,
                                        int W, void* stream) {
  IPDM_REQUIRE(sv_thresh >= 0.0 && sv_thresh < 1.0);                          // NaN fails
  int rc = esp_check(ah, aw, ksize, B, n_coils, H, W);
  if (rc) return rc;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && K && lam && rank && status && work);
  hipStream_t s = ipdm_stream(stream);
  const size_t M = (size_t)n_coils * ksize * ksize;
  cd* gram = reinterpret_cast<cd*>(work);
  cd* vws = gram + (size_t)B * M * M;
  rc = gram_launch(reinterpret_cast<const float2*>(y), ah, aw, ksize, gram, B, n_coils, H, W, s);
  if (rc) return rc;
  return kernels_launch(gram, vws, ksize, sv_thresh, reinterpret_cast<float2*>(K), lam, rank, status, sweeps, B, n_coils, s);
}

extern "C" int ipdm_espirit_pixel_c64(const float* K, const int32_t* status, int ksize, float crop, int power_iters, float* maps,
                                      float* eigval, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && ksize > 0 && H > 0 && W > 0 && power_iters >= 0 && crop == crop);
  if (!ipdm_espirit_supported(n_coils, ksize, H, W) || B > 65535) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(K && maps);
  return pixel_launch(reinterpret_cast<const float2*>(K), status, reinterpret_cast<float2*>(maps), eigval, B, n_coils, ksize, H, W,
                      power_iters, crop, ipdm_stream(stream));
}

extern "C" int ipdm_espirit_c64(const float* y, int ah, int aw, int ksize, double sv_thresh, float crop, int power_iters, float* maps,
                                float* eigval, float* K, double* lam, int32_t* rank, int32_t* status, double* work, int B,
                                int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(power_iters >= 0 && crop == crop);
  const int rc = ipdm_espirit_kernels_c64(y, ah, aw, ksize, sv_thresh, K, lam, rank, status, nullptr, work, B, n_coils, H, W, stream);
  if (rc) return rc;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(maps);
  return pixel_launch(reinterpret_cast<const float2*>(K), status, reinterpret_cast<float2*>(maps), eigval, B, n_coils, ksize, H, W,
                      power_iters, crop, ipdm_stream(stream));
}
