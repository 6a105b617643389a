// Non-Cartesian SENSE, the one-off transforms: an exact direct non-uniform DFT -- no gridding, no
// interpolation table, no approximation error -- run once per reconstruction for A^H y, for simulated measurements and for
// the Toeplitz kernel.  The per-iteration operator A^H W A is the Toeplitz chain of kspace_large.hip.
//   trajectory k [M][2] = (k_y, k_x), float64, cycles per field of view, |k_y| <= H/2, |k_x| <= W/2
//   forward   y[c,b,m] = (HW)^-1/2 sum_{r,col} S_c x[b] exp(-2 pi i (k_y (r - H/2)/H + k_x (col - W/2)/W))
//   adjoint   the conjugate transpose, samples weighted by w_m first
//   T[dr + H, dc + W] = sum_m w_m exp(+2 pi i (k_y dr/H + k_x dc/W)),   P = centred DFT of T / (HW)   (real)
// The phase is separable, so each axis gets a table of per-sample phasors exp(-2 pi i k (j - off)/N), formed from the
// float64 trajectory with sincospi in double (a float32 phase of hundreds of cycles would lose every digit).  The inner
// loops multiply table entries; all sums are double, in a fixed order, without atomics.
// Frame sets: traj [T][M][2] (weights [T][M]) holds one trajectory per frame and image row b reads frame
// b % T.  The tables are formed over the T*M samples at once; a row's workgroups tile the M samples of its own frame, from
// the frame's first sample, so every sum runs in the order the single-trajectory call has for that frame's trajectory.
#include "kspace_fft.h"

namespace {

using namespace ipdm_kspace;

constexpr int NC_THREADS = 256;
constexpr int NC_TILE = 64;                          // samples per forward workgroup: one per lane

// tab_s[j][M] (sample fastest) and, when asked for, tab_p[m][L] (position fastest) = exp(-2 pi i k[m][axis] (j - off) / N)
template <typename T2>
__global__ __launch_bounds__(NC_THREADS) void nc_phasor_kernel(const double* __restrict__ traj, int axis, int M, int L, int off,
                                                               int N, T2* tab_s, T2* tab_p) {
  const size_t total = (size_t)M * L;
  for (size_t i = (size_t)blockIdx.x * NC_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * NC_THREADS) {
    const int j = (int)(i / M), m = (int)(i - (size_t)j * M);
    double s, c;
    sincospi(-2.0 * traj[2 * (size_t)m + axis] * (double)(j - off) / (double)N, &s, &c);
    T2 v;
    v.x = c;
    v.y = s;
    tab_s[i] = v;
    if (tab_p) tab_p[(size_t)m * L + j] = v;
  }
}

// y[img][m] = scale * sum_r Ey[r][m] sum_col Ex[col][m] (S_c x)[r][col]; workgroup (sample tile, b, coil), lane = sample,
// the four waves take rows r = wave (mod 4) and their partial sums are added in wave order.  ey / ex hold sets * M samples
// per position; row b reads the M of frame b % sets
__global__ __launch_bounds__(NC_THREADS) void ndft_forward_kernel(const float2* __restrict__ x, const float2* __restrict__ sens,
                                                                  const float2* __restrict__ ey, const float2* __restrict__ ex,
                                                                  float2* __restrict__ y, int B, int M, int H, int W,
                                                                  int sets) {
  __shared__ double2 red[NC_THREADS / 64][NC_TILE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, coil = blockIdx.z;
  const int m = blockIdx.x * NC_TILE + lane;
  const int mc = m < M ? m : M - 1;                              // idle lanes read a valid sample and store nothing
  // sens given: x is [B][H][W] and coil picks the map; otherwise x is the coil image [n][B][H][W]
  const float2* __restrict__ img = x + ((sens ? (size_t)b : (size_t)coil * B + b) * H) * W;
  const float2* __restrict__ sm = sens ? sens + (size_t)coil * H * W : nullptr;
  const size_t Ms = (size_t)sets * M;                            // table row length; the frame's samples start at f0
  const size_t f0 = (size_t)(b % sets) * M;
  ey += f0;
  ex += f0;
  double ar = 0.0, ai = 0.0;
  for (int r = wave; r < H; r += NC_THREADS / 64) {
    double tr = 0.0, ti = 0.0;
    for (int c = 0; c < W; ++c) {
      float2 v = img[(size_t)r * W + c];
      if (sm) v = sens_mul(v, 1.f, sm[(size_t)r * W + c]);
      const float2 e = ex[(size_t)c * Ms + mc];
      const double vr = v.x, vi = v.y, er = e.x, ei = e.y;
      tr += er * vr - ei * vi;
      ti += er * vi + ei * vr;
    }
    const float2 e = ey[(size_t)r * Ms + mc];
    const double er = e.x, ei = e.y;
    ar += er * tr - ei * ti;
    ai += er * ti + ei * tr;
  }
  red[wave][lane] = make_double2(ar, ai);
  __syncthreads();
  if (threadIdx.x < NC_TILE && m < M) {
    double sr = red[0][lane].x, si = red[0][lane].y;
#pragma unroll
    for (int w = 1; w < NC_THREADS / 64; ++w) {
      sr += red[w][lane].x;
      si += red[w][lane].y;
    }
    const double scale = 1.0 / sqrt((double)H * (double)W);
    y[((size_t)coil * B + b) * M + m] = make_float2((float)(sr * scale), (float)(si * scale));
  }
}

// out[r][col] = scale * sum_m g_m conj(ty[r][m]) conj(tx[m][col]),  g_m = w_m y[m]  (y NULL: 1; w NULL: 1)
// workgroup (column tile, row, image); samples staged through LDS 256 at a time, summed in sample order.
// COMBINE: the image is sum_c conj(S_c) (coil image c), coils in order; otherwise one image per (coil, b).
// zero_edge: row 0 and column 0 are written as zero (the Toeplitz kernel's unused lag -N).
// wgt, ty, tx hold sets * M samples; image row b reads the M of frame b % sets, in sample order from the frame's first.
template <typename T2, bool COMBINE>
__global__ __launch_bounds__(NC_THREADS) void ndft_adjoint_kernel(const float2* __restrict__ y, const float* __restrict__ wgt,
                                                                  const float2* __restrict__ sens, const T2* __restrict__ ty,
                                                                  const T2* __restrict__ tx, float2* __restrict__ out, int B,
                                                                  int n_coils, int M, int Ly, int Lx, double scale,
                                                                  int zero_edge, int sets) {
  __shared__ double2 g[NC_THREADS];
  const int col = blockIdx.x * NC_THREADS + threadIdx.x, r = blockIdx.y;
  const int img = blockIdx.z;                                    // COMBINE: b; otherwise coil * B + b
  const int coils = COMBINE ? n_coils : 1;
  const size_t Ms = (size_t)sets * M;
  const size_t f0 = (size_t)((COMBINE ? img : img % B) % sets) * M;
  if (wgt) wgt += f0;
  ty += f0;
  tx += f0 * Lx;
  double tr = 0.0, ti = 0.0;
  for (int coil = 0; coil < coils; ++coil) {
    const float2* __restrict__ ys = !y ? nullptr : y + (COMBINE ? (size_t)coil * B + img : (size_t)img) * M;
    double ar = 0.0, ai = 0.0;
    for (int m0 = 0; m0 < M; m0 += NC_THREADS) {
      __syncthreads();
      const int mm = m0 + threadIdx.x;
      double2 gv = make_double2(0.0, 0.0);
      if (mm < M) {
        const double w = wgt ? (double)wgt[mm] : 1.0;
        const double yr = ys ? (double)ys[mm].x : 1.0, yi = ys ? (double)ys[mm].y : 0.0;
        const T2 e = ty[(size_t)r * Ms + mm];
        const double er = e.x, ei = -(double)e.y;                // conj
        gv = make_double2(w * (yr * er - yi * ei), w * (yr * ei + yi * er));
      }
      g[threadIdx.x] = gv;
      __syncthreads();
      if (col < Lx) {
        const int cnt = M - m0 < NC_THREADS ? M - m0 : NC_THREADS;
        for (int j = 0; j < cnt; ++j) {
          const T2 e = tx[(size_t)(m0 + j) * Lx + col];
          const double er = e.x, ei = -(double)e.y;
          const double2 gj = g[j];
          ar += gj.x * er - gj.y * ei;
          ai += gj.x * ei + gj.y * er;
        }
      }
    }
    ar *= scale;
    ai *= scale;
    if (COMBINE && sens && col < Lx) {                           // conj(S) * a
      const float2 sv = sens[((size_t)coil * Ly + r) * Lx + col];
      const double sr = sv.x, si = sv.y;
      tr += sr * ar + si * ai;
      ti += sr * ai - si * ar;
    } else {
      tr += ar;
      ti += ai;
    }
  }
  if (col < Lx) {
    if (zero_edge && (r == 0 || col == 0)) tr = ti = 0.0;
    out[((size_t)img * Ly + r) * Lx + col] = make_float2((float)tr, (float)ti);
  }
}

// P = Re(centred orthonormal FFT of T) * sqrt(4HW) / (HW)
__global__ __launch_bounds__(NC_THREADS) void psf_real_kernel(const float2* __restrict__ t, float* __restrict__ psf, size_t n,
                                                              float gain) {
  for (size_t i = (size_t)blockIdx.x * NC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * NC_THREADS) psf[i] = t[i].x * gain;
}

template <typename T2>
static int make_table(const double* traj, int axis, int M, int L, int off, int N, T2* tab_s, T2* tab_p, hipStream_t st) {
  hipLaunchKernelGGL(nc_phasor_kernel<T2>, dim3(ipdm_ew_grid((int64_t)M * L, NC_THREADS)), dim3(NC_THREADS), 0, st, traj, axis, M, L,
                     off, N, tab_s, tab_p);
  return ipdm_launch_status();
}

static inline bool nc_dims_ok(int B, int n_coils, int M, int H, int W) {
  return B >= 0 && n_coils > 0 && M > 0 && H > 0 && W > 0;
}
// grid limits of the one-off kernels: images on grid.y / grid.z
// frame sets: T >= 1 trajectories of M samples each, row b reads set b % T; the tables index T * M samples with int
static inline bool nc_sets_ok(int B, int sets) { return sets >= 1 && B % sets == 0; }
static inline bool nc_samples_ok(int sets, int M) { return (int64_t)sets * M <= INT32_MAX; }
static inline bool nc_grid_ok(int B, int n_coils, int H) { return B <= 65535 && n_coils <= 65535 && (int64_t)n_coils * B <= 65535 && 2 * H <= 65535; }

}  // namespace

extern "C" int ipdm_nc_supported(int H, int W) { return ipdm_kspace_large::toeplitz_ok(H, W) ? 1 : 0; }

// float2 tables: ey [H][M], ex [W][M], exp [M][W]
extern "C" int64_t ipdm_ndft_workspace_bytes(int M, int H, int W) {
  if (M <= 0 || H <= 0 || W <= 0) return 0;
  return ((int64_t)H + 2 * (int64_t)W) * M * (int64_t)sizeof(float2);
}

// float2 tables over the Mt = traj_sets * M samples: ey [H][Mt], ex [W][Mt]
extern "C" int ipdm_ndft_forward_sets_c64(const float* x, const float* sens, const double* traj, int traj_sets, float* y,
                                          float* work, int B, int n_coils, int M, int H, int W, void* stream) {
  IPDM_REQUIRE(nc_dims_ok(B, n_coils, M, H, W) && nc_sets_ok(B, traj_sets));
  if (B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::toeplitz_ok(H, W) || !nc_grid_ok(B, n_coils, H) || !nc_samples_ok(traj_sets, M)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(x && traj && y && work);
  hipStream_t st = ipdm_stream(stream);
  const int Mt = traj_sets * M;
  float2* ey = reinterpret_cast<float2*>(work);
  float2* ex = ey + (size_t)H * Mt;
  int rc = make_table<float2>(traj, 0, Mt, H, H / 2, H, ey, nullptr, st);
  if (rc) return rc;
  rc = make_table<float2>(traj, 1, Mt, W, W / 2, W, ex, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(ndft_forward_kernel, dim3((M + NC_TILE - 1) / NC_TILE, B, n_coils), dim3(NC_THREADS), 0, st,
                     reinterpret_cast<const float2*>(x), reinterpret_cast<const float2*>(sens), ey, ex, reinterpret_cast<float2*>(y),
                     B, M, H, W, traj_sets);
  return ipdm_launch_status();
}

extern "C" int ipdm_ndft_forward_c64(const float* x, const float* sens, const double* traj, float* y, float* work, int B,
                                     int n_coils, int M, int H, int W, void* stream) {
  return ipdm_ndft_forward_sets_c64(x, sens, traj, 1, y, work, B, n_coils, M, H, W, stream);
}

// float2 tables over the Mt = traj_sets * M samples: ey [H][Mt], ex [W][Mt], exp [Mt][W]
extern "C" int ipdm_ndft_adjoint_sets_c64(const float* y, const float* sens, const double* traj, int traj_sets,
                                          const float* weights, float* x, float* work, int B, int n_coils, int M, int H, int W,
                                          void* stream) {
  IPDM_REQUIRE(nc_dims_ok(B, n_coils, M, H, W) && nc_sets_ok(B, traj_sets));
  if (B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::toeplitz_ok(H, W) || !nc_grid_ok(B, n_coils, H) || !nc_samples_ok(traj_sets, M)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(y && traj && x && work);
  hipStream_t st = ipdm_stream(stream);
  const int Mt = traj_sets * M;
  float2* ey = reinterpret_cast<float2*>(work);
  float2* ex = ey + (size_t)H * Mt;
  float2* exp_ = ex + (size_t)W * Mt;
  int rc = make_table<float2>(traj, 0, Mt, H, H / 2, H, ey, nullptr, st);
  if (rc) return rc;
  rc = make_table<float2>(traj, 1, Mt, W, W / 2, W, ex, exp_, st);
  if (rc) return rc;
  const double scale = 1.0 / sqrt((double)H * (double)W);
  const dim3 grid((W + NC_THREADS - 1) / NC_THREADS, H, sens ? B : n_coils * B);
  if (sens)
    hipLaunchKernelGGL((ndft_adjoint_kernel<float2, true>), grid, dim3(NC_THREADS), 0, st, reinterpret_cast<const float2*>(y),
                       weights, reinterpret_cast<const float2*>(sens), ey, exp_, reinterpret_cast<float2*>(x), B, n_coils, M, H, W,
                       scale, 0, traj_sets);
  else
    hipLaunchKernelGGL((ndft_adjoint_kernel<float2, false>), grid, dim3(NC_THREADS), 0, st, reinterpret_cast<const float2*>(y),
                       weights, nullptr, ey, exp_, reinterpret_cast<float2*>(x), B, n_coils, M, H, W, scale, 0, traj_sets);
  return ipdm_launch_status();
}

extern "C" int ipdm_ndft_adjoint_c64(const float* y, const float* sens, const double* traj, const float* weights, float* x,
                                     float* work, int B, int n_coils, int M, int H, int W, void* stream) {
  return ipdm_ndft_adjoint_sets_c64(y, sens, traj, 1, weights, x, work, B, n_coils, M, H, W, stream);
}

// double2 lag tables ly [2H][M], lx [2W][M], lxp [M][2W], then T as complex64 [2H][2W]
extern "C" int64_t ipdm_toeplitz_psf_workspace_bytes(int M, int H, int W) {
  if (M <= 0 || H <= 0 || W <= 0) return 0;
  return (2 * (int64_t)H + 4 * (int64_t)W) * M * (int64_t)sizeof(double2) + 4 * (int64_t)H * W * (int64_t)sizeof(float2);
}

// one set: psf [2H][2W] of the trajectory traj [M][2]
static int toeplitz_psf_one(const double* traj, const float* weights, float* psf, float* work, int M, int H, int W, hipStream_t st) {
  const int H2 = 2 * H, W2 = 2 * W;
  double2* ly = reinterpret_cast<double2*>(work);
  double2* lx = ly + (size_t)H2 * M;
  double2* lxp = lx + (size_t)W2 * M;
  float2* t = reinterpret_cast<float2*>(lxp + (size_t)W2 * M);
  int rc = make_table<double2>(traj, 0, M, H2, H, H, ly, nullptr, st);
  if (rc) return rc;
  rc = make_table<double2>(traj, 1, M, W2, W, W, lx, lxp, st);
  if (rc) return rc;
  hipLaunchKernelGGL((ndft_adjoint_kernel<double2, false>), dim3((W2 + NC_THREADS - 1) / NC_THREADS, H2, 1), dim3(NC_THREADS), 0, st,
                     nullptr, weights, nullptr, ly, lxp, t, 1, 1, M, H2, W2, 1.0, 1, 1);
  rc = ipdm_launch_status();
  if (rc) return rc;
  rc = ipdm_kspace_large::fft2c(t, t, 1, H2, W2, 0, st);
  if (rc) return rc;
  const size_t n = (size_t)H2 * W2;
  hipLaunchKernelGGL(psf_real_kernel, dim3(ipdm_ew_grid((int64_t)n, NC_THREADS)), dim3(NC_THREADS), 0, st, t, psf, n,
                     (float)(2.0 / sqrt((double)H * (double)W)));
  return ipdm_launch_status();
}

// psf [traj_sets][2H][2W], set t from trajectory t: the sets one after another on the stream, through the one workspace
extern "C" int ipdm_toeplitz_psf_sets_f32(const double* traj, int traj_sets, const float* weights, float* psf, float* work, int M,
                                          int H, int W, void* stream) {
  IPDM_REQUIRE(M > 0 && H > 0 && W > 0 && traj_sets >= 1);
  if (!ipdm_kspace_large::toeplitz_ok(H, W)) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(traj && psf && work);
  hipStream_t st = ipdm_stream(stream);
  for (int t = 0; t < traj_sets; ++t) {
    const int rc = toeplitz_psf_one(traj + 2 * (size_t)t * M, weights ? weights + (size_t)t * M : nullptr,
                                    psf + 4 * (size_t)t * H * W, work, M, H, W, st);
    if (rc) return rc;
  }
  return IPDM_OK;
}

extern "C" int ipdm_toeplitz_psf_f32(const double* traj, const float* weights, float* psf, float* work, int M, int H, int W,
                                     void* stream) {
  return ipdm_toeplitz_psf_sets_f32(traj, 1, weights, psf, work, M, H, W, stream);
}

extern "C" int64_t ipdm_toeplitz_workspace_bytes(int B, int n_coils, int H, int W) {
  if (B <= 0 || n_coils <= 0 || !ipdm_kspace_large::toeplitz_ok(H, W)) return 0;
  return (int64_t)n_coils * B * H * 2 * W * (int64_t)sizeof(float2);
}

extern "C" int ipdm_toeplitz_normal_sets_c64(const float* v, const float* sens, const float* psf, int psf_sets, float* out,
                                             float* work, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && H > 0 && W > 0 && (sens || n_coils == 1) && nc_sets_ok(B, psf_sets));
  if (B == 0) return IPDM_OK;
  if (!ipdm_kspace_large::toeplitz_ok(H, W) || B > 65535 || n_coils > 65535) return IPDM_EUNSUPPORTED;
  IPDM_REQUIRE(v && psf && out && work && out != v);
  const ToepProblem tp{reinterpret_cast<const float2*>(sens), psf, B, n_coils, H, W, psf_sets};
  return ipdm_kspace_large::toeplitz_normal(reinterpret_cast<const float2*>(v), nullptr, nullptr, tp, nullptr,
                                            reinterpret_cast<float2*>(out), reinterpret_cast<float2*>(work), ipdm_stream(stream));
}

extern "C" int ipdm_toeplitz_normal_c64(const float* v, const float* sens, const float* psf, float* out, float* work, int B,
                                        int n_coils, int H, int W, void* stream) {
  return ipdm_toeplitz_normal_sets_c64(v, sens, psf, 1, out, work, B, n_coils, H, W, stream);
}
