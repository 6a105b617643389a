// Coil sensitivity maps from the fully sampled calibration region of multi-coil k-space (Walsh's adaptive estimator on
// low-resolution calibration images).  Four launches and one memset node, all asynchronous:
//     window the calibration box (zero elsewhere)  ->  centred inverse FFT in place, n_coils * B images (ipdm_fft2c_c64's
//     kernels: whole image in LDS, or row / column strips)  ->  RSS plane + per-image maximum  ->  Walsh kernel
// The Walsh kernel never forms the n x n local covariance: R(x) v = sum over the (2r+1)^2 neighbourhood of
// c(x') (c(x')^H v) is applied matrix-free from the calibration images of the tile and its halo held in LDS, a power
// iteration per pixel with v in registers.  The kernel is templated on a PADDED coil count (4, 8, 16, 32): padded coils
// are zero planes in LDS, every coil loop has a compile-time trip count and unrolls, so v is never indexed at run time.
// fp32 throughout; the per-image maximum is an atomic max on the bit pattern of a non-negative float, i.e. exact and
// order-independent, so the maps of an image are the same bits alone or in any batch.
#include "kspace_fft.h"

namespace {

using namespace ipdm_kspace;

constexpr int CSM_TILE = 16;                   // output tile side: 256 threads, one pixel each
constexpr int CSM_MAX_COILS = 32;
constexpr int CSM_MAX_RADIUS = 4;
constexpr size_t CSM_LDS_MAX = 160 * 1024;
static_assert((size_t)(CSM_TILE + 2 * CSM_MAX_RADIUS) * (CSM_TILE + 2 * CSM_MAX_RADIUS) * CSM_MAX_COILS * sizeof(float2) <= CSM_LDS_MAX,
              "the 32-coil tile with a halo of 4 must fit one CU's LDS");

// w(k) = 0.5 + 0.5 cos(pi (k - N/2) / (a + 1)) inside the box, 0 outside
__device__ __forceinline__ float csm_window(int k, int centre, int a) {
  const int d = k - centre;
  if (d < -a || d > a) return 0.f;
  return 0.5f + 0.5f * cospif((float)d / (float)(a + 1));
}

// calib[img] = w_H (x) w_W . y[img]; y is read inside the box only
__global__ __launch_bounds__(256) void csm_window_kernel(const float2* __restrict__ y, float2* __restrict__ calib, int H, int W,
                                                         int ah, int aw) {
  const int HW = H * W;
  const size_t base = (size_t)blockIdx.y * HW;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += gridDim.x * 256) {
    const int r = e / W, c = e - r * W;
    const float w = csm_window(r, H / 2, ah) * csm_window(c, W / 2, aw);
    float2 v = make_float2(0.f, 0.f);
    if (w != 0.f) {
      const float2 s = y[base + e];
      v = make_float2(s.x * w, s.y * w);
    }
    calib[base + e] = v;
  }
}

// rss[b][e] = sqrt(sum_j |c_j[b][e]|^2) (coil order), rss_max[b] = max over the image: one atomic per wave
__global__ __launch_bounds__(256) void csm_rss_kernel(const float2* __restrict__ calib, float* __restrict__ rss, float* rss_max,
                                                      int B, int n_coils, int HW) {
  const int b = blockIdx.y;
  float m = 0.f;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += gridDim.x * 256) {
    float a = 0.f;
    for (int j = 0; j < n_coils; ++j) {
      const float2 v = calib[((size_t)j * B + b) * HW + e];
      a += v.x * v.x + v.y * v.y;
    }
    a = sqrtf(a);
    rss[(size_t)b * HW + e] = a;
    m = fmaxf(m, a);
  }
  m = ipdm_wave_max(m);
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(rss_max + b), __builtin_bit_cast(unsigned, m));
}

template <int NC>
__device__ __forceinline__ void csm_normalise(float2 (&v)[NC]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) s += v[j].x * v[j].x + v[j].y * v[j].y;
  const float nrm = sqrtf(s);
  const float inv = nrm > 0.f ? 1.f / nrm : 1.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) v[j] = make_float2(v[j].x * inv, v[j].y * inv);
}

// One workgroup: one CSM_TILE x CSM_TILE tile of image b.  LDS: tile[NC][TP][TP] float2, TP = CSM_TILE + 2 radius; a
// wave reads 16 consecutive float2 along W of four tile rows.  Neighbours outside the image are zeros.  Each coil value is
// read twice per neighbour (once for c^H v, once for the update); at NC = 32 the registers cannot hold it in between.
template <int NC>
__global__ __launch_bounds__(CSM_TILE * CSM_TILE) void csm_walsh_kernel(const float2* __restrict__ calib,
                                                                        const float* __restrict__ rss,
                                                                        const float* __restrict__ rss_max, float2* __restrict__ maps,
                                                                        int B, int n_coils, int H, int W, int radius, int power_iters,
                                                                        float thresh, int tiles_w) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float2* tile = reinterpret_cast<float2*>(smem_raw);
  const int TP = CSM_TILE + 2 * radius;
  const int plane = TP * TP;
  const int b = blockIdx.y;
  const int th = blockIdx.x / tiles_w, tw = blockIdx.x - th * tiles_w;
  const int r0 = th * CSM_TILE - radius, c0 = tw * CSM_TILE - radius;
  const int HW = H * W;
  for (int i = threadIdx.x; i < NC * plane; i += CSM_TILE * CSM_TILE) {
    const int j = i / plane, p = i - j * plane;
    const int lr = p / TP, lc = p - lr * TP;
    const int r = r0 + lr, c = c0 + lc;
    float2 v = make_float2(0.f, 0.f);
    if (j < n_coils && r >= 0 && r < H && c >= 0 && c < W) v = calib[((size_t)j * B + b) * HW + (size_t)r * W + c];
    tile[i] = v;
  }
  __syncthreads();
  const int ly = threadIdx.x / CSM_TILE, lx = threadIdx.x - ly * CSM_TILE;
  const int r = th * CSM_TILE + ly, c = tw * CSM_TILE + lx;
  if (r >= H || c >= W) return;                                // (no barrier follows)
  const size_t e = (size_t)r * W + c;
  const bool inside = rss[(size_t)b * HW + e] > thresh * rss_max[b];
  if (!inside) {                                               // outside the support the maps are exactly 0
    for (int j = 0; j < n_coils; ++j) maps[((size_t)j * B + b) * HW + e] = make_float2(0.f, 0.f);
    return;
  }
  float2 v[NC], acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) v[j] = make_float2(1.f, 0.f);   // padded coils: their planes are zero, so R v is zero there
  const int side = 2 * radius + 1;
  for (int it = 0; it <= power_iters; ++it) {                  // v0 = normalise(R 1), then power_iters more applications
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = make_float2(0.f, 0.f);
    for (int dy = 0; dy < side; ++dy) {
      for (int dx = 0; dx < side; ++dx) {
        const float2* cp = tile + (ly + dy) * TP + (lx + dx);
        float2 t = make_float2(0.f, 0.f);                      // c(x')^H v
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const float2 cj = cp[j * plane];
          t.x += cj.x * v[j].x + cj.y * v[j].y;
          t.y += cj.x * v[j].y - cj.y * v[j].x;
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const float2 cj = cp[j * plane];
          acc[j].x += cj.x * t.x - cj.y * t.y;
          acc[j].y += cj.x * t.y + cj.y * t.x;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) v[j] = acc[j];
    csm_normalise<NC>(v);
  }
  // gauge: coil 0 real and non-negative
  const float mag = sqrtf(v[0].x * v[0].x + v[0].y * v[0].y);
  if (mag > 0.f) {
    const float2 ph = make_float2(v[0].x / mag, -v[0].y / mag);
#pragma unroll
    for (int j = 1; j < NC; ++j) v[j] = cmul(v[j], ph);
    v[0] = make_float2(mag, 0.f);
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (j < n_coils) maps[((size_t)j * B + b) * HW + e] = v[j];
}

static inline bool csm_size_ok(int H, int W) {
  return H <= 1024 && W <= 1024 && (lds_fft_ok(H, W) || ipdm_kspace_large::large_ok(H, W));
}
static inline int csm_padded(int n_coils) { return n_coils <= 4 ? 4 : n_coils <= 8 ? 8 : n_coils <= 16 ? 16 : 32; }
static inline bool box_ok(int a, int N) { return a >= 0 && N / 2 - a >= 0 && N / 2 + a <= N - 1; }

template <int NC>
static int launch_walsh(const float2* calib, const float* rss, const float* rss_max, float2* maps, int B, int n_coils, int H, int W,
                        int radius, int power_iters, float thresh, hipStream_t s) {
  const int TP = CSM_TILE + 2 * radius;
  const size_t lds = (size_t)NC * TP * TP * sizeof(float2);
  if (lds > CSM_LDS_MAX) return IPDM_EUNSUPPORTED;
  const int rc = ipdm_lds_optin(csm_walsh_kernel<NC>, lds);
  if (rc) return rc;
  const int tiles_h = (H + CSM_TILE - 1) / CSM_TILE, tiles_w = (W + CSM_TILE - 1) / CSM_TILE;
  hipLaunchKernelGGL(csm_walsh_kernel<NC>, dim3(tiles_h * tiles_w, B), dim3(CSM_TILE * CSM_TILE), lds, s, calib, rss, rss_max, maps, B,
                     n_coils, H, W, radius, power_iters, thresh, tiles_w);
  return ipdm_launch_status();
}

// window + centred inverse transform of n_coils * B images into calib (which may not alias y)
static int calib_images(const float2* y, int ah, int aw, float2* calib, int B, int n_coils, int H, int W, void* stream) {
  const int HW = H * W;
  int gx = (HW + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(csm_window_kernel, dim3(gx, n_coils * B), dim3(256), 0, ipdm_stream(stream), y, calib, H, W, ah, aw);
  const int rc = ipdm_launch_status();
  if (rc) return rc;
  float* c = reinterpret_cast<float*>(calib);
  return ipdm_fft2c_c64(c, c, n_coils * B, H, W, 1, nullptr, stream);
}

// the checks both entries share: IPDM_EINVAL first, then the sizes without a kernel
static int csm_check(int ah, int aw, int B, int n_coils, int H, int W) {
  IPDM_REQUIRE(B >= 0 && n_coils > 0 && H > 0 && W > 0 && box_ok(ah, H) && box_ok(aw, W));
  if (n_coils > CSM_MAX_COILS || !csm_size_ok(H, W) || (int64_t)n_coils * B > 65535) return IPDM_EUNSUPPORTED;
  return IPDM_OK;
}

}  // namespace

extern "C" int ipdm_csm_supported(int n_coils, int radius, int H, int W) {
  return n_coils >= 1 && n_coils <= CSM_MAX_COILS && radius >= 1 && radius <= CSM_MAX_RADIUS && H > 0 && W > 0 && csm_size_ok(H, W);
}

extern "C" size_t ipdm_csm_workspace_bytes(int B, int n_coils, int H, int W) {
  if (B <= 0 || !ipdm_csm_supported(n_coils, 1, H, W) || (int64_t)n_coils * B > 65535) return 0;
  return (size_t)B * H * W * ((size_t)n_coils * sizeof(float2) + sizeof(float));
}

extern "C" int ipdm_csm_calib_images_c64(const float* y, int ah, int aw, float* calib, int B, int n_coils, int H, int W,
                                         void* stream) {
  const int rc = csm_check(ah, aw, B, n_coils, H, W);
  if (rc) return rc;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && calib && y != calib);
  return calib_images(reinterpret_cast<const float2*>(y), ah, aw, reinterpret_cast<float2*>(calib), B, n_coils, H, W, stream);
}

extern "C" int ipdm_csm_walsh_c64(const float* y, int ah, int aw, int radius, int power_iters, float thresh, float* maps,
                                  float* rss, float* rss_max, float* work, int B, int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(radius >= 1 && radius <= CSM_MAX_RADIUS && power_iters >= 0 && thresh >= 0.f);     // NaN fails thresh >= 0
  int rc = csm_check(ah, aw, B, n_coils, H, W);
  if (rc) return rc;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && maps && rss_max && work && y != work);
  hipStream_t s = ipdm_stream(stream);
  const int HW = H * W;
  float2* calib = reinterpret_cast<float2*>(work);
  float* rss_plane = rss ? rss : work + (size_t)2 * n_coils * B * HW;
  rc = calib_images(reinterpret_cast<const float2*>(y), ah, aw, calib, B, n_coils, H, W, stream);
  if (rc) return rc;
  const hipError_t e = hipMemsetAsync(rss_max, 0, (size_t)B * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  int gx = (HW + 255) / 256;
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(csm_rss_kernel, dim3(gx, B), dim3(256), 0, s, calib, rss_plane, rss_max, B, n_coils, HW);
  rc = ipdm_launch_status();
  if (rc) return rc;
  float2* out = reinterpret_cast<float2*>(maps);
  switch (csm_padded(n_coils)) {
    case 4: return launch_walsh<4>(calib, rss_plane, rss_max, out, B, n_coils, H, W, radius, power_iters, thresh, s);
    case 8: return launch_walsh<8>(calib, rss_plane, rss_max, out, B, n_coils, H, W, radius, power_iters, thresh, s);
    case 16: return launch_walsh<16>(calib, rss_plane, rss_max, out, B, n_coils, H, W, radius, power_iters, thresh, s);
    default: return launch_walsh<32>(calib, rss_plane, rss_max, out, B, n_coils, H, W, radius, power_iters, thresh, s);
  }
}
