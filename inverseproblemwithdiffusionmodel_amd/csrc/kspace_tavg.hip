// Mask-weighted time average of 2D+time multi-coil k-space: the composite that cine acquisitions calibrate
// from (TSENSE, k-t methods).  The per-frame sampling patterns interleave, so their union is fully sampled around the centre
// where no single frame is:
//     count[b][p]   = number of frames t of image b whose mask plane (b*T + t) % Tm sampled pixel p
//     ybar[c][b][p] = (sum over those frames of y[c][b][t][p]) / count[b][p],   exactly 0 where count == 0
// One thread per pixel and pass.  The T mask bytes of the pixel are read once, packed into a bit table in LDS ([word][thread]:
// a thread reads back only what it wrote itself, so there is no barrier) and reused for every coil; y is read at the sampled
// frames only, in frame order (four coils at a time, so that four loads are in flight), summed in double, divided in double
// and rounded once.  No atomics, no reduction across pixels: a pixel's result depends on nothing but its own frames, whatever
// the batch, its position in it, or the grid.  All accesses are float2 or narrower (8-byte alignment suffices).
#include "ipdm_common.h"

namespace {

constexpr int TA_MAX_FRAMES = 4096;
constexpr int TA_THREADS = 256;                 // T <= 1024: 32 words per thread, 32 KiB of LDS at most
constexpr int TA_THREADS_LONG = 64;             // T <= 4096: 128 words per thread, 32 KiB
constexpr int TA_COILS = 4;                     // coils whose loads are in flight together

__global__ __launch_bounds__(TA_THREADS) void kspace_tavg_kernel(const float2* __restrict__ y, const uint8_t* __restrict__ mask,
                                                                 int Tm, int mask_2d, float2* __restrict__ ybar,
                                                                 int32_t* __restrict__ count, int B, int T, int n, int W, int64_t HW) {
  extern __shared__ uint32_t ta_bits[];         // [words][blockDim.x]
  const int words = (T + 31) >> 5;
  const int nt = blockDim.x;
  uint32_t* mine = ta_bits + threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int plane0 = (int)(((int64_t)b * T) % Tm);
    for (int64_t p = (int64_t)blockIdx.x * nt + threadIdx.x; p < HW; p += (int64_t)gridDim.x * nt) {
      const int64_t moff = mask_2d ? p : p % W;
      const int64_t mstride = mask_2d ? HW : (int64_t)W;
      int cnt = 0, plane = plane0;
      for (int w = 0; w < words; ++w) {
        uint32_t bits = 0;
        const int t1 = min(32, T - 32 * w);
        for (int k = 0; k < t1; ++k) {
          if (mask[(int64_t)plane * mstride + moff]) bits |= 1u << k;
          if (++plane == Tm) plane = 0;
        }
        cnt += __popc(bits);
        mine[w * nt] = bits;
      }
      if (count) count[(int64_t)b * HW + p] = cnt;
      const double denom = (double)cnt;
      // TA_COILS coils per pass: their loads of a frame are independent and in flight together (a coil past the last one
      // repeats the last one's loads and stores nothing); every coil still sums its own frames in frame order
      for (int c0 = 0; c0 < n; c0 += TA_COILS) {
        const float2* src[TA_COILS];
        double re[TA_COILS], im[TA_COILS];
#pragma unroll
        for (int k = 0; k < TA_COILS; ++k) {
          src[k] = y + ((size_t)min(c0 + k, n - 1) * B + b) * (size_t)T * HW + p;
          re[k] = im[k] = 0.0;
        }
        for (int w = 0; w < words; ++w) {
          uint32_t bits = mine[w * nt];
          while (bits) {                        // ascending bit = ascending frame
            const size_t off = (size_t)(32 * w + __ffs(bits) - 1) * HW;
            bits &= bits - 1;
            float2 v[TA_COILS];
#pragma unroll
            for (int k = 0; k < TA_COILS; ++k) v[k] = src[k][off];
#pragma unroll
            for (int k = 0; k < TA_COILS; ++k) {
              re[k] += (double)v[k].x;
              im[k] += (double)v[k].y;
            }
          }
        }
#pragma unroll
        for (int k = 0; k < TA_COILS; ++k)
          if (c0 + k < n)
            ybar[((size_t)(c0 + k) * B + b) * HW + p] =
                cnt ? make_float2((float)(re[k] / denom), (float)(im[k] / denom)) : make_float2(0.f, 0.f);
      }
    }
  }
}

static inline bool ta_overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int ipdm_kspace_tavg_c64(const float* y, const uint8_t* mask, int mask_t, float* ybar, int32_t* count, int B, int T,
                                    int n_coils, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && T > 0 && n_coils > 0 && H > 0 && W > 0 && mask_t != 0);
  if (T > TA_MAX_FRAMES) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(y && mask && ybar);
  const int64_t HW = (int64_t)H * W;
  IPDM_REQUIRE(!ta_overlaps(y, (size_t)n_coils * B * T * HW * sizeof(float2), ybar, (size_t)n_coils * B * HW * sizeof(float2)));
  const int threads = T <= 1024 ? TA_THREADS : TA_THREADS_LONG;
  const size_t lds = (size_t)((T + 31) >> 5) * threads * sizeof(uint32_t);
  int64_t gx = (HW + threads - 1) / threads;
  if (gx > 1024) gx = 1024;
  const int gy = B < 65535 ? B : 65535;         // larger batches are folded: image b, b + 65535, ... in one workgroup row
  hipLaunchKernelGGL(kspace_tavg_kernel, dim3((unsigned)gx, gy), dim3(threads), lds, ipdm_stream(stream),
                     reinterpret_cast<const float2*>(y), mask, mask_t > 0 ? mask_t : -mask_t, mask_t < 0 ? 1 : 0,
                     reinterpret_cast<float2*>(ybar), count, B, T, n_coils, W, HW);
  return ipdm_launch_status();
}
