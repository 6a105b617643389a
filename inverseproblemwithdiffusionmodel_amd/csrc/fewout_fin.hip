// The last layer of the NCSNv2 score networks with its input normalisation fused: end_conv(act(InstanceNorm++(x))), ngf -> 1|2|3
// channels (reference ncsn/models/ncsnv2.py:270-271).  The separate path writes the normalised, activated ngf-channel tensor
// (affine_act_kernel, norm_act.hip) and reads it back (conv3x3_fewout_kernel, conv_thin.hip); this kernel reads the RAW tensor once.
//
// Bits: the result equals affine_act -> conv3x3_fewout bit for bit.
//  * this file is built as norm_act.hip is, WITHOUT floating-point contraction, so `(v - mu) * sc + sh` is the same subtract,
//    multiply, add and expm1f the same code as in affine_act_kernel (build.py contracts the conv*.hip files only);
//  * every multiply-add of the convolution is an explicit fmaf, in conv3x3_fewout_kernel's order: wave g of a workgroup takes the
//    channels g, g + 4, ...; an output's taps of kernel row r form one chain (channel-major, left to right), the quad's two halo
//    columns chains of their own; the chains meet as middle, top, bottom row, left, right halo, then the four waves in wave order,
//    then the bias.
// What differs is the traffic: a thread owns R output rows of its quad, so a loaded row is normalised and activated ONCE and
// serves three output rows from registers ((R + 2) / R rows per output row instead of 3), and two channels' rows are in flight.
#include "ipdm_common.h"

namespace {

__device__ __forceinline__ float fin_elu(float v, float mu, float sc, float sh) {
  return ipdm_act_t<IPDM_ACT_ELU>((v - mu) * sc + sh);
}

// SHFL (W / 4 divides 64): the halo columns are the neighbouring lanes' own activated elements (items are dealt row-major, a row
// of quads never straddles a wave); else they are loaded and activated by the thread itself
template <int COUT, int R, bool SHFL>
__global__ __launch_bounds__(256) void conv3x3_fewout_fin_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const float* __restrict__ coef,
                                                                 float* __restrict__ out, int B, int Cin, int H, int W) {
  __shared__ float red[3][COUT][R][4][64];
  const int Q = W >> 2, S = (H + R - 1) / R;
  const long long items = (long long)B * S * Q;
  const long long HW = (long long)H * W;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (long long it0 = (long long)blockIdx.x * 64; it0 < items; it0 += (long long)gridDim.x * 64) {
    const long long it = it0 + lane < items ? it0 + lane : items - 1;       // a tail lane repeats the last item (not stored)
    const bool live = it0 + lane < items;
    const int q = (int)(it % Q);
    const long long t = it / Q;
    const int y0 = (int)(t % S) * R;
    const int b = (int)(t / S);
    // acc[co][k][r][j]: output row y0 + k, taps of kernel row r (input row y0 + k + r - 1) on the thread's own four columns
    float acc[COUT][R][3][4], hl[COUT][R][3], hr[COUT][R][3];
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
      for (int k = 0; k < R; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          hl[co][k][r] = 0.f; hr[co][k][r] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[co][k][r][j] = 0.f;
        }
    // input rows y0 - 1 .. y0 + R; a row outside the image is read from a valid one and lands in sums that are dropped
    bool ok[R + 2];
    int ro[R + 2];
#pragma unroll
    for (int i = 0; i < R + 2; ++i) {
      const int yy = y0 - 1 + i;
      ok[i] = yy >= 0 && yy < H;
      ro[i] = (yy < 0 ? 0 : (yy < H ? yy : H - 1)) * W;
    }
    const bool lf = q > 0, rt = q < Q - 1;
    const float* base = x + (long long)b * Cin * HW + 4 * q;
    const float* cfb = coef + (long long)b * Cin * 3;

    struct Rows {
      float4 m[R + 2];
      float l[R + 2], r[R + 2];                                   // (!SHFL) the raw halo elements
      float mu, sc, sh;
    };
    auto load = [&](int ci, Rows& d) {
      const float* cp = base + ci * HW;
      d.mu = cfb[ci * 3]; d.sc = cfb[ci * 3 + 1]; d.sh = cfb[ci * 3 + 2];
#pragma unroll
      for (int i = 0; i < R + 2; ++i) {
        const float* rp = cp + ro[i];
        d.m[i] = *reinterpret_cast<const float4*>(rp);
        if constexpr (!SHFL) {
          d.l[i] = rp[lf ? -1 : 0];
          d.r[i] = rp[rt ? 4 : 3];
        }
      }
    };
    auto compute = [&](int ci, const Rows& d) {
#pragma unroll
      for (int i = 0; i < R + 2; ++i) {
        const float mx = fin_elu(d.m[i].x, d.mu, d.sc, d.sh), my = fin_elu(d.m[i].y, d.mu, d.sc, d.sh);
        const float mz = fin_elu(d.m[i].z, d.mu, d.sc, d.sh), mw = fin_elu(d.m[i].w, d.mu, d.sc, d.sh);
        float l, rr;
        if constexpr (SHFL) {
          l = __shfl_up(mw, 1, 64);
          rr = __shfl_down(mx, 1, 64);
        } else {
          l = fin_elu(d.l[i], d.mu, d.sc, d.sh);
          rr = fin_elu(d.r[i], d.mu, d.sc, d.sh);
        }
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
          const float* wc = w + ((long long)co * Cin + ci) * 9;   // wave-uniform: scalar loads
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const int k = i - r;                                  // input row i is kernel row r of output row k
            if (k < 0 || k >= R) continue;
            const float w0 = wc[r * 3], w1 = wc[r * 3 + 1], w2 = wc[r * 3 + 2];
            // output column j takes w0 * in[j-1] + w1 * in[j] + w2 * in[j+1]
            hl[co][k][r] = fmaf(w0, l, hl[co][k][r]);
            acc[co][k][r][0] = fmaf(w1, mx, acc[co][k][r][0]);
            acc[co][k][r][0] = fmaf(w2, my, acc[co][k][r][0]);
            acc[co][k][r][1] = fmaf(w0, mx, acc[co][k][r][1]);
            acc[co][k][r][1] = fmaf(w1, my, acc[co][k][r][1]);
            acc[co][k][r][1] = fmaf(w2, mz, acc[co][k][r][1]);
            acc[co][k][r][2] = fmaf(w0, my, acc[co][k][r][2]);
            acc[co][k][r][2] = fmaf(w1, mz, acc[co][k][r][2]);
            acc[co][k][r][2] = fmaf(w2, mw, acc[co][k][r][2]);
            acc[co][k][r][3] = fmaf(w0, mz, acc[co][k][r][3]);
            acc[co][k][r][3] = fmaf(w1, mw, acc[co][k][r][3]);
            hr[co][k][r] = fmaf(w2, rr, hr[co][k][r]);
          }
        }
      }
    };
    // two channels per trip: both channels' rows are requested before the first is used (the cross-lane moves are convergent
    // operations, which keep hipcc from overlapping trips itself); every condition here is wave-uniform
    for (int ci = grp; ci < Cin; ci += 8) {
      Rows d0, d1;
      const bool two = ci + 4 < Cin;
      load(ci, d0);
      if (two) load(ci + 4, d1);
      compute(ci, d0);
      if (two) compute(ci + 4, d1);
    }
    float o[COUT][R][4];
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const bool up = ok[k], dn = ok[k + 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[co][k][1][j];
          if (up) v += acc[co][k][0][j];
          if (dn) v += acc[co][k][2][j];
          o[co][k][j] = v;
        }
        float left = hl[co][k][1], right = hr[co][k][1];
        if (up) { left += hl[co][k][0]; right += hr[co][k][0]; }
        if (dn) { left += hl[co][k][2]; right += hr[co][k][2]; }
        if (lf) o[co][k][0] += left;
        if (rt) o[co][k][3] += right;
      }
    if (grp > 0) {
#pragma unroll
      for (int co = 0; co < COUT; ++co)
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) red[grp - 1][co][k][j][lane] = o[co][k][j];
    }
    __syncthreads();
    if (grp == 0 && live) {
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int k = 0; k < R; ++k) {
          if (y0 + k >= H) continue;                              // a ragged last strip
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = bv + (((o[co][k][j] + red[0][co][k][j][lane]) + red[1][co][k][j][lane]) + red[2][co][k][j][lane]);
          *reinterpret_cast<float4*>(out + (((long long)b * COUT + co) * H + y0 + k) * W + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
    __syncthreads();                                            // red is rewritten by the next round
  }
}

}  // namespace

extern "C" int ipdm_conv3x3_fewout_fin_supported(int Cin, int Cout, int H, int W) {
  return (W % 4 == 0 && H > 0 && Cout >= 1 && Cout <= 3 && Cin >= 1) ? 1 : 0;
}

extern "C" int ipdm_conv3x3_fewout_fin_f32(const float* x, const float* w, const float* bias, const float* coef, int act,
                                           float* out, int B, int Cin, int Cout, int H, int W, void* stream) {
  IPDM_REQUIRE(B >= 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0);
  if (!ipdm_conv3x3_fewout_fin_supported(Cin, Cout, H, W) || act != IPDM_ACT_ELU) return IPDM_EUNSUPPORTED;
  if (B == 0) return IPDM_OK;
  IPDM_REQUIRE(x && w && coef && out && x != out);
  // float4 rows, as ipdm_conv3x3_thin_f32: a tensor off a 16-byte boundary is the caller's other path
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) return IPDM_EUNSUPPORTED;
  hipStream_t s = ipdm_stream(stream);
  const int Q = W / 4;
  const bool shfl = Q <= 64 && 64 % Q == 0;
  // one output channel: four rows per thread (72 accumulators); two or three: two rows (72 / 108)
#define IPDM_FEWOUT_FIN(CO, R)                                                                                              \
  do {                                                                                                                      \
    const int gx = ipdm_ew_grid((long long)B * ((H + R - 1) / R) * Q, 64);                                                  \
    if (shfl) hipLaunchKernelGGL((conv3x3_fewout_fin_kernel<CO, R, true>), dim3(gx), dim3(256), 0, s, x, w, bias, coef, out, B, Cin, H, W); \
    else hipLaunchKernelGGL((conv3x3_fewout_fin_kernel<CO, R, false>), dim3(gx), dim3(256), 0, s, x, w, bias, coef, out, B, Cin, H, W);     \
  } while (0)
  if (Cout == 1) IPDM_FEWOUT_FIN(1, 4);
  else if (Cout == 2) IPDM_FEWOUT_FIN(2, 2);
  else IPDM_FEWOUT_FIN(3, 2);
#undef IPDM_FEWOUT_FIN
  return ipdm_launch_status();
}
