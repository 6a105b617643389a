// 1-D convolution (k = 1 or 3, dilation 1 / 2 / 4, zero padding) of [N][C][L] float32 sequences on the f16x2 matrix-core
// arithmetic of conv_bx3.hip's HX kernels -- the temporal score networks NCSN1D* (reference ncsn/models/layers1d.py, ncsn1d.py).
//
// Why its own kernel: on the 2-D direct kernel a (N, C, L) tensor is a one-row image -- seven of its eight patch rows are
// padding and two of the three filter rows are zero taps.  Here the GEMM is
//     M = Cout,   K = k * Cin (a chunk: 16 input channels x the k taps, no dead taps),   N = the flattened (sequence, t) columns.
// L (12 / 24 / 48 ...) is shorter than or unrelated to the 32 columns of an MFMA block, so a workgroup's column tile is 96 columns
// = 96 / L WHOLE sequences per wave column group (4 x 24, 8 x 12, 2 x 48: three 32-column blocks, no dead column).  Every
// sequence's rows sit in LDS with `d` zeros on either side ([piece][8-channel half][sequence][L + 2d] x 8 fp16): a tap is a read
// at a shifted position, and no tap reads across the seam between two sequences.
//   arithmetic (conv_kernel.h, "f16x2"): operands as two fp16 pieces, three v_mfma_f32_32x32x16_f16 per product, fp32
//   accumulation; weights scaled by one power of two per output channel at pack time; inputs by one power of two per SEQUENCE
//   (hx_dynamic_scale of its maximum, ext->in_amax); both undone in the epilogue's fma(sum, inv_s, bias) -- the inverse input
//   scale is per column there.  A column's sum runs over (chunk, tap, piece) in one fixed order and involves no other column, so
//   a sequence's bits do not depend on the sequences that share its tile or its batch, nor on the tile shape chosen for Cout.
//   A fragments: global -> VGPR, [tap][ci/16][co/32][piece][lane] x 16 bytes, as the direct kernel's blob with k taps.
// Epilogue (run-time flags, one instantiation per (k, tile shape)): bias, residual (res_second: into the second output only),
// activated / copied second output, the pair mean of ConvMeanPool ((y[2j] + y[2j+1]) / 2: the two columns are neighbouring
// lanes), and the per-sequence maxima of what is stored -- reduced per sequence in LDS (a wave's columns span several sequences),
// then one atomic max per (sequence, workgroup) on the way of the workgroup's channel tile.
// Every global access of activations is a 4-byte one: any 4-byte aligned contiguous tensor is served.
#include "conv_kernel.h"

namespace ipdm_conv {

struct Conv1dArgs {
  const float* x;
  const uint4* wq;
  const float* bias;
  const float* residual;
  float* out;
  float* out_act;
  const float* in_amax;
  float* amax_out;
  float* amax_act;
  int act_out, res_second, pool2;
  int N, Cin, Cout, L, dil;
  int co_tiles;
};

constexpr int C1D_COLS = 96;        // columns per wave column group: three MFMA blocks, 96 / L whole sequences
constexpr int C1D_PLANE = 160;      // LDS positions per column group: (96 / L) * (L + 2 * 4) <= 160 for L >= 12
constexpr int C1D_SEQS = 8;         // sequences per column group at most (L = 12)

// power-of-two input scale of one sequence and its inverse (1, 1 under the static range contract)
__device__ __forceinline__ void c1d_seq_scale(const float* in_amax, int seq, float& s, float& inv_s) {
  s = 1.f;
  inv_s = 1.f;
  if (!in_amax) return;
  const float* p = in_amax + (size_t)seq * IPDM_AMAX_SLOT;
  float m = 0.f;
#pragma unroll
  for (int w = 0; w < IPDM_AMAX_WAYS; ++w) m = fmaxf(m, p[w * IPDM_AMAX_WAY_STRIDE]);
  hx_dynamic_scale(m, s, inv_s);
}

// WCO x WPX waves (WCO * WPX == 4): a wave owns one 32-channel tile and one 96-column group
template <int KS, int WCO, int WPX>
__global__ __launch_bounds__(256, 2) void conv1d_hx2_kernel(Conv1dArgs a) {
  static_assert(WCO * WPX == 4, "four waves per workgroup");
  constexpr int PLANE = C1D_PLANE * WPX;                   // positions of the workgroup's column groups, one behind the other
  constexpr int STAGE = 4 * PLANE;                         // [piece 2][h 2][PLANE] x 16 bytes
  constexpr int ITEMS = (2 * PLANE + 255) / 256;
  __shared__ __align__(16) uint4 lds4[2 * STAGE];
  __shared__ unsigned amx_lds[2][C1D_SEQS * WPX];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, j = lane & 31;
  const int wco = wave / WPX, wpx = wave % WPX;
  const int co_tile = blockIdx.x % a.co_tiles;
  const int col_tile = blockIdx.x / a.co_tiles;
  const int L = a.L;
  const int d = KS == 3 ? a.dil : 0;
  const int padl = L + 2 * d;
  const int seq_g = C1D_COLS / L;                          // sequences per column group
  const int seq_t = seq_g * WPX;                           // ... per workgroup
  const int seq0 = col_tile * seq_t;
  const int plane = seq_t * padl;                          // LDS positions in use (<= PLANE)
  const int n_cc = a.Cin >> 4, n_ct = a.Cout >> 5;

  if (tid < 2 * C1D_SEQS * WPX) (&amx_lds[0][0])[tid] = 0u;

  // ---- staging items: (8-channel half g, sequence, padded position) ----
  int it_lds[ITEMS], it_gofs[ITEMS], it_g[ITEMS];
  bool it_valid[ITEMS];
  float it_s[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    int idx = tid + i * 256;
    idx = idx < 2 * plane ? idx : 2 * plane - 1;           // beyond the last item: store the last one again (same value)
    const int g = idx >= plane ? 1 : 0;
    const int p = idx - g * plane;
    const int sq = p / padl, t = p - sq * padl - d;
    const int seq = seq0 + sq;
    it_g[i] = g;
    it_lds[i] = g * PLANE + p;
    it_valid[i] = t >= 0 && t < L && seq < a.N;
    it_gofs[i] = it_valid[i] ? seq * a.Cin * L + t : 0;
    float inv;
    c1d_seq_scale(a.in_amax, seq < a.N ? seq : 0, it_s[i], inv);
  }
  float preg[ITEMS][8];
  auto load_chunk = [&](int cc) {
    const float* xb = a.x + (size_t)cc * 16 * L;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) preg[i][q] = xb[it_gofs[i] + (it_g[i] * 8 + q) * L];
  };
  auto store_chunk = [&](uint4* st) {
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = it_valid[i] ? preg[i][q] : 0.f;
      uint4 ph, pl;
      split2_scaled(v, it_s[i], ph, pl);
      st[it_lds[i]] = ph;
      st[2 * PLANE + it_lds[i]] = pl;
    }
  };

  // ---- B operand read offsets: lane j of block n is column wpx * 96 + n * 32 + j ----
  int b_base[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const int c = n * 32 + j;
    const int sq = c / L, t = c - sq * L;
    b_base[n] = h * PLANE + (wpx * seq_g + sq) * padl + t + d;
  }

  // ---- A fragments: [tap][cc][ct][piece][lane] ----
  const int ct = co_tile * WCO + wco;
  const size_t tap_stride = (size_t)n_cc * n_ct * 128;
  auto load_A = [&](uint4 (&fr)[KS][2], int cc) {
    const uint4* p = a.wq + ((size_t)cc * n_ct + ct) * 128 + lane;
#pragma unroll
    for (int tap = 0; tap < KS; ++tap) {
      fr[tap][0] = p[tap * tap_stride];
      fr[tap][1] = p[tap * tap_stride + 64];
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int n = 0; n < 3; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

  uint4 afr[KS][2], anx[KS][2];
  load_A(afr, 0);
  load_chunk(0);
  store_chunk(lds4);
  __syncthreads();

  for (int cc = 0; cc < n_cc; ++cc) {
    const uint4* cur = lds4 + (cc & 1) * STAGE;
    uint4* nxt = lds4 + ((cc + 1) & 1) * STAGE;
    const bool more = cc + 1 < n_cc;
    if (more) {
      load_chunk(cc + 1);
      load_A(anx, cc + 1);
    }
#pragma unroll
    for (int tap = 0; tap < KS; ++tap) {
      const int off = (tap - KS / 2) * d;
      const f16x8 ah = __builtin_bit_cast(f16x8, afr[tap][0]), al = __builtin_bit_cast(f16x8, afr[tap][1]);
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const f16x8 bh = __builtin_bit_cast(f16x8, cur[b_base[n] + off]);
        const f16x8 bl = __builtin_bit_cast(f16x8, cur[2 * PLANE + b_base[n] + off]);
        f32x16 c = acc[n];
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, c, 0, 0, 0);
        acc[n] = c;
      }
    }
    if (more) {
      store_chunk(nxt);
#pragma unroll
      for (int tap = 0; tap < KS; ++tap) {
        afr[tap][0] = anx[tap][0];
        afr[tap][1] = anx[tap][1];
      }
    }
    __syncthreads();
  }

  // ---- epilogue: lane <-> column, registers <-> output channels ----
  const float* scale_p = reinterpret_cast<const float*>(a.wq + (size_t)KS * tap_stride);
  const int cob = ct * 32 + 4 * h;                          // channel of r = 0; r adds (r & 3) + 8 * (r >> 2)
  float sv[16], bv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = cob + (r & 3) + 8 * (r >> 2);
    sv[r] = scale_p[co];
    bv[r] = a.bias ? a.bias[co] : 0.f;
  }
  const int Lo = a.pool2 ? L / 2 : L;
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const int c = n * 32 + j;
    const int sq = c / L, t = c - sq * L;
    const int sq_t = wpx * seq_g + sq;
    const int seq = seq0 + sq_t;
    const bool ok = seq < a.N;
    float s_in, inv_in;
    c1d_seq_scale(a.in_amax, ok ? seq : 0, s_in, inv_in);
    const bool writer = ok && !(a.pool2 && (t & 1));        // pair mean: the even column of a pair stores it
    const int to = a.pool2 ? t >> 1 : t;
    const size_t ob = ((size_t)(ok ? seq : 0) * a.Cout + cob) * Lo + to;
    float mo = 0.f, ma = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = fmaf(acc[n][r], sv[r] * inv_in, bv[r]);
      if (a.pool2) {                                         // (uniform branch; every lane takes part in the exchange)
        const float p = __shfl_xor(v, 1, 64);
        v = ((t & 1) ? p + v : v + p) * 0.5f;
      }
      if (writer) {
        const size_t o = ob + (size_t)((r & 3) + 8 * (r >> 2)) * Lo;
        float vr = v;
        if (a.residual) v += a.residual[o];
        vr = a.res_second ? vr : v;
        mo = fmaxf(mo, fabsf(vr));
        if (a.out) a.out[o] = vr;
        if (a.out_act) {
          const float e = a.act_out == IPDM_ACT_ELU ? fast_elu(v) : ipdm_act(v, a.act_out);
          ma = fmaxf(ma, fabsf(e));
          a.out_act[o] = e;
        }
      }
    }
    if (writer) {
      if (a.amax_out) atomicMax(&amx_lds[0][sq_t], __builtin_bit_cast(unsigned, mo));
      if (a.amax_act) atomicMax(&amx_lds[1][sq_t], __builtin_bit_cast(unsigned, ma));
    }
  }
  if (a.amax_out || a.amax_act) {                            // (uniform)
    __syncthreads();
    if (tid < seq_t && seq0 + tid < a.N) {
      const size_t slot = (size_t)(seq0 + tid) * IPDM_AMAX_SLOT;
      if (a.amax_out) ipdm_amax_atomic(a.amax_out + slot, co_tile, __builtin_bit_cast(float, amx_lds[0][tid]));
      if (a.amax_act) ipdm_amax_atomic(a.amax_act + slot, co_tile, __builtin_bit_cast(float, amx_lds[1][tid]));
    }
  }
}

template <int KS, int WCO, int WPX>
static int launch_conv1d(Conv1dArgs a, hipStream_t s) {
  const int seq_t = (C1D_COLS / a.L) * WPX;
  a.co_tiles = a.Cout / (32 * WCO);
  const int64_t nblk = (int64_t)((a.N + seq_t - 1) / seq_t) * a.co_tiles;
  if (nblk > 0x7fffffff) return IPDM_EUNSUPPORTED;
  hipLaunchKernelGGL((conv1d_hx2_kernel<KS, WCO, WPX>), dim3((unsigned)nblk), dim3(256), 0, s, a);
  return ipdm_launch_status();
}

// per-output-channel power-of-two weight scale (max |w s| in [2^13, 2^14)) and the two-piece fragments, as conv_bx3.hip's blob
__global__ __launch_bounds__(256) void c1d_scale_kernel(const float* __restrict__ w, float* __restrict__ inv_scale, int Cout,
                                                        int per_co) {
  __shared__ float red[4];
  const int co = blockIdx.x;
  float m = 0.f;
  if (co < Cout)
    for (int i = threadIdx.x; i < per_co; i += 256) m = fmaxf(m, fabsf(w[(int64_t)co * per_co + i]));
  m = ipdm_wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int e = 0;
    const bool ok = mx > 0.f && mx < INFINITY;
    if (ok) (void)frexpf(mx, &e);
    inv_scale[co] = ok ? ldexpf(1.f, e - 14) : 1.f;
  }
}

__global__ __launch_bounds__(256) void c1d_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out,
                                                       const float* __restrict__ inv_scale, int Cout, int Cin, int k, int n_cc,
                                                       int n_ct) {
  const int64_t total = (int64_t)k * n_cc * n_ct * 512;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & 7), r = (int)((i >> 3) & 31), h = (int)((i >> 8) & 1);
    const int64_t rest = i >> 9;
    const int ct = (int)(rest % n_ct);
    const int cc = (int)((rest / n_ct) % n_cc);
    const int tap = (int)(rest / ((int64_t)n_ct * n_cc));
    const int co = ct * 32 + r, ci = cc * 16 + 8 * h + q;
    const float v = w[((int64_t)co * Cin + ci) * k + tap] * (1.f / inv_scale[co]);
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    const int64_t base = rest * 2 * 512 + h * 256 + r * 8 + q;
    out[base] = __builtin_bit_cast(unsigned short, hi);
    out[base + 512] = __builtin_bit_cast(unsigned short, lo);
  }
}

// pair mean along the last axis: y[row][j] = (x[row][2j] + x[row][2j+1]) / 2
__global__ __launch_bounds__(256) void meanpool1d2_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * 256)
    y[i] = (x[2 * i] + x[2 * i + 1]) * 0.5f;
}

// y = a * x + b and the per-image maxima of what is written (one workgroup per image)
__global__ __launch_bounds__(256) void scale_shift_amax_kernel(const float* __restrict__ x, float* __restrict__ y, float* amax,
                                                               int64_t per_image, float sa, float sb) {
  __shared__ float red[4];
  const float* p = x + (int64_t)blockIdx.x * per_image;
  float* o = y + (int64_t)blockIdx.x * per_image;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < per_image; i += 256) {
    const float v = fmaf(sa, p[i], sb);
    m = fmaxf(m, fabsf(v));
    o[i] = v;
  }
  ipdm_amax_commit_block(m, amax + (size_t)blockIdx.x * IPDM_AMAX_SLOT, 0, red);
}

static bool conv1d_shape_ok(int Cin, int Cout, int L, int k, int dilation) {
  return Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 64 == 0 && (k == 1 || k == 3) && L >= 12 && C1D_COLS % L == 0 &&
         (k == 1 || dilation == 1 || dilation == 2 || dilation == 4);
}

}  // namespace ipdm_conv

using namespace ipdm_conv;

extern "C" int ipdm_conv1d_hx2_supported(int Cin, int Cout, int L, int k, int dilation) {
  return conv1d_shape_ok(Cin, Cout, L, k, dilation) ? 1 : 0;
}

extern "C" int64_t ipdm_conv1d_hx2_weight_bytes(int Cout, int Cin, int k) {
  if (Cout <= 0 || Cin <= 0 || Cin % 16 || Cout % 32 || !(k == 1 || k == 3)) return -1;
  return (int64_t)k * (Cin / 16) * (Cout / 32) * 2048 + (int64_t)Cout * 4;
}

extern "C" int ipdm_conv1d_hx2_pack_weight(const float* w, void* packed, int Cout, int Cin, int k, void* stream) {
  IPDM_REQUIRE(w && packed && Cout > 0 && Cin > 0 && (k == 1 || k == 3));
  if (Cin % 16 || Cout % 32) return IPDM_EUNSUPPORTED;
  const int n_cc = Cin / 16, n_ct = Cout / 32;
  const int64_t total = (int64_t)k * n_cc * n_ct * 512;
  float* inv_scale = reinterpret_cast<float*>(static_cast<char*>(packed) + total * 4);
  hipLaunchKernelGGL(c1d_scale_kernel, dim3(Cout), dim3(256), 0, ipdm_stream(stream), w, inv_scale, Cout, Cin * k);
  hipLaunchKernelGGL(c1d_pack_kernel, dim3(ipdm_ew_grid(total, 256)), dim3(256), 0, ipdm_stream(stream), w,
                     (unsigned short*)packed, inv_scale, Cout, Cin, k, n_cc, n_ct);
  return ipdm_launch_status();
}

extern "C" int ipdm_conv1d_hx2_f32(const float* x, const void* packed, const float* bias, const float* residual, float* out,
                                   float* out_act, int act_out, int N, int Cin, int Cout, int L, int k, int dilation,
                                   int pool2, const ipdm_conv_ext_t* ext, void* stream) {
  IPDM_REQUIRE(N >= 0 && Cin > 0 && Cout > 0 && L > 0 && (k == 1 || k == 3) && dilation >= 1);
  if (N == 0) return IPDM_OK;
  IPDM_REQUIRE(x && packed && (out || out_act) && x != out && x != out_act);
  if (!conv1d_shape_ok(Cin, Cout, L, k, dilation)) return IPDM_EUNSUPPORTED;
  if (ext && (ext->bias_bstride != 0 || (ext->out_scale != 0.f && ext->out_scale != 1.f))) return IPDM_EUNSUPPORTED;
  if ((int64_t)N * (Cin > Cout ? Cin : Cout) * L >= (int64_t)1 << 31) return IPDM_EUNSUPPORTED;   // (32-bit input offsets)
  Conv1dArgs a;
  a.x = x; a.wq = static_cast<const uint4*>(packed); a.bias = bias; a.residual = residual; a.out = out; a.out_act = out_act;
  a.in_amax = ext ? ext->in_amax : nullptr;
  a.amax_out = ext && out ? ext->out_amax : nullptr;
  a.amax_act = ext && out_act ? ext->act_amax : nullptr;
  a.act_out = act_out; a.res_second = ext ? (ext->res_second != 0) : 0; a.pool2 = pool2 != 0;
  a.N = N; a.Cin = Cin; a.Cout = Cout; a.L = L; a.dil = k == 3 ? dilation : 1; a.co_tiles = 0;
  IPDM_REQUIRE(!a.res_second || (residual && out && out_act));
  hipStream_t s = ipdm_stream(stream);
  // 128 output channels per workgroup where Cout allows, else 64 channels x two column groups: a rule of Cout alone
  if (Cout % 128 == 0) return k == 3 ? launch_conv1d<3, 4, 1>(a, s) : launch_conv1d<1, 4, 1>(a, s);
  return k == 3 ? launch_conv1d<3, 2, 2>(a, s) : launch_conv1d<1, 2, 2>(a, s);
}

extern "C" int ipdm_meanpool1d2_f32(const float* x, float* y, int rows, int L, void* stream) {
  IPDM_REQUIRE(rows >= 0 && L > 0 && L % 2 == 0);
  if (rows == 0) return IPDM_OK;
  IPDM_REQUIRE(x && y && x != y);
  const int64_t n_out = (int64_t)rows * (L / 2);
  hipLaunchKernelGGL(meanpool1d2_kernel, dim3(ipdm_ew_grid(n_out, 256)), dim3(256), 0, ipdm_stream(stream), x, y, (long long)n_out);
  return ipdm_launch_status();
}

extern "C" int ipdm_scale_shift_amax_f32(const float* x, float* y, float* amax_out, int n_images, int64_t per_image, float a,
                                         float b, void* stream) {
  IPDM_REQUIRE(n_images >= 0 && per_image > 0);
  if (n_images == 0) return IPDM_OK;
  IPDM_REQUIRE(x && y && amax_out);
  hipLaunchKernelGGL(scale_shift_amax_kernel, dim3((unsigned)n_images), dim3(256), 0, ipdm_stream(stream), x, y, amax_out,
                     (long long)per_image, a, b);
  return ipdm_launch_status();
}
