// 3x3 SAME stride-1 convolution as an implicit GEMM on gfx950 MFMA.
//
// Replaces tf.nn.conv2d + tf.nn.bias_add (+ relu / sigmoid / inference BN / softmax) at
// unet.py:35-42, 44-63, 65-74; unet_simple.py:19-42, 98-107; small.py:13-34; refine.py:18-31.
//
// GEMM view: D[cout][pixel] = sum_k Wp[cout][k] * X[pixel][k], k <-> (tap, c), tap = kh*3 + kw,
// X[pixel][k] = x[n, h+kh-1, w+kw-1, c] (zero outside the frame).
//   A operand = packed weights (rows = output channels), B operand = activations (rows = pixels);
//   both K-contiguous, so every MFMA operand fragment is ONE 16-byte LDS read per lane, and a 16x16
//   MFMA tile leaves 4 consecutive output channels of one pixel in each lane.
// K layout ("granules" of 64 bytes = GE elements): when cin_pad % GE == 0 the K axis is
//   channel-chunk-major — granule g covers channels (g/9)*GE .. +GE of tap g%9 — so the 9 taps that
//   re-read the same input rows are consecutive K-steps and hit L2; otherwise tap-major k = tap*cin_pad+c.
//
// This file: the routing (conv_impl), the C entry points that only build a ConvCall, the option table (vm_set_option)
// and the two generic kernels.  Every other family has its own unit, reached through conv_dispatch.h: the patch kernels
// and the split-K reduction (conv_patch.hip), the narrow-cout / narrow-input convs (conv_thin.hip), the row-stationary
// kernel (conv_rows.hip), the first pair (conv_pair.hip), the folded 2x resize (conv_up2x.hip), the cin <= 8 first
// layer and refine conv + softmax (conv_first.hip), the cout == 1 head (conv_head.hip), weight packing (conv_pack.hip).
// The two generic kernels:
//   conv3x3_mfma  register-staged, 256 threads, tiles 128x128 / 256x64, 128-byte K-steps, 2-slot LDS.
//                 Used for small grids, the fused softmax and as the reference implementation.
//   conv3x3_glds  LDS-DMA pipelined (buffer_load ... lds), 512 threads, tiles 256x256 / 256x128 / 512x64,
//                 64-byte K-steps in a 4-6 slot ring with counted vmcnt (3-5 stages in flight).
// bf16: v_mfma_f32_16x16x32_bf16; f32: v_mfma_f32_16x16x4_f32 (exact f32 products; a 2-level sum).

#include <cstring>
#include <initializer_list>

#include "conv_dispatch.h"

namespace vm {

// ConvArgs, swizzles, MFMA wrappers, LDS-DMA helpers: conv_common.h

// Decode (h, w) of the pixels m0 + r of a tile without per-lane 64-bit division: the tile origin is decoded
// once (wave-uniform), a row offset r < BM + W is split by a float reciprocal (exact after one fix-up for
// values < 2^24).  Pixels at or past M get h = -2^30 so every tap is out of range.
struct TileOrigin {
  int h0, w0;
  float rcp_w, rcp_h;
};

__device__ __forceinline__ TileOrigin tile_origin(long m0, int H, int W) {
  TileOrigin o;
  const long q = m0 / W;
  o.w0 = (int)(m0 - q * W);
  o.h0 = (int)(q % H);
  o.rcp_w = __builtin_amdgcn_rcpf((float)W);  // approximate: fast_div corrects the quotient
  o.rcp_h = __builtin_amdgcn_rcpf((float)H);
  return o;
}

__device__ __forceinline__ int fast_div(int t, int d, float rcp) {
  int q = (int)((float)t * rcp);
  q -= (q * d > t) ? 1 : 0;
  q += ((q + 1) * d <= t) ? 1 : 0;
  return q;
}

__device__ __forceinline__ void pixel_hw(const TileOrigin& o, int r, int H, int W, bool valid, int& h, int& w) {
  const int t = o.w0 + r;
  const int dq = fast_div(t, W, o.rcp_w);
  w = t - dq * W;
  h = o.h0 + dq;
  if (h >= H) h -= fast_div(h, H, o.rcp_h) * H;  // the tile runs into the next frame
  if (!valid) h = -0x40000000;
}

// ================================================================ register-staged kernel
template <int BM, int BN>
constexpr int mfma_lds_bytes() {
  return (2 * (BM + BN) * 128) > (BM * (BN + 4) * 4) ? (2 * (BM + BN) * 128) : (BM * (BN + 4) * 4);
}

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256, 2) void conv3x3_mfma(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RB = 128;
  constexpr int CE = 16 / sizeof(T);  // elements per 16-byte chunk
  constexpr int GE = 64 / sizeof(T);  // elements per 64-byte granule
  constexpr int BKE = RB / sizeof(T);  // K elements per step
  constexpr int XR = BM / 32, WR = BN / 32;
  constexpr int WM = BM / 64, WN = BN / 64;
  static_assert(WM * WN == 4, "4 waves of 64x64");
  constexpr int STAGE = (BM + BN) * RB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int t = xcd_tile(blockIdx.x, a.tiles_total);
  const int mt = t / a.tiles_n, nt = t - mt * a.tiles_n;
  const long m0 = (long)mt * BM;
  const int n0 = nt * BN;
  const int H = a.H, W = a.W;
  const int chunk = tid & 7, rbase = tid >> 3;

  const long xbase = m0 - W - 1;  // lowest pixel any tap of this tile touches
  const __amdgpu_buffer_rsrc_t xrs = x_rsrc<T>(a, xbase);
  const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, n0);
  const TileOrigin org = tile_origin(m0, H, W);
  const int xcs = a.x_cstride;
  // per row: byte offset of the pixel relative to xbase, and a 9-bit mask of the taps that stay inside the
  // frame (bit 9, the K padding "tap", is never set) -> a K-step costs one bit test + add + select per load
  int pofs[XR], tmask[XR];
  int ph0, pw0;
  pixel_hw(org, rbase, H, W, true, ph0, pw0);
  const int pofs0 = (rbase + W + 1) * xcs * (int)sizeof(T);
#pragma unroll
  for (int i = 0; i < XR; ++i) {
    const int r = rbase + 32 * i;
    int ph, pw;
    if (W >= 32) {  // rows of a lane are 32 pixels apart: at most one row wrap per step
      ph = ph0;
      pw = pw0;
      pw0 += 32;
      if (pw0 >= W) {
        pw0 -= W;
        ph0 = ph0 + 1 == H ? 0 : ph0 + 1;
      }
    } else {
      pixel_hw(org, r, H, W, true, ph, pw);
    }
    if (m0 + r >= a.M) ph = -0x40000000;
    pofs[i] = pofs0 + i * 32 * xcs * (int)sizeof(T);
    const int vr = (ph >= 1 && ph <= H) | ((ph >= 0 && ph < H) << 1) | ((ph >= -1 && ph < H - 1) << 2);
    const int vc = (pw >= 1) | (((unsigned)pw < (unsigned)W) << 1) | ((pw < W - 1) << 2);
    const int vcc = ((unsigned)pw < (unsigned)W) ? vc : 0;
    int m = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) m |= (((vr >> (t / 3)) & (vcc >> (t % 3))) & 1) << t;
    tmask[i] = m;
  }
  uint4 xr[XR], wr[WR];
  const int wofs = (rbase * a.K_pad + chunk * CE) * (int)sizeof(T);
  const int wstride = 32 * a.K_pad * (int)sizeof(T);

  auto load = [&](int kt) {
    int tap, delta;
    if (a.chunk_major) {  // the step's two granules (chunks 0-3 and 4-7) decoded on the scalar unit
      const int g0 = 2 * kt, g1 = g0 + 1;
      const int cc0 = g0 / 9, cc1 = g1 / 9;
      const int tap0 = g0 < a.ng ? g0 - cc0 * 9 : 9, tap1 = g1 < a.ng ? g1 - cc1 * 9 : 9;
      const int d0 = (int)(((tap0 / 3 - 1) * W + tap0 % 3 - 1) * xcs + src_chan(a, cc0 * GE)) * (int)sizeof(T);
      const int d1 = (int)(((tap1 / 3 - 1) * W + tap1 % 3 - 1) * xcs + src_chan(a, cc1 * GE)) * (int)sizeof(T);
      const bool hi = chunk >= 4;
      tap = hi ? tap1 : tap0;
      delta = (hi ? d1 : d0) + (chunk & 3) * 16;
    } else {
      int c;
      k_to_tap<GE>(a, kt * BKE + chunk * CE, tap, c);
      delta = (int)(((tap / 3 - 1) * W + tap % 3 - 1) * xcs + src_chan(a, c)) * (int)sizeof(T);
    }
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int off = ((tmask[i] >> tap) & 1) ? pofs[i] + delta : OOB;
      xr[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < WR; ++i) {
      const int off = wofs + i * wstride + kt * RB;
      wr[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 0));
    }
  };
  auto store = [&](int buf) {
    char* s = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < XR; ++i) *reinterpret_cast<uint4*>(s + swz<RB>(rbase + 32 * i, chunk)) = xr[i];
#pragma unroll
    for (int i = 0; i < WR; ++i) *reinterpret_cast<uint4*>(s + BM * RB + swz<RB>(rbase + 32 * i, chunk)) = wr[i];
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // f32: the products of one K-step chain into a fresh partial added to the running sum (two-level
  // summation, error ~(32 + K/32) ulp instead of K ulp for K up to 9216); bf16: one chain.
  constexpr bool SPLIT = sizeof(T) == 4;
  auto compute = [&](int buf) {
    const char* s = smem + buf * STAGE;
    f32x4 part[4][4];
    if (SPLIT) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int ck = kb * 4 + (lane >> 4);
      uint4 av[4], bv[4];
#pragma unroll
      for (int f = 0; f < 4; ++f)
        av[f] = *reinterpret_cast<const uint4*>(s + BM * RB + swz<RB>(wn * 64 + f * 16 + (lane & 15), ck));
#pragma unroll
      for (int f = 0; f < 4; ++f) bv[f] = *reinterpret_cast<const uint4*>(s + swz<RB>(wm * 64 + f * 16 + (lane & 15), ck));
#pragma unroll
      for (int fc = 0; fc < 4; ++fc)
#pragma unroll
        for (int fp = 0; fp < 4; ++fp) mma16<T>(av[fc], bv[fp], SPLIT ? part[fc][fp] : acc[fc][fp]);
    }
    if (SPLIT) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
    }
  };

  const int nk = a.nk;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) load(kt + 1);
    compute(kt & 1);
    if (kt + 1 < nk) store((kt + 1) & 1);
    __syncthreads();
  }

  // fast epilogue (bf16 output, no softmax): y = act(acc * scale' + shift') in registers, bf16 rows staged
  // in LDS (4 channels = one ds_write_b64 per fragment), then 16-byte buffer stores whose descriptor ends at
  // the last pixel, so rows past M drop in hardware.
  if (sizeof(T) == 2 && a.y_dtype == VM_BF16 && a.act != VM_ACT_SOFTMAX && a.y_vec && (a.cout & 7) == 0) {
    constexpr int SR16 = BN * 2 + 16;  // staging row stride in bytes
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) {
      const int col = wn * 64 + fc * 16 + 4 * (lane >> 4);
      float mul[4], add[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = min(n0 + col + j, a.cout - 1);
        const float sc = a.scale ? a.scale[co] : 1.f;
        mul[j] = sc;
        add[j] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
      }
#pragma unroll
      for (int fp = 0; fp < 4; ++fp) {
        const int row = wm * 64 + fp * 16 + (lane & 15);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = fmaf(acc[fc][fp][j], mul[j], add[j]);
          if (a.act == VM_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
          else if (a.act == VM_ACT_SIGMOID) v[j] = sigmoid_precise(v[j]);
        }
        uint2 pk;
        pk.x = bf16x2_bits(v[0], v[1]);
        pk.y = bf16x2_bits(v[2], v[3]);
        *reinterpret_cast<uint2*>(smem + row * SR16 + col * 2) = pk;
      }
    }
    __syncthreads();
    constexpr int CPR = BN / 8;
    const int ycs2 = a.y_cstride * 2;
    const long rows_left = a.M - m0;
    const long rec = rows_left * (long)ycs2;
    uint16_t* Yb = reinterpret_cast<uint16_t*>(a.y) + a.y_coff + m0 * (long)a.y_cstride + n0;
    const __amdgpu_buffer_rsrc_t yrs =
        __builtin_amdgcn_make_buffer_rsrc(Yb, 0, rec > 0x7ffffff0L ? 0x7ffffff0 : (int)rec, 0x00020000);
#pragma unroll
    for (int it = 0; it < BM * CPR / 256; ++it) {
      const int idx = it * 256 + tid;
      const int rr = idx / CPR, cc = idx % CPR;
      const uint4 d = *reinterpret_cast<const uint4*>(smem + rr * SR16 + cc * 16);
      const int off = (n0 + cc * 8 < a.cout) ? rr * ycs2 + cc * 16 : OOB;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), yrs,
                                             off, 0, 0);
    }
    return;
  }

  // general epilogue: f32 staging in LDS, then coalesced 16-byte stores
  constexpr int SROW = BN + 4;
  float* stg = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int fc = 0; fc < 4; ++fc) {
    const int col = wn * 64 + fc * 16 + 4 * (lane >> 4);
    float bsv[4] = {0.f, 0.f, 0.f, 0.f}, scv[4] = {1.f, 1.f, 1.f, 1.f}, shv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = min(n0 + col + j, a.cout - 1);  // clamped: always a valid address
      if (a.bias) bsv[j] = a.bias[co];
      if (a.scale) scv[j] = a.scale[co];
      if (a.shift) shv[j] = a.shift[co];
    }
#pragma unroll
    for (int fp = 0; fp < 4; ++fp) {
      const int row = wm * 64 + fp * 16 + (lane & 15);
      float4 v;
      float* vv = reinterpret_cast<float*>(&v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float tv = (acc[fc][fp][j] + bsv[j]) * scv[j] + shv[j];
        if (a.act == VM_ACT_RELU) tv = tv > 0.f ? tv : 0.f;
        else if (a.act == VM_ACT_SIGMOID) tv = sigmoid_precise(tv);
        vv[j] = tv;
      }
      *reinterpret_cast<float4*>(stg + row * SROW + col) = v;
    }
  }
  __syncthreads();

  if (a.act == VM_ACT_SOFTMAX) {  // host guarantees a single channel tile (n0 == 0, cout <= BN)
    for (int rr = tid; rr < BM; rr += 256) {
      float* rowp = stg + rr * SROW;
      float mx = -INFINITY;
      for (int c = 0; c < a.cout; ++c) mx = fmaxf(mx, rowp[c]);
      float sum = 0.f;
      for (int c = 0; c < a.cout; ++c) {
        const float e = expf(rowp[c] - mx);
        rowp[c] = e;
        sum += e;
      }
      const float inv = 1.f / sum;
      for (int c = 0; c < a.cout; ++c) rowp[c] *= inv;
    }
    __syncthreads();
  }

  if (a.y_dtype == VM_BF16) {
    constexpr int CPR = BN / 8;
    uint16_t* Y = reinterpret_cast<uint16_t*>(a.y) + a.y_coff;
    for (int idx = tid; idx < BM * CPR; idx += 256) {
      const int rr = idx / CPR, cc = idx - rr * CPR;
      const long p = m0 + rr;
      const int co = n0 + cc * 8;
      if (p >= a.M || co >= a.cout) continue;
      const float* src = stg + rr * SROW + cc * 8;
      uint16_t* dst = Y + p * (long)a.y_cstride + co;
      if (a.y_vec && co + 8 <= a.cout) *reinterpret_cast<uint4*>(dst) = Chunk<uint16_t>::pack(src);
      else
        for (int j = 0; j < 8 && co + j < a.cout; ++j) dst[j] = f2bf(src[j]);
    }
  } else {
    constexpr int CPR = BN / 4;
    float* Y = reinterpret_cast<float*>(a.y) + a.y_coff;
    for (int idx = tid; idx < BM * CPR; idx += 256) {
      const int rr = idx / CPR, cc = idx - rr * CPR;
      const long p = m0 + rr;
      const int co = n0 + cc * 4;
      if (p >= a.M || co >= a.cout) continue;
      const float* src = stg + rr * SROW + cc * 4;
      float* dst = Y + p * (long)a.y_cstride + co;
      if (a.y_vec && co + 4 <= a.cout) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
      else
        for (int j = 0; j < 4 && co + j < a.cout; ++j) dst[j] = src[j];
    }
  }
}

// ================================================================ LDS-DMA pipelined kernel
// Tiles are filled by buffer_load_dwordx4 ... lds (global -> LDS, no VGPRs, 1 KiB = 1024/RB operand rows
// per wave-instruction, called a "piece"):
//   * the LDS image is lane-linear, so the XOR swizzle moves to the SOURCE: the lane that fills physical
//     chunk p of row r fetches logical chunk p ^ f(r) (an involution; the MFMA reads use swz<RB>()).
//   * SAME padding / pixels past the end get an out-of-range buffer offset -> the DMA writes zeros.
//   * S-slot ring with 64-byte K-steps: slot kt%S is waited with a COUNTED vmcnt (up to S-2 younger
//     stages stay in flight), then one raw s_barrier per K-step publishes slot kt and frees slot (kt-1)%S,
//     which the pieces of K-step kt+S-1 refill while the MFMAs of K-step kt run.
// 8 waves of (BM/WM) pixels x 64 output channels each.
template <typename T, int RB, int BM, int BN, int WM, int WN, int S>
struct GldsCfg {
  static constexpr int NW = WM * WN, NT = 64 * NW;
  static constexpr int TPM = BM / WM, TPN = BN / WN;
  static constexpr int FP = TPM / 16, FC = TPN / 16;
  static constexpr int RPP = 1024 / RB;           // operand rows per DMA piece
  static constexpr int XP = BM / RPP, WP = BN / RPP;  // pieces per stage
  static constexpr int XPW = XP / NW;              // X pieces per wave
  static constexpr int WPW = (WP + NW - 1) / NW;   // max W pieces per wave
  static constexpr int STAGE = (BM + BN) * RB;
  static constexpr int EPI = BM * (64 + 4) * 4;    // one 64-channel f32 slab
  static constexpr int LDS = (S * STAGE > EPI ? S * STAGE : EPI);
  static_assert(NW == 8, "8-wave blocks");
  static_assert(TPN == 64, "epilogue slabs are one wave-column (64 channels) wide");
  static_assert(XP % NW == 0, "whole X pieces per wave");
  static_assert(S >= 2 && S <= 8, "ring depth");
};

template <typename T, int RB, int BM, int BN, int WM, int WN, int S, bool FAST>
__global__ __launch_bounds__(512, 1) void conv3x3_glds(ConvArgs a) {
  using C = GldsCfg<T, RB, BM, BN, WM, WN, S>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CE = 16 / sizeof(T);
  constexpr int GE = 64 / sizeof(T);
  constexpr int BKE = RB / sizeof(T);
  constexpr int CPR = RB / 16;  // chunks per row
  constexpr int FP = C::FP, FC = C::FC, XPW = C::XPW, WPW = C::WPW, NT = C::NT, NW = C::NW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int t = xcd_tile(blockIdx.x, a.tiles_total);
  const int mt = t / a.tiles_n, nt = t - mt * a.tiles_n;
  const long m0 = (long)mt * BM;
  const int n0 = nt * BN;
  const int H = a.H, W = a.W;

  const long xbase = m0 - W - 1;
  const __amdgpu_buffer_rsrc_t xrs = x_rsrc<T>(a, xbase);
  const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, n0);

  // this lane's DMA rows: X piece i of this wave fills rows (wave + i*NW)*RPP + lane/CPR, physical chunk lane%CPR
  const int lrow = lane / CPR, lpos = lane % CPR;
  const TileOrigin org = tile_origin(m0, H, W);
  int prow[XPW], ph[XPW], pw[XPW], xq[XPW];
#pragma unroll
  for (int i = 0; i < XPW; ++i) {
    const int row = (wave + i * NW) * C::RPP + lrow;
    xq[i] = (swz<RB>(row, lpos) - row * RB) >> 4;  // logical chunk that belongs in physical chunk lpos
    prow[i] = row + W + 1;
    pixel_hw(org, row, H, W, m0 + row < a.M, ph[i], pw[i]);
  }
  int woff[WPW];
  int nwp = 0;  // W pieces of this wave (wave-uniform)
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int piece = wave + i * NW;
    const int row = piece * C::RPP + lrow;
    woff[i] = (row * a.K_pad + ((swz<RB>(row, lpos) - row * RB) >> 4) * CE) * (int)sizeof(T);
    if (piece < C::WP) ++nwp;
  }
  const int lps = XPW + nwp;  // DMA pieces this wave issues per stage
  const int xcs = a.x_cstride;

  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  auto issue = [&](int kt, int slot) {
    const uint32_t sbase = lds0 + slot * C::STAGE;
    int tapu = 0, c0 = 0;
    if (FAST && RB == 64) {  // one granule per K-step: tap and channel base are wave-uniform
      const int cc = kt / 9;
      tapu = kt - cc * 9;
      c0 = cc * GE;
    }
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      int tap, c;
      if (FAST && RB == 64) {
        tap = tapu;
        c = c0 + xq[i] * CE;
      } else {
        k_to_tap<GE>(a, kt * BKE + xq[i] * CE, tap, c);
      }
      const int dh = tap / 3 - 1, dw = tap - (tap / 3) * 3 - 1;
      const int hh = ph[i] + dh, ww = pw[i] + dw;
      const bool ok = tap < 9 && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
      const int off = ok ? ((prow[i] + dh * W + dw) * xcs + c) * (int)sizeof(T) : OOB;
      glds16(xrs, sbase + (wave + i * NW) * 1024, off);
    }
    const int kb = kt * RB;
#pragma unroll
    for (int i = 0; i < WPW; ++i)
      if (wave + i * NW < C::WP) glds16(wrs, sbase + BM * RB + (wave + i * NW) * 1024, woff[i] + kb);
  };

  f32x4 acc[FC][FP];
#pragma unroll
  for (int i = 0; i < FC; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr bool SPLIT = sizeof(T) == 4;
  auto compute = [&](int slot) {
    const char* sp = smem + slot * C::STAGE;
    f32x4 part[SPLIT ? FC : 1][SPLIT ? FP : 1];
    if constexpr (SPLIT) {
#pragma unroll
      for (int i = 0; i < FC; ++i)
#pragma unroll
        for (int j = 0; j < FP; ++j) part[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int kb = 0; kb < RB / 64; ++kb) {
      const int ck = kb * 4 + (lane >> 4);
      uint4 av[FC], bv[FP];
#pragma unroll
      for (int f = 0; f < FC; ++f)
        av[f] = *reinterpret_cast<const uint4*>(sp + BM * RB + swz<RB>(wn * 64 + f * 16 + (lane & 15), ck));
#pragma unroll
      for (int f = 0; f < FP; ++f)
        bv[f] = *reinterpret_cast<const uint4*>(sp + swz<RB>(wm * C::TPM + f * 16 + (lane & 15), ck));
#pragma unroll
      for (int fc = 0; fc < FC; ++fc)
#pragma unroll
        for (int fp = 0; fp < FP; ++fp) {
          if constexpr (SPLIT) mma16<T>(av[fc], bv[fp], part[fc][fp]);
          else mma16<T>(av[fc], bv[fp], acc[fc][fp]);
        }
    }
    if constexpr (SPLIT) {
#pragma unroll
      for (int i = 0; i < FC; ++i)
#pragma unroll
        for (int j = 0; j < FP; ++j) acc[i][j] += part[i][j];
    }
  };

  const int nk = a.nk;
#pragma unroll
  for (int s = 0; s < S - 1; ++s)
    if (s < nk) issue(s, s);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // stage kt has landed once only the min(S-2, nk-1-kt) younger stages are still in flight
    wait_vm(min(S - 2, nk - 1 - kt) * lps);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (fragment reads of the slot refilled below: see conv3x3_patch)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + S - 1 < nk) {
      int ns = slot + S - 1;
      ns -= ns >= S ? S : 0;
      issue(kt + S - 1, ns);
    }
    compute(slot);
    slot = slot + 1 == S ? 0 : slot + 1;
  }

  // ---------------------------------------------------------------- epilogue, one 64-channel slab at a time
  constexpr int SROW = 64 + 4;
  float* stg = reinterpret_cast<float*>(smem);
  for (int sl = 0; sl < WN; ++sl) {
    asm volatile("" ::: "memory");
    __syncthreads();
    if (wn == sl) {
#pragma unroll
      for (int fc = 0; fc < FC; ++fc) {
        const int col = fc * 16 + 4 * (lane >> 4);
        float bsv[4] = {0.f, 0.f, 0.f, 0.f}, scv[4] = {1.f, 1.f, 1.f, 1.f}, shv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = min(n0 + wn * 64 + col + j, a.cout - 1);
          if (a.bias) bsv[j] = a.bias[co];
          if (a.scale) scv[j] = a.scale[co];
          if (a.shift) shv[j] = a.shift[co];
        }
#pragma unroll
        for (int fp = 0; fp < FP; ++fp) {
          const int row = wm * C::TPM + fp * 16 + (lane & 15);
          float4 v;
          float* vv = reinterpret_cast<float*>(&v);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float tv = (acc[fc][fp][j] + bsv[j]) * scv[j] + shv[j];
            if (a.act == VM_ACT_RELU) tv = tv > 0.f ? tv : 0.f;
            else if (a.act == VM_ACT_SIGMOID) tv = sigmoid_precise(tv);
            vv[j] = tv;
          }
          *reinterpret_cast<float4*>(stg + row * SROW + col) = v;
        }
      }
    }
    __syncthreads();
    const int nb = n0 + sl * 64;
    if (a.y_dtype == VM_BF16) {
      uint16_t* Y = reinterpret_cast<uint16_t*>(a.y) + a.y_coff;
      for (int idx = tid; idx < BM * 8; idx += NT) {
        const int rr = idx >> 3, cc = idx & 7;
        const long p = m0 + rr;
        const int co = nb + cc * 8;
        if (p >= a.M || co >= a.cout) continue;
        const float* src = stg + rr * SROW + cc * 8;
        uint16_t* dst = Y + p * (long)a.y_cstride + co;
        if (a.y_vec && co + 8 <= a.cout) *reinterpret_cast<uint4*>(dst) = Chunk<uint16_t>::pack(src);
        else
          for (int j = 0; j < 8 && co + j < a.cout; ++j) dst[j] = f2bf(src[j]);
      }
    } else {
      float* Y = reinterpret_cast<float*>(a.y) + a.y_coff;
      for (int idx = tid; idx < BM * 16; idx += NT) {
        const int rr = idx >> 4, cc = idx & 15;
        const long p = m0 + rr;
        const int co = nb + cc * 4;
        if (p >= a.M || co >= a.cout) continue;
        const float* src = stg + rr * SROW + cc * 4;
        float* dst = Y + p * (long)a.y_cstride + co;
        if (a.y_vec && co + 4 <= a.cout) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
        else
          for (int j = 0; j < 4 && co + j < a.cout; ++j) dst[j] = src[j];
      }
    }
  }
}

// ================================================================ dispatch
thread_local char g_last_kernel[128];  // (conv_dispatch.h)
ConvOptions g_opt;
template <typename T>
static const char* tname() { return sizeof(T) == 2 ? "unsigned short" : "float"; }

template <typename T, int BM, int BN>
static int launch_mfma(ConvArgs& a, hipStream_t st) {
  constexpr int lds = mfma_lds_bytes<BM, BN>();
  static bool attr_set = false;  // idempotent; benign race
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_mfma<T, BM, BN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return fail(VM_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    attr_set = true;
  }
  a.nk = a.K_pad / (128 / (int)sizeof(T));
  a.tiles_n = (a.cout + BN - 1) / BN;
  a.tiles_total = (int)((a.M + BM - 1) / BM) * a.tiles_n;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_mfma<%s, %d, %d>", tname<T>(), BM, BN);
  hipLaunchKernelGGL((conv3x3_mfma<T, BM, BN>), dim3(a.tiles_total), dim3(256), lds, st, a);
  return check_launch("conv3x3_mfma");
}

template <typename T, int RB, int BM, int BN, int WM, int WN, int S, bool FAST>
static int launch_glds(ConvArgs& a, hipStream_t st) {
  using C = GldsCfg<T, RB, BM, BN, WM, WN, S>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_glds<T, RB, BM, BN, WM, WN, S, FAST>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS);
    if (e != hipSuccess) return fail(VM_EHIP, "hipFuncSetAttribute(glds): %s", hipGetErrorString(e));
    attr_set = true;
  }
  const int bke = RB / (int)sizeof(T);
  a.nk = (FAST && RB == 64) ? a.ng : a.K_pad / bke;
  a.tiles_n = (a.cout + BN - 1) / BN;
  a.tiles_total = (int)((a.M + BM - 1) / BM) * a.tiles_n;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_glds<%s, %d, %d, %d, %d, %d, %d, %s>", tname<T>(), RB,
           BM, BN, WM, WN, S, FAST ? "true" : "false");
  hipLaunchKernelGGL((conv3x3_glds<T, RB, BM, BN, WM, WN, S, FAST>), dim3(a.tiles_total), dim3(C::NT), C::LDS, st,
                     a);
  return check_launch("conv3x3_glds");
}

template <typename T, bool FAST>
static int dispatch_glds(ConvArgs& a, hipStream_t st) {
  if constexpr (sizeof(T) == 2) {
    if (a.cout > 128) {
      if (g_opt.glds_rb == 64) return launch_glds<T, 64, 256, 256, 2, 4, 4, FAST>(a, st);
      return launch_glds<T, 128, 256, 256, 2, 4, 2, FAST>(a, st);
    }
  }
  if (a.cout > 64) return launch_glds<T, 64, 256, 128, 4, 2, 6, FAST>(a, st);
  return launch_glds<T, 64, 512, 64, 8, 1, 4, FAST>(a, st);
}

template <typename T>
static int dispatch_mfma(ConvArgs& a, hipStream_t st, int cin = 0) {
  // f32 refine conv + softmax (cin <= 8 of a 16-byte-aligned 8-float pixel, 64 outputs, f32 out)
  if (sizeof(T) == 4 && g_opt.softmax_kernel != 0 && g_opt.conv_kernel != 1 && g_opt.conv_kernel != 2 && cin > 0 && cin <= 8 &&
      a.cin_pad == 8 && !a.chunk_major && a.x_src_c <= 0 && a.y_dtype == VM_F32 && a.y_vec && a.act == VM_ACT_SOFTMAX &&
      a.cout == 64 && a.K_pad == 96 && a.x_cstride % 4 == 0 && a.x_coff % 4 == 0 &&
      reinterpret_cast<uintptr_t>(a.x) % 16 == 0)
    return launch_first_softmax_f32(a, cin, st);
  if (sizeof(T) == 2 && g_opt.softmax_kernel != 0 && g_opt.conv_kernel != 1 && g_opt.conv_kernel != 2 && a.cin_pad == 8 &&
      !a.chunk_major && a.x_src_c <= 0 && a.y_dtype == VM_F32 && a.y_vec && a.act == VM_ACT_SOFTMAX && a.cout == 64 &&
      a.K_pad == 128)
    return launch_first_softmax(a, st);
  if (sizeof(T) == 2 && g_opt.conv_kernel != 1 && g_opt.conv_kernel != 2 && a.cin_pad == 8 && !a.chunk_major && a.x_src_c <= 0 &&
      a.y_dtype == VM_BF16 && a.y_vec && a.act != VM_ACT_SOFTMAX && (a.cout & 7) == 0 && a.K_pad == 128)
    return launch_first(a, st);
  if ((g_opt.conv_kernel == 0 || g_opt.conv_kernel == 3) && patch_ok(a, sizeof(T))) return dispatch_patch(a, st);
  if (g_opt.conv_kernel != 1 && a.act != VM_ACT_SOFTMAX && a.x_src_c <= 0) {
    // measured (tools/convbench.py): the LDS-DMA kernel wins for cout >= 256 (256x256 tiles); for
    // cout <= 128 its 64-channel-wide waves are DMA-issue-bound and the register-staged kernel is faster
    const int bm = a.cout > 64 ? 256 : 512;
    const long tiles = ((a.M + bm - 1) / bm) * ((a.cout + 255) / 256);
    const bool wide = sizeof(T) == 2 && a.cout > 128;
    if (g_opt.conv_kernel == 2 || (wide && tiles >= g_opt.conv_min_tiles))
      return a.chunk_major ? dispatch_glds<T, true>(a, st) : dispatch_glds<T, false>(a, st);
  }
  if (a.cout <= 64) return launch_mfma<T, 256, 64>(a, st);
  return launch_mfma<T, 128, 128>(a, st);
}

// every key of g_opt; the shipped library has neither the study-only keys nor the study tilings' values.  A value is
// accepted if any entry of its key accepts it.
static const OptDef conv_options[] = {
    {"conv_kernel", &g_opt.conv_kernel, OPT_RANGE, 2, {0, 3}},
    {"softmax_kernel", &g_opt.softmax_kernel, OPT_RANGE, 2, {0, 6}},
    {"softmax_blocks", &g_opt.softmax_blocks, OPT_RANGE, 2, {1, 1 << 20}},
    {"head_th", &g_opt.head_th, OPT_SET, 2, {8, 16}},
    {"softmax_f32p", &g_opt.softmax_f32p, OPT_RANGE, 2, {0, 7}},
    {"cband", &g_opt.cband, OPT_RANGE, 2, {0, 2}},
    {"ngroup", &g_opt.ngroup, OPT_RANGE, 2, {0, 64}},
    {"cband_bytes", &g_opt.cband_bytes, OPT_ANY},
    {"rows_kernel", &g_opt.rows_kernel, OPT_SET, 4, {0, 1, 8, 16}},
    {"pack_tiled", &g_opt.pack_tiled, OPT_ANY},
    {"persist_half", &g_opt.persist_half, OPT_ANY},
    {"rows_up", &g_opt.rows_up, OPT_ANY},
    {"rows_min_cin", &g_opt.rows_min_cin, OPT_ANY},
    {"rows_min_blocks", &g_opt.rows_min_blocks, OPT_ANY},
    {"rows_retire", &g_opt.rows_retire, OPT_RANGE, 2, {0, 1}},
    {"thin_rounds", &g_opt.thin_rounds, OPT_RANGE, 2, {0, 64}},
    {"pack_frames", &g_opt.pack_frames, OPT_RANGE, 2, {0, 1}},
    {"up_skip", &g_opt.up_skip, OPT_RANGE, 2, {0, 1}},
    {"src_span_limit", &g_opt.src_span_limit, OPT_RANGE, 2, {1, 0x7ffffff0L}},
    {"thin_blocks", &g_opt.thin_blocks, OPT_ANY},
    {"thin_th", &g_opt.thin_th, OPT_SET, 3, {4, 8, 16}},
    {"conv_prio", &g_opt.conv_prio, OPT_RANGE, 2, {0, 1}},
    {"thin_twalk", &g_opt.thin_twalk, OPT_RANGE, 2, {0, 1}},
    {"thin_rowreuse", &g_opt.thin_rowreuse, OPT_RANGE, 2, {0, 1}},
    {"thin_dma", &g_opt.thin_dma, OPT_RANGE, 2, {0, 4}},  // 0: conv3x3_thin; 1..4: conv3x3_thin_dma configs
    {"thin_dma_rounds", &g_opt.thin_dma_rounds, OPT_RANGE, 2, {1, 64}},
    {"narrowin_kernel", &g_opt.narrowin_kernel, OPT_RANGE, 2, {0, 1}},
    {"thin_kernel", &g_opt.thin_kernel, OPT_RANGE, 2, {0, 1}},
    {"conv_min_tiles", &g_opt.conv_min_tiles, OPT_ANY},
#ifdef VM_STUDY
    {"patch_cfg", &g_opt.patch_cfg, OPT_RANGE, 2, {0, 31}},
    {"patch_ablate", &g_opt.patch_ablate, OPT_ANY},  // timing-only ablations: garbage results
    {"rows_ablate", &g_opt.rows_ablate, OPT_RANGE, 2, {0, 2}},  // timing-only ablations of conv3x3_rows' epilogue
    {"softmax_abl", &g_opt.softmax_abl, OPT_ANY},    // timing-only ablations of the f32 refine kernel
    {"patch_rowslot", &g_opt.patch_rowslot, OPT_RANGE, 2, {0, 1}},
    {"pair_strip_abl", &g_opt.pair_strip_abl, OPT_ANY},  // timing-only ablations of the strip pair kernel
    {"pair_kernel", &g_opt.pair_kernel, OPT_RANGE, 2, {0, 1}},
    {"pair_kernel", &g_opt.pair_kernel, OPT_RANGE, 2, {10, 18}},  // conv3x3_pair_persist's timing ablations
#else
    {"patch_cfg", &g_opt.patch_cfg, OPT_SET, 5, {0, 19, 22, 25, 30}, " (other tilings: the study build)"},
    {"pair_kernel", &g_opt.pair_kernel, OPT_RANGE, 2, {0, 1}, " (ablations: the study build)"},
#endif
    {"pair_xin_wide", &g_opt.pair_xin_wide, OPT_RANGE, 2, {0, 1}},
    {"border_ks", &g_opt.border_ks, OPT_SET, 3, {1, 2, 4}},
    {"border_fuse", &g_opt.border_fuse, OPT_RANGE, 2, {0, 2}},
    {"patch_repi", &g_opt.patch_repi, OPT_RANGE, 2, {0, 1}},
    {"persist_rounds", &g_opt.persist_rounds, OPT_RANGE, 2, {0, 64}, " (0: any grid)"},
    {"persist_up_rounds", &g_opt.persist_up_rounds, OPT_RANGE, 2, {0, 64}, " (0: any grid)"},
    {"persist_all", &g_opt.persist_all, OPT_RANGE, 2, {0, 2}},
    {"persist_rot", &g_opt.persist_rot, OPT_RANGE, 2, {0, 2}},
    {"up_skip_mask", &g_opt.up_skip_mask, OPT_RANGE, 2, {0, 3}},
    {"patch_persist", &g_opt.patch_persist, OPT_RANGE, 2, {0, 1}},
    {"pair_strip_pin", &g_opt.pair_strip_pin, OPT_RANGE, 2, {0, 1}},
    {"pair_strip", &g_opt.pair_strip, OPT_RANGE, 2, {0, 1}},
    {"head_kernel", &g_opt.head_kernel, OPT_RANGE, 2, {0, 2}},
    {"splitk_tiles", &g_opt.splitk_tiles, OPT_ANY},
    {"glds_rb", &g_opt.glds_rb, OPT_SET, 2, {64, 128}},
    {nullptr},
};
}  // namespace vm

using namespace vm;

// VM_OK / VM_EINVAL, or 1 when the table has no entry for the key
static int set_from(const OptDef* t, const char* key, long value) {
  char want[160] = "";
  const char* note = "";
  for (; t->key; ++t) {
    if (strcmp(key, t->key)) continue;
    bool ok = t->kind == OPT_ANY || (t->kind == OPT_RANGE && value >= t->v[0] && value <= t->v[1]);
    for (int i = 0; t->kind == OPT_SET && i < t->n; ++i) ok = ok || value == t->v[i];
    if (ok) {
      *t->value = value;
      return VM_OK;
    }
    size_t len = strlen(want);
    if (len) len += snprintf(want + len, sizeof want - len, " or ");
    if (t->kind == OPT_RANGE) snprintf(want + len, sizeof want - len, "%ld..%ld", t->v[0], t->v[1]);
    for (int i = 0; t->kind == OPT_SET && i < t->n && len < sizeof want; ++i)
      len += snprintf(want + len, sizeof want - len, i == 0 ? "%ld" : i + 1 < t->n ? ", %ld" : " or %ld", t->v[i]);
    if (t->note) note = t->note;
  }
  return want[0] ? fail(VM_EINVAL, "set_option: %s must be %s%s", key, want, note) : 1;
}

extern "C" int vm_set_option(const char* key, long value) {
  if (!key) return fail(VM_EINVAL, "set_option: NULL key");
  for (const OptDef* t : {conv_options, bn_options, train_options, wgrad_options, flow_options}) {
    const int rc = set_from(t, key, value);
    if (rc != 1) return rc;
  }
  return fail(VM_EINVAL, "set_option: unknown key '%s'", key);
}

extern "C" const char* vm_conv3x3_last_kernel(void) { return g_last_kernel; }

static int conv_impl(const ConvCall& c);

extern "C" int vm_conv3x3_nhwc(const vm_tensor* x, const void* packed, int cin, int cout, const float* bias,
                               const float* scale, const float* shift, int act, vm_tensor* y, void* stream) {
  return conv_impl({x, packed, cin, cout, bias, scale, shift, act, y, stream});
}

extern "C" int vm_conv3x3_sources_nhwc(const vm_tensor* x, int nsrc, long src_stride, const void* packed, int cin,
                                       int cout, const float* bias, const float* scale, const float* shift, int act,
                                       vm_tensor* y, void* stream) {
  if (nsrc < 1 || (nsrc > 1 && src_stride <= 0)) return fail(VM_EINVAL, "conv3x3_sources: nsrc %d stride %ld", nsrc,
                                                            src_stride);
  ConvCall c{x, packed, cin, cout, bias, scale, shift, act, y, stream};
  c.nsrc = nsrc;
  c.src_stride = src_stride;
  return conv_impl(c);
}

extern "C" int vm_conv3x3_pool_nhwc(const vm_tensor* x, const void* packed, int cin, int cout, const float* bias,
                                    const float* scale, const float* shift, int act, vm_tensor* y, vm_tensor* ypool,
                                    void* stream) {
  if (!valid_tensor(ypool) || !y) return fail(VM_EINVAL, "conv3x3_pool: invalid pool tensor");
  if (ypool->n != y->n || ypool->h != (y->h + 1) / 2 || ypool->w != (y->w + 1) / 2 || ypool->c != cout ||
      ypool->dtype != y->dtype)
    return fail(VM_EINVAL, "conv3x3_pool: pool output must be [n, ceil(h/2), ceil(w/2), cout] in the output dtype");
  ConvCall c{x, packed, cin, cout, bias, scale, shift, act, y, stream};
  c.yp = ypool;
  return conv_impl(c);
}

extern "C" int vm_conv3x3_head_acc_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias,
                                        const float* y_acc, vm_tensor* y, float* alpha, void* stream) {
  if (!y_acc) return fail(VM_EINVAL, "conv3x3_head_acc: y_acc is NULL");
  ConvCall c{x, packed, cin, 1, bias, nullptr, nullptr, VM_ACT_NONE, y, stream};
  c.y2 = alpha;
  c.y_acc = y_acc;
  return conv_impl(c);
}

extern "C" int vm_conv3x3_head_acc_ex_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias,
                                           const float* scale, const float* shift, const float* y_acc, vm_tensor* y,
                                           float* alpha, void* stream) {
  ConvCall c{x, packed, cin, 1, bias, scale, shift, VM_ACT_NONE, y, stream};
  c.y2 = alpha;
  c.y_acc = y_acc;
  return conv_impl(c);
}

extern "C" int vm_conv3x3_split3_nhwc(const vm_tensor* x, const void* packed, int cin, int cout, const float* bias,
                                      const float* scale, const float* shift, int act, vm_tensor* y, int y_slab,
                                      vm_tensor* ypool, int pool_slab, int* overflow, void* work, size_t work_bytes,
                                      void* stream) {
  if (!x || !y || !valid_tensor(y, true) || (ypool && !valid_tensor(ypool, true)))
    return fail(VM_EINVAL, "conv3x3_split3: invalid tensor");
  SplitOut so{y_slab > 0 ? y_slab : y->cstride / 2, 0, overflow};
  if (cout % 8 || !split3_view_ok(y, so.yslab, cout))
    return fail(VM_EUNSUPPORTED, "conv3x3_split3: y must be an fp16 view of cout %% 8 == 0 channels inside the first "
                                 "of two (or three) slabs of S %% 8 == 0 channels, 16-byte aligned");
  if (ypool) {
    so.pslab = pool_slab > 0 ? pool_slab : ypool->cstride / 2;
    if (!split3_view_ok(ypool, so.pslab, cout) || ypool->n != y->n || ypool->h != (y->h + 1) / 2 ||
        ypool->w != (y->w + 1) / 2 || ypool->c != cout)
      return fail(VM_EINVAL, "conv3x3_split3: pool view must be [n, ceil(h/2), ceil(w/2), cout] in the split layout");
  }
  ConvCall c{x, packed, cin, cout, bias, scale, shift, act, y, stream};
  c.yp = ypool;
  c.work = work;
  c.work_bytes = work_bytes;
  c.so = &so;
  return conv_impl(c);
}

extern "C" int vm_conv3x3_head_partial_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias,
                                            const float* scale, const float* shift, int act, vm_tensor* y,
                                            float* alpha, const float* partial, void* stream) {
  if (!partial) return fail(VM_EINVAL, "conv3x3_head_partial: partial is NULL");
  ConvCall c{x, packed, cin, 1, bias, scale, shift, act, y, stream};
  c.y2 = alpha;
  c.head_part = partial;
  return conv_impl(c);
}

extern "C" int vm_conv3x3_head_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias,
                                    const float* scale, const float* shift, int act, vm_tensor* y, float* alpha,
                                    void* stream) {
  ConvCall c{x, packed, cin, 1, bias, scale, shift, act, y, stream};
  c.y2 = alpha;
  return conv_impl(c);
}

static int conv_impl(const ConvCall& c) {
  const vm_tensor* x = c.x;
  vm_tensor* y = c.y;
  const int cin = c.cin, cout = c.cout;
  if (!valid_tensor(x, true) || !valid_tensor(y, c.so != nullptr) || !c.packed)
    return fail(VM_EINVAL, "conv3x3: invalid tensor/weights");
  // fp16 operands (the split-fp16 forward, vmatting/split3.py): f32 outputs of the patch kernel (any cout % 4 == 0)
  // or the MFMA head (cout == 1, <= 256 channels per call), or (so) the split-fp16 output with its fused pool; no
  // split sources or softmax
  const bool f16 = x->dtype == VM_F16;
  if (c.so && (!f16 || y->dtype != VM_F16 || cout == 1))
    return fail(VM_EINVAL, "conv3x3_split3: fp16 input and fp16 split output views, cout > 1");
  if (f16 && ((!c.so && (y->dtype != VM_F32 || c.yp)) || c.nsrc > 1 || c.act == VM_ACT_SOFTMAX || c.head_part))
    return fail(VM_EUNSUPPORTED, "conv3x3: fp16 operands need an f32 (or split) output without sources / softmax");
  if (c.y_acc && cout != 1) return fail(VM_EINVAL, "conv3x3: an accumulated pre-activation needs cout == 1");
  if (c.head_part && cout != 1) return fail(VM_EINVAL, "conv3x3: head partials need cout == 1");
  int xc = c.nsrc > 1 ? c.nsrc * x->c : x->c;  // sources: x is the view of source 0
  // split-fp16 input stored as two slabs [l, h] (x->c = 2S) for a filter over [l, h, h] (cin = 3S): the third slab is
  // read from the second (ConvArgs::xalias)
  int xalias = 0;
  if (x->dtype == VM_F16 && c.nsrc <= 1 && 2 * cin == 3 * x->c && x->c % 64 == 0) {
    xalias = x->c / 2;
    xc = cin;
  }
  if (cin <= 0 || cout <= 0 || xc != cin || y->c != cout)
    return fail(VM_EINVAL, "conv3x3: channel mismatch x.c=%d cin=%d y.c=%d cout=%d", xc, cin, y->c, cout);
  if (c.nsrc > 1 && (cout == 1 || c.yp || x->c % (x->dtype == VM_BF16 ? 32 : 16) || c.src_stride % 8))
    return fail(VM_EUNSUPPORTED, "conv3x3: split sources need whole 64-byte granules per source (x.c=%d)", x->c);
  if (x->n != y->n || x->h != y->h || x->w != y->w)
    return fail(VM_EINVAL, "conv3x3: spatial mismatch [%d,%d,%d] vs [%d,%d,%d]", x->n, x->h, x->w, y->n, y->h, y->w);
  if (c.act < VM_ACT_NONE || c.act > VM_ACT_SOFTMAX) return fail(VM_EINVAL, "conv3x3: act %d", c.act);
  const int dt = x->dtype;
  PackGeom g = geom(cin, cout, dt);
  if (!view16_ok(x) || x->coff + (c.nsrc > 1 || xalias ? x->c : g.cin_pad) > x->cstride)
    return fail(VM_EUNSUPPORTED,
                "conv3x3: input view must be 16-byte aligned with channel padding to %d (coff=%d cstride=%d)",
                g.cin_pad, x->coff, x->cstride);
  if (c.act == VM_ACT_SOFTMAX && cout > 128) return fail(VM_EUNSUPPORTED, "conv3x3: fused softmax needs cout <= 128");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  const long M = (long)x->n * x->h * x->w;
  if (c.yp && cout == 1) return fail(VM_EUNSUPPORTED, "conv3x3_pool: no fused pooling for cout == 1");

  if (cout == 1) return dispatch_head(c, g, xalias, M, st);

  ConvArgs a{};
  a.x = x->ptr; a.x_cstride = x->cstride; a.x_coff = x->coff; a.H = x->h; a.W = x->w; a.M = M;
  fill_geom(a, g);
  if (c.nsrc > 1) {
    a.x_src_c = x->c;
    a.x_src_stride = c.src_stride;
  }
  a.ksplit = 1;
  a.w = c.packed; a.cout = cout;
  a.bias = c.bias; a.scale = c.scale; a.shift = c.shift; a.act = c.act;
  a.y = y->ptr; a.y_cstride = y->cstride; a.y_coff = y->coff; a.y_dtype = y->dtype;
  a.y_vec = view16_ok(y);
  if (c.yp && !f16) {
    if (cout == 1 || dt != VM_BF16 || !view16_ok(c.yp, 8) || !patch_ok(a, 2) || g_opt.conv_kernel == 1 || g_opt.conv_kernel == 2)
      return fail(VM_EUNSUPPORTED, "conv3x3_pool: fused pooling needs the bf16 patch kernel");
    a.py = c.yp->ptr;
    a.py_cstride = c.yp->cstride;
    a.py_coff = c.yp->coff;
    return dispatch_patch(a, st);
  }
  if (f16) {  // the patch kernel's fp16 form (+ split-K on small grids with a workspace)
    a.f16 = 1;
    a.xalias = xalias;
    a.py = nullptr;
    a.up = 0;
    if (c.so) {  // split output: staged like an f32 output, stored as fp16 slabs (y_cstride stays in fp16 elements)
      a.y_dtype = VM_F32;
      a.y_vec = 1;
      a.ysplit = c.so->yslab;
      a.ovf = c.so->ovf;
      if (c.yp) {
        a.py = c.yp->ptr;
        a.py_cstride = c.yp->cstride;
        a.py_coff = c.yp->coff;
        a.psplit = c.so->pslab;
      }
    }
    if (!patch_ok(a, 2)) return fail(VM_EUNSUPPORTED, "conv3x3: fp16 operands need the patch kernel (cin %% 32 == 0)");
    if (c.work && (cout & 3) == 0 && !c.yp) {
      const int ks = splitk_plan(x->n, x->h, x->w, a.cin_pad, cout);
      if (ks > 1 && c.work_bytes >= (size_t)ks * M * cout * sizeof(float)) {
        a.ksplit = ks;
        a.part = reinterpret_cast<float*>(c.work);
      }
    }
    return dispatch_patch(a, st);
  }
  if (g_opt.conv_kernel == 0 && thin_ok(dt, g, cout, a.x_src_c, c.act, x)) {
    const int ks = c.work ? thin_splitk_plan(x->n, x->h, x->w, a.cin_pad) : 1;
    if (ks > 1 && c.work_bytes >= (size_t)ks * M * cout * sizeof(float)) {
      a.ksplit = ks;
      a.part = reinterpret_cast<float*>(c.work);
    }
    return dispatch_thin(a, x->n, st);
  }
  if (c.nsrc > 1) {
    // the patch / row-stationary / generic kernels add source s's offset (s * src_stride elements) into 32-bit
    // byte offsets inside one image's buffer resource: the whole span must stay below it (the thin kernel above
    // forms 64-bit source pointers).  Callers materialise the concat instead (ops.conv3x3)
    const long span = ((long)(c.nsrc - 1) * c.src_stride + (long)x->h * x->w * x->cstride) * elem_bytes(dt);
    if (span >= g_opt.src_span_limit)
      return fail(VM_EUNSUPPORTED, "conv3x3: split sources span %ld bytes (limit %ld): materialise the concat", span,
                  g_opt.src_span_limit);
  }
  if (dt == VM_BF16 && c.work && g_opt.conv_kernel == 0 && patch_ok(a, 2) && (cout & 3) == 0) {
    const int ks = splitk_plan(x->n, x->h, x->w, a.cin_pad, cout);
    if (ks > 1 && c.work_bytes >= (size_t)ks * M * cout * sizeof(float)) {
      a.ksplit = ks;
      a.part = reinterpret_cast<float*>(c.work);
      return dispatch_patch(a, st);
    }
  }
  if (dt == VM_BF16 && g_opt.conv_kernel == 0 && narrowin_ok(a, g, cout, c.act, x, y)) return launch_narrowin(a, x->n, g, st);
  if (dt == VM_BF16) return dispatch_mfma<uint16_t>(a, st);
  return dispatch_mfma<float>(a, st, cin);
}

// workspace of vm_conv3x3_ex_nhwc: the split-K partial sums of a small-grid bf16 conv, else 0
extern "C" size_t vm_conv3x3_workspace_bytes(const vm_tensor* x, int cin, int cout) {
  if (!x || (x->dtype != VM_BF16 && x->dtype != VM_F16) || cin <= 0 || cout <= 0) return 0;
  const PackGeom g = geom(cin, cout, VM_BF16);
  if (x->dtype == VM_BF16 && g_opt.conv_kernel == 0 && thin_ok(VM_BF16, g, cout, cin == x->c ? 0 : x->c, VM_ACT_NONE, x)) {
    const int ks = thin_splitk_plan(x->n, x->h, x->w, g.cin_pad);
    return ks > 1 ? (size_t)ks * x->n * x->h * x->w * cout * sizeof(float) : 0;
  }
  if (cout & 3) return 0;
  if (!g.chunk_major || g.cin_pad % 32) return 0;
  const int ks = splitk_plan(x->n, x->h, x->w, g.cin_pad, cout);
  return ks > 1 ? (size_t)ks * x->n * x->h * x->w * cout * sizeof(float) : 0;
}

extern "C" int vm_conv3x3_ex_nhwc(const vm_tensor* x, int nsrc, long src_stride, const void* packed, int cin, int cout,
                                  const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                                  void* work, size_t work_bytes, void* stream) {
  if (nsrc < 0 || (nsrc > 1 && src_stride <= 0)) return fail(VM_EINVAL, "conv3x3_ex: nsrc %d stride %ld", nsrc,
                                                            src_stride);
  ConvCall c{x, packed, cin, cout, bias, scale, shift, act, y, stream};
  c.nsrc = nsrc;
  c.src_stride = src_stride;
  c.work = work;
  c.work_bytes = work_bytes;
  return conv_impl(c);
}
