// Border pass of the folded 2x upconv (conv_up2x.hip has the fold itself): the argument block and the device body,
// which conv3x3_up2x_border runs as a kernel of its own and the folded patch kernels (conv_patch.hip) run in extra
// blocks of their own launch (ConvArgs::bfuse).
#pragma once

#include "conv_common.h"

namespace vm {

struct BorderArgs {
  const void* x;  // low-res [N,H,W,cin] bf16 view
  int x_cstride, x_coff, H, W, nframes;
  const void* w;  // plain packed filter (chunk-major bf16)
  int K_pad, cout, nch;
  const float* bias;
  const float* scale;
  const float* shift;
  int act;
  void* y;  // [N,2H,2W,cout] bf16 view
  int y_cstride, y_coff;
  int nb;  // border pixels per frame
  float* hd;        // head split (cout == 64): per-tap head shares of the border pixels, as the conv's epilogue
  const float* hw;  // conv1_5 HWIO f32 [3,3,hw_cin,1]
  int hw_cin, hw_coff, y_skip;
  // SPL (split-fp16 x3, vm_conv3x3_up2x_split3_nhwc): x is the low-res split input [l, h] (xs channels per slab; the
  // K granules run over [l, h, h], nch = 3 xs / 32); y the split output (slab ysplit); ovf as ConvArgs::ovf
  int xs, ysplit;
  int* ovf;
};

// LDS of one 4-wave group of the border pass: two staging buffers [tap][pixel][32 ch] and its partial sums
constexpr int BORDER_STG = 9 * 16 * 64, BORDER_RED = 16 * 64 * 4, BORDER_LDS = 2 * BORDER_STG + BORDER_RED;

// 8 fp16 values of a 16-byte chunk -> f32
__device__ __forceinline__ void unpack_f16x8(uint4 u, float* f) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xffffu));
    f[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
  }
}

__device__ __forceinline__ uint4 sel3(int i, uint4 a, uint4 b, uint4 c) { return i == 0 ? a : (i == 1 ? b : c); }

// Border pixels of the folded upconv, computed the unfused way: the 9 resized taps (TF1 legacy bilinear in f32,
// rounded to bf16 as vm_resize_bilinear_tf1_nhwc stores them; zero outside the 2H x 2W frame) of 16 pixels are
// staged per 32-channel granule and consumed by MFMAs.  The pass is latency-bound (a few hundred blocks; each granule
// costs a round trip for its gathers), so a 1024-thread block splits the granules 4 ways (wave w: output channels
// 16 (w & 3) .. +15, granules (w >> 2), (w >> 2) + 4, ...: each 4-wave group stages and consumes its own granules,
// double-buffered, with one LDS-only barrier per step) and adds the 4 partial sums in a fixed order at the end.
//
// The body of one block: 256 * BD_KS threads (tid), the 16 border pixels from b0 of the pixel list, output channels
// cob .. cob + 63; stg = BD_KS x 2 staging buffers of BORDER_STG bytes, red = BD_KS x 16 x 64 partial sums.  Every
// thread of the block reaches every barrier whatever b0 (past the list: nothing is loaded or stored).
//
// SPL: the split-fp16 x3 form (the folded upconvs of vmatting/split3.py): each staged value is the resize of the f32
// activation x = h + l (exact in f32), split again into fp16 (h', l'); K granule cc stages l' (slab 0) or h' (slabs 1,
// 2) for the fp16 filter parts [Wh, Wl, Wh]; the output is written split (ConvArgs::ysplit's layout)
//
// LEAN (BD_KS == 1; the folded patch kernels' blocks, which hold to 128 VGPRs): a granule's gathers and filter
// fragments are loaded in its own step instead of one step ahead, so one set of each is live; the granule and tap
// order of every output, and so every bit of it, are those of BD_KS == 1.  Several 256-thread groups may share a block
// (tid is the thread's index in its group, stg / red the group's own): the barriers are the block's.
template <int BD_KS, bool SPL, bool LEAN>
__device__ __forceinline__ void up2x_border_body(const BorderArgs& a, char* stg, float* red, int tid, long b0, int cob) {
  using T = uint16_t;
  using MT = std::conditional_t<SPL, f16_t, uint16_t>;
  static_assert(!LEAN || (BD_KS == 1 && !SPL), "the lean form is the bf16 one-group pass");
  const int lane = tid & 63, wave = tid >> 6;
  const int cg = wave & 3, ks = wave >> 2, gt = tid & 255;  // channel group, granule split, thread in the split group
  const int OH = 2 * a.H, OW = 2 * a.W;
  const long total = (long)a.nframes * a.nb;
  auto decode = [&](long b, int& n, int& oy, int& ox) {
    n = (int)(b / a.nb);
    const int r = (int)(b - (long)n * a.nb);
    if (r < OW) { oy = 0; ox = r; }
    else if (r < 2 * OW) { oy = OH - 1; ox = r - OW; }
    else if (r < 2 * OW + OH - 2) { oy = r - 2 * OW + 1; ox = 0; }
    else { oy = r - 2 * OW - (OH - 2) + 1; ox = OW - 1; }
  };
  const T* xb = reinterpret_cast<const T*>(a.x) + a.x_coff;
  const T* wb = reinterpret_cast<const T*>(a.w);
  // staging role inside the split group: thread (px, q, dh) builds taps (dh, 0..2) of pixel px for channels 8q..8q+7
  // of the granule; its resized row oy + dh - 1 blends low-res rows y0, y1, whose columns x0c .. x0c+2 cover the taps
  const int spx = gt & 15, sq = (gt >> 4) & 3, sdh = gt >> 6;  // sdh == 3: no staging work
  int pn = 0, oy = 0, ox = 0;
  const bool live = b0 + spx < total && sdh < 3;
  if (b0 + spx < total) decode(b0 + spx, pn, oy, ox);
  const int ry = oy + sdh - 1;
  const bool rok = live && (unsigned)ry < (unsigned)OH;
  const float sy = (float)max(ry, 0) * 0.5f;
  const float fy0 = floorf(sy);
  const int y0 = (int)fy0, y1 = min(y0 + 1, a.H - 1);
  const float ly = sy - fy0;
  int cx0 = max(ox - 1, 0) >> 1;
  const T* xr = xb + ((long)pn * a.H) * a.W * (long)a.x_cstride + sq * 8;
  // SPL: granule cc of [l, h, h] reads input channels (cc mod xs/32) * 32 of both stored slabs (l at 0, h at xs)
  const int sg = SPL ? a.xs / 32 : 1;
  auto gather = [&](int cc, uint4 (&g)[SPL ? 12 : 6]) __attribute__((always_inline)) {
    const int cin0 = SPL ? (cc % sg) * 32 : cc * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int yy = i ? y1 : y0, xx = min(cx0 + j, a.W - 1);
        // (LEAN: 32-bit element offsets inside the frame, host-checked, so no 64-bit address is held per tap)
        const T* p = LEAN ? xr + ((yy * a.W + xx) * a.x_cstride + cin0) : xr + ((long)yy * a.W + xx) * a.x_cstride + cin0;
        const bool ok = rok && cc < a.nch;
        g[i * 3 + j] = ok ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
        if constexpr (SPL) g[6 + i * 3 + j] = ok ? *reinterpret_cast<const uint4*>(p + a.xs) : make_uint4(0, 0, 0, 0);
      }
  };
  auto stage = [&](const uint4 (&g)[SPL ? 12 : 6], char* dst, int cc) __attribute__((always_inline)) {
    if (sdh >= 3) return;
    // SPL: the tap's f32 value x = h + l (exact), unpacked from both slabs
    auto unp = [&](int k, float* f) __attribute__((always_inline)) {
      if constexpr (SPL) {
        float fl[8];
        unpack_f16x8(k < 3 ? sel3(k, g[6], g[7], g[8]) : sel3(k - 3, g[9], g[10], g[11]), f);
        unpack_f16x8(k < 3 ? sel3(k, g[0], g[1], g[2]) : sel3(k - 3, g[3], g[4], g[5]), fl);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += fl[e];
      } else {
        Chunk<T>::unpack(k < 3 ? sel3(k, g[0], g[1], g[2]) : sel3(k - 3, g[3], g[4], g[5]), f);
      }
    };
#pragma unroll
    for (int dw = 0; dw < 3; ++dw) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const int rx = ox + dw - 1;
      if (rok && (unsigned)rx < (unsigned)OW) {
#pragma clang fp contract(off)
        const float sx = (float)rx * 0.5f;
        const float fx0 = floorf(sx);
        const int x0 = (int)fx0, x1 = min(x0 + 1, a.W - 1);
        const float lx = sx - fx0;
        // (top row, then bottom row: fewer values live at once, the same arithmetic)
        float l8[8], r8[8], top[8];
        unp(x0 - cx0, l8);
        unp(x1 - cx0, r8);
#pragma unroll
        for (int e = 0; e < 8; ++e) top[e] = l8[e] + (r8[e] - l8[e]) * lx;
        unp(3 + x0 - cx0, l8);
        unp(3 + x1 - cx0, r8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float bot = l8[e] + (r8[e] - l8[e]) * lx;
          o[e] = top[e] + (bot - top[e]) * ly;
        }
      }
      uint4 q;
      if constexpr (SPL) {
        uint4 hq, lq;
        split3h_chunk(o, hq, lq);
        q = cc / sg == 0 ? lq : hq;
      } else {
        q = Chunk<T>::pack(o);
      }
      *reinterpret_cast<uint4*>(dst + ((sdh * 3 + dw) * 16 + spx) * 64 + sq * 16) = q;
    }
  };
  // filter fragments of this wave's 16 output channels: A rows = channels cob + 16 cg + (lane & 15)
  const T* wrow = wb + (long)(cob + cg * 16 + (lane & 15)) * a.K_pad + (lane >> 4) * 8;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (LEAN) {
    uint4 g[6];
    gather(0, g);
#pragma unroll 1
    for (int cc = 0; cc < a.nch; ++cc) {
      char* buf = stg + (cc & 1) * BORDER_STG;
      // (opaque copies: the per-tap columns, weights and offsets derived from them are recomputed per step, not held)
      asm volatile("" : "+v"(ox), "+v"(cx0));
      stage(g, buf, cc);
      gather(cc + 1, g);  // the next granule goes in flight under this one's barrier and MFMAs
      uint4 w[9];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) w[tap] = *reinterpret_cast<const uint4*>(wrow + (cc * 9 + tap) * 32);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        mma16<MT>(w[tap], *reinterpret_cast<const uint4*>(buf + (tap * 16 + (lane & 15)) * 64 + (lane >> 4) * 16), acc);
    }
  } else {
    const int steps = (a.nch + BD_KS - 1) / BD_KS;  // every group runs the same number of steps (uniform barriers)
    uint4 g[SPL ? 12 : 6];
    gather(ks, g);
    for (int i = 0; i < steps; ++i) {
      const int cc = ks + i * BD_KS;
      char* buf = stg + (ks * 2 + (i & 1)) * BORDER_STG;
      stage(g, buf, cc);
      gather(cc + BD_KS, g);  // the group's next granule goes in flight under this one's barrier and MFMAs
      uint4 w[9];
      if (cc < a.nch) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) w[tap] = *reinterpret_cast<const uint4*>(wrow + (cc * 9 + tap) * 32);
      }
      // LDS-only barrier: __syncthreads would also wait (vmcnt(0)) for the gathers in flight
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (cc < a.nch) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
          mma16<MT>(w[tap], *reinterpret_cast<const uint4*>(buf + (tap * 16 + (lane & 15)) * 64 + (lane >> 4) * 16), acc);
      }
    }
  }
  // partial sums: lane holds channels 16 cg + 4 (lane >> 4) + j of pixel lane & 15
#pragma unroll
  for (int j = 0; j < 4; ++j) red[(ks * 16 + (lane & 15)) * 64 + cg * 16 + 4 * (lane >> 4) + j] = acc[j];
  __syncthreads();
  // one thread per (pixel, 4 channels): the splits added in order, then bias / affine / act
  const bool ew = tid < 256;
  const int ep = tid >> 4, cq = (tid & 15) * 4;
  const long b = b0 + ep;
  const bool bok = ew && b < total;
  int n = 0, ey = 0, ex = 0;
  if (bok) decode(b, n, ey, ex);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  uint2 pk = make_uint2(0, 0);
  if (ew) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float sum = red[(0 * 16 + ep) * 64 + cq + j];
#pragma unroll
      for (int k = 1; k < BD_KS; ++k) sum += red[(k * 16 + ep) * 64 + cq + j];
      const int co = cob + cq + j;
      const float sc = a.scale ? a.scale[co] : 1.f;
      v[j] = fmaf(sum, sc, (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f));
      if (a.act == VM_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
      else if (a.act == VM_ACT_SIGMOID) v[j] = sigmoid_precise(v[j]);
    }
    if constexpr (SPL) {  // [l, h(, h)] of the 4 channels
      typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
      uint32_t hw2[2], lw2[2];
      bool o = false;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const h2_t hh = {(_Float16)v[2 * k], (_Float16)v[2 * k + 1]};
        const h2_t ll = {(_Float16)(v[2 * k] - (float)hh[0]), (_Float16)(v[2 * k + 1] - (float)hh[1])};
        hw2[k] = __builtin_bit_cast(uint32_t, hh);
        lw2[k] = __builtin_bit_cast(uint32_t, ll);
        o |= !(fabsf(v[2 * k]) < 65520.f) || !(fabsf(v[2 * k + 1]) < 65520.f);
      }
      if (bok) {
        T* yo = reinterpret_cast<T*>(a.y) + (((long)n * OH + ey) * OW + ex) * (long)a.y_cstride + a.y_coff + cob + cq;
        *reinterpret_cast<uint2*>(yo) = make_uint2(lw2[0], lw2[1]);
        *reinterpret_cast<uint2*>(yo + a.ysplit) = make_uint2(hw2[0], hw2[1]);
        if (3 * a.ysplit <= a.y_cstride) *reinterpret_cast<uint2*>(yo + 2 * a.ysplit) = make_uint2(hw2[0], hw2[1]);
        if (o && a.ovf) *a.ovf = 1;
      }
    } else {
      pk.x = bf16x2_bits(v[0], v[1]);
      pk.y = bf16x2_bits(v[2], v[3]);
      if (!a.y_skip && bok)
        *reinterpret_cast<uint2*>(reinterpret_cast<T*>(a.y) + (((long)n * OH + ey) * OW + ex) * (long)a.y_cstride +
                                  a.y_coff + cob + cq) = pk;
    }
  }
  if (!SPL && a.hd) {  // (uniform: a.hd is a kernel argument; every thread reaches the barriers below)
    // the border pixel's 64 bf16 outputs -> 9 per-tap shares sum_c bf16(hw[tap][coff + c]) * y[c] (f32, in channel
    // order); taps 9..11 zero like the MFMA epilogues'
    float* vals = reinterpret_cast<float*>(stg);  // [16 pixels][64]
    float* hwl = vals + 16 * 64;                  // the head filter's 9 x 64 taps, bf16-rounded
    __syncthreads();
    if (ew) {
#pragma unroll
      for (int j = 0; j < 4; ++j) vals[ep * 64 + cq + j] = bf2f(f2bf(v[j]));
    }
    for (int i = tid; i < 9 * 64; i += 256 * BD_KS) hwl[i] = bf2f(f2bf(a.hw[(i >> 6) * a.hw_cin + a.hw_coff + (i & 63)]));
    __syncthreads();
    if (tid < 16 * 12) {
      const int pe = tid / 12, tap = tid - pe * 12;
      const long bb = b0 + pe;
      if (bb < total) {
        int pn2, py, px2;
        decode(bb, pn2, py, px2);
        float hacc = 0.f;
        if (tap < 9)
#pragma unroll 16
          for (int c = 0; c < 64; ++c) hacc = fmaf(hwl[tap * 64 + c], vals[pe * 64 + c], hacc);
        a.hd[(((long)pn2 * OH + py) * OW + px2) * 12 + tap] = hacc;
      }
    }
  }
}

// The border blocks in a folded patch kernel's own launch (ConvArgs::bfuse): block bi of them is NT / 256 independent
// 4-wave groups, group gi = bi * NT / 256 + (thread / 256) taking output channels 64 (gi % (up_cout / 64)) of the 16
// border pixels from 16 (gi / (up_cout / 64)); each group's staging is its own slice of the kernel's dynamic LDS.
template <int NT>
__device__ __forceinline__ void up2x_border_fused(const ConvArgs& a, char* smem, int bi) {
  static_assert(NT % 256 == 0, "whole 4-wave groups");
  BorderArgs b;
  b.x = a.x; b.x_cstride = a.x_cstride; b.x_coff = a.x_coff; b.H = a.H; b.W = a.W; b.nframes = a.bframes;
  b.w = a.bw; b.K_pad = a.bK_pad; b.cout = a.up_cout; b.nch = a.cin_pad / 32;
  b.bias = a.bias; b.scale = a.scale; b.shift = a.shift; b.act = a.act;
  b.y = a.y; b.y_cstride = a.y_cstride; b.y_coff = a.y_coff;
  b.nb = 4 * a.W + 2 * (2 * a.H - 2);
  b.hd = a.hd; b.hw = a.hw; b.hw_cin = a.hw_cin; b.hw_coff = a.hw_coff; b.y_skip = a.y_skip;
  b.xs = 0; b.ysplit = 0; b.ovf = nullptr;
  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8), ncob = a.up_cout / 64;
  const long gi = (long)bi * (NT / 256) + grp;
  const long pb = gi / ncob, total = (long)b.nframes * b.nb;
  // (a group past the list, in the last block: nothing to load or store, the block's barriers all the same)
  const long b0 = pb * 16 < total ? pb * 16 : total;
  const int cob = pb * 16 < total ? (int)(gi - pb * ncob) * 64 : 0;
  char* stg = smem + grp * BORDER_LDS;
  up2x_border_body<1, false, true>(b, stg, reinterpret_cast<float*>(stg + 2 * BORDER_STG), (int)threadIdx.x & 255,
                                            b0, cob);
}

}  // namespace vm
