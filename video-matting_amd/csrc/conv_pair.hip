// The first pair: conv1_1 -> relu -> conv1_2 -> relu [-> pool1] [+ the head split's skip-half partials]
// (unet.py:170-172 at full resolution, and conv1_5's share of cat1's conv1_2 half, unet.py:203).  This file: the
// strip-walking kernel (first, the default), the tile-per-block persistent kernel (under its own heading below), their
// routing (pair_first_impl; the streaming fallback is conv_patch.hip's FIRST form) and the vm_conv3x3_pair_first* entry
// points.
//
// The tile-per-block pair kernel (conv3x3_pair_persist) runs its phases in lock step: all 8 waves evaluate conv1_1 on
// the tile's halo patch (VALU-heavy, a third of the patch is halo), meet at a barrier, run conv1_2, meet again, stage
// and store.  The matrix pipe idles through the first and last phase (MFMA busy 0.29).  Here a 2-wave workgroup walks
// a 32-pixel-wide column strip down a segment of rows and keeps a 4-row ring of conv1_1 output rows in LDS:
//   * per output row r it evaluates ONE new conv1_1 row (r + 2; 34 pixels for 32 outputs: the horizontal halo only,
//     no vertical recompute inside a segment) and conv1_2 row r from ring rows r-1 .. r+1;
//   * wave w owns output channels 32w .. 32w+31 of both convs, and holds its conv1_2 filter (18 K-steps x 2
//     fragments = 144 VGPRs) and conv1_1 filter in registers for the whole segment, so the only LDS reads in the
//     conv1_2 loop are the pixel fragments (2 per 4 MFMAs);
//   * the input rows (f32 frame -> bf16 8-channel chunks) go through an 8-row LDS ring, loaded a row ahead;
//   * one 128-thread barrier per output row; with 4 workgroups per CU the waves of other strips fill each SIMD's
//     gaps, so no phase of one strip stalls the matrix pipe of the CU;
//   * the epilogue works from registers: bias/affine/act, 16-byte stores of whole channel chunks (chunk_pair),
//     the 2x2 SAME max-pool from the previous row's registers and a DPP column exchange, and the head split's
//     per-tap partials (2 MFMAs on the bf16 outputs, handed to wave 0 through LDS a row later).
// Every MFMA sequence (conv1_1: 3 K-steps of 4 taps x 8 channels; conv1_2: granule 0 taps 0..8, granule 1 taps
// 0..8; head: channels 0..31 then 32..63) is the one the tile kernels run, so outputs, pool and partials are
// bit-identical to conv3x3_pair_persist (tests/test_gpu_parity.py::test_pair_strip_*).
#include "conv_dispatch.h"

namespace vm {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

struct StripCfg {
  // 30 output columns per strip: the conv1_1 row then spans exactly 32 columns (-1 .. 30) = two 16-pixel MFMA
  // fragments (a 32-column strip needs 34, i.e. a third fragment for 2 columns); conv1_2's last fragment computes 2
  // columns it does not store
  static constexpr int SW = 30;                  // output columns per strip
  static constexpr int RC = SW + 2;              // conv1_1 columns per ring row (strip columns -1 .. 30)
  static constexpr int RW = 32;                  // ring row stride in pixels: a multiple of 8 keeps swz2 row-independent
  static constexpr int RSLOT = 4;                // conv1_1 rows in the ring (r-1 .. r+1 read, r+2 written)
  static constexpr int PLANE = RSLOT * RW * 64;  // one 32-channel granule plane (64-byte pixel rows)
  static constexpr int IW = SW + 4, ISLOT = 8;   // input ring: strip columns -2 .. 31, 16 bytes per pixel
  static constexpr int I_OFF = 2 * PLANE;
  static constexpr int X_OFF = I_OFF + ISLOT * IW * 16;  // head B operands: [row parity][wave][fp][lane] uint4
  static constexpr int K_OFF = X_OFF + 2 * 2 * 2 * 64 * 16;  // mul[64], add[64], bias1[64]
  static constexpr int H_OFF = K_OFF + 3 * 64 * 4;       // head A fragments [kk][lane] uint4
  static constexpr int RSZ = 2048;                       // raw input window staging (<= 2 DMA instructions), 2 slots
  static constexpr int R_OFF = H_OFF + 2 * 64 * 16;
  static constexpr int LDS = R_OFF + 2 * RSZ;
};

// XIN: 0 = bf16 frame of 8-channel pixels, 2 = f32 frame with x_c <= 8 channels (cstride <= 8)
// ACT: the epilogue's activation as a compile-time constant (a runtime switch per element made hipcc emit a branch
// tree per value, and this kernel is issue-bound, not MFMA-bound)
// XC: the f32 frame's channel count when known at compile time (7: the video path's cmp / bg / trimap frame), 0 =
// a.x_c at run time (a per-channel branch with its own LDS-load wait)
template <int XIN, int ACT, int ABL = 0, int PIN = 1, int XC = 0>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2)))
void conv3x3_pair_strip(ConvArgs a, int seg, int nseg, int nstrip) {
  using C = StripCfg;
  using T = uint16_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int H = a.H, W = a.W;
  const int strip = blockIdx.x % nstrip, rest = blockIdx.x / nstrip;
  const int sg = rest % nseg, n = rest / nseg;
  const int c0 = strip * C::SW, s0 = sg * seg, s1 = min(s0 + seg, H);

  // filters in registers: conv1_2 K-step s = granule s / 9, tap s % 9 (chunk-major packing), conv1_1 K-step j =
  // taps 4j .. 4j+3 x 8 channels (tap-major, K_pad 128); rows = this wave's 32 output channels
  const T* wg = reinterpret_cast<const T*>(a.w);
  const T* w1 = reinterpret_cast<const T*>(a.w1);
  uint4 w2[18][2], w1f[3][2];
#pragma unroll
  for (int s = 0; s < 18; ++s)
#pragma unroll
    for (int f = 0; f < 2; ++f)
      w2[s][f] = *reinterpret_cast<const uint4*>(wg + (long)(32 * wave + 16 * f + col) * a.K_pad + s * 32 + q * 8);
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int f = 0; f < 2; ++f)
      w1f[j][f] = *reinterpret_cast<const uint4*>(w1 + (32 * wave + 16 * f + col) * 128 + j * 32 + q * 8);
  float* rk = reinterpret_cast<float*>(smem + C::K_OFF);
  if (tid < 64) {
    const int co = min(tid, a.cout - 1);
    const float sc = a.scale ? a.scale[co] : 1.f;
    rk[tid] = sc;
    rk[64 + tid] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
    rk[128 + tid] = a.bias1 ? a.bias1[tid] : 0.f;
  } else if (a.hd) {
    // head split: A fragments of the skip half's head filter, rows = taps (9 of 16), k = 8q + j <-> conv1_2 channel
    // (2kk + j/4)*16 + 4q + j%4, the order in which the epilogue's lanes hold their bf16 outputs (B operand)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint32_t u[4];
#pragma unroll
      for (int jp = 0; jp < 4; ++jp) {
        const int j0 = 2 * jp, j1 = 2 * jp + 1;
        const int ch0 = (2 * kk + j0 / 4) * 16 + 4 * q + j0 % 4, ch1 = (2 * kk + j1 / 4) * 16 + 4 * q + j1 % 4;
        const float h0 = col < 9 ? a.hw[col * a.hw_cin + a.hw_coff + ch0] : 0.f;
        const float h1 = col < 9 ? a.hw[col * a.hw_cin + a.hw_coff + ch1] : 0.f;
        u[jp] = bf16x2_bits(h0, h1);
      }
      *reinterpret_cast<uint4*>(smem + C::H_OFF + (kk * 64 + lane) * 16) = make_uint4(u[0], u[1], u[2], u[3]);
    }
  }

  // ---- input rows: the window of strip columns -2 .. 33 of one frame row is contiguous in HBM (NHWC), so wave 0
  // fetches it with one or two LDS-DMA instructions (no registers held across the MFMA phases) into a 2-slot raw
  // staging ring, and a row later lanes 0..35 convert it to bf16 8-channel chunks (zero outside the frame) in the
  // 8-row input ring.  The descriptor covers ONE image, and the fetched bytes [ws, ws + nd KB) are clamped inside it
  // (ws = the window's first byte, moved right at the image start and left at its end), so no 16-byte piece ever
  // straddles the image bounds: every needed byte is fetched, none outside the tensor.  Rows outside the frame fetch
  // nothing (out-of-range offsets read as zeros).
  const int es = XIN == 2 ? 4 : 2, cs = a.x_cstride;
  const int pxb = cs * es, imgb = H * W * pxb;  // host: imgb >= 2 KB and < 2 GB
  const char* ximg = reinterpret_cast<const char*>(a.x) + ((long)a.x_coff + (long)n * H * W * cs) * es;
  const __amdgpu_buffer_rsrc_t xrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ximg), 0, (uint32_t)imgb, 0x00020000);
  const int nd = (C::IW * pxb + 1023) / 1024;  // DMA instructions per row (host: <= 2)
  const uint32_t raw0 = __builtin_amdgcn_readfirstlane(lds_addr(smem + C::R_OFF));
  auto wstart = [&](int ir) __attribute__((always_inline)) {  // first fetched byte of row ir's window
    return min(max((ir * W + c0 - 2) * pxb, 0), imgb - nd * 1024);
  };
  auto dma_row = [&](int ir, int slot) __attribute__((always_inline)) {  // wave 0
    const bool ok = (unsigned)ir < (unsigned)H;
    const int base = wstart(ir) + lane * 16;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(raw0 + slot * C::RSZ);
    glds16(xrs, dst, ok ? base : OOB_INL);
    if (nd > 1) glds16(xrs, dst + 1024, ok ? base + 1024 : OOB_INL);
  };
  auto convert_row = [&](int ir, int slot) __attribute__((always_inline)) {  // wave 0, lanes 0..35
    if (lane < C::IW) {
      const int xc = c0 - 2 + lane;
      const bool ok = (unsigned)ir < (unsigned)H && (unsigned)xc < (unsigned)W;
      const char* rp = smem + C::R_OFF + slot * C::RSZ + (ok ? (ir * W + xc) * pxb - wstart(ir) : 0);
      uint4 v;
      if constexpr (XIN == 2) {
        float xz[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
          xz[c] = c < (XC ? XC : a.x_c) ? *reinterpret_cast<const float*>(rp + 4 * c) : 0.f;
        v = Chunk<T>::pack(xz);
      } else {
        v = *reinterpret_cast<const uint4*>(rp);
      }
      *reinterpret_cast<uint4*>(smem + C::I_OFF + ((ir & 7) * C::IW + lane) * 16) = ok ? v : make_uint4(0, 0, 0, 0);
    }
  };

  // ---- conv1_1 row jr (+ bias + relu; zero outside the frame = conv1_2's SAME padding) -> this wave's plane, slot jr&3
  T* y1b = a.y1 ? reinterpret_cast<T*>(a.y1) + a.y1_coff + ((long)n * H) * W * (long)a.y1_cstride : nullptr;
  const __amdgpu_buffer_rsrc_t y1rs = __builtin_amdgcn_make_buffer_rsrc(y1b, 0, 0x7ffffff0, 0x00020000);
  auto conv1 = [&](int jr) __attribute__((always_inline)) {
    // lane-derived addresses are recomputed per call (an opaque copy of the lane id): hoisted out of the row loop they
    // would hold a dozen registers the filters need
    int l = lane;
    asm volatile("" : "+v"(l));
    const int cl = l & 15, ql = l >> 4;
    const int cq16 = (ql & 1) ? 2 + (ql >> 1) : ql >> 1;
    const bool rin = (unsigned)jr < (unsigned)H;
    char* dst = smem + wave * C::PLANE + (jr & 3) * (C::RW * 64) + swz2(cl, cq16);
    float b1[2][4];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float4 bb = *reinterpret_cast<const float4*>(rk + 128 + 32 * wave + 16 * f + 4 * ql);
      b1[f][0] = bb.x; b1[f][1] = bb.y; b1[f][2] = bb.z; b1[f][3] = bb.w;
    }
    // input-ring byte offset of K-step j's tap (4j + ql, taps 9..11 -> 8) for ring column cl: the three input-row
    // offsets are uniform (scalar), the lane picks one (j = 0: tap ql, j = 1: tap 4 + ql, j = 2: tap 8)
    int ro[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) ro[d] = C::I_OFF + ((jr - 1 + d) & 7) * (C::IW * 16);
    const bool q3 = ql == 3, q01 = ql < 2;
    const int ib[3] = {(q3 ? ro[1] : ro[0]) + (cl + (q3 ? 0 : ql)) * 16,
                       (q01 ? ro[1] : ro[2]) + (cl + (q01 ? 1 + ql : ql - 2)) * 16, ro[2] + (cl + 2) * 16};
    // branch-free (one basic block with conv1_2's loop, so the two can interleave): rows outside the frame read the
    // input ring's zero rows and are masked to zero like columns outside it
#pragma unroll
    for (int fr = 0; fr < C::RC / 16; ++fr) {
      const int rc = fr * 16 + cl;  // ring column: strip column rc - 1
      f32x4 acc1[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // unconditional: taps 9..11 (K-step 2, q > 0) read tap 8's pixel, whose finite values meet zero weights
        // (the products are zeros, as with a zero operand)
        const uint4 bv = *reinterpret_cast<const uint4*>(smem + ib[j] + fr * 256);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          if constexpr (ABL & 1) asm volatile("" ::"v"(bv.x), "v"(w1f[j][f].x));
          else mma16<T>(w1f[j][f], bv, acc1[f]);
        }
      }
      const int cc = c0 - 1 + rc;
      const bool inside = rin && (unsigned)cc < (unsigned)W;
      uint2 pk[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        float v[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) v[jj] = fmaxf(acc1[f][jj] + b1[f][jj], 0.f);
        // outside the frame: +0 (masked on the packed pairs, the bits a +0 float converts to)
        pk[f].x = inside ? bf16x2_bits(v[0], v[1]) : 0u;
        pk[f].y = inside ? bf16x2_bits(v[2], v[3]) : 0u;
      }
      // swz2(16 fr + cl, c) = 1024 fr + swz2(cl, c): ((16 fr + cl) >> 1) & 3 == (cl >> 1) & 3
      const uint4 ck = chunk_pair(pk[0], pk[1]);
      *reinterpret_cast<uint4*>(dst + fr * 1024) = ck;
      if (a.y1) {  // conv1_1 itself (the training towers' select convs read it): this segment's rows, own columns
        const int c = c0 + rc - 1;
        const bool ok = jr >= s0 && jr < s1 && rc >= 1 && rc <= C::SW && c < W;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, ck), y1rs,
                                               ok ? ((int)__umul24(jr * W + c, a.y1_cstride) + 32 * wave + 8 * cq16) * 2 : OOB_INL, 0, 0);
      }
    }
  };

  const int ycs2 = a.y_cstride * 2;
  T* yrow0 = reinterpret_cast<T*>(a.y) + a.y_coff + ((long)n * H) * W * (long)a.y_cstride;
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yrow0, 0, 0x7ffffff0, 0x00020000);
  const int PH = (H + 1) >> 1, PWd = (W + 1) >> 1;
  T* prow0 = a.py ? reinterpret_cast<T*>(a.py) + a.py_coff + ((long)n * PH) * PWd * (long)a.py_cstride : nullptr;
  const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(prow0, 0, 0x7ffffff0, 0x00020000);
  uint2 prev[2][2];  // the even row's bf16 outputs [fp][f] (pool partner)

  const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.hd ? a.hd + (long)n * H * W * 12 : nullptr), 0, 0x7ffffff0, 0x00020000);
  auto head_finish = [&](int r) __attribute__((always_inline)) {  // wave 0: row r's partials (wave 1's half via LDS)
    const uint4 ha0 = *reinterpret_cast<const uint4*>(smem + C::H_OFF + lane * 16);
    const uint4 ha1 = *reinterpret_cast<const uint4*>(smem + C::H_OFF + (64 + lane) * 16);
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) {
      const uint4 hb0 = *reinterpret_cast<const uint4*>(smem + C::X_OFF + ((((r & 1) * 2 + 0) * 2 + fp) * 64 + lane) * 16);
      const uint4 hb1 = *reinterpret_cast<const uint4*>(smem + C::X_OFF + ((((r & 1) * 2 + 1) * 2 + fp) * 64 + lane) * 16);
      f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
      mma16<T>(ha0, hb0, d);
      mma16<T>(ha1, hb1, d);
      const int p = fp * 16 + col, c = c0 + p;
      // a buffer store per fragment whatever the lane mask (out-of-range offsets drop the rest), so the loop's
      // counted vmcnt knows exactly how many stores follow the row's DMA
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), hrs,
                                             q < 3 && p < C::SW && c < W ? ((r * W + c) * 12 + 4 * q) * 4 : OOB_INL, 0, 0);
    }
  };

  auto conv2 = [&](int r) __attribute__((always_inline)) {
    // fragment addresses: pixel x = fp*16 + col + dw of ring row slot (r-1+dh) & 3, chunk q; swz2's pattern does not
    // depend on the slot (RW % 8 == 0), and fp = 1 is fp = 0 shifted by 16 pixels: +1024 bytes, the same swizzle
    // ((p + 16) >> 1) & 3 == (p >> 1) & 3
    int so[3], sx[3];
    {
      int l = lane;
      asm volatile("" : "+v"(l));
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) sx[dw] = swz2((l & 15) + dw, l >> 4);
    }
#pragma unroll
    for (int dh = 0; dh < 3; ++dh) so[dh] = ((r - 1 + dh) & 3) * (C::RW * 64);
    f32x4 acc[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) acc[f][fp] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto frags = [&](uint4 (&bv)[2], int s) __attribute__((always_inline)) {
      const int g = s / 9, tap = s % 9;
#pragma unroll
      for (int fp = 0; fp < 2; ++fp)
        bv[fp] = *reinterpret_cast<const uint4*>(smem + g * C::PLANE + fp * 1024 + so[tap / 3] + sx[tap % 3]);
    };
    uint4 bv[2][2];
    frags(bv[0], 0);
#pragma unroll
    for (int s = 0; s < 18; ++s) {
      if (s + 1 < 18) frags(bv[(s + 1) & 1], s + 1);
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) {
          if constexpr (ABL & 2) asm volatile("" ::"v"(bv[s & 1][fp].x), "v"(w2[s][f].x));
          else mma16<T>(w2[s][f], bv[s & 1][fp], acc[f][fp]);
        }
    }
    // pin the order: step s+1's 2 reads ahead of step s's 4 MFMAs
    if constexpr (PIN) {
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int s = 0; s < 18; ++s) {
        if (s + 1 < 18) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
      }
    }

    if constexpr ((ABL & 16) != 0) {
      asm volatile("" ::"v"(acc[0][0][0]), "v"(acc[0][1][0]), "v"(acc[1][0][0]), "v"(acc[1][1][0]));
      return;
    }
    // epilogue: bias / affine / act in registers (lane-derived values recomputed from an opaque lane id, as in conv1)
    int l = lane;
    asm volatile("" : "+v"(l));
    const int cl = l & 15, ql = l >> 4;
    const int cq16 = (ql & 1) ? 2 + (ql >> 1) : ql >> 1;  // chunk_pair: the 16-byte chunk this lane ends up holding
    float mul[2][4], add[2][4];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float4 m4 = *reinterpret_cast<const float4*>(rk + 32 * wave + 16 * f + 4 * ql);
      const float4 a4 = *reinterpret_cast<const float4*>(rk + 64 + 32 * wave + 16 * f + 4 * ql);
      mul[f][0] = m4.x; mul[f][1] = m4.y; mul[f][2] = m4.z; mul[f][3] = m4.w;
      add[f][0] = a4.x; add[f][1] = a4.y; add[f][2] = a4.z; add[f][3] = a4.w;
    }
    const bool podd = (r & 1) != 0;
    const bool full = c0 + C::SW <= W;  // every stored column of the strip is inside the frame (uniform)
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) {
      const int c = c0 + fp * 16 + cl;
      const bool cok = fp * 16 + cl < C::SW && c < W;
      float v[2][4];
      uint2 pk[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float t = fmaf(acc[f][fp][j], mul[f][j], add[f][j]);
          if constexpr (ACT == VM_ACT_RELU) t = fmaxf(t, 0.f);
          else if constexpr (ACT == VM_ACT_SIGMOID) t = sigmoid_precise(t);
          v[f][j] = t;
        }
        pk[f].x = bf16x2_bits(v[f][0], v[f][1]);
        pk[f].y = bf16x2_bits(v[f][2], v[f][3]);
      }
      if (!a.y_skip) {
        const uint4 d = chunk_pair(pk[0], pk[1]);
        const int off = cok ? ((int)__umul24(r * W + c, ycs2) + (32 * wave + 8 * cq16) * 2) : OOB_INL;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), yrs,
                                               off, 0, 0);
      }
      if (a.hd) {
        const uint4 hb = make_uint4(pk[0].x, pk[0].y, pk[1].x, pk[1].y);
        *reinterpret_cast<uint4*>(smem + C::X_OFF + ((((r & 1) * 2 + wave) * 2 + fp) * 64 + l) * 16) = hb;
      }
      if (a.py) {
        // fused 2x2 SAME max-pool: even rows wait in registers for their partner (rows past the frame never win);
        // the column partner is lane cl ^ 1 (DPP quad_perm [1,0,3,2]); bf16 rounding is monotonic, so the max of
        // the rounded values is the rounded max
        if (!podd && r + 1 < H) {
          prev[fp][0] = pk[0];
          prev[fp][1] = pk[1];
        } else {
          uint2 m2[2];
          if constexpr (ACT == VM_ACT_RELU) {
            // relu outputs are +0 or positive (never -0: the sum starts at +0 and the bias add cannot make -0 unless
            // the affine shift is -0), so the order of their bf16 bit patterns is the unsigned order: the pool runs
            // on the packed pairs (v_pk_max_u16), and a position outside the frame enters as 0, which never wins
#pragma unroll
            for (int f = 0; f < 2; ++f) {
              uint32_t m[2] = {pk[f].x, pk[f].y};
              const uint32_t pp[2] = {prev[fp][f].x, prev[fp][f].y};
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                if (podd) m[h] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(
                                     __builtin_bit_cast(u16x2, m[h]), __builtin_bit_cast(u16x2, pp[h])));
                if (!full) m[h] = cok ? m[h] : 0u;
                const uint32_t u = (uint32_t)__builtin_amdgcn_mov_dpp((int)m[h], 0xB1, 0xF, 0xF, false);
                m[h] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, m[h]),
                                                                             __builtin_bit_cast(u16x2, u)));
              }
              m2[f] = make_uint2(m[0], m[1]);
            }
          } else {
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            float m[4];
            const uint2 pp = prev[fp][f];
            const float pv[4] = {__uint_as_float(pp.x << 16), __uint_as_float(pp.x & 0xffff0000u),
                                 __uint_as_float(pp.y << 16), __uint_as_float(pp.y & 0xffff0000u)};
            const float cv[4] = {__uint_as_float(pk[f].x << 16), __uint_as_float(pk[f].x & 0xffff0000u),
                                 __uint_as_float(pk[f].y << 16), __uint_as_float(pk[f].y & 0xffff0000u)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float t = podd ? fmaxf(pv[j], cv[j]) : cv[j];
              t = cok ? t : -INFINITY;
              const float u = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0xB1, 0xF, 0xF, false));
              m[j] = fmaxf(t, u);
            }
            m2[f].x = bf16x2_bits(m[0], m[1]);
            m2[f].y = bf16x2_bits(m[2], m[3]);
          }
          }
          const uint4 d = chunk_pair(m2[0], m2[1]);
          const int pr = r >> 1, pc = c >> 1;
          const bool pok = (cl & 1) == 0 && cok && pc < PWd;
          const int off = pok ? ((int)__umul24(pr * PWd + pc, a.py_cstride) + 32 * wave + 8 * cq16) * 2 : OOB_INL;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d),
                                                 prs, off, 0, 0);
        }
      }
    }
  };

  // ---- warm-up: input rows s0-2 .. s0+3 through the staging ring two at a time, row s0+4 left in staging (converted
  // in the first iteration), then conv1_1 rows s0-1 .. s0+1
  for (int k = 0; k < 6; k += 2) {
    if (wave == 0) {
      dma_row(s0 - 2 + k, 0);
      dma_row(s0 - 1 + k, 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (wave == 0) {
      convert_row(s0 - 2 + k, 0);
      convert_row(s0 - 1 + k, 1);
    }
    __syncthreads();
  }
  if (wave == 0) {
    dma_row(s0 + 4, (s0 - 1) & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  conv1(s0 - 1);
  conv1(s0);
  conv1(s0 + 1);
  __syncthreads();

  for (int r = s0; r < s1; ++r) {
    int nst = 0;  // wave 0: vector-memory ops issued after this row's DMA (counted vmcnt before the barrier)
    if (wave == 0) {
      if constexpr (!(ABL & 8)) convert_row(r + 4, (r - 1) & 1);  // read from iteration r + 1 on, after the barrier
      if constexpr (!(ABL & 8)) dma_row(r + 5, r & 1);
      // the previous row's head partials after the DMA (r04): the barrier's counted wait then leaves them in flight
      // (issued before the DMA, in-order counting made every row wait for their write-back too)
      const bool hf = a.hd && r > s0;
      if (hf) head_finish(r - 1);
      nst = (hf ? 2 : 0) + (a.y_skip ? 0 : 2) + (a.py && ((r & 1) || r + 1 == H) ? 2 : 0);
    }
    conv1(r + 2);  // (row s1 + 1 at a segment's last row: computed into a ring slot nothing reads)
    conv2(r);
    if (wave == 0) {  // nst is 0, 2, 4 or 6
      if ((ABL & 8) || nst == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (nst == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else if (nst == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // LDS-only barrier: global stores stay in flight
    if constexpr (!(ABL & 4)) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (a.hd && wave == 0) head_finish(s1 - 1);
}

// ================================================================ persistent first pair (conv1_1 -> conv1_2 [-> pool1])
// unet.py:170-172 at full resolution.  conv1_2 has only 2 channel granules (18 K-steps), so in the streaming patch
// kernel the per-tile fixed costs (input latency, the first conv, the epilogue) dominate.  Here ONE 512-thread block
// per CU keeps all of conv1_2's weights in LDS (18 K-step slots x 64 couts x 64 B = 72 KB, loaded once) and walks
// the 8 x 32 tiles t = blockIdx.x, +gridDim.x, ...: the main loop has no barrier and no DMA, and the next tile's
// input pixels are loaded into registers while the current tile's MFMAs run.
// The pair kernel's own patch images use a 2-bit chunk swizzle: like swz<64>, conflict-free for the ds_read_b128
// fragment reads from any start row, and also for ds_write_b128 of 8 consecutive rows (swz<64> is 2-way there)
// (swz2: conv_common.h)

struct PairCfg {
  static constexpr int TH = 8, TW = 32, BM = TH * TW, PW = TW + 2, PPIX = (TH + 2) * PW;
  static constexpr int IW = TW + 4, IPIX = (TH + 4) * IW;  // 8-channel input patch, origin (r0-2, c0-2)
  static constexpr int NW = 8, NT = 512, NSTEP = 18;
  static constexpr int PB = ((PPIX + 15) / 16) * 1024;     // one 32-channel granule of the patch (64-B rows)
  static constexpr int WSLOT = 64 * 64;
  static constexpr int PBU = PPIX * 64;                   // bytes of a granule buffer actually addressed
  static constexpr int SR = 64 * 2 + 16;                   // epilogue staging row
  static constexpr int P_OFF = NSTEP * WSLOT, I_OFF = P_OFF + 2 * PBU, S_OFF = I_OFF + IPIX * 16;
  static constexpr int R_OFF = S_OFF + BM * SR;             // per-channel epilogue constants: mul[64], add[64], b1[64]
  static constexpr int LDS = R_OFF + 3 * 64 * 4;
};
static_assert(PairCfg::LDS <= 163840, "weights + patch + input + staging in one CU's LDS");
static_assert(PairCfg::IPIX <= PairCfg::NT, "one input pixel per thread");

// PABL: timing ablations (results are garbage): 1 no first-conv MFMAs, 2 no conv1_2 MFMAs, 4 no output stores,
// 8 no input loads
// XIN: the input dtype/load form — a compile-time choice, so the input loads carry no runtime branch (a branch join
// made hipcc wait for the loads right after issuing them, before conv1_2).  0: bf16 8-channel chunks; 1: f32 frame,
// one dword load per channel; 2: f32 frame with 4 <= x_c <= 8 channels (the UNetVideo path), two 16-byte loads per
// pixel (channels 0..3 and x_c-4..x_c-1, dword-aligned) instead of 8 dword loads
// a workgroup barrier that orders LDS only (no vmcnt(0) as __syncthreads emits): global stores and loads stay in
// flight across it
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int PABL = 0, int XIN = 2>
__global__ __launch_bounds__(512) void conv3x3_pair_persist(ConvArgs a) {
  using C = PairCfg;
  using T = uint16_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W;
  const int th = (H + C::TH - 1) / C::TH, tw = (W + C::TW - 1) / C::TW;
  const int ntiles = (int)(a.M / ((long)H * W)) * th * tw;
  const int col = lane & 15, q = lane >> 4;

  // conv1_2 weights: slot s = K-step s of the chunk-major packing (granule cc*9 + tap), swizzled 64-B rows
  const T* wg = reinterpret_cast<const T*>(a.w);
  for (int i = tid; i < C::NSTEP * 64 * 4; i += C::NT) {
    const int st = i >> 8, row = (i >> 2) & 63, ch = i & 3;
    *reinterpret_cast<uint4*>(smem + st * C::WSLOT + swz<64>(row, ch)) =
        *reinterpret_cast<const uint4*>(wg + (long)row * a.K_pad + st * 32 + ch * 8);
  }
  // conv1_1 (tap-major, K_pad 128) weight fragments and bias stay in registers
  const T* w1 = reinterpret_cast<const T*>(a.w1);
  uint4 wf[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) wf[j][fc] = *reinterpret_cast<const uint4*>(w1 + (fc * 16 + col) * 128 + j * 32 + q * 8);
  // consume the fragments here: otherwise hipcc's wait for these loads sits inside the tile loop (it cannot tell the
  // first iteration from the rest), where every tile then waits vmcnt(3..0) for the PREVIOUS tile's output stores
  __builtin_amdgcn_s_waitcnt(0xF70);  // vmcnt(0) (expcnt / lgkmcnt at max): a real S_WAITCNT the wait pass accounts for
  // per-channel constants live in LDS (registers go to the conv1_2 fragment prefetch)
  float* rmul = reinterpret_cast<float*>(smem + C::R_OFF);
  if (tid < 64) {
    const int co = min(tid, a.cout - 1);
    const float sc = a.scale ? a.scale[co] : 1.f;
    rmul[tid] = sc;
    rmul[64 + tid] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
    rmul[128 + tid] = a.bias1 ? a.bias1[tid] : 0.f;
  }
  // head split: A fragments of the skip half's head filter, rows = taps (9 of 16), k = 8q + j <-> conv1_2 channel
  // (2kk + j/4)*16 + 4q + j%4 — the channel order in which the epilogue's lane holds its bf16 outputs (B operand)
  uint4 hwf[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  if (a.hd) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint32_t u[4];
#pragma unroll
      for (int jp = 0; jp < 4; ++jp) {
        const int j0 = 2 * jp, j1 = 2 * jp + 1;
        const int c0 = (2 * kk + j0 / 4) * 16 + 4 * q + j0 % 4, c1 = (2 * kk + j1 / 4) * 16 + 4 * q + j1 % 4;
        const float w0 = col < 9 ? a.hw[col * a.hw_cin + a.hw_coff + c0] : 0.f;
        const float w1 = col < 9 ? a.hw[col * a.hw_cin + a.hw_coff + c1] : 0.f;
        u[jp] = bf16x2_bits(w0, w1);
      }
      hwf[kk] = make_uint4(u[0], u[1], u[2], u[3]);
    }
  }

  // input pixel of this thread (one per thread): raw registers while in flight, bf16 chunk in LDS
  const T* x8 = reinterpret_cast<const T*>(a.x) + a.x_coff;
  const float* xf = reinterpret_cast<const float*>(a.x) + a.x_coff;
  uint4 xq = make_uint4(0, 0, 0, 0);
  float xr[8];
  f32x4 xlo = f32x4{0.f, 0.f, 0.f, 0.f}, xhi = xlo;
  bool xin = false;
  auto load_in = [&](int t) {
    const int n = t / (th * tw), rem = t - n * th * tw;
    const int ir = tid / C::IW, ic = tid - ir * C::IW;
    const int h = (rem / tw) * C::TH - 2 + ir, w = (rem % tw) * C::TW - 2 + ic;
    xin = tid < C::IPIX && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
    if (PABL & 8) return;
    // branch-free: out-of-frame lanes read pixel (0,0) and channels past x_c re-read the last one, so all loads
    // issue back to back and are waited for once, at store_in (a per-element conditional load makes hipcc wait
    // for each load in turn)
    const long pix = xin ? (((long)n * H + h) * W + w) * (long)a.x_cstride : 0;
    if constexpr (XIN == 2) {  // unaligned 16-byte loads (4-byte aligned): memcpy keeps hipcc from assuming 16
      __builtin_memcpy(&xlo, xf + pix, 16);
      __builtin_memcpy(&xhi, xf + pix + (a.x_c - 4), 16);
    } else if constexpr (XIN == 1) {
#pragma unroll
      for (int c = 0; c < 8; ++c) xr[c] = xf[pix + min(c, a.x_c - 1)];
    } else {
      xq = *reinterpret_cast<const uint4*>(x8 + pix);
    }
  };
  auto store_in = [&]() {
    if (tid < C::IPIX) {
      uint4 v = xq;
      if constexpr (XIN == 2) {
        float xz[8];
        const int sh = a.x_c - 4;  // xhi[k] = channel sh + k
#pragma unroll
        for (int c = 0; c < 4; ++c) xz[c] = xlo[c];
#pragma unroll
        for (int c = 4; c < 8; ++c) {
          const int k = c - sh;
          const float h = k == 0 ? xhi[0] : k == 1 ? xhi[1] : k == 2 ? xhi[2] : xhi[3];
          xz[c] = c < a.x_c ? h : 0.f;
        }
        v = Chunk<T>::pack(xz);
      } else if constexpr (XIN == 1) {
        float xz[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) xz[c] = c < a.x_c ? xr[c] : 0.f;
        v = Chunk<T>::pack(xz);
      }
      *reinterpret_cast<uint4*>(smem + C::I_OFF + tid * 16) = xin ? v : make_uint4(0, 0, 0, 0);
    }
  };

  int t = blockIdx.x;
  if (t < ntiles) {
    load_in(t);
    store_in();
    // the input of the block's second tile is in flight from here on (a whole tile ahead of its store_in)
    if (t + (int)gridDim.x < ntiles) load_in(t + gridDim.x);
  }
  __syncthreads();
  const int ycs2 = a.y_cstride * 2;
  for (; t < ntiles; t += gridDim.x) {
    const int n = t / (th * tw), rem = t - n * th * tw;
    const int r0 = (rem / tw) * C::TH, c0 = (rem % tw) * C::TW;
    // (1) conv1_1 + bias + relu of the (TH+2) x (TW+2) patch into both granule buffers (zero outside the frame)
    for (int f = wave; f < (C::PPIX + 15) / 16; f += C::NW) {
      const int p = f * 16 + col;
      const int pr = p / C::PW, pc = p - pr * C::PW;
      f32x4 acc1[4];
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) acc1[fc] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int tap = 4 * j + q;
        uint4 bv = make_uint4(0, 0, 0, 0);
        if (tap < 9 && p < C::PPIX)
          bv = *reinterpret_cast<const uint4*>(smem + C::I_OFF + ((pr + tap / 3) * C::IW + pc + tap % 3) * 16);
        if constexpr (PABL & 1) {
          asm volatile("" ::"v"(bv.x), "v"(bv.w));
        } else {
#pragma unroll
          for (int fc = 0; fc < 4; ++fc) mma16<T>(wf[j][fc], bv, acc1[fc]);
        }
      }
      const int h = r0 - 1 + pr, w = c0 - 1 + pc;
      const bool inside = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      uint2 pk[4];
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const float4 bb = *reinterpret_cast<const float4*>(rmul + 128 + fc * 16 + 4 * q);
        const float b1[4] = {bb.x, bb.y, bb.z, bb.w};
        float v[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) v[jj] = inside ? fmaxf(acc1[fc][jj] + b1[jj], 0.f) : 0.f;
        pk[fc].x = bf16x2_bits(v[0], v[1]);
        pk[fc].y = bf16x2_bits(v[2], v[3]);
      }
      // whole 16-byte chunks per lane (conflict-free ds_write_b128 under swz2) instead of 8-byte halves
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const uint4 ck = chunk_pair(pk[2 * g], pk[2 * g + 1]);
        if (p < C::PPIX)
          *reinterpret_cast<uint4*>(smem + C::P_OFF + g * C::PBU + swz2(p, (q & 1) ? 2 + (q >> 1) : q >> 1)) = ck;
      }
    }
    lds_barrier();  // LDS only: the previous tile's output stores stay in flight across it
    const int tn = t + gridDim.x;
    // (3) conv1_2: 2 granules x 9 taps, operands straight from LDS, no barrier
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k) acc[i][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    int abase[2];
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) {
      const int p = wave * 32 + fp * 16;
      abase[fp] = (p / C::TW) * C::PW + (p % C::TW) + col;
    }
    // K-step s = (granule s / 9, tap s % 9); the fragments of step s + 1 are read while step s's MFMAs run
    auto frags = [&](uint4 (&av)[4], uint4 (&bv)[2], int s) {
      const int cc = s / 9, tap = s - cc * 9;
      const char* wp = smem + s * C::WSLOT;
      const char* xp = smem + C::P_OFF + cc * C::PBU;
      const int toff = (tap / 3) * C::PW + tap % 3;
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) av[fc] = *reinterpret_cast<const uint4*>(wp + swz<64>(fc * 16 + col, q));
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) bv[fp] = *reinterpret_cast<const uint4*>(xp + swz2(abase[fp] + toff, q));
    };
    uint4 av[2][4], bv[2][2];
    frags(av[0], bv[0], 0);
#pragma unroll
    for (int s = 0; s < C::NSTEP; ++s) {
      if (s + 1 < C::NSTEP) frags(av[(s + 1) & 1], bv[(s + 1) & 1], s + 1);
      if constexpr (PABL & 2) {
#pragma unroll
        for (int fc = 0; fc < 4; ++fc) asm volatile("" ::"v"(av[s & 1][fc].x), "v"(av[s & 1][fc].w));
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) asm volatile("" ::"v"(bv[s & 1][fp].x), "v"(bv[s & 1][fp].w));
      } else {
#pragma unroll
        for (int fc = 0; fc < 4; ++fc)
#pragma unroll
          for (int fp = 0; fp < 2; ++fp) mma16<T>(av[s & 1][fc], bv[s & 1][fp], acc[fc][fp]);
      }
    }
    if constexpr (!(PABL & 2)) {  // pin the order: step s+1's 6 reads ahead of step s's 8 MFMAs
      __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
      for (int s = 0; s < C::NSTEP; ++s) {
        if (s + 1 < C::NSTEP) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x8, 8, 0);
      }
    }
    if (tn < ntiles) store_in();  // ip was last read by this tile's first conv, before the barrier above
    // (2') the input of the tile after next goes in flight now, in the registers store_in just freed: one whole tile
    // of work (its epilogue, first conv and conv1_2) covers the HBM latency of the f32 frame reads
    if (tn + (int)gridDim.x < ntiles) load_in(tn + gridDim.x);
    // (4) epilogue: bias/affine/act -> bf16 staging -> 16-byte stores (+ fused 2x2 SAME max-pool)
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) {
      const int row = wave * 32 + fp * 16 + col;
      uint2 pk[4];
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const int cl = fc * 16 + 4 * q;
        const float4 m4 = *reinterpret_cast<const float4*>(rmul + cl);
        const float4 a4 = *reinterpret_cast<const float4*>(rmul + 64 + cl);
        const float mul[4] = {m4.x, m4.y, m4.z, m4.w}, add[4] = {a4.x, a4.y, a4.z, a4.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = fmaf(acc[fc][fp][j], mul[j], add[j]);
          if (a.act == VM_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
          else if (a.act == VM_ACT_SIGMOID) v[j] = sigmoid_precise(v[j]);
        }
        pk[fc].x = bf16x2_bits(v[0], v[1]);
        pk[fc].y = bf16x2_bits(v[2], v[3]);
      }
      if (a.hd) {  // the skip half's head partials of this lane's pixel: 2 MFMAs on the bf16 outputs just made
        f32x4 dacc = f32x4{0.f, 0.f, 0.f, 0.f};
        mma16<T>(hwf[0], make_uint4(pk[0].x, pk[0].y, pk[1].x, pk[1].y), dacc);
        mma16<T>(hwf[1], make_uint4(pk[2].x, pk[2].y, pk[3].x, pk[3].y), dacc);
        const int pc = fp * 16 + col;
        if (q < 3 && r0 + wave < H && c0 + pc < W)
          *reinterpret_cast<f32x4*>(a.hd + (((long)n * H + r0 + wave) * W + c0 + pc) * 12 + 4 * q) = dacc;
      }
      // 16-byte chunks: rows of 144 B make 8 consecutive rows hit 8 distinct 4-bank groups (conflict-free b128)
#pragma unroll
      for (int g = 0; g < 2; ++g)
        *reinterpret_cast<uint4*>(smem + C::S_OFF + row * C::SR + 64 * g +
                                  16 * ((q & 1) ? 2 + (q >> 1) : q >> 1)) = chunk_pair(pk[2 * g], pk[2 * g + 1]);
    }
    // one barrier publishes the staging, the next tile's input and (for the next first conv) the end of this
    // tile's patch reads; the stores below then overlap the next tile's first conv (staging is rewritten only
    // after the next tile's first barrier)
    lds_barrier();  // LDS only: the previous tile's output stores stay in flight across it
    T* yb = reinterpret_cast<T*>(a.y) + a.y_coff + (((long)n * H + r0) * W + c0) * (long)a.y_cstride;
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yb, 0, 0x7ffffff0, 0x00020000);
#pragma unroll
    for (int it = 0; it < C::BM * 8 / C::NT; ++it) {
      if (a.y_skip) break;
      const int idx = it * C::NT + tid;
      const int rr = idx >> 3, cq = idx & 7;
      const uint4 d = *reinterpret_cast<const uint4*>(smem + C::S_OFF + rr * C::SR + cq * 16);
      const int pr = rr / C::TW, pc = rr % C::TW;
      const bool ok = r0 + pr < H && c0 + pc < W && cq * 8 < a.cout && !(PABL & 4);
      const int off = ok ? (pr * W + pc) * ycs2 + cq * 16 : OOB;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), yrs,
                                             off, 0, 0);
    }
    if (a.py) {
      const int PH = (H + 1) >> 1, PWd = (W + 1) >> 1;
      const int pr0 = r0 >> 1, pc0 = c0 >> 1;
      T* pb = reinterpret_cast<T*>(a.py) + a.py_coff + (((long)n * PH + pr0) * PWd + pc0) * (long)a.py_cstride;
      const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pb, 0, 0x7ffffff0, 0x00020000);
      constexpr int PTW = C::TW / 2, PITEMS = C::BM / 4 * 8;
#pragma unroll
      for (int it = 0; it < (PITEMS + C::NT - 1) / C::NT; ++it) {
        const int idx = it * C::NT + tid;
        if (idx >= PITEMS) break;
        const int pp = idx >> 3, cq = idx & 7;
        const int pr = pp / PTW, pc = pp % PTW;
        const int rr = 2 * pr * C::TW + 2 * pc;
        const bool vh = r0 + 2 * pr + 1 < H, vw = c0 + 2 * pc + 1 < W;
        float m[8], f[8];
        Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + C::S_OFF + rr * C::SR + cq * 16), m);
        if (vw) {
          Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + C::S_OFF + (rr + 1) * C::SR + cq * 16), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
        }
        if (vh) {
          Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + C::S_OFF + (rr + C::TW) * C::SR + cq * 16), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
        }
        if (vh && vw) {
          Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + C::S_OFF + (rr + C::TW + 1) * C::SR + cq * 16), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
        }
        const bool ok = pr0 + pr < PH && pc0 + pc < PWd && cq * 8 < a.cout && !(PABL & 4);
        const int off = ok ? ((pr * PWd + pc) * a.py_cstride + cq * 8) * 2 : OOB;
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, Chunk<T>::pack(m)), prs, off, 0, 0);
      }
    }
  }
}

static bool pair_strip_ok(const ConvArgs& a) {
  // the input window (36 pixels) is fetched whole by <= 2 LDS-DMA instructions and addressed with 32-bit offsets
  // (and an image holds at least the 2 KB a row fetch may span)
  const int es = a.x_f32 ? 4 : 2;
  const long imgb = (long)a.H * a.W * a.x_cstride * es;
  // (pixel indices of a frame < 2^24: the output offsets use the full-rate 24-bit multiply)
  return a.cout == 64 && a.x_c <= 8 && (a.x_f32 ? a.x_cstride <= 8 : a.x_cstride == 8) && imgb < 0x7ffffff0L - 4096 &&
         imgb >= 2048 && a.W > 0 && a.H > 0 && (long)a.H * a.W < (1L << 24);
}

template <int ACT, int ABL, int PIN = 1>
static void launch_strip_act(ConvArgs& a, long grid, int seg, int nseg, int nstrip, hipStream_t st) {
  if constexpr (PIN) {
    if (!g_opt.pair_strip_pin) return launch_strip_act<ACT, ABL, 0>(a, grid, seg, nseg, nstrip, st);
  }
  if (a.x_f32 && a.x_c == 7)
    hipLaunchKernelGGL((conv3x3_pair_strip<2, ACT, ABL, PIN, 7>), dim3((unsigned)grid), dim3(128), StripCfg::LDS, st, a,
                       seg, nseg, nstrip);
  else if (a.x_f32)
    hipLaunchKernelGGL((conv3x3_pair_strip<2, ACT, ABL, PIN>), dim3((unsigned)grid), dim3(128), StripCfg::LDS, st, a, seg,
                       nseg, nstrip);
  else
    hipLaunchKernelGGL((conv3x3_pair_strip<0, ACT, ABL, PIN>), dim3((unsigned)grid), dim3(128), StripCfg::LDS, st, a, seg,
                       nseg, nstrip);
}
template <int ABL>
static void launch_strip_abl(ConvArgs& a, long grid, int seg, int nseg, int nstrip, hipStream_t st) {
  launch_strip_act<VM_ACT_RELU, ABL>(a, grid, seg, nseg, nstrip, st);
}

static int launch_pair_strip(ConvArgs& a, long nimg, hipStream_t st) {
  static int attr_dev = -1, n_cu = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (attr_dev != dev) {
    hipError_t e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return fail(VM_EHIP, "conv3x3_pair_strip setup: %s", hipGetErrorString(e));
    attr_dev = dev;
  }
  // one round of 4 workgroups per CU: segments of equal (even) height so that images x segments x strips fills it
  const int nstrip = (a.W + StripCfg::SW - 1) / StripCfg::SW;
  const long slots = 4L * n_cu;
  long nseg = slots / (nimg * nstrip);
  if (nseg < 1) nseg = 1;
  int seg = (int)((a.H + nseg - 1) / nseg);
  seg += seg & 1;
  if (seg < 2) seg = 2;
  nseg = (a.H + seg - 1) / seg;
  const long grid = nimg * nseg * nstrip;
  if (grid > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3_pair_strip: grid too large");
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_pair_strip");
#ifdef VM_STUDY
  switch (g_opt.pair_strip_abl) {
    case 1: launch_strip_abl<1>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 2: launch_strip_abl<2>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 3: launch_strip_abl<3>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 4: launch_strip_abl<4>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 8: launch_strip_abl<8>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 16: launch_strip_abl<16>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 28: launch_strip_abl<28>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    case 31: launch_strip_abl<31>(a, grid, seg, (int)nseg, nstrip, st); return check_launch("abl");
    default: break;
  }
#endif
  switch (a.act) {
    case VM_ACT_RELU: launch_strip_act<VM_ACT_RELU, 0>(a, grid, seg, (int)nseg, nstrip, st); break;
    case VM_ACT_SIGMOID: launch_strip_act<VM_ACT_SIGMOID, 0>(a, grid, seg, (int)nseg, nstrip, st); break;
    default: launch_strip_act<VM_ACT_NONE, 0>(a, grid, seg, (int)nseg, nstrip, st); break;
  }
  return check_launch("conv3x3_pair_strip");
}

template <int PABL, int XIN = 2>
static int launch_pair_persist(ConvArgs& a, long sp, hipStream_t st) {
  if constexpr (XIN == 2) {
    if (!a.x_f32) return launch_pair_persist<PABL, 0>(a, sp, st);
    if (a.x_c < 4 || !g_opt.pair_xin_wide) return launch_pair_persist<PABL, 1>(a, sp, st);
  }
  static int attr_dev = -1, n_cu = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (attr_dev != dev) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_pair_persist<PABL, XIN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, PairCfg::LDS);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return fail(VM_EHIP, "conv3x3_pair_persist setup: %s", hipGetErrorString(e));
    attr_dev = dev;
  }
  const int grid = (int)(sp < n_cu ? sp : n_cu);
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_pair_persist");
  hipLaunchKernelGGL((conv3x3_pair_persist<PABL, XIN>), dim3(grid), dim3(PairCfg::NT), PairCfg::LDS, st, a);
  return check_launch("conv3x3_pair_persist");
}

}  // namespace vm

using namespace vm;

// One call of the conv1_1 -> conv1_2 pair (vm_conv3x3_pair_first*)
struct PairCall {
  const vm_tensor* x;
  const void* packed1;
  int cin1;
  const float* bias1;
  const void* packed2;
  int cout2;
  const float* bias2;
  const float* scale2;
  const float* shift2;
  int act2;
  vm_tensor* y;
  vm_tensor* ypool;
  void* stream;
  const float* head_w = nullptr;  // head split: conv1_5's HWIO f32 filter, head_cin input channels, ours at head_coff
  int head_cin = 0, head_coff = 0;
  float* partial = nullptr;       // ... its per-tap partials [pixel][12]; store_y = 0 leaves y unwritten
  int store_y = 1;
  vm_tensor* mid = nullptr;       // conv1_1's output too (the strip kernel only)
};

static int pair_first_impl(const PairCall& c) {
  const vm_tensor* x = c.x;
  vm_tensor *y = c.y, *ypool = c.ypool;
  const int cin1 = c.cin1, cout2 = c.cout2;
  if (!valid_tensor(x) || !valid_tensor(y) || !c.packed1 || !c.packed2)
    return fail(VM_EINVAL, "conv3x3_pair_first: invalid tensor/weights");
  if (cin1 <= 0 || cin1 > 8 || x->c != cin1 || cout2 <= 0 || y->c != cout2)
    return fail(VM_EINVAL, "conv3x3_pair_first: x.c=%d cin1=%d (<= 8) y.c=%d cout2=%d", x->c, cin1, y->c, cout2);
  if (x->n != y->n || x->h != y->h || x->w != y->w) return fail(VM_EINVAL, "conv3x3_pair_first: spatial mismatch");
  if (c.act2 < VM_ACT_NONE || c.act2 > VM_ACT_SOFTMAX) return fail(VM_EINVAL, "conv3x3_pair_first: act %d", c.act2);
  if (ypool && (!valid_tensor(ypool) || ypool->n != y->n || ypool->h != (y->h + 1) / 2 || ypool->w != (y->w + 1) / 2 ||
                ypool->c != cout2 || ypool->dtype != y->dtype))
    return fail(VM_EINVAL, "conv3x3_pair_first: pool output must be [n, ceil(h/2), ceil(w/2), cout2]");
  const bool xf32 = x->dtype == VM_F32;
  const bool xvec = xf32 || (view16_ok(x) && x->coff + 8 <= x->cstride);
  if (y->dtype != VM_BF16 || !xvec || !view16_ok(y) || (ypool && !view16_ok(ypool)) || cout2 % 8 ||
      c.act2 == VM_ACT_SOFTMAX || g_opt.conv_kernel == 1 || g_opt.conv_kernel == 2)
    return fail(VM_EUNSUPPORTED, "conv3x3_pair_first: needs a bf16 output and 16-byte channel views (bf16 x: "
                                 "8-channel pixels)");
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  ConvArgs a{};
  a.x = x->ptr; a.x_cstride = x->cstride; a.x_coff = x->coff; a.H = x->h; a.W = x->w;
  a.M = (long)x->n * x->h * x->w;
  fill_geom(a, geom(64, cout2, VM_BF16));
  a.w = c.packed2; a.cout = cout2;
  a.bias = c.bias2; a.scale = c.scale2; a.shift = c.shift2; a.act = c.act2;
  a.y = y->ptr; a.y_cstride = y->cstride; a.y_coff = y->coff; a.y_dtype = y->dtype; a.y_vec = 1;
  a.w1 = c.packed1; a.bias1 = c.bias1; a.x_f32 = xf32; a.x_c = cin1;
  if (ypool) { a.py = ypool->ptr; a.py_cstride = ypool->cstride; a.py_coff = ypool->coff; }
  const long sp = (long)x->n * ((x->h + 7) / 8) * ((x->w + 31) / 32);
  if (c.partial) {
    a.hd = c.partial; a.hw = c.head_w; a.hw_cin = c.head_cin; a.hw_coff = c.head_coff; a.y_skip = c.store_y ? 0 : 1;
  }
  // the strip kernel addresses one image's output / pool with 32-bit byte offsets
  const bool strip_fits = (long)x->h * x->w * y->cstride * 2 < 0x7ffffff0L &&
                          (!ypool || (long)ypool->h * ypool->w * ypool->cstride * 2 < 0x7ffffff0L);
  if (c.mid) {  // conv1_1's output too: the strip kernel only (the caller otherwise runs the two convs)
    if (!(g_opt.pair_strip && g_opt.pair_kernel == 0 && strip_fits && pair_strip_ok(a) &&
          (long)c.mid->h * c.mid->w * c.mid->cstride * 2 < 0x7ffffff0L))
      return fail(VM_EUNSUPPORTED, "conv3x3_pair_first_mid: needs the strip pair kernel");
    a.y1 = c.mid->ptr; a.y1_cstride = c.mid->cstride; a.y1_coff = c.mid->coff;
  }
  if (g_opt.pair_strip && g_opt.pair_kernel == 0 && strip_fits && pair_strip_ok(a)) return launch_pair_strip(a, x->n, st);
  if (c.partial) {  // the head split lives in the persistent pair kernel only
    if (cout2 != 64 || g_opt.pair_kernel != 0 || sp > 0x7fffffffL)
      return fail(VM_EUNSUPPORTED, "conv3x3_pair_first_head: needs the persistent pair kernel (cout2 64)");
    return launch_pair_persist<0>(a, sp, st);
  }
  if (cout2 == 64 && (g_opt.pair_kernel == 0 || g_opt.pair_kernel >= 10) && sp <= 0x7fffffffL) {
#ifdef VM_STUDY
    switch (g_opt.pair_kernel) {  // >= 10: timing ablations (garbage results), study build only
      case 11: return launch_pair_persist<1>(a, sp, st);
      case 12: return launch_pair_persist<2>(a, sp, st);
      case 14: return launch_pair_persist<4>(a, sp, st);
      case 18: return launch_pair_persist<8>(a, sp, st);
      case 13: return launch_pair_persist<3>(a, sp, st);
      default: break;
    }
#endif
    return launch_pair_persist<0>(a, sp, st);
  }
  return launch_patch_first(a, st);  // the streaming patch kernel's FIRST form (conv_patch.hip)
}

extern "C" int vm_conv3x3_pair_first_mid_nhwc(const vm_tensor* x, const void* packed1, int cin1, const float* bias1,
                                              const void* packed2, int cout2, const float* bias2, const float* scale2,
                                              const float* shift2, int act2, vm_tensor* y, vm_tensor* ypool,
                                              vm_tensor* mid, void* stream) {
  if (!valid_tensor(mid) || mid->dtype != VM_BF16 || mid->c != 64 || !x || mid->n != x->n || mid->h != x->h ||
      mid->w != x->w || !view16_ok(mid))
    return fail(VM_EINVAL, "conv3x3_pair_first_mid: mid must be a 16-byte aligned bf16 [n,h,w,64] view");
  PairCall c{x, packed1, cin1, bias1, packed2, cout2, bias2, scale2, shift2, act2, y, ypool, stream};
  c.mid = mid;
  return pair_first_impl(c);
}

extern "C" int vm_conv3x3_pair_first_nhwc(const vm_tensor* x, const void* packed1, int cin1, const float* bias1,
                                          const void* packed2, int cout2, const float* bias2, const float* scale2,
                                          const float* shift2, int act2, vm_tensor* y, vm_tensor* ypool, void* stream) {
  return pair_first_impl({x, packed1, cin1, bias1, packed2, cout2, bias2, scale2, shift2, act2, y, ypool, stream});
}

extern "C" int vm_conv3x3_pair_first_head_nhwc(const vm_tensor* x, const void* packed1, int cin1, const float* bias1,
                                               const void* packed2, int cout2, const float* bias2,
                                               const float* scale2, const float* shift2, int act2, vm_tensor* y,
                                               vm_tensor* ypool, const float* head_w, int head_cin, int head_coff,
                                               float* partial, int store_y, void* stream) {
  if (!head_w || !partial || head_cin <= 0 || head_coff < 0 || head_coff + cout2 > head_cin)
    return fail(VM_EINVAL, "conv3x3_pair_first_head: head filter [3,3,%d,1] with the pair's %d channels at %d",
                head_cin, cout2, head_coff);
  PairCall c{x, packed1, cin1, bias1, packed2, cout2, bias2, scale2, shift2, act2, y, ypool, stream};
  c.head_w = head_w;
  c.head_cin = head_cin;
  c.head_coff = head_coff;
  c.partial = partial;
  c.store_y = store_y;
  return pair_first_impl(c);
}
