// The narrow 3x3 convs (bf16): 2..16 output channels (conv3x3_thin and its LDS-DMA form conv3x3_thin_dma) and 8 or 16
// input channels (conv3x3_narrowin), with their shape tests, split-K plan and launchers (conv_impl routes to them).
#include "conv_dispatch.h"

namespace vm {

// ---------------------------------------------------------------- narrow convs (2 <= cout <= 16)
// The select convs of unet_simple.py:153-168 map 192..1536 channels onto 2..16: a 64-wide output tile would spend
// 4-32x the MFMA work on zero weights, and the conv is really a stream over its input.  One 16-column MFMA tile
// (A = the packed weights' first 16 output channels, B = 16 patch pixels), the (TH+2) x 34 input patch of one
// 32-channel chunk staged in LDS (swizzled 64-byte pixel rows), the next chunk's patch and filter held in registers
// while this one is consumed.  Output lane l: pixel l % 16, channels 4 (l / 16) .. +3.  ksplit > 1 splits the
// chunks over gridDim.y into raw f32 partials (splitk_reduce_kernel, fixed order).
// One chunk of the narrow conv for a wave's RPW output rows: the chunk's 9 filter fragments are read once, and each
// patch row's 6 pixel fragments (3 column shifts x 2 halves) once, each feeding the MFMAs of every output row it
// reaches (kernel row kh = patch row - output row).  Per accumulator the MFMAs still run taps 0..8 in order (patch
// rows ascend with kh), so the sums are those of the tap-major loop bit for bit, with (RPW + 2) * 6 fragment reads
// per chunk instead of RPW * 18.
template <int RPW, int PW>
__device__ __forceinline__ void thin_chunk(const uint4* xs, const uint4* ws, int wv, int lane, f32x4 (&acc)[2 * RPW]) {
  uint4 w[9];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp) w[tp] = ws[tp * 64 + lane];  // A operand: co lane % 16, k = 8 (lane / 16) .. +7
#pragma unroll
  for (int pr = 0; pr < RPW + 2; ++pr) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int pp = (wv * RPW + pr) * PW + h * 16 + (lane & 15) + kw;
        const uint4 b = xs[pp * 4 + ((lane >> 4) ^ (((pp >> 2) & 1) << 1))];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          const int kh = pr - r;
          if (kh >= 0 && kh < 3) mma16<uint16_t>(w[kh * 3 + kw], b, acc[2 * r + h]);
        }
      }
    }
  }
}

template <int TH, bool RR = true>  // RR: thin_chunk's row reuse (false: the r03 tap-major loop, for A/B)
__global__ __launch_bounds__(256, TH <= 4 ? 4 : TH <= 8 ? 3 : 2) void conv3x3_thin(ConvArgs a) {
  constexpr int TW = 32, PW = TW + 2, PPIX = (TH + 2) * PW, PIECES = PPIX * 4, PPT = (PIECES + 255) / 256;
  constexpr int RPW = TH / 4;    // patch rows per wave
  constexpr int WPIECES = 9 * 16 * 4, WPT = (WPIECES + 255) / 256;  // the chunk's filter: [tap][k/8][co 16]
  __shared__ uint4 xs[PPIX * 4];
  __shared__ uint4 ws[WPT * 256];  // tail slots hold clamped duplicates (unconditional stores)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tw = (a.W + TW - 1) / TW, th = (a.H + TH - 1) / TH;
  const int ntiles = a.tiles_total;
  const int nch = a.cin_pad / 32;
  int cb = 0, ce = nch;
  if (a.ksplit > 1) {
    const int per = (nch + a.ksplit - 1) / a.ksplit;
    cb = blockIdx.y * per;
    ce = min(nch, cb + per);
  }
  // persistent: the block walks tiles blockIdx.x, +gridDim.x, ...; with a.twalk (r04) XCD x = blockIdx.x % 8 takes
  // the contiguous eighth [lo, hi) of the tile list and its gridDim.x / 8 blocks every (gridDim.x / 8)-th tile of it,
  // so the tiles resident at once on one XCD are neighbours whose patches share halo rows and 128-byte lines in that
  // XCD's L2 (round-robin placement put horizontally adjacent tiles on different XCDs: FETCH_SIZE 1.8x the input)
  int tile = blockIdx.x, tstep = (int)gridDim.x, tend = ntiles;
  if (a.twalk && (gridDim.x & 7) == 0) {
    const int xcd = blockIdx.x & 7;
    tile = (int)((long)xcd * ntiles / 8) + (int)(blockIdx.x >> 3);
    tstep = (int)(gridDim.x >> 3);
    tend = (int)((long)(xcd + 1) * ntiles / 8);
  }
  if (cb >= ce || tile >= tend) return;
  // the block streams (tile, chunk) steps; the next step's
  // patch and filter pieces (the next tile's first chunk at a tile's end) are in registers while this one computes
  auto geo = [&](int t, int& n, int& r0, int& c0, int (&xo)[PPT]) {
    const int tx = t % tw;
    t /= tw;
    const int ty = t % th;
    n = t / th;
    r0 = ty * TH;
    c0 = tx * TW;
    // byte offsets of this thread's patch pieces inside image n (out of the frame: out of range -> the hardware
    // returns 0, SAME padding); the host guarantees H*W*cstride*2 < 2^31
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = tid + i * 256;
      const int p = id >> 2, q = id & 3;
      const int pr = p / PW, pc = p - pr * PW;
      const int yy = r0 - 1 + pr, xx = c0 - 1 + pc;
      const bool ok = id < PIECES && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      xo[i] = ok ? ((yy * a.W + xx) * a.x_cstride + q * 8) * 2 : OOB;
    }
  };
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7ffffff0, 0x00020000);  // 16 x K_pad bf16 used
  uint4 xr[PPT], wr[WPT];
  // a chunk's patch pieces and filter pieces (tap, k/8, co: the A operand's lane order) into registers
  auto fetch = [&](int n, const int (&xo)[PPT], int cc) {
    const uint16_t* Xn = reinterpret_cast<const uint16_t*>(a.x) + a.x_coff + (long)n * a.H * a.W * a.x_cstride;
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Xn + src_chan(a, cc * 32)), 0, 0x7ffffff0, 0x00020000);
#pragma unroll
    for (int i = 0; i < PPT; ++i)
      xr[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xo[i], 0, 0));
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int id = min(tid + i * 256, WPIECES - 1);
      wr[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                            wrs, ((id & 15) * a.K_pad + (cc * 9 + (id >> 6)) * 32 + ((id >> 4) & 3) * 8) * 2,
                                            0, 0));
    }
  };
  const int co0 = 4 * (lane >> 4);
  const bool splitk = a.ksplit > 1;
  float mul[4], add[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = min(co0 + j, a.cout - 1);
    const float sc = (a.scale && !splitk) ? a.scale[co] : 1.f;
    mul[j] = sc;
    add[j] = splitk ? 0.f : (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
  }

  int n, r0, c0, xo[PPT];
  geo(tile, n, r0, c0, xo);
  fetch(n, xo, cb);
  int cc = cb;
  f32x4 acc[2 * RPW];
#pragma unroll
  for (int f = 0; f < 2 * RPW; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (;;) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = tid + i * 256;
      const int p = id >> 2, q = id & 3;
      if (id < PIECES) xs[p * 4 + (q ^ (((p >> 2) & 1) << 1))] = xr[i];
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) ws[tid + i * 256] = wr[i];
    __syncthreads();
    // the next step: the next chunk of this tile, or the first chunk of the block's next tile
    const bool last = cc + 1 == ce;
    const int ntile = last ? tile + tstep : tile;
    const bool more = ntile < tend;
    int nn = n, nr0 = r0, nc0 = c0, nxo[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) nxo[i] = xo[i];
    if (more) {
      if (last) geo(ntile, nn, nr0, nc0, nxo);
      fetch(nn, nxo, last ? cb : cc + 1);
    }
    if constexpr (RR) {
      thin_chunk<RPW, PW>(xs, ws, wv, lane, acc);
    } else {
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const uint4 w = ws[tp * 64 + lane];  // A operand: output channel lane % 16, k = 8 (lane / 16) .. +7
#pragma unroll
        for (int f = 0; f < 2 * RPW; ++f) {
          const int rr = wv * RPW + (f >> 1), c = (f & 1) * 16 + (lane & 15);
          const int pp = (rr + tp / 3) * PW + c + tp % 3;
          const uint4 b = xs[pp * 4 + ((lane >> 4) ^ (((pp >> 2) & 1) << 1))];
          mma16<uint16_t>(w, b, acc[f]);
        }
        __builtin_amdgcn_sched_barrier(0);  // one tap's fragments live at a time (registers: the prefetch in flight)
      }
    }
    if (last) {  // the tile's epilogue, straight from registers (no LDS: the next step's commit may follow)
      if (co0 < a.cout) {
#pragma unroll
        for (int f = 0; f < 2 * RPW; ++f) {
          const int row = r0 + wv * RPW + (f >> 1), col = c0 + (f & 1) * 16 + (lane & 15);
          if (row >= a.H || col >= a.W) continue;
          const long m = ((long)n * a.H + row) * a.W + col;
          if (splitk) {
            float* d = a.part + ((long)blockIdx.y * a.M + m) * a.cout + co0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (co0 + j < a.cout) d[j] = acc[f][j];
            continue;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (co0 + j >= a.cout) break;
            float v = fmaf(acc[f][j], mul[j], add[j]);
            if (a.act == VM_ACT_RELU) v = fmaxf(v, 0.f);
            else if (a.act == VM_ACT_SIGMOID) v = sigmoid_precise(v);
            const long o = m * a.y_cstride + a.y_coff + co0 + j;
            if (a.y_dtype == VM_BF16) reinterpret_cast<uint16_t*>(a.y)[o] = f2bf(v);
            else reinterpret_cast<float*>(a.y)[o] = v;
          }
        }
      }
#pragma unroll
      for (int f = 0; f < 2 * RPW; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (!more) break;
    tile = ntile;
    cc = last ? cb : cc + 1;
    n = nn;
    r0 = nr0;
    c0 = nc0;
#pragma unroll
    for (int i = 0; i < PPT; ++i) xo[i] = nxo[i];
  }
}

// ---------------------------------------------------------------- narrow-input convs (cin <= 16, cout <= 32)
// UNetSmall's encoder and decoder convs (small.py:39-48: 6 -> 8, 8 -> 16, 16 -> 32, 16 -> 8) hold 8 or 16 channels per
// pixel, so there is no 32-channel granule: K runs tap-major (k = tap * cin_pad + c, the generic packing) and one
// MFMA K-step of 32 takes 4 (tap, 8-channel group) pieces, each a 16-byte LDS read of one patch pixel.  One 8 x 32
// tile per block: its 10 x 34 patch in LDS (G pieces per pixel), the filter (NS K-steps x NT 16-channel tiles) in
// registers.  Output lane l: pixel l % 16, channels 4 (l / 16) .. +3 of the tile.  The MFMAs chain k in ascending
// 32-blocks and the epilogue is conv3x3_mfma's (fmaf form for bf16 outputs, (acc + b) * s + t for f32), so the
// results are bit-identical to the generic kernel's (which spent a 256 x 64 tile and 64-K steps on these).
template <int G, int NT>
__global__ __launch_bounds__(256) void conv3x3_narrowin(ConvArgs a) {
  constexpr int TH = 8, TW = 32, PW = TW + 2, PPIX = (TH + 2) * PW, PIECES = PPIX * G, PPT = (PIECES + 255) / 256;
  constexpr int NQ = 9 * G, NS = (NQ + 3) / 4, RPW = TH / 4;
  __shared__ uint4 xs[PIECES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tw = (a.W + TW - 1) / TW, th = (a.H + TH - 1) / TH;
  int t = blockIdx.x;
  const int tx = t % tw;
  t /= tw;
  const int ty = t % th, n = t / th;
  const int r0 = ty * TH, c0 = tx * TW;
  const uint16_t* Xn = reinterpret_cast<const uint16_t*>(a.x) + a.x_coff + (long)n * a.H * a.W * a.x_cstride;
  const __amdgpu_buffer_rsrc_t xrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(Xn), 0, 0x7ffffff0, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7ffffff0, 0x00020000);
  uint4 xr[PPT], w[NT][NS];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {  // patch pieces: pixel id / G, channel group id % G (out of frame: zeros)
    const int id = tid + i * 256;
    const int p = id / G, q = id - p * G;
    const int pr = p / PW, pc = p - pr * PW;
    const int yy = r0 - 1 + pr, xx = c0 - 1 + pc;
    const bool ok = id < PIECES && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
    xr[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                          xrs, ok ? ((yy * a.W + xx) * a.x_cstride + q * 8) * 2 : OOB, 0, 0));
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)  // A operand: output channel nt * 16 + lane % 16, k = 32 s + 8 (lane / 16) .. +7
#pragma unroll
    for (int s = 0; s < NS; ++s)
      w[nt][s] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                               wrs, ((nt * 16 + (lane & 15)) * a.K_pad + 32 * s + 8 * (lane >> 4)) * 2,
                                               0, 0));
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int id = tid + i * 256;
    if (id < PIECES) xs[id] = xr[i];
  }
  __syncthreads();
  f32x4 acc[NT][2 * RPW];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int f = 0; f < 2 * RPW; ++f) acc[nt][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int q = 4 * s + (lane >> 4);
    const bool kv = q < NQ;  // K padding past tap 8: zero pieces (the packed filter is zero there too)
    const int tap = kv ? q / G : 0, g = q - (q / G) * G;
    const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
    for (int f = 0; f < 2 * RPW; ++f) {
      const int pp = (wv * RPW + (f >> 1) + kh) * PW + (f & 1) * 16 + (lane & 15) + kw;
      uint4 b = xs[pp * G + (kv ? g : 0)];
      if (!kv) b = uint4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) mma16<uint16_t>(w[nt][s], b, acc[nt][f]);
    }
  }
  const bool f32o = a.y_dtype == VM_F32;
  const bool fma_form = !f32o && a.y_vec && (a.cout & 7) == 0;  // conv3x3_mfma's fast bf16 epilogue, else its general one
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co0 = nt * 16 + 4 * (lane >> 4);
    if (co0 >= a.cout) continue;
    float bs[4], sc[4], sh[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = min(co0 + j, a.cout - 1);
      bs[j] = a.bias ? a.bias[co] : 0.f;
      sc[j] = a.scale ? a.scale[co] : 1.f;
      sh[j] = a.shift ? a.shift[co] : 0.f;
    }
    const bool full = co0 + 4 <= a.cout && a.y_vec;
#pragma unroll
    for (int f = 0; f < 2 * RPW; ++f) {
      const int row = r0 + wv * RPW + (f >> 1), col = c0 + (f & 1) * 16 + (lane & 15);
      if (row >= a.H || col >= a.W) continue;
      const long o = (((long)n * a.H + row) * a.W + col) * a.y_cstride + a.y_coff + co0;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float tv = fma_form ? fmaf(acc[nt][f][j], sc[j], bs[j] * sc[j] + sh[j]) : (acc[nt][f][j] + bs[j]) * sc[j] + sh[j];
        if (a.act == VM_ACT_RELU) tv = fma_form ? fmaxf(tv, 0.f) : (tv > 0.f ? tv : 0.f);
        else if (a.act == VM_ACT_SIGMOID) tv = sigmoid_precise(tv);
        v[j] = tv;
      }
      if (f32o) {
        float* Y = reinterpret_cast<float*>(a.y) + o;
        if (full) {
          *reinterpret_cast<float4*>(Y) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co0 + j < a.cout) Y[j] = v[j];
        }
      } else {
        uint16_t* Y = reinterpret_cast<uint16_t*>(a.y) + o;
        if (full) {
          *reinterpret_cast<uint2*>(Y) = uint2{bf16x2_bits(v[0], v[1]), bf16x2_bits(v[2], v[3])};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co0 + j < a.cout) Y[j] = f2bf(v[j]);
        }
      }
    }
  }
}

// LDS-DMA form of conv3x3_thin (r04).  The select convs are a stream over 192..1536-channel tower features (1.3 GB
// per training step) and conv3x3_thin ran them at 1.1-2.8 TB/s: one chunk in flight per block, its patch and filter
// held in registers from the end of one chunk's compute to the start of the next, so every chunk exposed most of
// the load latency.  Here chunk t+S-1's patch and filter are DMA'd (buffer_load ... lds) into an S-slot LDS ring
// while chunk t computes: S-1 chunks in flight per block, no registers held.  One raw barrier per chunk, after the
// wave's own DMAs of chunk t have landed (counted vmcnt: every thread issues exactly PPT + WPT pieces per step;
// steps past the end load out-of-range zeros) and its fragment reads of chunk t-1 have retired (lgkmcnt(0): the
// slot the next DMA overwrites).  The patch swizzle is applied on the source side (LDS position p*4 + q holds
// piece (p, q ^ swz(p))); MFMA order and epilogue are conv3x3_thin's, so results are bit-identical to it.
template <int TH, int S>
__global__ __launch_bounds__(256, 1) void conv3x3_thin_dma(ConvArgs a) {
  constexpr int TW = 32, PW = TW + 2, PPIX = (TH + 2) * PW, PIECES = PPIX * 4, PPT = (PIECES + 255) / 256;
  constexpr int RPW = TH / 4;
  constexpr int WPIECES = 9 * 16 * 4, WPT = (WPIECES + 255) / 256;
  constexpr int XS = PPT * 256 * 16, WS = WPT * 256 * 16, SLOT = XS + WS, NP = PPT + WPT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tw = (a.W + TW - 1) / TW, th = (a.H + TH - 1) / TH;
  const int ntiles = a.tiles_total;
  const int nch = a.cin_pad / 32;
  int cb = 0, ce = nch;
  if (a.ksplit > 1) {
    const int per = (nch + a.ksplit - 1) / a.ksplit;
    cb = blockIdx.y * per;
    ce = min(nch, cb + per);
  }
  if (cb >= ce || (int)blockIdx.x >= ntiles) return;
  const int nsteps_per_tile = ce - cb;
  // step j of this block: tile blockIdx.x + (j / nsteps) * gridDim.x, chunk cb + j % nsteps
  const int ntile_blk = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int nsteps = ntile_blk * nsteps_per_tile;
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, 0x7ffffff0, 0x00020000);
  const uint32_t lds0 = lds_addr(smem);
  // DMA of step j into slot j % S (j >= nsteps: out-of-range zeros, so every step issues NP pieces)
  auto issue = [&](int j) __attribute__((always_inline)) {
    const bool real = j < nsteps;
    const int jj = real ? j : 0;
    const int t = (int)blockIdx.x + (jj / nsteps_per_tile) * (int)gridDim.x;
    const int cc = cb + jj % nsteps_per_tile;
    int tt = t;
    const int tx = tt % tw;
    tt /= tw;
    const int ty = tt % th;
    const int n = tt / th;
    const int r0 = ty * TH, c0 = tx * TW;
    const uint16_t* Xn = reinterpret_cast<const uint16_t*>(a.x) + a.x_coff + (long)n * a.H * a.W * a.x_cstride +
                         src_chan(a, cc * 32);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<uint16_t*>(Xn)), 0,
                                                                         0x7ffffff0, 0x00020000);
    const uint32_t slot = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)((j % S) * SLOT));
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = tid + i * 256;
      const int p = id >> 2, qq = id & 3;
      const int q = qq ^ (((p >> 2) & 1) << 1);  // the piece whose swizzled home is LDS position id
      const int pr = p / PW, pc = p - pr * PW;
      const int yy = r0 - 1 + pr, xx = c0 - 1 + pc;
      const bool ok = real & (id < PIECES) & ((unsigned)yy < (unsigned)a.H) & ((unsigned)xx < (unsigned)a.W);
      const int off = ((yy * a.W + xx) * a.x_cstride + q * 8) * 2;  // (32-bit: checked by the host)
      glds16(xrs, slot + (uint32_t)((i * 256 + wv * 64) * 16), ok ? off : OOB);
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int id = tid + i * 256;
      const bool ok = real & (id < WPIECES);
      const int off = ((id & 15) * a.K_pad + (cc * 9 + (id >> 6)) * 32 + ((id >> 4) & 3) * 8) * 2;
      glds16(wrs, slot + (uint32_t)(XS + (i * 256 + wv * 64) * 16), ok ? off : OOB);
    }
  };
  const int co0 = 4 * (lane >> 4);
  const bool splitk = a.ksplit > 1;
  float mul[4], add[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = min(co0 + j, a.cout - 1);
    const float sc = (a.scale && !splitk) ? a.scale[co] : 1.f;
    mul[j] = sc;
    add[j] = splitk ? 0.f : (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the epilogue constants: nothing older in the DMA counts
#pragma unroll
  for (int j = 0; j < S - 1; ++j) issue(j);
  f32x4 acc[2 * RPW];
#pragma unroll
  for (int f = 0; f < 2 * RPW; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  int tile = blockIdx.x;
  for (int j = 0; j < nsteps; ++j) {
    // chunk j landed (the S-2 younger steps may stay in flight); this wave's reads of slot (j-1) % S retired
    if constexpr (S == 2) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else wait_vm((S - 2) * NP);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    issue(j + S - 1);  // into slot (j - 1) % S, free since the barrier
    const uint4* xs = reinterpret_cast<const uint4*>(smem + (j % S) * SLOT);
    const uint4* ws = reinterpret_cast<const uint4*>(smem + (j % S) * SLOT + XS);
    thin_chunk<RPW, PW>(xs, ws, wv, lane, acc);
    if ((j + 1) % nsteps_per_tile == 0) {  // the tile's epilogue (conv3x3_thin's), straight from registers
      int t = tile;
      const int tx = t % tw;
      t /= tw;
      const int ty = t % th;
      const int n = t / th;
      const int r0 = ty * TH, c0 = tx * TW;
      if (co0 < a.cout) {
#pragma unroll
        for (int f = 0; f < 2 * RPW; ++f) {
          const int row = r0 + wv * RPW + (f >> 1), col = c0 + (f & 1) * 16 + (lane & 15);
          if (row >= a.H || col >= a.W) continue;
          const long m = ((long)n * a.H + row) * a.W + col;
          if (splitk) {
            float* d = a.part + ((long)blockIdx.y * a.M + m) * a.cout + co0;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
              if (co0 + jj < a.cout) d[jj] = acc[f][jj];
            continue;
          }
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            if (co0 + jj >= a.cout) break;
            float v = fmaf(acc[f][jj], mul[jj], add[jj]);
            if (a.act == VM_ACT_RELU) v = fmaxf(v, 0.f);
            else if (a.act == VM_ACT_SIGMOID) v = sigmoid_precise(v);
            const long o = m * a.y_cstride + a.y_coff + co0 + jj;
            if (a.y_dtype == VM_BF16) reinterpret_cast<uint16_t*>(a.y)[o] = f2bf(v);
            else reinterpret_cast<float*>(a.y)[o] = v;
          }
        }
      }
#pragma unroll
      for (int f = 0; f < 2 * RPW; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      tile += gridDim.x;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing zero-fill DMAs land before the block exits
}
template <int TH, int S>
constexpr int thin_dma_lds() {
  constexpr int PPT = ((TH + 2) * 34 * 4 + 255) / 256, WPT = (9 * 16 * 4 + 255) / 256;
  return S * (PPT + WPT) * 256 * 16;
}

// narrow-cout convs (conv3x3_thin): bf16, chunk-major 32-channel granules, 2..16 output channels, no pool / resize
bool thin_ok(int dt, const PackGeom& g, int cout, int x_src_c, int act, const vm_tensor* x) {
  return g_opt.thin_kernel && dt == VM_BF16 && cout >= 2 && cout <= 16 && g.chunk_major && g.cin_pad % 32 == 0 &&
         (x_src_c <= 0 || x_src_c % 32 == 0) && act != VM_ACT_SOFTMAX &&
         (long)x->h * x->w * x->cstride * 2 < 0x7ffffff0L;  // 32-bit byte offsets inside one image
}
// narrow-input convs (conv3x3_narrowin): bf16, 8 or 16 tap-major input channels, <= 32 outputs, one source
bool narrowin_ok(const ConvArgs& a, const PackGeom& g, int cout, int act, const vm_tensor* x, const vm_tensor* y) {
  return g_opt.narrowin_kernel && !g.chunk_major && (g.cin_pad == 8 || g.cin_pad == 16) && cout <= 32 && a.x_src_c <= 0 &&
         act != VM_ACT_SOFTMAX && (y->dtype == VM_F32 || y->dtype == VM_BF16) && g.K_pad >= 32 * ((9 * g.cin_pad / 8 + 3) / 4) &&
         (long)x->h * x->w * x->cstride * 2 < 0x7ffffff0L;
}
int launch_narrowin(ConvArgs& a, long n, const PackGeom& g, hipStream_t st) {
  const long tiles = n * ((a.H + 7) / 8) * (long)((a.W + 31) / 32);
  if (tiles > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3_narrowin: too many tiles");
  const int G = g.cin_pad / 8, NT = a.cout > 16 ? 2 : 1;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_narrowin<%d, %d>", G, NT);
  const dim3 grid((unsigned)tiles);
  if (G == 1 && NT == 1) hipLaunchKernelGGL((conv3x3_narrowin<1, 1>), grid, dim3(256), 0, st, a);
  else if (G == 1) hipLaunchKernelGGL((conv3x3_narrowin<1, 2>), grid, dim3(256), 0, st, a);
  else if (NT == 1) hipLaunchKernelGGL((conv3x3_narrowin<2, 1>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((conv3x3_narrowin<2, 2>), grid, dim3(256), 0, st, a);
  return check_launch("conv3x3_narrowin");
}
// split-K plan: below 1024 blocks of 8 x 32 pixels, split the 32-channel chunks over ~thin_blocks (512) blocks
int thin_splitk_plan(long n, int h, int w, int cin_pad) {
  const long tiles = n * ((h + 7) / 8) * ((w + 31) / 32);  // in 8-row units whatever the tile height
  const int nch = cin_pad / 32;
  if (tiles <= 0 || tiles >= 1024 || nch < 4) return 1;
  int ks = (int)((g_opt.thin_blocks + tiles - 1) / tiles);
  if (ks > nch / 2) ks = nch / 2;
  if (ks < 2) return 1;
  const int per = (nch + ks - 1) / ks;
  return (nch + per - 1) / per;
}
// persistent grid: at most g_opt.thin_rounds resident rounds of blocks (0: one block per tile, the r02 launch)
template <int TH>
static int thin_resident() {
  static int dev_seen = -1, resident = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != dev_seen) {
    int per_cu = 0, n_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void*>(&conv3x3_thin<TH, true>), 256, 0);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return -1;
    resident = per_cu * n_cu;
    dev_seen = dev;
  }
  return resident;
}
template <int TH, int S>
static int launch_thin_dma_cfg(ConvArgs& a, long n, int ks, hipStream_t st) {
  constexpr int lds = thin_dma_lds<TH, S>();
  static int dev_seen = -1, resident = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != dev_seen) {
    const void* fn = reinterpret_cast<const void*>(&conv3x3_thin_dma<TH, S>);
    int per_cu = 0, n_cu = 0;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return fail(VM_EHIP, "conv3x3_thin_dma: %s", hipGetErrorString(e));
    resident = per_cu * n_cu;
    dev_seen = dev;
  }
  long gx = n * ((a.H + TH - 1) / TH) * (long)((a.W + 31) / 32);
  if (gx > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3_thin_dma: too many tiles");
  a.tiles_total = (int)gx;
  const long cap = g_opt.thin_dma_rounds * (long)resident / ks;
  if (gx > cap) gx = cap < 1 ? 1 : cap;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_thin_dma<%d, %d>", TH, S);
  hipLaunchKernelGGL((conv3x3_thin_dma<TH, S>), dim3((unsigned)gx, ks), dim3(256), lds, st, a);
  return check_launch("conv3x3_thin_dma");
}
static int launch_thin_dma(ConvArgs& a, long n, int ks, hipStream_t st) {
  switch (g_opt.thin_dma) {
    case 2: return launch_thin_dma_cfg<4, 4>(a, n, ks, st);
    case 3: return launch_thin_dma_cfg<4, 3>(a, n, ks, st);
    case 4: return launch_thin_dma_cfg<8, 2>(a, n, ks, st);
    default: return launch_thin_dma_cfg<8, 3>(a, n, ks, st);
  }
}
// the thin conv at tile height TH: conv3x3_thin<TH, thin_rowreuse> on at most g_opt.thin_rounds resident rounds of
// blocks, or (thin_dma) the LDS-DMA form
template <int TH>
static int launch_thin(ConvArgs& a, long n, int ks, hipStream_t st) {
  const int res = thin_resident<TH>();
  if (res < 0) return fail(VM_EHIP, "conv3x3_thin: occupancy query failed");
  if (g_opt.thin_dma) return launch_thin_dma(a, n, ks, st);
  long gx = a.tiles_total;
  if (g_opt.thin_rounds > 0 && res > 0) {
    const long cap = g_opt.thin_rounds * (long)res / ks;
    if (gx > cap) gx = cap < 1 ? 1 : cap;
  }
  const dim3 grid((unsigned)gx, ks);
  a.twalk = (int)g_opt.thin_twalk;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_thin<%d, %s>", TH, g_opt.thin_rowreuse ? "true" : "false");
  if (g_opt.thin_rowreuse) hipLaunchKernelGGL((conv3x3_thin<TH, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((conv3x3_thin<TH, false>), grid, dim3(256), 0, st, a);
  return check_launch("conv3x3_thin");
}
int dispatch_thin(ConvArgs& a, long n, hipStream_t st) {
  const int th = (int)g_opt.thin_th;
  const long tiles = n * ((a.H + th - 1) / th) * ((a.W + 31) / 32);
  if (tiles > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3_thin: too many tiles");
  a.tiles_total = (int)tiles;
  const int ks = a.ksplit > 1 ? a.ksplit : 1;
  const int rc = th == 16 ? launch_thin<16>(a, n, ks, st) : th == 4 ? launch_thin<4>(a, n, ks, st) : launch_thin<8>(a, n, ks, st);
  return rc || a.ksplit <= 1 ? rc : launch_splitk_reduce(a, st);
}

}  // namespace vm
