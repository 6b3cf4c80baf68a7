// The narrow-cout MFMA weight gradients of the bf16 training path with the 9 taps packed into the GEMM's N axis: the
// register-staged kernel (cout <= 8) and its LDS-DMA form (cout <= 16).  wgrad.hip's launch_wgrad_mfma routes to them.

#include "wgrad_common.h"

namespace vm {
namespace trn {

// Narrow-cout weight gradient with the taps packed into N (select convs, cout <= 8): one GEMM
//   dW[ci][t*cout + co] = sum_q X[q][ci] * DY[q - off_t][co]
// whose N axis holds all 9 taps x cout columns (cout 2 -> 18 of 32, 4 -> 36 of 48, 8 -> 72 of 80), so a K-step of 32
// pixels costs NCI x NT MFMAs (2 x 4 = 8 for cout 2) where wgrad_mfma_kernel's !SX form spends 9 per 16 channels
// on one 16-wide column block holding cout of them.  The B fragments come from three bf16 planes of the DY patch,
// plane kw pre-shifted by its tap column (P_kw[r][j] = patch(r, j + 2 - kw)), so every lane's 8 pixels are one
// aligned 16-byte LDS read: lane (n, g) reads P_kw[row + 2 - kh][8g .. 8g + 7] of channel co, (kh, kw, co) = n's tap.
// With 32-80 accumulator registers a block holds 64 input channels (one tower source: 128-byte pixel rows) and
// 8 blocks fit a CU, so ~4x the bytes of X are in flight per CU than with the 160-register variants — the select
// wgrads read 40-315 MB of tower features each and are bound by that.
template <int TH>
constexpr int wt_drows() { return TH + 2; }

template <int NCI, int NT, int TH>
__global__ __launch_bounds__(256) void wgrad_taps_kernel(WgArgs a) {
  constexpr int CIB = NCI * 16;
  constexpr int RBX = NCI == 1 ? 32 : NCI == 2 ? 64 : 128;
  constexpr int XPIX = TH * WM_TW, XCH = CIB / 8, NXC = XPIX * XCH, XPT = (NXC + 255) / 256;
  constexpr int DR = wt_drows<TH>();
  constexpr int COMAX = NT * 16 / 9;                        // the widest cout this NT serves
  constexpr int NDE = DR * WM_PW * COMAX, DPT = (NDE + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.y * CIB;
  const int cout = a.cout, ndy = DR * WM_PW * cout;
  char* ximg = smem;
  uint16_t* dpl = reinterpret_cast<uint16_t*>(smem + XPIX * RBX);  // [3][cout][DR][32]

  f32x4 acc[NCI][NT];
#pragma unroll
  for (int i = 0; i < NCI; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's B column: n = nt * 16 + (lane & 15) -> (tap, co); columns past 9 * cout read a zero slot
  const int g = lane >> 4;
  int boff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = t * 16 + (lane & 15);
    if (n < 9 * cout) {
      const int tap = n / cout, co = n - tap * cout, kh = tap / 3, kw = tap - kh * 3;
      boff[t] = ((kw * cout + co) * DR + 2 - kh) * WM_TW + 8 * g;  // + row * 32 per K-step
    } else {
      boff[t] = -1;
    }
  }

  uint4 xb[XPT];
  float db[DPT];
  auto coords = [&](int tile, int& n, int& y0, int& x0) {
    const int tx = tile % a.tiles_w;
    const int t2 = tile / a.tiles_w;
    y0 = (t2 % a.tiles_h) * TH;
    n = t2 / a.tiles_h;
    x0 = tx * WM_TW;
  };
  auto issue = [&](int tile) {
    int n, y0, x0;
    coords(tile, n, y0, x0);
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int e = tid + k * 256;
      xb[k] = make_uint4(0, 0, 0, 0);
      if (NXC % 256 == 0 || e < NXC) {
        const int pe = e / XCH, j = e % XCH;
        const int gy = y0 + pe / WM_TW, gx = x0 + pe % WM_TW, c = c0 + j * 8;
        if (gy < a.h && gx < a.w && c < a.cin) {
          long off = (((long)n * a.h + gy) * a.w + gx) * a.xcs;
          if (a.x_src_c > 0) off += (long)(c / a.x_src_c) * a.x_src_stride + c % a.x_src_c;
          else off += c;
          xb[k] = *reinterpret_cast<const uint4*>(a.x + off);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {  // the halo patch, (pixel, co) elements in memory order
      const int e = tid + k * 256;
      db[k] = 0.f;
      if (e < ndy) {
        const int pe = e / cout, co = e - pe * cout;
        const int gy = y0 - 1 + pe / WM_PW, gx = x0 - 1 + pe % WM_PW;
        if ((unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w)
          db[k] = a.dy[(((long)n * a.h + gy) * a.w + gx) * a.dcs + co];
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int e = tid + k * 256;
      if (NXC % 256 == 0 || e < NXC) {
        const int pe = e / XCH, j = e % XCH;
        uint4 v = xb[k];
        const int c = c0 + j * 8;
        if (c + 8 > a.cin) {  // a chunk straddling cin (padded views): zero the lanes past it
          uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (c + 2 * i >= a.cin) w4[i] = 0u;
            else if (c + 2 * i + 1 >= a.cin) w4[i] &= 0xffffu;
          }
          v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
        *reinterpret_cast<uint4*>(ximg + wm_off<RBX>(pe, j >> 1) + (j & 1) * 16) = v;
      }
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
      const int e = tid + k * 256;
      if (e < ndy) {
        const int pe = e / cout, co = e - pe * cout;
        const int r = pe / WM_PW, pc = pe % WM_PW;
        const uint16_t v = f2bf(db[k]);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int j = pc - 2 + kw;
          if (j >= 0 && j < WM_TW) dpl[((kw * cout + co) * DR + r) * WM_TW + j] = v;
        }
      }
    }
  };

  const int t_beg = (int)((long)blockIdx.x * a.ntiles / gridDim.x);
  const int t_end = (int)((long)(blockIdx.x + 1) * a.ntiles / gridDim.x);
  if (t_beg < t_end) issue(t_beg);
  for (int tile = t_beg; tile < t_end; ++tile) {
    commit();
    __syncthreads();
    if (tile + 1 < t_end) issue(tile + 1);
#pragma unroll
    for (int rr = 0; rr < TH / 4; ++rr) {
      const int row = wave + 4 * rr;
      bf16x8 ax[NCI];
#pragma unroll
      for (int i = 0; i < NCI; ++i) ax[i] = wm_frag<RBX>(ximg, row * WM_TW + 8 * g, i, lane);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x8 bd = {};
        if (boff[t] >= 0) bd = *reinterpret_cast<const bf16x8*>(dpl + boff[t] + row * WM_TW);
#pragma unroll
        for (int i = 0; i < NCI; ++i) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[i], bd, acc[i][t], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // fold the 4 waves' accumulators (LDS, two rounds), wave 0 stores the block's partial
  float* red = reinterpret_cast<float*>(smem);
  constexpr int NA = NCI * NT * 4;
  auto put = [&](int slot) {
#pragma unroll
    for (int i = 0; i < NCI; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[(slot * NA + (i * NT + t) * 4 + j) * 64 + lane] = acc[i][t][j];
  };
  auto add = [&](int slot) {
#pragma unroll
    for (int i = 0; i < NCI; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][t][j] += red[(slot * NA + (i * NT + t) * 4 + j) * 64 + lane];
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) add(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave == 0) {
    add(0);
    float* part = a.part + (long)blockIdx.x * 9 * a.cin * cout;
    const int ci_l = 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 16 + (lane & 15);
      if (n < 9 * cout) {
        const int tap = n / cout, co = n - tap * cout;
#pragma unroll
        for (int i = 0; i < NCI; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ci = c0 + i * 16 + ci_l + j;
            if (ci < a.cin) part[((long)tap * a.cin + ci) * cout + co] = acc[i][t][j];
          }
      }
    }
  }
  (void)COMAX;
}

template <int NCI, int NT, int TH>
constexpr int wgrad_taps_lds() {
  constexpr int RBX = NCI == 1 ? 32 : NCI == 2 ? 64 : 128;
  constexpr int COMAX = NT * 16 / 9;
  constexpr int MAIN = TH * WM_TW * RBX + 3 * COMAX * wt_drows<TH>() * WM_TW * 2;
  constexpr int RED = 2 * NCI * NT * 4 * 64 * 4;
  return MAIN > RED ? MAIN : RED;
}

// ---------------------------------------------------------------- narrow weight gradient, LDS-DMA stream (r05)
// The select convs' weight gradients (unet_simple.py:120-139 through train.py:288-304's minimize) read 39-315 MB of
// tower features each for a few GFLOP: a stream.  wgrad_taps_kernel stages one 4 x 32-pixel tile per block in
// registers and exposes its load latency every step (2.0 TB/s at 320^2, 0.4 TB/s at 40^2 on MI355X; 1.0 ms of the
// 4.9 ms step).  Here the X tiles and the f32 DY halo patches are DMA'd (buffer_load ... lds) into an S-slot LDS
// ring, S-1 tiles in flight per block and no staging registers, so two blocks per CU keep ~100 KB in flight.  Same
// GEMM as wgrad_taps_kernel (taps in N, B from the three pre-shifted bf16 DY planes, built from the landed f32 patch
// after the ring barrier), same tiles per block and the same MFMA order: the partials are bit-identical to it.
// The X image keeps wm_off's swizzle by permuting the SOURCE chunk of each LDS position (the DMA writes lane-linear).
// cout <= 16 (NT <= 9 column tiles); cin a multiple of 8, the block's 16 NCI channels inside one source.
template <int RB>
__device__ __forceinline__ void wm_src(int e, int& pe, int& j) {  // LDS chunk e of the X image -> (pixel, chunk)
  if constexpr (RB == 32) {
    const int r = e >> 1;
    pe = r ^ (((r >> 3) & 1) << 2);
    j = e & 1;
  } else if constexpr (RB == 64) {
    const int r = e >> 2, s = e & 3;
    pe = r;
    j = 2 * ((s >> 1) ^ ((r >> 3) & 1)) + (s & 1);
  } else {
    const int r = e >> 3, s = e & 7;
    pe = r;
    j = 2 * ((s >> 1) ^ ((r >> 1) & 1) ^ (((r >> 3) & 1) << 1)) + (s & 1);
  }
}

// one 4-byte-per-lane LDS-DMA (buffer_load_dword ... offen lds): lane l writes lds_dst + 4 l (see glds16)
__device__ __forceinline__ void glds4(__amdgpu_buffer_rsrc_t rsrc, uint32_t lds_dst, int voffset) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "buffer_load_dword %1, %3, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voffset), "s"(lds_dst), "s"(rsrc)
      : "memory");
}

template <int NCI, int NT, int TH_>
struct WtDma {
  static constexpr int TH = TH_, CIB = NCI * 16, RBX = NCI == 1 ? 32 : NCI == 2 ? 64 : 128;
  static constexpr int XPIX = TH * WM_TW, XCH = CIB / 8, NXC = XPIX * XCH, XPT = (NXC + 255) / 256;
  static constexpr int DR = TH + 2, COMAX = NT * 16 / 9, NDE = DR * WM_PW * COMAX, DPT = (NDE + 255) / 256;
  static constexpr int XS = XPT * 256 * 16, DS = DPT * 256 * 4, SLOT = XS + DS, NP = XPT + DPT;
  static constexpr int PLANES = 3 * COMAX * DR * WM_TW * 2;
  static constexpr int RED = 2 * NCI * NT * 4 * 64 * 4;
  template <int S>
  static constexpr int lds() { return S * SLOT + PLANES > RED ? S * SLOT + PLANES : RED; }
};

template <int NCI, int NT, int TH_, int S>
__global__ __launch_bounds__(256, 2) void wgrad_taps_dma_kernel(WgArgs a) {
  using C = WtDma<NCI, NT, TH_>;
  constexpr int TH = C::TH, RBX = C::RBX, XPT = C::XPT, DPT = C::DPT, DR = C::DR, NP = C::NP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.y * C::CIB;
  const int cout = a.cout, ndy = DR * WM_PW * cout;
  uint16_t* dpl = reinterpret_cast<uint16_t*>(smem + S * C::SLOT);  // [3][cout][DR][32]
  const uint32_t lds0 = lds_addr(smem);

  f32x4 acc[NCI][NT];
#pragma unroll
  for (int i = 0; i < NCI; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4;
  int boff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = t * 16 + (lane & 15);
    if (n < 9 * cout) {
      const int tap = n / cout, co = n - tap * cout, kh = tap / 3, kw = tap - kh * 3;
      boff[t] = ((kw * cout + co) * DR + 2 - kh) * WM_TW + 8 * g;
    } else {
      boff[t] = -1;
    }
  }
  // this block's channel slice inside its source (the host checks it does not straddle two)
  const long xsrc = a.x_src_c > 0 ? (long)(c0 / a.x_src_c) * a.x_src_stride + c0 % a.x_src_c : (long)c0;
  const int t_beg = (int)((long)blockIdx.x * a.ntiles / gridDim.x);
  const int t_end = (int)((long)(blockIdx.x + 1) * a.ntiles / gridDim.x);
  const int nsteps = t_end - t_beg;
  // DMA of step j (tile t_beg + j) into slot j % S; steps past the end load out-of-range zeros, so every thread
  // issues exactly NP pieces per step and the counted waits stay uniform
  auto issue = [&](int j) __attribute__((always_inline)) {
    const bool real = j < nsteps;
    const int tile = t_beg + (real ? j : 0);
    const int tx = tile % a.tiles_w, t2 = tile / a.tiles_w;
    const int y0 = (t2 % a.tiles_h) * TH, n = t2 / a.tiles_h, x0 = tx * WM_TW;
    const uint16_t* Xn = a.x + (long)n * a.h * a.w * a.xcs + xsrc;
    const float* Dn = a.dy + (long)n * a.h * a.w * a.dcs;
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<uint16_t*>(Xn)), 0, 0x7ffffff0, 0x00020000);
    const __amdgpu_buffer_rsrc_t drs =
        __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<float*>(Dn)), 0, 0x7ffffff0, 0x00020000);
    const uint32_t slot = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)((j % S) * C::SLOT));
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int e = tid + k * 256;
      int pe, jj;
      wm_src<RBX>(e, pe, jj);
      const int gy = y0 + pe / WM_TW, gx = x0 + pe % WM_TW, c = c0 + jj * 8;
      const bool ok = real & (e < C::NXC) & (gy < a.h) & (gx < a.w) & (c < a.cin);
      glds16(xrs, slot + (uint32_t)((k * 256 + wave * 64) * 16), ok ? ((gy * a.w + gx) * a.xcs + jj * 8) * 2 : OOB);
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {  // the halo patch, (pixel, co) elements in memory order
      const int e = tid + k * 256;
      const int pe = e / cout, co = e - pe * cout;
      const int gy = y0 - 1 + pe / WM_PW, gx = x0 - 1 + pe % WM_PW;
      const bool ok = real & (e < ndy) & ((unsigned)gy < (unsigned)a.h) & ((unsigned)gx < (unsigned)a.w);
      glds4(drs, slot + (uint32_t)(C::XS + (k * 256 + wave * 64) * 4), ok ? ((gy * a.w + gx) * a.dcs + co) * 4 : OOB);
    }
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing older in the DMA counts
#pragma unroll
  for (int j = 0; j < S - 1; ++j) issue(j);
  for (int j = 0; j < nsteps; ++j) {
    // step j landed (this wave's own DMAs; the S-2 younger steps may fly), then everyone's, and every wave's reads
    // of step j-1 (slot (j-1) % S and the planes) retired
    wait_vm((S - 2) * NP);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    issue(j + S - 1);  // into slot (j - 1) % S
    const char* ximg = smem + (j % S) * C::SLOT;
    const float* dys = reinterpret_cast<const float*>(ximg + C::XS);
    for (int e = tid; e < ndy; e += 256) {  // the three pre-shifted bf16 DY planes (wgrad_taps_kernel's commit)
      const int pe = e / cout, co = e - pe * cout;
      const int r = pe / WM_PW, pc = pe % WM_PW;
      const uint16_t v = f2bf(dys[e]);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int jx = pc - 2 + kw;
        if (jx >= 0 && jx < WM_TW) dpl[((kw * cout + co) * DR + r) * WM_TW + jx] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < TH / 4; ++rr) {  // K-steps: tile rows wave, wave + 4 (wgrad_taps_kernel's order)
      const int row = wave + 4 * rr;
      bf16x8 ax[NCI];
#pragma unroll
      for (int i = 0; i < NCI; ++i) ax[i] = wm_frag<RBX>(ximg, row * WM_TW + 8 * g, i, lane);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x8 bd = {};
        if (boff[t] >= 0) bd = *reinterpret_cast<const bf16x8*>(dpl + boff[t] + row * WM_TW);
#pragma unroll
        for (int i = 0; i < NCI; ++i)
          acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[i], bd, acc[i][t], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // ring drained: LDS reused

  float* red = reinterpret_cast<float*>(smem);
  constexpr int NA = NCI * NT * 4;
  auto put = [&](int sl) {
#pragma unroll
    for (int i = 0; i < NCI; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(sl * NA + (i * NT + t) * 4 + q) * 64 + lane] = acc[i][t][q];
  };
  auto add = [&](int sl) {
#pragma unroll
    for (int i = 0; i < NCI; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][t][q] += red[(sl * NA + (i * NT + t) * 4 + q) * 64 + lane];
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) add(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave == 0) {
    add(0);
    float* part = a.part + (long)blockIdx.x * 9 * a.cin * cout;
    const int ci_l = 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 16 + (lane & 15);
      if (n < 9 * cout) {
        const int tap = n / cout, co = n - tap * cout;
#pragma unroll
        for (int i = 0; i < NCI; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int ci = c0 + i * 16 + ci_l + q;
            if (ci < a.cin) part[((long)tap * a.cin + ci) * cout + co] = acc[i][t][q];
          }
      }
    }
  }
}

template <int NCI, int TH, int... NTS>
static int launch_wgrad_taps_t(WgArgs& a, int nt, float* dw, hipStream_t st) {
  return dispatch<NTS...>(nt, [&](auto nt_c) {
    constexpr int NT = decltype(nt_c)::value;
    return launch_wgrad_grid_k<wgrad_taps_kernel<NCI, NT, TH>>(wgrad_taps_lds<NCI, NT, TH>(), TH, NCI * 16, a, dw, st);
  });
}

// NT = nt column tiles: 1-5 for 16 / 32 input channels per block, 1-3 for 64; 4- or 8-row tiles
int launch_wgrad_taps(WgArgs& a, int nci, int nt, int th, float* dw, hipStream_t st) {
  return dispatch<8, 4>(th, [&](auto th_c) {
    constexpr int TH = decltype(th_c)::value;
    if (nci == 1) return launch_wgrad_taps_t<1, TH, 1, 2, 3, 4, 5>(a, nt, dw, st);
    if (nci == 2) return launch_wgrad_taps_t<2, TH, 1, 2, 3, 4, 5>(a, nt, dw, st);
    return launch_wgrad_taps_t<4, TH, 1, 2, 3>(a, nt, dw, st);
  });
}

// the LDS-DMA kernel takes 64 input channels per block where its column tiles leave the registers (NT <= 5), else 32
static int wgrad_dma_nci(const WgArgs& a) { return (9 * a.cout + 15) / 16 <= 5 && a.cin > 32 ? 4 : 2; }

// the LDS-DMA narrow weight gradient: cout <= 16, 8-channel chunks, the block's channels inside one source, 32-bit
// byte offsets inside one image
bool wgrad_dma_ok(const WgArgs& a) {
  const int cib = wgrad_dma_nci(a) * 16;
  return g_wgrad_dma && a.cout >= 1 && a.cout <= 16 && a.cin % 8 == 0 && a.xcs % 8 == 0 &&
         reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && (a.x_src_c <= 0 || (a.x_src_c % cib == 0 && a.x_src_stride % 8 == 0)) &&
         (long)a.h * a.w * a.xcs * 2 < 0x7ff00000L && (long)a.h * a.w * a.dcs * 4 < 0x7ff00000L;
}

template <int NCI, int NT, int TH, int S>
static int launch_wgrad_taps_dma_s(WgArgs& a, float* dw, hipStream_t st) {
  return launch_wgrad_grid_k<wgrad_taps_dma_kernel<NCI, NT, TH, S>>(WtDma<NCI, NT, TH>::template lds<S>(), TH, NCI * 16, a, dw, st);
}

template <int NCI, int... NTS>
static int launch_wgrad_taps_dma_t(WgArgs& a, int nt, float* dw, hipStream_t st) {
  return dispatch<NTS...>(nt, [&](auto nt_c) {
    constexpr int NT = decltype(nt_c)::value;
    // 4 ring slots where two blocks still fit a CU's 160 KB, else 3
    constexpr int S4 = WtDma<NCI, NT, 4>::template lds<4>() <= 80 * 1024 ? 4 : 3;
    if (g_wgrad_dma_cfg == 1) return launch_wgrad_taps_dma_s<NCI, NT, 8, 3>(a, dw, st);
    if (g_wgrad_dma_cfg == 2) return launch_wgrad_taps_dma_s<NCI, NT, 4, 6>(a, dw, st);
    return launch_wgrad_taps_dma_s<NCI, NT, 4, S4>(a, dw, st);
  });
}

int launch_wgrad_taps_dma(WgArgs& a, float* dw, hipStream_t st) {
  const int nt = (9 * a.cout + 15) / 16;
  if (wgrad_dma_nci(a) == 4) return launch_wgrad_taps_dma_t<4, 1, 2, 3, 4, 5>(a, nt, dw, st);
  return launch_wgrad_taps_dma_t<2, 1, 2, 3, 4, 5, 6, 7, 8, 9>(a, nt, dw, st);
}

}  // namespace trn
}  // namespace vm

