// The wide conv weight gradients (cout > 48, UNetImage training): the bf16 MFMA kernel and the exact f32 FMA kernel.

#include "wgrad_common.h"

namespace vm {
namespace trn {

// ---------------------------------------------------------------- wide conv weight gradient (UNetImage training)
// train.py's training_procedure (train.py:37-109) back-propagates through every conv of unet.UNetImage
// (unet.py:86-148): cin 6 ... 1024, cout 64 ... 512.  dW_t[ci][co] = sum_p X[p + off_t][ci] * DY[p][co] as 9 GEMMs
// with K = the pixels, v_mfma_f32_16x16x32_bf16 (A = X^T: 16 input channels x 32 pixels, B = DY: 32 pixels x 16
// output channels, f32 accumulation), both operands read k-major from their natural NHWC LDS images with
// ds_read_b64_tr_b16 (wm_frag), like wgrad_mfma_kernel.  That narrow kernel runs every output channel in one
// block and splits its K-steps over the waves (cout <= 48); here a block owns a 64 x 64 (ci x co) tile of all 9
// taps and the 4 waves split the OUTPUT: wave w holds ci 16w..16w+15 x all 64 co x 9 taps (144 f32 accumulators)
// and walks every pixel row of the tile, so no cross-wave reduction is needed.  Per 32-pixel row a wave reads 4 DY
// fragments (reused by the 9 taps) and 9 X fragments (each reused by the 4 co pieces): 13 fragment reads per 36
// MFMAs, i.e. ~370 B of LDS reads per MFMA — inside the CU's LDS bandwidth at the matrix pipes' rate (a 32 x 32
// split read 20 fragments per 36 MFMAs, ~570 B, above it).
// Grid: gx K-split blocks (contiguous tile ranges, one partial filter gradient each, summed in fixed order by
// wgrad_reduce_kernel: deterministic) x the 64-channel blocks of cin and cout, as ONE dimension whose order is
// XCD-aware: the blocks that share a pixel range (every channel block of it) are dispatched to the same XCD, so
// its X patch and DY tile are fetched from HBM once per XCD and re-read from that XCD's L2.
// DY is bf16 (the bf16 gradient copy the relu / BN backward writes for the data-gradient conv) or f32 (rounded
// to bf16 when staged); X is the bf16 conv input, channels past cin (UNetImage's 6-channel conv1_1) read as 0.
struct WwArgs {
  const uint16_t* x;  // bf16 input view base (pixel 0, coff applied)
  int n, h, w, cin, xcs;
  const void* dy;     // bf16 / f32 output-gradient view base (coff applied)
  int cout, dcs;
  float* part;        // [gx][9][cin][cout]
  int tiles_h, tiles_w;
  long ntiles;
  int gx, ncin, ncout;
  int dbuf;           // PIPE: two LDS image buffers, tile t in buffer t & 1 (one barrier per tile)
};

constexpr int WW_TH = 4;

// Pipelined fragment reads (PIPE, r05).  The plain loop below left hipcc a per-tap chain of ~12 VALU for the
// swizzled row address, two ds_read_b64_tr_b16 and an lgkmcnt(0) wait in front of every 4 MFMAs, so each tap paid
// the whole LDS latency.  The row loop is unrolled and every fragment address is a per-lane base register plus an
// immediate: wm_off<128>(C + u, c) = 128 C + [128 u + 32 (c ^ x((C + u) mod 16))] for the lane's u = 8g + q, so 16
// bases per X piece (C mod 16) and 2 per DY piece cover every (row, tap); the next tap's X fragment (and, over the
// last two taps of a row, the next row's DY fragments and first X fragment) is read while the current tap's MFMAs
// run.  Each accumulator sees the same MFMAs in the same order: bit-identical to the plain loop.
template <int RB>
__device__ __forceinline__ int wm_base(int u, int c, int p) {  // wm_off<RB>(u, c) + 8p, RB = 128
  static_assert(RB == 128, "the 128-byte image rows of wgrad_wide_kernel");
  return 128 * u + 32 * (c ^ ((u >> 1) & 1) ^ (((u >> 3) & 1) << 1)) + 8 * p;
}

template <int C>  // fragment whose k rows are image rows C + u (lo) and C + 4 + u (hi), bases per C mod 16
__device__ __forceinline__ bf16x8 wm_frag_b(const char* img, const int (&b)[16]) {
  typedef __attribute__((address_space(3))) v4s* lp;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + 128 * C + b[C & 15]));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + 128 * (C + 4) + b[(C + 4) & 15]));
  v4s v[2] = {lo, hi};
  return __builtin_bit_cast(bf16x8, v);
}

// PIPE: one block per CU (the unrolled rows, the bases and the next tile's staging registers need > 256 VGPRs)
// CS (cin <= 16, plain loop): the 4 waves split the OUTPUT channels instead — wave w takes ci 0..15 x co 16w..16w+15
// x 9 taps — so UNetImage's 6-channel conv1_1 does not leave 3 of 4 waves multiplying zero input channels.  Each
// accumulator (ci piece 0, co piece w) sees the same MFMAs on the same fragments in the same order as wave 0's
// accumulator o = w in the default split: bit-identical.
template <int TH, bool DYF32, bool PIPE = true, bool CS = false>
__global__ __launch_bounds__(256, PIPE ? 1 : 2) void wgrad_wide_kernel(WwArgs a) {  // A/B (scripts/build_variant.sh):
                                                                           // (256,2) 2.58 ms vs (256,1) 2.87 ms
  constexpr int XPIX = wm_ppix<TH>(), DPIX = TH * WM_TW;
  constexpr int XBYTES = wm_prows<TH>() * 128;
  constexpr int NXC = XPIX * 8, NDC = DPIX * 8;                 // 16-byte chunks (8 channels) of each image
  constexpr int XPT = (NXC + 255) / 256, DPT = (NDC + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ximg = smem;
  char* dimg = smem + XBYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // = the 16-channel piece of ci this wave owns
  const int nb = gridDim.x, lin = blockIdx.x;
  // consecutive work ids on one XCD (workgroups are dealt to the 8 XCDs round-robin)
  const int wid = (nb % 8 == 0) ? (lin % 8) * (nb / 8) + lin / 8 : lin;
  const int nch = a.ncin * a.ncout;
  const int kx = wid / nch, cb = wid - kx * nch;
  const int c0 = (cb % a.ncin) * 64, o0 = (cb / a.ncin) * 64;

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[t][o] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 xb[XPT];
  uint4 db[DPT];
  float4 df[DYF32 ? DPT : 1][2];
  auto issue = [&](int tile) {
    const int tx = tile % a.tiles_w;
    const int t2 = tile / a.tiles_w;
    const int y0 = (t2 % a.tiles_h) * TH, n = t2 / a.tiles_h, x0 = tx * WM_TW;
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int e = tid + k * 256;
      xb[k] = make_uint4(0, 0, 0, 0);
      if (NXC % 256 == 0 || e < NXC) {
        const int pe = e >> 3, j = e & 7;
        const int gy = y0 - 1 + pe / WM_PW, gx = x0 - 1 + pe % WM_PW;
        const int c = c0 + j * 8;
        if ((unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w && c < a.cin)
          xb[k] = *reinterpret_cast<const uint4*>(a.x + (((long)n * a.h + gy) * a.w + gx) * a.xcs + c);
      }
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
      const int e = tid + k * 256;
      const int pe = e >> 3, j = e & 7;
      const int gy = y0 + pe / WM_TW, gx = x0 + pe % WM_TW;
      const bool in = (NDC % 256 == 0 || e < NDC) && (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
      const long off = (((long)n * a.h + gy) * a.w + gx) * a.dcs + o0 + j * 8;
      if constexpr (DYF32) {
        df[k][0] = df[k][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) {
          const float* src = reinterpret_cast<const float*>(a.dy) + off;
          df[k][0] = *reinterpret_cast<const float4*>(src);
          df[k][1] = *reinterpret_cast<const float4*>(src + 4);
        }
      } else {
        db[k] = make_uint4(0, 0, 0, 0);
        if (in) db[k] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(a.dy) + off);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
      const int e = tid + k * 256;
      if (NXC % 256 == 0 || e < NXC) {
        const int pe = e >> 3, j = e & 7;
        uint4 v = xb[k];
        const int c = c0 + j * 8;
        if (c + 8 > a.cin) {  // a chunk straddling cin: zero the channels past it
          uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (c + 2 * i >= a.cin) w4[i] = 0u;
            else if (c + 2 * i + 1 >= a.cin) w4[i] &= 0xffffu;
          }
          v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
        *reinterpret_cast<uint4*>(ximg + wm_off<128>(pe, j >> 1) + (j & 1) * 16) = v;
      }
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
      const int e = tid + k * 256;
      if (NDC % 256 == 0 || e < NDC) {
        const int pe = e >> 3, j = e & 7;
        uint4 v;
        if constexpr (DYF32) {
          const float f[8] = {df[k][0].x, df[k][0].y, df[k][0].z, df[k][0].w,
                              df[k][1].x, df[k][1].y, df[k][1].z, df[k][1].w};
          v = Chunk<uint16_t>::pack(f);
        } else {
          v = db[k];
        }
        *reinterpret_cast<uint4*>(dimg + wm_off<128>(pe, j >> 1) + (j & 1) * 16) = v;
      }
    }
  };

  const int g = lane >> 4;
  const int t_beg = (int)((long)kx * a.ntiles / a.gx);
  const int t_end = (int)((long)(kx + 1) * a.ntiles / a.gx);
  if constexpr (PIPE) {
    // per-lane fragment bases: X piece `wave` for every C mod 16, DY piece o for C mod 16 in {0, 4} (C = 32 row)
    const int u = 8 * g + ((lane >> 2) & 3), p = lane & 3;
    int bx[16], bdy[4][16];
#pragma unroll
    for (int k = 0; k < 16; ++k) bx[k] = wm_base<128>(k + u, wave, p) - 128 * k;
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int k = 0; k < 16; ++k) bdy[o][k] = (k == 0 || k == 4) ? wm_base<128>(k + u, o, p) - 128 * k : 0;
    // dbuf: tile t's images go to buffer t & 1.  Buffer (t + 1) & 1 was last read by tile t - 1's MFMAs, which every
    // wave finished before the barrier after tile t's commit, so the trailing barrier is not needed: a wave that is
    // done with tile t commits tile t + 1 while the others still compute.
    const int bstride = a.dbuf ? XBYTES + DPIX * 128 : 0;
    if (t_beg < t_end) issue(t_beg);
    for (int tile = t_beg; tile < t_end; ++tile) {
      ximg = smem + ((tile - t_beg) & 1) * bstride;
      dimg = ximg + XBYTES;
      commit();
      __syncthreads();
      if (tile + 1 < t_end) issue(tile + 1);
      bf16x8 bd[2][4], ax[2];
#pragma unroll
      for (int o = 0; o < 4; ++o) bd[0][o] = wm_frag_b<0>(dimg, bdy[o]);
      ax[0] = wm_frag_b<0>(ximg, bx);
      static_for<0, TH>([&](auto rc) __attribute__((always_inline)) {
        constexpr int row = decltype(rc)::value, cb = row & 1;
        static_for<0, 9>([&](auto tc) __attribute__((always_inline)) {
          constexpr int t = decltype(tc)::value;
          constexpr int gi = row * 9 + t;  // X fragments alternate between two slots over the tile's rows x taps
          if constexpr (t + 1 < 9) {
            constexpr int C = (row + (t + 1) / 3) * WM_PW + (t + 1) % 3;
            ax[(gi + 1) & 1] = wm_frag_b<C>(ximg, bx);
          } else if constexpr (row + 1 < TH) {
            constexpr int C = (row + 1) * WM_PW;  // the next row's tap 0
            ax[(gi + 1) & 1] = wm_frag_b<C>(ximg, bx);
          }
          if constexpr (t == 7 && row + 1 < TH) {
#pragma unroll
            for (int o = 0; o < 4; ++o) bd[cb ^ 1][o] = wm_frag_b<(row + 1) * WM_TW>(dimg, bdy[o]);
          }
#pragma unroll
          for (int o = 0; o < 4; ++o)
            acc[t][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[gi & 1], bd[cb][o], acc[t][o], 0, 0, 0);
          // the reads issued above go out ahead of this tap's MFMAs
          if constexpr (t == 7 && row + 1 < TH) __builtin_amdgcn_sched_group_barrier(0x100, 10, 0);
          else if constexpr (t + 1 < 9 || row + 1 < TH) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        });
      });
      if (!a.dbuf) __syncthreads();
    }
  } else {
  if (t_beg < t_end) issue(t_beg);
  for (int tile = t_beg; tile < t_end; ++tile) {
    commit();
    __syncthreads();
    if (tile + 1 < t_end) issue(tile + 1);
#pragma unroll 1
    for (int row = 0; row < TH; ++row) {
      if constexpr (CS) {
        const bf16x8 bdw = wm_frag<128>(dimg, row * WM_TW + 8 * g, wave, lane);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int r0 = (row + t / 3) * WM_PW + t % 3 + 8 * g;
          const bf16x8 ax = wm_frag<128>(ximg, r0, 0, lane);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, bdw, acc[t][0], 0, 0, 0);
        }
        continue;
      }
      bf16x8 bd[4];
#pragma unroll
      for (int o = 0; o < 4; ++o) bd[o] = wm_frag<128>(dimg, row * WM_TW + 8 * g, o, lane);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int r0 = (row + t / 3) * WM_PW + t % 3 + 8 * g;
        const bf16x8 ax = wm_frag<128>(ximg, r0, wave, lane);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[t][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, bd[o], acc[t][o], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  }

  // this block's partial of its 64 x 64 x 9 tile (lanes: co = lane & 15, ci = 4 * (lane >> 4) + j)
  float* part = a.part + (long)kx * 9 * a.cin * a.cout;
  const int co_l = lane & 15, ci_l = 4 * g;
  if constexpr (CS) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int co = o0 + 16 * wave + co_l;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ci = c0 + ci_l + j;
        if (ci < a.cin) part[((long)t * a.cin + ci) * a.cout + co] = acc[t][0][j];
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int co = o0 + 16 * o + co_l;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ci = c0 + 16 * wave + ci_l + j;
        if (ci < a.cin) part[((long)t * a.cin + ci) * a.cout + co] = acc[t][o][j];
      }
    }
}

template <int TH>
constexpr int wgrad_wide_lds() { return wm_prows<TH>() * 128 + TH * WM_TW * 128; }

// The exact-f32 wide weight gradient of the fp32 (parity) training path: a plain FMA GEMM per tap.  Block = 256
// threads on one (tap, 32 input channels, 64 output channels) tile; per 32-pixel K chunk the shifted X rows and
// the DY rows are staged in LDS, each thread accumulates 2 ci x 4 co in f32 over its block's contiguous pixel
// range (fixed order), and wgrad_reduce_kernel sums the gx partials in fixed order: deterministic.
struct WfArgs {
  const float* x;
  int n, h, w, cin, xcs;
  const float* dy;
  int cout, dcs;
  float* part;  // [gx][9][cin][cout]
  long npix;
  int gx, ncin, ncout;
};

__global__ __launch_bounds__(256) void wgrad_wide_f32_kernel(WfArgs a) {
  __shared__ float xs[32][33];
  __shared__ float ds[32][65];
  const int tid = threadIdx.x;
  int b = blockIdx.y;
  const int t = b % 9;
  b /= 9;
  const int c0 = (b % a.ncin) * 32, o0 = (b / a.ncin) * 64;
  const int kh = t / 3 - 1, kw = t % 3 - 1;
  const int kx = blockIdx.x;
  const long p_beg = kx * a.npix / a.gx, p_end = (kx + 1) * a.npix / a.gx;
  const int tc = tid / 16, to = tid % 16;  // thread: ci 2tc, 2tc+1; co 4to .. 4to+3
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (long p0 = p_beg; p0 < p_end; p0 += 32) {
    // stage X[p + off_t][c0 .. c0+31] and DY[p][o0 .. o0+63] for 32 pixels
    for (int e = tid; e < 32 * 32; e += 256) {
      const int pk = e / 32, c = e % 32;
      const long p = p0 + pk;
      float v = 0.f;
      if (p < p_end && c0 + c < a.cin) {
        const int xx = (int)(p % a.w);
        const long r = p / a.w;
        const int yy = (int)(r % a.h), nn = (int)(r / a.h);
        const int gy = yy + kh, gx = xx + kw;
        if ((unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w)
          v = a.x[(((long)nn * a.h + gy) * a.w + gx) * a.xcs + c0 + c];
      }
      xs[pk][c] = v;
    }
    for (int e = tid; e < 32 * 64; e += 256) {
      const int pk = e / 64, c = e % 64;
      const long p = p0 + pk;
      ds[pk][c] = (p < p_end && o0 + c < a.cout) ? a.dy[p * a.dcs + o0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const float x0 = xs[k][2 * tc], x1 = xs[k][2 * tc + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = ds[k][4 * to + j];
        acc[0][j] = fmaf(x0, d, acc[0][j]);
        acc[1][j] = fmaf(x1, d, acc[1][j]);
      }
    }
    __syncthreads();
  }
  float* part = a.part + (long)kx * 9 * a.cin * a.cout;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ci = c0 + 2 * tc + i;
    if (ci >= a.cin) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = o0 + 4 * to + j;
      if (co < a.cout) part[((long)t * a.cin + ci) * a.cout + co] = acc[i][j];
    }
  }
}

// K-split of the wide weight gradients: WW_TARGET_BLOCKS blocks in all (one resident round), at most one per pixel
// tile (bf16) / 32-pixel chunk (f32), and partials of at most WW_WS_CAP bytes
constexpr size_t WW_WS_CAP = 128ull << 20;

long wgrad_wide_gx(int n, int h, int w, int cin, int cout, bool f32, long target) {
  long units, nch;
  if (f32) {
    units = ((long)n * h * w + 31) / 32;
    nch = 9L * ((cin + 31) / 32) * ((cout + 63) / 64);
  } else {
    units = (long)n * ((h + WW_TH - 1) / WW_TH) * ((w + WM_TW - 1) / WM_TW);
    nch = (long)((cin + 63) / 64) * (cout / 64);
  }
  long gx = (target + nch - 1) / nch;
  const long cap = (long)(WW_WS_CAP / (9ull * cin * cout * sizeof(float)));
  if (gx > cap) gx = cap;
  if (gx > units) gx = units;
  return gx < 1 ? 1 : gx;
}

// the pipelined kernel or its plain-loop form (CS has no other) on nb blocks; the pair may take two LDS image buffers
template <bool DYF32, bool CS>
static int launch_wgrad_wide_k(bool pipe, long nb, int lds, const WwArgs& a, hipStream_t st) {
  constexpr auto KP = wgrad_wide_kernel<WW_TH, DYF32, !CS, CS>, K = wgrad_wide_kernel<WW_TH, DYF32, false, CS>;
  static int attr = -1;
  const std::initializer_list<const void*> pair = {reinterpret_cast<const void*>(KP), reinterpret_cast<const void*>(K)};
  if (int rc = wgrad_lds_once("wgrad_wide", pair, wgrad_wide_lds<WW_TH>() * (CS ? 1 : 2), attr)) return rc;
  if (pipe && !CS) hipLaunchKernelGGL(KP, dim3((unsigned)nb), dim3(256), lds, st, a);
  else hipLaunchKernelGGL(K, dim3((unsigned)nb), dim3(256), lds, st, a);
  return VM_OK;
}

int launch_wgrad_wide(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, hipStream_t st) {
  WwArgs a = wgrad_args<WwArgs>(x, dy, work);
  a.tiles_h = (a.h + WW_TH - 1) / WW_TH;
  a.tiles_w = (a.w + WM_TW - 1) / WM_TW;
  a.ntiles = (long)a.n * a.tiles_h * a.tiles_w;
  if (a.ntiles > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv_wgrad: too many pixel tiles");
  a.ncin = (a.cin + 63) / 64;
  a.ncout = a.cout / 64;
  // the pipelined kernel runs one block per CU: one resident round of WW_TARGET_BLOCKS / 2 blocks (half the partials)
  const bool pipe = g_wgrad_wide_pipe != 0;
  long target = pipe ? WW_TARGET_BLOCKS / 2 : WW_TARGET_BLOCKS;
  if (g_wgrad_wide_target > 0 && g_wgrad_wide_target <= WW_TARGET_BLOCKS) target = g_wgrad_wide_target;
  a.gx = (int)wgrad_wide_gx(a.n, a.h, a.w, a.cin, a.cout, false, target);
  const long nb = (long)a.gx * a.ncin * a.ncout;
  if (nb > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv_wgrad: grid too large");
  a.dbuf = pipe && g_wgrad_wide_dbuf ? 1 : 0;
  constexpr int lds1 = wgrad_wide_lds<WW_TH>();
  const int lds = lds1 * (a.dbuf ? 2 : 1);
  int rc;
  if (dy->dtype == VM_F32) rc = launch_wgrad_wide_k<true, false>(pipe, nb, lds, a, st);
  else if (a.cin <= 16 && g_wgrad_wide_cs) rc = launch_wgrad_wide_k<false, true>(pipe, nb, lds1, a, st);  // (conv1_1)
  else rc = launch_wgrad_wide_k<false, false>(pipe, nb, lds, a, st);
  if (rc) return rc;
  launch_wgrad_reduce(a.part, a.gx, 9L * a.cin * a.cout, dw, st);
  return VM_OK;
}

int launch_wgrad_wide_f32(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, hipStream_t st) {
  WfArgs a = wgrad_args<WfArgs>(x, dy, work);
  a.npix = (long)a.n * a.h * a.w;
  a.ncin = (a.cin + 31) / 32;
  a.ncout = (a.cout + 63) / 64;
  a.gx = (int)wgrad_wide_gx(a.n, a.h, a.w, a.cin, a.cout, true);
  const long ny = 9L * a.ncin * a.ncout;
  if (ny > 65535) return fail(VM_EUNSUPPORTED, "conv_wgrad: too many channel blocks");
  hipLaunchKernelGGL(wgrad_wide_f32_kernel, dim3((unsigned)a.gx, (unsigned)ny), dim3(256), 0, st, a);
  launch_wgrad_reduce(a.part, a.gx, 9L * a.cin * a.cout, dw, st);
  return VM_OK;
}

}  // namespace trn
}  // namespace vm

