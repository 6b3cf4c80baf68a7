// Conv weight gradients of the training steps (the backward pass around them: train.hip).
//
//   conv_wgrad      dW[kh,kw,ci,co] = sum_p x[p + (kh-1, kw-1), ci] * dy[p, co]: per block an LDS patch of
//                   (4+2) x (32+2) pixels x CC channels and the 4 x 32 dy tile; each thread owns one (kh, ci,
//                   4-channel co group) and slides the three kw taps along a pixel row (1 new LDS x read and one
//                   float4 dy read per 12 FMAs); blocks walk tiles persistently and store one partial filter
//                   gradient each, summed in fixed order by a second pass (deterministic, no atomics)

#include <initializer_list>

#include "train_common.h"

namespace vm {
namespace trn {

// ---------------------------------------------------------------- conv weight gradient
constexpr int WG_TH = 4, WG_TW = 32, WG_PH = WG_TH + 2, WG_PW = WG_TW + 2, WG_NT = 256;

// XV: x is T-typed with 16-byte aligned channel vectors (cin, coff, cstride multiples of the vector width), so a
// pixel's CC channels arrive as CC/VE 16-byte loads, all of a thread's loads issued before any LDS store.
// DV: likewise dy as float4 (cout % 4 == 0).  Otherwise element loads.
template <int CC, int CO4, typename T, bool XV, bool DV>
__global__ __launch_bounds__(WG_NT) void wgrad_kernel(V x, V dy, float* partials,
                                                      int tiles_h, int tiles_w, long ntiles) {
  constexpr int TASKS = 3 * CC * CO4;
  constexpr int TPT = (TASKS + WG_NT - 1) / WG_NT;
  constexpr int VE = 16 / sizeof(T), NVP = CC / VE, NV = WG_PH * WG_PW * NVP;
  constexpr int VPT = XV ? (NV + WG_NT - 1) / WG_NT : 1;
  constexpr int ND = WG_TH * WG_TW * CO4, DPT = DV ? (ND + WG_NT - 1) / WG_NT : 1;
  __shared__ float xs[WG_PH * WG_PW * CC];
  __shared__ float4 ds[WG_TH * WG_TW * CO4];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * CC;
  const int cin = x.c, cout = dy.c;
  // this block's partial filter gradient: row blockIdx.x of the [gridDim.x][3][3][cin][cout] workspace
  float* part = partials + (long)blockIdx.x * 9 * cin * cout;
  float acc[TPT][3][4];
#pragma unroll
  for (int k = 0; k < TPT; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[k][j][0] = acc[k][j][1] = acc[k][j][2] = acc[k][j][3] = 0.f;

  // vector paths: the next tile's 16-byte loads are issued into registers before the current tile's FMAs,
  // so their latency hides under the compute (register double buffer; LDS holds the current tile)
  uint4 xb[VPT];
  float4 db[DPT];
  auto coords = [&](long tile, int& n, int& y0, int& x0) {
    const int tx = (int)(tile % tiles_w);
    const long t2 = tile / tiles_w;
    y0 = (int)(t2 % tiles_h) * WG_TH;
    n = (int)(t2 / tiles_h);
    x0 = tx * WG_TW;
  };
  auto issue = [&](int tile) {
    int n, y0, x0;
    coords(tile, n, y0, x0);
    if constexpr (XV) {
#pragma unroll
      for (int k = 0; k < VPT; ++k) {
        const int e = tid + k * WG_NT;
        xb[k] = make_uint4(0, 0, 0, 0);
        if (NV % WG_NT == 0 || e < NV) {
          const int j = e % NVP, pc = e / NVP;
          const int gy = y0 + pc / WG_PW - 1, gx = x0 + pc % WG_PW - 1, c = c0 + j * VE;
          if (gy >= 0 && gy < x.h && gx >= 0 && gx < x.w && c < cin)
            xb[k] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(x.p) +
                                                    (((long)n * x.h + gy) * x.w + gx) * x.cs + x.coff + vchan(x, c));
        }
      }
    }
    if constexpr (DV) {
#pragma unroll
      for (int k = 0; k < DPT; ++k) {
        const int e = tid + k * WG_NT;
        db[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ND % WG_NT == 0 || e < ND) {
          const int cg = e % CO4, pp = e / CO4;
          const int gy = y0 + pp / WG_TW, gx = x0 + pp % WG_TW;
          if (gy < x.h && gx < x.w && cg * 4 < cout)
            db[k] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(dy.p) +
                                                     (((long)n * x.h + gy) * x.w + gx) * dy.cs + dy.coff + cg * 4);
        }
      }
    }
  };
  auto commit = [&](long tile) {
    int n, y0, x0;
    coords(tile, n, y0, x0);
    if constexpr (XV) {
#pragma unroll
      for (int k = 0; k < VPT; ++k) {
        const int e = tid + k * WG_NT;
        if (NV % WG_NT == 0 || e < NV) {
          float f[VE];
          Chunk<T>::unpack(xb[k], f);
          const int c = c0 + (e % NVP) * VE;  // a vector straddling cin (padded views): zero the lanes past it
#pragma unroll
          for (int i = 0; i < VE; ++i)
            if (c + i >= cin) f[i] = 0.f;
          float4* d = reinterpret_cast<float4*>(xs + (e / NVP) * CC + (e % NVP) * VE);
#pragma unroll
          for (int i = 0; i < VE / 4; ++i) d[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
        }
      }
    } else {
      for (int e = tid; e < WG_PH * WG_PW * CC; e += WG_NT) {
        const int ci = e % CC;
        const int pc = e / CC;
        const int gy = y0 + pc / WG_PW - 1, gx = x0 + pc % WG_PW - 1, c = c0 + ci;
        float v = 0.f;
        if (gy >= 0 && gy < x.h && gx >= 0 && gx < x.w && c < cin) v = ld(x, ((long)n * x.h + gy) * x.w + gx, c);
        xs[e] = v;
      }
    }
    if constexpr (DV) {
#pragma unroll
      for (int k = 0; k < DPT; ++k) {
        const int e = tid + k * WG_NT;
        if (ND % WG_NT == 0 || e < ND) ds[e] = db[k];
      }
    } else {
      float* dsf = reinterpret_cast<float*>(ds);
      for (int e = tid; e < WG_TH * WG_TW * CO4 * 4; e += WG_NT) {
        const int co = e % (CO4 * 4);
        const int pp = e / (CO4 * 4);
        const int gy = y0 + pp / WG_TW, gx = x0 + pp % WG_TW;
        float v = 0.f;
        if (gy < x.h && gx < x.w && co < cout) v = ld(dy, ((long)n * x.h + gy) * x.w + gx, co);
        dsf[e] = v;
      }
    }
  };

  if (blockIdx.x < ntiles) issue(blockIdx.x);
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    commit(tile);
    __syncthreads();
    if (tile + gridDim.x < ntiles) issue(tile + gridDim.x);
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
      const int t = tid + k * WG_NT;
      if (TASKS % WG_NT == 0 || t < TASKS) {
        const int ci = t % CC;
        const int cg = (t / CC) % CO4;
        const int kh = t / (CC * CO4);
        for (int py = 0; py < WG_TH; ++py) {
          const float* row = xs + ((py + kh) * WG_PW) * CC + ci;
          const float4* drow = ds + py * WG_TW * CO4 + cg;
          float xa = row[0], xb = row[CC];
#pragma unroll 8
          for (int px = 0; px < WG_TW; ++px) {
            const float xc = row[(px + 2) * CC];
            const float4 d = drow[px * CO4];
            acc[k][0][0] += xa * d.x; acc[k][0][1] += xa * d.y; acc[k][0][2] += xa * d.z; acc[k][0][3] += xa * d.w;
            acc[k][1][0] += xb * d.x; acc[k][1][1] += xb * d.y; acc[k][1][2] += xb * d.z; acc[k][1][3] += xb * d.w;
            acc[k][2][0] += xc * d.x; acc[k][2][1] += xc * d.y; acc[k][2][2] += xc * d.z; acc[k][2][3] += xc * d.w;
            xa = xb;
            xb = xc;
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const int t = tid + k * WG_NT;
    if (TASKS % WG_NT == 0 || t < TASKS) {
      const int ci = t % CC;
      const int cg = (t / CC) % CO4;
      const int kh = t / (CC * CO4);
      const int c = c0 + ci;
      if (c < cin) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int co = cg * 4 + j;
            if (co < cout) part[(((long)(kh * 3 + kw) * cin + c) * cout + co)] = acc[k][kw][j];
          }
      }
    }
  }
}

// ---------------------------------------------------------------- conv weight gradient on MFMA (bf16 operands)
// dW_t[ci][co] = sum_p X[p + off_t][ci] * DY[p][co] (t = kh*3 + kw, off_t = (kh-1, kw-1)) as 9 GEMMs whose K axis is
// the pixels: v_mfma_f32_16x16x32_bf16 with A = X^T (16 input channels x 32 pixels), B = DY (32 pixels x 16 output
// channels), f32 accumulation.  Both operands sit in LDS in their natural NHWC order ([pixel][channel] rows) and are
// read k-major with ds_read_b64_tr_b16, so no transpose pass exists anywhere.  One of the two operands carries the
// 1-pixel halo and is read at the 9 tap offsets; the other is read once per K-step and reused by the 9 taps:
//   SX  (shift x):  X patch (TH+2) x (TW+2) x CIB, DY tile TH x TW x COP        — wide cout (upconv*, conv*)
//   !SX (shift dy): X tile TH x TW x CIB, DY patch (TH+2) x (TW+2) x COP       — narrow cout (select*, output):
//                   dW_t = sum_q X[q] * DY[q - off_t], with DY zero outside the frame
// Block = 4 waves on one TH(4) x TW(32) pixel tile, wave w owns tile row w (one 32-pixel K-step); blocks walk tiles
// (split-K over gridDim.x, one partial per block, the fixed-order wgrad_reduce_kernel sums them: deterministic).
// DY arrives f32 and is rounded to bf16 when staged (the bf16 training path's precision: bf16 operands, f32 sums).
// The LDS images are swizzled so every transposed read (two 16-lane groups 8 rows apart per 32-lane half) is
// conflict-free for any row base (tap shifts move it by 0..2 rows/pixels).
constexpr int WM_TW = 32, WM_PW = WM_TW + 2;
// patch pixels of a TH x 32 tile with its halo, and the image rows allocated for them (a multiple of 16, so the row
// swizzle stays in range)
template <int TH>
constexpr int wm_ppix() { return (TH + 2) * WM_PW; }
template <int TH>
constexpr int wm_prows() { return (wm_ppix<TH>() + 15) / 16 * 16; }

struct WgArgs {
  const uint16_t* x;  // bf16 input view base (pixel 0, channel coff applied)
  int n, h, w, cin, xcs, x_src_c;  // x_src_c > 0: channel c lives in source c / x_src_c at + x_src_stride elements
  long x_src_stride;
  const float* dy;  // f32 output-gradient view base (coff applied)
  int cout, dcs;
  float* part;      // [gridDim.x][9][cin][cout]
  int tiles_h, tiles_w;
  long ntiles;
};

// byte offset of 32-byte piece c (16 bf16 channels) of image row r, rows of RB bytes (32, 64 or 128)
template <int RB>
__device__ __forceinline__ int wm_off(int r, int c) {
  if constexpr (RB == 32) return 32 * (r ^ (((r >> 3) & 1) << 2));
  else if constexpr (RB == 64) return 64 * r + 32 * (c ^ ((r >> 3) & 1));
  else return 128 * r + 32 * (c ^ ((r >> 1) & 1) ^ (((r >> 3) & 1) << 1));
}

typedef short v4s __attribute__((ext_vector_type(4)));

// the 16x16x32 operand fragment whose k rows are image rows rk(0..7) (8 consecutive pixels of one image row band),
// columns = 16-channel piece c: two transposed 4-row reads
template <int RB>
__device__ __forceinline__ bf16x8 wm_frag(const char* img, int r0, int c, int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3;
  typedef __attribute__((address_space(3))) v4s* lp;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + wm_off<RB>(r0 + q, c) + 8 * p));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + wm_off<RB>(r0 + 4 + q, c) + 8 * p));
  v4s v[2] = {lo, hi};
  return __builtin_bit_cast(bf16x8, v);
}

// PIPE (r05): every fragment address is computed once per kernel (the LDS images keep their layout from tile to
// tile) and the next tap's fragments are read while the current tap's MFMAs run (the plain loop let hipcc recompute
// the swizzled addresses and wait lgkmcnt(0) in front of every tap's MFMAs).  Same MFMAs per accumulator in the same
// order: bit-identical.
template <int NCI, int NCO, bool SX, int TH, bool PIPE = true>
__global__ __launch_bounds__(256, 2) void wgrad_mfma_kernel(WgArgs a) {
  constexpr int WM_TH = TH, WM_PPIX = wm_ppix<TH>(), WM_PROWS = wm_prows<TH>();
  constexpr int CIB = NCI * 16, COP = NCO * 16;
  constexpr int RBX = NCI == 1 ? 32 : NCI == 2 ? 64 : 128;
  constexpr int RBD = NCO == 1 ? 32 : NCO == 2 ? 64 : 128;
  constexpr int XROWS = SX ? WM_PROWS : WM_TH * WM_TW, DROWS = SX ? WM_TH * WM_TW : WM_PROWS;
  constexpr int XBYTES = XROWS * RBX, DBYTES = DROWS * RBD;
  constexpr int XPIX = SX ? WM_PPIX : WM_TH * WM_TW, DPIX = SX ? WM_TH * WM_TW : WM_PPIX;
  constexpr int XCH = CIB / 8, DCH = COP / 8;                    // 16-byte chunks per pixel row
  constexpr int NXC = XPIX * XCH, NDC = DPIX * DCH;
  constexpr int XPT = (NXC + 255) / 256, DPT = (NDC + 255) / 256;
  constexpr int RED = 9 * NCI * NCO * 4 * 64 * 4;                // one wave's accumulators in bytes
  constexpr int MAIN = XBYTES + DBYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  (void)RED;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.y * CIB;
  char* ximg = smem;
  char* dimg = smem + XBYTES;

  f32x4 acc[9][NCI][NCO];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < NCI; ++i)
#pragma unroll
      for (int o = 0; o < NCO; ++o) acc[t][i][o] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 xb[XPT];
  float4 db[DPT][2];
  auto coords = [&](int tile, int& n, int& y0, int& x0) {
    const int tx = tile % a.tiles_w;
    const int t2 = tile / a.tiles_w;
    y0 = (t2 % a.tiles_h) * WM_TH;
    n = t2 / a.tiles_h;
    x0 = tx * WM_TW;
  };
  // image pixel e of the patch (halo: origin (y0-1, x0-1), 34 wide) or the tile (origin (y0, x0), 32 wide)
  auto pix = [&](int e, bool halo, int y0, int x0, int& gy, int& gx) {
    if (halo) {
      gy = y0 - 1 + e / WM_PW;
      gx = x0 - 1 + e % WM_PW;
    } else {
      gy = y0 + e / WM_TW;
      gx = x0 + e % WM_TW;
    }
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
        int gy, gx;
        pix(pe, SX, y0, x0, gy, gx);
        const int c = c0 + j * 8;
        if ((unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w && c < a.cin) {
          long off = (((long)n * a.h + gy) * a.w + gx) * a.xcs;
          if (a.x_src_c > 0) off += (long)(c / a.x_src_c) * a.x_src_stride + c % a.x_src_c;
          else off += c;
          xb[k] = *reinterpret_cast<const uint4*>(a.x + off);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
      const int e = tid + k * 256;
      db[k][0] = db[k][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (NDC % 256 == 0 || e < NDC) {
        const int pe = e / DCH, j = e % DCH;
        int gy, gx;
        pix(pe, !SX, y0, x0, gy, gx);
        const int co = j * 8;
        if ((unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w && co < a.cout) {
          const float* src = a.dy + (((long)n * a.h + gy) * a.w + gx) * a.dcs + co;
          if (co + 8 <= a.cout && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            db[k][0] = *reinterpret_cast<const float4*>(src);
            db[k][1] = *reinterpret_cast<const float4*>(src + 4);
          } else {
            float f[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = co + i < a.cout ? src[i] : 0.f;
            db[k][0] = make_float4(f[0], f[1], f[2], f[3]);
            db[k][1] = make_float4(f[4], f[5], f[6], f[7]);
          }
        }
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
      if (NDC % 256 == 0 || e < NDC) {
        const int pe = e / DCH, j = e % DCH;
        const float f[8] = {db[k][0].x, db[k][0].y, db[k][0].z, db[k][0].w,
                            db[k][1].x, db[k][1].y, db[k][1].z, db[k][1].w};
        *reinterpret_cast<uint4*>(dimg + wm_off<RBD>(pe, j >> 1) + (j & 1) * 16) = Chunk<uint16_t>::pack(f);
      }
    }
  };

  const int g = lane >> 4;
  // a contiguous run of tiles per block: consecutive K-steps stay on neighbouring rows of the same pages (a
  // gridDim-strided walk jumps megabytes per step and pays TLB misses on every one)
  const int t_beg = (int)((long)blockIdx.x * a.ntiles / gridDim.x);
  const int t_end = (int)((long)(blockIdx.x + 1) * a.ntiles / gridDim.x);
  if constexpr (PIPE) {
    constexpr int RR = TH / 4, NTX = SX ? 9 : 1, NTD = SX ? 1 : 9;
    const int q = (lane >> 2) & 3, p = lane & 3;
    int xa[RR][NTX][NCI][2], da[RR][NTD][NCO][2];  // byte offsets of the lo / hi reads of every fragment
#pragma unroll
    for (int rr = 0; rr < RR; ++rr) {
      const int row = wave + 4 * rr;
#pragma unroll
      for (int tt = 0; tt < NTX; ++tt) {
        const int r0 = SX ? (row + tt / 3) * WM_PW + tt % 3 + 8 * g : row * WM_TW + 8 * g;
#pragma unroll
        for (int i = 0; i < NCI; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) xa[rr][tt][i][h] = wm_off<RBX>(r0 + 4 * h + q, i) + 8 * p;
      }
#pragma unroll
      for (int tt = 0; tt < NTD; ++tt) {
        const int r0 = SX ? row * WM_TW + 8 * g : (row + 2 - tt / 3) * WM_PW + 2 - tt % 3 + 8 * g;
#pragma unroll
        for (int o = 0; o < NCO; ++o)
#pragma unroll
          for (int h = 0; h < 2; ++h) da[rr][tt][o][h] = wm_off<RBD>(r0 + 4 * h + q, o) + 8 * p;
      }
    }
    auto frag = [&](const char* img, const int (&ad)[2]) __attribute__((always_inline)) {
      typedef __attribute__((address_space(3))) v4s* lp;
      const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + ad[0]));
      const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + ad[1]));
      v4s v[2] = {lo, hi};
      return __builtin_bit_cast(bf16x8, v);
    };
    constexpr int NP = SX ? NCI : NCO;  // fragments read per tap (the shifted operand)
    if (t_beg < t_end) issue(t_beg);
    for (int tile = t_beg; tile < t_end; ++tile) {
      commit();
      __syncthreads();
      if (tile + 1 < t_end) issue(tile + 1);
      // (a row's 9 taps carry only 9 x NCI x NCO MFMAs, too few to hide a read one tap ahead: all of the row's
      // fragments are read up front and the MFMAs wait for them in order)
      static_for<0, RR>([&](auto rc) __attribute__((always_inline)) {
        constexpr int rr = decltype(rc)::value;
        bf16x8 fix[SX ? NCO : NCI], sh[9][NP];  // the per-row operand, the per-tap one
#pragma unroll
        for (int k = 0; k < (SX ? NCO : NCI); ++k) fix[k] = SX ? frag(dimg, da[rr][0][k]) : frag(ximg, xa[rr][0][k]);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int k = 0; k < NP; ++k) sh[t][k] = SX ? frag(ximg, xa[rr][SX ? t : 0][k]) : frag(dimg, da[rr][SX ? 0 : t][k]);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int i = 0; i < NCI; ++i)
#pragma unroll
            for (int o = 0; o < NCO; ++o)
              acc[t][i][o] = SX ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(sh[t][i], fix[o], acc[t][i][o], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fix[i], sh[t][o], acc[t][i][o], 0, 0, 0);
        // (pinned: left alone, hipcc sinks each tap's reads to just before its MFMAs to keep 3 waves per SIMD)
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * ((SX ? NCO : NCI) + 9 * NP), 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 9 * NCI * NCO, 0);
      });
      __syncthreads();
    }
  } else {
  if (t_beg < t_end) issue(t_beg);
  for (int tile = t_beg; tile < t_end; ++tile) {
    commit();
    __syncthreads();
    if (tile + 1 < t_end) issue(tile + 1);
    // K-steps: the 32 pixels of tile rows wave, wave+4, ...; group g of a fragment holds pixels 8g..8g+7
#pragma unroll
    for (int rr = 0; rr < TH / 4; ++rr) {
      const int row = wave + 4 * rr;
      if constexpr (SX) {
        bf16x8 bd[NCO];
#pragma unroll
        for (int o = 0; o < NCO; ++o) bd[o] = wm_frag<RBD>(dimg, row * WM_TW + 8 * g, o, lane);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int r0 = (row + t / 3) * WM_PW + t % 3 + 8 * g;
#pragma unroll
          for (int i = 0; i < NCI; ++i) {
            const bf16x8 ax = wm_frag<RBX>(ximg, r0, i, lane);
#pragma unroll
            for (int o = 0; o < NCO; ++o)
              acc[t][i][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, bd[o], acc[t][i][o], 0, 0, 0);
          }
        }
      } else {
        bf16x8 ax[NCI];
#pragma unroll
        for (int i = 0; i < NCI; ++i) ax[i] = wm_frag<RBX>(ximg, row * WM_TW + 8 * g, i, lane);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          // DY[q - off_t]: patch coordinates (row + 2 - kh, col + 2 - kw)
          const int r0 = (row + 2 - t / 3) * WM_PW + 2 - t % 3 + 8 * g;
#pragma unroll
          for (int o = 0; o < NCO; ++o) {
            const bf16x8 bd = wm_frag<RBD>(dimg, r0, o, lane);
#pragma unroll
            for (int i = 0; i < NCI; ++i)
              acc[t][i][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[i], bd, acc[t][i][o], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  }

  // fold the 4 waves' accumulators (LDS, two rounds), wave 0 stores the block's partial
  float* red = reinterpret_cast<float*>(smem);
  constexpr int NA = 9 * NCI * NCO * 4;
  auto put = [&](int slot) {
    int k = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < NCI; ++i)
#pragma unroll
        for (int o = 0; o < NCO; ++o)
#pragma unroll
          for (int j = 0; j < 4; ++j, ++k) red[(slot * NA + k) * 64 + lane] = acc[t][i][o][j];
  };
  auto add = [&](int slot) {
    int k = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < NCI; ++i)
#pragma unroll
        for (int o = 0; o < NCO; ++o)
#pragma unroll
          for (int j = 0; j < 4; ++j, ++k) acc[t][i][o][j] += red[(slot * NA + k) * 64 + lane];
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) add(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave == 0) {
    add(0);
    float* part = a.part + (long)blockIdx.x * 9 * a.cin * a.cout;
    const int co_l = lane & 15, ci_l = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < NCI; ++i)
#pragma unroll
        for (int o = 0; o < NCO; ++o) {
          const int co = o * 16 + co_l;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ci = c0 + i * 16 + ci_l + j;
            if (ci < a.cin && co < a.cout) part[((long)t * a.cin + ci) * a.cout + co] = acc[t][i][o][j];
          }
        }
  }
  (void)MAIN;
}

template <int NCI, int NCO, bool SX, int TH>
constexpr int wgrad_mfma_lds() {
  constexpr int RBX = NCI == 1 ? 32 : NCI == 2 ? 64 : 128;
  constexpr int RBD = NCO == 1 ? 32 : NCO == 2 ? 64 : 128;
  constexpr int XROWS = SX ? wm_prows<TH>() : TH * WM_TW, DROWS = SX ? TH * WM_TW : wm_prows<TH>();
  constexpr int MAIN = XROWS * RBX + DROWS * RBD;
  constexpr int RED = 2 * 9 * NCI * NCO * 4 * 64 * 4;
  return MAIN > RED ? MAIN : RED;
}

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

// ---------------------------------------------------------------- wide conv weight gradient (UNetImage training)
// train.py's training_procedure (train.py:37-109) back-propagates through every conv of unet.UNetImage
// (unet.py:86-148): cin 6 ... 1024, cout 64 ... 512.  dW_t[ci][co] = sum_p X[p + off_t][ci] * DY[p][co] as 9 GEMMs
// with K = the pixels, v_mfma_f32_16x16x32_bf16 (A = X^T: 16 input channels x 32 pixels, B = DY: 32 pixels x 16
// output channels, f32 accumulation), both operands read k-major from their natural NHWC LDS images with
// ds_read_b64_tr_b16 (wm_frag), like wgrad_mfma_kernel.  The narrow kernel above runs every output channel in one
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
constexpr int WW_TARGET_BLOCKS = 512;  // ~2 resident blocks per CU: one round; the partials stay <= 75 MB

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

// dw[i] += sum over the gx block rows of the partials (fixed order: deterministic).  A block owns COLS columns;
// its 256 / COLS row groups stride the rows (independent loads in flight), then fold through LDS.  64 columns for
// wide filters; 16 for narrow ones (S = 9 cin cout under 32k: 64-column blocks left a few hundred blocks each
// walking hundreds of rows).  256-thread blocks: a 1024-thread form waited for whole free CUs behind the
// side-stream weight gradients.
template <int COLS>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* part, int rows, long S, float* dw) {
  constexpr int RG = 256 / COLS;
  __shared__ float sh[RG][COLS];
  const int col = threadIdx.x % COLS, rg = threadIdx.x / COLS;
  const long i = (long)blockIdx.x * COLS + col;
  float s = 0.f;
  if (i < S) {
#pragma unroll 8
    for (int b = rg; b < rows; b += RG) s += part[(long)b * S + i];
  }
  sh[rg][col] = s;
  __syncthreads();
  if (rg == 0 && i < S) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < RG; ++g) t += sh[g][col];
    dw[i] += t;
  }
}

// The same fixed-order sum, 4 columns per lane (16-byte loads) and 16 row groups per block (r06): the 64-column form
// kept one 256-byte run per row group in flight and read the partials at ~0.8 TB/s (UNetImage step: 18 reductions,
// 45 us each, profiles/r05_train_image_kernel_stats.csv).  Each column's rows are summed in the order b = rg, rg + 16,
// ... per group, then the 16 groups in order: deterministic (another order than wgrad_reduce_kernel's).
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(const float* __restrict__ part, int rows, long S,
                                                            float* __restrict__ dw) {
  constexpr int RG = 16, CQ = 256 / RG;
  __shared__ float4 sh[RG][CQ];
  const int cq = threadIdx.x % CQ, rg = threadIdx.x / CQ;
  const long i = ((long)blockIdx.x * CQ + cq) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < S) {
#pragma unroll 4
    for (int b = rg; b < rows; b += RG) {
      const float4 v = *reinterpret_cast<const float4*>(part + (long)b * S + i);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  sh[rg][cq] = s;
  __syncthreads();
  if (rg == 0 && i < S) {
    float4 t = sh[0][cq];
#pragma unroll
    for (int g = 1; g < RG; ++g) {
      const float4 v = sh[g][cq];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    float4 d = *reinterpret_cast<float4*>(dw + i);
    d.x += t.x; d.y += t.y; d.z += t.z; d.w += t.w;
    *reinterpret_cast<float4*>(dw + i) = d;
  }
}

static long g_wgrad_reduce4 = 1;  // vm_set_option "wgrad_reduce4": 0 = the r05 scalar-column reduction (A/B)

static void launch_wgrad_reduce(const float* part, int rows, long S, float* dw, hipStream_t st) {
  if (g_wgrad_reduce4 && S % 4 == 0 && reinterpret_cast<uintptr_t>(dw) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(part) % 16 == 0 && rows > 1) {
    hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3((unsigned)((S / 4 + 15) / 16)), dim3(256), 0, st, part, rows, S, dw);
    return;
  }
  if (S >= 64L * 512)
    hipLaunchKernelGGL(wgrad_reduce_kernel<64>, dim3((unsigned)((S + 63) / 64)), dim3(256), 0, st, part, rows, S, dw);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3((unsigned)((S + 15) / 16)), dim3(256), 0, st, part, rows, S, dw);
}

constexpr size_t WG_WS_CAP = 64ull << 20;  // workspace bytes

// pixel-tile blocks per channel chunk: ~1024 blocks in all (4 per CU), fewer when the partial rows would pass
// WG_WS_CAP
static long wgrad_rows(int n, int h, int w, int cin, int cout, int cc) {
  const long ntiles = (long)n * ((h + WG_TH - 1) / WG_TH) * ((w + WG_TW - 1) / WG_TW);
  const int ncc = (cin + cc - 1) / cc;
  long gx = (1024 + ncc - 1) / ncc;
  const long cap = (long)(WG_WS_CAP / (9ull * cin * cout * sizeof(float)));
  if (gx > cap) gx = cap;
  if (gx > ntiles) gx = ntiles;
  return gx < 1 ? 1 : gx;
}

static int wgrad_cc(int cout) { return (cout + 3) / 4 <= 2 ? 64 : 32; }

template <int CC, int CO4, typename T, bool XV, bool DV>
static void launch_wgrad_t(const V& xv, const V& dy, float* dw, float* ws, hipStream_t st) {
  const int tiles_h = (xv.h + WG_TH - 1) / WG_TH, tiles_w = (xv.w + WG_TW - 1) / WG_TW;
  const long ntiles = (long)xv.n * tiles_h * tiles_w;
  const int ncc = (xv.c + CC - 1) / CC;
  const long gx = wgrad_rows(xv.n, xv.h, xv.w, xv.c, dy.c, CC);
  hipLaunchKernelGGL((wgrad_kernel<CC, CO4, T, XV, DV>), dim3((unsigned)gx, ncc), dim3(WG_NT), 0, st, xv, dy, ws,
                     tiles_h, tiles_w, ntiles);
  const long S = 9L * xv.c * dy.c;
  launch_wgrad_reduce(ws, (int)gx, S, dw, st);
}

static bool vec_ok(const V& v, int ve) {
  return reinterpret_cast<uintptr_t>(v.p) % 16 == 0 && v.c % ve == 0 && v.coff % ve == 0 && v.cs % ve == 0;
}

// x may also be read in 16-byte vectors past its last channel when the row stride holds them (the padded
// concat / input buffers: up1n[..., :30] of a 32-wide row, in9[..., :9] of a 16-wide row); the extra lanes are zeroed
static bool xvec_ok(const V& v, int ve) {
  if (v.sc > 0)  // split sources: a vector never straddles two sources
    return reinterpret_cast<uintptr_t>(v.p) % 16 == 0 && v.coff % ve == 0 && v.cs % ve == 0 && v.sc % ve == 0 &&
           v.ss % ve == 0 && v.coff + v.sc <= v.cs;
  return reinterpret_cast<uintptr_t>(v.p) % 16 == 0 && v.coff % ve == 0 && v.cs % ve == 0 &&
         v.coff + (v.c + ve - 1) / ve * ve <= v.cs;
}

template <int CC, int CO4>
static void launch_wgrad(const V& xv, const V& dy, float* dw, float* ws, hipStream_t st) {
  const bool dv = vec_ok(dy, 4);
  if (xv.dt == VM_BF16 && xvec_ok(xv, 8)) {
    if (dv) launch_wgrad_t<CC, CO4, uint16_t, true, true>(xv, dy, dw, ws, st);
    else launch_wgrad_t<CC, CO4, uint16_t, true, false>(xv, dy, dw, ws, st);
  } else if (xv.dt == VM_F32 && xvec_ok(xv, 4)) {
    if (dv) launch_wgrad_t<CC, CO4, float, true, true>(xv, dy, dw, ws, st);
    else launch_wgrad_t<CC, CO4, float, true, false>(xv, dy, dw, ws, st);
  } else {
    if (dv) launch_wgrad_t<CC, CO4, float, false, true>(xv, dy, dw, ws, st);
    else launch_wgrad_t<CC, CO4, float, false, false>(xv, dy, dw, ws, st);
  }
}

// the exact f32 FMA kernel's tiling by output channels (cout <= 48)
static void launch_wgrad_fma(const V& xv, const V& dy, float* dw, float* ws, hipStream_t st) {
  switch ((dy.c + 3) / 4) {
    case 1: launch_wgrad<64, 1>(xv, dy, dw, ws, st); break;
    case 2: launch_wgrad<64, 2>(xv, dy, dw, ws, st); break;
    case 3:
    case 4: launch_wgrad<32, 4>(xv, dy, dw, ws, st); break;
    case 5:
    case 6: launch_wgrad<32, 6>(xv, dy, dw, ws, st); break;
    case 7:
    case 8: launch_wgrad<32, 8>(xv, dy, dw, ws, st); break;
    default: launch_wgrad<32, 12>(xv, dy, dw, ws, st); break;
  }
}

struct WmCfg {
  int nci, nco;
  bool sx;
  int nt;  // > 0: wgrad_taps_kernel with NT = nt column tiles (cout <= 8)
};

// blocks per channel chunk of the MFMA weight gradient: ~1024 in all, at most one per tile (tiles of the smallest
// variant, so the workspace query, which cannot know the variant, is an upper bound), capped by the workspace
static long wgrad_mfma_rows(const WgArgs& a, int cib) {
  const long rows = wgrad_rows(a.n, a.h, a.w, a.cin, a.cout, cib);
  return rows < a.ntiles ? rows : (a.ntiles < 1 ? 1 : a.ntiles);
}

// operand tiling of the MFMA weight gradient: cout -> NCO 16-wide fragments, the input-channel fragments per block
// as wide as 144 accumulator registers allow; the operand with fewer fragments per K-step carries the tap shift
// (at most 72-108 accumulator registers: the 144-register tilings spill next to the staging registers)
// cout <= 8: the taps-in-N kernel, 64 input channels per block (32 for NT 4-5: 80 accumulator registers at most)
static WmCfg wgrad_mfma_cfg(int cin, int cout) {
  WmCfg c;
  c.nco = cout <= 16 ? 1 : cout <= 32 ? 2 : 3;
  c.nci = (c.nco == 1 && cin > 16) ? 2 : 1;
  c.sx = c.nco >= c.nci;
  c.nt = cout <= 8 ? (9 * cout + 15) / 16 : 0;
  if (c.nt) c.nci = cin <= 16 ? 1 : cin <= 32 || c.nt > 3 ? 2 : 4;
  return c;
}

// Once per device: lets `kerns` take `lds` bytes of dynamic LDS.  attr_dev is the caller's cached device id (-1
// before the first call), set to the current device once every kernel's attribute is in place.
static int wgrad_lds_once(const char* what, std::initializer_list<const void*> kerns, int lds, int& attr_dev) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (attr_dev == dev) return VM_OK;
  for (const void* k : kerns) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return fail(VM_EHIP, "%s setup: %s", what, hipGetErrorString(e));
  }
  attr_dev = dev;
  return VM_OK;
}

// one round of blocks: the ~1024-block target (the workspace bound) cut to what is resident at once (160-VGPR
// variants: 3 blocks per CU), so no block waits for a second round (measured 2 x 72 us per select wgrad)
static int launch_wgrad_grid(const void* kern, int lds, int th, int cib, int& attr_dev, int& resident, WgArgs& a,
                             float* dw, hipStream_t st, void (*launch)(dim3, int, hipStream_t, const WgArgs&)) {
  int dev = attr_dev;  // the caller's cache follows only once the occupancy query has succeeded too
  if (int rc = wgrad_lds_once("wgrad_mfma", {kern}, lds, dev)) return rc;
  if (attr_dev != dev) {
    int per_cu = 0, n_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return fail(VM_EHIP, "wgrad_mfma setup: %s", hipGetErrorString(e));
    resident = per_cu * n_cu;
    attr_dev = dev;
  }
  a.tiles_h = (a.h + th - 1) / th;
  a.tiles_w = (a.w + WM_TW - 1) / WM_TW;
  a.ntiles = (long)a.n * a.tiles_h * a.tiles_w;
  if (a.ntiles > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv_wgrad: too many pixel tiles");
  const int ncc = (a.cin + cib - 1) / cib;
  long gx = wgrad_mfma_rows(a, cib);
  if (resident >= ncc && gx * ncc > resident) gx = resident / ncc;
  launch(dim3((unsigned)gx, ncc), lds, st, a);
  const long S = 9L * a.cin * a.cout;
  launch_wgrad_reduce(a.part, (int)gx, S, dw, st);
  return VM_OK;
}

static long g_wgrad_mfma_pipe = 1;  // vm_set_option "wgrad_mfma_pipe": 0 = wgrad_mfma_kernel's plain loop (A/B)
template <int NCI, int NCO, bool SX, int TH, bool PIPE>
static int launch_wgrad_mfma_p(WgArgs& a, float* dw, hipStream_t st) {
  static int attr_dev = -1, resident = 0;  // blocks of this variant resident on the whole chip at once
  return launch_wgrad_grid(reinterpret_cast<const void*>(&wgrad_mfma_kernel<NCI, NCO, SX, TH, PIPE>),
                           wgrad_mfma_lds<NCI, NCO, SX, TH>(), TH, NCI * 16, attr_dev, resident, a, dw, st,
                           [](dim3 g, int lds, hipStream_t s, const WgArgs& x) {
                             hipLaunchKernelGGL((wgrad_mfma_kernel<NCI, NCO, SX, TH, PIPE>), g, dim3(256), lds, s, x);
                           });
}
template <int NCI, int NCO, bool SX, int TH>
static int launch_wgrad_mfma_t(WgArgs& a, float* dw, hipStream_t st) {
  return g_wgrad_mfma_pipe ? launch_wgrad_mfma_p<NCI, NCO, SX, TH, true>(a, dw, st)
                           : launch_wgrad_mfma_p<NCI, NCO, SX, TH, false>(a, dw, st);
}

template <int NCI, int NT, int TH>
static int launch_wgrad_taps_t(WgArgs& a, float* dw, hipStream_t st) {
  static int attr_dev = -1, resident = 0;
  return launch_wgrad_grid(reinterpret_cast<const void*>(&wgrad_taps_kernel<NCI, NT, TH>),
                           wgrad_taps_lds<NCI, NT, TH>(), TH, NCI * 16, attr_dev, resident, a, dw, st,
                           [](dim3 g, int lds, hipStream_t s, const WgArgs& x) {
                             hipLaunchKernelGGL((wgrad_taps_kernel<NCI, NT, TH>), g, dim3(256), lds, s, x);
                           });
}

static long g_wgrad_variant = 0;  // A/B knob (vm_set_option "wgrad_variant"): 0/1 4-row tiles, 2 8-row tiles
static long g_wgrad_taps = 1;     // vm_set_option "wgrad_taps": 0 sends cout <= 8 to wgrad_mfma_kernel (A/B)
// vm_set_option "wgrad_dma": 1 = the LDS-DMA narrow kernel.  Off: measured at the config-5 select shapes with L2 /
// MALL flushed between calls (tools/selectwgrad_bench.py, MI355X) it streams x no faster than the register-staged
// kernels (select1 136 vs 128 us, 2.3-2.5 TB/s; select4 150 vs 42 us: its f32 DY patch outweighs the 40^2 X tile)
static long g_wgrad_dma = 0;

// the LDS-DMA narrow weight gradient: cout <= 16, 8-channel chunks, the block's channels inside one source, 32-bit
// byte offsets inside one image
static bool wgrad_dma_ok(const WgArgs& a, int cib) {
  return g_wgrad_dma && a.cout >= 1 && a.cout <= 16 && a.cin % 8 == 0 && a.xcs % 8 == 0 &&
         reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && (a.x_src_c <= 0 || (a.x_src_c % cib == 0 && a.x_src_stride % 8 == 0)) &&
         (long)a.h * a.w * a.xcs * 2 < 0x7ff00000L && (long)a.h * a.w * a.dcs * 4 < 0x7ff00000L;
}

static long g_wgrad_wide_pipe = 1;  // vm_set_option "wgrad_wide_pipe": 0 = the plain-loop kernel at 2 blocks per CU (A/B)
static long g_wgrad_wide_cs = 1;  // vm_set_option "wgrad_wide_cs": 0 = the input-channel wave split for cin <= 16 too
static long g_wgrad_wide_dbuf = 1;  // vm_set_option "wgrad_wide_dbuf": 0 = one LDS image buffer, two barriers per tile
static long g_wgrad_wide_target = 0;  // vm_set_option "wgrad_wide_target": > 0 overrides the K-split's block target

static long g_wgrad_dma_cfg = 0;  // vm_set_option "wgrad_dma_cfg" (A/B): 0 auto, 1 = 8-row tiles, 2 = 4 rows x 6 slots

template <int NCI, int NT, int TH, int S>
static int launch_wgrad_taps_dma_s(WgArgs& a, float* dw, hipStream_t st) {
  using C = WtDma<NCI, NT, TH>;
  static int attr_dev = -1, resident = 0;
  return launch_wgrad_grid(reinterpret_cast<const void*>(&wgrad_taps_dma_kernel<NCI, NT, TH, S>),
                           C::template lds<S>(), TH, C::CIB, attr_dev, resident, a, dw, st,
                           [](dim3 g, int lds, hipStream_t s, const WgArgs& x) {
                             hipLaunchKernelGGL((wgrad_taps_dma_kernel<NCI, NT, TH, S>), g, dim3(256), lds, s, x);
                           });
}

template <int NCI, int NT>
static int launch_wgrad_taps_dma_t(WgArgs& a, float* dw, hipStream_t st) {
  // 4 ring slots where two blocks still fit a CU's 160 KB, else 3
  constexpr int S4 = WtDma<NCI, NT, 4>::template lds<4>() <= 80 * 1024 ? 4 : 3;
  if (g_wgrad_dma_cfg == 1) return launch_wgrad_taps_dma_s<NCI, NT, 8, 3>(a, dw, st);
  if (g_wgrad_dma_cfg == 2) return launch_wgrad_taps_dma_s<NCI, NT, 4, 6>(a, dw, st);
  return launch_wgrad_taps_dma_s<NCI, NT, 4, S4>(a, dw, st);
}

static int launch_wgrad_taps_dma(WgArgs& a, float* dw, hipStream_t st) {
  const int nt = (9 * a.cout + 15) / 16;
  if (nt <= 5 && a.cin > 32) {
    switch (nt) {
      case 1: return launch_wgrad_taps_dma_t<4, 1>(a, dw, st);
      case 2: return launch_wgrad_taps_dma_t<4, 2>(a, dw, st);
      case 3: return launch_wgrad_taps_dma_t<4, 3>(a, dw, st);
      case 4: return launch_wgrad_taps_dma_t<4, 4>(a, dw, st);
      default: return launch_wgrad_taps_dma_t<4, 5>(a, dw, st);
    }
  }
  switch (nt) {
    case 1: return launch_wgrad_taps_dma_t<2, 1>(a, dw, st);
    case 2: return launch_wgrad_taps_dma_t<2, 2>(a, dw, st);
    case 3: return launch_wgrad_taps_dma_t<2, 3>(a, dw, st);
    case 4: return launch_wgrad_taps_dma_t<2, 4>(a, dw, st);
    case 5: return launch_wgrad_taps_dma_t<2, 5>(a, dw, st);
    case 6: return launch_wgrad_taps_dma_t<2, 6>(a, dw, st);
    case 7: return launch_wgrad_taps_dma_t<2, 7>(a, dw, st);
    case 8: return launch_wgrad_taps_dma_t<2, 8>(a, dw, st);
    default: return launch_wgrad_taps_dma_t<2, 9>(a, dw, st);
  }
}

static int launch_wgrad_mfma(WgArgs& a, float* dw, hipStream_t st) {
  WmCfg c = wgrad_mfma_cfg(a.cin, a.cout);
  const bool th8 = g_wgrad_variant == 2;
  if (wgrad_dma_ok(a, (9 * a.cout + 15) / 16 <= 5 && a.cin > 32 ? 64 : 32)) return launch_wgrad_taps_dma(a, dw, st);
  if (c.nt && g_wgrad_taps) {
#define VM_WT(NCI, NT) \
  return th8 ? launch_wgrad_taps_t<NCI, NT, 8>(a, dw, st) : launch_wgrad_taps_t<NCI, NT, 4>(a, dw, st)
    if (c.nci == 1) {
      switch (c.nt) { case 1: VM_WT(1, 1); case 2: VM_WT(1, 2); case 3: VM_WT(1, 3); case 4: VM_WT(1, 4); default: VM_WT(1, 5); }
    } else if (c.nci == 2) {
      switch (c.nt) { case 1: VM_WT(2, 1); case 2: VM_WT(2, 2); case 3: VM_WT(2, 3); case 4: VM_WT(2, 4); default: VM_WT(2, 5); }
    } else {
      switch (c.nt) { case 1: VM_WT(4, 1); case 2: VM_WT(4, 2); default: VM_WT(4, 3); }
    }
#undef VM_WT
  }
  if (c.nt) {  // the legacy tiling of this shape
    c.nt = 0;
    c.nci = a.cin > 16 ? 2 : 1;
  }
  if (c.nco == 1 && c.nci >= 2)
    return th8 ? launch_wgrad_mfma_t<2, 1, false, 8>(a, dw, st) : launch_wgrad_mfma_t<2, 1, false, 4>(a, dw, st);
  if (c.nci == 1 && c.nco == 1)
    return th8 ? launch_wgrad_mfma_t<1, 1, true, 8>(a, dw, st) : launch_wgrad_mfma_t<1, 1, true, 4>(a, dw, st);
  if (c.nci == 2 && c.nco == 2)
    return th8 ? launch_wgrad_mfma_t<2, 2, true, 8>(a, dw, st) : launch_wgrad_mfma_t<2, 2, true, 4>(a, dw, st);
  if (c.nci == 1 && c.nco == 2)
    return th8 ? launch_wgrad_mfma_t<1, 2, true, 8>(a, dw, st) : launch_wgrad_mfma_t<1, 2, true, 4>(a, dw, st);
  return th8 ? launch_wgrad_mfma_t<1, 3, true, 8>(a, dw, st) : launch_wgrad_mfma_t<1, 3, true, 4>(a, dw, st);
}

// K-split of the wide weight gradients: WW_TARGET_BLOCKS blocks in all (one resident round), at most one per pixel
// tile (bf16) / 32-pixel chunk (f32), and partials of at most WW_WS_CAP bytes
constexpr size_t WW_WS_CAP = 128ull << 20;

static long wgrad_wide_gx(int n, int h, int w, int cin, int cout, bool f32, long target = WW_TARGET_BLOCKS) {
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

static int launch_wgrad_wide(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, hipStream_t st) {
  WwArgs a{};
  a.x = reinterpret_cast<const uint16_t*>(x->ptr) + x->coff;
  a.n = x->n; a.h = x->h; a.w = x->w; a.cin = x->c; a.xcs = x->cstride;
  const bool f32 = dy->dtype == VM_F32;
  a.dy = f32 ? static_cast<const void*>(reinterpret_cast<const float*>(dy->ptr) + dy->coff)
             : static_cast<const void*>(reinterpret_cast<const uint16_t*>(dy->ptr) + dy->coff);
  a.cout = dy->c; a.dcs = dy->cstride;
  a.part = reinterpret_cast<float*>(work);
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
  const int lds = wgrad_wide_lds<WW_TH>() * (a.dbuf ? 2 : 1);
  constexpr int lds_max = 2 * wgrad_wide_lds<WW_TH>();
#define VM_WW(...) reinterpret_cast<const void*>(&wgrad_wide_kernel<__VA_ARGS__>)
  if (f32) {
    static int attr = -1;
    if (int rc = wgrad_lds_once("wgrad_wide", {VM_WW(WW_TH, true), VM_WW(WW_TH, true, false)}, lds_max, attr)) return rc;
    if (pipe) hipLaunchKernelGGL((wgrad_wide_kernel<WW_TH, true>), dim3((unsigned)nb), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((wgrad_wide_kernel<WW_TH, true, false>), dim3((unsigned)nb), dim3(256), lds, st, a);
  } else if (a.cin <= 16 && g_wgrad_wide_cs) {  // (the 6-channel conv1_1: output-channel wave split)
    static int attr = -1;
    constexpr int lds1 = wgrad_wide_lds<WW_TH>();
    if (int rc = wgrad_lds_once("wgrad_wide", {VM_WW(WW_TH, false, false, true)}, lds1, attr)) return rc;
    hipLaunchKernelGGL((wgrad_wide_kernel<WW_TH, false, false, true>), dim3((unsigned)nb), dim3(256), lds1, st, a);
  } else {
    static int attr = -1;
    if (int rc = wgrad_lds_once("wgrad_wide", {VM_WW(WW_TH, false), VM_WW(WW_TH, false, false)}, lds_max, attr)) return rc;
    if (pipe) hipLaunchKernelGGL((wgrad_wide_kernel<WW_TH, false>), dim3((unsigned)nb), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((wgrad_wide_kernel<WW_TH, false, false>), dim3((unsigned)nb), dim3(256), lds, st, a);
  }
#undef VM_WW
  launch_wgrad_reduce(a.part, a.gx, 9L * a.cin * a.cout, dw, st);
  return VM_OK;
}

static int launch_wgrad_wide_f32(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, hipStream_t st) {
  WfArgs a{};
  a.x = reinterpret_cast<const float*>(x->ptr) + x->coff;
  a.n = x->n; a.h = x->h; a.w = x->w; a.cin = x->c; a.xcs = x->cstride;
  a.dy = reinterpret_cast<const float*>(dy->ptr) + dy->coff;
  a.cout = dy->c; a.dcs = dy->cstride;
  a.part = reinterpret_cast<float*>(work);
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

// this file's vm_set_option keys (vm_common.h OptDef): every one takes any value
const OptDef wgrad_options[] = {
    {"wgrad_reduce4", &trn::g_wgrad_reduce4, OPT_ANY},
    {"wgrad_variant", &trn::g_wgrad_variant, OPT_ANY},
    {"wgrad_taps", &trn::g_wgrad_taps, OPT_ANY},
    {"wgrad_dma", &trn::g_wgrad_dma, OPT_ANY},
    {"wgrad_mfma_pipe", &trn::g_wgrad_mfma_pipe, OPT_ANY},
    {"wgrad_wide_pipe", &trn::g_wgrad_wide_pipe, OPT_ANY},
    {"wgrad_wide_target", &trn::g_wgrad_wide_target, OPT_ANY},  // (<= WW_TARGET_BLOCKS: the workspace query's bound)
    {"wgrad_wide_cs", &trn::g_wgrad_wide_cs, OPT_ANY},
    {"wgrad_wide_dbuf", &trn::g_wgrad_wide_dbuf, OPT_ANY},
    {"wgrad_dma_cfg", &trn::g_wgrad_dma_cfg, OPT_ANY},
    {nullptr},
};

}  // namespace vm

using namespace vm;
using namespace vm::trn;

extern "C" size_t vm_conv3x3_wgrad_workspace_bytes(int n, int h, int w, int cin, int cout) {
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return 0;
  return (size_t)wgrad_rows(n, h, w, cin, cout, wgrad_cc(cout)) * 9 * cin * cout * sizeof(float);
}

extern "C" int vm_conv3x3_wgrad_nhwc(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, void* stream) {
  if (!ok_view(x) || !ok_view(dy) || !dw || !work || dy->dtype != VM_F32 || dy->n != x->n || dy->h != x->h ||
      dy->w != x->w)
    return fail(VM_EINVAL, "conv3x3_wgrad: bad argument");
  if (dy->c > 48) return fail(VM_EUNSUPPORTED, "conv3x3_wgrad: cout %d > 48", dy->c);
  launch_wgrad_fma(mk(x), mk(dy), dw, reinterpret_cast<float*>(work), reinterpret_cast<hipStream_t>(stream));
  return check_launch("conv3x3_wgrad");
}

extern "C" size_t vm_conv3x3_wgrad_ex_workspace_bytes(int n, int h, int w, int cin, int cout, int mode) {
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return 0;
  if (cout > 48)  // the wide kernels (UNetImage training)
    return (size_t)wgrad_wide_gx(n, h, w, cin, cout, mode != 1) * 9 * cin * cout * sizeof(float);
  if (mode != 1) return (size_t)wgrad_rows(n, h, w, cin, cout, wgrad_cc(cout)) * 9 * cin * cout * sizeof(float);
  const WmCfg c = wgrad_mfma_cfg(cin, cout);
  long rows = wgrad_rows(n, h, w, cin, cout, c.nci * 16);
  if (cout <= 16) {  // the LDS-DMA narrow kernel may take 64-channel blocks (fewer of them, more rows each)
    const long r64 = wgrad_rows(n, h, w, cin, cout, 64);
    if (r64 > rows) rows = r64;
  }
  return (size_t)rows * 9 * cin * cout * sizeof(float);
}

extern "C" int vm_conv3x3_wgrad_ex_nhwc(const vm_tensor* x, int x_src_c, long x_src_stride, const vm_tensor* dy,
                                        float* dw, void* work, int mode, void* stream) {
  vm_tensor xs = x ? *x : vm_tensor{};
  if (x_src_c > 0) xs.c = x_src_c;  // the view of source 0 must be valid; the others follow at x_src_stride
  if (!x || !ok_view(&xs) || !ok_view(dy) || !dw || !work || (dy->dtype != VM_F32 && !(dy->dtype == VM_BF16 && dy->c > 48)) || dy->n != x->n || dy->h != x->h ||
      dy->w != x->w || x_src_c < 0 || (x_src_c > 0 && (x_src_stride <= 0 || x->c % x_src_c)) ||
      (mode != 0 && mode != 1))
    return fail(VM_EINVAL, "conv3x3_wgrad_ex: bad argument");
  if (dy->c > 48) {  // the wide weight gradients of UNetImage's convs (train.py:37-109)
    if (x_src_c > 0) return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: split sources need cout <= 48");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (mode == 0) {
      if (x->dtype != VM_F32 || dy->dtype != VM_F32)
        return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: the exact mode with cout > 48 needs f32 x and dy");
      int rc = launch_wgrad_wide_f32(x, dy, dw, work, st);
      return rc ? rc : check_launch("conv3x3_wgrad_ex");
    }
    const int dch = dy->dtype == VM_F32 ? 4 : 8;  // elements per 16 bytes
    if (x->dtype != VM_BF16 || reinterpret_cast<uintptr_t>(x->ptr) % 16 || x->coff % 8 || x->cstride % 8 ||
        x->coff + (x->c + 7) / 8 * 8 > x->cstride || dy->c % 64 || (dy->dtype != VM_F32 && dy->dtype != VM_BF16) ||
        reinterpret_cast<uintptr_t>(dy->ptr) % 16 || dy->coff % dch || dy->cstride % dch)
      return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: the wide MFMA mode needs a bf16 x of 16-byte channel chunks "
                                   "and a 16-byte aligned dy of a multiple of 64 channels");
    int rc = launch_wgrad_wide(x, dy, dw, work, st);
    return rc ? rc : check_launch("conv3x3_wgrad_ex");
  }
  if (mode == 0) {  // exact f32 FMA kernel, optionally over split sources
    V xv = mk(x), dv = mk(dy);
    xv.sc = x_src_c;
    xv.ss = x_src_stride;
    launch_wgrad_fma(xv, dv, dw, reinterpret_cast<float*>(work), reinterpret_cast<hipStream_t>(stream));
    return check_launch("conv3x3_wgrad_ex");
  }
  if (x->dtype != VM_BF16 || reinterpret_cast<uintptr_t>(x->ptr) % 16 || x->coff % 8 || x->cstride % 8 ||
      (x_src_c > 0 ? (x_src_c % 8 || x->c % x_src_c || x->coff + x_src_c > x->cstride || x_src_stride % 8)
                   : x->coff + (x->c + 7) / 8 * 8 > x->cstride))
    return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: the MFMA mode needs a bf16 x of 16-byte channel chunks");
  WgArgs a{};
  a.x = reinterpret_cast<const uint16_t*>(x->ptr) + x->coff;
  a.n = x->n; a.h = x->h; a.w = x->w; a.cin = x->c; a.xcs = x->cstride;
  a.x_src_c = x_src_c; a.x_src_stride = x_src_stride;
  a.dy = reinterpret_cast<const float*>(dy->ptr) + dy->coff;
  a.cout = dy->c; a.dcs = dy->cstride;
  a.part = reinterpret_cast<float*>(work);
  int rc = launch_wgrad_mfma(a, dw, reinterpret_cast<hipStream_t>(stream));
  if (rc) return rc;
  return check_launch("conv3x3_wgrad_ex");
}
