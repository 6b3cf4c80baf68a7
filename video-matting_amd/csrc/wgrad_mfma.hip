// The MFMA conv weight gradient of the bf16 training path for cout <= 48 (wgrad.hip's launch_wgrad_mfma routes to it).

#include "wgrad_common.h"

namespace vm {
namespace trn {

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

template <int NCI, int NCO, bool SX, int TH, bool PIPE>
static int launch_wgrad_mfma_t(WgArgs& a, float* dw, hipStream_t st) {
  return launch_wgrad_grid_k<wgrad_mfma_kernel<NCI, NCO, SX, TH, PIPE>>(wgrad_mfma_lds<NCI, NCO, SX, TH>(), TH, NCI * 16, a, dw, st);
}

// the five operand tilings wgrad_mfma_cfg picks, on 4- or 8-row tiles, pipelined or (wgrad_mfma_pipe 0) the plain loop
int launch_wgrad_mfma_tiled(WgArgs& a, int nci, int nco, int th, float* dw, hipStream_t st) {
  return dispatch<8, 4>(th, [&](auto th_c) {
    return dispatch<0, 1>(g_wgrad_mfma_pipe != 0, [&](auto pipe_c) {
      constexpr int TH = decltype(th_c)::value;
      constexpr bool PIPE = decltype(pipe_c)::value != 0;
      if (nco == 1 && nci >= 2) return launch_wgrad_mfma_t<2, 1, false, TH, PIPE>(a, dw, st);
      if (nci == 1 && nco == 1) return launch_wgrad_mfma_t<1, 1, true, TH, PIPE>(a, dw, st);
      if (nci == 2 && nco == 2) return launch_wgrad_mfma_t<2, 2, true, TH, PIPE>(a, dw, st);
      if (nci == 1 && nco == 2) return launch_wgrad_mfma_t<1, 2, true, TH, PIPE>(a, dw, st);
      return launch_wgrad_mfma_t<1, 3, true, TH, PIPE>(a, dw, st);
    });
  });
}

}  // namespace trn
}  // namespace vm
