// Conv weight gradients of the training steps (the backward pass around them: train.hip).
//
//   conv_wgrad      dW[kh,kw,ci,co] = sum_p x[p + (kh-1, kw-1), ci] * dy[p, co]: per block an LDS patch of
//                   (4+2) x (32+2) pixels x CC channels and the 4 x 32 dy tile; each thread owns one (kh, ci,
//                   4-channel co group) and slides the three kw taps along a pixel row (1 new LDS x read and one
//                   float4 dy read per 12 FMAs); blocks walk tiles persistently and store one partial filter
//                   gradient each, summed in fixed order by a second pass (deterministic, no atomics)
//
// Here too: the K-split reductions, routing, options and entry points of wgrad_mfma.hip, wgrad_taps.hip, wgrad_wide.hip.

#include "wgrad_common.h"

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

void launch_wgrad_reduce(const float* part, int rows, long S, float* dw, hipStream_t st) {
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
long wgrad_rows(int n, int h, int w, int cin, int cout, int cc) {
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
  dispatch<1, 0>(vec_ok(dy, 4), [&](auto dv_c) {
    constexpr bool DV = decltype(dv_c)::value != 0;
    if (xv.dt == VM_BF16 && xvec_ok(xv, 8)) launch_wgrad_t<CC, CO4, uint16_t, true, DV>(xv, dy, dw, ws, st);
    else if (xv.dt == VM_F32 && xvec_ok(xv, 4)) launch_wgrad_t<CC, CO4, float, true, DV>(xv, dy, dw, ws, st);
    else launch_wgrad_t<CC, CO4, float, false, DV>(xv, dy, dw, ws, st);
    return 0;
  });
}

// the exact f32 FMA kernel's tiling by output channels (cout <= 48): 1, 2 or the next even count of float4 groups
static void launch_wgrad_fma(const V& xv, const V& dy, float* dw, float* ws, hipStream_t st) {
  const int co4 = (dy.c + 3) / 4;
  if (co4 <= 2) dispatch<1, 2>(co4, [&](auto c) { return launch_wgrad<64, decltype(c)::value>(xv, dy, dw, ws, st), 0; });
  else dispatch<4, 6, 8, 12>((co4 + 1) / 2 * 2, [&](auto c) { return launch_wgrad<32, decltype(c)::value>(xv, dy, dw, ws, st), 0; });
}

struct WmCfg {
  int nci, nco;
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
  c.nt = cout <= 8 ? (9 * cout + 15) / 16 : 0;
  if (c.nt) c.nci = cin <= 16 ? 1 : cin <= 32 || c.nt > 3 ? 2 : 4;
  return c;
}

// Once per device: lets `kerns` take `lds` bytes of dynamic LDS.  attr_dev is the caller's cached device id (-1
// before the first call), set to the current device once every kernel's attribute is in place.
int wgrad_lds_once(const char* what, std::initializer_list<const void*> kerns, int lds, int& attr_dev) {
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
int launch_wgrad_grid(const void* kern, int lds, int th, int cib, int& attr_dev, int& resident, WgArgs& a, float* dw,
                      hipStream_t st, void (*launch)(dim3, int, hipStream_t, const WgArgs&)) {
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

static long g_wgrad_variant = 0;  // A/B knob (vm_set_option "wgrad_variant"): 0/1 4-row tiles, 2 8-row tiles
static long g_wgrad_taps = 1;     // vm_set_option "wgrad_taps": 0 sends cout <= 8 to wgrad_mfma_kernel (A/B)
// vm_set_option "wgrad_dma": 1 = the LDS-DMA narrow kernel.  Off: measured at the config-5 select shapes with L2 /
// MALL flushed between calls (tools/selectwgrad_bench.py, MI355X) it streams x no faster than the register-staged
// kernels (select1 136 vs 128 us, 2.3-2.5 TB/s; select4 150 vs 42 us: its f32 DY patch outweighs the 40^2 X tile)
long g_wgrad_dma = 0;
long g_wgrad_dma_cfg = 0;  // vm_set_option "wgrad_dma_cfg" (A/B): 0 auto, 1 = 8-row tiles, 2 = 4 rows x 6 slots
long g_wgrad_mfma_pipe = 1;  // vm_set_option "wgrad_mfma_pipe": 0 = wgrad_mfma_kernel's plain loop (A/B)
long g_wgrad_wide_pipe = 1;  // vm_set_option "wgrad_wide_pipe": 0 = the plain-loop kernel at 2 blocks per CU (A/B)
long g_wgrad_wide_cs = 1;  // vm_set_option "wgrad_wide_cs": 0 = the input-channel wave split for cin <= 16 too
long g_wgrad_wide_dbuf = 1;  // vm_set_option "wgrad_wide_dbuf": 0 = one LDS image buffer, two barriers per tile
long g_wgrad_wide_target = 0;  // vm_set_option "wgrad_wide_target": > 0 overrides the K-split's block target

static int launch_wgrad_mfma(WgArgs& a, float* dw, hipStream_t st) {
  WmCfg c = wgrad_mfma_cfg(a.cin, a.cout);
  const int th = g_wgrad_variant == 2 ? 8 : 4;
  if (wgrad_dma_ok(a)) return launch_wgrad_taps_dma(a, dw, st);
  if (c.nt && g_wgrad_taps) return launch_wgrad_taps(a, c.nci, c.nt, th, dw, st);
  if (c.nt) c.nci = a.cin > 16 ? 2 : 1;  // the legacy tiling of this shape
  return launch_wgrad_mfma_tiled(a, c.nci, c.nco, th, dw, st);
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

static size_t ws_bytes(long rows, int cin, int cout) { return (size_t)rows * 9 * cin * cout * sizeof(float); }

// a bf16 x whose pixels are whole 16-byte chunks of 8 channels, the last chunk of the c channels inside the row
static bool x_chunks_ok(const vm_tensor* x, int c) {
  return x->dtype == VM_BF16 && view16_ok(x, 8) && x->coff + (c + 7) / 8 * 8 <= x->cstride;
}

extern "C" size_t vm_conv3x3_wgrad_workspace_bytes(int n, int h, int w, int cin, int cout) {
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return 0;
  return ws_bytes(wgrad_rows(n, h, w, cin, cout, wgrad_cc(cout)), cin, cout);
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
  if (cout > 48) return ws_bytes(wgrad_wide_gx(n, h, w, cin, cout, mode != 1), cin, cout);  // (UNetImage training)
  if (mode != 1) return vm_conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout);
  // wgrad_rows grows with the channel block: the widest one routed to, 64 where the LDS-DMA kernel may run (cout <= 16)
  return ws_bytes(wgrad_rows(n, h, w, cin, cout, cout <= 16 ? 64 : wgrad_mfma_cfg(cin, cout).nci * 16), cin, cout);
}

extern "C" int vm_conv3x3_wgrad_ex_nhwc(const vm_tensor* x, int x_src_c, long x_src_stride, const vm_tensor* dy,
                                        float* dw, void* work, int mode, void* stream) {
  vm_tensor xs = x ? *x : vm_tensor{};
  if (x_src_c > 0) xs.c = x_src_c;  // the view of source 0 must be valid; the others follow at x_src_stride
  if (!x || !ok_view(&xs) || !ok_view(dy) || !dw || !work || (dy->dtype != VM_F32 && !(dy->dtype == VM_BF16 && dy->c > 48)) || dy->n != x->n || dy->h != x->h ||
      dy->w != x->w || x_src_c < 0 || (x_src_c > 0 && (x_src_stride <= 0 || x->c % x_src_c)) ||
      (mode != 0 && mode != 1))
    return fail(VM_EINVAL, "conv3x3_wgrad_ex: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = VM_OK;
  if (dy->c > 48) {  // the wide weight gradients of UNetImage's convs (train.py:37-109)
    if (x_src_c > 0) return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: split sources need cout <= 48");
    if (mode == 0) {
      if (x->dtype != VM_F32 || dy->dtype != VM_F32)
        return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: the exact mode with cout > 48 needs f32 x and dy");
      rc = launch_wgrad_wide_f32(x, dy, dw, work, st);
    } else {
      if (!x_chunks_ok(x, x->c) || dy->c % 64 || !view16_ok(dy))
        return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: the wide MFMA mode needs a bf16 x of 16-byte channel chunks "
                                     "and a 16-byte aligned dy of a multiple of 64 channels");
      rc = launch_wgrad_wide(x, dy, dw, work, st);
    }
  } else if (mode == 0) {  // exact f32 FMA kernel, optionally over split sources
    V xv = mk(x), dv = mk(dy);
    xv.sc = x_src_c;
    xv.ss = x_src_stride;
    launch_wgrad_fma(xv, dv, dw, reinterpret_cast<float*>(work), st);
  } else {
    if (!x_chunks_ok(x, x_src_c > 0 ? x_src_c : x->c) || (x_src_c > 0 && (x_src_c % 8 || x_src_stride % 8)))
      return fail(VM_EUNSUPPORTED, "conv3x3_wgrad_ex: the MFMA mode needs a bf16 x of 16-byte channel chunks");
    WgArgs a = wgrad_args<WgArgs>(x, dy, work);
    a.x_src_c = x_src_c; a.x_src_stride = x_src_stride;
    rc = launch_wgrad_mfma(a, dw, st);
  }
  return rc ? rc : check_launch("conv3x3_wgrad_ex");
}

