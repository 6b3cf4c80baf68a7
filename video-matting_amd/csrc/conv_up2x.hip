// The folded 2x resize + 3x3 conv (unet.py:44-63 upconv_concat): the phase-filter fold, the border pass that recomputes
// the frame's outer ring, and the vm_conv3x3_up2x* entry points (bf16, split-fp16 x3 and head-split forms), which run
// the folded conv itself on the patch kernel (conv_patch.hip).
#include "conv_dispatch.h"

namespace vm {

// ================================================================ folded 2x resize (unet.py:44-63 upconv_concat)
// conv3x3(resize2x(x)) with TF1 legacy bilinear (scale 0.5) is linear in x: resized row 2i = x[i], row 2i+1 =
// (x[i] + x[i+1]) / 2.  So output pixel (2i+a, 2j+b) is a 3x3 conv of the LOW-RES frame at (i, j) with a phase
// filter W'_ab[u][v] = sum_{kh,kw} R_a[u][kh] R_b[v][kw] W[kh][kw], u,v in {-1,0,+1}:
//   R_0 = [[.5,0,0],[.5,1,.5],[0,0,.5]]  (rows u, columns kh)      R_1 = [[0,0,0],[1,.5,0],[0,.5,1]]
// Output channel p*cout + co of the folded conv is phase p = 2a+b of channel co.  Exact in the interior and, with
// the low-res frame replicated past its bottom/right edge, at output rows/columns 2H-2; output row/column 0 and
// 2H-1 / 2W-1 see the resized image's zero padding instead and are recomputed by conv3x3_up2x_border.
__global__ void fold_up2x_weights(const float* w, int cin, int cout, float* wu) {
  const long total = 9L * cin * cout;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % cout);
    const long r = i / cout;
    const int ci = (int)(r % cin);
    const int tap = (int)(r / cin), u = tap / 3, v = tap % 3;  // low-res tap (u, v) = offset (u-1, v-1)
    constexpr float R[2][3][3] = {{{.5f, 0.f, 0.f}, {.5f, 1.f, .5f}, {0.f, 0.f, .5f}},
                                  {{0.f, 0.f, 0.f}, {1.f, .5f, 0.f}, {0.f, .5f, 1.f}}};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int pa = p >> 1, pb = p & 1;
      double s = 0.0;
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) {
          const float c = R[pa][u][kh] * R[pb][v][kw];
          if (c != 0.f) s += (double)c * (double)w[((long)(kh * 3 + kw) * cin + ci) * cout + co];
        }
      wu[((long)tap * cin + ci) * (4L * cout) + (long)p * cout + co] = (float)s;
    }
  }
}

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

// 8 fp16 values of a 16-byte chunk -> f32
__device__ __forceinline__ void unpack_f16x8(uint4 u, float* f) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xffffu));
    f[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
  }
}

// Border pixels of the folded upconv, computed the unfused way: the 9 resized taps (TF1 legacy bilinear in f32,
// rounded to bf16 as vm_resize_bilinear_tf1_nhwc stores them; zero outside the 2H x 2W frame) of 16 pixels are
// staged per 32-channel granule and consumed by MFMAs.  The pass is latency-bound (a few hundred blocks; each granule
// costs a round trip for its gathers), so a 1024-thread block splits the granules 4 ways (wave w: output channels
// 16 (w & 3) .. +15, granules (w >> 2), (w >> 2) + 4, ...: each 4-wave group stages and consumes its own granules,
// double-buffered, with one LDS-only barrier per step) and adds the 4 partial sums in a fixed order at the end.
__device__ __forceinline__ uint4 sel3(int i, uint4 a, uint4 b, uint4 c) { return i == 0 ? a : (i == 1 ? b : c); }

// SPL: the split-fp16 x3 form (the folded upconvs of vmatting/split3.py): each staged value is the resize of the f32
// activation x = h + l (exact in f32), split again into fp16 (h', l'); K granule cc stages l' (slab 0) or h' (slabs 1,
// 2) for the fp16 filter parts [Wh, Wl, Wh]; the output is written split (ConvArgs::ysplit's layout)
template <int BD_KS, bool SPL = false>  // granule split of the border pass (waves = 4 x BD_KS)
__global__ __launch_bounds__(256 * BD_KS) void conv3x3_up2x_border(BorderArgs a) {
  using T = uint16_t;
  using MT = std::conditional_t<SPL, f16_t, uint16_t>;
  __shared__ __attribute__((aligned(16))) char stg[BD_KS][2][9 * 16 * 64];  // [split][buffer][tap][pixel][32 ch]
  __shared__ __attribute__((aligned(16))) float red[BD_KS * 16 * 64];       // [split][pixel][channel] partial sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = wave & 3, ks = wave >> 2, gt = tid & 255;  // channel group, granule split, thread in the split group
  const int OH = 2 * a.H, OW = 2 * a.W;
  const long total = (long)a.nframes * a.nb, b0 = (long)blockIdx.x * 16;
  const int cob = blockIdx.y * 64;
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
  const int cx0 = max(ox - 1, 0) >> 1;
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
        const T* p = xr + ((long)yy * a.W + xx) * a.x_cstride + cin0;
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
  const int steps = (a.nch + BD_KS - 1) / BD_KS;  // every group runs the same number of steps (uniform barriers)
  uint4 g[SPL ? 12 : 6];
  gather(ks, g);
  for (int i = 0; i < steps; ++i) {
    const int cc = ks + i * BD_KS;
    char* buf = stg[ks][i & 1];
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
    float* vals = reinterpret_cast<float*>(&stg[0][0][0]);  // [16 pixels][64]
    float* hwl = vals + 16 * 64;                              // the head filter's 9 x 64 taps, bf16-rounded
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

}  // namespace vm

using namespace vm;

extern "C" int vm_conv3x3_fold_up2x_weights(const float* w_hwio, int cin, int cout, float* w_up_hwio, void* stream) {
  if (!w_hwio || !w_up_hwio || cin <= 0 || cout <= 0) return fail(VM_EINVAL, "fold_up2x: bad argument");
  hipLaunchKernelGGL(fold_up2x_weights, dim3(grid_for(9L * cin * cout, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), w_hwio, cin, cout, w_up_hwio);
  return check_launch("fold_up2x_weights");
}

// One call of a folded upconv (vm_conv3x3_up2x*), checked by its entry point: the arguments every form has, then the
// optional ones
struct UpCall {
  const vm_tensor* x;
  const void* packed_up;
  const void* packed;
  int cin, cout;
  const float* bias;
  const float* scale;
  const float* shift;
  int act;
  vm_tensor* y;
  void* stream;
  const float* head_w = nullptr;  // head split (ConvArgs::hd): conv1_5's HWIO f32 filter, ours at head_coff
  int head_cin = 0, head_coff = 0;
  float* partial = nullptr;       // ... its per-tap partials [pixel][12]; store_y = 0 leaves y unwritten
  int store_y = 1;
  int ysplit = 0;                 // > 0: the split-fp16 x3 form (x = [l, h] slabs, y split at this slab)
  int* overflow = nullptr;
};

// the folded conv on the patch kernel (interior and, replicated, the far edges), then the border pass
static int up2x_impl(const UpCall& c) {
  const vm_tensor *x = c.x, *y = c.y;
  const bool spl = c.ysplit > 0;
  const char* name = spl ? "conv3x3_up2x_split3" : "conv3x3_up2x";
  const PackGeom g = geom(c.cin, 4 * c.cout, x->dtype), g1 = geom(c.cin, c.cout, x->dtype);
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  ConvArgs a{};
  BorderArgs b{};
  a.x = b.x = x->ptr; a.x_cstride = b.x_cstride = x->cstride; a.x_coff = b.x_coff = x->coff;
  a.H = b.H = x->h; a.W = b.W = x->w; b.nframes = x->n;
  a.M = (long)x->n * x->h * x->w;
  fill_geom(a, g);
  a.w = c.packed_up; a.cout = 4 * c.cout;
  b.w = c.packed; b.K_pad = g1.K_pad; b.cout = c.cout; b.nch = g1.cin_pad / 32;
  a.bias = b.bias = c.bias; a.scale = b.scale = c.scale; a.shift = b.shift = c.shift; a.act = b.act = c.act;
  a.y = b.y = y->ptr; a.y_cstride = b.y_cstride = y->cstride; a.y_coff = b.y_coff = y->coff;
  a.y_dtype = spl ? VM_F32 : y->dtype;  // split: f32 staging, split stores (ConvArgs::ysplit)
  a.y_vec = 1;
  a.up = 1; a.up_cout = c.cout;
  a.hd = b.hd = c.partial; a.hw = b.hw = c.head_w; a.hw_cin = b.hw_cin = c.head_cin; a.hw_coff = b.hw_coff = c.head_coff;
  a.y_skip = b.y_skip = c.store_y ? 0 : 1;
  if (spl) {
    a.ysplit = b.ysplit = c.ysplit; a.ovf = b.ovf = c.overflow;
    a.f16 = 1; a.xalias = b.xs = x->c / 2; a.ksplit = 1;
  }
  if (!patch_ok(a, 2)) return fail(VM_EUNSUPPORTED, "%s: shape not supported by the patch kernel", name);
  const int rc = dispatch_patch(a, st);
  if (rc != VM_OK) return rc;
  const int OH = 2 * x->h, OW = 2 * x->w;
  b.nb = 2 * OW + 2 * (OH - 2);
  const long nblk = ((long)x->n * b.nb + 15) / 16;
  if (nblk > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "%s: too many border pixels", name);
  const dim3 grid((unsigned)nblk, c.cout / 64);
  if (spl) hipLaunchKernelGGL((conv3x3_up2x_border<4, true>), grid, dim3(1024), 0, st, b);
  else if (g_opt.border_ks == 4) hipLaunchKernelGGL(conv3x3_up2x_border<4>, grid, dim3(1024), 0, st, b);
  else if (g_opt.border_ks == 2) hipLaunchKernelGGL(conv3x3_up2x_border<2>, grid, dim3(512), 0, st, b);
  else hipLaunchKernelGGL(conv3x3_up2x_border<1>, grid, dim3(256), 0, st, b);
  return check_launch(spl ? "conv3x3_up2x_border(split)" : "conv3x3_up2x_border");
}

// the bf16 form's checks (vm_conv3x3_up2x_nhwc, and vm_conv3x3_up2x_head_nhwc after its own)
static int up2x_bf16(const UpCall& c) {
  const vm_tensor *x = c.x, *y = c.y;
  const int cin = c.cin, cout = c.cout;
  if (!valid_tensor(x) || !valid_tensor(y) || !c.packed_up || !c.packed)
    return fail(VM_EINVAL, "conv3x3_up2x: invalid tensor/weights");
  if (cin <= 0 || cout <= 0 || x->c != cin || y->c != cout)
    return fail(VM_EINVAL, "conv3x3_up2x: channel mismatch x.c=%d cin=%d y.c=%d cout=%d", x->c, cin, y->c, cout);
  if (y->n != x->n || y->h != 2 * x->h || y->w != 2 * x->w)
    return fail(VM_EINVAL, "conv3x3_up2x: output must be [%d,%d,%d,%d]", x->n, 2 * x->h, 2 * x->w, cout);
  if (c.act < VM_ACT_NONE || c.act > VM_ACT_SOFTMAX) return fail(VM_EINVAL, "conv3x3_up2x: act %d", c.act);
  const bool xvec = view16_ok(x) && x->coff + geom(cin, 4 * cout, x->dtype).cin_pad <= x->cstride;
  if (x->dtype != VM_BF16 || y->dtype != VM_BF16 || cout % 64 || !xvec || !view16_ok(y) || c.act == VM_ACT_SOFTMAX ||
      g_opt.conv_kernel == 1 || g_opt.conv_kernel == 2)
    return fail(VM_EUNSUPPORTED, "conv3x3_up2x: folded resize needs the bf16 patch kernel (cout %% 64 == 0, "
                                 "16-byte channel views)");
  return up2x_impl(c);
}

extern "C" int vm_conv3x3_up2x_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin, int cout,
                                    const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                                    void* stream) {
  return up2x_bf16({x, packed_up, packed, cin, cout, bias, scale, shift, act, y, stream});
}

extern "C" int vm_conv3x3_up2x_split3_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin,
                                           int cout, const float* bias, const float* scale, const float* shift, int act,
                                           vm_tensor* y, int y_slab, int* overflow, void* stream) {
  if (!valid_tensor(x, true) || !valid_tensor(y, true) || !packed_up || !packed)
    return fail(VM_EINVAL, "conv3x3_up2x_split3: invalid tensor/weights");
  const int S = x->c / 2;
  if (x->dtype != VM_F16 || y->dtype != VM_F16 || x->c % 64 || cin != 3 * S || y->c != cout)
    return fail(VM_EINVAL, "conv3x3_up2x_split3: fp16 views, x = [l, h] slabs of S %% 32 == 0 channels, cin = 3 S "
                           "(x.c=%d cin=%d y.c=%d cout=%d)", x->c, cin, y->c, cout);
  if (y->n != x->n || y->h != 2 * x->h || y->w != 2 * x->w)
    return fail(VM_EINVAL, "conv3x3_up2x_split3: output must be [%d,%d,%d,%d]", x->n, 2 * x->h, 2 * x->w, cout);
  if (act < VM_ACT_NONE || act >= VM_ACT_SOFTMAX) return fail(VM_EINVAL, "conv3x3_up2x_split3: act %d", act);
  const int ys = y_slab > 0 ? y_slab : y->cstride / 2;
  const bool xvec = view16_ok(x) && x->coff + x->c <= x->cstride;
  if (cout % 64 || !xvec || !split3_view_ok(y, ys, cout) || !g_opt.up_skip || g_opt.conv_kernel == 1 || g_opt.conv_kernel == 2)
    return fail(VM_EUNSUPPORTED, "conv3x3_up2x_split3: cout %% 64 == 0, 16-byte channel views, the split layout");
  UpCall c{x, packed_up, packed, cin, cout, bias, scale, shift, act, y, stream};
  c.ysplit = ys;
  c.overflow = overflow;
  return up2x_impl(c);
}

extern "C" int vm_conv3x3_up2x_head_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin,
                                         int cout, const float* bias, const float* scale, const float* shift, int act,
                                         vm_tensor* y, const float* head_w, int head_cin, int head_coff, float* partial,
                                         int store_y, void* stream) {
  if (!head_w || !partial || cout != 64 || head_cin <= 0 || head_coff < 0 || head_coff + cout > head_cin)
    return fail(VM_EINVAL, "conv3x3_up2x_head: head filter [3,3,%d,1] with the conv's %d channels at %d", head_cin, cout,
                head_coff);
  // the partials come from the patch kernel's register epilogue (64-channel row-slot tilings)
  if (!g_opt.patch_repi || g_opt.patch_cfg || g_opt.rows_up || !g_opt.up_skip)
    return fail(VM_EUNSUPPORTED, "conv3x3_up2x_head: needs the patch kernel's register epilogue");
  return up2x_bf16({x, packed_up, packed, cin, cout, bias, scale, shift, act, y, stream, head_w, head_cin, head_coff,
                    partial, store_y});
}
