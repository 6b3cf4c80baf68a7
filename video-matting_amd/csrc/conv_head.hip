// The cout == 1 head (conv1_5 + sigmoid, unet.py:203-205): a 3x3 conv to one channel, from the activations
// (conv3x3_head / _strip / _mfma, routed by dispatch_head) or from per-tap partials made where the two halves of its
// input were (head_from_partials).
#include <type_traits>

#include "conv_dispatch.h"

namespace vm {

// ================================================================ Cout == 1 head (conv1_5 + sigmoid)
// unet.py:203-205 / unet_simple.py:142 / small.py:49-50: a 1-channel 3x3 conv over <=128 channels at full
// resolution is a memory-bound dot product: 16 lanes per pixel, each lane one 16-byte channel chunk per
// tap (a wave reads 4 pixels x 256 contiguous bytes), a 4-step xor-shuffle reduction inside each 16-lane
// group, weights un-permuted once per block into tap-major order in LDS.
struct HeadArgs {
  const void* x;
  int x_cstride, x_coff, H, W;
  long M;
  int cin_pad, K9, K_pad, chunk_major, ng;
  const void* w;
  const float* bias;
  const float* scale;
  const float* shift;
  int act;
  void* y;
  int y_cstride, y_coff, y_dtype;
  float* y2;  // optional: sigmoid of the pre-activation value, f32 [M] (unet.py:204-205 output beside conv1_3)
  const float* part;  // optional: per-tap partials [M][12] of the channels x does not carry (the pair kernel's hd)
  const float* yacc;  // optional: f32 [M] added to the pre-activation (a head over channel chunks, split-bf16 x6)
};

template <typename T>
__global__ __launch_bounds__(256) void conv3x3_head(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CE = 16 / sizeof(T);
  constexpr int GE = 64 / sizeof(T);
  float* sw = reinterpret_cast<float*>(smem);
  const T* Wt = reinterpret_cast<const T*>(a.w);
  for (int k = threadIdx.x; k < a.K_pad; k += 256) {
    int tap, c;
    if (a.chunk_major) {
      const int g = k / GE;
      if (g >= a.ng) continue;
      const int cc = g / 9;
      tap = g - cc * 9;
      c = cc * GE + (k - g * GE);
    } else {
      if (k >= a.K9) continue;
      tap = k / a.cin_pad;
      c = k - tap * a.cin_pad;
    }
    sw[tap * a.cin_pad + c] = ld_elem<T>(Wt + k);
  }
  __syncthreads();

  const int sub = threadIdx.x & 15;
  const int slot = threadIdx.x >> 4;
  const T* X = reinterpret_cast<const T*>(a.x) + a.x_coff;
  const long HW = (long)a.H * a.W;
  const float bias = a.bias ? a.bias[0] : 0.f;
  const float sc = a.scale ? a.scale[0] : 1.f;
  const float sh = a.shift ? a.shift[0] : 0.f;
  for (long p = (long)blockIdx.x * 16 + slot; p < a.M; p += (long)gridDim.x * 16) {
    const long rem = p % HW;
    const int h = (int)(rem / a.W);
    const int w = (int)(rem - (long)h * a.W);
    float acc = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int dh = tap / 3 - 1, dw = tap % 3 - 1;
      const int hh = h + dh, ww = w + dw;
      if ((unsigned)hh >= (unsigned)a.H || (unsigned)ww >= (unsigned)a.W) continue;
      const T* px = X + (p + (long)dh * a.W + dw) * a.x_cstride;
      const float* wt = sw + tap * a.cin_pad;
      for (int c = sub * CE; c < a.cin_pad; c += 16 * CE) {
        float f[CE];
        Chunk<T>::unpack(*reinterpret_cast<const uint4*>(px + c), f);
#pragma unroll
        for (int j = 0; j < CE; ++j) acc = fmaf(f[j], wt[c + j], acc);
      }
    }
    acc += __shfl_xor(acc, 8, 16);
    acc += __shfl_xor(acc, 4, 16);
    acc += __shfl_xor(acc, 2, 16);
    acc += __shfl_xor(acc, 1, 16);
    if (sub == 0) {
      float v = (acc + bias) * sc + sh;
      if (a.y2) a.y2[p] = sigmoid_precise(v);
      if (a.act == VM_ACT_RELU) v = v > 0.f ? v : 0.f;
      else if (a.act == VM_ACT_SIGMOID) v = sigmoid_precise(v);
      else if (a.act == VM_ACT_SOFTMAX) v = 1.f;  // softmax over a single channel
      const long o = p * (long)a.y_cstride + a.y_coff;
      if (a.y_dtype == VM_BF16) reinterpret_cast<uint16_t*>(a.y)[o] = f2bf(v);
      else reinterpret_cast<float*>(a.y)[o] = v;
    }
  }
}

// Strip variant for cin_pad == 16 * CE * NCH (conv1_5: 128 channels).  A 16-lane group owns NCH 16-byte channel
// chunks of P consecutive output pixels of one row: it loads the 3 x (P+2) input pixels once (all loads of a
// row in flight together), keeps its 9-tap weight slice in registers and reduces the P sums across the group.
// bf16 uses v_dot2_f32_bf16 on the packed pairs (f32 accumulation, no unpack); f32 uses fma.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

template <typename T, int NCH>
__device__ __forceinline__ float chunk_dot(const uint4 (&x)[NCH], const uint4 (&w)[NCH], float acc) {
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const uint32_t xs[4] = {x[q].x, x[q].y, x[q].z, x[q].w};
    const uint32_t ws[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (sizeof(T) == 2)
        acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, xs[j]), __builtin_bit_cast(bf16x2_t, ws[j]),
                                              acc, false);
      else
        acc = fmaf(__uint_as_float(xs[j]), __uint_as_float(ws[j]), acc);
    }
  }
  return acc;
}

template <typename T, int NCH, int P>
__global__ __launch_bounds__(256) void conv3x3_head_strip(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CE = 16 / sizeof(T);
  constexpr int GE = 64 / sizeof(T);
  T* sw = reinterpret_cast<T*>(smem);  // [9][cin_pad] tap-major, compute dtype
  const T* Wt = reinterpret_cast<const T*>(a.w);
  for (int k = threadIdx.x; k < a.K_pad; k += 256) {
    int tap, c;
    if (a.chunk_major) {
      const int g = k / GE;
      if (g >= a.ng) continue;
      const int cc = g / 9;
      tap = g - cc * 9;
      c = cc * GE + (k - g * GE);
    } else {
      if (k >= a.K9) continue;
      tap = k / a.cin_pad;
      c = k - tap * a.cin_pad;
    }
    sw[tap * a.cin_pad + c] = Wt[k];
  }
  __syncthreads();

  const int sub = threadIdx.x & 15;
  const int grp = threadIdx.x >> 4;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  uint4 wr[9][NCH];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int q = 0; q < NCH; ++q)
      wr[t][q] = *reinterpret_cast<const uint4*>(sw + t * a.cin_pad + (q * 16 + sub) * CE);

  const T* X = reinterpret_cast<const T*>(a.x) + a.x_coff;
  const float bias = a.bias ? a.bias[0] : 0.f;
  const float sc = a.scale ? a.scale[0] : 1.f;
  const float sh = a.shift ? a.shift[0] : 0.f;
  const int spr = (W + P - 1) / P;
  const long rows = a.M / W;
  const long nstrips = rows * spr;
  const int rowb = W * cs * (int)sizeof(T);
  for (long s0 = (long)blockIdx.x * 16; s0 < nstrips; s0 += (long)gridDim.x * 16) {
    // buffer descriptor rebased on the row above the block's first strip (wave-uniform); halo and
    // out-of-image taps get an out-of-range offset and read as zero (SAME padding)
    const long row0 = s0 / spr - 1;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(X + row0 * (long)W * cs), 0, 0x7ffffff0, 0x00020000);
    const long s = s0 + grp;
    if (s >= nstrips) break;
    const long row = s / spr;
    const int w0 = (int)(s - row * spr) * P;
    const int h = (int)(row % H);
    const int rel = (int)(row - row0);
    float acc[P];
#pragma unroll
    for (int o = 0; o < P; ++o) acc[o] = 0.f;
#pragma unroll
    for (int dh = -1; dh <= 1; ++dh) {
      const bool rok = (unsigned)(h + dh) < (unsigned)H;
      const int rbase = (rel + dh) * rowb + sub * CE * (int)sizeof(T);
      uint4 v[P + 2][NCH];
#pragma unroll
      for (int i = 0; i < P + 2; ++i) {
        const int ww = w0 - 1 + i;
        const bool ok = rok && (unsigned)ww < (unsigned)W;
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
          const int off = ok ? rbase + ww * cs * (int)sizeof(T) + q * 16 * CE * (int)sizeof(T) : OOB;
          v[i][q] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the row's loads in flight together (the scheduler serialises them)
#pragma unroll
      for (int i = 0; i < P + 2; ++i)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
          const int o = i - dw;
          if (o >= 0 && o < P) acc[o] = chunk_dot<T, NCH>(v[i], wr[(dh + 1) * 3 + dw], acc[o]);
        }
    }
    float mine = 0.f;
#pragma unroll
    for (int o = 0; o < P; ++o) {
      float r = acc[o];
      r += __shfl_xor(r, 8, 16);
      r += __shfl_xor(r, 4, 16);
      r += __shfl_xor(r, 2, 16);
      r += __shfl_xor(r, 1, 16);
      if (sub == o) mine = r;
    }
    if (sub < P && w0 + sub < W) {
      float v = (mine + bias) * sc + sh;
      if (a.y2) a.y2[row * W + w0 + sub] = sigmoid_precise(v);
      if (a.act == VM_ACT_RELU) v = v > 0.f ? v : 0.f;
      else if (a.act == VM_ACT_SIGMOID) v = sigmoid_precise(v);
      else if (a.act == VM_ACT_SOFTMAX) v = 1.f;
      const long o = (row * W + w0 + sub) * (long)a.y_cstride + a.y_coff;
      if (a.y_dtype == VM_BF16) reinterpret_cast<uint16_t*>(a.y)[o] = f2bf(v);
      else reinterpret_cast<float*>(a.y)[o] = v;
    }
  }
}

// MFMA head: cout == 1 recast as a 1x1 GEMM over the 9 taps.  For a TH x TW output tile the block computes
// Y[p][t] = sum_c X[p][c] * W[t][c] for every pixel p of the (TH+2) x (TW+2) input window (MFMA: 16 pixels x
// 16 tap-columns, 9 used), parks Y in LDS, then out(r,c) = sum_t Y[(r+dh_t, c+dw_t)][t].  Every input pixel is
// read once per tile (plus the halo) straight into MFMA A-fragments; no 3x3 re-reads, no VALU dot products.
// ALIAS (split-fp16 x3, vmatting/split3.py): x holds two slabs [l, h] of S = cin / 3 channels and the filter runs over
// [l, h, h] (cin = 3S): the k-steps of the third range reuse the second range's fragments (no extra loads), so one
// call does conv1_5's three products, the small ones first in each tap's chain
template <typename T, int TH, int TW, int NKS, bool ALIAS = false>
__global__ __launch_bounds__(256) void conv3x3_head_mfma(HeadArgs a) {
  constexpr int CE = 16 / sizeof(T);
  constexpr int KS = 4 * CE;  // channels per MFMA k-step
  constexpr int GE = 64 / sizeof(T);
  constexpr int IW = TW + 2, NPIX = (TH + 2) * IW, NG = (NPIX + 15) / 16;
  // pixel groups whose loads are in flight together (ALIAS: 8 of the 12 k-steps' fragments are loaded, so the
  // registers hold 4 groups)
  constexpr int GB = ALIAS ? 4 : 3;
  constexpr int NL = ALIAS ? 2 * (NKS / 3) : NKS;  // fragments loaded per pixel group
  __shared__ float ys[NG * 16 * 9];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sw = reinterpret_cast<T*>(smem);  // [9][cin_pad] tap-major
  const T* Wt = reinterpret_cast<const T*>(a.w);
  if (sizeof(T) == 2 && a.chunk_major) {
    // 16-byte pieces: 8 consecutive k of a granule are 8 consecutive channels of one tap (the element loop below
    // issued 14 dependent 2-byte loads per thread for a 384-channel head before any pixel load)
    const int nvec = a.ng * GE / 8;
    for (int v = threadIdx.x; v < nvec; v += 256) {
      const int k = v * 8, g = k / GE, cc = g / 9, tap = g - cc * 9;
      *reinterpret_cast<uint4*>(sw + tap * a.cin_pad + cc * GE + (k - g * GE)) =
          *reinterpret_cast<const uint4*>(Wt + k);
    }
  } else {
    for (int k = threadIdx.x; k < a.K_pad; k += 256) {
      int tap, c;
      if (a.chunk_major) {
        const int g = k / GE;
        if (g >= a.ng) continue;
        const int cc = g / 9;
        tap = g - cc * 9;
        c = cc * GE + (k - g * GE);
      } else {
        if (k >= a.K9) continue;
        tap = k / a.cin_pad;
        c = k - tap * a.cin_pad;
      }
      sw[tap * a.cin_pad + c] = Wt[k];
    }
  }
  __syncthreads();

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, ks = lane >> 4;
  const int H = a.H, W = a.W, cs = a.x_cstride, cin = a.cin_pad;
  uint4 wf[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const int c = s * KS + ks * CE;
    wf[s] = (col < 9 && c < cin) ? *reinterpret_cast<const uint4*>(sw + col * cin + c) : make_uint4(0, 0, 0, 0);
  }

  const int tw = (W + TW - 1) / TW, th = (H + TH - 1) / TH;
  const int b = blockIdx.x;
  const int n = b / (tw * th), rem = b - n * tw * th;
  const int r0 = (rem / tw) * TH, c0 = (rem % tw) * TW;
  const T* base = reinterpret_cast<const T*>(a.x) + a.x_coff + ((long)n * H + r0 - 1) * (long)W * cs;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, 0x7ffffff0, 0x00020000);

  for (int g0 = wave * GB; g0 < NG; g0 += 4 * GB) {
    uint4 xa[GB][NL];
    float pv[GB][4];  // head split: the partials this lane adds (issued with the input loads, used after the MFMAs)
#pragma unroll
    for (int u = 0; u < GB; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = (g0 + u) * 16 + 4 * ks + i, lr = j / IW, lc = j - lr * IW;
        const int hh = r0 - 1 + lr, ww = c0 - 1 + lc;
        const bool ok = a.part && col < 9 && g0 + u < NG && j < NPIX && (unsigned)hh < (unsigned)H &&
                        (unsigned)ww < (unsigned)W;
        pv[u][i] = ok ? a.part[(((long)n * H + hh) * W + ww) * 12 + col] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      const int j = (g0 + u) * 16 + col;  // input-window pixel of this lane's A row
      const int lr = j / IW, lc = j - lr * IW;
      const int hh = r0 - 1 + lr, ww = c0 - 1 + lc;
      const bool ok = g0 + u < NG && j < NPIX && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
      const int pix = (lr * W + ww) * cs;
#pragma unroll
      for (int s = 0; s < NL; ++s) {  // (ALIAS: the third range reuses the second's fragments)
        const int c = s * KS + ks * CE;
        const int off = (ok && c < cin) ? (pix + c) * (int)sizeof(T) : OOB;
        xa[u][s] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      if (g0 + u >= NG) break;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NKS; ++s) mma16<T>(xa[u][s < NL ? s : s - NKS / 3], wf[s], acc);
      if (col < 9) {
        const int p = (g0 + u) * 16 + 4 * ks;
#pragma unroll
        for (int i = 0; i < 4; ++i) ys[(p + i) * 9 + col] = acc[i] + pv[u][i];  // + the other channels' share
      }
    }
  }
  __syncthreads();

  const float bias = a.bias ? a.bias[0] : 0.f;
  const float sc = a.scale ? a.scale[0] : 1.f;
  const float sh = a.shift ? a.shift[0] : 0.f;
  for (int o = tid; o < TH * TW; o += 256) {
    const int orow = o / TW, ocol = o - orow * TW;
    const int h = r0 + orow, w = c0 + ocol;
    if (h >= H || w >= W) continue;
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) sum += ys[((orow + t / 3) * IW + ocol + t % 3) * 9 + t];
    if (a.yacc) sum += a.yacc[((long)n * H + h) * W + w];
    float v = (sum + bias) * sc + sh;
    if (a.y2) a.y2[((long)n * H + h) * W + w] = sigmoid_precise(v);
    if (a.act == VM_ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (a.act == VM_ACT_SIGMOID) v = sigmoid_precise(v);
    else if (a.act == VM_ACT_SOFTMAX) v = 1.f;
    const long oi = (((long)n * H + h) * W + w) * a.y_cstride + a.y_coff;
    if (a.y_dtype == VM_BF16) reinterpret_cast<uint16_t*>(a.y)[oi] = f2bf(v);
    else reinterpret_cast<float*>(a.y)[oi] = v;
  }
}

// ================================================================ head from per-tap partials (unet.py:203-205)
// conv1_5 over cat1 = [upconv_4, conv1_2] with both halves' shares taken where they were made (the folded upconv's
// and the pair kernel's epilogues): logits[p] = bias + sum_tap (pa + pb)[p + off(tap)][tap] (zero outside the
// frame), alpha = sigmoid(logits).  A block owns 8 x 64 output pixels: the (8+2) x 66 partial rows it needs are
// contiguous runs of 66 x 48 bytes, staged with 16-byte loads (taps summed over the two halves on the way, taps
// 9..11 dropped), and each thread then adds its pixels' 9 taps from LDS.
constexpr int HS_TH = 8, HS_TW = 64, HS_PW = HS_TW + 2, HS_PR = HS_TH + 2;
__global__ __launch_bounds__(256) void head_from_partials(const float* __restrict__ pa, const float* __restrict__ pb,
                                                          int N, int H, int W, const float* __restrict__ bias,
                                                          float* __restrict__ logits, int l_cstride,
                                                          float* __restrict__ alpha) {
  __shared__ float sp[HS_PR * HS_PW * 9];
  const int tw = (W + HS_TW - 1) / HS_TW, th = (H + HS_TH - 1) / HS_TH;
  const int b = blockIdx.x, n = b / (th * tw), rem = b - n * th * tw;
  const int y0 = (rem / tw) * HS_TH, x0 = (rem % tw) * HS_TW;
  const long img = (long)n * H * W;
  // stage: item i = (row, pixel, float4 group g < 3)
  for (int i = threadIdx.x; i < HS_PR * HS_PW * 3; i += 256) {
    const int g = i % 3, px = (i / 3) % HS_PW, row = i / (3 * HS_PW);
    const int yy = y0 - 1 + row, xx = x0 - 1 + px;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
      const long q = (img + (long)yy * W + xx) * 12 + 4 * g;
      const float4 u = *reinterpret_cast<const float4*>(pa + q), w = *reinterpret_cast<const float4*>(pb + q);
      v = make_float4(u.x + w.x, u.y + w.y, u.z + w.z, u.w + w.w);
    }
    float* d = sp + (row * HS_PW + px) * 9 + 4 * g;
    d[0] = v.x;
    if (g < 2) { d[1] = v.y; d[2] = v.z; d[3] = v.w; }  // (group 2 holds tap 8 and the three zero taps)
  }
  __syncthreads();
  const float b0 = bias ? bias[0] : 0.f;
  for (int o = threadIdx.x; o < HS_TH * HS_TW; o += 256) {
    const int ty = o / HS_TW, tx = o % HS_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    float s = b0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) s += sp[((ty + tap / 3) * HS_PW + tx + tap % 3) * 9 + tap];
    const long p = img + (long)y * W + x;
    if (logits) logits[p * l_cstride] = s;
    if (alpha) alpha[p] = sigmoid_precise(s);
  }
}

// ================================================================ dispatch
// conv_impl's cout == 1 route
int dispatch_head(const ConvCall& c, const PackGeom& g, int xalias, long M, hipStream_t st) {
  const vm_tensor* x = c.x;
  vm_tensor* y = c.y;
  const int dt = x->dtype, ce = 16 / elem_bytes(dt);
  const bool f16 = dt == VM_F16;
  HeadArgs h{};
  h.x = x->ptr; h.x_cstride = x->cstride; h.x_coff = x->coff; h.H = x->h; h.W = x->w; h.M = M;
  h.cin_pad = g.cin_pad; h.K9 = g.K9; h.K_pad = g.K_pad; h.chunk_major = g.chunk_major; h.ng = g.ng;
  h.w = c.packed; h.bias = c.bias; h.scale = c.scale; h.shift = c.shift; h.act = c.act;
  h.y = y->ptr; h.y_cstride = y->cstride; h.y_coff = y->coff; h.y_dtype = y->dtype; h.y2 = c.y2;
  h.part = c.head_part;
  h.yacc = c.y_acc;
  const int nks = (g.cin_pad + 4 * ce - 1) / (4 * ce);
  // the split-fp16 x3 head over a two-slab [l, h] view of 128-channel slabs (cin 384 as [l, h, h]): one call
  if (f16 && xalias == 128 && nks == 12 && g_opt.head_kernel == 0) {
    // 16-row tiles: an 18 x 66 input window per 16 x 64 outputs (1.16x the tile's pixels, 1.29x for 8 rows); the
    // per-pixel tap sums and the 9-tap epilogue are the same arithmetic whatever the tile: bit-identical
    constexpr int TW = 64;
    const int th16 = g_opt.head_th == 16 ? 16 : 8;
    const long tiles = (long)x->n * ((x->h + th16 - 1) / th16) * ((x->w + TW - 1) / TW);
    if (tiles > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3 head: too many tiles");
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_head_mfma<vm::f16_t, %d, %d, 12, true>", th16, TW);
    if (th16 == 16)
      hipLaunchKernelGGL((conv3x3_head_mfma<f16_t, 16, TW, 12, true>), dim3(tiles), dim3(256),
                         (size_t)9 * g.cin_pad * 2, st, h);
    else
      hipLaunchKernelGGL((conv3x3_head_mfma<f16_t, 8, TW, 12, true>), dim3(tiles), dim3(256),
                         (size_t)9 * g.cin_pad * 2, st, h);
    return check_launch("conv3x3_head_mfma");
  }
  if ((c.head_part || c.y_acc || f16) && (g_opt.head_kernel != 0 || nks > 8))
    return fail(VM_EUNSUPPORTED, "conv3x3 head: partials / accumulation / fp16 need the MFMA head kernel (cin <= 256, "
                                 "or 384 as a two-slab split-fp16 view)");
  if (g_opt.head_kernel == 0 && nks <= 8) {
    constexpr int TW = 64;
    // 16-row tiles for the bf16 128-channel head (cat1 of UNetVideo): input window 18 x 66 per 16 x 64 outputs
    // (1.16x the tile's bytes instead of 1.29x for 8 rows)
    const int TH = (dt == VM_BF16 && (nks == 4 || (nks == 2 && c.head_part)) && g_opt.head_th == 16) ? 16 : 8;
    const long tiles = (long)x->n * ((x->h + TH - 1) / TH) * ((x->w + TW - 1) / TW);
    if (tiles > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3 head: too many tiles");
    const size_t lds = (size_t)9 * g.cin_pad * elem_bytes(dt);
    const int nk = nks <= 1 ? 1 : nks <= 2 ? 2 : nks <= 4 ? 4 : 8;
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_head_mfma<%s, %d, %d, %d>",
             dt == VM_BF16 ? "unsigned short" : "float", TH, TW, nk);
#define VM_HEAD_MFMA(TT, NK) \
hipLaunchKernelGGL((conv3x3_head_mfma<TT, 8, TW, NK>), dim3(tiles), dim3(256), lds, st, h)
    if (f16) {
      snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_head_mfma<vm::f16_t, 8, %d, %d>", TW, nk);
      if (nk == 1) VM_HEAD_MFMA(f16_t, 1); else if (nk == 2) VM_HEAD_MFMA(f16_t, 2);
      else if (nk == 4) VM_HEAD_MFMA(f16_t, 4); else VM_HEAD_MFMA(f16_t, 8);
    } else if (TH == 16 && nk == 2) {  // the split head's 64-channel half
      hipLaunchKernelGGL((conv3x3_head_mfma<uint16_t, 16, TW, 2>), dim3(tiles), dim3(256), lds, st, h);
    } else if (TH == 16) {
      hipLaunchKernelGGL((conv3x3_head_mfma<uint16_t, 16, TW, 4>), dim3(tiles), dim3(256), lds, st, h);
    } else if (dt == VM_BF16) {
      if (nk == 1) VM_HEAD_MFMA(uint16_t, 1); else if (nk == 2) VM_HEAD_MFMA(uint16_t, 2);
      else if (nk == 4) VM_HEAD_MFMA(uint16_t, 4); else VM_HEAD_MFMA(uint16_t, 8);
    } else {
      if (nk == 1) VM_HEAD_MFMA(float, 1); else if (nk == 2) VM_HEAD_MFMA(float, 2);
      else if (nk == 4) VM_HEAD_MFMA(float, 4); else VM_HEAD_MFMA(float, 8);
    }
#undef VM_HEAD_MFMA
    return check_launch("conv3x3_head_mfma");
  }
  constexpr int P = 8;
  const int nch = g.cin_pad / (16 * ce);
  if ((nch == 1 || nch == 2) && g.cin_pad % (16 * ce) == 0 && g_opt.head_kernel != 1) {
    const long strips = (M / x->w) * ((x->w + P - 1) / P);
    const int grid = grid_for((strips + 15) / 16, 1, 256 * 8);
    const size_t lds = (size_t)9 * g.cin_pad * elem_bytes(dt);
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_head_strip<%s, %d, %d>",
             dt == VM_BF16 ? "unsigned short" : "float", nch, P);
    if (dt == VM_BF16) {
      if (nch == 1) hipLaunchKernelGGL((conv3x3_head_strip<uint16_t, 1, P>), dim3(grid), dim3(256), lds, st, h);
      else hipLaunchKernelGGL((conv3x3_head_strip<uint16_t, 2, P>), dim3(grid), dim3(256), lds, st, h);
    } else {
      if (nch == 1) hipLaunchKernelGGL((conv3x3_head_strip<float, 1, P>), dim3(grid), dim3(256), lds, st, h);
      else hipLaunchKernelGGL((conv3x3_head_strip<float, 2, P>), dim3(grid), dim3(256), lds, st, h);
    }
    return check_launch("conv3x3_head_strip");
  }
  const int grid = grid_for((M + 15) / 16, 1, 256 * 8);
  const size_t lds = (size_t)9 * g.cin_pad * 4;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_head<%s>", dt == VM_BF16 ? "unsigned short" : "float");
  if (dt == VM_BF16) hipLaunchKernelGGL(conv3x3_head<uint16_t>, dim3(grid), dim3(256), lds, st, h);
  else hipLaunchKernelGGL(conv3x3_head<float>, dim3(grid), dim3(256), lds, st, h);
  return check_launch("conv3x3_head");
}

}  // namespace vm

using namespace vm;

extern "C" int vm_conv3x3_head_from_partials(const float* pa, const float* pb, int n, int h, int w, const float* bias,
                                             vm_tensor* logits, float* alpha, void* stream) {
  if (!pa || !pb || n <= 0 || h <= 0 || w <= 0) return fail(VM_EINVAL, "head_from_partials: bad argument");
  if (logits && (!valid_tensor(logits) || logits->dtype != VM_F32 || logits->n != n || logits->h != h ||
                 logits->w != w || logits->c != 1))
    return fail(VM_EINVAL, "head_from_partials: logits must be an f32 [n,h,w,1] view");
  const long tiles = (long)n * ((h + HS_TH - 1) / HS_TH) * ((w + HS_TW - 1) / HS_TW);
  if (tiles > 0x7fffffffL || (long)n * h * w * 12 > 0x7fffffffffffL) return fail(VM_EUNSUPPORTED, "head_from_partials");
  float* lp = logits ? reinterpret_cast<float*>(logits->ptr) + logits->coff : nullptr;
  hipLaunchKernelGGL(head_from_partials, dim3((unsigned)tiles), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), pa, pb, n, h, w, bias, lp, logits ? logits->cstride : 1,
                     alpha);
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::head_from_partials");
  return check_launch("head_from_partials");
}
