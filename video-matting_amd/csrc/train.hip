// Backward pass + optimizer of the config-5 training step (train.py:288-343, video_procedure; the same graph
// as simple_procedure, train.py:176-227): the gradient of
//   loss = mean(0.5*regular_l1(pred, gt) + 0.5*regular_l1(composite(raw_fg, bg, pred), cmp))   (train.py:294-298)
// through UNetSimple's trainable layers (unet_simple.py:116-142: conv + bias -> batch_norm(is_training) -> relu,
// upconv_concat's resize -> conv -> relu -> concat -> batch_norm), and tf.train.AdamOptimizer's update
// (train.py:302-304).  The frozen VGG towers (tf.constant weights, unet_simple.py:109-113) need no gradient.
//
//   loss_backward   dL/dlogits of sigmoid(logits) under the Charbonnier alpha + compositional loss
//   bn_backward     fused-BN gradient (batch statistics), optional relu mask from the BN+relu output:
//                   dx = gamma*rstd*(g - sum(g)/M - xhat*sum(g*xhat)/M), dgamma = sum(g*xhat), dbeta = sum(g)
//   conv_wgrad      the filter gradients: wgrad.hip
//   conv dgrad      the forward conv kernels on flipped, transposed weights (flip_weights here)
//   resize_backward adjoint of the TF-1 legacy bilinear resize, gathered per input element (no atomics)
//   relu_backward   dy * (y > 0)
//   maxpool_bwd     tf.nn.max_pool 2x2/2 SAME adjoint: the window's gradient to its first maximum (small.py:40,42)
//   adam            TF ApplyAdam: m += (g-m)(1-b1); v += (g^2-v)(1-b2); var -= m*lr_t/(sqrt(v)+eps)

#include <algorithm>
#include <cstring>

#include "train_common.h"

namespace vm {
namespace trn {

// ---------------------------------------------------------------- loss backward (train.py:21-28, 294-298)
// s_loss is [N,H,W,3] (the [N,H,W,1] alpha term broadcast), so with P pixels
//   dL/dpred = 0.5/(3P) * (3*(a-g)/La + sum_k e_k/Lc_k * (fg_k - bg_k)),   e_k = a*fg_k + (1-a)*bg_k - cmp_k
// and dL/dlogits = dL/dpred * a*(1-a) (tf.nn.sigmoid's gradient in terms of its output).
__global__ __launch_bounds__(256) void loss_backward_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                            const float* __restrict__ fg, const float* __restrict__ bg,
                                                            const float* __restrict__ cmp, long P, float* dlogit) {
  const float eps2 = 1e-6f * 1e-6f;
  const float k = 0.5f / (3.0f * (float)P);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < P; i += (long)gridDim.x * blockDim.x) {
    const float a = pred[i];
    const float d = a - gt[i];
    float s = 3.f * d / sqrtf(d * d + eps2);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float f = fg[i * 3 + j], b = bg[i * 3 + j];
      const float e = a * f + (1.f - a) * b - cmp[i * 3 + j];
      s += e / sqrtf(e * e + eps2) * (f - b);
    }
    dlogit[i] = k * s * a * (1.f - a);
  }
}

// ---------------------------------------------------------------- batch-norm backward (training statistics)

template <bool MASK>
__device__ __forceinline__ float grad_in(const V& dy, const V& y, long p, int c) {
  const float g = ld(dy, p, c);
  if (MASK) return ld(y, p, c) > 0.f ? g : 0.f;
  return g;
}

// per (channel group, pixel block): double partial sums of g and g*xhat (x == NULL: g only).  CP lanes per pixel as
// in elementwise.hip's bn_partial_kernel: narrow tensors put 64 / CP pixels in flight per wave.
template <bool MASK, int CP>
__global__ __launch_bounds__(256) void bn_bwd_partial(V x, V dy, V y, const float* mean, const float* var, float eps,
                                                      double* part, int nblk) {
  constexpr int PPW = 64 / CP;
  __shared__ double sh[3][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * CP + (lane % CP);
  const long M = (long)dy.n * dy.h * dy.w;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (c < dy.c) {
    const float m = x.p ? mean[c] : 0.f;
    const float r = x.p ? 1.0f / sqrtf(var[c] + eps) : 0.f;
    const long stp = (long)nblk * 4 * PPW;
    long p = ((long)blockIdx.y * 4 + wave) * PPW + lane / CP;
    // 4 pixels' loads in flight per lane before any is summed (same summation order as one at a time)
    for (; p + 3 * stp < M; p += 4 * stp) {
      float g[4], xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        g[u] = grad_in<MASK>(dy, y, p + u * stp, c);
        xv[u] = x.p ? ld(x, p + u * stp, c) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s1 += g[u];
        if (x.p) {
          const float xh = (xv[u] - m) * r;
          s2 += (double)g[u] * (double)xh;
          s3 += (double)xh;
        }
      }
    }
    for (; p < M; p += stp) {
      const float g = grad_in<MASK>(dy, y, p, c);
      s1 += g;
      if (x.p) {
        const float xh = (ld(x, p, c) - m) * r;
        s2 += (double)g * (double)xh;
        s3 += (double)xh;
      }
    }
  }
  sh[0][wave][lane] = s1;
  sh[1][wave][lane] = s2;
  sh[2][wave][lane] = s3;
  __syncthreads();
  if ((int)threadIdx.x < CP && c < dy.c) {
    s1 = s2 = s3 = 0.0;
    for (int w = 0; w < 4; ++w)
      for (int k = 0; k < PPW; ++k) {
        s1 += sh[0][w][k * CP + threadIdx.x];
        s2 += sh[1][w][k * CP + threadIdx.x];
        s3 += sh[2][w][k * CP + threadIdx.x];
      }
    part[(long)c * nblk + blockIdx.y] = s1;  // channel-major [k][C][nblk] (vm_common.h fold_columns)
    part[(long)nblk * dy.c + (long)c * nblk + blockIdx.y] = s2;
    part[2L * nblk * dy.c + (long)c * nblk + blockIdx.y] = s3;
  }
}

// folds the partials; with dbias also the gradient of a bias added before the BN (new_conv's conv bias,
// unet_simple.py:23-25): sum_p dx = gamma*rstd*(sum g - M*mean g - sum xhat * sum(g*xhat)/M), zero in exact
// arithmetic (BN removes the bias), evaluated from the same double sums instead of a pass over dx
__global__ __launch_bounds__(256) void bn_bwd_final(const double* part, int nblk, int C, float* sum_g, float* sum_gx,
                                                    float* dbias, const float* gamma, const float* var, float eps,
                                                    long M) {
  const int c = blockIdx.x;
  double r[3];
  fold_columns(part, nblk, C, c, dbias ? 3 : 2, r);
  if (threadIdx.x == 0) {
    const double s1 = r[0], s2 = r[1], s3 = r[2];
    if (sum_g) sum_g[c] = (float)s1;
    if (sum_gx) sum_gx[c] = (float)s2;
    if (dbias) {
      const double rs = 1.0 / sqrt((double)var[c] + (double)eps), g = gamma ? gamma[c] : 1.0;
      dbias[c] = (float)(g * rs * (s1 - (double)M * (s1 / (double)M) - s3 * s2 / (double)M));
    }
  }
}

// Vectorised BN backward for whole 8-channel runs (f32 x / dy / dx, an optional bf16 relu mask y and bf16 copy dx2;
// every view 16-byte aligned, C % 8 == 0, C <= 512): a lane takes 8 channels of a pixel — two f32x4 of x and of dy,
// one 16-byte y chunk — where the per-channel forms above issue a 4-byte access per element (~3.5 TB/s on the 32-
// channel full-resolution layers of the config-5 step).  Per element the same expressions, summed in f64 per block
// into the same [3][C][nblk] tables (another partition of the pixels; bn_bwd_final folds them as before).
__device__ __forceinline__ void ld8f32(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ld8bf(const uint16_t* p, float (&v)[8]) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = bf2f((uint16_t)(w4[k] & 0xffffu));
    v[2 * k + 1] = bf2f((uint16_t)(w4[k] >> 16));
  }
}
struct Bn8 {
  const float* x;
  const float* dy;
  const uint16_t* y;  // bf16 relu output (mask) or nullptr
  float* dx;
  uint16_t* dx2;      // bf16 copy or nullptr
  int xcs, dycs, ycs, dxcs, dx2cs, C;
  long M;
};

template <bool MASK, int TPG>
__global__ __launch_bounds__(256) void bn_bwd_partial8(Bn8 a, const float* mean, const float* var, float eps,
                                                       double* part, int nblk) {
  constexpr int PPB = 256 / TPG;
  __shared__ double sh[8][256];
  const int t = threadIdx.x, j = t % TPG, pl = t / TPG, c0 = 8 * j;
  double s1[8], s2[8], s3[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = s3[k] = 0.0;
  if (c0 < a.C) {
    float m[8], r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      m[k] = mean[c0 + k];
      r[k] = 1.0f / sqrtf(var[c0 + k] + eps);
    }
    for (long p = (long)blockIdx.x * PPB + pl; p < a.M; p += (long)nblk * PPB) {
      float g[8], xv[8];
      ld8f32(a.dy + p * a.dycs + c0, g);
      ld8f32(a.x + p * a.xcs + c0, xv);
      if constexpr (MASK) {
        float yv[8];
        ld8bf(a.y + p * a.ycs + c0, yv);
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1[k] += g[k];
        const float xh = (xv[k] - m[k]) * r[k];
        s2[k] += (double)g[k] * (double)xh;
        s3[k] += (double)xh;
      }
    }
  }
  // three tables through one 16 KB staging buffer
#pragma unroll
  for (int tab = 0; tab < 3; ++tab) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k][t] = tab == 0 ? s1[k] : tab == 1 ? s2[k] : s3[k];
    __syncthreads();
    for (int c = t; c < a.C; c += 256) {
      const int jj = c >> 3, k = c & 7;
      double v = 0.0;
      for (int q = 0; q < PPB; ++q) v += sh[k][q * TPG + jj];
      part[(long)tab * nblk * a.C + (long)c * nblk + blockIdx.x] = v;
    }
    __syncthreads();
  }
}

template <bool MASK, bool DX2, int TPG>
__global__ __launch_bounds__(256) void bn_bwd_apply8(Bn8 a, const float* mean, const float* var, const float* gamma,
                                                     float eps, const float* sum_g, const float* sum_gx) {
  constexpr int PPB = 256 / TPG;
  const int t = threadIdx.x, j = t % TPG, pl = t / TPG, c0 = 8 * j;
  if (c0 >= a.C) return;
  const float invM = 1.0f / (float)a.M;
  float m[8], r[8], kk[8], sg[8], sgx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    r[k] = 1.0f / sqrtf(var[c] + eps);
    m[k] = mean[c];
    kk[k] = (gamma ? gamma[c] : 1.f) * r[k];
    sg[k] = sum_g[c] * invM;
    sgx[k] = sum_gx[c] * invM;
  }
  for (long p = (long)blockIdx.x * PPB + pl; p < a.M; p += (long)gridDim.x * PPB) {
    float g[8], xv[8], v[8];
    ld8f32(a.dy + p * a.dycs + c0, g);
    ld8f32(a.x + p * a.xcs + c0, xv);
    if constexpr (MASK) {
      float yv[8];
      ld8bf(a.y + p * a.ycs + c0, yv);
#pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = kk[k] * (g[k] - sg[k] - (xv[k] - m[k]) * r[k] * sgx[k]);
    float* o = a.dx + p * a.dxcs + c0;
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
    if constexpr (DX2) *reinterpret_cast<uint4*>(a.dx2 + p * a.dx2cs + c0) = Chunk<uint16_t>::pack(v);
  }
}

// elementwise passes over [M pixels x C channels]: CP (power of two >= C, at most 64) lanes per pixel, channel
// block blockIdx.y, so a lane keeps one channel (its per-channel constants in registers) and no element index is
// ever divided
// count > 0: the sums are over `count` pixels (SyncBN: all replicas' pixels), else over this view's M
template <bool MASK, int CP>
__global__ __launch_bounds__(256) void bn_bwd_apply(V x, V dy, V y, const float* mean, const float* var,
                                                    const float* gamma, float eps, const float* sum_g,
                                                    const float* sum_gx, V dx, V dx2, long count = 0) {
  const long M = (long)dy.n * dy.h * dy.w;
  const int c = blockIdx.y * CP + (threadIdx.x & (CP - 1));
  if (c >= dy.c) return;
  const float invM = 1.0f / (float)(count > 0 ? count : M);
  const float r = 1.0f / sqrtf(var[c] + eps);
  const float m = mean[c];
  const float k = (gamma ? gamma[c] : 1.f) * r;
  const float sg = sum_g[c] * invM, sgx = sum_gx[c] * invM;
  const long step = (long)gridDim.x * (blockDim.x / CP);
  long p = (long)blockIdx.x * (blockDim.x / CP) + threadIdx.x / CP;
  for (; p + 3 * step < M; p += 4 * step) {  // 4 pixels' loads in flight before the stores
    float xv[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xv[u] = ld(x, p + u * step, c);
      g[u] = grad_in<MASK>(dy, y, p + u * step, c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float v = k * (g[u] - sg - (xv[u] - m) * r * sgx);
      st(dx, p + u * step, c, v);
      if (dx2.p) st(dx2, p + u * step, c, v);
    }
  }
  for (; p < M; p += step) {
    const float xh = (ld(x, p, c) - m) * r;
    const float g = grad_in<MASK>(dy, y, p, c);
    const float v = k * (g - sg - xh * sgx);
    st(dx, p, c, v);
    if (dx2.p) st(dx2, p, c, v);  // the bf16 copy the data-gradient conv reads
  }
}

// the unmasked 2-channel f32 case (the training step's select1_* convs) one pixel per thread with 8-byte loads and
// stores: at their 32-byte pixel stride the 2-lanes-per-pixel form above ran at ~0.5 TB/s, its per-element dtype
// branches and 64-bit index products the bound.  Per element the same expression as bn_bwd_apply, so the same values.
__global__ __launch_bounds__(256) void bn_bwd_apply2_f32(const float* x, int xcs, const float* dy, int dycs, float* dx,
                                                         int dxcs, long M, const float* mean, const float* var,
                                                         const float* gamma, float eps, const float* sum_g,
                                                         const float* sum_gx) {
  const float invM = 1.0f / (float)M;
  float r[2], m[2], k[2], sg[2], sgx[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    r[c] = 1.0f / sqrtf(var[c] + eps);
    m[c] = mean[c];
    k[c] = (gamma ? gamma[c] : 1.f) * r[c];
    sg[c] = sum_g[c] * invM;
    sgx[c] = sum_gx[c] * invM;
  }
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < M; p += (long)gridDim.x * blockDim.x) {
    const float2 x2 = *reinterpret_cast<const float2*>(x + p * xcs);
    const float2 g2 = *reinterpret_cast<const float2*>(dy + p * dycs);
    const float xv[2] = {x2.x, x2.y}, g[2] = {g2.x, g2.y};
    float v[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) v[c] = k[c] * (g[c] - sg[c] - (xv[c] - m[c]) * r[c] * sgx[c]);
    *reinterpret_cast<float2*>(dx + p * dxcs) = make_float2(v[0], v[1]);
  }
}

static bool f32_pair(const vm_tensor* t) {  // 2 f32 channels at an 8-byte aligned offset of every pixel
  return t->dtype == VM_F32 && t->c == 2 && t->cstride % 2 == 0 && t->coff % 2 == 0 &&
         reinterpret_cast<uintptr_t>(t->ptr) % 8 == 0;
}

// channels [0, split) go to dxlo at c, [split, C) to dx / dx2 at c - split (split 0: all to dx / dx2)
template <int CP>
__global__ __launch_bounds__(256) void relu_bwd_kernel(V dy, V y, V dx, V dx2, V dxlo, int split) {
  const long M = (long)dy.n * dy.h * dy.w;
  const int c = blockIdx.y * CP + (threadIdx.x & (CP - 1));
  if (c >= dy.c) return;
  const bool lo = c < split;
  const V o = lo ? dxlo : dx;
  const int oc = lo ? c : c - split;
  const bool two = dx2.p && !lo;
  const long step = (long)gridDim.x * (blockDim.x / CP);
  long p = (long)blockIdx.x * (blockDim.x / CP) + threadIdx.x / CP;
  for (; p + 3 * step < M; p += 4 * step) {  // 4 pixels' loads in flight before the stores
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld(y, p + u * step, c) > 0.f ? ld(dy, p + u * step, c) : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      st(o, p + u * step, oc, v[u]);
      if (two) st(dx2, p + u * step, oc, v[u]);
    }
  }
  for (; p < M; p += step) {
    const float v = ld(y, p, c) > 0.f ? ld(dy, p, c) : 0.f;
    st(o, p, oc, v);
    if (two) st(dx2, p, oc, v);
  }
}

static int lanes_for(int C) { return C > 32 ? 64 : C > 16 ? 32 : C > 8 ? 16 : C > 4 ? 8 : C > 2 ? 4 : C > 1 ? 2 : 1; }

// grid of an [M x C] packed-lane pass: x = pixel blocks (256/CP pixels each, capped), y = channel blocks
static dim3 lanes_grid(long M, int C, int cp) {
  const long px = (M + 256 / cp - 1) / (256 / cp);
  return dim3((unsigned)(px < 4096 ? px : 4096), (unsigned)((C + cp - 1) / cp));
}

#define VM_CP_SWITCH(CP_, CALL) \
  switch (CP_) {                \
    case 1: CALL(1); break;     \
    case 2: CALL(2); break;     \
    case 4: CALL(4); break;     \
    case 8: CALL(8); break;     \
    case 16: CALL(16); break;   \
    case 32: CALL(32); break;   \
    default: CALL(64); break;   \
  }

template <bool MASK>
static void launch_bn_bwd_partial(const V& x, const V& dy, const V& y, const float* mean, const float* var, float eps,
                                  double* part, int nb, hipStream_t st) {
  const int C = dy.c, cp = lanes_for(C);
  dim3 g(cp == 64 ? (C + 63) / 64 : 1, nb), b(256);
#define VM_BP(CP) hipLaunchKernelGGL((bn_bwd_partial<MASK, CP>), g, b, 0, st, x, dy, y, mean, var, eps, part, nb)
  VM_CP_SWITCH(cp, VM_BP)
#undef VM_BP
}

// ---------------------------------------------------------------- max-pool backward (small.py:40,42)
// Adjoint of tf.nn.max_pool 2x2/2 SAME (vm_maxpool2x2_same_nhwc): an input element receives its window's gradient
// iff it is the window's FIRST maximum in row-major order — TF's MaxPoolGrad scans the window with a strict '>'
// (taps past an odd edge are not in the window).  dx = add + that share (add optional; it may alias dx: each lane
// reads its own element before writing it).  CP lanes per input pixel as the other elementwise passes; a lane
// re-reads its window's other three values (L1/L2 hits) instead of a stored argmax.
template <int CP>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(V x, V dy, V add, V dx) {
  const long HW = (long)x.h * x.w, M = (long)x.n * HW;
  const int c = blockIdx.y * CP + (threadIdx.x & (CP - 1));
  if (c >= x.c) return;
  const int oh = dy.h, ow = dy.w;
  const long step = (long)gridDim.x * (blockDim.x / CP);
  for (long p = (long)blockIdx.x * (blockDim.x / CP) + threadIdx.x / CP; p < M; p += step) {
    const int n = (int)(p / HW);
    const int r = (int)(p - (long)n * HW);
    const int iy = r / x.w, ix = r - iy * x.w;
    const int y0 = iy & ~1, x0 = ix & ~1;
    const long base = (long)n * HW;
    float best = 0.f;
    int win = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
      if (yy < x.h && xx < x.w) {
        const float v = ld(x, base + (long)yy * x.w + xx, c);
        if (win < 0 || v > best) { best = v; win = k; }
      }
    }
    float g = win == ((iy - y0) << 1) + (ix - x0) ? ld(dy, ((long)n * oh + (iy >> 1)) * ow + (ix >> 1), c) : 0.f;
    if (add.p) g += ld(add, p, c);
    st(dx, p, c, g);
  }
}

// ---------------------------------------------------------------- relu conv backward front end (UNetImage training)
// For y = relu(conv(x) + b) (unet.py:35-42,65-74), one pass from the incoming gradient to what the conv's filter /
// data gradients read: dz = (y > 0) * g, written ONLY as the bf16 copy those MFMA convs read (no f32 dz), with the
// bias gradient sum_p dz from the same pass (f64 partials per block, folded in fixed order: deterministic).
//   plain: g = dy (+ add)                                 dy, add, y, dz all [n,h,w,c]
//   POOL : g = add + the 2x2 SAME max-pool adjoint of dy   dy [n,ceil(h/2),ceil(w/2),c], y / add / dz [n,h,w,c]
//          (tf.nn.max_pool's gradient to the window's first maximum of y in row-major order, TF MaxPoolGrad; the
//          skip half of an [up, skip] concat carries `add`, unet.py:62, so pool adjoint + concat gradient + relu
//          mask + bias sum are one pass instead of three)
// One lane per channel (CP lanes per pixel / window), a block's 4 waves stride over pixels (windows).
template <bool POOL, int CP>
__global__ __launch_bounds__(256) void relu_bwd_bias_kernel(V dy, V y, V add, V dz, double* part, int nblk) {
  constexpr int PPW = 64 / CP;
  __shared__ double sh[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * CP + (lane % CP);
  double s = 0.0;
  if (c < y.c) {
    const long units = POOL ? (long)dy.n * dy.h * dy.w : (long)y.n * y.h * y.w;
    const long stp = (long)nblk * 4 * PPW;
    for (long u = ((long)blockIdx.y * 4 + wave) * PPW + lane / CP; u < units; u += stp) {
      if constexpr (!POOL) {
        float g = ld(dy, u, c);
        if (add.p) g += ld(add, u, c);
        const float z = ld(y, u, c) > 0.f ? g : 0.f;
        st(dz, u, c, z);
        s += (double)z;
      } else {
        const long hw = (long)dy.h * dy.w;
        const int n = (int)(u / hw);
        const int r = (int)(u - (long)n * hw);
        const int oy = r / dy.w, ox = r - oy * dy.w;
        const long base = (long)n * y.h * y.w;
        const float gp = ld(dy, u, c);
        float yv[4];
        long pix[4];
        bool in[4];
        float best = 0.f;
        int win = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int yy = 2 * oy + (k >> 1), xx = 2 * ox + (k & 1);
          in[k] = yy < y.h && xx < y.w;
          pix[k] = base + (long)yy * y.w + xx;
          yv[k] = in[k] ? ld(y, pix[k], c) : 0.f;
          if (in[k] && (win < 0 || yv[k] > best)) {
            best = yv[k];
            win = k;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!in[k]) continue;
          float g = k == win ? gp : 0.f;
          if (add.p) g += ld(add, pix[k], c);
          const float z = yv[k] > 0.f ? g : 0.f;
          st(dz, pix[k], c, z);
          s += (double)z;
        }
      }
    }
  }
  sh[wave][lane] = s;
  __syncthreads();
  if ((int)threadIdx.x < CP && c < y.c) {
    s = 0.0;
    for (int w = 0; w < 4; ++w)
      for (int k = 0; k < PPW; ++k) s += sh[w][k * CP + threadIdx.x];
    part[(long)c * nblk + blockIdx.y] = s;  // channel-major [C][nblk] (vm_common.h fold_columns)
  }
}

// Vectorised form for the bf16 path (bf16 y and dz, f32 dy / add; C % 8 == 0, C <= 512): a lane takes 8 channels of
// a pixel — one 16-byte y chunk, two f32x4 of dy and of add, one 16-byte dz store — where the per-element form above
// issued a 2- to 4-byte access per channel (~2.5 TB/s).  Per element the same arithmetic (g = dy, g += add in f32;
// the first-maximum pool adjoint; z rounded to bf16 as st() does), so dz is bit-identical; the channel sums are f64
// partials per block in another partition of the pixels, folded in fixed order by fold_sum_kernel as before.
// TPG: lanes per pixel (a power of two >= C / 8).  TD / TA: f32 or bf16 dy / add (the bf16 training path hands its
// data gradients over as bf16; a bf16 chunk widens exactly to f32, so the arithmetic after the load is the same).
template <bool POOL, bool ADD, int TPG, typename TD = float, typename TA = float>
__global__ __launch_bounds__(256) void relu_bwd_bias8_kernel(const TD* __restrict__ dy, int dycs,
                                                             const uint16_t* __restrict__ y, int ycs,
                                                             const TA* __restrict__ add, int acs,
                                                             uint16_t* __restrict__ dz, int zcs, int N, int H, int W,
                                                             int DH, int DW, int C, double* part, int nblk) {
  constexpr int PPB = 256 / TPG;
  __shared__ double sh[8][256];
  const int t = threadIdx.x, j = t % TPG, pl = t / TPG;
  const int c0 = 8 * j;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto ld8y = [&](const uint16_t* p, float (&v)[8]) __attribute__((always_inline)) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = bf2f((uint16_t)(w4[k] & 0xffffu));
      v[2 * k + 1] = bf2f((uint16_t)(w4[k] >> 16));
    }
  };
  auto ld8f = [&](const auto* p, float (&v)[8]) __attribute__((always_inline)) {
    if constexpr (sizeof(*p) == 4) {
      const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
      ld8y(reinterpret_cast<const uint16_t*>(p), v);
    }
  };
  auto st8 = [&](uint16_t* p, const float (&z)[8]) __attribute__((always_inline)) {
    uint32_t w4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = (uint32_t)f2bf(z[2 * k]) | ((uint32_t)f2bf(z[2 * k + 1]) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
  };
  if (c0 < C) {
    const long units = POOL ? (long)N * DH * DW : (long)N * H * W;
    for (long u = (long)blockIdx.x * PPB + pl; u < units; u += (long)gridDim.x * PPB) {
      if constexpr (!POOL) {
        float g[8], yv[8], z[8];
        ld8f(dy + u * dycs + c0, g);
        if constexpr (ADD) {
          float a8[8];
          ld8f(add + u * acs + c0, a8);
#pragma unroll
          for (int k = 0; k < 8; ++k) g[k] += a8[k];
        }
        ld8y(y + u * ycs + c0, yv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          z[k] = yv[k] > 0.f ? g[k] : 0.f;
          s[k] += (double)z[k];
        }
        st8(dz + u * zcs + c0, z);
      } else {
        const long hw = (long)DH * DW;
        const int n = (int)(u / hw);
        const int r = (int)(u - (long)n * hw);
        const int oy = r / DW, ox = r - oy * DW;
        float gp[8], yv[4][8];
        ld8f(dy + u * dycs + c0, gp);
        long pix[4];
        bool in[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int yy = 2 * oy + (q >> 1), xx = 2 * ox + (q & 1);
          in[q] = yy < H && xx < W;
          pix[q] = ((long)n * H + yy) * W + xx;
          if (in[q]) ld8y(y + pix[q] * ycs + c0, yv[q]);
          else
#pragma unroll
            for (int k = 0; k < 8; ++k) yv[q][k] = 0.f;
        }
        int win[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // TF MaxPoolGrad: the window's first maximum
          float best = 0.f;
          win[k] = -1;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (in[q] && (win[k] < 0 || yv[q][k] > best)) {
              best = yv[q][k];
              win[k] = q;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!in[q]) continue;
          float a8[8], z[8];
          if constexpr (ADD) ld8f(add + pix[q] * acs + c0, a8);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float g = k < 8 && win[k] == q ? gp[k] : 0.f;
            if constexpr (ADD) g += a8[k];
            z[k] = yv[q][k] > 0.f ? g : 0.f;
            s[k] += (double)z[k];
          }
          st8(dz + pix[q] * zcs + c0, z);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[k][t] = s[k];
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    const int jj = c >> 3, k = c & 7;
    double r = 0.0;
    for (int q = 0; q < PPB; ++q) r += sh[k][q * TPG + jj];
    part[(long)c * nblk + blockIdx.x] = r;  // channel-major [C][nblk], as relu_bwd_bias_kernel
  }
}

__global__ __launch_bounds__(256) void fold_sum_kernel(const double* part, int nblk, int C, float* out) {
  double r[3];
  fold_columns(part, nblk, C, blockIdx.x, 1, r);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)r[0];
}

// ---------------------------------------------------------------- resize backward (adjoint of resize_tf1)
__device__ __forceinline__ void tf1c(int i, float scale, int in, int& lo, int& hi, float& lerp) {
#pragma clang fp contract(off)
  const float src = (float)i * scale;
  const float fl = floorf(src);
  lo = (int)fl;
  hi = min(lo + 1, in - 1);
  lerp = src - fl;
}

// Gather form (deterministic, no atomics): input pixel (iy, ix) collects the output pixels whose taps hit it.  With
// scale = in/out <= ~1 those lie in rows [floor((iy-1)/sy)-1, ceil((iy+1)/sy)+1] (likewise columns); each candidate's
// taps are recomputed with the forward's exact f32 coordinate arithmetic, so the weights match it bit for bit.
__device__ __forceinline__ float tap_w(int o, float scale, int in, int i) {
  int lo, hi;
  float l;
  tf1c(o, scale, in, lo, hi, l);
  return (lo == i ? 1.f - l : 0.f) + (hi == i ? l : 0.f);
}

__global__ void resize_bwd_kernel(V dy, float* dx, int ih, int iw, float sy, float sx) {
  const long total = (long)dy.n * ih * iw * dy.c;
  const int C = dy.c;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long ip = i / C;
    const int ix = (int)(ip % iw);
    const long t = ip / iw;
    const int iy = (int)(t % ih);
    const int n = (int)(t / ih);
    const int r0 = max(0, (int)floorf((iy - 1) / sy) - 1), r1 = min(dy.h - 1, (int)ceilf((iy + 1) / sy) + 1);
    const int q0 = max(0, (int)floorf((ix - 1) / sx) - 1), q1 = min(dy.w - 1, (int)ceilf((ix + 1) / sx) + 1);
    float acc = 0.f;
    for (int oh = r0; oh <= r1; ++oh) {
      const float wy = tap_w(oh, sy, ih, iy);
      if (wy == 0.f) continue;
      float row = 0.f;
      for (int ow = q0; ow <= q1; ++ow) {
        const float wx = tap_w(ow, sx, iw, ix);
        if (wx != 0.f) row += wx * ld(dy, ((long)n * dy.h + oh) * dy.w + ow, c);
      }
      acc += wy * row;
    }
    dx[i] = acc;
  }
}

// the same gather, 4 channels per thread with 16-byte loads / stores (c % 4 == 0, 16-byte aligned dy channel
// vectors): the taps and weights are computed once per 4 channels; per channel the arithmetic is resize_bwd_kernel's
// TD: dy f32 (16-byte loads) or bf16 (8-byte loads: the bf16 training path's data gradients); TX: dx f32, or bf16
// (each f32 sum rounded to nearest even once, as a bf16 store of the f32 result would)
template <typename TD, typename TX = float>
__global__ void resize_bwd_kernel4(V dy, TX* dx, int ih, int iw, float sy, float sx) {
  const int C4 = dy.c / 4;
  const long total = (long)dy.n * ih * iw * C4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const long ip = i / C4;
    const int ix = (int)(ip % iw);
    const long t = ip / iw;
    const int iy = (int)(t % ih);
    const int n = (int)(t / ih);
    const int r0 = max(0, (int)floorf((iy - 1) / sy) - 1), r1 = min(dy.h - 1, (int)ceilf((iy + 1) / sy) + 1);
    const int q0 = max(0, (int)floorf((ix - 1) / sx) - 1), q1 = min(dy.w - 1, (int)ceilf((ix + 1) / sx) + 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oh = r0; oh <= r1; ++oh) {
      const float wy = tap_w(oh, sy, ih, iy);
      if (wy == 0.f) continue;
      float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int ow = q0; ow <= q1; ++ow) {
        const float wx = tap_w(ow, sx, iw, ix);
        if (wx != 0.f) {
          float4 v;
          if constexpr (sizeof(TD) == 4) {
            v = *reinterpret_cast<const float4*>(
                reinterpret_cast<const float*>(dy.p) + (((long)n * dy.h + oh) * dy.w + ow) * dy.cs + dy.coff + c);
          } else {
            const uint2 u = *reinterpret_cast<const uint2*>(
                reinterpret_cast<const uint16_t*>(dy.p) + (((long)n * dy.h + oh) * dy.w + ow) * dy.cs + dy.coff + c);
            v = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                            __uint_as_float(u.y & 0xffff0000u));
          }
          row.x += wx * v.x;
          row.y += wx * v.y;
          row.z += wx * v.z;
          row.w += wx * v.w;
        }
      }
      acc.x += wy * row.x;
      acc.y += wy * row.y;
      acc.z += wy * row.z;
      acc.w += wy * row.w;
    }
    if constexpr (sizeof(TX) == 4) {
      *reinterpret_cast<float4*>(dx + ip * dy.c + c) = acc;
    } else {
      const uint2 u = make_uint2((uint32_t)f2bf(acc.x) | ((uint32_t)f2bf(acc.y) << 16),
                                 (uint32_t)f2bf(acc.z) | ((uint32_t)f2bf(acc.w) << 16));
      *reinterpret_cast<uint2*>(dx + ip * dy.c + c) = u;
    }
  }
}

// HWIO [3][3][cin][cout] -> the dgrad filter [3][3][cout][cin], spatially flipped
__global__ void flip_weights_kernel(const float* w, int cin, int cout, float* wt) {
  const long total = 9L * cin * cout;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % cout);
    const long r = i / cout;
    const int ci = (int)(r % cin);
    const int tap = (int)(r / cin);
    wt[((long)(8 - tap) * cout + co) * cin + ci] = w[i];
  }
}

// ---------------------------------------------------------------- Adam (tf.train.AdamOptimizer, train.py:302-304)
__global__ void adam_kernel(float* var, float* m, float* v, const float* grad, long n, float lr_t, float beta1,
                            float beta2, float eps, float grad_scale) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
    const float g = grad[i] * grad_scale;
    const float mi = m[i] + (g - m[i]) * (1.f - beta1);
    const float vi = v[i] + (g * g - v[i]) * (1.f - beta2);
    m[i] = mi;
    v[i] = vi;
    var[i] = var[i] - (mi * lr_t) / (sqrtf(vi) + eps);
  }
}

static long g_bn_vec = 1;  // vm_set_option "bn_vec": 0 = the per-channel BN backward forms (A/B)
static long g_resize_bwd_2x = 1;  // vm_set_option "resize_bwd_2x": 0 = the windowed-search kernels for 2x too (A/B)
static long g_relu_bias_vec = 1;  // vm_set_option "relu_bias_vec": 0 = the per-element relu / bias backward (A/B)
static long g_relu_bias_iters = 8;  // vm_set_option "relu_bias_iters": pixel iterations per thread of the 8-channel
                                    // form's grid (0 = bn_blocks' rule)

}  // namespace trn

// this file's vm_set_option keys (vm_common.h OptDef): every one takes any value
const OptDef train_options[] = {
    {"bn_vec", &trn::g_bn_vec, OPT_ANY},
    {"relu_bias_vec", &trn::g_relu_bias_vec, OPT_ANY},
    {"resize_bwd_2x", &trn::g_resize_bwd_2x, OPT_ANY},
    {"relu_bias_iters", &trn::g_relu_bias_iters, OPT_ANY},
    {nullptr},
};

}  // namespace vm

using namespace vm;
using namespace vm::trn;

extern "C" int vm_matting_loss_backward(const float* pred, const float* gt, const float* raw_fg, const float* bg,
                                        const float* cmp, long pixels, float* dlogits, void* stream) {
  if (!pred || !gt || !raw_fg || !bg || !cmp || !dlogits || pixels <= 0)
    return fail(VM_EINVAL, "matting_loss_backward: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(loss_backward_kernel, dim3(grid_for(pixels, 256)), dim3(256), 0, st, pred, gt, raw_fg, bg, cmp,
                     pixels, dlogits);
  return check_launch("matting_loss_backward");
}

extern "C" size_t vm_bn_backward_workspace_bytes(int channels) {
  return channels <= 0 ? 0 : (size_t)3 * bn_max_blocks(channels) * channels * sizeof(double) + (size_t)2 * channels * sizeof(float);
}

extern "C" int vm_bn_backward_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* y, const float* mean,
                                   const float* var, const float* gamma, float eps, vm_tensor* dx, float* dgamma,
                                   float* dbeta, void* work, void* stream) {
  return vm_bn_backward_ex_nhwc(x, dy, y, mean, var, gamma, eps, dx, nullptr, dgamma, dbeta, nullptr, work, stream);
}

extern "C" int vm_bn_backward_ex_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* y, const float* mean,
                                      const float* var, const float* gamma, float eps, vm_tensor* dx, vm_tensor* dx2,
                                      float* dgamma, float* dbeta, float* dbias, void* work, void* stream) {
  if (dx2 && (!dx || !ok_view(dx2) || !same_shape(dx2, dy)))
    return fail(VM_EINVAL, "bn_backward: dx2 needs dx and an [n,h,w,c] view");
  if (dbias && !x) return fail(VM_EINVAL, "bn_backward: dbias needs x");
  if (!ok_view(dy) || dy->dtype != VM_F32 || !work) return fail(VM_EINVAL, "bn_backward: bad dy / workspace");
  if (x && (!ok_view(x) || !same_shape(x, dy) || !mean || !var)) return fail(VM_EINVAL, "bn_backward: bad x");
  if (y && (!ok_view(y) || !same_shape(y, dy))) return fail(VM_EINVAL, "bn_backward: bad relu mask y");
  if (dx && (!x || !ok_view(dx) || !same_shape(dx, dy) || dx->dtype != VM_F32))
    return fail(VM_EINVAL, "bn_backward: dx needs x and an f32 [n,h,w,c] view");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  V xv{}, yv{}, dyv = mk(dy);
  if (x) xv = mk(x);
  if (y) yv = mk(y);
  const int C = dy->c;
  double* part = reinterpret_cast<double*>(work);
  // the two channel sums land in dbeta / dgamma when given, else in the float tail of the workspace
  float* tail = reinterpret_cast<float*>(part + 3L * bn_max_blocks(C) * C);
  float* sg = dbeta ? dbeta : tail;
  float* sgx = dgamma ? dgamma : tail + C;
  const long M = (long)dy->n * dy->h * dy->w;
  const int nb = bn_blocks(M, C);
  auto v16 = [](const vm_tensor* t) {
    return t->cstride % 8 == 0 && t->coff % 8 == 0 && reinterpret_cast<uintptr_t>(t->ptr) % 16 == 0;
  };
  const bool vec = g_bn_vec && x && x->dtype == VM_F32 && C % 8 == 0 && C <= 512 && v16(x) && v16(dy) &&
                   (!y || (y->dtype == VM_BF16 && v16(y))) && (!dx || v16(dx)) &&
                   (!dx2 || (dx2->dtype == VM_BF16 && v16(dx2)));
  Bn8 b8{};
  int tpg = 1;
  if (vec) {
    b8.x = reinterpret_cast<const float*>(x->ptr) + x->coff;
    b8.dy = reinterpret_cast<const float*>(dy->ptr) + dy->coff;
    b8.y = y ? reinterpret_cast<const uint16_t*>(y->ptr) + y->coff : nullptr;
    b8.dx = dx ? reinterpret_cast<float*>(dx->ptr) + dx->coff : nullptr;
    b8.dx2 = dx2 ? reinterpret_cast<uint16_t*>(dx2->ptr) + dx2->coff : nullptr;
    b8.xcs = x->cstride; b8.dycs = dy->cstride; b8.ycs = y ? y->cstride : 0;
    b8.dxcs = dx ? dx->cstride : 0; b8.dx2cs = dx2 ? dx2->cstride : 0;
    b8.C = C; b8.M = M;
    tpg = lanes_for(C / 8);
#define VM_BP8(TPG)                                                                                                   \
  case TPG:                                                                                                           \
    if (y) hipLaunchKernelGGL((bn_bwd_partial8<true, TPG>), dim3(nb), dim3(256), 0, st, b8, mean, var, eps, part, nb); \
    else hipLaunchKernelGGL((bn_bwd_partial8<false, TPG>), dim3(nb), dim3(256), 0, st, b8, mean, var, eps, part, nb); \
    break;
    switch (tpg) { VM_BP8(1) VM_BP8(2) VM_BP8(4) VM_BP8(8) VM_BP8(16) VM_BP8(32) VM_BP8(64) }
#undef VM_BP8
  } else if (y) {
    launch_bn_bwd_partial<true>(xv, dyv, yv, mean, var, eps, part, nb, st);
  } else {
    launch_bn_bwd_partial<false>(xv, dyv, yv, mean, var, eps, part, nb, st);
  }
  int rc = check_launch("bn_backward_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_bwd_final, dim3(C), dim3(256), 0, st, part, nb, C, sg, x ? sgx : nullptr, dbias, gamma, var,
                     eps, M);
  rc = check_launch("bn_backward_final");
  if (rc || !dx) return rc;
  if (vec) {
    const long px = (M + 256 / tpg - 1) / (256 / tpg);
    const dim3 g8((unsigned)(px < 4096 ? px : 4096));
#define VM_BA8(TPG)                                                                                                  \
  case TPG:                                                                                                          \
    if (y && dx2) hipLaunchKernelGGL((bn_bwd_apply8<true, true, TPG>), g8, dim3(256), 0, st, b8, mean, var, gamma,   \
                                     eps, sg, sgx);                                                                  \
    else if (y) hipLaunchKernelGGL((bn_bwd_apply8<true, false, TPG>), g8, dim3(256), 0, st, b8, mean, var, gamma,    \
                                   eps, sg, sgx);                                                                    \
    else if (dx2) hipLaunchKernelGGL((bn_bwd_apply8<false, true, TPG>), g8, dim3(256), 0, st, b8, mean, var, gamma,  \
                                     eps, sg, sgx);                                                                  \
    else hipLaunchKernelGGL((bn_bwd_apply8<false, false, TPG>), g8, dim3(256), 0, st, b8, mean, var, gamma, eps, sg, \
                            sgx);                                                                                    \
    break;
    switch (tpg) { VM_BA8(1) VM_BA8(2) VM_BA8(4) VM_BA8(8) VM_BA8(16) VM_BA8(32) VM_BA8(64) }
#undef VM_BA8
    return check_launch("bn_backward_apply");
  }
  if (!y && !dx2 && f32_pair(x) && f32_pair(dy) && f32_pair(dx) && x->cstride > 0) {
    hipLaunchKernelGGL(bn_bwd_apply2_f32, dim3(grid_for(M, 256)), dim3(256), 0, st,
                       reinterpret_cast<const float*>(x->ptr) + x->coff, x->cstride,
                       reinterpret_cast<const float*>(dy->ptr) + dy->coff, dy->cstride,
                       reinterpret_cast<float*>(dx->ptr) + dx->coff, dx->cstride, M, mean, var, gamma, eps, sg, sgx);
    return check_launch("bn_backward_apply");
  }
  const int cp = lanes_for(C);
  const dim3 grid = lanes_grid(M, C, cp);
  const V dxv = mk(dx), dx2v = dx2 ? mk(dx2) : V{};
#define VM_BNA(CP)                                                                                                    \
  if (y) hipLaunchKernelGGL((bn_bwd_apply<true, CP>), grid, dim3(256), 0, st, xv, dyv, yv, mean, var, gamma, eps, sg, \
                            sgx, dxv, dx2v);                                                                          \
  else hipLaunchKernelGGL((bn_bwd_apply<false, CP>), grid, dim3(256), 0, st, xv, dyv, yv, mean, var, gamma, eps, sg,  \
                          sgx, dxv, dx2v)
  VM_CP_SWITCH(cp, VM_BNA)
#undef VM_BNA
  return check_launch("bn_backward_apply");
}

extern "C" int vm_bn_backward_apply_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* y,
                                         const float* mean, const float* var, const float* gamma, float eps,
                                         const float* sum_g, const float* sum_gx, long count, vm_tensor* dx,
                                         vm_tensor* dx2, void* stream) {
  if (!ok_view(x) || !ok_view(dy) || dy->dtype != VM_F32 || !same_shape(x, dy) || !mean || !var || !sum_g ||
      !sum_gx || count <= 0 || !dx || !ok_view(dx) || !same_shape(dx, dy) || dx->dtype != VM_F32 ||
      (y && (!ok_view(y) || !same_shape(y, dy))) || (dx2 && (!ok_view(dx2) || !same_shape(dx2, dy))))
    return fail(VM_EINVAL, "bn_backward_apply: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long M = (long)dy->n * dy->h * dy->w;
  const V xv = mk(x), dyv = mk(dy), yv = y ? mk(y) : V{}, dxv = mk(dx), dx2v = dx2 ? mk(dx2) : V{};
  const int cp = lanes_for(dy->c);
  const dim3 grid = lanes_grid(M, dy->c, cp);
#define VM_BNA(CP)                                                                                                    \
  if (y) hipLaunchKernelGGL((bn_bwd_apply<true, CP>), grid, dim3(256), 0, st, xv, dyv, yv, mean, var, gamma, eps,     \
                            sum_g, sum_gx, dxv, dx2v, count);                                                         \
  else hipLaunchKernelGGL((bn_bwd_apply<false, CP>), grid, dim3(256), 0, st, xv, dyv, yv, mean, var, gamma, eps,      \
                          sum_g, sum_gx, dxv, dx2v, count)
  VM_CP_SWITCH(cp, VM_BNA)
#undef VM_BNA
  return check_launch("bn_backward_apply");
}

extern "C" int vm_relu_backward_nhwc(const vm_tensor* dy, const vm_tensor* y, vm_tensor* dx, void* stream) {
  return vm_relu_backward_ex_nhwc(dy, y, dx, nullptr, stream);
}

extern "C" int vm_relu_backward_ex_nhwc(const vm_tensor* dy, const vm_tensor* y, vm_tensor* dx, vm_tensor* dx2,
                                        void* stream) {
  return vm_relu_backward_split_nhwc(dy, y, 0, nullptr, dx, dx2, stream);
}

extern "C" int vm_relu_backward_split_nhwc(const vm_tensor* dy, const vm_tensor* y, int split, vm_tensor* dx_lo,
                                           vm_tensor* dx, vm_tensor* dx2, void* stream) {
  if (!ok_view(dy) || !ok_view(y) || !same_shape(dy, y) || split < 0 || split >= dy->c)
    return fail(VM_EINVAL, "relu_backward: bad tensors");
  auto part_ok = [&](const vm_tensor* t, int c) {
    return ok_view(t) && t->n == dy->n && t->h == dy->h && t->w == dy->w && t->c == c;
  };
  if (!part_ok(dx, dy->c - split) || (dx2 && !part_ok(dx2, dy->c - split)) || (split > 0 && !(dx_lo && part_ok(dx_lo, split))))
    return fail(VM_EINVAL, "relu_backward: outputs must be [n,h,w,%d] (dx, dx2) and [n,h,w,%d] (dx_lo)",
                dy->c - split, split);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long M = (long)dy->n * dy->h * dy->w;
  const int cp = lanes_for(dy->c);
  const dim3 grid = lanes_grid(M, dy->c, cp);
  const V a = mk(dy), b = mk(y), c = mk(dx), d = dx2 ? mk(dx2) : V{}, e = split > 0 ? mk(dx_lo) : V{};
#define VM_RB(CP) hipLaunchKernelGGL((relu_bwd_kernel<CP>), grid, dim3(256), 0, st, a, b, c, d, e, split)
  VM_CP_SWITCH(cp, VM_RB)
#undef VM_RB
  return check_launch("relu_backward");
}

extern "C" int vm_maxpool2x2_backward_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* add, vm_tensor* dx,
                                           void* stream) {
  if (!ok_view(x) || !ok_view(dy) || !ok_view(dx) || !same_shape(x, dx) || (add && (!ok_view(add) || !same_shape(add, x))))
    return fail(VM_EINVAL, "maxpool_backward: bad tensors");
  if (dy->n != x->n || dy->h != (x->h + 1) / 2 || dy->w != (x->w + 1) / 2 || dy->c != x->c)
    return fail(VM_EINVAL, "maxpool_backward: dy must be [%d,%d,%d,%d]", x->n, (x->h + 1) / 2, (x->w + 1) / 2, x->c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long M = (long)x->n * x->h * x->w;
  const int cp = lanes_for(x->c);
  const dim3 grid = lanes_grid(M, x->c, cp);
  const V a = mk(x), b = mk(dy), c = add ? mk(add) : V{}, d = mk(dx);
#define VM_MPB(CP) hipLaunchKernelGGL((maxpool_bwd_kernel<CP>), grid, dim3(256), 0, st, a, b, c, d)
  VM_CP_SWITCH(cp, VM_MPB)
#undef VM_MPB
  return check_launch("maxpool_backward");
}


extern "C" size_t vm_relu_backward_bias_workspace_bytes(int channels) {
  return channels <= 0 ? 0 : (size_t)bn_max_blocks(channels) * channels * sizeof(double);
}

extern "C" int vm_relu_backward_bias_nhwc(const vm_tensor* dy, const vm_tensor* y, const vm_tensor* add,
                                          vm_tensor* dz, float* dbias, void* work, void* stream) {
  if (!ok_view(dy) || !ok_view(y) || !ok_view(dz) || (add && !ok_view(add)) || !dbias || !work)
    return fail(VM_EINVAL, "relu_backward_bias: bad argument");
  if (!same_shape(dz, y) || (add && !same_shape(add, y)) || dy->n != y->n || dy->c != y->c)
    return fail(VM_EINVAL, "relu_backward_bias: dz and add shaped like y");
  const bool pool = !(dy->h == y->h && dy->w == y->w);
  if (pool && (dy->h != (y->h + 1) / 2 || dy->w != (y->w + 1) / 2))
    return fail(VM_EINVAL, "relu_backward_bias: dy must be y's shape or its 2x2 SAME pool's");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int C = y->c;
  const long units = pool ? (long)dy->n * dy->h * dy->w : (long)y->n * y->h * y->w;
  auto al16 = [](const vm_tensor* t, int es) {  // every 8-channel run of the view 16-byte aligned
    return t->cstride % 8 == 0 && t->coff % 8 == 0 && reinterpret_cast<uintptr_t>(t->ptr) % 16 == 0 && es > 0;
  };
  if (g_relu_bias_vec && y->dtype == VM_BF16 && dz->dtype == VM_BF16 && C % 8 == 0 && C <= 512 && al16(y, 2) &&
      al16(dz, 2) && al16(dy, 4) && (!add || al16(add, 4))) {
    const int tpg = lanes_for(C / 8);
    // every block covers all C channels of 256 / tpg pixels per iteration: size the grid for ~g_relu_bias_iters
    // iterations per thread (bn_blocks' per-channel-group rule left the 512-channel levels at 12-50 blocks)
    int nb = bn_blocks(pool ? 4 * units : units, C);
    if (g_relu_bias_iters > 0) {
      const long want = (pool ? 4 * units : units) / ((256 / tpg) * g_relu_bias_iters);
      nb = (int)std::max(1L, std::min<long>(want, bn_max_blocks(C)));
    }
    const uint16_t* yp = reinterpret_cast<const uint16_t*>(y->ptr) + y->coff;
    uint16_t* zp = reinterpret_cast<uint16_t*>(dz->ptr) + dz->coff;
    double* part = reinterpret_cast<double*>(work);
    auto go = [&](auto dyt, auto at) {  // dy / add element types
      using TD = decltype(dyt);
      using TA = decltype(at);
      const TD* dyp = reinterpret_cast<const TD*>(dy->ptr) + dy->coff;
      const TA* ap = add ? reinterpret_cast<const TA*>(add->ptr) + add->coff : nullptr;
      const int acs = add ? add->cstride : 0;
#define VM_RB8(TPG)                                                                                                  \
  case TPG:                                                                                                          \
    if (pool && add)                                                                                                 \
      hipLaunchKernelGGL((relu_bwd_bias8_kernel<true, true, TPG, TD, TA>), dim3(nb), dim3(256), 0, st, dyp,          \
                         dy->cstride, yp, y->cstride, ap, acs, zp, dz->cstride, y->n, y->h, y->w, dy->h, dy->w, C,   \
                         part, nb);                                                                                  \
    else if (pool)                                                                                                   \
      hipLaunchKernelGGL((relu_bwd_bias8_kernel<true, false, TPG, TD, TA>), dim3(nb), dim3(256), 0, st, dyp,         \
                         dy->cstride, yp, y->cstride, ap, acs, zp, dz->cstride, y->n, y->h, y->w, dy->h, dy->w, C,   \
                         part, nb);                                                                                  \
    else if (add)                                                                                                    \
      hipLaunchKernelGGL((relu_bwd_bias8_kernel<false, true, TPG, TD, TA>), dim3(nb), dim3(256), 0, st, dyp,         \
                         dy->cstride, yp, y->cstride, ap, acs, zp, dz->cstride, y->n, y->h, y->w, dy->h, dy->w, C,   \
                         part, nb);                                                                                  \
    else                                                                                                             \
      hipLaunchKernelGGL((relu_bwd_bias8_kernel<false, false, TPG, TD, TA>), dim3(nb), dim3(256), 0, st, dyp,        \
                         dy->cstride, yp, y->cstride, ap, acs, zp, dz->cstride, y->n, y->h, y->w, dy->h, dy->w, C,   \
                         part, nb);                                                                                  \
    break;
      switch (tpg) { VM_RB8(1) VM_RB8(2) VM_RB8(4) VM_RB8(8) VM_RB8(16) VM_RB8(32) VM_RB8(64) }
#undef VM_RB8
    };
    const bool dyb = dy->dtype == VM_BF16, ab = add && add->dtype == VM_BF16;
    if (dyb && ab) go(uint16_t{}, uint16_t{});
    else if (dyb) go(uint16_t{}, float{});
    else if (ab) go(float{}, uint16_t{});
    else go(float{}, float{});
    int rc = check_launch("relu_backward_bias");
    if (rc) return rc;
    hipLaunchKernelGGL(fold_sum_kernel, dim3(C), dim3(256), 0, st, part, nb, C, dbias);
    return check_launch("relu_backward_bias fold");
  }
  const int nb = bn_blocks(pool ? 4 * units : units, C);
  const int cp = lanes_for(C);
  const dim3 grid(cp == 64 ? (C + 63) / 64 : 1, nb);
  V a = mk(dy), b = mk(y), c = add ? mk(add) : V{}, d = mk(dz);
  double* part = reinterpret_cast<double*>(work);
#define VM_RBB(CP)                                                                                           \
  if (pool) hipLaunchKernelGGL((relu_bwd_bias_kernel<true, CP>), grid, dim3(256), 0, st, a, b, c, d, part, nb); \
  else hipLaunchKernelGGL((relu_bwd_bias_kernel<false, CP>), grid, dim3(256), 0, st, a, b, c, d, part, nb)
  VM_CP_SWITCH(cp, VM_RBB)
#undef VM_RBB
  int rc = check_launch("relu_backward_bias");
  if (rc) return rc;
  hipLaunchKernelGGL(fold_sum_kernel, dim3(C), dim3(256), 0, st, part, nb, C, dbias);
  return check_launch("relu_backward_bias fold");
}

// Exact 2x upsampling (oh = 2 ih, ow = 2 iw: scale 0.5, the UNet decoders' every resize): the TF-1 taps are known in
// closed form — output o takes input o/2 with weight 1 when o is even; lo = (o-1)/2 and hi = min(lo + 1, in - 1) with
// 0.5 each when odd (1.0 on the last input, where hi = lo) — so input i collects output rows 2i-1, 2i, 2i+1 (weights
// 0.5, 1, 0.5 or 1 on the last) and the same columns.  Only resize_bwd_kernel's nonzero terms, in its order (rows
// ascending, columns ascending within a row, row = sum of wx * v from 0, acc = sum of wy * row from 0), and every
// product is exact (weights 0.5 / 1), so the sums are bit-identical to the windowed search's.  A lane takes 8 channels
// of one input pixel: 9 16-byte (bf16) or 2x16-byte (f32) loads, one 16-byte / 2x16-byte store.
template <typename TD, typename TX>
__global__ __launch_bounds__(256) void resize2x_bwd_kernel8(V dy, TX* __restrict__ dx, int ih, int iw) {
  const int C8 = dy.c / 8;
  const long total = (long)dy.n * ih * iw * C8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C8) * 8;
    const long ip = i / C8;
    const int ix = (int)(ip % iw);
    const long t = ip / iw;
    const int iy = (int)(t % ih);
    const int n = (int)(t / ih);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int oh = 2 * iy - 1 + r;
      if (oh < 0) continue;
      const float wy = r == 1 ? 1.f : (r == 2 && iy == ih - 1) ? 1.f : 0.5f;
      float row[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int ow = 2 * ix - 1 + q;
        if (ow < 0) continue;
        const float wx = q == 1 ? 1.f : (q == 2 && ix == iw - 1) ? 1.f : 0.5f;
        const long off = (((long)n * dy.h + oh) * dy.w + ow) * dy.cs + dy.coff + c;
        float v[8];
        if constexpr (sizeof(TD) == 4) {
          const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(dy.p) + off);
          const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(dy.p) + off + 4);
          v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
          const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(dy.p) + off);
          const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            v[2 * k] = __uint_as_float(w4[k] << 16);
            v[2 * k + 1] = __uint_as_float(w4[k] & 0xffff0000u);
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] += wx * v[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += wy * row[k];
    }
    TX* o = dx + ip * dy.c + c;
    if constexpr (sizeof(TX) == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
      uint32_t w4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w4[k] = (uint32_t)f2bf(acc[2 * k]) | ((uint32_t)f2bf(acc[2 * k + 1]) << 16);
      *reinterpret_cast<uint4*>(o) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
  }
}

// the exact-2x form when it applies (dy 2x dx, c % 8 == 0, 16-byte aligned); false = not launched
static bool resize2x_bwd(const vm_tensor* dy, void* dx, bool dx_bf16, int ih, int iw, hipStream_t st) {
  if (!g_resize_bwd_2x || dy->h != 2 * ih || dy->w != 2 * iw || dy->c % 8 || dy->cstride % 8 || dy->coff % 8 ||
      reinterpret_cast<uintptr_t>(dy->ptr) % 16 || reinterpret_cast<uintptr_t>(dx) % 16)
    return false;
  const long n8 = (long)dy->n * ih * iw * (dy->c / 8);
  const dim3 g(grid_for(n8, 256, 256 * 64)), b(256);
  if (dy->dtype == VM_F32 && !dx_bf16)
    hipLaunchKernelGGL((resize2x_bwd_kernel8<float, float>), g, b, 0, st, mk(dy), (float*)dx, ih, iw);
  else if (dy->dtype == VM_F32)
    hipLaunchKernelGGL((resize2x_bwd_kernel8<float, uint16_t>), g, b, 0, st, mk(dy), (uint16_t*)dx, ih, iw);
  else if (!dx_bf16)
    hipLaunchKernelGGL((resize2x_bwd_kernel8<uint16_t, float>), g, b, 0, st, mk(dy), (float*)dx, ih, iw);
  else
    hipLaunchKernelGGL((resize2x_bwd_kernel8<uint16_t, uint16_t>), g, b, 0, st, mk(dy), (uint16_t*)dx, ih, iw);
  return true;
}

extern "C" int vm_resize_bilinear_tf1_backward(const vm_tensor* dy, float* dx, int ih, int iw, void* stream) {
  if (!ok_view(dy) || !dx || ih <= 0 || iw <= 0) return fail(VM_EINVAL, "resize_backward: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dy->h > 4 * ih || dy->w > 4 * iw || ih > 2 * dy->h || iw > 2 * dy->w)
    return fail(VM_EUNSUPPORTED, "resize_backward: scale %dx%d -> %dx%d outside the upsampling range", ih, iw, dy->h,
                dy->w);
  const float sy = (float)ih / (float)dy->h, sx = (float)iw / (float)dy->w;
  if (resize2x_bwd(dy, dx, false, ih, iw, st)) return check_launch("resize_backward");
  if (dy->c % 4 == 0 && dy->cstride % 4 == 0 && dy->coff % 4 == 0 && reinterpret_cast<uintptr_t>(dy->ptr) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(dx) % 16 == 0) {
    const long n4 = (long)dy->n * ih * iw * (dy->c / 4);
    if (dy->dtype == VM_F32)
      hipLaunchKernelGGL(resize_bwd_kernel4<float>, dim3(grid_for(n4, 256)), dim3(256), 0, st, mk(dy), dx, ih, iw, sy,
                         sx);
    else
      hipLaunchKernelGGL(resize_bwd_kernel4<uint16_t>, dim3(grid_for(n4, 256)), dim3(256), 0, st, mk(dy), dx, ih, iw,
                         sy, sx);
    return check_launch("resize_backward");
  }
  const long n = (long)dy->n * ih * iw * dy->c;
  hipLaunchKernelGGL(resize_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, mk(dy), dx, ih, iw, sy, sx);
  return check_launch("resize_backward");
}

// dx as a view: f32 as above, or dense bf16 with c % 4 == 0 and 8-byte aligned (the bf16 training path's relu
// gradients: the relu backward rounds dz to bf16 anyway, so a bf16 dx changes no dz where no `add` joins it)
extern "C" int vm_resize_bilinear_tf1_backward_nhwc(const vm_tensor* dy, vm_tensor* dx, void* stream) {
  if (!ok_view(dy) || !ok_view(dx) || dx->n != dy->n || dx->c != dy->c)
    return fail(VM_EINVAL, "resize_backward: dx [n,ih,iw,c] with dy's n and c");
  if (dx->cstride != dx->c || dx->coff != 0) return fail(VM_EUNSUPPORTED, "resize_backward: dx must be dense");
  if (dx->dtype == VM_F32) return vm_resize_bilinear_tf1_backward(dy, reinterpret_cast<float*>(dx->ptr), dx->h, dx->w,
                                                                  stream);
  const int ih = dx->h, iw = dx->w;
  if (dy->h > 4 * ih || dy->w > 4 * iw || ih > 2 * dy->h || iw > 2 * dy->w)
    return fail(VM_EUNSUPPORTED, "resize_backward: scale %dx%d -> %dx%d outside the upsampling range", ih, iw, dy->h,
                dy->w);
  if (dy->c % 4 || dy->cstride % 4 || dy->coff % 4 || reinterpret_cast<uintptr_t>(dy->ptr) % 16 ||
      reinterpret_cast<uintptr_t>(dx->ptr) % 8)
    return fail(VM_EUNSUPPORTED, "resize_backward: bf16 dx needs c %% 4 == 0 and aligned views");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (resize2x_bwd(dy, dx->ptr, true, ih, iw, st)) return check_launch("resize_backward");
  const float sy = (float)ih / (float)dy->h, sx = (float)iw / (float)dy->w;
  const long n4 = (long)dy->n * ih * iw * (dy->c / 4);
  uint16_t* d = reinterpret_cast<uint16_t*>(dx->ptr);
  if (dy->dtype == VM_F32)
    hipLaunchKernelGGL((resize_bwd_kernel4<float, uint16_t>), dim3(grid_for(n4, 256)), dim3(256), 0, st, mk(dy), d, ih,
                       iw, sy, sx);
  else
    hipLaunchKernelGGL((resize_bwd_kernel4<uint16_t, uint16_t>), dim3(grid_for(n4, 256)), dim3(256), 0, st, mk(dy), d,
                       ih, iw, sy, sx);
  return check_launch("resize_backward");
}

extern "C" int vm_conv3x3_flip_weights(const float* w_hwio, int cin, int cout, float* w_flipped, void* stream) {
  if (!w_hwio || !w_flipped || cin <= 0 || cout <= 0) return fail(VM_EINVAL, "flip_weights: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(flip_weights_kernel, dim3(grid_for(9L * cin * cout, 256)), dim3(256), 0, st, w_hwio, cin, cout,
                     w_flipped);
  return check_launch("flip_weights");
}

extern "C" int vm_adam_tf(float* var, float* m, float* v, const float* grad, long n, float lr_t, float beta1,
                          float beta2, float eps, float grad_scale, void* stream) {
  if (!var || !m || !v || !grad || n <= 0) return fail(VM_EINVAL, "adam: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, var, m, v, grad, n, lr_t, beta1, beta2,
                     eps, grad_scale);
  return check_launch("adam");
}
