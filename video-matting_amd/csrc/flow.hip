// Two-frame temporal path: optical-flow backward warp (flow.warp_img / warp_bgr) and the
// forward/backward consistency mask (flow.correct_alpha).  Gather-bound: one thread per output
// pixel, coalesced reads of the flow field and the output, L2-served bilinear taps.

#include "vm_common.h"

namespace vm {

// cv2.remap(img, identity+flow (CV_32FC2), None, INTER_LINEAR), BORDER_CONSTANT 0 (flow.py:12-18).
// mode 0 (OpenCV): X = cvRound(x*32) (round-half-even), integer X>>5, fraction (X&31)/32, weights from
// the 32x32 table (exact products of k/32), taps summed TL,TR,BL,BR; a tap outside the frame reads 0.
// mode 1: exact bilinear on the float coordinate.
__global__ void remap_f32_kernel(const float* __restrict__ img, int ih, int iw, const float* __restrict__ flow, int h,
                                 int w, int nfr, float* __restrict__ out, int mode) {
  const long per = (long)h * w;
  const long total = per * nfr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long f = i / per;
    const long pi = i - f * per;
    const int y = (int)(pi / w), x = (int)(pi - (long)y * w);
    const float2 fl = reinterpret_cast<const float2*>(flow)[i];
    const float mx = (float)x + fl.x;  // (identity + flow).astype(float32): one rounding
    const float my = (float)y + fl.y;
    int x0, y0;
    float fx, fy;
    if (mode == 0) {
      const int X = (int)rintf(mx * 32.f);
      const int Y = (int)rintf(my * 32.f);
      x0 = X >> 5;
      y0 = Y >> 5;
      fx = (float)(X & 31) * (1.f / 32.f);
      fy = (float)(Y & 31) * (1.f / 32.f);
    } else {
      const float flx = floorf(mx), fly = floorf(my);
      x0 = (int)flx;
      y0 = (int)fly;
      fx = mx - flx;
      fy = my - fly;
    }
    const float* im = img + f * (long)ih * iw;
    auto tap = [&](int yy, int xx) -> float {
      return ((unsigned)yy < (unsigned)ih && (unsigned)xx < (unsigned)iw) ? im[(long)yy * iw + xx] : 0.f;
    };
    const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
    float s = tap(y0, x0) * w00;
    s += tap(y0, x0 + 1) * w01;
    s += tap(y0 + 1, x0) * w10;
    s += tap(y0 + 1, x0 + 1) * w11;
    out[i] = s;
  }
}

// uint8 planes (flow.py:29-31): 15-bit integer weights (32-fy)(32-fx)*32 etc. (exact), (sum + 2^14) >> 15.
__global__ void remap_u8_kernel(const uint8_t* __restrict__ img, int ih, int iw, int cn, const float* __restrict__ flow,
                                int h, int w, uint8_t* __restrict__ out) {
  const long total = (long)h * w;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    const float2 fl = reinterpret_cast<const float2*>(flow)[i];
    const int X = (int)rintf(((float)x + fl.x) * 32.f);
    const int Y = (int)rintf(((float)y + fl.y) * 32.f);
    const int x0 = X >> 5, y0 = Y >> 5, ax = X & 31, ay = Y & 31;
    const int w00 = (32 - ay) * (32 - ax) * 32, w01 = (32 - ay) * ax * 32, w10 = ay * (32 - ax) * 32, w11 = ay * ax * 32;
    for (int k = 0; k < cn; ++k) {
      auto tap = [&](int yy, int xx) -> int {
        return ((unsigned)yy < (unsigned)ih && (unsigned)xx < (unsigned)iw) ? (int)img[((long)yy * iw + xx) * cn + k] : 0;
      };
      const int s = tap(y0, x0) * w00 + tap(y0, x0 + 1) * w01 + tap(y0 + 1, x0) * w10 + tap(y0 + 1, x0 + 1) * w11;
      int v = (s + (1 << 14)) >> 15;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      out[i * cn + k] = (uint8_t)v;
    }
  }
}

// flow.correct_alpha (flow.py:41-50): j0 = min(int(bw[i,j,0] + j), w-1), i0 = min(int(bw[i,j,1] + i), h-1)
// (int() truncates toward 0; negative indices wrap numpy-style, below -dim the reference raises IndexError);
// (j1, i1) the same through fw[i0, j0]; alpha[i,j] = 0 where ||(i1 - i, j1 - j)|| > thresh.
template <int PROMOTE>
__device__ __forceinline__ long step_index(float u, long base, long lim) {
  long t;
  if (PROMOTE == 0) t = (long)((double)u + (double)base);  // numpy-1: float64, exact
  else t = (long)(u + (float)base);                         // numpy-2: float32 add
  return t < lim - 1 ? t : lim - 1;
}

// Pass 1 only validates the indices; pass 2 returns early when pass 1 flagged an IndexError, so on
// error alpha is left untouched — as in the reference, where the exception escapes the loop before
// the masked assignment (flow.py:41-50).
template <int PROMOTE>
__global__ void fb_check_kernel(const float* __restrict__ bw, int h, int w, int* err) {
  const long total = (long)h * w;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), c = (int)(i - (long)r * w);
    const float2 b = reinterpret_cast<const float2*>(bw)[i];
    const long j0 = step_index<PROMOTE>(b.x, c, w);
    const long i0 = step_index<PROMOTE>(b.y, r, h);
    if (j0 < -(long)w || i0 < -(long)h) atomicOr(err, 1);
  }
}

template <int PROMOTE>
__global__ void fb_consistency_kernel(const float* __restrict__ bw, const float* __restrict__ fw, int h, int w,
                                      float* __restrict__ alpha, double thresh, const int* err) {
  if (*err) return;
  const long total = (long)h * w;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / w), c = (int)(i - (long)r * w);
    const float2 b = reinterpret_cast<const float2*>(bw)[i];
    const long j0 = step_index<PROMOTE>(b.x, c, w);
    const long i0 = step_index<PROMOTE>(b.y, r, h);
    const long ji = j0 < 0 ? j0 + w : j0, ii = i0 < 0 ? i0 + h : i0;  // numpy negative-index wrap
    const float2 f = reinterpret_cast<const float2*>(fw)[ii * w + ji];
    const long j1 = step_index<PROMOTE>(f.x, j0, w);
    const long i1 = step_index<PROMOTE>(f.y, i0, h);
    const double di = (double)(i1 - r), dj = (double)(j1 - c);
    if (sqrt(di * di + dj * dj) > thresh) alpha[i] = 0.f;
  }
}

// ---------------------------------------------------------------- the per-pixel pieces of the fused kernels
// warp_img at output pixel (x, y) of one [h,w] frame: remap_f32_kernel's mode-0 expressions (cv2.remap's 1/32-pixel
// fixed point, taps outside the frame read 0, summed TL, TR, BL, BR), so the value is bit-identical to that kernel's.
__device__ __forceinline__ float warp_fixed(const float* __restrict__ prev, int h, int w, int x, int y, float2 fl) {
  const int X = (int)rintf(((float)x + fl.x) * 32.f);
  const int Y = (int)rintf(((float)y + fl.y) * 32.f);
  const int x0 = X >> 5, y0 = Y >> 5;
  const float fx = (float)(X & 31) * (1.f / 32.f), fy = (float)(Y & 31) * (1.f / 32.f);
  auto tap = [&](int yy, int xx) -> float {
    return ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) ? prev[(long)yy * w + xx] : 0.f;
  };
  const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
  float a = tap(y0, x0) * w00;
  a += tap(y0, x0 + 1) * w01;
  a += tap(y0 + 1, x0) * w10;
  a += tap(y0 + 1, x0 + 1) * w11;
  return a;
}

// correct_alpha at pixel (x, y) (fb_check_kernel + fb_consistency_kernel): true where the forward/backward round trip
// misses by more than thresh; raises *err (and returns false) where the reference raises IndexError.
template <int PROMOTE>
__device__ __forceinline__ bool fb_occluded(float2 fl, const float* __restrict__ fw, int h, int w, int x, int y,
                                            double thresh, int* err) {
  const long j0 = step_index<PROMOTE>(fl.x, x, w);
  const long i0 = step_index<PROMOTE>(fl.y, y, h);
  if (j0 < -(long)w || i0 < -(long)h) {
    atomicOr(err, 1);
    return false;
  }
  const long ji = j0 < 0 ? j0 + w : j0, ii = i0 < 0 ? i0 + h : i0;
  const float2 f = reinterpret_cast<const float2*>(fw)[ii * w + ji];
  const long j1 = step_index<PROMOTE>(f.x, j0, w);
  const long i1 = step_index<PROMOTE>(f.y, i0, h);
  const double di = (double)(i1 - y), dj = (double)(j1 - x);
  return sqrt(di * di + dj * dj) > thresh;
}

// ---------------------------------------------------------------- config 3: warp + occlusion + refine input
// One pass per pixel of the two-frame chain flow.py's demo runs (flow.py:69-77): alpha_w = warp_img(prev, flow_b)
// (the remap_f32 mode-0 arithmetic above), correct_alpha(flow_b, flow_f, alpha_w) (fb_consistency above: one
// gather of flow_f at the backward target), and the RefineNet input row [cmp B,G,R, alpha_t, alpha_w, 0, 0, 0]
// (refine.py:27, Cin = 5 padded to 8, the concat of SURVEY.md 8(a) a14) written as one 16- or 32-byte NHWC pixel.
// Every value is bit-identical to the separate kernels; the IndexError flag is raised as in fb_check (the caller
// raises before using the output).
template <typename T, int PROMOTE>
__global__ __launch_bounds__(256) void temporal_input_kernel(const float* __restrict__ prev,
                                                             const float* __restrict__ bw,
                                                             const float* __restrict__ fw,
                                                             const float* __restrict__ cmp,
                                                             const float* __restrict__ cur, int h, int w,
                                                             double thresh, T* __restrict__ out,
                                                             float* __restrict__ warped, int* err) {
  const long total = (long)h * w;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    const float2 fl = reinterpret_cast<const float2*>(bw)[i];
    float a = warp_fixed(prev, h, w, x, y, fl);                          // warp_img (remap_f32_kernel, mode 0)
    if (fb_occluded<PROMOTE>(fl, fw, h, w, x, y, thresh, err)) a = 0.f;  // correct_alpha (fb_consistency_kernel)
    if (warped) warped[i] = a;
    float v[8] = {cmp[i * 3], cmp[i * 3 + 1], cmp[i * 3 + 2], cur[i], a, 0.f, 0.f, 0.f};
    if constexpr (sizeof(T) == 2) {
      reinterpret_cast<uint4*>(out)[i] = Chunk<T>::pack(v);
    } else {
      reinterpret_cast<float4*>(out)[2 * i] = make_float4(v[0], v[1], v[2], v[3]);
      reinterpret_cast<float4*>(out)[2 * i + 1] = make_float4(v[4], 0.f, 0.f, 0.f);
    }
  }
}

// ---------------------------------------------------------------- the video model's feed (vm_clip_feed)
// One pass per pixel of everything UNetSimple reads for alpha[t] = model(cmp[t], bg[t], warp_img(alpha[t-1], backward[t])):
// the uint8 feed of cmp and bg (vm_frames_from_u8's values), the warped (and optionally occlusion-corrected) previous
// matte, the three towers' 8-channel input pixels and the 9-channel concat the level-0 select conv reads.  Traffic per
// pixel: 6 B of uint8 + 8 B of flow (+ 8 B gathered forward flow) in, the 4 taps of the previous matte from L2, and
// 3 x 16 + 32 B (bf16) or 3 x 32 + 64 B (f32) out.  One thread per pixel: every store instruction of a wave then covers
// 64 adjacent pixels (1 KB of a tower, whole 16-byte chunks per lane), and the byte loads of the uint8 planes coalesce
// across the wave whatever the planes' alignment.  A form with 4 pixels per thread and dword loads of the planes, as
// vm_frames_from_u8 has, measured 0.131 ms against 0.080 ms at 1080x1920: its stores are 16 bytes at a 64-byte lane
// stride, and with 80 B written for 14 B read the stores decide.
struct ClipFeedArgs {
  const uint8_t* cmp;
  const uint8_t* bg;
  const float* prev;  // [n,h,w]
  const float* bw;    // [n,h,w,2]
  const float* fw;    // [n,h,w,2] (OCC != 0)
  void* towers;       // [3n,h,w,8]
  void* cat;          // [n,h,w,cat_stride]
  float* warped;      // [n,h,w] or null
  int* err;
  long total;         // n * h * w
  long hw;
  int h, w;
  int bg_bcast;       // 1: bg is one [h,w,3] plate
  int cat_stride;     // elements per pixel of cat
  double thresh;
};

// the third tower's value at global pixel `pix`.  OCC: 0 = warp only, 1 / 2 = correct_alpha with promote 0 / 1
template <int OCC>
__device__ __forceinline__ float feed_alpha(const ClipFeedArgs& a, long pix) {
  const long f = pix / a.hw;
  const long pi = pix - f * a.hw;
  const int y = (int)(pi / a.w), x = (int)(pi - (long)y * a.w);
  const float2 fl = reinterpret_cast<const float2*>(a.bw)[pix];
  float v = warp_fixed(a.prev + f * a.hw, a.h, a.w, x, y, fl);
  if constexpr (OCC != 0) {
    if (fb_occluded<OCC - 1>(fl, a.fw + f * a.hw * 2, a.h, a.w, x, y, a.thresh, a.err)) v = 0.f;
  }
  if (a.warped) a.warped[pix] = v;
  return v;
}

// c = cmp B,G,R, b = bg B,G,R (mean-subtracted f32), v = the warped matte
template <typename T>
__device__ __forceinline__ void store_feed(const ClipFeedArgs& a, long pix, const float* c, const float* b, float v) {
  if constexpr (sizeof(T) == 2) {
    uint4* tw = reinterpret_cast<uint4*>(a.towers);
    const float t0[8] = {c[0], c[1], c[2], 0.f, 0.f, 0.f, 0.f, 0.f};
    const float t1[8] = {b[0], b[1], b[2], 0.f, 0.f, 0.f, 0.f, 0.f};
    const float t2[8] = {v, v, v, 0.f, 0.f, 0.f, 0.f, 0.f};
    tw[pix] = Chunk<T>::pack(t0);
    tw[a.total + pix] = Chunk<T>::pack(t1);
    tw[2 * a.total + pix] = Chunk<T>::pack(t2);
    uint4* cp = reinterpret_cast<uint4*>(reinterpret_cast<T*>(a.cat) + pix * a.cat_stride);
    const float c0[8] = {c[0], c[1], c[2], b[0], b[1], b[2], v, v};
    const float c1[8] = {v, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    cp[0] = Chunk<T>::pack(c0);
    cp[1] = Chunk<T>::pack(c1);
  } else {
    float4* tw = reinterpret_cast<float4*>(a.towers);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    tw[2 * pix] = make_float4(c[0], c[1], c[2], 0.f);
    tw[2 * pix + 1] = z;
    tw[2 * (a.total + pix)] = make_float4(b[0], b[1], b[2], 0.f);
    tw[2 * (a.total + pix) + 1] = z;
    tw[2 * (2 * a.total + pix)] = make_float4(v, v, v, 0.f);
    tw[2 * (2 * a.total + pix) + 1] = z;
    float4* cp = reinterpret_cast<float4*>(reinterpret_cast<float*>(a.cat) + pix * a.cat_stride);
    cp[0] = make_float4(c[0], c[1], c[2], b[0]);
    cp[1] = make_float4(b[1], b[2], v, v);
    cp[2] = make_float4(v, 0.f, 0.f, 0.f);
    cp[3] = z;
  }
}

template <typename T, int OCC>
__global__ void __launch_bounds__(256) clip_feed_kernel(const ClipFeedArgs a) {
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nthreads = (long)gridDim.x * 256;
  for (long pix = tid; pix < a.total; pix += nthreads) {
    const long bp = a.bg_bcast ? pix % a.hw : pix;
    float c[3], b[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = bgr_value(a.cmp[pix * 3 + k], k);
      b[k] = bgr_value(a.bg[bp * 3 + k], k);
    }
    store_feed<T>(a, pix, c, b, feed_alpha<OCC>(a, pix));
  }
}

// ---------------------------------------------------------------- training loss (train.py:14-28, 42-47)
constexpr int LOSS_NBLK = 512;

__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const float* __restrict__ fg, const float* __restrict__ bg,
                                                           const float* __restrict__ cmp, long P, double* part) {
  __shared__ double sh[2][256];
  double sa = 0.0, sc = 0.0;
  const float eps2 = 1e-6f * 1e-6f;  // tf.square(tf.constant(1e-6)) in f32
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < P; i += (long)gridDim.x * blockDim.x) {
    const float a = pred[i];
    const float d = a - gt[i];
    sa += sqrtf(d * d + eps2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float pc = a * fg[i * 3 + k] + (1.f - a) * bg[i * 3 + k];
      const float e = pc - cmp[i * 3 + k];
      sc += sqrtf(e * e + eps2);
    }
  }
  sh[0][threadIdx.x] = sa;
  sh[1][threadIdx.x] = sc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = sh[0][0];
    part[blockIdx.x * 2 + 1] = sh[1][0];
  }
}

// one 256-thread block folds the nblk partial pairs (a fixed tree: deterministic; a single thread's serial walk of
// 1024 dependent loads took 47 us)
__global__ __launch_bounds__(256) void loss_final_kernel(const double* part, int nblk, long P, float* out) {
  __shared__ double sh[2][256];
  double sa = 0.0, sc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    sa += part[2 * b];
    sc += part[2 * b + 1];
  }
  sh[0][threadIdx.x] = sa;
  sh[1][threadIdx.x] = sc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double la = sh[0][0] / (double)P, lc = sh[1][0] / (3.0 * (double)P);
    out[0] = (float)(0.5 * la + 0.5 * lc);
    out[1] = (float)la;
    out[2] = (float)lc;
  }
}

}  // namespace vm

using namespace vm;

extern "C" int vm_remap_bilinear_f32(const float* img, int ih, int iw, const float* flow, int h, int w, int n,
                                     float* out, int mode, void* stream) {
  if (!img || !flow || !out || ih <= 0 || iw <= 0 || h <= 0 || w <= 0 || n <= 0 || (mode != 0 && mode != 1))
    return fail(VM_EINVAL, "remap_f32: bad argument");
  if (reinterpret_cast<uintptr_t>(flow) % 8) return fail(VM_EUNSUPPORTED, "remap_f32: flow must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long total = (long)h * w * n;
  hipLaunchKernelGGL(remap_f32_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, img, ih, iw, flow, h, w, n, out,
                     mode);
  return check_launch("remap_f32");
}

extern "C" int vm_remap_bilinear_u8(const uint8_t* img, int ih, int iw, int cn, const float* flow, int h, int w,
                                    uint8_t* out, void* stream) {
  if (!img || !flow || !out || ih <= 0 || iw <= 0 || cn <= 0 || h <= 0 || w <= 0)
    return fail(VM_EINVAL, "remap_u8: bad argument");
  if (reinterpret_cast<uintptr_t>(flow) % 8) return fail(VM_EUNSUPPORTED, "remap_u8: flow must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(remap_u8_kernel, dim3(grid_for((long)h * w, 256)), dim3(256), 0, st, img, ih, iw, cn, flow, h, w,
                     out);
  return check_launch("remap_u8");
}

extern "C" int vm_fb_consistency(const float* backward, const float* forward, int h, int w, float* alpha, float thresh,
                                 int promote, int* err_flag, void* stream) {
  if (!backward || !forward || !alpha || !err_flag || h <= 0 || w <= 0 || (promote != 0 && promote != 1))
    return fail(VM_EINVAL, "fb_consistency: bad argument");
  if ((reinterpret_cast<uintptr_t>(backward) | reinterpret_cast<uintptr_t>(forward)) % 8)
    return fail(VM_EUNSUPPORTED, "fb_consistency: flows must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for((long)h * w, 256);
  if (promote == 0) {
    hipLaunchKernelGGL(fb_check_kernel<0>, dim3(grid), dim3(256), 0, st, backward, h, w, err_flag);
    hipLaunchKernelGGL(fb_consistency_kernel<0>, dim3(grid), dim3(256), 0, st, backward, forward, h, w, alpha,
                       (double)thresh, err_flag);
  } else {
    hipLaunchKernelGGL(fb_check_kernel<1>, dim3(grid), dim3(256), 0, st, backward, h, w, err_flag);
    hipLaunchKernelGGL(fb_consistency_kernel<1>, dim3(grid), dim3(256), 0, st, backward, forward, h, w, alpha,
                       (double)thresh, err_flag);
  }
  return check_launch("fb_consistency");
}

extern "C" int vm_temporal_refine_input(const float* prev_alpha, const float* backward, const float* forward,
                                        const float* cmp, const float* alpha, int h, int w, float thresh, int promote,
                                        void* out, int out_dtype, float* warped, int* err_flag, void* stream) {
  if (!prev_alpha || !backward || !forward || !cmp || !alpha || !out || !err_flag || h <= 0 || w <= 0 ||
      (promote != 0 && promote != 1) || (out_dtype != VM_F32 && out_dtype != VM_BF16))
    return fail(VM_EINVAL, "temporal_refine_input: bad argument");
  if ((reinterpret_cast<uintptr_t>(backward) | reinterpret_cast<uintptr_t>(forward)) % 8 ||
      reinterpret_cast<uintptr_t>(out) % 16)
    return fail(VM_EUNSUPPORTED, "temporal_refine_input: flows 8-byte and out 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for((long)h * w, 256);
#define VM_TEMPORAL(TT, PR)                                                                                           \
  hipLaunchKernelGGL((temporal_input_kernel<TT, PR>), dim3(grid), dim3(256), 0, st, prev_alpha, backward, forward, cmp, \
                     alpha, h, w, (double)thresh, reinterpret_cast<TT*>(out), warped, err_flag)
  if (out_dtype == VM_BF16) {
    if (promote == 0) VM_TEMPORAL(uint16_t, 0); else VM_TEMPORAL(uint16_t, 1);
  } else {
    if (promote == 0) VM_TEMPORAL(float, 0); else VM_TEMPORAL(float, 1);
  }
#undef VM_TEMPORAL
  return check_launch("temporal_refine_input");
}

extern "C" int vm_clip_feed(const uint8_t* cmp, const uint8_t* bg, int nb, const float* prev_alpha,
                            const float* backward, const float* forward, float thresh, int promote,
                            vm_tensor* towers, vm_tensor* cat, float* warped, int* err_flag, void* stream) {
  if (!cmp || !bg || !prev_alpha || !backward) return fail(VM_EINVAL, "clip_feed: null cmp / bg / prev_alpha / backward");
  if (!towers || !towers->ptr || !cat || !cat->ptr) return fail(VM_EINVAL, "clip_feed: null towers / cat view");
  if (forward && !err_flag) return fail(VM_EINVAL, "clip_feed: a forward flow needs an err_flag");
  if (promote != 0 && promote != 1) return fail(VM_EINVAL, "clip_feed: promote %d (0 or 1)", promote);
  if (cat->n <= 0 || cat->h <= 0 || cat->w <= 0)
    return fail(VM_EINVAL, "clip_feed: bad cat view [%d,%d,%d]", cat->n, cat->h, cat->w);
  if (nb != 1 && nb != cat->n) return fail(VM_EINVAL, "clip_feed: %d backgrounds for %d frames (1 or n)", nb, cat->n);
  if ((long)towers->n != 3L * cat->n || towers->h != cat->h || towers->w != cat->w)
    return fail(VM_EINVAL, "clip_feed: towers [%d,%d,%d] against cat [%d,%d,%d] (towers are [3n,h,w])", towers->n,
                towers->h, towers->w, cat->n, cat->h, cat->w);
  if (towers->c != 3 || cat->c != 9)
    return fail(VM_EINVAL, "clip_feed: towers hold 3 channels and cat 9 (got %d and %d)", towers->c, cat->c);
  if ((cat->dtype != VM_F32 && cat->dtype != VM_BF16) || towers->dtype != cat->dtype)
    return fail(VM_EINVAL, "clip_feed: towers / cat dtypes %d / %d (both f32 or both bf16)", towers->dtype, cat->dtype);
  const int eb = elem_bytes(cat->dtype);
  if (towers->coff != 0 || towers->cstride != 8 || reinterpret_cast<uintptr_t>(towers->ptr) % 16)
    return fail(VM_EUNSUPPORTED, "clip_feed: towers are 16-byte aligned 8-channel pixels (channel offset 0)");
  if (cat->coff != 0 || cat->cstride < 16 || (cat->cstride * eb) % 16 || reinterpret_cast<uintptr_t>(cat->ptr) % 16)
    return fail(VM_EUNSUPPORTED, "clip_feed: cat pixels are 16-byte aligned, >= 16 channels apart (channel offset 0)");
  if ((reinterpret_cast<uintptr_t>(backward) | reinterpret_cast<uintptr_t>(forward)) % 8)
    return fail(VM_EUNSUPPORTED, "clip_feed: flows must be 8-byte aligned");
  ClipFeedArgs a{};
  a.cmp = cmp; a.bg = bg; a.prev = prev_alpha; a.bw = backward; a.fw = forward;
  a.towers = towers->ptr; a.cat = cat->ptr; a.warped = warped; a.err = err_flag;
  a.h = cat->h; a.w = cat->w;
  a.hw = (long)cat->h * cat->w;
  a.total = a.hw * cat->n;
  a.bg_bcast = nb == 1 && cat->n > 1;
  a.cat_stride = cat->cstride;
  a.thresh = (double)thresh;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(grid_for(a.total, 256, 256 * 32));
  const int occ = forward ? 1 + promote : 0;
#define VM_CLIP_FEED(TT, OCC) hipLaunchKernelGGL((clip_feed_kernel<TT, OCC>), grid, dim3(256), 0, st, a)
  if (cat->dtype == VM_BF16) {
    if (occ == 0) VM_CLIP_FEED(uint16_t, 0); else if (occ == 1) VM_CLIP_FEED(uint16_t, 1); else VM_CLIP_FEED(uint16_t, 2);
  } else {
    if (occ == 0) VM_CLIP_FEED(float, 0); else if (occ == 1) VM_CLIP_FEED(float, 1); else VM_CLIP_FEED(float, 2);
  }
#undef VM_CLIP_FEED
  return check_launch("clip_feed");
}

extern "C" size_t vm_loss_workspace_bytes(long pixels) {
  (void)pixels;
  return (size_t)LOSS_NBLK * 2 * sizeof(double);
}

extern "C" int vm_matting_loss(const float* pred, const float* gt, const float* raw_fg, const float* bg,
                               const float* cmp, long pixels, float* out, void* work, void* stream) {
  if (!pred || !gt || !raw_fg || !bg || !cmp || !out || !work || pixels <= 0)
    return fail(VM_EINVAL, "matting_loss: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nblk = grid_for(pixels, 256, LOSS_NBLK);
  double* part = reinterpret_cast<double*>(work);
  hipLaunchKernelGGL(loss_partial_kernel, dim3(nblk), dim3(256), 0, st, pred, gt, raw_fg, bg, cmp, pixels, part);
  int rc = check_launch("loss_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, part, nblk, pixels, out);
  return check_launch("loss_final");
}
