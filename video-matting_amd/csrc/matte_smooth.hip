// vm_matte_smooth: the flow-compensated temporal filter of a clip's mattes (the definition: include/vmatting.h).  Frame
// j's matte is pulled towards the previous filtered matte, sampled where the backward flow says the pixel came from, by
// a weight that two gates close: the colour difference between the frame and the warped previous frame, and the jump
// between the matte and the warped previous matte.  Every step is f32 with nothing contracted (the unit is built with
// -ffp-contract=off), so the numpy restatement (tests/matte_smooth_ref.py) is matched bit for bit.
//
// One launch per frame, in stream order: frame j gathers from out[j - 1], which the launch before it wrote.  A thread
// owns 4 consecutive pixels of a row.  Where all four lie in the row and their alpha, out, weight and flow addresses
// are 16-byte aligned it moves them with 16-byte loads and stores (one for alpha, two for the flow, one per result) and
// reads the 12 frame bytes as the aligned dwords around them (vm_common.h's load_bytes); a ragged row end, and every
// group of a row that does not start on 16 bytes (w no multiple of 4, or an odd frame base), goes pixel by pixel.  The
// four taps of the previous matte and of the previous frame are gathers: neighbouring lanes read neighbouring
// addresses wherever the flow is smooth, and the previous matte was written by the launch just before, so they mostly
// hit L2.  Streamed per pixel: flow 8 + alpha 4 + out 4 + frame 3 bytes (+ 4 with `weight`).  No LDS, no atomics.
//
// A frame without a predecessor is the clamp alone: out = unit(alpha), weight = 0.
#include "vm_common.h"

#include <cfloat>
#include <climits>

namespace vm {
namespace {

constexpr int PX = 4;  // pixels per thread

struct SmoothFrame {
  const float* alpha;       // [h,w] (may be `out`)
  const uint8_t* cmp;       // [h,w,3]
  const float* backward;    // [h,w,2]
  const float* prev;        // [h,w]: the previous filtered matte
  const uint8_t* prev_cmp;  // [h,w,3]
  float* out;               // [h,w]
  float* weight;            // [h,w] or null
  int h, w;
  float strength, inv_tol, inv_jump;
};

// vm_matte_score's clamp to [0,1] (NaN -> 0)
__device__ __forceinline__ float unit(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }

__device__ __forceinline__ float bilinear(float v00, float v01, float v10, float v11, float fx, float fy) {
  const float top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
  return top + fy * (bot - top);
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// steps 1-10 of the definition for pixel (x, y): its stored alpha, its flow and its three frame bytes -> s; *k = weight
__device__ __forceinline__ float smooth_pixel(const SmoothFrame& f, int x, int y, float alpha, float u, float v,
                                              uint32_t c0, uint32_t c1, uint32_t c2, float* k) {
  const int h = f.h, w = f.w;
  const float a = unit(alpha);
  const float xs = (float)x + u, ys = (float)y + v;
  const bool inside = xs >= 0.f && xs <= (float)(w - 1) && ys >= 0.f && ys <= (float)(h - 1);  // (false for NaN)
  // no branch around the gathers: a pixel outside reads pixel (0, 0) and gives it weight 0
  const float xc = inside ? xs : 0.f, yc = inside ? ys : 0.f;
  const float xf = floorf(xc), yf = floorf(yc);
  const float fx = xc - xf, fy = yc - yf;
  const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
  const size_t i00 = (size_t)y0 * w + x0, i01 = (size_t)y0 * w + x1;
  const size_t i10 = (size_t)y1 * w + x0, i11 = (size_t)y1 * w + x1;
  const float p = bilinear(unit(f.prev[i00]), unit(f.prev[i01]), unit(f.prev[i10]), unit(f.prev[i11]), fx, fy);
  const uint8_t* pc = f.prev_cmp;
  const uint32_t c[3] = {c0, c1, c2};
  float d = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float cp = bilinear((float)pc[3 * i00 + ch], (float)pc[3 * i01 + ch], (float)pc[3 * i10 + ch],
                              (float)pc[3 * i11 + ch], fx, fy);
    d = fmaxf(d, fabsf((float)c[ch] - cp));
  }
  const float gates = unit(1.f - d * f.inv_tol) * unit(1.f - fabsf(a - p) * f.inv_jump);
  *k = inside ? gates : 0.f;
  return unit(a + (f.strength * *k) * (p - a));
}

template <bool HAS_PREV>
__global__ void __launch_bounds__(256) smooth_kernel(SmoothFrame f, int groups, long items) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int y = (int)(i / groups), x = PX * (int)(i - (long)y * groups);
  const size_t p = (size_t)y * f.w + x;
  const int count = min(PX, f.w - x);
  bool wide = count == PX && aligned16(f.alpha + p) && aligned16(f.out + p) && (!f.weight || aligned16(f.weight + p));
  if (HAS_PREV) wide = wide && aligned16(f.backward + 2 * p);
  if (wide) {
    float a[PX], s[PX], k[PX];
    Chunk<float>::unpack(*reinterpret_cast<const uint4*>(f.alpha + p), a);
    if (HAS_PREV) {
      float fl[2 * PX];
      Chunk<float>::unpack(*reinterpret_cast<const uint4*>(f.backward + 2 * p), fl);
      Chunk<float>::unpack(*reinterpret_cast<const uint4*>(f.backward + 2 * p + 4), fl + 4);
      uint32_t d[3];
      load_bytes<3>(f.cmp + 3 * p, d);
#pragma unroll
      for (int e = 0; e < PX; ++e)
        s[e] = smooth_pixel(f, x + e, y, a[e], fl[2 * e], fl[2 * e + 1], byte_of(d, 3 * e), byte_of(d, 3 * e + 1),
                            byte_of(d, 3 * e + 2), &k[e]);
    } else {
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        s[e] = unit(a[e]);
        k[e] = 0.f;
      }
    }
    *reinterpret_cast<uint4*>(f.out + p) = Chunk<float>::pack(s);
    if (f.weight) *reinterpret_cast<uint4*>(f.weight + p) = Chunk<float>::pack(k);
    return;
  }
  for (int e = 0; e < count; ++e) {
    const size_t q = p + e;
    float k = 0.f, s;
    if (HAS_PREV) {
      s = smooth_pixel(f, x + e, y, f.alpha[q], f.backward[2 * q], f.backward[2 * q + 1], f.cmp[3 * q], f.cmp[3 * q + 1],
                       f.cmp[3 * q + 2], &k);
    } else {
      s = unit(f.alpha[q]);
    }
    f.out[q] = s;
    if (f.weight) f.weight[q] = k;
  }
}

inline bool bytes_ok(int n, int h, int w) { return shape_ok(n, h, w) && (long)n * h * w <= (long)INT_MAX / 3; }

inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" int vm_matte_smooth(const float* alpha, const uint8_t* cmp, const float* backward, const float* prev_alpha,
                               const uint8_t* prev_cmp, int n, int h, int w, float strength, float tol, float jump,
                               float* out, float* weight, void* stream) {
  const char* who = "matte_smooth";
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!bytes_ok(n, h, w)) return fail(VM_EINVAL, "%s: %d x %d x %d x 3 bytes exceed %d", who, n, h, w, INT_MAX);
  if (!alpha || !cmp || !backward || !out) return fail(VM_EINVAL, "%s: null alpha / cmp / backward / out", who);
  if (!prev_alpha != !prev_cmp) return fail(VM_EINVAL, "%s: prev_alpha and prev_cmp go together", who);
  if (!(strength >= 0.f && strength < 1.f)) return fail(VM_EINVAL, "%s: strength %g (0 <= strength < 1)", who, strength);
  if (!(tol > 0.f && tol <= FLT_MAX)) return fail(VM_EINVAL, "%s: tol %g (a positive finite number)", who, tol);
  if (!(jump > 0.f && jump <= FLT_MAX)) return fail(VM_EINVAL, "%s: jump %g (a positive finite number)", who, jump);
  if (!aligned4(alpha) || !aligned4(backward) || !aligned4(prev_alpha) || !aligned4(out) || !aligned4(weight))
    return fail(VM_EINVAL, "%s: alpha, backward, prev_alpha, out and weight must be 4-byte aligned", who);
  const size_t plane = (size_t)h * w, all = (size_t)n * plane;
  const struct {
    const void* p;
    size_t bytes;
  } inputs[5] = {{alpha, all * 4}, {cmp, all * 3}, {backward, all * 8}, {prev_alpha, plane * 4}, {prev_cmp, plane * 3}};
  for (int i = 0; i < 5; ++i) {
    if (!inputs[i].p) continue;
    if (!(i == 0 && out == alpha) && overlap(out, all * 4, inputs[i].p, inputs[i].bytes))
      return fail(VM_EINVAL, "%s: out must be alpha itself or overlap no input", who);
    if (weight && overlap(weight, all * 4, inputs[i].p, inputs[i].bytes))
      return fail(VM_EINVAL, "%s: weight must not overlap an input", who);
  }
  if (weight && overlap(weight, all * 4, out, all * 4)) return fail(VM_EINVAL, "%s: weight must not overlap out", who);

  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int groups = (w + PX - 1) / PX;
  const long items = (long)h * groups;
  const dim3 grid((unsigned)((items + 255) / 256));
  SmoothFrame f;
  f.h = h;
  f.w = w;
  f.strength = strength;
  f.inv_tol = 1.0f / tol;  // f32, here: the kernel has no division
  f.inv_jump = 1.0f / jump;
  for (int j = 0; j < n; ++j) {
    f.alpha = alpha + j * plane;
    f.cmp = cmp + j * plane * 3;
    f.backward = backward + j * plane * 2;
    f.out = out + j * plane;
    f.weight = weight ? weight + j * plane : nullptr;
    f.prev = j ? out + (j - 1) * plane : prev_alpha;
    f.prev_cmp = j ? cmp + (j - 1) * plane * 3 : prev_cmp;
    if (f.prev)
      hipLaunchKernelGGL(smooth_kernel<true>, grid, dim3(256), 0, st, f, groups, items);
    else
      hipLaunchKernelGGL(smooth_kernel<false>, grid, dim3(256), 0, st, f, groups, items);
  }
  return check_launch(who);
}
