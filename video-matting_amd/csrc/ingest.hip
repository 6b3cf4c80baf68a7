// The two ends of inference on a decoded clip: uint8 frames -> the network's input (vm_frames_from_u8) and f32
// alpha -> 8- / 16-bit mattes (vm_matte_quantize).  Both are pure memory traffic (7 B in, 28 or 16 B out per pixel;
// 4 B in, 1 or 2 B out), so each thread takes 4 pixels: dword loads of the u8 planes, 16-byte stores of the frame,
// 16-byte loads of the alpha, one packed store of the matte; a scalar tail covers pixels % 4.
//
// Arithmetic of vm_frames_from_u8 (the reference's inference feed, loader.py:45,75-78): the mean and the 0.5 are
// subtracted in float64 and the result is rounded to f32 once; the bf16 form is the RNE bf16 of that f32, the rounding
// Chunk<T>::pack applies when the pair kernel reads an f32 frame.  The BGR planes are computed directly in double
// (convert, subtract, convert); the trimap's u / 255.0 - 0.5 comes from a 256-entry table each block builds in double
// (one f64 division per entry instead of one per pixel).
//
// vm_matte_compose applies the matte: with C = a F + (1 - a) B and B known, the BGRA foreground layer (straight or
// premultiplied, a = q / 255 of the stored 8-bit matte) or the frame over a new plate N, C + (1 - a)(N - B).  All in
// float64, one rounding at the end (the formulas: include/vmatting.h).  Traffic per pixel: 4 B alpha + 3 B cmp + 3 B
// bg (+ 3 B new plate) read, 3 or 4 B written = 13 - 16 B; a static plate is re-read from cache.  Same shape as the
// ingest kernel: 4 pixels per thread, a scalar tail, one pixel per thread when an operand is unaligned.
#include "vm_common.h"

namespace vm {
namespace {

// (bgr_value is in vm_common.h: vm_clip_feed in flow.hip feeds the same values)
struct IngestArgs {
  const uint8_t* cmp;
  const uint8_t* bg;
  const uint8_t* tri;  // null: 6 channels
  void* out;           // first element of the view (coff applied)
  long total;          // n * h * w
  long hw;             // pixels per frame (bg broadcast: nb == 1)
  int bg_bcast;        // 1: bg is one [h,w,3] plate
  int cstride;         // elements per output pixel
  int vec;             // 1: the u8 planes are 4-byte aligned (dword loads of 4-pixel groups)
};

// one pixel's C values (C = 7 with a trimap, 6 without) + zeros up to 8
template <int C>
__device__ __forceinline__ void pixel_values(const IngestArgs& a, const float* lut, long pix, float* v) {
  const long bp = a.bg_bcast ? pix % a.hw : pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = bgr_value(a.cmp[pix * 3 + c], c);
    v[3 + c] = bgr_value(a.bg[bp * 3 + c], c);
  }
  v[6] = C == 7 ? lut[a.tri[pix]] : 0.f;
  v[7] = 0.f;
}

// BF8 = 0: f32 pixels of C channels at any stride; BF8 = 1: bf16 pixels of 8 channels (C values + zeros), 16 bytes
template <int C, int BF8>
__device__ __forceinline__ void store_pixel(const IngestArgs& a, long pix, const float* v) {
  if constexpr (BF8) {
    reinterpret_cast<uint4*>(a.out)[pix] = Chunk<uint16_t>::pack(v);
  } else {
    float* o = reinterpret_cast<float*>(a.out) + pix * a.cstride;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = v[c];
  }
}

// 12 bytes = 4 BGR pixels starting at byte offset `off` (a multiple of 12 from a 4-byte aligned plane)
__device__ __forceinline__ void load12(const uint8_t* p, long off, uint32_t* w) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p + off);
  w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
}

// DENSE = 1: f32 [pixels, C] without gaps, 16-byte aligned -> 4 pixels are C float4 stores; BF8 = 1: 4 uint4 stores.
// DENSE = 0 and BF8 = 0: f32 at a channel offset / stride, one pixel per thread and scalar stores.
template <int C, int BF8, int DENSE>
__global__ void __launch_bounds__(256) frames_from_u8_kernel(const IngestArgs a) {
  __shared__ float lut[256];
  if (C == 7) {
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0 - 0.5);
    __syncthreads();
  }
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nthreads = (long)gridDim.x * 256;
  const bool vec = a.vec && (BF8 || DENSE);
  const long groups = vec ? a.total / 4 : 0;
  const bool bg_vec = !a.bg_bcast || a.hw % 4 == 0;  // a 4-pixel group never straddles the plate's end
  for (long g = tid; g < groups; g += nthreads) {
    const long p0 = g * 4;
    uint32_t wc[3], wb[3], wt = 0;
    load12(a.cmp, p0 * 3, wc);
    if (bg_vec) {
      load12(a.bg, (a.bg_bcast ? p0 % a.hw : p0) * 3, wb);
    } else {
      wb[0] = wb[1] = wb[2] = 0;
#pragma unroll
      for (int i = 0; i < 12; ++i) wb[i >> 2] |= (uint32_t)a.bg[((p0 + i / 3) % a.hw) * 3 + i % 3] << ((i & 3) * 8);
    }
    if (C == 7) wt = *reinterpret_cast<const uint32_t*>(a.tri + p0);
    float v[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[j][c] = bgr_value(byte_of(wc, 3 * j + c), c);
        v[j][3 + c] = bgr_value(byte_of(wb, 3 * j + c), c);
      }
      v[j][6] = C == 7 ? lut[(wt >> (8 * j)) & 0xffu] : 0.f;
      v[j][7] = 0.f;
    }
    if constexpr (BF8) {
      uint4* o = reinterpret_cast<uint4*>(a.out) + p0;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = Chunk<uint16_t>::pack(v[j]);
    } else {
      float f[4 * C];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) f[j * C + c] = v[j][c];
      float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + p0 * C);
#pragma unroll
      for (int q = 0; q < C; ++q) o[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
    }
  }
  // scalar tail (total % 4 pixels), or every pixel when the planes are unaligned / the output is strided
  for (long pix = groups * 4 + tid; pix < a.total; pix += nthreads) {
    float v[8];
    pixel_values<C>(a, lut, pix, v);
    store_pixel<C, BF8>(a, pix, v);
  }
}

template <int BITS>
__device__ __forceinline__ uint32_t quantize1(float x) {
  constexpr float M = BITS == 8 ? 255.f : 65535.f;
  float r = rintf(x * M);    // f32 product, round half to even
  r = r >= 0.f ? r : 0.f;    // NaN and negatives -> 0
  r = r > M ? M : r;
  return (uint32_t)r;
}

// 4 alphas per thread: one 16-byte load, one 4-byte (u8) or 8-byte (u16) store; groups = 0 when unaligned
template <int BITS>
__global__ void __launch_bounds__(256) matte_quantize_kernel(const float* __restrict__ alpha, long pixels, long groups,
                                                             void* __restrict__ out) {
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nthreads = (long)gridDim.x * 256;
  for (long g = tid; g < groups; g += nthreads) {
    const float4 a = reinterpret_cast<const float4*>(alpha)[g];
    const uint32_t q0 = quantize1<BITS>(a.x), q1 = quantize1<BITS>(a.y), q2 = quantize1<BITS>(a.z),
                   q3 = quantize1<BITS>(a.w);
    if constexpr (BITS == 8)
      reinterpret_cast<uint32_t*>(out)[g] = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
    else
      reinterpret_cast<uint2*>(out)[g] = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
  }
  for (long i = groups * 4 + tid; i < pixels; i += nthreads) {
    const uint32_t q = quantize1<BITS>(alpha[i]);
    if constexpr (BITS == 8)
      reinterpret_cast<uint8_t*>(out)[i] = (uint8_t)q;
    else
      reinterpret_cast<uint16_t*>(out)[i] = (uint16_t)q;
  }
}

// ---------------------------------------------------------------- the matte applied (vm_matte_compose)
struct ComposeArgs {
  const float* alpha;
  const uint8_t* cmp;
  const uint8_t* bg;
  const uint8_t* nw;  // the new plate(s): OVER only
  uint8_t* out;
  long total;         // n * h * w
  long hw;            // pixels per frame (a broadcast plate wraps here)
  int bg_bcast;       // 1: bg is one [h,w,3] plate under n > 1 frames
  int nw_bcast;       // likewise for the new plate
  int vec;            // 1: every operand is aligned for the 4-pixel form
};

// (uint8) rint(min(max(v, 0), 255)), ties to even; v is never NaN here
__device__ __forceinline__ uint32_t fin(double v) {
  v = v > 0.0 ? v : 0.0;
  v = v < 255.0 ? v : 255.0;
  return (uint32_t)rint(v);
}

// One pixel: c / b / nw point at its 3 BGR bytes' values.  Returns B | G << 8 | R << 16 (| A << 24 for the layers).
template <int MODE>
__device__ __forceinline__ uint32_t compose1(float alpha, const uint32_t* c, const uint32_t* b, const uint32_t* nw) {
  uint32_t px = 0;
  if constexpr (MODE == VM_COMPOSE_OVER) {
    double a = (double)alpha;
    a = a >= 0.0 ? a : 0.0;  // NaN and negatives -> 0
    a = a > 1.0 ? 1.0 : a;
    const double k = 1.0 - a;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      px |= fin((double)c[ch] + k * ((double)nw[ch] - (double)b[ch])) << (8 * ch);
  } else {
    const uint32_t q = quantize1<8>(alpha);
    const double qd = (double)q;
    if constexpr (MODE == VM_COMPOSE_PREMUL) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        px |= fin((double)c[ch] - ((255.0 - qd) * (double)b[ch]) / 255.0) << (8 * ch);
    } else if (q != 0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        px |= fin((double)b[ch] + (((double)c[ch] - (double)b[ch]) * 255.0) / qd) << (8 * ch);
    }
    px |= q << 24;
  }
  return px;
}

// 12 bytes = the 4 BGR pixels from p0 of a plane that is per-frame, or one plate wrapping at hw
__device__ __forceinline__ void load_plane12(const uint8_t* p, int bcast, long hw, long p0, uint32_t* w) {
  if (!bcast) {
    load12(p, p0 * 3, w);
  } else if (hw % 4 == 0) {  // a 4-pixel group never straddles the plate's end
    load12(p, (p0 % hw) * 3, w);
  } else {
    w[0] = w[1] = w[2] = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i >> 2] |= (uint32_t)p[((p0 + i / 3) % hw) * 3 + i % 3] << ((i & 3) * 8);
  }
}

// 4 pixels per thread when a.vec: one float4 of alpha, 3 dwords per u8 plane, one 16-byte (BGRA) or three 4-byte
// (BGR) stores; then a scalar tail, which is every pixel when an operand is unaligned
template <int MODE>
__global__ void __launch_bounds__(256) matte_compose_kernel(const ComposeArgs a) {
  constexpr bool OVER = MODE == VM_COMPOSE_OVER;
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nthreads = (long)gridDim.x * 256;
  const long groups = a.vec ? a.total / 4 : 0;
  for (long g = tid; g < groups; g += nthreads) {
    const long p0 = g * 4;
    const float4 al = reinterpret_cast<const float4*>(a.alpha)[g];
    const float av[4] = {al.x, al.y, al.z, al.w};
    uint32_t wc[3], wb[3], wn[3] = {0, 0, 0};
    load12(a.cmp, p0 * 3, wc);
    load_plane12(a.bg, a.bg_bcast, a.hw, p0, wb);
    if constexpr (OVER) load_plane12(a.nw, a.nw_bcast, a.hw, p0, wn);
    uint32_t px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t c[3], b[3], nw[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        c[ch] = byte_of(wc, 3 * j + ch);
        b[ch] = byte_of(wb, 3 * j + ch);
        nw[ch] = byte_of(wn, 3 * j + ch);
      }
      px[j] = compose1<MODE>(av[j], c, b, nw);
    }
    if constexpr (OVER) {
      uint32_t* o = reinterpret_cast<uint32_t*>(a.out + p0 * 3);
      o[0] = px[0] | (px[1] << 24);
      o[1] = (px[1] >> 8) | (px[2] << 16);
      o[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
      reinterpret_cast<uint4*>(a.out)[g] = make_uint4(px[0], px[1], px[2], px[3]);
    }
  }
  for (long pix = groups * 4 + tid; pix < a.total; pix += nthreads) {
    const long bp = a.bg_bcast ? pix % a.hw : pix, np = a.nw_bcast ? pix % a.hw : pix;
    uint32_t c[3], b[3], nw[3] = {0, 0, 0};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      c[ch] = a.cmp[pix * 3 + ch];
      b[ch] = a.bg[bp * 3 + ch];
      if constexpr (OVER) nw[ch] = a.nw[np * 3 + ch];
    }
    const uint32_t px = compose1<MODE>(a.alpha[pix], c, b, nw);
    uint8_t* o = a.out + pix * (OVER ? 3 : 4);
#pragma unroll
    for (int ch = 0; ch < (OVER ? 3 : 4); ++ch) o[ch] = (uint8_t)(px >> (8 * ch));
  }
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" int vm_frames_from_u8(const uint8_t* cmp, const uint8_t* bg, const uint8_t* trimap, int nb,
                                 vm_tensor* out, void* stream) {
  if (!cmp || !bg || !out || !out->ptr) return fail(VM_EINVAL, "frames_from_u8: null cmp / bg / output");
  if (out->n <= 0 || out->h <= 0 || out->w <= 0 || out->coff < 0 || out->c <= 0 || out->coff + out->c > out->cstride)
    return fail(VM_EINVAL, "frames_from_u8: bad output view [%d,%d,%d,%d] at %d of %d", out->n, out->h, out->w, out->c,
                out->coff, out->cstride);
  if (nb != 1 && nb != out->n) return fail(VM_EINVAL, "frames_from_u8: %d backgrounds for %d frames (1 or n)", nb, out->n);
  if (out->c != (trimap ? 7 : 6))
    return fail(VM_EINVAL, "frames_from_u8: %d output channels %s a trimap (7 with, 6 without)", out->c,
                trimap ? "with" : "without");
  if (out->dtype != VM_F32 && out->dtype != VM_BF16)
    return fail(VM_EINVAL, "frames_from_u8: output dtype %d (f32 or bf16)", out->dtype);
  const bool bf = out->dtype == VM_BF16;
  if (bf && (out->coff != 0 || out->cstride != 8 || reinterpret_cast<uintptr_t>(out->ptr) % 16))
    return fail(VM_EUNSUPPORTED, "frames_from_u8: a bf16 frame is 16-byte aligned 8-channel pixels (channel offset 0)");
  IngestArgs a{};
  a.cmp = cmp; a.bg = bg; a.tri = trimap;
  a.out = reinterpret_cast<char*>(out->ptr) + (size_t)out->coff * (bf ? 2 : 4);
  a.hw = (long)out->h * out->w;
  a.total = a.hw * out->n;
  a.bg_bcast = nb == 1 && out->n > 1;
  a.cstride = out->cstride;
  a.vec = reinterpret_cast<uintptr_t>(cmp) % 4 == 0 && reinterpret_cast<uintptr_t>(bg) % 4 == 0 &&
          reinterpret_cast<uintptr_t>(trimap) % 4 == 0;
  const bool dense = !bf && out->cstride == out->c && reinterpret_cast<uintptr_t>(a.out) % 16 == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool grouped = a.vec && (bf || dense);
  const dim3 grid(grid_for(grouped ? (a.total + 3) / 4 : a.total, 256, 256 * 32));
#define VM_INGEST(C, BF8, DENSE) \
  hipLaunchKernelGGL((frames_from_u8_kernel<C, BF8, DENSE>), grid, dim3(256), 0, st, a)
  if (trimap) {
    if (bf) VM_INGEST(7, 1, 0); else if (dense) VM_INGEST(7, 0, 1); else VM_INGEST(7, 0, 0);
  } else {
    if (bf) VM_INGEST(6, 1, 0); else if (dense) VM_INGEST(6, 0, 1); else VM_INGEST(6, 0, 0);
  }
#undef VM_INGEST
  return check_launch("frames_from_u8");
}

extern "C" int vm_matte_quantize(const float* alpha, long pixels, int bits, void* out, void* stream) {
  if (!alpha || !out || pixels <= 0) return fail(VM_EINVAL, "matte_quantize: null pointer or no pixels");
  if (bits != 8 && bits != 16) return fail(VM_EINVAL, "matte_quantize: %d-bit mattes (8 or 16)", bits);
  const bool vec = reinterpret_cast<uintptr_t>(alpha) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % (bits / 2) == 0;
  const long groups = vec ? pixels / 4 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(grid_for(vec ? (pixels + 3) / 4 : pixels, 256, 256 * 32));
  if (bits == 8)
    hipLaunchKernelGGL((matte_quantize_kernel<8>), grid, dim3(256), 0, st, alpha, pixels, groups, out);
  else
    hipLaunchKernelGGL((matte_quantize_kernel<16>), grid, dim3(256), 0, st, alpha, pixels, groups, out);
  return check_launch("matte_quantize");
}

extern "C" int vm_matte_compose(const float* alpha, const uint8_t* cmp, const uint8_t* bg, int nb, const uint8_t* new_bg,
                                int nn, int n, int h, int w, int mode, uint8_t* out, void* stream) {
  if (!alpha || !cmp || !bg || !out) return fail(VM_EINVAL, "matte_compose: null alpha / cmp / bg / output");
  if (n <= 0 || h <= 0 || w <= 0) return fail(VM_EINVAL, "matte_compose: bad shape [%d,%d,%d]", n, h, w);
  if (nb != 1 && nb != n) return fail(VM_EINVAL, "matte_compose: %d backgrounds for %d frames (1 or n)", nb, n);
  if (mode < VM_COMPOSE_OVER || mode > VM_COMPOSE_PREMUL)
    return fail(VM_EINVAL, "matte_compose: mode %d (0 over, 1 straight BGRA, 2 premultiplied BGRA)", mode);
  const bool over = mode == VM_COMPOSE_OVER;
  if (over && (!new_bg || (nn != 1 && nn != n)))
    return fail(VM_EINVAL, "matte_compose: over takes a new background, %d plates for %d frames (1 or n)", nn, n);
  if (!over && (new_bg || nn != 0)) return fail(VM_EINVAL, "matte_compose: a BGRA layer takes no new background");
  ComposeArgs a{};
  a.alpha = alpha; a.cmp = cmp; a.bg = bg; a.nw = new_bg; a.out = out;
  a.hw = (long)h * w;
  a.total = a.hw * n;
  a.bg_bcast = nb == 1 && n > 1;
  a.nw_bcast = over && nn == 1 && n > 1;
  auto aligned = [](const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; };
  a.vec = aligned(alpha, 16) && aligned(cmp, 4) && aligned(bg, 4) && (!over || aligned(new_bg, 4)) &&
          aligned(out, over ? 4 : 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(grid_for(a.vec ? (a.total + 3) / 4 : a.total, 256, 256 * 32));
  if (mode == VM_COMPOSE_OVER)
    hipLaunchKernelGGL((matte_compose_kernel<VM_COMPOSE_OVER>), grid, dim3(256), 0, st, a);
  else if (mode == VM_COMPOSE_STRAIGHT)
    hipLaunchKernelGGL((matte_compose_kernel<VM_COMPOSE_STRAIGHT>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((matte_compose_kernel<VM_COMPOSE_PREMUL>), grid, dim3(256), 0, st, a);
  return check_launch("matte_compose");
}
