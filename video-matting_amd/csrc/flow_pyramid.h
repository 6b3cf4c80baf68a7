// What the units that read a vm_flow_pyramid result share (flow_est.hip, which writes it, and plate_align.hip): the
// levels' sizes and offsets, and the bilinear sample with coordinates clamped to the image (include/vmatting.h).
#pragma once

#include "vm_common.h"

namespace vm {

constexpr int FLOW_MAX_LEVELS = 32, FLOW_MAX_SIDE = 32768;

struct Plan {
  int n;                   // levels built
  int h[FLOW_MAX_LEVELS], w[FLOW_MAX_LEVELS];
  size_t off[FLOW_MAX_LEVELS];  // floats from the pyramid's start (each a multiple of 4)
  size_t floats;           // one pyramid
};

inline Plan plan_levels(int h, int w, int levels) {
  Plan p{};
  p.n = 1;
  p.h[0] = h;
  p.w[0] = w;
  while (p.n < levels && p.n < FLOW_MAX_LEVELS &&
         (p.h[p.n - 1] < p.w[p.n - 1] ? p.h[p.n - 1] : p.w[p.n - 1]) / 2 >= 8) {
    p.h[p.n] = (p.h[p.n - 1] + 1) / 2;
    p.w[p.n] = (p.w[p.n - 1] + 1) / 2;
    ++p.n;
  }
  for (int k = 0; k < p.n; ++k) {
    p.off[k] = p.floats;
    p.floats += ((size_t)p.h[k] * p.w[k] + 3) / 4 * 4;
  }
  return p;
}

// ---------------------------------------------------------------- bilinear, coordinates clamped to the image
struct Tap {
  long i00, i01, i10, i11;
  float fx, fy;
};

__device__ __forceinline__ Tap tap_at(float x, float y, int h, int w) {
  x = fminf(fmaxf(x, 0.f), (float)(w - 1));  // (a NaN coordinate becomes 0: every index stays inside)
  y = fminf(fmaxf(y, 0.f), (float)(h - 1));
  const float xf = floorf(x), yf = floorf(y);
  const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
  Tap t;
  t.fx = x - xf;
  t.fy = y - yf;
  t.i00 = (long)y0 * w + x0; t.i01 = (long)y0 * w + x1;
  t.i10 = (long)y1 * w + x0; t.i11 = (long)y1 * w + x1;
  return t;
}

__device__ __forceinline__ float lerp2(float p00, float p01, float p10, float p11, float fx, float fy) {
  const float top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
  return top + fy * (bot - top);
}

}  // namespace vm
