// What the training units share (train.hip: element-wise backward + optimizer; wgrad*.hip: conv weight gradients):
// the strided NHWC view their kernels take by value, its element accessors and the entry points' argument checks.
#pragma once

#include "conv_common.h"

namespace vm {
namespace trn {

struct V {
  char* p;
  int n, h, w, c, cs, coff, dt;
  int sc;     // > 0: channel c lives in source c / sc (tower-major features), sources ss elements apart
  long ss;
};

static V mk(const vm_tensor* t) {
  V v;
  v.p = reinterpret_cast<char*>(t->ptr);
  v.n = t->n; v.h = t->h; v.w = t->w; v.c = t->c; v.cs = t->cstride; v.coff = t->coff; v.dt = t->dtype;
  v.sc = 0; v.ss = 0;
  return v;
}

__device__ __forceinline__ long vchan(const V& v, int c) {
  if (v.sc <= 0) return c;
  const int s = c / v.sc;
  return (long)s * v.ss + (c - s * v.sc);
}

__device__ __forceinline__ float ld(const V& v, long pix, int c) {
  const long o = pix * v.cs + v.coff + vchan(v, c);
  return v.dt == VM_F32 ? reinterpret_cast<const float*>(v.p)[o] : bf2f(reinterpret_cast<const uint16_t*>(v.p)[o]);
}

__device__ __forceinline__ void st(const V& v, long pix, int c, float x) {
  const long o = pix * v.cs + v.coff + c;
  if (v.dt == VM_F32) reinterpret_cast<float*>(v.p)[o] = x;
  else reinterpret_cast<uint16_t*>(v.p)[o] = f2bf(x);
}

static bool ok_view(const vm_tensor* t) { return valid_tensor(t); }

static bool same_shape(const vm_tensor* a, const vm_tensor* b) {
  return a->n == b->n && a->h == b->h && a->w == b->w && a->c == b->c;
}

}  // namespace trn
}  // namespace vm
