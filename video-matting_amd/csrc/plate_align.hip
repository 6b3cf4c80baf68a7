// vm_plate_align_fit / vm_plate_align_apply: one affine map and one photometric gain per frame between a frame and its
// background plate, and the plate seen through that map (the definition: include/vmatting.h; the numpy restatement:
// tests/plate_align_ref.py).  Per-pixel quantities are f32 in the written order (this unit is built with
// -ffp-contract=off and correctly rounded division, like flow_est.hip, whose pyramids and bilinear sample it reads:
// flow_pyramid.h); the sums over the inliers and the 7 x 7 solve are f64.
//
//   start   one block per frame: the f64 sums of the coarsest level of both pyramids; params = (0 .. 0, g0, 0).
//   sums    one Gauss-Newton step's sums for all frames: block b of the 1-D grid is block b % bpf of frame b / bpf and
//       walks its share of the level's pixels, one pixel per thread and pass.  A lane keeps the 28 + 7 sums in f64
//       registers (each term one f32 product, widened, then added: 130 VGPRs in all, no scratch - `make asm`) and
//       the two counts as integers; the block reduces them in a fixed tree - wave-64 shuffles, then the four waves'
//       results in LDS added in wave order - and writes its PART doubles to `work`.  bpf depends on the level's size
//       only, never on n, so a batch gives what single calls give.  No atomics.
//   solve   one block per frame: thread e adds entry e of the frame's bpf partials in block order; thread 0 then runs
//       the share test and the elimination in f64, adds the step to params and writes the support; after the last step
//       it applies the guards.
//   apply   a thread per output pixel: four taps of three bytes each, one rounding.
//
// A fit is 1 + 2 levels iters launches for all n frames, a fixed sequence: no allocation, no synchronisation, no
// read-back.  The sums kernel reads the frame level once and the plate level at five positions per pixel, which share
// their cache lines; the coarse levels are launch-bound.
#include "flow_pyramid.h"
#include "vm_common.h"

#include <cmath>

namespace vm {
namespace {

constexpr int NPAR = 7;                     // six affine deviations and the gain
constexpr int NSUM = 28 + NPAR;             // the upper triangle of J^T J, then J^T r
constexpr int PART = 40;                    // doubles per block in `work`: NSUM sums, count, close, 3 unused
constexpr int I_COUNT = NSUM, I_CLOSE = NSUM + 1;
constexpr int BPF_MAX = 256;                // blocks per frame at most: the solve adds that many partials in order
constexpr int PIX_PER_THREAD = 8;           // ... and about this many pixels per thread below that
constexpr int ITERS_MAX = 64, SHARE_MAX = 4096, REACH_MAX = 1024;
constexpr int PARAM_FLOATS = 8;

inline int blocks_per_frame(long pixels) {
  const long b = (pixels + 256L * PIX_PER_THREAD - 1) / (256L * PIX_PER_THREAD);
  return (int)(b < 1 ? 1 : b > BPF_MAX ? BPF_MAX : b);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__device__ __forceinline__ bool all_finite(const float* p) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NPAR; ++i) ok = ok && isfinite(p[i]);
  return ok;
}

__global__ void __launch_bounds__(256)
align_start_kernel(const float* __restrict__ cmp, long cmp_stride, const float* __restrict__ bg, long bg_stride, int nb,
                   long off, long count, float* __restrict__ params) {
  __shared__ double part[2][4];
  const int t = threadIdx.x, f = blockIdx.x;
  const float* a = cmp + (size_t)f * cmp_stride + off;
  const float* b = bg + (size_t)(nb == 1 ? 0 : f) * bg_stride + off;
  double sa = 0.0, sb = 0.0;
  for (long i = t; i < count; i += 256) {
    sa += (double)a[i];
    sb += (double)b[i];
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if ((t & 63) == 0) {
    part[0][t >> 6] = sa;
    part[1][t >> 6] = sb;
  }
  __syncthreads();
  if (t == 0) {
    sa = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    sb = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    float* p = params + (size_t)f * PARAM_FLOATS;
#pragma unroll
    for (int i = 0; i < PARAM_FLOATS; ++i) p[i] = 0.f;
    p[6] = sb > 0.0 ? (float)(sa / sb) : 1.f;
  }
}

// the plate level at level position (xl, yl)
__device__ __forceinline__ float sample(const float* __restrict__ P, float xl, float yl, int hk, int wk) {
  const Tap t = tap_at(xl, yl, hk, wk);
  return lerp2(P[t.i00], P[t.i01], P[t.i10], P[t.i11], t.fx, t.fy);
}

__global__ void __launch_bounds__(256)
align_sums_kernel(const float* __restrict__ cmp, long cmp_stride, const float* __restrict__ bg, long bg_stride, int nb,
                  long off, int hk, int wk, float scale, float inv, float cx, float cy, float tol, int bpf,
                  const float* __restrict__ params, double* __restrict__ work) {
  __shared__ double part[4][PART];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, f = blockIdx.x / bpf, bx = blockIdx.x - f * bpf;
  const float* I = cmp + (size_t)f * cmp_stride + off;
  const float* P = bg + (size_t)(nb == 1 ? 0 : f) * bg_stride + off;
  float p[PARAM_FLOATS];
#pragma unroll
  for (int i = 0; i < PARAM_FLOATS; ++i) p[i] = params[(size_t)f * PARAM_FLOATS + i];
  const float g = p[6], close_tol = tol * 0.25f;
  double acc[NSUM];
#pragma unroll
  for (int i = 0; i < NSUM; ++i) acc[i] = 0.0;
  unsigned count = 0u, close = 0u;
  const long pixels = all_finite(p) ? (long)hk * wk : 0;  // (a parameter that is not finite: nothing is summed)
  for (long i = (long)bx * 256 + t; i < pixels; i += (long)bpf * 256) {
    const int y = (int)(i / wk), x = (int)(i - (long)y * wk);
    const float X0 = ((float)x + 0.5f) * scale - 0.5f, Y0 = ((float)y + 0.5f) * scale - 0.5f;
    const float xc = X0 - cx, yc = Y0 - cy;
    const float X = X0 + ((p[0] * xc + p[1] * yc) + p[2]), Y = Y0 + ((p[3] * xc + p[4] * yc) + p[5]);
    const float xl = (X + 0.5f) * inv - 0.5f, yl = (Y + 0.5f) * inv - 0.5f;
    const bool inside = xl >= 0.f && xl <= (float)(wk - 1) && yl >= 0.f && yl <= (float)(hk - 1);
    const float pw = sample(P, xl, yl, hk, wk);
    const float gx = ((sample(P, xl + 1.f, yl, hk, wk) - sample(P, xl - 1.f, yl, hk, wk)) * 0.5f) * inv;
    const float gy = ((sample(P, xl, yl + 1.f, hk, wk) - sample(P, xl, yl - 1.f, hk, wk)) * 0.5f) * inv;
    const float r = I[i] - g * pw;
    const float a = g * gx, b = g * gy;
    const float J[NPAR] = {a * xc, a * yc, a, b * xc, b * yc, b, pw};
    const bool in = inside && fabsf(r) <= tol;
    count += in;
    close += inside && fabsf(r) <= close_tol;
    int e = 0;
#pragma unroll
    for (int u = 0; u < NPAR; ++u)
#pragma unroll
      for (int v = u; v < NPAR; ++v) {
        const float q = J[u] * J[v];
        acc[e++] += in ? (double)q : 0.0;
      }
#pragma unroll
    for (int u = 0; u < NPAR; ++u) {
      const float q = J[u] * r;
      acc[e++] += in ? (double)q : 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < NSUM; ++i) {
    const double s = wave_sum(acc[i]);
    if (lane == 0) part[wave][i] = s;
  }
  const double sc = wave_sum((double)count), sl = wave_sum((double)close);  // (integers below 2^53: exact in any order)
  if (lane == 0) {
    part[wave][I_COUNT] = sc;
    part[wave][I_CLOSE] = sl;
  }
  __syncthreads();
  if (t < PART) {
    const double s = t <= I_CLOSE ? ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t] : 0.0;
    work[((size_t)f * bpf + bx) * PART + t] = s;
  }
}

// sums[e] of the upper triangle: row u, column v >= u
__device__ __forceinline__ int tri(int u, int v) { return u * NPAR - u * (u - 1) / 2 + (v - u); }

__global__ void __launch_bounds__(64)
align_solve_kernel(const double* __restrict__ work, int bpf, long level_pixels, long frame_pixels, int min_share,
                   int last, float cx, float cy, float lim, float* __restrict__ params, int32_t* __restrict__ support) {
  __shared__ double sums[PART], A[NPAR][NPAR], b[NPAR], x[NPAR];  // (thread 0's own: indexed in loops, so not registers)
  const int t = threadIdx.x, f = blockIdx.x;
  if (t <= I_CLOSE) {
    const double* q = work + (size_t)f * bpf * PART + t;
    double s = 0.0;
    for (int b = 0; b < bpf; ++b) s += q[(size_t)b * PART];
    sums[t] = s;
  }
  __syncthreads();
  if (t != 0) return;
  float* p = params + (size_t)f * PARAM_FLOATS;
  const long count = (long)sums[I_COUNT], close = (long)sums[I_CLOSE];
  const bool share = count * min_share >= level_pixels;
  bool solved = share;
  if (share) {
    for (int u = 0; u < NPAR; ++u) {
      for (int v = 0; v < NPAR; ++v) A[u][v] = sums[u <= v ? tri(u, v) : tri(v, u)];
      b[u] = sums[28 + u];
    }
    // Gaussian elimination without pivoting, one rounding per operation; a pivot that is not positive (NaN included)
    // ends it
    for (int i = 0; i < NPAR && solved; ++i) {
      const double piv = A[i][i];
      if (!(piv > 0.0)) {
        solved = false;
        break;
      }
      for (int j = i + 1; j < NPAR; ++j) {
        const double m = A[j][i] / piv;
        for (int k = i; k < NPAR; ++k) A[j][k] = A[j][k] - m * A[i][k];
        b[j] = b[j] - m * b[i];
      }
    }
    if (solved)
      for (int i = NPAR - 1; i >= 0; --i) {
        double s = b[i];
        for (int k = i + 1; k < NPAR; ++k) s = s - A[i][k] * x[k];
        x[i] = s / A[i][i];
      }
  }
  const long sup = solved || !share ? close : 0;
  if (solved)
    for (int i = 0; i < NPAR; ++i) p[i] = (float)((double)p[i] + x[i]);
  support[f] = (int32_t)sup;
  if (!last) return;
  bool keep = sup * min_share >= frame_pixels;
  for (int i = 0; i < NPAR; ++i) keep = keep && isfinite(p[i]);
  for (int c = 0; c < 4 && keep; ++c) {
    const float xc = c & 1 ? cx : -cx, yc = c & 2 ? cy : -cy;
    const float dx = (p[0] * xc + p[1] * yc) + p[2], dy = (p[3] * xc + p[4] * yc) + p[5];
    keep = dx * dx + dy * dy <= lim * lim;
  }
  if (!keep) {
    for (int i = 0; i < PARAM_FLOATS; ++i) p[i] = 0.f;
    p[6] = 1.f;
  }
  p[7] = 0.f;
}

__global__ void __launch_bounds__(256)
align_apply_kernel(const uint8_t* __restrict__ bg, int nb, const float* __restrict__ params, int h, int w, float cx,
                   float cy, int bpf, uint8_t* __restrict__ out) {
  const int f = blockIdx.x / bpf, bx = blockIdx.x - f * bpf;
  const long pixels = (long)h * w;
  const uint8_t* src = bg + (size_t)(nb == 1 ? 0 : f) * pixels * 3;
  uint8_t* dst = out + (size_t)f * pixels * 3;
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) p[i] = params[(size_t)f * PARAM_FLOATS + i];
  for (long i = (long)bx * 256 + threadIdx.x; i < pixels; i += (long)bpf * 256) {
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    const float xc = (float)x - cx, yc = (float)y - cy;
    const float X = (float)x + ((p[0] * xc + p[1] * yc) + p[2]), Y = (float)y + ((p[3] * xc + p[4] * yc) + p[5]);
    const Tap t = tap_at(X, Y, h, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = lerp2((float)src[t.i00 * 3 + c], (float)src[t.i01 * 3 + c], (float)src[t.i10 * 3 + c],
                            (float)src[t.i11 * 3 + c], t.fx, t.fy);
      dst[i * 3 + c] = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
    }
  }
}

bool misaligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

bool shape_in_range(int n, int h, int w, int levels) {
  return n >= 1 && h >= 16 && w >= 16 && levels >= 1 && h <= FLOW_MAX_SIDE && w <= FLOW_MAX_SIDE &&
         (long)n * h * w <= (long)INT_MAX / 3;
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" size_t vm_plate_align_workspace_bytes(int n, int h, int w, int levels) {
  if (!shape_in_range(n, h, w, levels)) return 0;
  return (size_t)n * blocks_per_frame((long)h * w) * PART * sizeof(double);
}

extern "C" int vm_plate_align_fit(const float* cmp_pyr, long cmp_stride, const float* bg_pyr, long bg_stride, int nb,
                                  int n, int h, int w, int levels, int iters, float tol, int min_share, int reach,
                                  float* params, int32_t* support, void* work, void* stream) {
  const char* who = "plate_align_fit";
  if (!cmp_pyr || !bg_pyr || !params || !support || !work)
    return fail(VM_EINVAL, "%s: null pyramids / params / support / work", who);
  if (n < 1 || h < 16 || w < 16) return fail(VM_EINVAL, "%s: n >= 1 frames of at least 16 x 16, got [%d,%d,%d]", who, n, h, w);
  if (levels < 1) return fail(VM_EINVAL, "%s: levels %d (at least 1)", who, levels);
  if (!shape_in_range(n, h, w, levels))
    return fail(VM_EINVAL, "%s: frames up to %d a side and n h w 3 within %d, got [%d,%d,%d]", who, FLOW_MAX_SIDE, INT_MAX,
                n, h, w);
  if (nb != 1 && nb != n) return fail(VM_EINVAL, "%s: %d background pyramids for %d frames (1 or n)", who, nb, n);
  if (iters < 1 || iters > ITERS_MAX) return fail(VM_EINVAL, "%s: iters %d (1..%d)", who, iters, ITERS_MAX);
  if (!(tol > 0.f) || !std::isfinite(tol)) return fail(VM_EINVAL, "%s: tol %g (a positive number)", who, (double)tol);
  if (min_share < 1 || min_share > SHARE_MAX)
    return fail(VM_EINVAL, "%s: min_share %d (1..%d)", who, min_share, SHARE_MAX);
  if (reach < 1 || reach > REACH_MAX) return fail(VM_EINVAL, "%s: reach %d (1..%d)", who, reach, REACH_MAX);
  const Plan p = plan_levels(h, w, levels);
  if (cmp_stride < (long)p.floats || (nb == n && n > 1 && bg_stride < (long)p.floats))
    return fail(VM_EINVAL, "%s: a pyramid is %zu floats, the strides are %ld and %ld", who, p.floats, cmp_stride,
                bg_stride);
  if (misaligned(cmp_pyr, 4) || misaligned(bg_pyr, 4) || misaligned(params, 4) || misaligned(support, 4))
    return fail(VM_EINVAL, "%s: pyramids, params and support must be 4-byte aligned", who);
  if (misaligned(work, 16)) return fail(VM_EINVAL, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* wk = static_cast<double*>(work);
  const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
  const float lim = (float)(h < w ? h : w) / (float)reach;
  const int top = p.n - 1;
  hipLaunchKernelGGL(align_start_kernel, dim3((unsigned)n), dim3(256), 0, st, cmp_pyr, cmp_stride, bg_pyr, bg_stride, nb,
                     (long)p.off[top], (long)p.h[top] * p.w[top], params);
  for (int k = top; k >= 0; --k) {
    const long pixels = (long)p.h[k] * p.w[k];
    const int bpf = blocks_per_frame(pixels);  // (level 0's is the largest: the workspace is sized for it)
    const float scale = (float)(1 << k), inv = 1.f / scale;
    for (int i = 0; i < iters; ++i) {
      hipLaunchKernelGGL(align_sums_kernel, dim3((unsigned)bpf * n), dim3(256), 0, st, cmp_pyr, cmp_stride, bg_pyr,
                         bg_stride, nb, (long)p.off[k], p.h[k], p.w[k], scale, inv, cx, cy, tol, bpf, params, wk);
      hipLaunchKernelGGL(align_solve_kernel, dim3((unsigned)n), dim3(64), 0, st, wk, bpf, pixels, (long)h * w, min_share,
                         (int)(k == 0 && i + 1 == iters), cx, cy, lim, params, support);
    }
  }
  return check_launch(who);
}

extern "C" int vm_plate_align_apply(const uint8_t* bg, int nb, const float* params, int n, int h, int w, uint8_t* out,
                                    void* stream) {
  const char* who = "plate_align_apply";
  if (!bg || !params || !out) return fail(VM_EINVAL, "%s: null bg / params / out", who);
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!shape_ok(n, h, w) || (long)n * h * w > (long)INT_MAX / 3 || h > FLOW_MAX_SIDE || w > FLOW_MAX_SIDE)
    return fail(VM_EINVAL, "%s: frames up to %d a side and n h w 3 within %d, got [%d,%d,%d]", who, FLOW_MAX_SIDE, INT_MAX,
                n, h, w);
  if (nb != 1 && nb != n) return fail(VM_EINVAL, "%s: %d background frames for %d frames (1 or n)", who, nb, n);
  if (misaligned(params, 4)) return fail(VM_EINVAL, "%s: params must be 4-byte aligned", who);
  const size_t len = (size_t)h * w * 3;
  if (overlap(out, n * len, bg, nb * len) || overlap(out, n * len, params, (size_t)n * PARAM_FLOATS * 4))
    return fail(VM_EINVAL, "%s: out must not overlap bg or params", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
  const int bpf = grid_for((long)h * w, 256, 1024);  // (bpf n blocks: at most n h w / 256 + n)
  hipLaunchKernelGGL(align_apply_kernel, dim3((unsigned)bpf * n), dim3(256), 0, st, bg, nb, params, h, w, cx, cy, bpf,
                     out);
  return check_launch(who);
}
