// vm_matte_score: the matting metrics of a predicted matte against ground truth (the definition: include/vmatting.h).
// Per frame SAD, squared error and the Gaussian-gradient error over the trimap's unknown region, and against the frame
// before it the dtSSD and MESSDdt terms.  Every per-pixel term is f32 with nothing contracted (the unit is built with
// -ffp-contract=off and IEEE division / sqrt), so the terms of the numpy restatement (tests/score_ref.py) are matched
// bit for bit; the sums are f64 in a fixed order, so a call gives the same bits every time.
//
// One fused launch and a fold:
//
//   score_kernel  a block of 256 threads takes a 64 x 16 tile of one frame.  It stages the tile of pred and gt with
//       the filters' 4-pixel halo into LDS as unit f32 values (72 x 24 each, coordinates clamped: the replicated
//       border), 16-byte f32 / dword uint8 loads where the plane allows it, else element by element.  The horizontal
//       derivative and smoothing passes of both planes go into four 64 x 24 LDS planes; the vertical passes come out of
//       them: a thread owns one column and 4 rows, reads the 12 rows it needs of a plane once and slides the 9 taps
//       down them in registers.  Lanes of a wave lie along a row in every pass, so each LDS access of a wave is 64
//       consecutive dwords, one per bank, whatever the row stride: the rows need no pad.  The thread then forms every
//       term of its 4 pixels (trimap byte, the previous frame's two values, the flow and the four neighbours of both
//       previous planes come straight from global memory, lanes on consecutive pixels), adds them up in f64, and the
//       block reduces over the wave (__shfl_down, wave64), then over its 4 waves in LDS, to one row of 7 partials.
//   score_fold    per (frame, entry) one block adds the frame's partials in a fixed order.
//
// The tile is 64 x 16 rather than 64 x 32: 38.6 KB of LDS instead of 64.2 KB, so 4 blocks per CU instead of 2; the halo
// rows' share of the horizontal passes grows from 1.25 to 1.5, and the 1080p call was still a fifth faster.
//
// The dtypes of pred and gt, "no trimap", "no previous frame at all" and "no flow" are template arguments; what is left
// inside is uniform per block (frame 0 without prev_*, the vector or scalar staging, grad_map given or not).
#include "vm_common.h"

namespace vm {
namespace {

constexpr int TW = 64, TH = 16, R = 4;            // tile, filter radius
constexpr int SW = TW + 2 * R, SH = TH + 2 * R;   // staged tile: 72 x 24
constexpr int ROWS = TH / 4;                      // rows per thread: wave i takes rows 4 i .. 4 i + 3
constexpr int NSUM = 7;                           // partial sums per block: entries 0..6 of a stats row
constexpr long BLOCKS_MAX = 1l << 23;             // blocks of a launch (256 threads each: within HIP's 2^32 threads)

// G = g / sqrt(sum g^2), D = d / sqrt(sum d^2) of g_i = exp(-i^2 / (2 * 1.4^2)), d_i = -i g_i, i = -4..4, computed in
// float64 and rounded to f32; the centre tap of D is +0
__device__ constexpr float TAP_G[9] = {0.010715649f, 0.0639064f, 0.22881863f, 0.4918805f, 0.63481766f,
                                       0.4918805f, 0.22881863f, 0.0639064f, 0.010715649f};
__device__ constexpr float TAP_D[9] = {0.04329901f, 0.19367121f, 0.46229678f, 0.49688867f, 0.0f,
                                       -0.49688867f, -0.46229678f, -0.19367121f, -0.04329901f};

// the unit value of a stored matte value, and 4 of them from one wide load
__device__ __forceinline__ float unit(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }  // (NaN -> 0)
__device__ __forceinline__ float unit(uint8_t q) { return (float)q / 255.f; }
__device__ __forceinline__ void unit4(const float* p, float* o) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = unit(v.x); o[1] = unit(v.y); o[2] = unit(v.z); o[3] = unit(v.w);
}
__device__ __forceinline__ void unit4(const uint8_t* p, float* o) {
  const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = unit((uint8_t)(v >> (8 * e)));
}
template <typename T>
constexpr int wide_bytes() { return sizeof(T) == 4 ? 16 : 4; }

// the tile of `plane` ([h,w], one frame) at (x0 - R, y0 - R) as unit values into s, coordinates clamped to the image
template <typename T>
__device__ __forceinline__ void stage(const T* __restrict__ plane, float (*s)[SW], int x0, int y0, int h, int w,
                                      bool vec) {
  const int t = threadIdx.x;
  if (vec) {  // w is a multiple of 4 here: a group of 4 lies wholly inside the row or wholly outside
    for (int i = t; i < SH * (SW / 4); i += 256) {
      const int r = i / (SW / 4), q = i - r * (SW / 4);
      const int y = min(max(y0 - R + r, 0), h - 1), x = x0 - R + 4 * q;
      const T* row = plane + (size_t)y * w;
      float v[4];
      if (x >= 0 && x + 4 <= w) {
        unit4(row + x, v);
      } else {
        v[0] = v[1] = v[2] = v[3] = unit(row[x < 0 ? 0 : w - 1]);
      }
      *reinterpret_cast<float4*>(&s[r][4 * q]) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    for (int i = t; i < SH * SW; i += 256) {
      const int r = i / SW, c = i - r * SW;
      const int y = min(max(y0 - R + r, 0), h - 1), x = min(max(x0 - R + c, 0), w - 1);
      s[r][c] = unit(plane[(size_t)y * w + x]);
    }
  }
}

// both horizontal passes of the staged plane s: hd = D along x, hg = G along x, for every staged row
__device__ __forceinline__ void horizontal(const float (*s)[SW], float (*hd)[TW], float (*hg)[TW]) {
  for (int i = threadIdx.x; i < SH * TW; i += 256) {
    const int r = i / TW, c = i % TW;
    float ad = 0.f, ag = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float v = s[r][c + k];
      ad = ad + TAP_D[k] * v;
      ag = ag + TAP_G[k] * v;
    }
    hd[r][c] = ad;
    hg[r][c] = ag;
  }
}

// m = sqrt(gx^2 + gy^2) of the thread's ROWS pixels in column c from row r0 on: gx = G down hd, gy = D down hg
__device__ __forceinline__ void magnitude(const float (*hd)[TW], const float (*hg)[TW], int r0, int c, float* m) {
  float vd[ROWS + 2 * R], vg[ROWS + 2 * R];
#pragma unroll
  for (int j = 0; j < ROWS + 2 * R; ++j) {
    vd[j] = hd[r0 + j][c];
    vg[j] = hg[r0 + j][c];
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    float gx = 0.f, gy = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      gx = gx + TAP_G[k] * vd[i + k];
      gy = gy + TAP_D[k] * vg[i + k];
    }
    m[i] = sqrtf(gx * gx + gy * gy);
  }
}

// part: [n][NSUM][tiles] f64, one column per block
template <typename PT, typename GT, bool TRIMAP, bool TEMPORAL, bool FLOW>
__global__ void __launch_bounds__(256)
score_kernel(const PT* __restrict__ pred, const GT* __restrict__ gt, const uint8_t* __restrict__ trimap,
             const PT* __restrict__ prev_pred, const GT* __restrict__ prev_gt, const float2* __restrict__ backward,
             int h, int w, int tiles_x, int tiles, double* __restrict__ part, float* __restrict__ grad_map,
             bool pred_vec, bool gt_vec) {
  static_assert(TEMPORAL || !FLOW, "the flow term is a temporal term");
  __shared__ __attribute__((aligned(16))) float sa[SH][SW];
  __shared__ __attribute__((aligned(16))) float sg[SH][SW];
  __shared__ float hda[SH][TW], hga[SH][TW], hdg[SH][TW], hgg[SH][TW];
  __shared__ double red[4][NSUM];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x0 = tx * TW, y0 = ty * TH;
  const size_t plane = (size_t)h * w, base = (size_t)frame * plane;

  stage(pred + base, sa, x0, y0, h, w, pred_vec);
  stage(gt + base, sg, x0, y0, h, w, gt_vec);
  __syncthreads();
  horizontal(sa, hda, hga);
  horizontal(sg, hdg, hgg);
  __syncthreads();
  float ma[ROWS], mg[ROWS];
  magnitude(hda, hga, wave * ROWS, lane, ma);
  magnitude(hdg, hgg, wave * ROWS, lane, mg);

  // the frame before this one: frame - 1 of the same arrays, or prev_* for frame 0 (which may be absent)
  const PT* pp = nullptr;
  const GT* pg = nullptr;
  if (TEMPORAL) {
    pp = frame ? pred + base - plane : prev_pred;
    pg = frame ? gt + base - plane : prev_gt;
  }
  const bool temporal = TEMPORAL && pp != nullptr;
  const float xmax = (float)(w - 1), ymax = (float)(h - 1);
  const int x = x0 + lane;
  double sum[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int y = y0 + wave * ROWS + i;
    const bool valid = x < w && y < h;
    const size_t p = valid ? (size_t)y * w + x : 0;  // (no branch around the loads: pixel 0 stands in)
    const float a = sa[wave * ROWS + i + R][lane + R], g = sg[wave * ROWS + i + R][lane + R];
    bool in_region = valid;
    if (TRIMAP) {
      const uint8_t tri = trimap[base + p];
      in_region = valid && tri != 0 && tri != 255;
    }
    const float d = a - g;
    const float sad = fabsf(d), sse = d * d;
    const float dm = ma[i] - mg[i];
    const float grad = dm * dm;
    if (grad_map && valid) grad_map[base + p] = grad;
    const double keep = in_region ? 1.0 : 0.0;
    sum[0] += keep;
    sum[1] += in_region ? (double)sad : 0.0;
    sum[2] += in_region ? (double)sse : 0.0;
    sum[3] += in_region ? (double)grad : 0.0;
    if (temporal) {
      const float a1 = unit(pp[p]), g1 = unit(pg[p]);
      const float dd = (a - a1) - (g - g1);
      sum[4] += in_region ? (double)(dd * dd) : 0.0;
      if (FLOW) {
        const float2 b = backward[base + p];
        const float xs = (float)x + b.x, ys = (float)y + b.y;
        const bool take = in_region && xs >= 0.f && xs <= xmax && ys >= 0.f && ys <= ymax;  // (false for NaN)
        // no branch around the gather either: a pixel that takes no part reads pixel (0, 0) and drops it
        const float xc = take ? xs : 0.f, yc = take ? ys : 0.f;
        const float xf = floorf(xc), yf = floorf(yc);
        const float fx = xc - xf, fy = yc - yf;
        const int xi0 = (int)xf, yi0 = (int)yf, xi1 = min(xi0 + 1, w - 1), yi1 = min(yi0 + 1, h - 1);
        const size_t i00 = (size_t)yi0 * w + xi0, i01 = (size_t)yi0 * w + xi1;
        const size_t i10 = (size_t)yi1 * w + xi0, i11 = (size_t)yi1 * w + xi1;
        const float d00 = unit(pp[i00]) - unit(pg[i00]), d01 = unit(pp[i01]) - unit(pg[i01]);
        const float d10 = unit(pp[i10]) - unit(pg[i10]), d11 = unit(pp[i11]) - unit(pg[i11]);
        const float e00 = d00 * d00, e01 = d01 * d01, e10 = d10 * d10, e11 = d11 * d11;
        const float top = e00 + fx * (e01 - e00), bot = e10 + fx * (e11 - e10);
        const float e = top + fy * (bot - top);
        sum[5] += take ? (double)fabsf(sse - e) : 0.0;
        sum[6] += take ? 1.0 : 0.0;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NSUM; ++j) {
    for (int o = 32; o > 0; o >>= 1) sum[j] += __shfl_down(sum[j], o);
    if (lane == 0) red[wave][j] = sum[j];
  }
  __syncthreads();
  if (t < NSUM) part[((size_t)frame * NSUM + t) * tiles + tile] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// stats[frame][entry] = the sum of the frame's partials of that entry, always in the same order; entry 7 is 0
__global__ void __launch_bounds__(256) score_fold_kernel(const double* __restrict__ part, int tiles,
                                                         double* __restrict__ stats) {
  __shared__ double sh[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int frame = blockIdx.x, entry = blockIdx.y;
  double s = 0.0;
  if (entry < NSUM) {
    const double* col = part + ((size_t)frame * NSUM + entry) * tiles;
    for (int b = t; b < tiles; b += 256) s += col[b];
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) sh[wave] = s;
  __syncthreads();
  if (t == 0) stats[(size_t)frame * 8 + entry] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

struct Shape {
  int tiles_x, tiles;
  long blocks;
};
inline bool shape_of(int n, int h, int w, Shape* s) {
  if (n < 1 || h < 1 || w < 1) return false;
  const long tx = (w + TW - 1) / TW, ty = (h + TH - 1) / TH;
  s->tiles_x = (int)tx;
  s->tiles = (int)(tx * ty);
  s->blocks = tx * ty * n;
  return tx * ty <= BLOCKS_MAX && s->blocks <= BLOCKS_MAX;
}

struct Args {
  const void *pred, *gt, *prev_pred, *prev_gt;
  const uint8_t* trimap;
  const float* backward;
  int h, w;
  Shape s;
  double* part;
  float* grad_map;
  hipStream_t st;
};

template <typename T>
bool wide_ok(const void* p, int w) { return reinterpret_cast<uintptr_t>(p) % wide_bytes<T>() == 0 && w % 4 == 0; }

template <typename PT, typename GT, bool TRIMAP, bool TEMPORAL, bool FLOW>
void launch(const Args& a) {
  hipLaunchKernelGGL((score_kernel<PT, GT, TRIMAP, TEMPORAL, FLOW>), dim3((unsigned)a.s.blocks), dim3(256), 0, a.st,
                     static_cast<const PT*>(a.pred), static_cast<const GT*>(a.gt), a.trimap,
                     static_cast<const PT*>(a.prev_pred), static_cast<const GT*>(a.prev_gt),
                     reinterpret_cast<const float2*>(a.backward), a.h, a.w, a.s.tiles_x, a.s.tiles, a.part, a.grad_map,
                     wide_ok<PT>(a.pred, a.w), wide_ok<GT>(a.gt, a.w));
}

template <typename PT, typename GT>
void launch_flags(const Args& a, bool temporal) {
  const bool tri = a.trimap != nullptr, flow = temporal && a.backward != nullptr;
  if (tri) {
    if (flow) launch<PT, GT, true, true, true>(a);
    else if (temporal) launch<PT, GT, true, true, false>(a);
    else launch<PT, GT, true, false, false>(a);
  } else {
    if (flow) launch<PT, GT, false, true, true>(a);
    else if (temporal) launch<PT, GT, false, true, false>(a);
    else launch<PT, GT, false, false, false>(a);
  }
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" size_t vm_matte_score_workspace_bytes(int n, int h, int w) {
  Shape s;
  if (!shape_of(n, h, w, &s)) return 0;
  return (size_t)s.blocks * NSUM * sizeof(double);
}

extern "C" int vm_matte_score(const void* pred, int pred_dtype, const void* gt, int gt_dtype, const uint8_t* trimap,
                              const void* prev_pred, const void* prev_gt, const float* backward, int n, int h, int w,
                              double* stats, float* grad_map, void* work, void* stream) {
  Args a;
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "matte_score: bad shape [%d,%d,%d]", n, h, w);
  if (!shape_of(n, h, w, &a.s))
    return fail(VM_EINVAL, "matte_score: [%d,%d,%d] exceeds %ld tiles of %d x %d", n, h, w, BLOCKS_MAX, TW, TH);
  if (!pred || !gt || !stats || !work) return fail(VM_EINVAL, "matte_score: null pred / gt / stats / work");
  if ((pred_dtype != VM_F32 && pred_dtype != VM_U8) || (gt_dtype != VM_F32 && gt_dtype != VM_U8))
    return fail(VM_EINVAL, "matte_score: pred and gt are VM_F32 or VM_U8, got dtypes %d and %d", pred_dtype, gt_dtype);
  if (!prev_pred != !prev_gt) return fail(VM_EINVAL, "matte_score: prev_pred and prev_gt go together");
  if (reinterpret_cast<uintptr_t>(backward) % 8) return fail(VM_EINVAL, "matte_score: backward must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(stats) % 8 || reinterpret_cast<uintptr_t>(work) % 8)
    return fail(VM_EINVAL, "matte_score: stats and work must be 8-byte aligned");
  if ((pred_dtype == VM_F32 && (reinterpret_cast<uintptr_t>(pred) % 4 || reinterpret_cast<uintptr_t>(prev_pred) % 4)) ||
      (gt_dtype == VM_F32 && (reinterpret_cast<uintptr_t>(gt) % 4 || reinterpret_cast<uintptr_t>(prev_gt) % 4)) ||
      reinterpret_cast<uintptr_t>(grad_map) % 4)
    return fail(VM_EINVAL, "matte_score: f32 planes must be 4-byte aligned");
  a.pred = pred; a.gt = gt; a.prev_pred = prev_pred; a.prev_gt = prev_gt;
  a.trimap = trimap; a.backward = backward;
  a.h = h; a.w = w;
  a.part = static_cast<double*>(work);
  a.grad_map = grad_map;
  a.st = reinterpret_cast<hipStream_t>(stream);
  const bool temporal = n > 1 || prev_pred;
  if (pred_dtype == VM_F32) {
    if (gt_dtype == VM_F32) launch_flags<float, float>(a, temporal);
    else launch_flags<float, uint8_t>(a, temporal);
  } else {
    if (gt_dtype == VM_F32) launch_flags<uint8_t, float>(a, temporal);
    else launch_flags<uint8_t, uint8_t>(a, temporal);
  }
  hipLaunchKernelGGL(score_fold_kernel, dim3(n, 8), dim3(256), 0, a.st, a.part, a.s.tiles, stats);
  return check_launch("matte_score");
}
