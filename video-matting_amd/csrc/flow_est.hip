// Dense two-frame optical flow on the device (vm_flow_estimate): what ClipStream needs when the caller has no .flo
// files.  Coarse-to-fine Horn-Schunck with warping and Jacobi sweeps; the arithmetic, operation for operation, is in
// include/vmatting.h and restated in numpy by tests/flow_est_ref.py.  All f32, nothing contracted (this unit is built
// with -ffp-contract=off and correctly rounded division), so the result is the restatement's bit for bit.
//
// Every step is a kernel launch on the caller's stream (no memset / memcpy calls: captured in a graph those replayed
// wrongly); the last sweep launch writes the caller's flow.
// Kernels: grey (u8 BGR -> level 0), down (2x2 box mean), smooth (the separable [1/4 1/2 1/4] in one pass: the three
// horizontal sums a pixel's vertical sum needs are recomputed, the same values in the same order), upsample (coarse
// flow -> the next level's start), warp (the previous level warped by the flow at the start of the warp, and from it
// (Ix, Iy, It, den) as one float4 per pixel) and the Jacobi sweep in two forms:
//
//   sweep_kernel        one sweep per launch, one pixel per thread, 8 neighbour loads from global memory.
//   sweep_block_kernel  FT sweeps per launch (temporal blocking).  A 256-thread block owns a TX x TY tile; it stages
//                       the iterate of the tile plus a halo of FT pixels (RW x RH float2) in LDS and keeps each
//                       staged pixel's coefficients (float4) and start-of-warp flow (float2) in registers, PPT pixels
//                       per thread.  Every sweep updates every staged pixel from one LDS buffer into the other (one
//                       barrier per sweep); the last sweep stores the tile's interior to global memory instead.
//
// The halo rule.  A staged pixel's neighbours are found in image coordinates, clamped to the image (the replicate
// border of the *current* iterate, re-applied every sweep exactly as sweep_kernel does) and only then clamped to the
// staged region.  The second clamp reads a wrong neighbour, and it happens only on region edges that are not image
// edges; the error moves inwards one ring per sweep, so after n <= FT sweeps it has not left the halo and the tile's
// interior holds exactly what n single sweeps give.  Staged cells outside the image are never written or read.
//
// LDS layout: 8-byte cells, RW = 64 cells per row.  A lane is a staged column and a wave owns PPT consecutive rows,
// which each thread walks downwards: per row it reads the centre and the left and right neighbour (three 8-byte reads
// of 64 consecutive cells per wave, shifted by at most one: no padding is needed) and forms left + right once; a
// pixel's update takes the centres of the rows above and below and the three rows' sums, which is hs_update's
// additions in hs_update's order.  36 LDS reads per thread and sweep instead of 80.
// 2 x RW x RH x 8 B = 40 KB per block, 3 blocks per CU; 132 VGPRs, no spills.
#include "flow_pyramid.h"
#include "vm_common.h"

namespace vm {

static long g_flow_blocked = 1;  // vm_set_option "flow_blocked": 0 = one sweep per launch (sweep_kernel)
// this file's vm_set_option keys (vm_common.h OptDef)
const OptDef flow_options[] = {
    {"flow_blocked", &g_flow_blocked, OPT_RANGE, 2, {0, 1}},
    {nullptr},
};

namespace {

constexpr int FT = 4;                     // sweeps per blocked launch = halo width
constexpr int TX = 56, TY = 32;           // the tile a block writes (RW = 64: a wave is one staged row)
constexpr int RW = TX + 2 * FT, RH = TY + 2 * FT, RN = RW * RH;  // the staged region
constexpr int PPT = RN / 256;             // staged pixels per thread
static_assert(RW == 64 && RH == 4 * PPT, "a lane is a staged column, a wave PPT staged rows");
constexpr int MAX_SIDE = FLOW_MAX_SIDE;

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// the workspace: [cur pyramid | prev pyramid | unsmoothed pyramid | three flow buffers | coefficients]
struct Work {
  float *cur, *prev, *raw;
  float2* f[3];
  float4* coef;
  size_t bytes;
};

Work carve(void* base, const Plan& p) {
  Work k{};
  char* b = reinterpret_cast<char*>(base);
  const size_t pyr = align256(p.floats * 4), hw = (size_t)p.h[0] * p.w[0];
  size_t o = 0;
  k.cur = reinterpret_cast<float*>(b + o); o += pyr;
  k.prev = reinterpret_cast<float*>(b + o); o += pyr;
  k.raw = reinterpret_cast<float*>(b + o); o += pyr;
  for (int i = 0; i < 3; ++i) { k.f[i] = reinterpret_cast<float2*>(b + o); o += align256(hw * 8); }
  k.coef = reinterpret_cast<float4*>(b + o); o += align256(hw * 16);
  k.bytes = o;
  return k;
}

// ---------------------------------------------------------------- pyramid
__global__ void __launch_bounds__(256) grey_kernel(const uint8_t* __restrict__ bgr, long n, float* __restrict__ g) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int s = 29 * bgr[i * 3] + 150 * bgr[i * 3 + 1] + 77 * bgr[i * 3 + 2];
    g[i] = (float)s / 256.f;
  }
}

__global__ void __launch_bounds__(256) down_kernel(const float* __restrict__ a, int h, int w, float* __restrict__ o,
                                                   int oh, int ow) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= ow || y >= oh) return;
  const int x0 = 2 * x, x1 = min(x0 + 1, w - 1);
  const long r0 = (long)(2 * y) * w, r1 = (long)min(2 * y + 1, h - 1) * w;
  o[(long)y * ow + x] = ((a[r0 + x0] + a[r0 + x1]) + (a[r1 + x0] + a[r1 + x1])) * 0.25f;
}

__global__ void __launch_bounds__(256) smooth_kernel(const float* __restrict__ a, int h, int w, float* __restrict__ o) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  const int xl = max(x - 1, 0), xr = min(x + 1, w - 1);
  const long ru = (long)max(y - 1, 0) * w, rc = (long)y * w, rd = (long)min(y + 1, h - 1) * w;
  const float hu = (a[ru + xl] + a[ru + xr]) * 0.25f + a[ru + x] * 0.5f;
  const float hc = (a[rc + xl] + a[rc + xr]) * 0.25f + a[rc + x] * 0.5f;
  const float hd = (a[rd + xl] + a[rd + xr]) * 0.25f + a[rd + x] * 0.5f;
  o[rc + x] = (hu + hd) * 0.25f + hc * 0.5f;
}

// the coarsest level's start (a kernel, like every step of the estimate: one chain of kernel nodes when captured)
__global__ void __launch_bounds__(256) zero_kernel(float2* __restrict__ f, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) f[i] = make_float2(0.f, 0.f);
}

__global__ void __launch_bounds__(256) upsample_kernel(const float2* __restrict__ c, int ch, int cw,
                                                       float2* __restrict__ f, int h, int w) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  const Tap t = tap_at(((float)x - 0.5f) * 0.5f, ((float)y - 0.5f) * 0.5f, ch, cw);
  const float2 p00 = c[t.i00], p01 = c[t.i01], p10 = c[t.i10], p11 = c[t.i11];
  f[(long)y * w + x] = make_float2(2.f * lerp2(p00.x, p01.x, p10.x, p11.x, t.fx, t.fy),
                                   2.f * lerp2(p00.y, p01.y, p10.y, p11.y, t.fx, t.fy));
}

// ---------------------------------------------------------------- warp + derivatives
// the previous level at (x + u0, y + v0) of pixel (x, y)
__device__ __forceinline__ float warped_at(const float* __restrict__ prev, const float2* __restrict__ flow0, int h,
                                           int w, int x, int y) {
  const float2 f = flow0[(long)y * w + x];
  const Tap t = tap_at((float)x + f.x, (float)y + f.y, h, w);
  return lerp2(prev[t.i00], prev[t.i01], prev[t.i10], prev[t.i11], t.fx, t.fy);
}

__global__ void __launch_bounds__(256) warp_kernel(const float* __restrict__ cur, const float* __restrict__ prev,
                                                   const float2* __restrict__ flow0, int h, int w, float a2,
                                                   float4* __restrict__ coef) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  const float iw = warped_at(prev, flow0, h, w, x, y);
  const float ix = (warped_at(prev, flow0, h, w, min(x + 1, w - 1), y) -
                    warped_at(prev, flow0, h, w, max(x - 1, 0), y)) * 0.5f;
  const float iy = (warped_at(prev, flow0, h, w, x, min(y + 1, h - 1)) -
                    warped_at(prev, flow0, h, w, x, max(y - 1, 0))) * 0.5f;
  const float it = iw - cur[(long)y * w + x];
  coef[(long)y * w + x] = make_float4(ix, iy, it, (a2 + ix * ix) + iy * iy);
}

// ---------------------------------------------------------------- the Jacobi sweep
// one pixel's update from the neighbour means (ub, vb) of the previous iterate; c = (Ix, Iy, It, den), f0 = (u0, v0)
__device__ __forceinline__ float2 hs_solve(float ub, float vb, float4 c, float2 f0) {
  const float r = (c.x * (ub - f0.x) + c.y * (vb - f0.y)) + c.z;
  const float q = r / c.w;
  return make_float2(ub - c.x * q, vb - c.y * q);
}

constexpr float K6 = 1 / 6.f, K12 = 1 / 12.f;

// ... from its 8 neighbours
__device__ __forceinline__ float2 hs_update(float2 up, float2 dn, float2 lf, float2 rt, float2 ul, float2 ur, float2 dl,
                                            float2 dr, float4 c, float2 f0) {
  const float ub = ((up.x + dn.x) + (lf.x + rt.x)) * K6 + ((ul.x + ur.x) + (dl.x + dr.x)) * K12;
  const float vb = ((up.y + dn.y) + (lf.y + rt.y)) * K6 + ((ul.y + ur.y) + (dl.y + dr.y)) * K12;
  return hs_solve(ub, vb, c, f0);
}

// ... from the centres of the rows above and below (up, dn) and the three rows' left + right sums: su = ul + ur,
// sc = lf + rt, sd = dl + dr.  The same additions in the same order as hs_update; a thread walking down a column
// forms each row's sum once and uses it for three pixels.
__device__ __forceinline__ float2 hs_update_rows(float2 up, float2 dn, float2 su, float2 sc, float2 sd, float4 c,
                                                 float2 f0) {
  const float ub = ((up.x + dn.x) + sc.x) * K6 + (su.x + sd.x) * K12;
  const float vb = ((up.y + dn.y) + sc.y) * K6 + (su.y + sd.y) * K12;
  return hs_solve(ub, vb, c, f0);
}

__global__ void __launch_bounds__(256) sweep_kernel(const float2* __restrict__ src, const float2* __restrict__ f0,
                                                    const float4* __restrict__ coef, float2* __restrict__ dst, int h,
                                                    int w) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  const int xl = max(x - 1, 0), xr = min(x + 1, w - 1);
  const long ru = (long)max(y - 1, 0) * w, rc = (long)y * w, rd = (long)min(y + 1, h - 1) * w;
  dst[rc + x] = hs_update(src[ru + x], src[rd + x], src[rc + xl], src[rc + xr], src[ru + xl], src[ru + xr],
                          src[rd + xl], src[rd + xr], coef[rc + x], f0[rc + x]);
}

__global__ void __launch_bounds__(256) sweep_block_kernel(const float2* __restrict__ src, const float2* __restrict__ f0,
                                                          const float4* __restrict__ coef, float2* __restrict__ dst,
                                                          int h, int w, int nsweeps) {
  __shared__ float2 buf[2][RN];
  // lane -> column rx of the region, wave -> its rows ry0 .. ry0 + PPT - 1: a thread walks down its column
  const int rx = threadIdx.x & (RW - 1), ry0 = threadIdx.x / RW * PPT;
  const int ox = blockIdx.x * TX - FT, oy = blockIdx.y * TY - FT;  // the region's origin in the image
  const int x = ox + rx;
  const bool xin = x >= 0 && x < w;
  // image clamp (the replicate border of the current iterate), then region clamp (the halo's outer ring): the
  // neighbour columns of column rx, and the staged rows [lo, hi] a neighbour row is clamped to
  const int xl = max(max(x - 1, 0) - ox, 0), xr = min(min(x + 1, w - 1) - ox, RW - 1);
  const int lo = max(-oy, 0), hi = min(h - 1 - oy, RH - 1);
  float4 c[PPT];
  float2 z[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int ry = ry0 + k;
    c[k] = make_float4(0.f, 0.f, 0.f, 1.f);
    z[k] = make_float2(0.f, 0.f);
    if (xin && ry >= lo && ry <= hi) {
      const long i = (long)(oy + ry) * w + x;
      buf[0][ry * RW + rx] = src[i];
      c[k] = coef[i];
      z[k] = f0[i];
    }
  }
  __syncthreads();
  for (int s = 0; s < nsweeps; ++s) {
    const float2* in = buf[s & 1];
    float2* out = buf[(s + 1) & 1];
    const bool last = s + 1 == nsweeps;
    if (xin) {
      // row j of the column: its centre and its left + right sum (rows outside [lo, hi] are their clamped row)
      auto row = [&](int j, float2& ctr, float2& sum) {
        const int r = min(max(j, lo), hi) * RW;
        const float2 l = in[r + xl], rt = in[r + xr];
        ctr = in[r + rx];
        sum = make_float2(l.x + rt.x, l.y + rt.y);
      };
      float2 cu, su, cc, sc, cd, sd;
      row(ry0 - 1, cu, su);
      row(ry0, cc, sc);
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const int ry = ry0 + k;
        row(ry + 1, cd, sd);
        if (ry >= lo && ry <= hi) {
          const float2 r = hs_update_rows(cu, cd, su, sc, sd, c[k], z[k]);
          if (!last)
            out[ry * RW + rx] = r;
          else if (rx >= FT && rx < FT + TX && ry >= FT && ry < FT + TY)
            dst[(long)(oy + ry) * w + x] = r;
        }
        cu = cc; su = sc;
        cc = cd; sc = sd;
      }
    }
    __syncthreads();
  }
}

dim3 grid2(int h, int w) { return dim3((w + 63) / 64, (h + 3) / 4); }
const dim3 block2(64, 4);

void build_pyramid(const uint8_t* frame, const Plan& p, float* pyr, float* raw, hipStream_t st) {
  const long hw = (long)p.h[0] * p.w[0];
  hipLaunchKernelGGL(grey_kernel, dim3(grid_for(hw, 256, 256 * 32)), dim3(256), 0, st, frame, hw, raw);
  for (int k = 1; k < p.n; ++k)
    hipLaunchKernelGGL(down_kernel, grid2(p.h[k], p.w[k]), block2, 0, st, raw + p.off[k - 1], p.h[k - 1], p.w[k - 1],
                       raw + p.off[k], p.h[k], p.w[k]);
  for (int k = 0; k < p.n; ++k)
    hipLaunchKernelGGL(smooth_kernel, grid2(p.h[k], p.w[k]), block2, 0, st, raw + p.off[k], p.h[k], p.w[k],
                       pyr + p.off[k]);
}

void solve(const float* cur, const float* prev, const Plan& p, int warps, int iters, float alpha, float* flow,
           const Work& wk, hipStream_t st) {
  float2 *a = wk.f[0], *b = wk.f[1], *c = wk.f[2];  // a: the current flow
  const float a2 = alpha * alpha;
  for (int k = p.n - 1; k >= 0; --k) {
    const int h = p.h[k], w = p.w[k];
    if (k == p.n - 1) {
      hipLaunchKernelGGL(zero_kernel, dim3(grid_for((long)h * w, 256)), dim3(256), 0, st, a, (long)h * w);
    } else {
      hipLaunchKernelGGL(upsample_kernel, grid2(h, w), block2, 0, st, a, p.h[k + 1], p.w[k + 1], b, h, w);
      float2* t = a; a = b; b = t;
    }
    for (int i = 0; i < warps; ++i) {
      hipLaunchKernelGGL(warp_kernel, grid2(h, w), block2, 0, st, cur + p.off[k], prev + p.off[k], a, h, w, a2, wk.coef);
      float2* src = a;  // a stays the flow at the start of the warp; the sweeps alternate between b and c
      for (int left = iters; left > 0;) {
        const int n = g_flow_blocked ? (left < FT ? left : FT) : 1;
        // the last launch of the last warp of level 0 writes the caller's flow
        float2* dst = k == 0 && i + 1 == warps && left == n ? reinterpret_cast<float2*>(flow) : src == b ? c : b;
        if (g_flow_blocked) {
          hipLaunchKernelGGL(sweep_block_kernel, dim3((w + TX - 1) / TX, (h + TY - 1) / TY), dim3(256), 0, st, src, a,
                             wk.coef, dst, h, w, n);
          left -= n;
        } else {
          hipLaunchKernelGGL(sweep_kernel, grid2(h, w), block2, 0, st, src, a, wk.coef, dst, h, w);
          --left;
        }
        src = dst;
      }
      if (src == b) { b = a; a = src; } else if (src == c) { c = a; a = src; }
    }
  }
}

int check_shape(const char* who, int h, int w, int levels) {
  if (h < 16 || w < 16) return fail(VM_EINVAL, "%s: frames of at least 16 x 16, got %d x %d", who, h, w);
  if (levels < 1) return fail(VM_EINVAL, "%s: levels %d (at least 1)", who, levels);
  if (h > MAX_SIDE || w > MAX_SIDE) return fail(VM_EUNSUPPORTED, "%s: frames up to %d a side, got %d x %d", who, MAX_SIDE, h, w);
  return VM_OK;
}

int check_solver(const char* who, int warps, int iters, float alpha) {
  if (warps < 1 || iters < 1) return fail(VM_EINVAL, "%s: warps %d and iters %d (both at least 1)", who, warps, iters);
  if (!(alpha > 0.f)) return fail(VM_EINVAL, "%s: alpha %g (a positive number)", who, (double)alpha);
  return VM_OK;
}

bool misaligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" size_t vm_flow_pyramid_bytes(int h, int w, int levels) {
  if (h < 16 || w < 16 || levels < 1 || h > MAX_SIDE || w > MAX_SIDE) return 0;
  return plan_levels(h, w, levels).floats * 4;
}

extern "C" size_t vm_flow_estimate_workspace_bytes(int h, int w, int levels) {
  if (h < 16 || w < 16 || levels < 1 || h > MAX_SIDE || w > MAX_SIDE) return 0;
  return carve(nullptr, plan_levels(h, w, levels)).bytes;
}

extern "C" int vm_flow_pyramid(const uint8_t* frame, int h, int w, int levels, float* pyr, void* work, void* stream) {
  if (!frame || !pyr || !work) return fail(VM_EINVAL, "flow_pyramid: null frame / pyramid / workspace");
  if (int rc = check_shape("flow_pyramid", h, w, levels)) return rc;
  if (misaligned(pyr, 16) || misaligned(work, 16))
    return fail(VM_EUNSUPPORTED, "flow_pyramid: the pyramid and the workspace are 16-byte aligned");
  const Plan p = plan_levels(h, w, levels);
  build_pyramid(frame, p, pyr, carve(work, p).raw, reinterpret_cast<hipStream_t>(stream));
  return check_launch("flow_pyramid");
}

extern "C" int vm_flow_from_pyramids(const float* cur, const float* prev, int h, int w, int levels, int warps,
                                     int iters, float alpha, float* flow, void* work, void* stream) {
  if (!cur || !prev || !flow || !work) return fail(VM_EINVAL, "flow_from_pyramids: null pyramid / flow / workspace");
  if (int rc = check_shape("flow_from_pyramids", h, w, levels)) return rc;
  if (int rc = check_solver("flow_from_pyramids", warps, iters, alpha)) return rc;
  if (misaligned(cur, 16) || misaligned(prev, 16) || misaligned(work, 16) || misaligned(flow, 8))
    return fail(VM_EUNSUPPORTED, "flow_from_pyramids: pyramids and workspace 16-byte, the flow 8-byte aligned");
  const Plan p = plan_levels(h, w, levels);
  solve(cur, prev, p, warps, iters, alpha, flow, carve(work, p), reinterpret_cast<hipStream_t>(stream));
  return check_launch("flow_from_pyramids");
}

extern "C" int vm_flow_estimate(const uint8_t* cur, const uint8_t* prev, int h, int w, int levels, int warps,
                                int iters, float alpha, float* flow, void* work, void* stream) {
  if (!cur || !prev || !flow || !work) return fail(VM_EINVAL, "flow_estimate: null frame / flow / workspace");
  if (int rc = check_shape("flow_estimate", h, w, levels)) return rc;
  if (int rc = check_solver("flow_estimate", warps, iters, alpha)) return rc;
  if (misaligned(work, 16) || misaligned(flow, 8))
    return fail(VM_EUNSUPPORTED, "flow_estimate: the workspace is 16-byte, the flow 8-byte aligned");
  const Plan p = plan_levels(h, w, levels);
  const Work wk = carve(work, p);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  build_pyramid(cur, p, wk.cur, wk.raw, st);
  build_pyramid(prev, p, wk.prev, wk.raw, st);
  solve(wk.cur, wk.prev, p, warps, iters, alpha, flow, wk, st);
  return check_launch("flow_estimate");
}
