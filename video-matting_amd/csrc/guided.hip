// Guided matte upsampling (the definitions: include/vmatting.h): run the model on frames reduced by s = 2..4 and carry
// its matte back to full resolution with a guided filter steered by the full-resolution frame (He & Sun, "Fast Guided
// Filter").  Three calls, every kernel in this unit:
//
//   vm_frames_reduce_u8  uint8 frames -> the model's resolution: block means (BGR) or block agreement (trimaps).
//   vm_guided_coeffs     per low-resolution pixel the linear model alpha ~ a . I + b over its window, then the box mean
//                        of (a, b).  Two launches over 32 x 8 tiles staged in LDS with their halo.
//   vm_guided_apply      alpha = clamp(a . I + b) per full-resolution pixel, (a, b) interpolated bilinearly.
//
// The unit is built with -ffp-contract=off and IEEE division: the apply's f32 arithmetic is fixed operation by
// operation and tests/guided_ref.py restates it in numpy to the bit; the reductions are integer.
//
// Byte rows at any address are read with whole dwords.  A thread that needs the L bytes (L a multiple of 4) at address
// A = 4 q + k reads the aligned dwords q .. q + L / 4 (the last one only when k != 0) and shifts each pair right by k
// bytes.  Every dword it reads holds at least one byte of the span, and an aligned dword never straddles a page, so
// the up to 3 bytes before and after the span are read from wherever the span's own first and last bytes live.
#include "vm_common.h"

namespace vm {
namespace {

constexpr int SCALE_MIN = 2, SCALE_MAX = 4;

// ---------------------------------------------------------------- vm_frames_reduce_u8
// One thread makes P consecutive output pixels of one output row: P C = 12 (BGR) or 16 (trimap) bytes, stored as dwords
// when the output address allows it.  Where its P blocks are whole in x it reads each of the block's rows as P S C / 4
// dwords (load_bytes); the ragged last thread of a row goes byte by byte.  A short last block row only changes the row
// count (and cnt).  TRI: the block's byte if all agree, else 128; otherwise (2 sum + cnt) / (2 cnt).
template <int S, int C, int P, bool TRI>
__global__ void __launch_bounds__(256)
reduce_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int hm, int wm, int tcols,
              long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long row = idx / tcols;  // frame * hm + Y
  const int tc = (int)(idx - row * tcols);
  const int frame = (int)(row / hm), Y = (int)(row - (long)frame * hm);
  const int X0 = tc * P;
  const int rows = min(S, h - S * Y);
  const size_t pitch = (size_t)w * C;
  const uint8_t* in = src + ((size_t)frame * h + (size_t)S * Y) * pitch;
  uint8_t* out = dst + ((size_t)row * wm + X0) * C;
  if ((long)(X0 + P) * S <= w) {
    constexpr int ND = P * S * C / 4;
    uint32_t lo[P * C], hi[P * C];  // mean: lo is the sum; trimap: the smallest and the largest byte
#pragma unroll
    for (int e = 0; e < P * C; ++e) {
      lo[e] = TRI ? 255u : 0u;
      hi[e] = 0u;
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (j < rows) {
        uint32_t d[ND];
        load_bytes<ND>(in + j * pitch + (size_t)X0 * S * C, d);
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int ch = 0; ch < C; ++ch)
#pragma unroll
            for (int i = 0; i < S; ++i) {
              const uint32_t v = byte_of(d, (p * S + i) * C + ch);
              if (TRI) {
                lo[p * C + ch] = min(lo[p * C + ch], v);
                hi[p * C + ch] = max(hi[p * C + ch], v);
              } else {
                lo[p * C + ch] += v;
              }
            }
      }
    }
    uint32_t o[P * C / 4];
#pragma unroll
    for (int e = 0; e < P * C / 4; ++e) o[e] = 0u;
    const uint32_t cnt = (uint32_t)rows * S;
#pragma unroll
    for (int e = 0; e < P * C; ++e) {
      uint32_t v;
      if (TRI) v = lo[e] == hi[e] ? lo[e] : 128u;
      else if (rows == S) v = (2u * lo[e] + S * S) / (2u * S * S);
      else v = (2u * lo[e] + cnt) / (2u * cnt);
      o[e >> 2] |= v << (8 * (e & 3));
    }
    if ((reinterpret_cast<uintptr_t>(out) & 3) == 0) {
#pragma unroll
      for (int e = 0; e < P * C / 4; ++e) reinterpret_cast<uint32_t*>(out)[e] = o[e];
    } else {
#pragma unroll
      for (int e = 0; e < P * C; ++e) out[e] = (uint8_t)(o[e >> 2] >> (8 * (e & 3)));
    }
    return;
  }
  for (int p = 0; p < P && X0 + p < wm; ++p) {
    const int xs = (X0 + p) * S, bw = min(S, w - xs);
    const uint32_t cnt = (uint32_t)rows * bw;
    for (int ch = 0; ch < C; ++ch) {
      uint32_t sum = 0u, mn = 255u, mx = 0u;
      for (int j = 0; j < rows; ++j)
        for (int i = 0; i < bw; ++i) {
          const uint32_t v = in[j * pitch + (size_t)(xs + i) * C + ch];
          sum += v;
          mn = min(mn, v);
          mx = max(mx, v);
        }
      out[p * C + ch] = (uint8_t)(TRI ? (mn == mx ? mn : 128u) : (2u * sum + cnt) / (2u * cnt));
    }
  }
}

template <int S, int C, int P, bool TRI>
void launch_reduce(const uint8_t* src, uint8_t* dst, int n, int h, int w, int hm, int wm, hipStream_t st) {
  const int tcols = (wm + P - 1) / P;
  const long total = (long)n * hm * tcols;
  hipLaunchKernelGGL((reduce_kernel<S, C, P, TRI>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, dst, h,
                     w, hm, wm, tcols, total);
}

// ---------------------------------------------------------------- vm_guided_coeffs
constexpr int CTW = 32, CTH = 8, RMAX = 8;                 // tile of low-resolution pixels (one per thread), radius bound
constexpr int CSW = CTW + 2 * RMAX, CSH = CTH + 2 * RMAX;  // staged tile at the largest radius: 48 x 24

// The unaveraged (a, b) of every pixel of the tile.  The guide's moments are integers: S_I (3), S_II (6) and
// M = N S_II - S_I S_I^T (int64) are exact, so Sigma = M / (255 N)^2 + eps 1 has one rounding per entry; the moments
// with p and the solve (an LDL^T factorisation, backward stable: the cofactor form is not at conditioning 1 / eps) are
// f64.  Pixels outside the image are staged as zeros and never read: every thread loops over its clipped window.
__global__ void __launch_bounds__(256)
coeffs_kernel(const uint8_t* __restrict__ g, const float* __restrict__ p, float4* __restrict__ raw, int hm, int wm, int r,
              double eps) {
  __shared__ uint32_t sg[CSH][CSW];
  __shared__ float sp[CSH][CSW];
  const int t = threadIdx.x;
  const int tx0 = blockIdx.x * CTW, ty0 = blockIdx.y * CTH;
  const size_t base = (size_t)blockIdx.z * hm * wm;
  const int sw = CTW + 2 * r, sh = CTH + 2 * r;
  for (int i = t; i < sw * sh; i += 256) {
    const int rr = i / sw, cc = i - rr * sw;
    const int y = ty0 - r + rr, x = tx0 - r + cc;
    uint32_t gv = 0u;
    float pv = 0.f;
    if (y >= 0 && y < hm && x >= 0 && x < wm) {
      const size_t px = base + (size_t)y * wm + x;
      const uint8_t* q = g + px * 3;
      gv = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
      pv = p[px];
    }
    sg[rr][cc] = gv;
    sp[rr][cc] = pv;
  }
  __syncthreads();
  const int x = tx0 + (t & (CTW - 1)), y = ty0 + t / CTW;
  if (x >= wm || y >= hm) return;
  const int ylo = max(y - r, 0), yhi = min(y + r, hm - 1), xlo = max(x - r, 0), xhi = min(x + r, wm - 1);
  uint32_t s1[3] = {0u, 0u, 0u}, s2[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // S_II: 00 01 02 11 12 22
  double sp1 = 0.0, sip[3] = {0.0, 0.0, 0.0};
  for (int yy = ylo; yy <= yhi; ++yy)
    for (int xx = xlo; xx <= xhi; ++xx) {
      const uint32_t gv = sg[yy - ty0 + r][xx - tx0 + r];
      const double pv = (double)sp[yy - ty0 + r][xx - tx0 + r];
      const uint32_t c0 = gv & 255u, c1 = (gv >> 8) & 255u, c2 = gv >> 16;
      s1[0] += c0; s1[1] += c1; s1[2] += c2;
      s2[0] += c0 * c0; s2[1] += c0 * c1; s2[2] += c0 * c2;
      s2[3] += c1 * c1; s2[4] += c1 * c2; s2[5] += c2 * c2;
      sp1 += pv;
      sip[0] += (double)c0 * pv; sip[1] += (double)c1 * pv; sip[2] += (double)c2 * pv;
    }
  const long N = (long)(yhi - ylo + 1) * (xhi - xlo + 1);
  const double dn = (double)N, d2 = dn * dn * 65025.0, d1 = dn * dn * 255.0;
  auto cov = [&](int e, int i, int j) { return (double)(N * (long)s2[e] - (long)s1[i] * (long)s1[j]) / d2; };
  const double m00 = cov(0, 0, 0) + eps, m01 = cov(1, 0, 1), m02 = cov(2, 0, 2);
  const double m11 = cov(3, 1, 1) + eps, m12 = cov(4, 1, 2), m22 = cov(5, 2, 2) + eps;
  double c[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = (dn * sip[i] - (double)s1[i] * sp1) / d1;
  // Sigma = L D L^T, then L z = c, D w = z, L^T a = w
  const double l10 = m01 / m00, l20 = m02 / m00;
  const double e1 = m11 - l10 * m01;
  const double l21 = (m12 - l20 * m01) / e1;
  const double e2 = m22 - l20 * m02 - l21 * (l21 * e1);
  const double z0 = c[0], z1 = c[1] - l10 * z0, z2 = c[2] - l20 * z0 - l21 * z1;
  const double a2 = z2 / e2;
  const double a1 = z1 / e1 - l21 * a2;
  const double a0 = z0 / m00 - l10 * a1 - l20 * a2;
  const double mi = 255.0 * dn;
  const double b = sp1 / dn - (a0 * ((double)s1[0] / mi) + a1 * ((double)s1[1] / mi) + a2 * ((double)s1[2] / mi));
  raw[base + (size_t)y * wm + x] = make_float4((float)a0, (float)a1, (float)a2, (float)b);
}

// ab = the mean of the unaveraged (a, b) over the same clipped window: f64 sums, one rounding
__global__ void __launch_bounds__(256)
box_kernel(const float4* __restrict__ raw, float4* __restrict__ ab, int hm, int wm, int r) {
  __shared__ float4 s[CSH][CSW];
  const int t = threadIdx.x;
  const int tx0 = blockIdx.x * CTW, ty0 = blockIdx.y * CTH;
  const size_t base = (size_t)blockIdx.z * hm * wm;
  const int sw = CTW + 2 * r, sh = CTH + 2 * r;
  for (int i = t; i < sw * sh; i += 256) {
    const int rr = i / sw, cc = i - rr * sw;
    const int y = ty0 - r + rr, x = tx0 - r + cc;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < hm && x >= 0 && x < wm) v = raw[base + (size_t)y * wm + x];
    s[rr][cc] = v;
  }
  __syncthreads();
  const int x = tx0 + (t & (CTW - 1)), y = ty0 + t / CTW;
  if (x >= wm || y >= hm) return;
  const int ylo = max(y - r, 0), yhi = min(y + r, hm - 1), xlo = max(x - r, 0), xhi = min(x + r, wm - 1);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int yy = ylo; yy <= yhi; ++yy)
    for (int xx = xlo; xx <= xhi; ++xx) {
      const float4 v = s[yy - ty0 + r][xx - tx0 + r];
      acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
    }
  const double dn = (double)((long)(yhi - ylo + 1) * (xhi - xlo + 1));
  ab[base + (size_t)y * wm + x] =
      make_float4((float)(acc[0] / dn), (float)(acc[1] / dn), (float)(acc[2] / dn), (float)(acc[3] / dn));
}

// ---------------------------------------------------------------- vm_guided_apply
// A block of 4 waves takes a 256 x 64 tile of full-resolution pixels: a lane owns 4 consecutive pixels of a column
// strip (12 bytes of the frame in through load_bytes, one 16-byte store where the row's address allows it) and its wave
// walks 16 rows down the strip.  The strip's four fx weights and texel columns are computed once per lane, the tile's
// fy weights and texel rows once per block into LDS: the row loop has no division.  The horizontally interpolated
// (a, b) of a texel row is kept in registers for as long as rows use it, and the lower row of one step is the upper row
// of the next, so a texel row is read (16-byte loads, neighbouring lanes on neighbouring texels: L1 / L2 hits) and
// interpolated once per wave per strip instead of once per pixel.
constexpr int AP = 4, ATW = 64 * AP, ATR = 16, ATH = 4 * ATR;

// the texel below coordinate i of `lim` texels and the weight of the next one:
// f = (i + 0.5f) / s - 0.5f clamped to [0, lim - 1]
__device__ __forceinline__ void texel(int i, int s, int lim, int* i0, float* t) {
  float f = ((float)i + 0.5f) / (float)s - 0.5f;
  f = fminf(fmaxf(f, 0.f), (float)(lim - 1));
  const float fl = floorf(f);
  *i0 = (int)fl;
  *t = f - fl;
}

// float(u) / 255.0f, correctly rounded, without the division: one Newton step on u * fl(1 / 255) gives the quotient's
// f32 rounding for every u in 0..255 (checked exhaustively against exact rationals; tests/test_gpu_guided.py compares
// every byte value with numpy's division)
__device__ __forceinline__ float unit255(uint32_t u) {
  const float x = (float)u, rc = 1.f / 255.f;
  const float q = x * rc;
  return fmaf(fmaf(-q, 255.f, x), rc, q);
}

// dst[i][k] = u + tx (v - u) for the lane's AP pixels, u and v the texels x0[i] and x1[i] of `row`
__device__ __forceinline__ void texel_row(const float4* __restrict__ row, const int* x0, const int* x1, const float* tx,
                                          float (*dst)[4]) {
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const float4 u = row[x0[i]], v = row[x1[i]];
    dst[i][0] = u.x + tx[i] * (v.x - u.x);
    dst[i][1] = u.y + tx[i] * (v.y - u.y);
    dst[i][2] = u.z + tx[i] * (v.z - u.z);
    dst[i][3] = u.w + tx[i] * (v.w - u.w);
  }
}

template <int S>
__global__ void __launch_bounds__(256)
apply_kernel(const float4* __restrict__ ab, const uint8_t* __restrict__ cmp, float* __restrict__ alpha, int h, int w,
             int hm, int wm) {
  __shared__ int s_y0[ATH];
  __shared__ float s_ty[ATH];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int frame = blockIdx.z, ytile = blockIdx.y * ATH;
  if (t < ATH) {
    int i0;
    float f;
    texel(ytile + t, S, hm, &i0, &f);
    s_y0[t] = i0;
    s_ty[t] = f;
  }
  __syncthreads();
  const int x = blockIdx.x * ATW + lane * AP;
  if (x >= w) return;
  int x0[AP], x1[AP];
  float tx[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    texel(x + i, S, wm, &x0[i], &tx[i]);
    x1[i] = min(x0[i] + 1, wm - 1);
  }
  const bool full = x + AP <= w;
  const float4* tex = ab + (size_t)frame * hm * wm;
  float top[AP][4], bot[AP][4];
  int c0 = -1, c1 = -1;  // the texel rows top and bot hold
  const int ybeg = ytile + wave * ATR, yend = min(ybeg + ATR, h);
  for (int y = ybeg; y < yend; ++y) {
    const int y0 = __builtin_amdgcn_readfirstlane(s_y0[y - ytile]), y1 = min(y0 + 1, hm - 1);
    const float ty = s_ty[y - ytile];
    if (y0 != c0) {
      if (y0 == c1) {
#pragma unroll
        for (int i = 0; i < AP; ++i)
#pragma unroll
          for (int k = 0; k < 4; ++k) top[i][k] = bot[i][k];
      } else {
        texel_row(tex + (size_t)y0 * wm, x0, x1, tx, top);
      }
      c0 = y0;
    }
    if (y1 != c1) {
      if (y1 == c0) {
#pragma unroll
        for (int i = 0; i < AP; ++i)
#pragma unroll
          for (int k = 0; k < 4; ++k) bot[i][k] = top[i][k];
      } else {
        texel_row(tex + (size_t)y1 * wm, x0, x1, tx, bot);
      }
      c1 = y1;
    }
    const size_t px = ((size_t)frame * h + y) * w + x;
    const uint8_t* in = cmp + px * 3;
    uint32_t d[3] = {0u, 0u, 0u};
    if (full) {
      load_bytes<3>(in, d);
    } else {
#pragma unroll
      for (int e = 0; e < 3 * AP; ++e)
        if (e < 3 * (w - x)) d[e >> 2] |= (uint32_t)in[e] << (8 * (e & 3));
    }
    float q[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      float m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = top[i][k] + ty * (bot[i][k] - top[i][k]);
      const float i0 = unit255(byte_of(d, 3 * i)), i1 = unit255(byte_of(d, 3 * i + 1)),
                  i2 = unit255(byte_of(d, 3 * i + 2));
      const float v = ((m[0] * i0 + m[1] * i1) + m[2] * i2) + m[3];
      q[i] = fminf(fmaxf(v, 0.f), 1.f);
    }
    float* out = alpha + px;
    if (full && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
      *reinterpret_cast<float4*>(out) = make_float4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
      for (int i = 0; i < AP; ++i)
        if (x + i < w) out[i] = q[i];
    }
  }
}

inline bool shape_ok(int n, int h, int w, int c) {
  return n >= 1 && h >= 1 && w >= 1 && (long)n * h * w * c <= 2147483647l;
}
inline int reduced(int v, int s) { return (v + s - 1) / s; }
constexpr int GRID_MAX = 65535;  // blocks along y and z

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" int vm_frames_reduce_u8(const uint8_t* src, int n, int h, int w, int c, int scale, int kind, uint8_t* dst,
                                   void* stream) {
  const char* who = "frames_reduce_u8";
  if (!src || !dst) return fail(VM_EINVAL, "%s: null src / dst", who);
  if (scale < SCALE_MIN || scale > SCALE_MAX) return fail(VM_EINVAL, "%s: scale must be 2, 3 or 4, got %d", who, scale);
  if (kind != VM_REDUCE_MEAN && kind != VM_REDUCE_TRIMAP) return fail(VM_EINVAL, "%s: unknown kind %d", who, kind);
  if (c != (kind == VM_REDUCE_MEAN ? 3 : 1))
    return fail(VM_EINVAL, "%s: kind mean takes c = 3 and kind trimap c = 1, got c = %d", who, c);
  if (!shape_ok(n, h, w, c)) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d,%d]", who, n, h, w, c);
  const int hm = reduced(h, scale), wm = reduced(w, scale);
  if (overlap(src, (size_t)n * h * w * c, dst, (size_t)n * hm * wm * c))
    return fail(VM_EINVAL, "%s: dst overlaps src", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (kind == VM_REDUCE_MEAN) {
    if (scale == 2) launch_reduce<2, 3, 4, false>(src, dst, n, h, w, hm, wm, st);
    else if (scale == 3) launch_reduce<3, 3, 4, false>(src, dst, n, h, w, hm, wm, st);
    else launch_reduce<4, 3, 4, false>(src, dst, n, h, w, hm, wm, st);
  } else {
    if (scale == 2) launch_reduce<2, 1, 16, true>(src, dst, n, h, w, hm, wm, st);
    else if (scale == 3) launch_reduce<3, 1, 16, true>(src, dst, n, h, w, hm, wm, st);
    else launch_reduce<4, 1, 16, true>(src, dst, n, h, w, hm, wm, st);
  }
  return check_launch(who);
}

extern "C" size_t vm_guided_workspace_bytes(int n, int hm, int wm) {
  if (!shape_ok(n, hm, wm, 4) || n > GRID_MAX || hm > GRID_MAX * CTH) return 0;
  return (size_t)n * hm * wm * sizeof(float4);
}

extern "C" int vm_guided_coeffs(const uint8_t* guide, const float* p, int n, int hm, int wm, int r, double eps,
                                float* ab, void* work, void* stream) {
  const char* who = "guided_coeffs";
  if (!guide || !p || !ab || !work) return fail(VM_EINVAL, "%s: null guide / p / ab / work", who);
  if (!shape_ok(n, hm, wm, 4) || n > GRID_MAX || hm > GRID_MAX * CTH)
    return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, hm, wm);
  if (r < 1 || r > RMAX) return fail(VM_EINVAL, "%s: r must be in 1..%d, got %d", who, RMAX, r);
  if (!(eps >= 1e-5 && eps <= 1.0)) return fail(VM_EINVAL, "%s: eps must be in [1e-5, 1], got %g", who, eps);
  if (reinterpret_cast<uintptr_t>(p) % 4) return fail(VM_EINVAL, "%s: p must be 4-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(ab) % 16 || reinterpret_cast<uintptr_t>(work) % 16)
    return fail(VM_EINVAL, "%s: ab and work must be 16-byte aligned", who);
  const size_t px = (size_t)n * hm * wm;
  if (overlap(ab, px * 16, work, px * 16) || overlap(ab, px * 16, guide, px * 3) || overlap(ab, px * 16, p, px * 4) ||
      overlap(work, px * 16, guide, px * 3) || overlap(work, px * 16, p, px * 4))
    return fail(VM_EINVAL, "%s: ab and work overlap each other or an input", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((wm + CTW - 1) / CTW, (hm + CTH - 1) / CTH, n);
  hipLaunchKernelGGL(coeffs_kernel, grid, dim3(256), 0, st, guide, p, static_cast<float4*>(work), hm, wm, r, eps);
  hipLaunchKernelGGL(box_kernel, grid, dim3(256), 0, st, static_cast<const float4*>(work),
                     reinterpret_cast<float4*>(ab), hm, wm, r);
  return check_launch(who);
}

extern "C" int vm_guided_apply(const float* ab, const uint8_t* cmp, int n, int h, int w, int scale, float* alpha,
                               void* stream) {
  const char* who = "guided_apply";
  if (!ab || !cmp || !alpha) return fail(VM_EINVAL, "%s: null ab / cmp / alpha", who);
  if (scale < SCALE_MIN || scale > SCALE_MAX) return fail(VM_EINVAL, "%s: scale must be 2, 3 or 4, got %d", who, scale);
  if (!shape_ok(n, h, w, 4) || n > GRID_MAX || h > GRID_MAX * ATH)
    return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (reinterpret_cast<uintptr_t>(ab) % 16) return fail(VM_EINVAL, "%s: ab must be 16-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(alpha) % 4) return fail(VM_EINVAL, "%s: alpha must be 4-byte aligned", who);
  const int hm = reduced(h, scale), wm = reduced(w, scale);
  const size_t px = (size_t)n * h * w;
  if (overlap(alpha, px * 4, ab, (size_t)n * hm * wm * 16) || overlap(alpha, px * 4, cmp, px * 3))
    return fail(VM_EINVAL, "%s: alpha overlaps an input", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((w + ATW - 1) / ATW, (h + ATH - 1) / ATH, n);
  const float4* tex = reinterpret_cast<const float4*>(ab);
  if (scale == 2) hipLaunchKernelGGL(apply_kernel<2>, grid, dim3(256), 0, st, tex, cmp, alpha, h, w, hm, wm);
  else if (scale == 3) hipLaunchKernelGGL(apply_kernel<3>, grid, dim3(256), 0, st, tex, cmp, alpha, h, w, hm, wm);
  else hipLaunchKernelGGL(apply_kernel<4>, grid, dim3(256), 0, st, tex, cmp, alpha, h, w, hm, wm);
  return check_launch(who);
}
