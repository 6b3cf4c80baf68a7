// vm_trimap_from_plate: a trimap from the difference between a frame and its background plate (the definition:
// include/vmatting.h).  Integer arithmetic only, so the numpy restatement (tests/trimap_plate_ref.py) is matched byte
// for byte.  Two launches, the shape of trimap_prop.hip's class map:
//
//   candidates  per pixel the squared colour distance d to the plate, its 3 x 3 box sum D (replicated border) and the
//       two thresholds, kept as bit rows in `work`: per frame, row and 64 pixels one {background, foreground} pair of
//       64-bit words (16 bytes, 0.25 B per pixel), rows padded to 64 pixels, bit i of a word its pixel i; the pad bits
//       are set in both words (pixels outside the image do not erode).  A block takes 256 x 16 pixels.  The 3-byte
//       pixels of a row are contiguous, so the rows of both planes are read as dwords (the row's first byte rounded
//       down to 4; bytewise for a plane that is not 4-byte aligned and for the plane's last, partial dword), PLANE_BATCH
//       rows of both planes in flight per thread, and unpacked from LDS into a tile of d with a 1-pixel halo, whose
//       border entries are the clamped pixels: every box sum is then 9 plain terms.  One thread per column walks its 16
//       rows with the three row sums in registers; a wave is one word, its two ballots one 16-byte store.  For
//       vm_trimap_from_plate_shadow the tile holds the shadow-tolerant d' (shadow_distance below) in place of d: the
//       SHADOW instantiation, which differs in that one value only.
//   erode and emit  a block takes 128 x 32 pixels with a halo of max(r_bg, r_fg) rows and one word each side (r <= 32 <
//       64) in LDS.  Row erosion is shifts and ANDs across the left, middle and right word, column erosion an AND down
//       2 r + 1 rows, each class with its own radius; words and rows outside the image are all ones.  Every thread then
//       turns 16 bits of each class into 16 result bytes: one 16-byte store where the address allows it, bytewise at a
//       row's ragged end and where the row does not start on 16 bytes.
//
// 7.5 B per pixel all told (6 read, 1 written, 0.25 written and read back); at 1080p that is 16 MB per frame, so a
// single frame waits for latency, not bandwidth, which is why the plane loads are batched.
#include "vm_common.h"

#include <climits>

namespace vm {
namespace {

constexpr int R_MAX = 32, LEVEL_MAX = 442;        // 442^2 >= 3 * 255^2: no distance reaches beyond it
constexpr int SHADOW_ONE = 256;                   // floor and ceil are light ratios in 1/256
constexpr int CAND_WORDS = 4, CAND_COLS = CAND_WORDS * 64, CAND_ROWS = 16;
constexpr int CAND_HALO = CAND_ROWS + 2, PLANE_BATCH = 6;
static_assert(CAND_HALO % PLANE_BATCH == 0, "the halo rows are staged in whole batches");
// the dwords that cover a row segment of CAND_COLS + 2 pixels starting at any byte of a dword
constexpr int SEG_DWORDS = ((CAND_COLS + 2) * 3 + 3 + 3) / 4;
static_assert(SEG_DWORDS <= 256, "one dword of a row segment per thread");
constexpr int ERODE_WORDS = 2, ERODE_ROWS = 32, ERODE_HALO = ERODE_ROWS + 2 * R_MAX;
static_assert(ERODE_ROWS * ERODE_WORDS * 64 == 256 * 16, "16 result bytes per thread");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the 4 bytes of plane p from byte `off` on (off a multiple of 4), in two steps.  plane_dword: the dword itself where
// it lies wholly in the plane; any other thread reads the plane's first dword (no branch around the load, so that a
// batch of them is in flight together).  plane_tail, after the batch: the plane's last dword when its size is no
// multiple of 4, byte by byte, bytes from `total` on as 0.  A plane that is not 4-byte aligned takes only the second.
template <bool VEC>
__device__ __forceinline__ uint32_t plane_dword(const uint8_t* __restrict__ p, size_t off, size_t total, bool active) {
  if (!VEC) return 0;
  return *reinterpret_cast<const uint32_t*>(p + (active && off + 4 <= total ? off : 0));
}

template <bool VEC>
__device__ __forceinline__ uint32_t plane_tail(const uint8_t* __restrict__ p, size_t off, size_t total, bool active,
                                               uint32_t v) {
  if (!active || (VEC && off + 4 <= total)) return v;
  v = 0;
  for (int k = 0; k < 4; ++k)
    if (off + k < total) v |= (uint32_t)p[off + k] << (8 * k);
  return v;
}

// the shadow-tolerant distance d' of one pixel (the definition: include/vmatting.h): floor(cross / ee), the squared
// distance of I from the line through E, where the plate is bright enough (ee >= ee_min >= 1) and the light ratio ie /
// ee lies within [lo256, hi256] / 256; the plain d elsewhere.  Branch-free: every lane computes both and selects.  The
// floor quotient q <= ii < 2^18 comes from an f32 estimate: (float)cross, v_rcp_f32 (1 ulp) and the product are each
// within 2^-23 relative, so the estimate is within 2^18 * 2^-21.4 < 0.1 of cross / ee and its truncation within 1 of q.
// The remainder cross - q0 ee then lies in (-ee, 2 ee), inside int32, so its low 32 bits are exact and one step either
// way settles q.
__device__ __forceinline__ int shadow_distance(const uint8_t* __restrict__ pc, const uint8_t* __restrict__ pb, int d,
                                               int lo256, int hi256, int ee_min) {
  uint32_t ee = 0, ie = 0, ii = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t i = pc[c], e = pb[c];
    ee += e * e;
    ie += i * e;
    ii += i * i;
  }
  // floor ee <= 256 ie <= ceil ee: all below 2^27
  const bool in_range = ee >= (uint32_t)ee_min && (uint32_t)lo256 * ee <= 256u * ie && 256u * ie <= (uint32_t)hi256 * ee;
  const unsigned long long cross = (unsigned long long)ii * ee - (unsigned long long)ie * ie;  // >= 0 (Cauchy-Schwarz)
  const uint32_t den = ee ? ee : 1u;                                                          // (not in range then)
  uint32_t q = (uint32_t)((float)cross * __builtin_amdgcn_rcpf((float)den));
  int r = (int)((uint32_t)cross - q * den);
  if (r < 0) {
    --q;
    r += (int)den;
  }
  if (r >= (int)den) ++q;
  return in_range ? (int)q : d;
}

// work: [n][h][words][2] 64-bit, words = ceil(w / 64): {background, foreground} candidate bits.  SHADOW: the tile holds
// d' (shadow_distance) in place of d; nothing else differs.
template <bool VEC, bool SHADOW>
__global__ void __launch_bounds__(256)
plate_candidates_kernel(const uint8_t* __restrict__ cmp, const uint8_t* __restrict__ bg, int nb, int h, int w, int words,
                        int tiles_x, int tiles_y, int d_lo, int d_hi, size_t cmp_bytes, size_t bg_bytes,
                        unsigned long long* __restrict__ work, int lo256, int hi256, int ee_min) {
  __shared__ uint32_t raw[PLANE_BATCH][2][SEG_DWORDS];
  __shared__ int dist[CAND_HALO][CAND_COLS + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, f = b / tiles_y;
  const int x0 = tx * CAND_COLS, y0 = ty * CAND_ROWS;
  // the columns the tile reads: its own and one each side, inside the image
  const int xs = x0 > 0 ? x0 - 1 : 0, xe = x0 + CAND_COLS + 1 < w ? x0 + CAND_COLS + 1 : w;
  const int seg_bytes = (xe - xs) * 3;
  const int fb = nb == 1 ? 0 : f;

  for (int j0 = 0; j0 < CAND_HALO; j0 += PLANE_BATCH) {
    // halo row j is image row y0 - 1 + j, clamped: the replicated border
    uint32_t v[PLANE_BATCH][2];
#pragma unroll
    for (int u = 0; u < PLANE_BATCH; ++u) {
      const int yc = clampi(y0 - 1 + j0 + u, 0, h - 1);
      const size_t gc = (((size_t)f * h + yc) * w + xs) * 3, gb = (((size_t)fb * h + yc) * w + xs) * 3;
      v[u][0] = plane_dword<VEC>(cmp, (gc & ~(size_t)3) + 4 * (size_t)t, cmp_bytes,
                                 t < ((int)(gc & 3) + seg_bytes + 3) / 4);
      v[u][1] = plane_dword<VEC>(bg, (gb & ~(size_t)3) + 4 * (size_t)t, bg_bytes,
                                 t < ((int)(gb & 3) + seg_bytes + 3) / 4);
    }
#pragma unroll
    for (int u = 0; u < PLANE_BATCH; ++u) {
      const int yc = clampi(y0 - 1 + j0 + u, 0, h - 1);
      const size_t gc = (((size_t)f * h + yc) * w + xs) * 3, gb = (((size_t)fb * h + yc) * w + xs) * 3;
      v[u][0] = plane_tail<VEC>(cmp, (gc & ~(size_t)3) + 4 * (size_t)t, cmp_bytes,
                                t < ((int)(gc & 3) + seg_bytes + 3) / 4, v[u][0]);
      v[u][1] = plane_tail<VEC>(bg, (gb & ~(size_t)3) + 4 * (size_t)t, bg_bytes,
                                t < ((int)(gb & 3) + seg_bytes + 3) / 4, v[u][1]);
    }
    if (t < SEG_DWORDS) {
#pragma unroll
      for (int u = 0; u < PLANE_BATCH; ++u) {
        raw[u][0][t] = v[u][0];
        raw[u][1][t] = v[u][1];
      }
    }
    __syncthreads();
    // entry e of a halo row is column x0 - 1 + e, clamped
    for (int i = t; i < PLANE_BATCH * (CAND_COLS + 2); i += 256) {
      const int u = i / (CAND_COLS + 2), e = i - u * (CAND_COLS + 2);
      const int yc = clampi(y0 - 1 + j0 + u, 0, h - 1);
      const int px = clampi(x0 - 1 + e, 0, w - 1) - xs;
      const size_t gc = (((size_t)f * h + yc) * w + xs) * 3, gb = (((size_t)fb * h + yc) * w + xs) * 3;
      const uint8_t* pc = reinterpret_cast<const uint8_t*>(raw[u][0]) + (gc & 3) + 3 * px;
      const uint8_t* pb = reinterpret_cast<const uint8_t*>(raw[u][1]) + (gb & 3) + 3 * px;
      int s = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int q = (int)pc[c] - (int)pb[c];
        s += q * q;
      }
      dist[j0 + u][e] = SHADOW ? shadow_distance(pc, pb, s, lo256, hi256, ee_min) : s;
    }
    __syncthreads();
  }

  // thread t is column x0 + t, entry t + 1 of the halo rows; row sums of halo rows r, r + 1, r + 2 make D of tile row r
  const int x = x0 + t, word = tx * CAND_WORDS + wave;
  const bool pad = x >= w;
  int s0 = dist[0][t] + dist[0][t + 1] + dist[0][t + 2], s1 = dist[1][t] + dist[1][t + 1] + dist[1][t + 2];
#pragma unroll
  for (int r = 0; r < CAND_ROWS; ++r) {
    const int s2 = dist[r + 2][t] + dist[r + 2][t + 1] + dist[r + 2][t + 2];
    const int D = s0 + s1 + s2;
    s0 = s1;
    s1 = s2;
    const unsigned long long back = __ballot(pad || D <= d_lo), fore = __ballot(pad || D >= d_hi);
    const int y = y0 + r;
    if (lane == 0 && y < h && word < words)
      *reinterpret_cast<ulonglong2*>(work + (((size_t)f * h + y) * words + word) * 2) = make_ulonglong2(back, fore);
  }
}

__global__ void __launch_bounds__(256)
plate_erode_emit_kernel(const unsigned long long* __restrict__ work, int h, int w, int words, int tiles_x, int tiles_y,
                        int r_bg, int r_fg, uint8_t* __restrict__ out) {
  __shared__ unsigned long long raw[ERODE_HALO][ERODE_WORDS + 2][2];
  __shared__ unsigned long long hor[ERODE_HALO][ERODE_WORDS][2];
  __shared__ unsigned long long ver[ERODE_ROWS][ERODE_WORDS][2];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, f = b / tiles_y;
  const int word0 = tx * ERODE_WORDS, y0 = ty * ERODE_ROWS;
  const int halo = r_bg > r_fg ? r_bg : r_fg, rows = ERODE_ROWS + 2 * halo;

  // halo row r is image row y0 - halo + r, halo word j is word0 - 1 + j; outside the image every bit is set
  static_assert(ERODE_HALO * (ERODE_WORDS + 2) <= 2 * 256, "two candidate words per thread");
  ulonglong2 v[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = t + u * 256, r = i / (ERODE_WORDS + 2), j = i % (ERODE_WORDS + 2);
    const int y = y0 - halo + r, word = word0 - 1 + j;
    const bool inside = r < rows && y >= 0 && y < h && word >= 0 && word < words;
    v[u] = *reinterpret_cast<const ulonglong2*>(work + (inside ? (((size_t)f * h + y) * words + word) * 2 : 0));
    if (!inside) v[u] = make_ulonglong2(~0ull, ~0ull);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = t + u * 256, r = i / (ERODE_WORDS + 2), j = i % (ERODE_WORDS + 2);
    if (r < rows) {
      raw[r][j][0] = v[u].x;
      raw[r][j][1] = v[u].y;
    }
  }
  __syncthreads();

  // rows: pixel x keeps a class if x - r .. x + r all have it
  for (int i = t; i < rows * ERODE_WORDS * 2; i += 256) {
    const int r = i / (ERODE_WORDS * 2), j = (i >> 1) % ERODE_WORDS, c = i & 1;
    const int rad = c ? r_fg : r_bg;
    const unsigned long long left = raw[r][j][c], mid = raw[r][j + 1][c], right = raw[r][j + 2][c];
    unsigned long long acc = mid;
    for (int s = 1; s <= rad; ++s)
      acc &= ((mid >> s) | (right << (64 - s))) & ((mid << s) | (left >> (64 - s)));
    hor[r][j][c] = acc;
  }
  __syncthreads();

  // columns: tile row r is halo row r + halo
  if (t < ERODE_ROWS * ERODE_WORDS * 2) {
    const int r = t / (ERODE_WORDS * 2), j = (t >> 1) % ERODE_WORDS, c = t & 1;
    const int rad = c ? r_fg : r_bg;
    unsigned long long acc = ~0ull;
    for (int s = halo - rad; s <= halo + rad; ++s) acc &= hor[r + s][j][c];
    ver[r][j][c] = acc;
  }
  __syncthreads();

  // out: 16 pixels per thread
  const int r = t >> 3, seg = t & 7, j = seg >> 2, shift = (seg & 3) * 16;
  const int y = y0 + r, x = (word0 + j) * 64 + shift;
  if (y >= h || x >= w) return;
  const uint32_t back = (uint32_t)(ver[r][j][0] >> shift) & 0xffffu, fore = (uint32_t)(ver[r][j][1] >> shift) & 0xffffu;
  uint32_t q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q[k] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int bit = k * 4 + i;
      q[k] |= (((fore >> bit) & 1) ? 255u : ((back >> bit) & 1) ? 0u : 128u) << (8 * i);
    }
  }
  uint8_t* dst = out + ((size_t)f * h + y) * w + x;
  if (x + 16 <= w && reinterpret_cast<uintptr_t>(dst) % 16 == 0) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
  } else {
    for (int i = 0; i < 16 && x + i < w; ++i) dst[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
  }
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" size_t vm_trimap_from_plate_workspace_bytes(int n, int h, int w) {
  if (!shape_ok(n, h, w)) return 0;
  return (size_t)n * h * row_words(w) * 16;
}

namespace {

// both entry points: shadow == false is the plain distance (floor, ceil and dark are not looked at)
int trimap_from_plate(const char* who, const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int lo, int hi,
                      int r_bg, int r_fg, bool shadow, int floor, int ceil, int dark, uint8_t* out, void* work,
                      void* stream) {
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!shape_ok(n, h, w)) return fail(VM_EINVAL, "%s: %d x %d x %d pixels exceed %d", who, n, h, w, INT_MAX);
  if (nb != 1 && nb != n) return fail(VM_EINVAL, "%s: %d background frames for %d frames (1 or n)", who, nb, n);
  if (lo < 0 || hi > LEVEL_MAX || lo >= hi)
    return fail(VM_EINVAL, "%s: lo %d, hi %d (0 <= lo < hi <= %d)", who, lo, hi, LEVEL_MAX);
  if (r_bg < 0 || r_bg > R_MAX || r_fg < 0 || r_fg > R_MAX)
    return fail(VM_EINVAL, "%s: r_bg %d, r_fg %d (0..%d)", who, r_bg, r_fg, R_MAX);
  if (shadow) {
    if (floor < 1 || floor > SHADOW_ONE || ceil < SHADOW_ONE || ceil > 2 * SHADOW_ONE)
      return fail(VM_EINVAL, "%s: floor %d, ceil %d (1 <= floor <= %d <= ceil <= %d)", who, floor, ceil, SHADOW_ONE,
                  2 * SHADOW_ONE);
    if (dark < 0 || dark > 255) return fail(VM_EINVAL, "%s: dark %d (0..255)", who, dark);
  }
  if (!cmp || !bg || !out || !work) return fail(VM_EINVAL, "%s: null cmp / bg / out / work", who);
  const size_t pixels = (size_t)n * h * w, cmp_bytes = pixels * 3, bg_bytes = (size_t)nb * h * w * 3;
  if (overlap(out, pixels, cmp, cmp_bytes) || overlap(out, pixels, bg, bg_bytes))
    return fail(VM_EINVAL, "%s: out must not alias cmp or bg", who);
  if (reinterpret_cast<uintptr_t>(work) % 16) return fail(VM_EINVAL, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int words = row_words(w);
  unsigned long long* rows = static_cast<unsigned long long*>(work);
  {
    const int tiles_x = (words + CAND_WORDS - 1) / CAND_WORDS, tiles_y = (h + CAND_ROWS - 1) / CAND_ROWS;
    const dim3 grid((unsigned)tiles_x * tiles_y * n);  // (at most n h w tiles: within int)
    const bool vec = reinterpret_cast<uintptr_t>(cmp) % 4 == 0 && reinterpret_cast<uintptr_t>(bg) % 4 == 0 && bg_bytes >= 4;
    const int ee_min = shadow && dark > 0 ? 3 * dark * dark : 1;
    auto kernel = shadow ? (vec ? plate_candidates_kernel<true, true> : plate_candidates_kernel<false, true>)
                         : (vec ? plate_candidates_kernel<true, false> : plate_candidates_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, cmp, bg, nb, h, w, words, tiles_x, tiles_y, 9 * lo * lo,
                       9 * hi * hi, cmp_bytes, bg_bytes, rows, floor, ceil, ee_min);
  }
  const int tiles_x = (words + ERODE_WORDS - 1) / ERODE_WORDS, tiles_y = (h + ERODE_ROWS - 1) / ERODE_ROWS;
  hipLaunchKernelGGL(plate_erode_emit_kernel, dim3((unsigned)tiles_x * tiles_y * n), dim3(256), 0, st, rows, h, w, words,
                     tiles_x, tiles_y, r_bg, r_fg, out);
  return check_launch(who);
}

}  // namespace

extern "C" int vm_trimap_from_plate(const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int lo, int hi,
                                    int r_bg, int r_fg, uint8_t* out, void* work, void* stream) {
  return trimap_from_plate("trimap_from_plate", cmp, bg, nb, n, h, w, lo, hi, r_bg, r_fg, false, 0, 0, 0, out, work,
                           stream);
}

extern "C" int vm_trimap_from_plate_shadow(const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int lo,
                                           int hi, int r_bg, int r_fg, int floor, int ceil, int dark, uint8_t* out,
                                           void* work, void* stream) {
  return trimap_from_plate("trimap_from_plate_shadow", cmp, bg, nb, n, h, w, lo, hi, r_bg, r_fg, true, floor, ceil, dark,
                           out, work, stream);
}
