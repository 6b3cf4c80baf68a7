// vm_components_label and vm_trimap_fill_enclosed: connected components of a byte mask by a union-find with a fixed
// number of launches, and the fill of enclosed background built on it (the definitions: include/vmatting.h).
//
// THE INVARIANT.  L is a frame's int32 label array, indexed by the row-major pixel index i = y w + x.  A pixel that is
// not set holds -1 from the first launch on and is never written again.  For a set pixel L[i] is the index of a set
// pixel of the same component with L[i] <= i, at every moment of every launch, and every store to L[i] lowers it or
// leaves it (the first store aside): parents only ever decrease.  Hence
//   - a find loop (a = L[a] until L[a] == a) walks strictly downwards and terminates on any mixture of old and new
//     values; every value L[i] ever held is an ancestor of i for good, so a stale read costs steps, never a wrong set;
//   - a root (L[r] == r) is the smallest index of its tree, so the final labels are canonical: they do not depend on
//     the order in which the atomics arrived;
//   - a union ends only on the value an atomicMin returned (old == a: a was a root and now hangs below b), never on
//     a plain load; every other outcome replaces the larger of the two indices by a smaller one and goes round again.
// No block waits for another: there are no spin loops, flags or tickets, and cross-block order comes from the kernel
// boundaries alone.  Integer atomics only (min, or, add on separate bit fields): every result is order-independent.
//
// Launches (the same for every input of a shape):
//   tile    a block labels a 64 x 32 tile in LDS.  A wave is a row: its ballot gives the row's runs, and every pixel
//       starts at its run's first pixel.  Runs of adjacent rows that touch are united once, at their first common
//       column, by the atomic-min union on LDS.  Every pixel then stores its tile root as a frame index into L (-1
//       where it is not set); the fill also zeroes `aux` at every tile root (a superset of the final roots).
//   seam    a thread per pixel on a tile's first row or first column unites it with its neighbours across the seam,
//       again once per pair of touching runs (a run ends at a tile's edge here: across it the pixels of a row or
//       column are not united yet), by the atomic-min union on L.  Labels are read with agent-scope relaxed
//       atomic loads in this launch: the eight XCDs' L2s are not coherent for plain loads, and although a stale
//       ancestor would only cost a retry (the invariant, and the returning atomic), the seam traffic is small enough
//       that fresh values are the cheaper choice.  Only pixels that were roots at some time are ever the target of an
//       atomic, so a pixel that is no tile root keeps pointing at its tile root throughout.
//   finish  per tile again.  A pixel whose label still lies in its tile is counted at that label's LDS entry, any other
//       at its own; only the entries that were counted walk to their root in L (plain loads: nothing lowers a root in
//       this launch, and the launch before is complete), everything else reads the root from LDS.  The fill adds the
//       tile's border flag (bit 31) and, only with max_area > 0, its pixel count (bits 0..30) to aux[root]: one atomic
//       per entry and block, after the reduction in LDS.
//   emit    (fill) 16 pixels per thread: a zero byte whose root has no border flag, and an area within the cap, becomes
//       128; 16-byte loads and stores where the address allows, bytewise at ragged ends and unaligned rows.
#include "vm_common.h"

#include <climits>

namespace vm {
namespace {

constexpr int TILE_W = 64, TILE_H = 32, TILE_PIX = TILE_W * TILE_H, ROWS_PER_WAVE = TILE_H / 4;
constexpr unsigned BORDER_BIT = 0x80000000u;
enum { MODE_LABEL = 0, MODE_BORDER = 1, MODE_AREA = 2 };

__device__ __forceinline__ int lds_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lds_find(const int* lab, int a) {
  for (int p; (p = lds_load(lab + a)) != a;) a = p;
  return a;
}

__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  for (;;) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(lab + a, b);  // a > b
    if (old == a) return;
    a = old;  // a was no root any more: old < a
  }
}

__device__ __forceinline__ int agent_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool FRESH>
__device__ __forceinline__ int global_find(const int* L, int a) {
  for (int p; (p = FRESH ? agent_load(L + a) : L[a]) != a;) a = p;
  return a;
}

__device__ __forceinline__ void global_union(int* L, int a, int b) {
  for (;;) {
    a = global_find<true>(L, a);
    b = global_find<true>(L, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(L + a, b);  // a > b
    if (old == a) return;
    a = old;
  }
}

// bit `lane - 1`, `lane`, `lane + 1` of a row's mask; outside the word nothing is set
__device__ __forceinline__ bool bit_at(unsigned long long m, int i) { return i >= 0 && i < 64 && ((m >> i) & 1); }

// labels: [n][h][w]; aux: [n][h][w] or null
__global__ void __launch_bounds__(256)
cc_tile_kernel(const uint8_t* mask, int h, int w, int tiles_x, int tiles_y, int value, bool eight,
               int* __restrict__ labels, int* __restrict__ aux) {
  __shared__ int lab[TILE_PIX];
  __shared__ unsigned long long bits[TILE_H];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, f = b / tiles_y;
  const int x0 = tx * TILE_W, y0 = ty * TILE_H, x = x0 + lane;
  const size_t frame = (size_t)f * h * w;

#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wave + 4 * k, y = y0 + r;
    const bool set = y < h && x < w && mask[frame + (size_t)y * w + x] == value;
    const unsigned long long m = __ballot(set);
    if (lane == 0) bits[r] = m;
    // the run's first pixel: one past the highest clear bit below this lane
    const unsigned long long below = ~m & ((1ull << lane) - 1);
    const int start = below ? 64 - __clzll((long long)below) : 0;
    lab[r * TILE_W + lane] = set ? r * TILE_W + start : -1;
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wave + 4 * k;
    if (r == 0) continue;
    const unsigned long long cur = bits[r], up = bits[r - 1];
    if (!bit_at(cur, lane)) continue;
    const int me = r * TILE_W + lane, above = me - TILE_W;
    if (bit_at(up, lane)) {
      // once per pair of touching runs: at the first column they share
      if (!bit_at(cur, lane - 1) || !bit_at(up, lane - 1)) lds_union(lab, me, above);
    } else if (eight) {
      if (bit_at(up, lane - 1)) lds_union(lab, me, above - 1);
      if (bit_at(up, lane + 1)) lds_union(lab, me, above + 1);
    }
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wave + 4 * k, y = y0 + r;
    if (y >= h || x >= w) continue;
    const int me = r * TILE_W + lane;
    int g = -1;
    if (lab[me] >= 0) {
      const int root = lds_find(lab, me);
      g = (y0 + root / TILE_W) * w + x0 + root % TILE_W;
      if (aux && root == me) aux[frame + g] = 0;
    }
    labels[frame + (size_t)y * w + x] = g;
  }
}

// seams_y rows (y = TILE_H, 2 TILE_H, ...) of w pixels, then seams_x columns (x = TILE_W, ...) of h pixels, per frame
__global__ void __launch_bounds__(256)
cc_seam_kernel(int* labels, int n, int h, int w, int seams_y, int seams_x, bool eight) {
  const long per_frame = (long)seams_y * w + (long)seams_x * h;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= per_frame * n) return;
  const int f = (int)(id / per_frame);
  const long s = id - (long)f * per_frame;
  int* L = labels + (size_t)f * h * w;
  auto set = [&](int xx, int yy) { return xx >= 0 && xx < w && yy >= 0 && yy < h && L[(size_t)yy * w + xx] >= 0; };
  if (s < (long)seams_y * w) {
    const int y = ((int)(s / w) + 1) * TILE_H, x = (int)(s % w);
    if (!set(x, y)) return;
    const int me = y * w + x, above = me - w;
    if (set(x, y - 1)) {
      if (x % TILE_W == 0 || !set(x - 1, y) || !set(x - 1, y - 1)) global_union(L, me, above);
    } else if (eight) {
      if (set(x - 1, y - 1)) global_union(L, me, above - 1);
      if (set(x + 1, y - 1)) global_union(L, me, above + 1);
    }
  } else {
    const long v = s - (long)seams_y * w;
    const int x = ((int)(v / h) + 1) * TILE_W, y = (int)(v % h);
    if (!set(x, y)) return;
    const int me = y * w + x, left = me - 1;
    if (set(x - 1, y)) {
      if (y % TILE_H == 0 || !set(x, y - 1) || !set(x - 1, y - 1)) global_union(L, me, left);
    } else if (eight) {
      if (set(x - 1, y - 1)) global_union(L, me, left - w);
      if (set(x - 1, y + 1)) global_union(L, me, left + w);
    }
  }
}

template <int MODE>
__global__ void __launch_bounds__(256)
cc_finish_kernel(int h, int w, int tiles_x, int tiles_y, int* labels, int* aux) {
  __shared__ unsigned cnt[TILE_PIX];  // bit 31: a counted pixel lies on the frame's border; bits 0..30: the count
  __shared__ int root[TILE_PIX];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, f = b / tiles_y;
  const int x0 = tx * TILE_W, y0 = ty * TILE_H, x = x0 + lane;
  int* L = labels + (size_t)f * h * w;

  int key[ROWS_PER_WAVE];
#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wave + 4 * k, y = y0 + r, me = r * TILE_W + lane;
    cnt[me] = 0;
    key[k] = -1;
    if (y >= h || x >= w) continue;
    const int p = L[(size_t)y * w + x];
    if (p < 0) continue;
    const int py = p / w - y0, px = p - (py + y0) * w - x0;
    key[k] = py >= 0 && py < TILE_H && px >= 0 && px < TILE_W ? py * TILE_W + px : me;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    if (key[k] < 0) continue;
    const int y = y0 + wave + 4 * k;
    const bool border = y == 0 || y == h - 1 || x == 0 || x == w - 1;
    if (MODE == MODE_AREA) atomicAdd(&cnt[key[k]], 1u);
    if (MODE != MODE_AREA || border) atomicOr(&cnt[key[k]], MODE != MODE_LABEL && border ? BORDER_BIT : 1u);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wave + 4 * k, y = y0 + r, me = r * TILE_W + lane;
    const unsigned c = cnt[me];
    if (!c) continue;  // (counted entries are set pixels of this tile inside the image)
    const int g = global_find<false>(L, y * w + x);
    root[me] = g;
    if (MODE != MODE_LABEL && (c & BORDER_BIT)) atomicOr(reinterpret_cast<unsigned*>(aux) + (size_t)f * h * w + g, BORDER_BIT);
    if (MODE == MODE_AREA) atomicAdd(reinterpret_cast<unsigned*>(aux) + (size_t)f * h * w + g, c & ~BORDER_BIT);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k)
    if (key[k] >= 0) L[(size_t)(y0 + wave + 4 * k) * w + x] = root[key[k]];
}

// trimap and out may be the same array: every thread reads its 16 bytes before it writes them
__global__ void __launch_bounds__(256)
fill_emit_kernel(const uint8_t* trimap, int n, int h, int w, int segs, unsigned max_area, const int* __restrict__ labels,
                 const unsigned* __restrict__ aux, uint8_t* out) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)n * h * segs) return;
  const int seg = (int)(id % segs);
  const long row = id / segs;  // f h + y
  const int x = seg * 16, f = (int)(row / h);
  const size_t at = (size_t)row * w + x, frame = (size_t)f * h * w;
  const uint8_t* src = trimap + at;
  uint8_t* dst = out + at;
  const bool wide = x + 16 <= w;
  uint32_t q[4] = {0, 0, 0, 0};
  if (wide && reinterpret_cast<uintptr_t>(src) % 16 == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(src);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
  } else {
    for (int i = 0; i < 16 && x + i < w; ++i) q[i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (x + i < w && ((q[i >> 2] >> (8 * (i & 3))) & 0xffu) == 0) {
      const unsigned a = aux[frame + labels[at + i]];
      if (!(a & BORDER_BIT) && (max_area == 0 || (a & ~BORDER_BIT) <= max_area)) q[i >> 2] |= 128u << (8 * (i & 3));
    }
  }
  if (wide && reinterpret_cast<uintptr_t>(dst) % 16 == 0) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
  } else {
    for (int i = 0; i < 16 && x + i < w; ++i) dst[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
  }
}

// the tile, seam and finish launches: the final labels of every frame in `labels`
template <int MODE>
void label_launches(const uint8_t* mask, int n, int h, int w, int value, bool eight, int* labels, int* aux,
                    hipStream_t st) {
  const int tiles_x = (w + TILE_W - 1) / TILE_W, tiles_y = (h + TILE_H - 1) / TILE_H;
  const dim3 tiles((unsigned)tiles_x * tiles_y * n);  // (at most n h w tiles: within int)
  hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, st, mask, h, w, tiles_x, tiles_y, value, eight, labels, aux);
  const int seams_y = tiles_y - 1, seams_x = tiles_x - 1;
  const long seam_pixels = ((long)seams_y * w + (long)seams_x * h) * n;
  if (seam_pixels > 0)
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((seam_pixels + 255) / 256)), dim3(256), 0, st, labels, n, h, w,
                       seams_y, seams_x, eight);
  hipLaunchKernelGGL((cc_finish_kernel<MODE>), tiles, dim3(256), 0, st, h, w, tiles_x, tiles_y, labels, aux);
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" int vm_components_label(const uint8_t* mask, int n, int h, int w, int value, int connectivity, int32_t* labels,
                                   void* stream) {
  const char* who = "components_label";
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!shape_ok(n, h, w)) return fail(VM_EINVAL, "%s: %d x %d x %d pixels exceed %d", who, n, h, w, INT_MAX);
  if (value < 0 || value > 255) return fail(VM_EINVAL, "%s: value %d (0..255)", who, value);
  if (connectivity != 4 && connectivity != 8) return fail(VM_EINVAL, "%s: connectivity %d (4 or 8)", who, connectivity);
  if (!mask || !labels) return fail(VM_EINVAL, "%s: null mask / labels", who);
  if (reinterpret_cast<uintptr_t>(labels) % 4) return fail(VM_EINVAL, "%s: labels must be 4-byte aligned", who);
  const size_t pixels = (size_t)n * h * w;
  if (overlap(mask, pixels, labels, pixels * 4)) return fail(VM_EINVAL, "%s: labels must not overlap mask", who);
  label_launches<MODE_LABEL>(mask, n, h, w, value, connectivity == 8, labels, nullptr,
                             reinterpret_cast<hipStream_t>(stream));
  return check_launch(who);
}

extern "C" size_t vm_trimap_fill_enclosed_workspace_bytes(int n, int h, int w) {
  if (!shape_ok(n, h, w)) return 0;
  return (size_t)n * h * w * 8;
}

extern "C" int vm_trimap_fill_enclosed(const uint8_t* trimap, int n, int h, int w, int max_area, uint8_t* out, void* work,
                                       void* stream) {
  const char* who = "trimap_fill_enclosed";
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!shape_ok(n, h, w)) return fail(VM_EINVAL, "%s: %d x %d x %d pixels exceed %d", who, n, h, w, INT_MAX);
  if (max_area < 0) return fail(VM_EINVAL, "%s: max_area %d (0: any area, or a cap >= 1)", who, max_area);
  if (!trimap || !out || !work) return fail(VM_EINVAL, "%s: null trimap / out / work", who);
  if (reinterpret_cast<uintptr_t>(work) % 16) return fail(VM_EINVAL, "%s: the workspace must be 16-byte aligned", who);
  const size_t pixels = (size_t)n * h * w;
  if (out != trimap && overlap(out, pixels, trimap, pixels))
    return fail(VM_EINVAL, "%s: out must be trimap itself or not overlap it", who);
  if (overlap(work, pixels * 8, trimap, pixels) || overlap(work, pixels * 8, out, pixels))
    return fail(VM_EINVAL, "%s: work must not overlap trimap or out", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (h < 3 || w < 3) {  // no interior pixel: nothing is enclosed
    if (out != trimap) {
      const hipError_t e = hipMemcpyAsync(out, trimap, pixels, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return fail(VM_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    return VM_OK;
  }
  int* labels = static_cast<int*>(work);
  int* aux = labels + pixels;
  if (max_area > 0)
    label_launches<MODE_AREA>(trimap, n, h, w, 0, false, labels, aux, st);
  else
    label_launches<MODE_BORDER>(trimap, n, h, w, 0, false, labels, aux, st);
  const int segs = (w + 15) / 16;
  const long threads = (long)n * h * segs;
  hipLaunchKernelGGL(fill_emit_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, trimap, n, h, w, segs,
                     (unsigned)max_area, labels, reinterpret_cast<const unsigned*>(aux), out);
  return check_launch(who);
}
