// vm_trimap_propagate: a key frame's trimap carried to the next frame by that frame's backward flow (the definition:
// include/vmatting.h).  A label survives where every pixel of the window the bilinear warp would touch, grown by
// `grow` pixels, carries it; everything else is unknown.  Integer logic after two f32 adds and floors, so the numpy
// restatement (tests/trimap_prop_ref.py) is matched byte for byte.
//
// The window at a displaced position is the union of the symmetric (2 grow + 1)^2 windows at the up to four pixels the
// warp touches, so the work splits in two:
//
//   class map (grow > 0)  per pixel, two bits: "every pixel of its (2 grow + 1)^2 window, clipped to the image, is
//       foreground" and the same for background.  The map is kept as bit rows: one {foreground, background} pair of
//       32-bit words (8 bytes, one load of the gather) per 32 pixels of a row, rows padded to 64 pixels.  A wave
//       classifies 64 pixels with one coalesced byte load and two ballots; the row reduction is then shifts and ANDs
//       of three neighbouring 64-bit words, the column reduction an AND down 2 grow + 1 rows, both on LDS tiles of
//       128 x 32 pixels with a grow halo (pixels outside the image count as both classes: the window is clipped).
//       1 B read and 0.25 B written per pixel.
//   gather  per output pixel one coalesced 8-byte flow load, the two adds and floors, and the AND of the up to four
//       class-map entries (grow == 0: of the classes of the up to four bytes of prev, no map).  A block takes 2048
//       consecutive pixels of the flat image, 8 per thread at a stride of 256 so that every flow load of a wave is
//       512 contiguous bytes, all 8 loads in flight before the first gather; the result bytes go through LDS and leave
//       as one 16-byte store per thread of the first two waves.  The image is flat, so an odd w costs nothing; the
//       last block's ragged end and an output that is not 16-byte aligned are stored bytewise.
//
// Both kernels move few bytes per launch (20 MB at 1080p), so what they wait for is latency, not bandwidth: every
// thread has its loads in flight together (LOAD_BATCH rows of the class map, all 8 pixels of the gather).
#include "vm_common.h"

#include <climits>

namespace vm {
namespace {

constexpr int GROW_MAX = 8;
constexpr int TILE_WORDS = 2, TILE_ROWS = 32;   // the class-map tile: 128 x 32 pixels
constexpr int HALO_ROWS = TILE_ROWS + 2 * GROW_MAX, LOAD_BATCH = 16;
constexpr int GATHER_PER_THREAD = 8, GATHER_BLOCK = 256 * GATHER_PER_THREAD;

// pixel indices stay int, the last gather block's overhang included
constexpr long PIXELS_MAX = (long)INT_MAX - GATHER_BLOCK;

constexpr uint32_t FG = 1, BG = 2;
__device__ __forceinline__ uint32_t class_of(uint32_t v) { return v == 255 ? FG : v == 0 ? BG : 0; }

// map: [h][words][2][2] 32-bit, words = ceil(w / 64): per row and 64 pixels, {foreground, background} bits of the
// first 32 pixels, then of the other 32; bit i of a 32-bit word is its pixel i
__global__ void __launch_bounds__(256)
trimap_class_map_kernel(const uint8_t* __restrict__ prev, int h, int w, int words, int grow,
                        unsigned long long* __restrict__ map) {
  __shared__ unsigned long long raw[HALO_ROWS][TILE_WORDS + 2][2];
  __shared__ unsigned long long hor[HALO_ROWS][TILE_WORDS][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int word0 = blockIdx.x * TILE_WORDS, y0 = blockIdx.y * TILE_ROWS;
  const int rows = TILE_ROWS + 2 * grow;
  const int x_lo = word0 * 64 - grow, x_hi = (word0 + TILE_WORDS) * 64 + grow;  // the columns the tile reads

  // classify: wave j takes word j of every row of the halo tile (TILE_WORDS + 2 = 4 waves), LOAD_BATCH rows' loads in
  // flight at once (one after another, the rows' load latencies would add up to the kernel's time); lanes outside
  // the image or the halo load nothing
  static_assert(TILE_WORDS + 2 == 4, "one wave per word of a halo row");
  const int x = (word0 + wave - 1) * 64 + lane;
  const bool x_in = x >= 0 && x < w && x >= x_lo && x < x_hi;
  for (int r0 = 0; r0 < rows; r0 += LOAD_BATCH) {
    uint32_t c[LOAD_BATCH];
#pragma unroll
    for (int u = 0; u < LOAD_BATCH; ++u) {
      const int y = y0 - grow + r0 + u;
      const bool inside = x_in && r0 + u < rows && y >= 0 && y < h;
      // (no branch around the load, or the batch would wait for each in turn: pixel 0 stands in, and the OR below,
      // unlike a select of the loaded value, gives the compiler no reason to put one back)
      const uint32_t v = prev[inside ? (size_t)y * w + x : 0];
      c[u] = class_of(v) | (inside ? 0u : (FG | BG));
    }
#pragma unroll
    for (int u = 0; u < LOAD_BATCH; ++u) {
      const unsigned long long fg = __ballot(c[u] & FG), bg = __ballot(c[u] & BG);
      if (lane == 0 && r0 + u < rows) {
        raw[r0 + u][wave][0] = fg;
        raw[r0 + u][wave][1] = bg;
      }
    }
  }
  __syncthreads();

  // rows: pixel x keeps a class if x - grow .. x + grow all have it
  if (t < rows * TILE_WORDS * 2) {
    const int r = t / (TILE_WORDS * 2), j = (t >> 1) % TILE_WORDS, c = t & 1;
    const unsigned long long left = raw[r][j][c], mid = raw[r][j + 1][c], right = raw[r][j + 2][c];
    unsigned long long acc = mid;
    for (int s = 1; s <= grow; ++s)
      acc &= ((mid >> s) | (right << (64 - s))) & ((mid << s) | (left >> (64 - s)));
    hor[r][j][c] = acc;
  }
  __syncthreads();

  // columns, and out: the two threads of a word hold its foreground and its background bits and trade halves, so that
  // each stores {foreground, background} of 32 pixels
  if (t < TILE_ROWS * TILE_WORDS * 2) {
    const int r = t / (TILE_WORDS * 2), j = (t >> 1) % TILE_WORDS, c = t & 1;
    const int y = y0 + r, word = word0 + j;
    unsigned long long acc = hor[r][j][c];
    for (int s = 1; s <= 2 * grow; ++s) acc &= hor[r + s][j][c];
    const unsigned long long other = __shfl_xor(acc, 1);
    const unsigned long long fg = c ? other : acc, bg = c ? acc : other;
    if (y < h && word < words)
      map[((size_t)y * words + word) * 2 + c] =
          c ? (fg >> 32) | (bg & 0xffffffff00000000ull) : (fg & 0xffffffffull) | (bg << 32);
  }
}

// the class bits of pixel (x, y): from prev itself (RAW, grow == 0) or from the class map
template <bool RAW>
__device__ __forceinline__ uint32_t class_at(const void* __restrict__ src, int w, int words, int x, int y) {
  if (RAW) return class_of(static_cast<const uint8_t*>(src)[(size_t)y * w + x]);
  const uint2 e = static_cast<const uint2*>(src)[((size_t)y * words + (x >> 6)) * 2 + ((x >> 5) & 1)];
  return ((e.x >> (x & 31)) & 1) | (((e.y >> (x & 31)) & 1) << 1);
}

template <bool RAW>
__global__ void __launch_bounds__(256)
trimap_gather_kernel(const void* __restrict__ src, const float2* __restrict__ flow, int h, int w, int words,
                     uint8_t* __restrict__ out, bool vec) {
  __shared__ __attribute__((aligned(16))) uint8_t res[GATHER_BLOCK];
  const int t = threadIdx.x;
  const int total = h * w;
  const int base = blockIdx.x * GATHER_BLOCK;  // (the host keeps h * w within int)
  const float xmax = (float)(w - 1), ymax = (float)(h - 1);
  // every flow load first, then every gather: the loads of one thread overlap instead of queueing behind each other
  float2 f[GATHER_PER_THREAD];
#pragma unroll
  for (int k = 0; k < GATHER_PER_THREAD; ++k) {
    const int p = base + k * 256 + t;
    f[k] = flow[p < total ? p : total - 1];  // (no branch around the load; the overhang's results are not stored)
  }
  uint32_t c[GATHER_PER_THREAD];
#pragma unroll
  for (int k = 0; k < GATHER_PER_THREAD; ++k) {
    const int p = base + k * 256 + t;
    const int y = p / w, x = p - y * w;
    const float xs = (float)x + f[k].x, ys = (float)y + f[k].y;
    const bool inside = p < total && xs >= 0.f && xs <= xmax && ys >= 0.f && ys <= ymax;  // (false for NaN)
    // no branch around the gather: a target outside the image reads pixel (0, 0) and drops it, and the 4 loads of
    // each of the thread's pixels can all be in flight together
    const float xc = inside ? xs : 0.f, yc = inside ? ys : 0.f;
    const int x0 = (int)floorf(xc), y0 = (int)floorf(yc);
    const int x1 = x0 + (xc > (float)x0), y1 = y0 + (yc > (float)y0);
    const uint32_t g = class_at<RAW>(src, w, words, x0, y0) & class_at<RAW>(src, w, words, x1, y0) &
                       class_at<RAW>(src, w, words, x0, y1) & class_at<RAW>(src, w, words, x1, y1);
    c[k] = inside ? g : 0;
  }
#pragma unroll
  for (int k = 0; k < GATHER_PER_THREAD; ++k) res[k * 256 + t] = (c[k] & FG) ? 255 : (c[k] & BG) ? 0 : 128;
  __syncthreads();
  if (t >= GATHER_BLOCK / 16) return;
  const int q = base + t * 16;
  if (vec && q + 16 <= total) {
    *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(res + t * 16);
  } else {
    for (int i = 0; i < 16 && q + i < total; ++i) out[q + i] = res[t * 16 + i];
  }
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" size_t vm_trimap_propagate_workspace_bytes(int h, int w, int grow) {
  if (h < 1 || w < 1 || grow < 1 || grow > GROW_MAX || (long)h * w > PIXELS_MAX) return 0;
  return (size_t)h * row_words(w) * 16;
}

extern "C" int vm_trimap_propagate(const uint8_t* prev, const float* flow, int h, int w, int grow, uint8_t* out,
                                   void* work, void* stream) {
  if (h < 1 || w < 1) return fail(VM_EINVAL, "trimap_propagate: bad shape [%d,%d]", h, w);
  if ((long)h * w > PIXELS_MAX) return fail(VM_EINVAL, "trimap_propagate: %d x %d pixels exceed %ld", h, w, PIXELS_MAX);
  if (grow < 0 || grow > GROW_MAX) return fail(VM_EINVAL, "trimap_propagate: grow %d (0..%d)", grow, GROW_MAX);
  if (!prev || !flow || !out) return fail(VM_EINVAL, "trimap_propagate: null prev / flow / out");
  if (grow > 0 && !work) return fail(VM_EINVAL, "trimap_propagate: null workspace (grow > 0 needs one)");
  if (out == prev) return fail(VM_EINVAL, "trimap_propagate: out must not alias prev");
  if (reinterpret_cast<uintptr_t>(flow) % 8) return fail(VM_EINVAL, "trimap_propagate: flow must be 8-byte aligned");
  if (grow > 0 && reinterpret_cast<uintptr_t>(work) % 16)
    return fail(VM_EINVAL, "trimap_propagate: the workspace must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int words = row_words(w);
  const bool vec = reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const dim3 grid(((long)h * w + GATHER_BLOCK - 1) / GATHER_BLOCK);
  const float2* fl = reinterpret_cast<const float2*>(flow);
  if (grow == 0) {
    hipLaunchKernelGGL((trimap_gather_kernel<true>), grid, dim3(256), 0, st, prev, fl, h, w, words, out, vec);
    return check_launch("trimap_propagate");
  }
  const dim3 tiles((words + TILE_WORDS - 1) / TILE_WORDS, (h + TILE_ROWS - 1) / TILE_ROWS);
  hipLaunchKernelGGL(trimap_class_map_kernel, tiles, dim3(256), 0, st, prev, h, w, words, grow,
                     static_cast<unsigned long long*>(work));
  hipLaunchKernelGGL((trimap_gather_kernel<false>), grid, dim3(256), 0, st, work, fl, h, w, words, out, vec);
  return check_launch("trimap_propagate");
}
