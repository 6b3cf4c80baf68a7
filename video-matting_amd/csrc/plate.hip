// vm_plate_from_samples: the background plate of a locked-off shot as the per-byte temporal lower median of n sample
// frames, and the per-pixel interquantile spread (the definition: include/vmatting.h).  Integer only, so the numpy
// restatement (tests/plate_ref.py) is matched byte for byte.  One launch:
//
//   A thread takes one dword of the frame, 4 byte positions, and reads the 4 bytes at that offset of each of the n
//   frames: adjacent lanes read adjacent dwords of every frame.  Frames need not start on a dword (h w 3 is any multiple
//   of 3, and `samples` sits anywhere), so the loads are unaligned dword loads; the frame's last, partial dword is read
//   as the dword that ends with the frame and shifted down (the first frame of a 1 x 1 clip, which has no 4 bytes, byte
//   by byte).  The bytes are widened to 16-bit lanes, even and odd bytes of the dword as two packed pairs, and each
//   array of n pairs goes through Batcher's odd-even merge sorting network with v_pk_min_u16 / v_pk_max_u16: the
//   network for the next power of two with every comparator that touches an index >= n left out (those inputs would be
//   +inf and never move).  The kernel is instantiated per n, so the three ranks are register names, the network is
//   straight-line code, and the compiler drops every comparator that none of the three ranks depends on.  2 n VGPRs
//   hold the samples (128 at n = 64); nothing is indexed at run time, so nothing goes to scratch.
//   A block of 256 threads takes 3 x 256 dwords = 3072 bytes = 1024 whole pixels, dword j * 256 + t in round j (not
//   unrolled: one round's samples in registers at a time).  Each round leaves its hi - lo bytes in LDS; after a
//   barrier every thread folds 12 of them into 4 spread bytes, one dword store.  Blocks own whole pixels, so the fold
//   never crosses a block, whatever the image size.
//   Stores are dwords where all 4 bytes exist (unaligned when `plate` / `spread` are), single bytes at the ragged end.
//
// (3 n + 4) B per pixel.  Not chosen: a bit-serial radix select on the same 16-bit lanes, counting per bit the samples
// below the candidate: 3 packed operations per sample, bit, rank and half, 8 x 3 x 2 x 3 n = 144 n per dword (9216 at
// n = 64) against the network's 4 per comparator (543 comparators at n = 64, 445 of them left after pruning: 1778).  It
// is kept in the study build (radix_select below) and measured in DESIGN 3.4i.
#include "vm_common.h"

#include <array>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace vm {
namespace {

constexpr int ROUNDS = 3, BLOCK_DWORDS = ROUNDS * 256, BLOCK_BYTES = BLOCK_DWORDS * 4, BLOCK_PIXELS = BLOCK_BYTES / 3;
static_assert(BLOCK_PIXELS * 3 == BLOCK_BYTES && BLOCK_PIXELS == 4 * 256, "whole pixels per block, 4 per thread");

// Batcher's merge exchange (Knuth 5.2.2 M) for the power of two >= n, comparators with an index >= n dropped
constexpr int NET_MAX = 543;  // comparators at n = 64
struct Net {
  int a[NET_MAX], b[NET_MAX], count;
};

constexpr Net make_net(int n) {
  Net net{};
  int size = 1;
  while (size < n) size *= 2;
  for (int p = 1; p < size; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < size; j += 2 * k)
        for (int i = 0; i < k && i + j + k < size; ++i) {
          const int lo = i + j, hi = i + j + k;
          if (lo / (2 * p) == hi / (2 * p) && hi < n) {
            net.a[net.count] = lo;
            net.b[net.count] = hi;
            ++net.count;
          }
        }
  return net;
}
static_assert(make_net(64).count == NET_MAX && make_net(4).count == 5 && make_net(1).count == 0, "the network's size");

template <int N>
struct NetOf {
  static constexpr Net net = make_net(N);
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

template <int N, size_t... I>
__device__ __forceinline__ void sort_pairs(u16x2 (&v)[N], std::index_sequence<I...>) {
  (([&] {
     constexpr int a = NetOf<N>::net.a[I], b = NetOf<N>::net.b[I];
     const u16x2 lo = __builtin_elementwise_min(v[a], v[b]), hi = __builtin_elementwise_max(v[a], v[b]);
     v[a] = lo;
     v[b] = hi;
   }()),
   ...);
}

__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }

#ifdef VM_STUDY
// The variant not chosen, kept in the study build for tools/plate_bench.py (VM_PLATE_RADIX=1, n = 8, 16, 32, 64): a
// bit-serial select from the top bit down.  The rank-th smallest is >= t exactly when at most `rank` samples lie below
// t; in 16-bit lanes holding bytes, bit 15 of v - t is v < t.  3 packed operations per sample, bit, rank and half.
template <int N>
__device__ __forceinline__ u16x2 radix_select(const u16x2 (&v)[N], int rank) {
  u16x2 res = {0, 0};
#pragma unroll
  for (int bit = 7; bit >= 0; --bit) {
    const u16x2 t = res | (u16x2)(unsigned short)(1 << bit);
    u16x2 below = {0, 0};
#pragma unroll
    for (int k = 0; k < N; ++k) below += (v[k] - t) >> 15;
    res |= ((below - (u16x2)(unsigned short)(rank + 1)) >> 15) << bit;
  }
  return res;
}
#endif

// v sorted as far as its entries LO, MID and HI need -> those three
template <int N, bool RADIX>
__device__ __forceinline__ void three_ranks(u16x2 (&v)[N], u16x2& lo, u16x2& mid, u16x2& hi) {
  constexpr int LO = (N - 1) / 4, MID = (N - 1) / 2, HI = N - 1 - LO;
#ifdef VM_STUDY
  if constexpr (RADIX) {
    lo = radix_select<N>(v, LO);
    mid = radix_select<N>(v, MID);
    hi = radix_select<N>(v, HI);
    return;
  }
#endif
  sort_pairs<N>(v, std::make_index_sequence<NetOf<N>::net.count>{});
  lo = v[LO];
  mid = v[MID];
  hi = v[HI];
}

// frame_bytes = h w 3; pixels = h w
template <int N, bool RADIX = false>
__global__ void __launch_bounds__(256)
plate_kernel(const uint8_t* __restrict__ samples, size_t frame_bytes, int pixels, uint8_t* __restrict__ plate,
             uint8_t* __restrict__ spread) {
  __shared__ uint32_t range[BLOCK_DWORDS];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * BLOCK_BYTES;

#pragma unroll 1
  for (int j = 0; j < ROUNDS; ++j) {
    const size_t off = base + 4 * (size_t)(j * 256 + t);
    uint32_t d = 0;
    if (off < frame_bytes) {
      const int valid = frame_bytes - off >= 4 ? 4 : (int)(frame_bytes - off);
      const uint8_t* p = samples + off;
      uint32_t v[N];
      if (valid == 4) {
#pragma unroll
        for (int k = 0; k < N; ++k) memcpy(&v[k], p + k * frame_bytes, 4);
      } else {
        // the dword that ends with the frame holds the bytes wanted on top: it starts inside `samples` for every frame
        // but the first of a frame smaller than a dword
        const int back = 4 - valid;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          if (k > 0 || off >= (size_t)back) {
            memcpy(&v[k], p + k * frame_bytes - back, 4);
            v[k] >>= 8 * back;
          } else {
            v[k] = 0;
            for (int b = 0; b < valid; ++b) v[k] |= (uint32_t)p[b] << (8 * b);
          }
        }
      }
      u16x2 even[N], odd[N];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        even[k] = __builtin_bit_cast(u16x2, v[k] & 0x00ff00ffu);
        odd[k] = __builtin_bit_cast(u16x2, (v[k] >> 8) & 0x00ff00ffu);
      }
      u16x2 lo_e, mid_e, hi_e, lo_o, mid_o, hi_o;
      three_ranks<N, RADIX>(even, lo_e, mid_e, hi_e);
      three_ranks<N, RADIX>(odd, lo_o, mid_o, hi_o);
      const uint32_t med = as_u32(mid_e) | (as_u32(mid_o) << 8);
      d = as_u32(hi_e - lo_e) | (as_u32(hi_o - lo_o) << 8);
      uint8_t* q = plate + off;
      if (valid == 4) {
        memcpy(q, &med, 4);
      } else {
        for (int b = 0; b < valid; ++b) q[b] = (uint8_t)(med >> (8 * b));
      }
    }
    range[j * 256 + t] = d;
  }
  if (!spread) return;
  __syncthreads();

  // pixel first + i is bytes 3 i .. 3 i + 2 of this thread's 12
  const long first = (long)blockIdx.x * BLOCK_PIXELS + 4 * t;
  if (first >= pixels) return;
  const uint32_t r0 = range[3 * t], r1 = range[3 * t + 1], r2 = range[3 * t + 2];
  const uint32_t b[12] = {r0 & 255, (r0 >> 8) & 255, (r0 >> 16) & 255, r0 >> 24, r1 & 255, (r1 >> 8) & 255,
                          (r1 >> 16) & 255, r1 >> 24, r2 & 255, (r2 >> 8) & 255, (r2 >> 16) & 255, r2 >> 24};
  uint32_t out = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t m = b[3 * i] > b[3 * i + 1] ? b[3 * i] : b[3 * i + 1];
    m = m > b[3 * i + 2] ? m : b[3 * i + 2];
    out |= m << (8 * i);
  }
  uint8_t* q = spread + first;
  if (first + 4 <= pixels) {
    memcpy(q, &out, 4);
  } else {
    for (int i = 0; first + i < pixels; ++i) q[i] = (uint8_t)(out >> (8 * i));
  }
}

typedef void (*PlateKernel)(const uint8_t*, size_t, int, uint8_t*, uint8_t*);

template <size_t... I>
constexpr std::array<PlateKernel, sizeof...(I)> kernels_by_n(std::index_sequence<I...>) {
  return {{plate_kernel<(int)I + 1>...}};
}

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" int vm_plate_from_samples(const uint8_t* samples, int n, int h, int w, uint8_t* plate, uint8_t* spread,
                                     void* stream) {
  static const auto kernels = kernels_by_n(std::make_index_sequence<VM_PLATE_MAX_SAMPLES>{});
  const char* who = "plate_from_samples";
  if (!samples || !plate) return fail(VM_EINVAL, "%s: null samples / plate", who);
  if (n < 1 || n > VM_PLATE_MAX_SAMPLES)
    return fail(VM_EINVAL, "%s: %d samples (1..%d)", who, n, VM_PLATE_MAX_SAMPLES);
  if (h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d]", who, h, w);
  if ((long long)n * h * w * 3 > (long long)INT_MAX)
    return fail(VM_EINVAL, "%s: %d x %d x %d x 3 sample bytes exceed %d", who, n, h, w, INT_MAX);
  const size_t pixels = (size_t)h * w, frame_bytes = pixels * 3, all = frame_bytes * n;
  if (overlap(plate, frame_bytes, samples, all) || (spread && overlap(spread, pixels, samples, all)))
    return fail(VM_EINVAL, "%s: plate and spread must not alias samples", who);
  if (spread && overlap(spread, pixels, plate, frame_bytes))
    return fail(VM_EINVAL, "%s: spread must not alias plate", who);
  const unsigned blocks = (unsigned)((frame_bytes + BLOCK_BYTES - 1) / BLOCK_BYTES);
  PlateKernel kernel = kernels[n - 1];
#ifdef VM_STUDY
  static const bool radix = getenv("VM_PLATE_RADIX") != nullptr;
  if (radix)
    kernel = n == 8 ? plate_kernel<8, true> : n == 16 ? plate_kernel<16, true> : n == 32 ? plate_kernel<32, true>
           : n == 64 ? plate_kernel<64, true> : kernel;
#endif
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), samples,
                     frame_bytes, (int)pixels, plate, spread);
  return check_launch(who);
}
