// vm_plate_gain_fit / vm_plate_gain_apply: one multiplicative gain per frame and colour channel between a frame and its
// background plate, and the plate under that gain (the definition: include/vmatting.h).  Integer arithmetic only, so the
// numpy restatement (tests/plate_gain_ref.py) is matched exactly: gain, support and every byte of the gained plate.
//
// A frame is h w 3 bytes whose byte p belongs to channel p % 3, so the kernels walk it as a flat byte run in units of 12
// bytes (4 pixels): the channel of a unit's byte k is k % 3, known at compile time.  cmp and bg may sit at any byte
// address; a whole unit is read as the aligned dwords around it, shifted into place (vm_common.h's load_bytes), the
// frame's ragged last unit byte by byte.
//
//   zero       the part of `work` the next two launches add into.
//   histogram  per frame and channel H[q] of the valid bytes, q = (64 a + (b >> 1)) / b.  The quotient comes from
//       v_rcp_f32 and one correction step (exact for every pair: t < 2^14, so the estimate is off by at most one, and
//       only downwards).  Each block keeps HIST_COPIES copies of the 3 x 256 bins in LDS, a lane adding into copy
//       lane % HIST_COPIES (copy-minor, so the lanes of one bin spread over HIST_COPIES banks), and a thread first merges
//       the equal bins among its unit's four bytes of a channel into one add: in a real frame nearly every pixel falls
//       into three or four bins, and same-address LDS atomics are serviced one after another.  The block then adds its
//       non-empty bins to the frame's histogram in `work`.  Integer atomics: the result does not depend on their order.
//   sums       every block finds its frame's three modes q0 from the finished histogram (768 loads, one max-reduction of
//       (S << 8 | 255 - q) keys: the largest S, and among equals the smallest q), then walks its share of the frame
//       again: count, sum a b and sum b b over the inliers, per unit in 32 bits (4 x 250 x 250 fits), across units in
//       64, reduced by wave shuffles, then in LDS, then nine 64-bit atomic adds per block.
//   finish     one thread per frame and channel: the rounded quotient (or the identity), and the support.
//   apply      a thread makes 16 output bytes that are 16-byte aligned in memory (one 16-byte store), from the plate's
//       bytes at the same frame offset (aligned dwords shifted into place); the channel phase of the chunk rotates the
//       three gains once.  The bytes of a frame before its first and after its last aligned chunk go byte by byte.
//
// The fit reads 12 B per pixel (both planes twice; the second read of a 1080p frame comes from L2 / Infinity Cache);
// the apply reads 3 and writes 3.
#include "vm_common.h"

#include <climits>

namespace vm {
namespace {

constexpr int BAND_MAX = 16, SHARE_MAX = 4096;
constexpr int Q_LO = 16, Q_HI = 254;                // the mode's range; valid quotients are 0..254
constexpr int UNIT = 12;                            // bytes per thread and step: 4 pixels, channel of byte k = k % 3
constexpr int HIST_COPIES = 8;
constexpr int BINS = 256, HIST_WORDS = 3 * BINS;    // per frame in `work`: uint32 H[3][256], then
constexpr int SUM_WORDS = 9;                        // 64-bit {count, sum a b, sum b b}[3]
constexpr size_t FRAME_WORK = HIST_WORDS * 4 + 128; // (the sums 16-byte aligned, the next frame too)
static_assert(SUM_WORDS * 8 <= 128, "the sums fit their slot");
constexpr int GAIN_ONE = 4096, GAIN_CLAMP = 1 << 20;

// the unit at frame offset `off` of a plane of `len` bytes: whole as dwords, the frame's last one byte by byte with
// zeros behind the frame's end (a zero plate byte is not valid, so those bytes count nowhere)
__device__ __forceinline__ void load_unit(const uint8_t* __restrict__ p, long off, long len, uint32_t* d) {
  if (off + UNIT <= len) {
    load_bytes<UNIT / 4>(p + off, d);
    return;
  }
  d[0] = d[1] = d[2] = 0u;
  for (int k = 0; off + k < len; ++k) d[k >> 2] |= (uint32_t)p[off + k] << (8 * (k & 3));
}

// valid: 16 <= b <= 250, a <= 250 and t = 64 a + (b >> 1) < 255 b
__device__ __forceinline__ bool valid_pair(uint32_t a, uint32_t b, uint32_t t) {
  return b - 16u <= 234u && a <= 250u && t < 255u * b;
}

// t / b for 1 <= b <= 255, t < 2^14: the f32 estimate is within 0.001 of the quotient, whose fraction is at most
// 1 - 1/255, so truncation gives the quotient or one less
__device__ __forceinline__ uint32_t div_byte(uint32_t t, uint32_t b) {
  uint32_t q = (uint32_t)((float)t * __builtin_amdgcn_rcpf((float)b));
  const int r = (int)t - (int)(q * b);
  q += r >= (int)b;
  q -= r < 0;
  return q;
}

__global__ void __launch_bounds__(256) gain_zero_kernel(uint4* __restrict__ work, long n16) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) work[i] = make_uint4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(256)
gain_hist_kernel(const uint8_t* __restrict__ cmp, const uint8_t* __restrict__ bg, int nb, long len, long units, int bpf,
                 unsigned char* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) uint32_t lh[HIST_WORDS * HIST_COPIES];
  const int t = threadIdx.x, f = blockIdx.x / bpf, bx = blockIdx.x - f * bpf, copy = t & (HIST_COPIES - 1);
  for (int i = t; i < HIST_WORDS * HIST_COPIES; i += 256) lh[i] = 0u;
  __syncthreads();
  const uint8_t* pc = cmp + (size_t)f * len;
  const uint8_t* pb = bg + (size_t)(nb == 1 ? 0 : f) * len;
  for (long u = (long)bx * 256 + t; u < units; u += (long)bpf * 256) {
    uint32_t da[UNIT / 4], db[UNIT / 4];
    load_unit(pc, u * UNIT, len, da);
    load_unit(pb, u * UNIT, len, db);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int q[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t a = byte_of(da, 3 * p + c), b = byte_of(db, 3 * p + c), tt = 64u * a + (b >> 1);
        q[p] = valid_pair(a, b, tt) ? (int)div_byte(tt, b) : -1;
      }
      // one add per distinct bin among the four: byte p adds its bin's count unless an earlier byte had the same bin
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        bool first = q[p] >= 0;
        uint32_t cnt = 1u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < p) first = first && q[j] != q[p];
          if (j > p) cnt += q[j] == q[p];
        }
        if (first) atomicAdd(&lh[(c * BINS + q[p]) * HIST_COPIES + copy], cnt);
      }
    }
  }
  __syncthreads();
  uint32_t* H = reinterpret_cast<uint32_t*>(work + (size_t)f * FRAME_WORK);
  for (int i = t; i < HIST_WORDS; i += 256) {
    const uint4 lo = *reinterpret_cast<const uint4*>(&lh[i * HIST_COPIES]);
    const uint4 hi = *reinterpret_cast<const uint4*>(&lh[i * HIST_COPIES + 4]);
    static_assert(HIST_COPIES == 8, "two 16-byte reads per bin");
    const uint32_t s = lo.x + lo.y + lo.z + lo.w + hi.x + hi.y + hi.z + hi.w;
    if (s) atomicAdd(&H[i], s);
  }
}

__global__ void __launch_bounds__(256)
gain_sums_kernel(const uint8_t* __restrict__ cmp, const uint8_t* __restrict__ bg, int nb, long len, long units, int bpf,
                 int band, unsigned char* __restrict__ work) {
  __shared__ unsigned long long keys[3][4];
  __shared__ unsigned long long part[4][SUM_WORDS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, f = blockIdx.x / bpf, bx = blockIdx.x - f * bpf;
  const uint32_t* H = reinterpret_cast<const uint32_t*>(work + (size_t)f * FRAME_WORK);
  // thread t is bin t of every channel: S = H[t - 1] + H[t] + H[t + 1]; the key orders by S, then by the smaller bin
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    unsigned long long key = 0ull;
    if (t >= Q_LO && t <= Q_HI) {
      const unsigned long long s = (unsigned long long)H[c * BINS + t - 1] + H[c * BINS + t] +
                                   (t + 1 < BINS - 1 ? H[c * BINS + t + 1] : 0u);
      key = (s << 8) | (unsigned long long)(255 - t);
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_down(key, o);
      key = other > key ? other : key;
    }
    if (lane == 0) keys[c][wave] = key;
  }
  __syncthreads();
  int q0[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    unsigned long long key = keys[c][0];
#pragma unroll
    for (int v = 1; v < 4; ++v) key = keys[c][v] > key ? keys[c][v] : key;
    q0[c] = 255 - (int)(key & 255ull);
  }

  const uint8_t* pc = cmp + (size_t)f * len;
  const uint8_t* pb = bg + (size_t)(nb == 1 ? 0 : f) * len;
  unsigned long long acc[SUM_WORDS];
#pragma unroll
  for (int i = 0; i < SUM_WORDS; ++i) acc[i] = 0ull;
  for (long u = (long)bx * 256 + t; u < units; u += (long)bpf * 256) {
    uint32_t da[UNIT / 4], db[UNIT / 4];
    load_unit(pc, u * UNIT, len, da);
    load_unit(pb, u * UNIT, len, db);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t cnt = 0u, sab = 0u, sbb = 0u;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t a = byte_of(da, 3 * p + c), b = byte_of(db, 3 * p + c), tt = 64u * a + (b >> 1);
        int dev = (int)(64u * a) - q0[c] * (int)b;
        dev = dev < 0 ? -dev : dev;
        const bool in = valid_pair(a, b, tt) && dev <= band * (int)b;
        cnt += in;
        sab += in ? a * b : 0u;
        sbb += in ? b * b : 0u;
      }
      acc[3 * c] += cnt;
      acc[3 * c + 1] += sab;
      acc[3 * c + 2] += sbb;
    }
  }
#pragma unroll
  for (int i = 0; i < SUM_WORDS; ++i) {
    for (int o = 32; o > 0; o >>= 1) acc[i] += __shfl_down(acc[i], o);
    if (lane == 0) part[wave][i] = acc[i];
  }
  __syncthreads();
  if (t < SUM_WORDS) {
    const unsigned long long s = part[0][t] + part[1][t] + part[2][t] + part[3][t];
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(work + (size_t)f * FRAME_WORK + HIST_WORDS * 4);
    if (s) atomicAdd(&sums[t], s);
  }
}

__global__ void __launch_bounds__(64)
gain_finish_kernel(const unsigned char* __restrict__ work, int n, long pixels, int min_share, int32_t* __restrict__ gain,
                   int32_t* __restrict__ support) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= 3 * n) return;
  const int f = i / 3, c = i - 3 * f;
  const long long* s = reinterpret_cast<const long long*>(work + (size_t)f * FRAME_WORK + HIST_WORDS * 4) + 3 * c;
  const long long cnt = s[0], N = s[1], D = s[2];
  gain[i] = cnt * min_share >= pixels ? (int32_t)((4096 * N + (D >> 1)) / D) : GAIN_ONE;  // (cnt >= 1: D >= 256)
  support[i] = (int32_t)cnt;
}

__device__ __forceinline__ uint32_t gained(uint32_t b, uint32_t g) {
  const uint32_t v = (g * b + 2048u) >> 12;
  return v < 255u ? v : 255u;
}

// chunk j of frame f: the 16 bytes at `body` + 16 j of the frame's output, `body` the frame offset of its first 16-byte
// aligned output byte
__global__ void __launch_bounds__(256)
gain_apply_kernel(const uint8_t* __restrict__ bg, int nb, const int32_t* __restrict__ gain, long len, int bpf,
                  uint8_t* __restrict__ out) {
  const int f = blockIdx.x / bpf, bx = blockIdx.x - f * bpf;
  const uint8_t* src = bg + (size_t)(nb == 1 ? 0 : f) * len;
  uint8_t* dst = out + (size_t)f * len;
  uint32_t g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = gain[3 * f + c];  // outside 0 .. 2^20 the result is that of the nearer end, and g * 255 fits
    g[c] = (uint32_t)(v < 0 ? 0 : v > GAIN_CLAMP ? GAIN_CLAMP : v);
  }
  const long head = (long)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
  const long body = head < len ? head : len, chunks = (len - body) / 16, tail = body + 16 * chunks;
  for (long j = (long)bx * 256 + threadIdx.x; j < chunks; j += (long)bpf * 256) {
    const long off = body + 16 * j;
    const int c0 = (int)(off % 3);
    // byte k of the chunk is channel (c0 + k) % 3
    const uint32_t r0 = c0 == 0 ? g[0] : c0 == 1 ? g[1] : g[2], r1 = c0 == 0 ? g[1] : c0 == 1 ? g[2] : g[0],
                   r2 = c0 == 0 ? g[2] : c0 == 1 ? g[0] : g[1];
    uint32_t d[4], o[4];
    load_bytes<4>(src + off, d);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 4 * e + i;
        o[e] |= gained(byte_of(d, k), k % 3 == 0 ? r0 : k % 3 == 1 ? r1 : r2) << (8 * i);
      }
    }
    *reinterpret_cast<uint4*>(dst + off) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  // the at most 15 bytes before the first chunk and after the last: the first threads of the frame's first block
  if (bx == 0) {
    const long ragged = body + (len - tail);
    for (long i = threadIdx.x; i < ragged; i += 256) {
      const long off = i < body ? i : tail + (i - body);
      dst[off] = (uint8_t)gained(src[off], g[off % 3]);
    }
  }
}

// blocks per frame (bpf; block b of the 1-D grid is block b % bpf of frame b / bpf) for `items` items of one thread
// each, about `steps` per thread, all frames together within 4096 where that leaves every frame a block
inline int frame_blocks(long items, int steps, int n) {
  long b = (items + 256L * steps - 1) / (256L * steps);
  const long cap = 4096 / n > 1 ? 4096 / n : 1;
  b = b > cap ? cap : b;
  return (int)(b < 1 ? 1 : b);
}

inline bool bytes_ok(int n, int h, int w) { return shape_ok(n, h, w) && (long)n * h * w <= (long)INT_MAX / 3; }

}  // namespace
}  // namespace vm

using namespace vm;

extern "C" size_t vm_plate_gain_workspace_bytes(int n) {
  if (n < 1 || (long)n * 3 > (long)INT_MAX) return 0;
  return (size_t)n * FRAME_WORK;
}

extern "C" int vm_plate_gain_fit(const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int band,
                                 int min_share, int32_t* gain, int32_t* support, void* work, void* stream) {
  const char* who = "plate_gain_fit";
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!bytes_ok(n, h, w)) return fail(VM_EINVAL, "%s: %d x %d x %d x 3 bytes exceed %d", who, n, h, w, INT_MAX);
  if (nb != 1 && nb != n) return fail(VM_EINVAL, "%s: %d background frames for %d frames (1 or n)", who, nb, n);
  if (band < 1 || band > BAND_MAX) return fail(VM_EINVAL, "%s: band %d (1..%d)", who, band, BAND_MAX);
  if (min_share < 1 || min_share > SHARE_MAX)
    return fail(VM_EINVAL, "%s: min_share %d (1..%d)", who, min_share, SHARE_MAX);
  if (!cmp || !bg || !gain || !support || !work)
    return fail(VM_EINVAL, "%s: null cmp / bg / gain / support / work", who);
  if (reinterpret_cast<uintptr_t>(gain) % 4 || reinterpret_cast<uintptr_t>(support) % 4)
    return fail(VM_EINVAL, "%s: gain and support must be 4-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(work) % 16) return fail(VM_EINVAL, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long len = (long)h * w * 3, units = (len + UNIT - 1) / UNIT, n16 = (long)(n * FRAME_WORK / 16);
  unsigned char* wk = static_cast<unsigned char*>(work);
  hipLaunchKernelGGL(gain_zero_kernel, dim3((unsigned)grid_for(n16, 256)), dim3(256), 0, st,
                     reinterpret_cast<uint4*>(wk), n16);
  const int bpf = frame_blocks(units, 8, n);
  const dim3 grid((unsigned)bpf * n);  // (at most max(4096, n) blocks)
  hipLaunchKernelGGL(gain_hist_kernel, grid, dim3(256), 0, st, cmp, bg, nb, len, units, bpf, wk);
  hipLaunchKernelGGL(gain_sums_kernel, grid, dim3(256), 0, st, cmp, bg, nb, len, units, bpf, band, wk);
  hipLaunchKernelGGL(gain_finish_kernel, dim3((unsigned)((3 * n + 63) / 64)), dim3(64), 0, st, wk, n, (long)h * w,
                     min_share, gain, support);
  return check_launch(who);
}

extern "C" int vm_plate_gain_apply(const uint8_t* bg, int nb, const int32_t* gain, int n, int h, int w, uint8_t* out,
                                   void* stream) {
  const char* who = "plate_gain_apply";
  if (n < 1 || h < 1 || w < 1) return fail(VM_EINVAL, "%s: bad shape [%d,%d,%d]", who, n, h, w);
  if (!bytes_ok(n, h, w)) return fail(VM_EINVAL, "%s: %d x %d x %d x 3 bytes exceed %d", who, n, h, w, INT_MAX);
  if (nb != 1 && nb != n) return fail(VM_EINVAL, "%s: %d background frames for %d frames (1 or n)", who, nb, n);
  if (!bg || !gain || !out) return fail(VM_EINVAL, "%s: null bg / gain / out", who);
  if (reinterpret_cast<uintptr_t>(gain) % 4) return fail(VM_EINVAL, "%s: gain must be 4-byte aligned", who);
  const size_t len = (size_t)h * w * 3;
  if (overlap(out, n * len, bg, nb * len) || overlap(out, n * len, gain, (size_t)n * 12))
    return fail(VM_EINVAL, "%s: out must not overlap bg or gain", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int bpf = frame_blocks((long)(len / 16) + 1, 4, n);
  hipLaunchKernelGGL(gain_apply_kernel, dim3((unsigned)bpf * n), dim3(256), 0, st, bg, nb, gain, (long)len, bpf, out);
  return check_launch(who);
}
