// 3x3 SAME convs over cin <= 8 (one 16-byte chunk per pixel): the first layer (conv1_1, unet.py:65-74) and the refine
// conv + channel softmax (refine.py:18-31) in bf16 and f32.  Kernels and their launchers; conv3x3.hip's dispatch_mfma
// decides when each applies.
#include <algorithm>
#include <type_traits>

#include "conv_dispatch.h"

namespace vm {

// ================================================================ first layer: cin <= 8 (conv1_1, unet.py:65-74)
// One 16-byte chunk per pixel, so a 32-deep MFMA K-step covers 4 taps x 8 channels: lane group q of the pixel
// fragment reads the patch row shifted by tap 4j+q (taps >= 9 read as zero), matching the tap-major packing
// k = tap*8 + c.  The 10 x 34 patch (5.4 KB) is loaded once per tile; the 64 x 96 weight slice sits in LDS (12 KB,
// one uint4 per MFMA operand lane: in registers it took 48 VGPRs and the persistent loop spilled).
// 8 waves of 32 px x 64 channels; same bf16 slab epilogue as the patch kernel.  Persistent: a block walks tiles
// b, b + G, ... (G a multiple of 8, so xcd_tile keeps each block on its XCD's tile range) with the next tile's
// patch chunk in flight in a register while the current one computes and stores, and reloads its weight slice
// only when the output-channel block changes.  (One tile per block spent ~10 us of serial load latency per tile
// at 2 resident blocks per CU: 185 us for the training towers' 2.5 M pixels, 1.7 TB/s of stores.)
__global__ __launch_bounds__(512, 4) void conv3x3_first(ConvArgs a) {
  using T = uint16_t;
  constexpr int TH = 8, TW = 32, PW = TW + 2, PPIX = (TH + 2) * PW, BM = TH * TW, SR = 64 * 2 + 16;
  __shared__ __attribute__((aligned(16))) uint4 patch[PPIX];
  __shared__ __attribute__((aligned(16))) char stg[BM * SR];
  __shared__ __attribute__((aligned(16))) uint4 wl[3][4][64];  // the weight slice, one uint4 per (step, fc, lane)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  const int col = lane & 15, q = lane >> 4;
  auto coords = [&](int l, int& n, int& r0, int& c0, int& n0) {
    const int t = xcd_tile(l, a.tiles_total);
    const int st = t / a.tiles_n, nt = t - st * a.tiles_n;
    n = st / (th * tw);
    const int srem = st - n * th * tw;
    r0 = (srem / tw) * TH;
    c0 = (srem - (srem / tw) * tw) * TW;
    n0 = nt * 64;
  };
  auto load_patch = [&](int n, int r0, int c0) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (tid < PPIX) {
      const T* xb = reinterpret_cast<const T*>(a.x) + a.x_coff + ((long)n * H + r0 - 1) * (long)W * cs;
      const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(xb), 0, 0x7ffffff0, 0x00020000);
      const int pr = tid / PW, pc = tid - pr * PW;
      const int h = r0 - 1 + pr, w = c0 - 1 + pc;
      const bool ok = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      const int off = ok ? (pr * W + w) * cs * 2 : OOB;
      v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
    }
    return v;
  };
  const int G = gridDim.x;
  int l = blockIdx.x;
  if (l >= a.tiles_total) return;
  int n, r0, c0, n0, wn0 = -1;
  coords(l, n, r0, c0, n0);
  uint4 pv = load_patch(n, r0, c0);
  for (; l < a.tiles_total; l += G) {
    if (n0 != wn0) {  // block-uniform; the previous tile's MFMAs are behind its two barriers
      const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, n0);
      for (int e = tid; e < 3 * 4 * 64; e += 512) {
        const int j = e >> 8, fc = (e >> 6) & 3, ln = e & 63;
        wl[j][fc][ln] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                      wrs, ((fc * 16 + (ln & 15)) * a.K_pad + j * 32 + (ln >> 4) * 8) * 2,
                                                      0, 0));
      }
      wn0 = n0;
    }
    if (tid < PPIX) patch[tid] = pv;
    __syncthreads();
    // the next tile's patch chunk: in flight through this tile's MFMAs, epilogue and stores
    const int cn = n, cr0 = r0, cc0 = c0, cn0 = n0;
    if (l + G < a.tiles_total) {
      coords(l + G, n, r0, c0, n0);
      pv = load_patch(n, r0, c0);
    }

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k) acc[i][k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int tap = 4 * j + q;
      const int toff = (tap / 3) * PW + tap % 3;
      uint4 bv[2];
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) {
        const int p = wave * 32 + fp * 16;  // tile pixel of the fragment's first row: one patch row per wave
        const uint4 v = patch[(p / TW) * PW + (p % TW) + col + (tap < 9 ? toff : 0)];
        bv[fp] = tap < 9 ? v : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const uint4 wv = wl[j][fc][lane];
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) mma16<T>(wv, bv[fp], acc[fc][fp]);
      }
    }

#pragma unroll
    for (int fc = 0; fc < 4; ++fc) {
      const int cc = fc * 16 + 4 * q;
      float mul[4], add[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int co = min(cn0 + cc + jj, a.cout - 1);
        const float sc = a.scale ? a.scale[co] : 1.f;
        mul[jj] = sc;
        add[jj] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
      }
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) {
        const int row = wave * 32 + fp * 16 + col;
        float v[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          v[jj] = fmaf(acc[fc][fp][jj], mul[jj], add[jj]);
          if (a.act == VM_ACT_RELU) v[jj] = fmaxf(v[jj], 0.f);
          else if (a.act == VM_ACT_SIGMOID) v[jj] = sigmoid_precise(v[jj]);
        }
        uint2 pk;
        pk.x = bf16x2_bits(v[0], v[1]);
        pk.y = bf16x2_bits(v[2], v[3]);
        *reinterpret_cast<uint2*>(stg + row * SR + cc * 2) = pk;
      }
    }
    __syncthreads();
    const int ycs2 = a.y_cstride * 2;
    T* yb = reinterpret_cast<T*>(a.y) + a.y_coff + (((long)cn * H + cr0) * W + cc0) * (long)a.y_cstride + cn0;
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yb, 0, 0x7ffffff0, 0x00020000);
#pragma unroll
    for (int it = 0; it < BM * 8 / 512; ++it) {
      const int idx = it * 512 + tid;
      const int rr = idx >> 3, cq = idx & 7;
      const uint4 d = *reinterpret_cast<const uint4*>(stg + rr * SR + cq * 16);
      const int pr = rr / TW, pc = rr % TW;
      const bool ok = cr0 + pr < H && cc0 + pc < W && cn0 + cq * 8 < a.cout;
      const int off = ok ? (pr * W + pc) * ycs2 + cq * 16 : OOB;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), yrs,
                                             off, 0, 0);
    }
  }
}

// {x[l], x[l ^ 16]} and {x[l], x[l ^ 32]} in VALU (v_permlane16/32_swap of x with itself) instead of ds_bpermute:
// max and + of the pair are commutative, so the results equal fmaxf / + with __shfl_xor bit for bit
__device__ __forceinline__ float max_xor16(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float max_xor32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float add_xor16(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float add_xor32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ================================================================ refine conv4 + softmax (refine.py:27-32)
// RefineNet's only live layer: a cin <= 8 -> 64 3x3 conv whose 64 logits per pixel go straight into
// tf.nn.softmax and out as f32.  The conv is conv3x3_first's (one 16-byte chunk per pixel, 4 taps x 8 channels
// per K-step, the 64 x 96 weight slice in registers); the softmax never leaves registers: a pixel's 64 logits
// sit in the 4 lanes col, col+16, col+32, col+48 (16 each), so two xor-shuffles give the row max and the row
// sum.  Every lane then stores its four 16-byte channel quads (a wave store covers 16 pixels x 64 contiguous
// bytes).  The kernel writes 256 B per pixel and reads 16: HBM-write-bound.  NT: nontemporal stores (the
// 531 MB 1080p output is never re-read by this pass).
// STG: each wave transposes its 16 pixels x 64 channels through a private LDS slab so that every store instruction
// writes 4 whole pixels (1 KB contiguous when the output is dense) instead of 16 pixels x 64 bytes.
// WL: the weight fragments staged once per block in LDS instead of 48 registers (4 waves per SIMD without spills)
template <bool NT, bool STG = false, bool WL = false>
__global__ __launch_bounds__(512, WL ? 4 : 2) void conv3x3_first_softmax(ConvArgs a) {
  using T = uint16_t;
  constexpr int TH = 8, TW = 32, PW = TW + 2, PPIX = (TH + 2) * PW;
  constexpr int SRF = 68;  // staging row: 64 floats + 4 (rows 272 B apart)
  __shared__ __attribute__((aligned(16))) uint4 patch[PPIX];
  __shared__ __attribute__((aligned(16))) float stg[STG ? 8 * 16 * SRF : 4];
  __shared__ __attribute__((aligned(16))) float rmul[2 * 64];  // per-channel scale, bias*scale + shift
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  const int ntiles = a.tiles_total;
  // persistent: the block walks tiles blockIdx.x, +gridDim.x, ... (bands of consecutive tiles per XCD); the next
  // tile's patch pixel is loaded into a register while the current tile computes and stores
  auto tile_of = [&](int i) {  // a partial last round keeps block order (the band remap is a bijection of a full one)
    const int base = (i / a.tiles_n) * a.tiles_n;
    return base + a.tiles_n <= ntiles ? base + xcd_tile(i - base, a.tiles_n) : i;
  };
  auto load_patch = [&](int t) {
    const int n = t / (th * tw), srem = t - n * th * tw;
    const int r0 = (srem / tw) * TH, c0 = (srem - (srem / tw) * tw) * TW;
    const int pr = tid / PW, pc = tid - pr * PW;
    const int h = r0 - 1 + pr, w = c0 - 1 + pc;
    const bool ok = tid < PPIX && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
    const T* xb = reinterpret_cast<const T*>(a.x) + a.x_coff + ((long)n * H + (ok ? h : 0)) * (long)W * cs;
    return ok ? *reinterpret_cast<const uint4*>(xb + (long)w * cs) : make_uint4(0, 0, 0, 0);
  };
  const int col = lane & 15, q = lane >> 4;
  const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, 0);
  __shared__ __attribute__((aligned(16))) uint4 wlds[WL ? 3 * 4 * 64 : 1];
  uint4 wf[WL ? 1 : 3][4];
  if constexpr (WL) {
    for (int e = tid; e < 3 * 4 * 64; e += 512) {  // [j][fc][lane]
      const int j = e >> 8, fc = (e >> 6) & 3, l = e & 63;
      wlds[e] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                              wrs, ((fc * 16 + (l & 15)) * a.K_pad + j * 32 + (l >> 4) * 8) * 2, 0, 0));
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int fc = 0; fc < 4; ++fc)
        wf[j][fc] = __builtin_bit_cast(
            uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, ((fc * 16 + col) * a.K_pad + j * 32 + q * 8) * 2, 0, 0));
  }
  if (tid < 64) {  // constants in LDS (read per tile): 2 blocks per CU fit the register file
    const float sc = a.scale ? a.scale[tid] : 1.f;
    rmul[tid] = sc;
    rmul[64 + tid] = (a.bias ? a.bias[tid] : 0.f) * sc + (a.shift ? a.shift[tid] : 0.f);
  }
  int i = blockIdx.x;
  uint4 nxt = i < ntiles ? load_patch(tile_of(i)) : make_uint4(0, 0, 0, 0);
  for (; i < ntiles; i += gridDim.x) {
    const int t = tile_of(i);
    const int n = t / (th * tw), srem = t - n * th * tw;
    const int r0 = (srem / tw) * TH, c0 = (srem - (srem / tw) * tw) * TW;
    __syncthreads();  // the previous tile's patch reads are done
    if (tid < PPIX) patch[tid] = nxt;
    __syncthreads();
    if (i + (int)gridDim.x < ntiles) nxt = load_patch(tile_of(i + gridDim.x));

    f32x4 acc[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) acc[k][fp] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int tap = 4 * j + q;
      const int toff = (tap / 3) * PW + tap % 3;
      uint4 bv[2];
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) {
        const uint4 v = patch[wave * PW + fp * 16 + col + (tap < 9 ? toff : 0)];  // patch row `wave` + kernel row
        bv[fp] = tap < 9 ? v : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const uint4 wv = WL ? wlds[(j * 4 + fc) * 64 + lane] : wf[WL ? 0 : j][fc];
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) mma16<T>(wv, bv[fp], acc[fc][fp]);
      }
    }

    const int ycs = a.y_cstride;
    float* yb = reinterpret_cast<float*>(a.y) + a.y_coff + (((long)n * H + r0 + wave) * W + c0) * (long)ycs;
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) {
      float v[4][4];
      float mx = -INFINITY;
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const float4 m4 = *reinterpret_cast<const float4*>(rmul + fc * 16 + 4 * q);
        const float4 a4 = *reinterpret_cast<const float4*>(rmul + 64 + fc * 16 + 4 * q);
        const float mul[4] = {m4.x, m4.y, m4.z, m4.w}, add[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          v[fc][jj] = fmaf(acc[fc][fp][jj], mul[jj], add[jj]);
          mx = fmaxf(mx, v[fc][jj]);
        }
      }
      mx = max_xor32(max_xor16(mx));
      float sum = 0.f;
#pragma unroll
      for (int fc = 0; fc < 4; ++fc)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          v[fc][jj] = expf(v[fc][jj] - mx);
          sum += v[fc][jj];
        }
      sum = add_xor32(add_xor16(sum));
      const float inv = 1.f / sum;
      if constexpr (STG) {
        float* ws = stg + wave * 16 * SRF;
#pragma unroll
        for (int fc = 0; fc < 4; ++fc)
          *reinterpret_cast<f32x4*>(ws + col * SRF + fc * 16 + 4 * q) =
              f32x4{v[fc][0] * inv, v[fc][1] * inv, v[fc][2] * inv, v[fc][3] * inv};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 4; ++it) {  // lane l: pixel 4*it + l/16, channels 4*(l%16) .. +3
          const int px = 4 * it + (lane >> 4), ch = 4 * (lane & 15);
          const f32x4 o = *reinterpret_cast<const f32x4*>(ws + px * SRF + ch);
          const int pc = fp * 16 + px;
          if (r0 + wave < H && c0 + pc < W) {
            float* yp = yb + (long)pc * ycs + ch;
            if constexpr (NT) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(yp));
            else *reinterpret_cast<f32x4*>(yp) = o;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // reads done before the next fragment's writes
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      } else {
        const int pc = fp * 16 + col;
        if (r0 + wave < H && c0 + pc < W) {
          float* yp = yb + (long)pc * ycs + 4 * q;
#pragma unroll
          for (int fc = 0; fc < 4; ++fc) {
            const f32x4 o = f32x4{v[fc][0] * inv, v[fc][1] * inv, v[fc][2] * inv, v[fc][3] * inv};
            if constexpr (NT) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(yp + fc * 16));
            else *reinterpret_cast<f32x4*>(yp + fc * 16) = o;
          }
        }
      }
    }
  }
}

// The refine softmax of one wave's 32-pixel x 64-channel accumulator strip (acc[fc][fp]: MFMA 16x16 layout, pixel
// fp*16 + col, channels fc*16 + 4q .. +3), its per-channel affine from rmul ([scale | bias*scale + shift]), and the
// whole-pixel nontemporal stores through the wave's private 16 x 68-float LDS slab `ws`: every store instruction
// writes 4 whole pixels.  `valid` = pixels of the strip inside the frame.
// strip accumulators: zero (the epilogue applies the affine), or the bias (no scale / shift: rmul[64..] = bias)
__device__ __forceinline__ void init_strip_acc(f32x4 (&acc)[4][2], const float* rmul, bool aff, int q) {
#pragma unroll
  for (int fc = 0; fc < 4; ++fc) {
    const f32x4 b = aff ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(rmul + 64 + fc * 16 + 4 * q);
    acc[fc][0] = b;
    acc[fc][1] = b;
  }
}

// AFF: apply rmul's per-channel affine; without it the accumulators already hold the logits (the kernel started
// them at the bias: the refine conv has no BN, scale/shift are absent).  The exponential is v_exp_f32 on x*log2(e)
// (__expf): for the softmax of logits bounded by max-subtraction its relative error (~1e-6 near 0, below 1e-5
// absolute on every probability) is far inside the 1e-4 bound, at a third of expf's instructions — this epilogue is
// the VALU-bound half of the kernel.
template <bool AFF>
__device__ __forceinline__ void softmax_store_strip(const f32x4 (&acc)[4][2], const float* rmul, float* ws, float* yb,
                                                    int ycs, int valid, int lane) {
  constexpr int SRF = 68;
  const int col = lane & 15, q = lane >> 4;
#pragma unroll
  for (int fp = 0; fp < 2; ++fp) {
    float v[4][4];
    float mx = -INFINITY;
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) {
      if constexpr (AFF) {
        const float4 m4 = *reinterpret_cast<const float4*>(rmul + fc * 16 + 4 * q);
        const float4 a4 = *reinterpret_cast<const float4*>(rmul + 64 + fc * 16 + 4 * q);
        const float mul[4] = {m4.x, m4.y, m4.z, m4.w}, add[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) v[fc][jj] = fmaf(acc[fc][fp][jj], mul[jj], add[jj]);
      } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) v[fc][jj] = acc[fc][fp][jj];
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) mx = fmaxf(mx, v[fc][jj]);
    }
    mx = max_xor32(max_xor16(mx));
    float sum = 0.f;
#pragma unroll
    for (int fc = 0; fc < 4; ++fc)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        v[fc][jj] = __expf(v[fc][jj] - mx);
        sum += v[fc][jj];
      }
    sum = add_xor32(add_xor16(sum));
    const float inv = 1.f / sum;
#pragma unroll
    for (int fc = 0; fc < 4; ++fc)
      *reinterpret_cast<f32x4*>(ws + col * SRF + fc * 16 + 4 * q) =
          f32x4{v[fc][0] * inv, v[fc][1] * inv, v[fc][2] * inv, v[fc][3] * inv};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 4; ++it) {  // lane l: pixel 4*it + l/16, channels 4*(l%16) .. +3
      const int px = 4 * it + (lane >> 4), ch = 4 * (lane & 15);
      const f32x4 o = *reinterpret_cast<const f32x4*>(ws + px * SRF + ch);
      const int pc = fp * 16 + px;
      if (pc < valid) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(yb + (long)pc * ycs + ch));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// bf16 refine conv4 + softmax on wave-private strips (see conv3x3_first_softmax_f32 below for the strip scheme): the
// conv is conv3x3_first's (one 16-byte pixel chunk per lane, 4 taps x 8 channels per 32-deep K-step, 3 steps); each
// wave stages its 3 x 34-pixel patch, the weight fragments live in LDS ([step][fc][lane]), no block barrier per tile.
__global__ __launch_bounds__(512, 4) void conv3x3_first_softmax_strip(ConvArgs a) {
  using T = uint16_t;
  constexpr int TH = 8, TW = 32, PW = TW + 2, SP = 3 * PW;
  constexpr int SRF = 68;
  __shared__ __attribute__((aligned(16))) uint4 wlds[3 * 4 * 64];
  __shared__ __attribute__((aligned(16))) float rmul[2 * 64];
  __shared__ __attribute__((aligned(16))) uint4 pat[8 * SP];
  __shared__ __attribute__((aligned(16))) float stg[8 * 16 * SRF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  const int ntiles = a.tiles_total;
  auto tile_of = [&](int i) {
    const int base = (i / a.tiles_n) * a.tiles_n;
    return base + a.tiles_n <= ntiles ? base + xcd_tile(i - base, a.tiles_n) : i;
  };
  auto load_strip = [&](int t, uint4 (&v)[2]) {
    const int n = t / (th * tw), srem = t - n * th * tw;
    const int r = (srem / tw) * TH + wave, c0 = (srem - (srem / tw) * tw) * TW;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const int pr = e / PW, pc = e - pr * PW;
      const int h = r - 1 + pr, w = c0 - 1 + pc;
      const bool ok = e < SP && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      const T* xp = reinterpret_cast<const T*>(a.x) + a.x_coff + ((long)n * H + (ok ? h : 0)) * (long)W * cs +
                    (long)(ok ? w : 0) * cs;
      v[k] = ok ? *reinterpret_cast<const uint4*>(xp) : make_uint4(0, 0, 0, 0);
    }
  };
  const int col = lane & 15, q = lane >> 4;
  const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, 0);
  for (int e = tid; e < 3 * 4 * 64; e += 512) {  // [j][fc][lane]
    const int j = e >> 8, fc = (e >> 6) & 3, l = e & 63;
    wlds[e] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                            wrs, ((fc * 16 + (l & 15)) * a.K_pad + j * 32 + (l >> 4) * 8) * 2, 0, 0));
  }
  if (tid < 64) {
    const float sc = a.scale ? a.scale[tid] : 1.f;
    rmul[tid] = sc;
    rmul[64 + tid] = (a.bias ? a.bias[tid] : 0.f) * sc + (a.shift ? a.shift[tid] : 0.f);
  }
  uint4* P = pat + wave * SP;
  const bool aff = a.scale || a.shift;  // else the accumulators start at the bias and hold the logits
  __syncthreads();  // the only block-wide barrier: the staged tables
  int i = blockIdx.x;
  uint4 nv[2];
  if (i < ntiles) load_strip(tile_of(i), nv);
  for (; i < ntiles; i += gridDim.x) {
    const int t = tile_of(i);
    const int n = t / (th * tw), srem = t - n * th * tw;
    const int r = (srem / tw) * TH + wave, c0 = (srem - (srem / tw) * tw) * TW;
    P[lane] = nv[0];
    if (lane + 64 < SP) P[lane + 64] = nv[1];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (i + (int)gridDim.x < ntiles) load_strip(tile_of(i + gridDim.x), nv);
    if (r >= H) continue;
    f32x4 acc[4][2];
    init_strip_acc(acc, rmul, aff, q);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int tap = 4 * j + q;
      const int toff = (tap / 3) * PW + tap % 3;
      uint4 bv[2];
#pragma unroll
      for (int fp = 0; fp < 2; ++fp) {
        const uint4 v = P[fp * 16 + col + (tap < 9 ? toff : 0)];
        bv[fp] = tap < 9 ? v : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const uint4 wv = wlds[(j * 4 + fc) * 64 + lane];
#pragma unroll
        for (int fp = 0; fp < 2; ++fp) mma16<T>(wv, bv[fp], acc[fc][fp]);
      }
    }
    float* yb = reinterpret_cast<float*>(a.y) + a.y_coff + (((long)n * H + r) * W + c0) * (long)a.y_cstride;
    if (aff) softmax_store_strip<true>(acc, rmul, stg + wave * 16 * SRF, yb, a.y_cstride, W - c0, lane);
    else softmax_store_strip<false>(acc, rmul, stg + wave * 16 * SRF, yb, a.y_cstride, W - c0, lane);
  }
}

// ================================================================ refine conv4 + softmax in f32 (refine.py:27-32)
// The reference's precision for config 3: f32 input row [cmp, alpha, warped] (CIN <= 8 of an 8-channel pixel), exact
// f32 products on v_mfma_f32_16x16x4_f32, f32 sums, f32 softmax.  K is COMPACT: k = tap * CIN + c over the 9 * CIN
// real taps (45 for the refine's CIN 5 -> 12 four-deep MFMA steps instead of the 18 of the padded 72); the lane in
// k-slot q of step s reads tap (4s+q) / CIN, channel (4s+q) % CIN.
// Work unit = one wave's STRIP (1 output row x 32 px x 64 channels): the wave stages its own 3 x 34 px patch in LDS as
// channel planes (the 16 lanes of a k-slot read 16 consecutive pixels: conflict-free) and never waits for the other
// waves, so one wave's MFMA phase (12 steps x 8 MFMAs of 32 cycles) runs under another's softmax + store phase; a
// block-wide barrier per tile had serialised the two (0.225 ms at 1080p).  The 8 waves of a block take the 8 rows of
// one 8 x 32 tile (their halo rows meet in L1/L2), tiles walk persistently in XCD bands.  Weights and per-lane patch
// offsets are staged once per block ([step][lane] records: one ds_read_b128 for the 4 cout fragments + one offset);
// the next strip's pixels are prefetched into registers.  Softmax + per-wave LDS transpose + whole-pixel nontemporal
// stores as in conv3x3_first_softmax.
template <int CIN, int ABL = 0>  // ABL (study builds only, results are garbage): 1 = no softmax / store, 2 = no MFMA
__global__ __launch_bounds__(512, 4) void conv3x3_first_softmax_f32(ConvArgs a) {
  constexpr int NS = (9 * CIN + 3) / 4;
  constexpr int TH = 8, TW = 32, PW = TW + 2, SP = 3 * PW;  // strip patch: 3 rows x 34 px
  constexpr int WPF = (CIN * SP + 32 + 3) / 4 * 4;            // per-wave patch floats (+ 32 zeros)
  constexpr int ZERO = CIN * SP;
  constexpr int SRF = 68;  // staging row: 64 floats + 4
  __shared__ __attribute__((aligned(16))) f32x4 wl[NS * 64];
  __shared__ int pl[NS * 4];
  __shared__ __attribute__((aligned(16))) float rmul[2 * 64];
  __shared__ __attribute__((aligned(16))) float pat[8 * WPF];
  __shared__ __attribute__((aligned(16))) float stg[8 * 16 * SRF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  const int ntiles = a.tiles_total;
  auto tile_of = [&](int i) {
    const int base = (i / a.tiles_n) * a.tiles_n;
    return base + a.tiles_n <= ntiles ? base + xcd_tile(i - base, a.tiles_n) : i;
  };
  // this wave's strip of tile t: rows r - 1 .. r + 1 (r = tile row 0 + wave), pixels c0 - 1 .. c0 + 32; lane e (and
  // e + 64) fetch patch pixel e
  auto load_strip = [&](int t, float4 (&v)[2][2]) {
    const int n = t / (th * tw), srem = t - n * th * tw;
    const int r = (srem / tw) * TH + wave, c0 = (srem - (srem / tw) * tw) * TW;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const int pr = e / PW, pc = e - pr * PW;
      const int h = r - 1 + pr, w = c0 - 1 + pc;
      const bool ok = e < SP && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      const float* xp = reinterpret_cast<const float*>(a.x) + a.x_coff + ((long)n * H + (ok ? h : 0)) * (long)W * cs +
                        (long)(ok ? w : 0) * cs;
      v[k][0] = ok ? *reinterpret_cast<const float4*>(xp) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[k][1] = ok && CIN > 4 ? *reinterpret_cast<const float4*>(xp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  const int col = lane & 15, q = lane >> 4;
  const float* Wt = reinterpret_cast<const float*>(a.w);
  for (int e = tid; e < NS * 64; e += 512) {  // wl[s][l] = the 4 cout fragments of lane l's (tap, c) at step s
    const int st = e >> 6, l = e & 63;
    const int kk = 4 * st + (l >> 4), co = l & 15;
    const int tap = kk / CIN, c = kk - tap * CIN;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kk < 9 * CIN)
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) v[fc] = Wt[(long)(fc * 16 + co) * a.K_pad + tap * 8 + c];
    wl[e] = v;
  }
  if (tid < NS * 4) {
    const int kk = tid;  // step tid / 4, k-slot tid % 4
    const int tap = kk / CIN, c = kk - tap * CIN;
    pl[tid] = kk < 9 * CIN ? c * SP + (tap / 3) * PW + tap % 3 : ZERO;  // k past 9 * CIN: 32 zeros
  }
  float* P = pat + wave * WPF;
  if (lane < 32) P[ZERO + lane] = 0.f;
  if (tid < 64) {
    const float sc = a.scale ? a.scale[tid] : 1.f;
    rmul[tid] = sc;
    rmul[64 + tid] = (a.bias ? a.bias[tid] : 0.f) * sc + (a.shift ? a.shift[tid] : 0.f);
  }
  const bool aff = a.scale || a.shift;  // else the accumulators start at the bias and hold the logits
  __syncthreads();  // the only block-wide barrier: the staged tables
  int poff[NS];  // this lane's patch offset of every K step in registers (no dependent LDS load per step)
#pragma unroll
  for (int s = 0; s < NS; ++s) poff[s] = pl[s * 4 + q] + col;
  int i = blockIdx.x;
  float4 nv[2][2];
  if (i < ntiles) load_strip(tile_of(i), nv);
  for (; i < ntiles; i += gridDim.x) {
    const int t = tile_of(i);
    const int n = t / (th * tw), srem = t - n * th * tw;
    const int r = (srem / tw) * TH + wave, c0 = (srem - (srem / tw) * tw) * TW;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const float v[8] = {nv[k][0].x, nv[k][0].y, nv[k][0].z, nv[k][0].w, nv[k][1].x, nv[k][1].y, nv[k][1].z, nv[k][1].w};
      if (e < SP)
#pragma unroll
        for (int c = 0; c < CIN; ++c) P[c * SP + e] = v[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (i + (int)gridDim.x < ntiles) load_strip(tile_of(i + gridDim.x), nv);
    if (r >= H) continue;  // a strip below the frame (wave-uniform): nothing to compute or store

    f32x4 acc[4][2];
    init_strip_acc(acc, rmul, aff, q);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const f32x4 w4 = wl[s * 64 + lane];
      const float b0 = P[poff[s]], b1 = P[poff[s] + 16];
      if constexpr (ABL & 2) {
        asm volatile("" ::"v"(w4[0]), "v"(w4[3]), "v"(b0), "v"(b1));
        continue;
      }
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        acc[fc][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[fc], b0, acc[fc][0], 0, 0, 0);
        acc[fc][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[fc], b1, acc[fc][1], 0, 0, 0);
      }
    }

    if constexpr (ABL & 1) {
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) asm volatile("" ::"v"(acc[fc][0][0]), "v"(acc[fc][1][3]));
      continue;
    }
    float* yb = reinterpret_cast<float*>(a.y) + a.y_coff + (((long)n * H + r) * W + c0) * (long)a.y_cstride;
    if (aff) softmax_store_strip<true>(acc, rmul, stg + wave * 16 * SRF, yb, a.y_cstride, W - c0, lane);
    else softmax_store_strip<false>(acc, rmul, stg + wave * 16 * SRF, yb, a.y_cstride, W - c0, lane);
  }
}

// Pipelined form of conv3x3_first_softmax_f32 (r04): a wave computes strip i+1's MFMAs (accumulator set N) in the same
// basic block as strip i's softmax + stores (set C), so the matrix pipe runs under the VALU-bound softmax instead of
// beside it only when another wave happens to be in the other phase (ablations: the two phases of the non-pipelined
// kernel overlapped by ~0.02 ms).  What makes one basic block possible: the per-wave patch is double-buffered, the
// output is written straight from the accumulator lanes (per (16-pixel fragment, 16-channel group) one store of 16
// pixels x 64 contiguous bytes: the four stores of a fragment fill its 16 whole pixels) through a buffer descriptor
// whose out-of-range offsets drop the pixels past the frame — no LDS transpose, no wave barrier, no branch; the next
// strip's global loads are clamped the same way.  Arithmetic per output is the non-pipelined kernel's (same K order,
// same softmax expression), so results are bit-identical to it.

// The strip softmax of softmax_store_strip cut into 10 chunks, one per K step of the next strip's MFMAs, computed in
// place in the accumulators C (acc[fc][fp]: pixel fp*16 + col, channels fc*16 + 4q .. +3); same operations in the same
// order as softmax_store_strip (max over fc, jj; exp and the sum fc-major), so the probabilities are bit-identical.
// Chunks: 0, 1 affine + row max of fragment 0 / 1; 2 the max across the 4 lane groups; 3..6 exp + partial sums (half a
// fragment each); 7 the sums across lanes and their reciprocals; 8, 9 the scaled stores of fragment 0 / 1, straight
// from the lanes (per 16-channel group one store of 16 pixels x 64 contiguous bytes; pixels past `valid` dropped by
// the buffer descriptor's range check).
// AUX: the stores' cache policy (0: through L2, where the four 64-byte pieces of a pixel's 256-byte row meet before
// write-back; 2: non-temporal, each piece its own partial-line write)
// AUX & 16: the scaled fragment goes through a wave-private LDS slab (16 pixels x 68 floats) and leaves as 4 stores
// of 4 whole pixels (1 KB contiguous for a dense 64-channel output), with cache policy AUX & 15.
template <bool AFF, int S, int ABL = 0, int AUX = 0>  // ABL (study build, timing only): 1 no stores, 4 no softmax math
__device__ __forceinline__ void softmax_chunk(f32x4 (&C)[4][2], float (&mx)[2], float (&sm)[2], const float* rmul,
                                              __amdgpu_buffer_rsrc_t yrs, int ycs, int valid, int lane,
                                              float* slab = nullptr) {
  const int col = lane & 15, q = lane >> 4;
  if constexpr ((ABL & 4) && S < 8) {
    return;
  } else if constexpr (S == 0 || S == 1) {
    constexpr int fp = S;
    float m = -INFINITY;
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) {
      if constexpr (AFF) {
        const float4 m4 = *reinterpret_cast<const float4*>(rmul + fc * 16 + 4 * q);
        const float4 a4 = *reinterpret_cast<const float4*>(rmul + 64 + fc * 16 + 4 * q);
        const float mul[4] = {m4.x, m4.y, m4.z, m4.w}, add[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) C[fc][fp][jj] = fmaf(C[fc][fp][jj], mul[jj], add[jj]);
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) m = fmaxf(m, C[fc][fp][jj]);
    }
    mx[fp] = m;
  } else if constexpr (S == 2) {
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) mx[fp] = max_xor32(max_xor16(mx[fp]));
  } else if constexpr (S >= 3 && S <= 6) {
    constexpr int fp = (S - 3) / 2, h = (S - 3) % 2;
    float t = h ? sm[fp] : 0.f;
#pragma unroll
    for (int fc = 2 * h; fc < 2 * h + 2; ++fc)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        C[fc][fp][jj] = __expf(C[fc][fp][jj] - mx[fp]);
        t += C[fc][fp][jj];
      }
    sm[fp] = t;
  } else if constexpr (S == 7) {
#pragma unroll
    for (int fp = 0; fp < 2; ++fp) sm[fp] = 1.f / add_xor32(add_xor16(sm[fp]));
  } else if constexpr ((S == 8 || S == 9) && (AUX & 16)) {
    constexpr int fp = S - 8, SRF = 68;
    const float inv = sm[fp];
#pragma unroll
    for (int fc = 0; fc < 4; ++fc)
      *reinterpret_cast<f32x4*>(slab + col * SRF + fc * 16 + 4 * q) =
          f32x4{C[fc][fp][0] * inv, C[fc][fp][1] * inv, C[fc][fp][2] * inv, C[fc][fp][3] * inv};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 4; ++it) {  // lane l: pixel 4 it + l / 16, channels 4 (l % 16) .. +3
      const int px = 4 * it + (lane >> 4), ch = 4 * (lane & 15);
      const f32x4 o = *reinterpret_cast<const f32x4*>(slab + px * SRF + ch);
      const int pc = fp * 16 + px;
      if constexpr (ABL & 1) {
        asm volatile("" ::"v"(o[0]), "v"(o[3]));
        continue;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, o), yrs,
                                             pc < valid ? (pc * ycs + ch) * 4 : OOB, 0, AUX & 15);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the slab's reads retire before fragment 1 rewrites it
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else if constexpr (S == 8 || S == 9) {
    constexpr int fp = S - 8;
    const float inv = sm[fp];
    const int pc = fp * 16 + col;
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) {
      const f32x4 o = f32x4{C[fc][fp][0] * inv, C[fc][fp][1] * inv, C[fc][fp][2] * inv, C[fc][fp][3] * inv};
      if constexpr (ABL & 1) {
        asm volatile("" ::"v"(o[0]), "v"(o[3]));
        continue;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, o), yrs,
                                             pc < valid ? (pc * ycs + fc * 16 + 4 * q) * 4 : OOB, 0, AUX);
    }
  }
}

// X6 (CIN <= 5): the same conv at f32 accuracy on the bf16 MFMA (v_mfma_f32_16x16x32_bf16, 16x the f32 rate).  Each
// f32 input x and filter tap w is split exactly into three bf16 parts (h + m + l, as split6_kernel in elementwise.hip),
// and one 32-deep K step per tap carries the six products l*Wh + m*Wm + h*Wl + m*Wh + h*Wm + h*Wh of every channel
// (the parts' 24 significant bits; the dropped m*Wl, l*Wm, l*Wl terms are below 2^-24 of h*Wh): the per-wave patch
// holds a 64-byte record [l, m, h, m, h, h] (CIN channels each, zero padded) per pixel in 4 chunk planes, the weight
// table the matching [Wh, Wm, Wl, Wh, Wm, Wh] fragments.  9 steps of 8 bf16 MFMAs replace 12 of 8 f32 ones at a
// quarter of the cycles each, which leaves the kernel bound by its softmax and its 256-byte-per-pixel output stores.
// Single-buffered patch (the LDS budget: 36 KB of weight fragments + 8 x 6.5 KB of records + the store slabs; a wave's
// LDS reads and writes stay in program order, so restaging over the previous strip's records is safe).
__device__ __forceinline__ void split3_bf16(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = f2bf(x);
  const float r1 = x - bf2f((uint16_t)h);
  m = f2bf(r1);
  l = f2bf(r1 - bf2f((uint16_t)m));
}

template <int CIN, int MINW = 2, bool AFF = false, int ABL = 0, int AUX = 0, bool X6 = false>  // MINW: min waves per
                                                                      // SIMD; AFF: a scale / shift epilogue; AUX: stores
__global__ __launch_bounds__(512, MINW) void conv3x3_first_softmax_f32p(ConvArgs a) {  // epilogue; ABL: study only
  static_assert(!X6 || CIN * 6 <= 32, "x6: six parts of every channel in one 32-deep K step");
  constexpr int NS = X6 ? 9 : (9 * CIN + 3) / 4;
  constexpr int TH = 8, TW = 32, PW = TW + 2, SP = 3 * PW;
  constexpr int WPF = X6 ? 4 * SP * 4 : (CIN * SP + 32 + 3) / 4 * 4;  // per-wave patch floats (x6: 4 chunk planes)
  constexpr int NBUF = X6 ? 1 : 2;
  constexpr int ZERO = CIN * SP;
  __shared__ __attribute__((aligned(16))) f32x4 wl[X6 ? 1 : NS * 64];
  __shared__ __attribute__((aligned(16))) uint4 wx[X6 ? 9 * 4 * 64 : 1];  // x6: [tap][fc][lane] A fragments
  __shared__ int pl[X6 ? 1 : NS * 4];
  __shared__ __attribute__((aligned(16))) float rmul[2 * 64];
  __shared__ __attribute__((aligned(16))) float pat[8 * NBUF * WPF];
  __shared__ __attribute__((aligned(16))) float stg[(AUX & 16) ? 8 * 16 * 68 : 4];  // AUX & 16: the store slabs
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* const slab = stg + ((AUX & 16) ? wave * 16 * 68 : 0);
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  const int ntiles = a.tiles_total;
  const int G = (int)gridDim.x;
  auto tile_of = [&](int i) {
    const int base = (i / a.tiles_n) * a.tiles_n;
    return base + a.tiles_n <= ntiles ? base + xcd_tile(i - base, a.tiles_n) : i;
  };
  // strip i of this wave: frame n, row r, first column c0 (i past the end: a zero strip below every frame)
  auto strip = [&](int i, int& n, int& r, int& c0) __attribute__((always_inline)) {
    const bool real = i < ntiles;
    const int t = tile_of(real ? i : 0);
    n = t / (th * tw);
    const int srem = t - n * th * tw;
    r = real ? (srem / tw) * TH + wave : H;
    c0 = (srem - (srem / tw) * tw) * TW;
  };
  // strip coordinates are decoded outside the interleaved region (the decode's integer divisions expand with
  // branches, which would split the basic block the schedule below needs)
  struct SC {
    int n, r, c0;
  };
  auto coords = [&](int i) __attribute__((always_inline)) {
    SC c;
    strip(i, c.n, c.r, c.c0);
    return c;
  };
  auto load_strip = [&](const SC& sc, float4 (&v)[2][2]) __attribute__((always_inline)) {
    const int n = sc.n, r = sc.r, c0 = sc.c0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const int pr = e / PW, pc = e - pr * PW;
      const int h = r - 1 + pr, w = c0 - 1 + pc;
      const bool ok = e < SP && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      const float* xp = reinterpret_cast<const float*>(a.x) + a.x_coff + ((long)n * H + (ok ? h : 0)) * (long)W * cs +
                        (long)(ok ? w : 0) * cs;
      v[k][0] = ok ? *reinterpret_cast<const float4*>(xp) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[k][1] = ok && CIN > 4 ? *reinterpret_cast<const float4*>(xp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  const int col = lane & 15, q = lane >> 4;
  const float* Wt = reinterpret_cast<const float*>(a.w);
  if constexpr (X6) {
    // k slot kk of a tap: part group g = kk / CIN (record [l, m, h, m, h, h] against filter parts [h, m, l, h, m, h]),
    // channel kk % CIN; slots past 6 * CIN are zero
    for (int e = tid; e < 9 * 4 * 64; e += 512) {
      const int tap = e >> 8, fc = (e >> 6) & 3, l = e & 63;
      const int co = fc * 16 + (l & 15);
      uint32_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = 8 * (l >> 4) + j, g = kk / CIN, c = kk - g * CIN;
        uint32_t h = 0, m = 0, lo = 0;
        if (kk < 6 * CIN) split3_bf16(Wt[(long)co * a.K_pad + tap * 8 + c], h, m, lo);
        v[j] = g == 0 || g == 3 || g == 5 ? h : g == 1 || g == 4 ? m : g == 2 ? lo : 0u;
      }
      wx[e] = make_uint4(v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16, v[6] | v[7] << 16);
    }
  } else {
    for (int e = tid; e < NS * 64; e += 512) {
      const int st = e >> 6, l = e & 63;
      const int kk = 4 * st + (l >> 4), co = l & 15;
      const int tap = kk / CIN, c = kk - tap * CIN;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kk < 9 * CIN)
#pragma unroll
        for (int fc = 0; fc < 4; ++fc) v[fc] = Wt[(long)(fc * 16 + co) * a.K_pad + tap * 8 + c];
      wl[e] = v;
    }
    if (tid < NS * 4) {
      const int kk = tid;
      const int tap = kk / CIN, c = kk - tap * CIN;
      pl[tid] = kk < 9 * CIN ? c * SP + (tap / 3) * PW + tap % 3 : ZERO;
    }
  }
  float* P0 = pat + wave * NBUF * WPF;
  float* P1 = P0 + (NBUF - 1) * WPF;
  if (!X6 && lane < 32) {
    P0[ZERO + lane] = 0.f;
    P1[ZERO + lane] = 0.f;
  }
  if (tid < 64) {
    const float sc = a.scale ? a.scale[tid] : 1.f;
    rmul[tid] = sc;
    rmul[64 + tid] = (a.bias ? a.bias[tid] : 0.f) * sc + (a.shift ? a.shift[tid] : 0.f);
  }
  constexpr bool aff = AFF;
  __syncthreads();  // the only block-wide barrier: the staged tables
  auto stage = [&](float* P, const float4 (&v)[2][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const float vv[8] = {v[k][0].x, v[k][0].y, v[k][0].z, v[k][0].w, v[k][1].x, v[k][1].y, v[k][1].z, v[k][1].w};
      if constexpr (X6) {  // the pixel's 32-slot record [l, m, h, m, h, h] as 4 chunk planes of SP x 16 bytes
        uint32_t h[CIN], m[CIN], lo[CIN], r[32];
#pragma unroll
        for (int c = 0; c < CIN; ++c) split3_bf16(vv[c], h[c], m[c], lo[c]);
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) {
          const int g = kk / CIN, c = kk % CIN;
          r[kk] = kk >= 6 * CIN ? 0u : g == 0 ? lo[c] : (g == 1 || g == 3) ? m[c] : h[c];
        }
        if (e < SP)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            reinterpret_cast<uint4*>(P)[j * SP + e] =
                make_uint4(r[8 * j] | r[8 * j + 1] << 16, r[8 * j + 2] | r[8 * j + 3] << 16,
                           r[8 * j + 4] | r[8 * j + 5] << 16, r[8 * j + 6] | r[8 * j + 7] << 16);
      } else if (e < SP) {
#pragma unroll
        for (int c = 0; c < CIN; ++c) P[c * SP + e] = vv[c];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // the MFMAs of strip P into N; with C, the 10 softmax chunks of the previous strip, one per K step: each step is its
  // own scheduling region (sched_barrier), so the chunk's VALU work issues between that step's MFMAs, and the next
  // step's fragments are read under them
  // this lane's patch offsets of every K step (the pl table's entry for its k-slot q, plus its pixel column), held
  // in registers: read from LDS inside the step they made each step's fragment reads wait on a dependent LDS load
  int poff[X6 ? 1 : NS];
  if constexpr (!X6) {
#pragma unroll
    for (int s = 0; s < NS; ++s) poff[s] = pl[s * 4 + q] + col;
  }
  // x6: step s = tap s; A = the 4 cout fragments of the tap, B = chunk q of the records of pixels col, col + 16
  auto mma_x6 = [&](const float* P, f32x4 (&N)[4][2], f32x4* Cp, const __amdgpu_buffer_rsrc_t& yrs, int valid)
      __attribute__((always_inline)) {
    init_strip_acc(N, rmul, aff, q);
    float mx[2] = {0.f, 0.f}, sm[2] = {0.f, 0.f};
    const uint4* R = reinterpret_cast<const uint4*>(P) + q * SP + col;
    uint4 av[4], bv[2];
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) av[fc] = wx[fc * 64 + lane];
    bv[0] = R[0];
    bv[1] = R[16];
    static_for<0, 9>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value;
      uint4 an[4], bn[2];
      if constexpr (s + 1 < 9) {
        constexpr int toff = ((s + 1) / 3) * PW + (s + 1) % 3;
#pragma unroll
        for (int fc = 0; fc < 4; ++fc) an[fc] = wx[((s + 1) * 4 + fc) * 64 + lane];
        bn[0] = R[toff];
        bn[1] = R[toff + 16];
      }
      if constexpr (!(ABL & 2)) {
#pragma unroll
        for (int fc = 0; fc < 4; ++fc) {
          mma16<uint16_t>(av[fc], bv[0], N[fc][0]);
          mma16<uint16_t>(av[fc], bv[1], N[fc][1]);
        }
      }
      if (Cp) {
        softmax_chunk<AFF, s, ABL, AUX>(*reinterpret_cast<f32x4(*)[4][2]>(Cp), mx, sm, rmul, yrs, a.y_cstride, valid,
                                        lane, slab);
      }
      if constexpr (s + 1 < 9) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (s + 1 < 9) {
#pragma unroll
        for (int fc = 0; fc < 4; ++fc) av[fc] = an[fc];
        bv[0] = bn[0];
        bv[1] = bn[1];
      }
    });
    if (Cp) {  // the 10th chunk
      softmax_chunk<AFF, 9, ABL, AUX>(*reinterpret_cast<f32x4(*)[4][2]>(Cp), mx, sm, rmul, yrs, a.y_cstride, valid,
                                      lane, slab);
    }
  };
  auto mma = [&](const float* P, f32x4 (&N)[4][2], f32x4* Cp, const __amdgpu_buffer_rsrc_t& yrs, int valid)
      __attribute__((always_inline)) {
    if constexpr (X6) {
      mma_x6(P, N, Cp, yrs, valid);
    } else {
      init_strip_acc(N, rmul, aff, q);
      float mx[2] = {0.f, 0.f}, sm[2] = {0.f, 0.f};
      f32x4 w4 = wl[lane];
      float b0 = P[poff[0]], b1 = P[poff[0] + 16];
      static_for<0, NS>([&](auto sc) __attribute__((always_inline)) {
        constexpr int s = decltype(sc)::value;
        f32x4 w4n = w4;
        float b0n = b0, b1n = b1;
        if constexpr (s + 1 < NS) {
          w4n = wl[(s + 1) * 64 + lane];
          b0n = P[poff[s + 1]];
          b1n = P[poff[s + 1] + 16];
        }
        if constexpr (ABL & 2) {
          asm volatile("" ::"v"(w4[0]), "v"(w4[3]), "v"(b0), "v"(b1));
        } else {
  #pragma unroll
          for (int fc = 0; fc < 4; ++fc) {
            N[fc][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[fc], b0, N[fc][0], 0, 0, 0);
            N[fc][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[fc], b1, N[fc][1], 0, 0, 0);
          }
        }
        if (Cp) {
          if constexpr (s < 10)
            softmax_chunk<AFF, s, ABL, AUX>(*reinterpret_cast<f32x4(*)[4][2]>(Cp), mx, sm, rmul, yrs, a.y_cstride, valid,
                                            lane, slab);
        }
        // the next step's fragment reads first (else hipcc sinks them to the step's end and the next step's first
        // MFMA waits a whole LDS latency), then one MFMA per 3 VALU of the softmax chunk
        if constexpr (s + 1 < NS) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        if constexpr (s + 1 >= NS) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        w4 = w4n;
        b0 = b0n;
        b1 = b1n;
      });
      if (Cp) {  // a short K loop (CIN < 4): the chunks left over
        static_for<NS, 10>([&](auto sc) __attribute__((always_inline)) {
          softmax_chunk<AFF, decltype(sc)::value, ABL, AUX>(*reinterpret_cast<f32x4(*)[4][2]>(Cp), mx, sm, rmul, yrs,
                                                             a.y_cstride, valid, lane, slab);
        });
      }
    }
  };
  auto yrs_of = [&](const SC& sc, int& valid) __attribute__((always_inline)) {
    float* yb = reinterpret_cast<float*>(a.y) + a.y_coff +
                (((long)sc.n * H + (sc.r < H ? sc.r : 0)) * W + sc.c0) * (long)a.y_cstride;
    valid = sc.r < H ? W - sc.c0 : 0;
    return __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(yb), 0, 0x7ffffff0, 0x00020000);
  };
  // the last strip's softmax alone (no MFMAs left to hide it under)
  auto store = [&](const SC& sc, f32x4 (&C)[4][2]) __attribute__((always_inline)) {
    int valid;
    const __amdgpu_buffer_rsrc_t yrs = yrs_of(sc, valid);
    float mx[2] = {0.f, 0.f}, sm[2] = {0.f, 0.f};
    static_for<0, 10>([&](auto sc2) __attribute__((always_inline)) {
      softmax_chunk<AFF, decltype(sc2)::value, ABL, AUX>(C, mx, sm, rmul, yrs, a.y_cstride, valid, lane, slab);
    });
  };
  int cur = blockIdx.x;
  if (cur >= ntiles) return;
  float4 nv[2][2];
  SC s0 = coords(cur), s1 = coords(cur + G), s2;  // strips cur (accumulators C), cur + G (patch in flight)
  load_strip(s0, nv);
  stage(P0, nv);
  load_strip(s1, nv);
  f32x4 acc0[4][2], acc1[4][2];
  {
    int v0;
    mma(P0, acc0, nullptr, yrs_of(s0, v0), 0);
  }
  // one step: strip cur's accumulators are in C; stage strip cur+G into buffer B and compute it into N while C's
  // softmax and stores go out between its MFMAs
  auto step = [&](auto bconst, f32x4 (&C)[4][2], f32x4 (&N)[4][2]) __attribute__((always_inline)) {
    constexpr int b = decltype(bconst)::value;
    float* Pn = b ? P1 : P0;
    stage(Pn, nv);
    s2 = coords(cur + 2 * G);
    int valid;
    const __amdgpu_buffer_rsrc_t yrs = yrs_of(s0, valid);
    load_strip(s2, nv);
    mma(Pn, N, &C[0][0], yrs, valid);
    s0 = s1;
    s1 = s2;
    cur += G;
  };
  while (true) {
    if (cur + G >= ntiles) {
      store(s0, acc0);
      break;
    }
    step(std::integral_constant<int, 1>{}, acc0, acc1);
    if (cur + G >= ntiles) {
      store(s0, acc1);
      break;
    }
    step(std::integral_constant<int, 0>{}, acc1, acc0);
  }
}

// Row-ring form of conv3x3_first_softmax_f32p (r04): a wave walks a column band of 32 pixels down a segment of
// a.seg rows instead of taking one row of an 8-row tile, so each strip stages ONE new input row (its window's bottom
// row) instead of three: the per-wave patch is a ring of 4 row slots, and the rows in slots 0 and 1 are written
// twice (slots 4 and 5 too), so the 3-row window of every strip is contiguous at slot base (strip - first) % 4 and
// the per-step patch offsets stay fixed registers (the window base moves the pointer, not the offsets).  Staging
// alone was 0.048 of the pipelined kernel's 0.167 ms (smxabl abl 7): 3 input rows read per output row.  The MFMA
// order, softmax chunks and stores are the pipelined kernel's, so results are bit-identical to it.
template <int CIN, int AUX = 18>
__global__ __launch_bounds__(512, 2) void conv3x3_first_softmax_f32r(ConvArgs a) {
  constexpr int NS = (9 * CIN + 3) / 4;
  constexpr int TW = 32, PW = TW + 2, SP = 6 * PW;  // 6 row slots: ring of 4 + copies of slots 0 and 1
  constexpr int ZERO = CIN * SP;                     // 32 + 3 * PW zeros: the padded k-slots read at any base
  constexpr int WPF = (ZERO + 32 + 3 * PW + 3) / 4 * 4;
  constexpr bool AFF = false;
  __shared__ __attribute__((aligned(16))) f32x4 wl[NS * 64];
  __shared__ int pl[NS * 4];
  __shared__ __attribute__((aligned(16))) float rmul[2 * 64];
  __shared__ __attribute__((aligned(16))) float pat[8 * WPF];
  __shared__ __attribute__((aligned(16))) float stg[(AUX & 16) ? 8 * 16 * 68 : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* const slab = stg + ((AUX & 16) ? wave * 16 * 68 : 0);
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int tw = (W + TW - 1) / TW, RS = a.seg, nseg = (H + RS - 1) / RS;
  const int nitems = a.tiles_total;  // frames x segments x bands
  const int gw = blockIdx.x * 8 + wave, GW = (int)gridDim.x * 8;
  // strip = (item, row); the walk: rows r0 .. rend-1 of item gw, then of gw + GW, ...
  struct SC {
    int n, r, c0, rend, item;
  };
  auto item_start = [&](int item) __attribute__((always_inline)) {
    SC c;
    c.item = item;
    if (item >= nitems) {
      c.n = 0; c.r = H; c.c0 = 0; c.rend = H;
      return c;
    }
    const int band = item % tw, t = item / tw;
    const int seg = t % nseg;
    c.n = t / nseg;
    c.c0 = band * TW;
    c.r = seg * RS;
    c.rend = min(H, c.r + RS);
    return c;
  };
  auto next_strip = [&](const SC& c) __attribute__((always_inline)) {
    if (c.item < nitems && c.r + 1 < c.rend) {
      SC d = c;
      d.r += 1;
      return d;
    }
    return item_start(c.item + GW);
  };
  const int col = lane & 15, q = lane >> 4;
  const float* Wt = reinterpret_cast<const float*>(a.w);
  for (int e = tid; e < NS * 64; e += 512) {
    const int st = e >> 6, l = e & 63;
    const int kk = 4 * st + (l >> 4), co = l & 15;
    const int tap = kk / CIN, c = kk - tap * CIN;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kk < 9 * CIN)
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) v[fc] = Wt[(long)(fc * 16 + co) * a.K_pad + tap * 8 + c];
    wl[e] = v;
  }
  if (tid < NS * 4) {
    const int kk = tid;
    const int tap = kk / CIN, c = kk - tap * CIN;
    pl[tid] = kk < 9 * CIN ? c * SP + (tap / 3) * PW + tap % 3 : ZERO;
  }
  float* const P = pat + wave * WPF;
  for (int e = lane; e < 32 + 3 * PW; e += 64) P[ZERO + e] = 0.f;
  if (tid < 64) {
    rmul[tid] = 1.f;
    rmul[64 + tid] = a.bias ? a.bias[tid] : 0.f;
  }
  __syncthreads();  // the only block-wide barrier: the staged tables
  int poff[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) poff[s] = pl[s * 4 + q] + col;
  // input rows of a strip: its whole 3-row window when it starts an item (first), else the window's bottom row
  auto load_rows = [&](const SC& sc, bool first, float4 (&v)[2][2]) __attribute__((always_inline)) {
    const int n = sc.n, c0 = sc.c0;
    const int rlo = first ? sc.r - 1 : sc.r + 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const int pr = e / PW, pc = e - pr * PW;
      const int h = rlo + pr, w = c0 - 1 + pc;
      const bool ok = e < (first ? 3 * PW : PW) && sc.r < H && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      const float* xp = reinterpret_cast<const float*>(a.x) + a.x_coff + ((long)n * H + (ok ? h : 0)) * (long)W * cs +
                        (long)(ok ? w : 0) * cs;
      v[k][0] = ok ? *reinterpret_cast<const float4*>(xp) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[k][1] = ok && CIN > 4 ? *reinterpret_cast<const float4*>(xp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  // ring slot of the window's first row for strip row r of an item starting at r0
  auto base_of = [&](const SC& sc) __attribute__((always_inline)) {
    return (sc.r - (sc.r / RS) * RS) & 3;
  };
  auto stage = [&](const SC& sc, bool first, const float4 (&v)[2][2]) __attribute__((always_inline)) {
    const int j = base_of(sc);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * k;
      const float vv[8] = {v[k][0].x, v[k][0].y, v[k][0].z, v[k][0].w, v[k][1].x, v[k][1].y, v[k][1].z, v[k][1].w};
      const int pr = e / PW, pc = e - pr * PW;
      const int slot = first ? pr : (j + 2) & 3;  // first: window base 0
      if (e < (first ? 3 * PW : PW)) {
#pragma unroll
        for (int c = 0; c < CIN; ++c) {
          P[c * SP + slot * PW + pc] = vv[c];
          if (slot < 2) P[c * SP + (slot + 4) * PW + pc] = vv[c];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto mma = [&](const float* Pw, f32x4 (&N)[4][2], f32x4* Cp, const __amdgpu_buffer_rsrc_t& yrs, int valid)
      __attribute__((always_inline)) {
    init_strip_acc(N, rmul, false, q);
    float mx[2] = {0.f, 0.f}, sm[2] = {0.f, 0.f};
    f32x4 w4 = wl[lane];
    float b0 = Pw[poff[0]], b1 = Pw[poff[0] + 16];
    static_for<0, NS>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value;
      f32x4 w4n = w4;
      float b0n = b0, b1n = b1;
      if constexpr (s + 1 < NS) {
        w4n = wl[(s + 1) * 64 + lane];
        b0n = Pw[poff[s + 1]];
        b1n = Pw[poff[s + 1] + 16];
      }
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        N[fc][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[fc], b0, N[fc][0], 0, 0, 0);
        N[fc][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[fc], b1, N[fc][1], 0, 0, 0);
      }
      if (Cp) {
        if constexpr (s < 10)
          softmax_chunk<AFF, s, 0, AUX>(*reinterpret_cast<f32x4(*)[4][2]>(Cp), mx, sm, rmul, yrs, a.y_cstride, valid,
                                        lane, slab);
      }
      if constexpr (s + 1 < NS) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      if constexpr (s + 1 >= NS) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      w4 = w4n;
      b0 = b0n;
      b1 = b1n;
    });
    if (Cp) {
      static_for<NS, 10>([&](auto sc) __attribute__((always_inline)) {
        softmax_chunk<AFF, decltype(sc)::value, 0, AUX>(*reinterpret_cast<f32x4(*)[4][2]>(Cp), mx, sm, rmul, yrs,
                                                         a.y_cstride, valid, lane, slab);
      });
    }
  };
  auto yrs_of = [&](const SC& sc, int& valid) __attribute__((always_inline)) {
    float* yb = reinterpret_cast<float*>(a.y) + a.y_coff +
                (((long)sc.n * H + (sc.r < H ? sc.r : 0)) * W + sc.c0) * (long)a.y_cstride;
    valid = sc.r < H ? W - sc.c0 : 0;
    return __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(yb), 0, 0x7ffffff0, 0x00020000);
  };
  auto store = [&](const SC& sc, f32x4 (&C)[4][2]) __attribute__((always_inline)) {
    int valid;
    const __amdgpu_buffer_rsrc_t yrs = yrs_of(sc, valid);
    float mx[2] = {0.f, 0.f}, sm[2] = {0.f, 0.f};
    static_for<0, 10>([&](auto sc2) __attribute__((always_inline)) {
      softmax_chunk<AFF, decltype(sc2)::value, 0, AUX>(C, mx, sm, rmul, yrs, a.y_cstride, valid, lane, slab);
    });
  };
  SC s0 = item_start(gw);
  if (s0.item >= nitems) return;  // (wave-uniform; the block barrier above is behind every wave)
  float4 nv[2][2];
  load_rows(s0, true, nv);
  stage(s0, true, nv);
  SC s1 = next_strip(s0);
  bool f1 = s1.item != s0.item;
  load_rows(s1, f1, nv);
  f32x4 acc0[4][2], acc1[4][2];
  {
    int v0;
    mma(P + base_of(s0) * PW, acc0, nullptr, yrs_of(s0, v0), 0);
  }
  // one step: strip s0's accumulators are in C; stage strip s1 and compute it into N while C's softmax and stores go
  // out between its MFMAs
  auto step = [&](f32x4 (&C)[4][2], f32x4 (&N)[4][2]) __attribute__((always_inline)) {
    stage(s1, f1, nv);
    const SC s2 = next_strip(s1);
    const bool f2 = s2.item != s1.item;
    int valid;
    const __amdgpu_buffer_rsrc_t yrs = yrs_of(s0, valid);
    load_rows(s2, f2, nv);
    mma(P + base_of(s1) * PW, N, &C[0][0], yrs, valid);
    s0 = s1;
    s1 = s2;
    f1 = f2;
  };
  while (true) {
    if (s1.item >= nitems) {
      store(s0, acc0);
      break;
    }
    step(acc0, acc1);
    if (s1.item >= nitems) {
      store(s0, acc1);
      break;
    }
    step(acc1, acc0);
  }
}

// ================================================================ launchers (called from conv3x3.hip's dispatch_mfma)
int launch_first(ConvArgs& a, hipStream_t st) {
  const long N = a.M / ((long)a.H * a.W);
  const long sp = N * ((a.H + 7) / 8) * ((a.W + 31) / 32);
  a.tiles_n = (a.cout + 63) / 64;
  if (sp * a.tiles_n > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3: too many tiles");
  a.tiles_total = (int)(sp * a.tiles_n);
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first");
  static int attr_dev = -1, resident = 0;  // blocks resident on the whole chip (2 per CU at 98 VGPRs, 41 KB LDS)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (attr_dev != dev) {
    int per_cu = 0, n_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&conv3x3_first),
                                                                512, 0);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return fail(VM_EHIP, "conv3x3_first setup: %s", hipGetErrorString(e));
    resident = per_cu * n_cu / 8 * 8;
    attr_dev = dev;
  }
  // a multiple of 8 blocks (xcd_tile's XCD ranges stay per block), at most one resident round
  int grid = resident > 0 && resident < a.tiles_total ? resident : a.tiles_total;
  if (grid > 8) grid = grid / 8 * 8;
  hipLaunchKernelGGL(conv3x3_first, dim3(grid), dim3(512), 0, st, a);
  return check_launch("conv3x3_first");
}

int launch_first_softmax(ConvArgs& a, hipStream_t st) {
  const long N = a.M / ((long)a.H * a.W);
  const long sp = N * ((a.H + 7) / 8) * ((a.W + 31) / 32);
  if (sp > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3: too many tiles");
  a.tiles_total = (int)sp;
  // persistent grid of g_opt.softmax_blocks; tile_of() maps block-order indices in rounds of tiles_n = grid onto
  // contiguous per-XCD bands (xcd_tile within a round)
  const int grid = (int)std::min<long>(sp, g_opt.softmax_blocks);
  a.tiles_n = grid;
  if (g_opt.softmax_kernel == 3) {
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax<false, true>");
    hipLaunchKernelGGL((conv3x3_first_softmax<false, true>), dim3(grid), dim3(512), 0, st, a);
  } else if (g_opt.softmax_kernel == 4) {
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax<true, true>");
    hipLaunchKernelGGL((conv3x3_first_softmax<true, true>), dim3(grid), dim3(512), 0, st, a);
  } else if (g_opt.softmax_kernel == 6) {
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_strip");
    hipLaunchKernelGGL(conv3x3_first_softmax_strip, dim3(grid), dim3(512), 0, st, a);
  } else if (g_opt.softmax_kernel == 5) {
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax<true, true, true>");
    hipLaunchKernelGGL((conv3x3_first_softmax<true, true, true>), dim3(grid), dim3(512), 0, st, a);
  } else if (g_opt.softmax_kernel == 2) {
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax<true>");
    hipLaunchKernelGGL(conv3x3_first_softmax<true>, dim3(grid), dim3(512), 0, st, a);
  } else {
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax<false>");
    hipLaunchKernelGGL(conv3x3_first_softmax<false>, dim3(grid), dim3(512), 0, st, a);
  }
  return check_launch("conv3x3_first_softmax");
}

int launch_first_softmax_f32(ConvArgs& a, int cin, hipStream_t st) {
  const long N = a.M / ((long)a.H * a.W);
  const long sp = N * ((a.H + 7) / 8) * ((a.W + 31) / 32);
  if (sp > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3: too many tiles");
  a.tiles_total = (int)sp;
  const int grid = (int)std::min<long>(sp, g_opt.softmax_blocks);
  a.tiles_n = grid;
  if (g_opt.softmax_f32p && !a.scale && !a.shift) {  // (a scale / shift epilogue: the r03 kernel below)
    // one resident round (2 waves per SIMD: one 512-thread block per CU); softmax_blocks caps it for tests
    static int n_cu = 0;
    if (!n_cu) {
      int dev = 0;
      (void)hipGetDevice(&dev);
      if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
        return fail(VM_EHIP, "conv3x3_first_softmax_f32p: CU count query failed");
    }
    const int gp = (int)std::min<long>(std::min<long>(sp, n_cu), g_opt.softmax_blocks);
    a.tiles_n = gp;
#define VM_SMP(C)                                                                             \
  case C:                                                                                    \
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<%d, 2, false, 0, 18>", C); \
    hipLaunchKernelGGL((conv3x3_first_softmax_f32p<C, 2, false, 0, 18>), dim3(gp), dim3(512), 0, st, a);     \
    break;
    if (g_opt.softmax_f32p == 6) {  // the row-ring form: segments of a.seg rows x 32-pixel bands, one per wave
      const long nimg = N, bands = (a.W + 31) / 32;
      const long waves = (long)gp * 8;
      long seg = (nimg * bands * a.H + waves - 1) / waves;  // rows per segment for about one item per wave
      if (seg < 4) seg = 4;
      const long items = nimg * bands * ((a.H + seg - 1) / seg);
      if (items > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3_first_softmax_f32r: too many items");
      a.seg = (int)seg;
      a.tiles_total = (int)items;
      switch (cin) {
#define VM_SMR(C)                                                                                              \
  case C:                                                                                                      \
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32r<%d>", C);                   \
    hipLaunchKernelGGL((conv3x3_first_softmax_f32r<C>), dim3((unsigned)std::min<long>(gp, (items + 7) / 8)),  \
                       dim3(512), 0, st, a);                                                                   \
    break;
        VM_SMR(1) VM_SMR(2) VM_SMR(3) VM_SMR(4) VM_SMR(5) VM_SMR(6) VM_SMR(7) VM_SMR(8)
#undef VM_SMR
        default: return fail(VM_EINVAL, "conv3x3_first_softmax_f32r: cin %d", cin);
      }
      return check_launch("conv3x3_first_softmax_f32r");
    }
#ifdef VM_STUDY
    if (cin == 5 && g_opt.softmax_abl) {  // timing ablations (garbage results): 1 no stores, 2 no MFMA, 4 no softmax
      snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<5, 2, false, %ld, 18>", g_opt.softmax_abl);
      switch (g_opt.softmax_abl) {
        case 1: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 1, 18>), dim3(gp), dim3(512), 0, st, a); break;
        case 2: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 2, 18>), dim3(gp), dim3(512), 0, st, a); break;
        case 3: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 3, 18>), dim3(gp), dim3(512), 0, st, a); break;
        case 4: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 4, 18>), dim3(gp), dim3(512), 0, st, a); break;
        case 5: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 5, 18>), dim3(gp), dim3(512), 0, st, a); break;
        case 6: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 6, 18>), dim3(gp), dim3(512), 0, st, a); break;
        default: hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 7, 18>), dim3(gp), dim3(512), 0, st, a); break;
      }
      return check_launch("conv3x3_first_softmax_f32p");
    }
#endif
    if (cin <= 5 && g_opt.softmax_f32p == 7) {  // split-bf16 x6 on the bf16 MFMA (f32 accuracy; X6 above)
      switch (cin) {
#define VM_SMX(C)                                                                                        \
  case C:                                                                                                \
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<%d, 2, false, 0, 18, true>", C); \
    hipLaunchKernelGGL((conv3x3_first_softmax_f32p<C, 2, false, 0, 18, true>), dim3(gp), dim3(512), 0, st, a);     \
    break;
        VM_SMX(1) VM_SMX(2) VM_SMX(3) VM_SMX(4) VM_SMX(5)
#undef VM_SMX
        default: break;
      }
      return check_launch("conv3x3_first_softmax_f32p");
    }
    if (cin == 5 && g_opt.softmax_f32p == 2) {
      snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<5, 4>");
      hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 4>), dim3(gp), dim3(512), 0, st, a);
      return check_launch("conv3x3_first_softmax_f32p");
    }
    if (cin == 5 && g_opt.softmax_f32p >= 4) {  // LDS-transposed whole-pixel stores: 4 non-temporal, 5 through L2
      if (g_opt.softmax_f32p == 4) {
        snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<5, 2, false, 0, 18>");
        hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 0, 18>), dim3(gp), dim3(512), 0, st, a);
      } else {
        snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<5, 2, false, 0, 16>");
        hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 0, 16>), dim3(gp), dim3(512), 0, st, a);
      }
      return check_launch("conv3x3_first_softmax_f32p");
    }
    if (cin == 5 && g_opt.softmax_f32p == 1) {  // stores straight from the accumulator lanes through L2 (A/B)
      snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<5>");
      hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5>), dim3(gp), dim3(512), 0, st, a);
      return check_launch("conv3x3_first_softmax_f32p");
    }
    if (cin == 5 && g_opt.softmax_f32p == 3) {  // non-temporal stores (A/B)
      snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32p<5, 2, false, 0, 2>");
      hipLaunchKernelGGL((conv3x3_first_softmax_f32p<5, 2, false, 0, 2>), dim3(gp), dim3(512), 0, st, a);
      return check_launch("conv3x3_first_softmax_f32p");
    }
    switch (cin) {
      VM_SMP(1) VM_SMP(2) VM_SMP(3) VM_SMP(4) VM_SMP(5) VM_SMP(6) VM_SMP(7) VM_SMP(8)
      default: return fail(VM_EINVAL, "conv3x3_first_softmax_f32p: cin %d", cin);
    }
#undef VM_SMP
    return check_launch("conv3x3_first_softmax_f32p");
  }
#define VM_SMF(C)                                                                            \
  case C:                                                                                   \
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32<%d>", C); \
    hipLaunchKernelGGL(conv3x3_first_softmax_f32<C>, dim3(grid), dim3(512), 0, st, a);      \
    break;
#ifdef VM_STUDY
  if (cin == 5 && g_opt.softmax_abl) {  // timing ablations of the f32 refine kernel (results are garbage)
    snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_first_softmax_f32<5, %ld>", g_opt.softmax_abl);
    if (g_opt.softmax_abl == 1) hipLaunchKernelGGL((conv3x3_first_softmax_f32<5, 1>), dim3(grid), dim3(512), 0, st, a);
    else if (g_opt.softmax_abl == 2) hipLaunchKernelGGL((conv3x3_first_softmax_f32<5, 2>), dim3(grid), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((conv3x3_first_softmax_f32<5, 3>), dim3(grid), dim3(512), 0, st, a);
    return check_launch("conv3x3_first_softmax_f32");
  }
#endif
  switch (cin) {
    VM_SMF(1) VM_SMF(2) VM_SMF(3) VM_SMF(4) VM_SMF(5) VM_SMF(6) VM_SMF(7) VM_SMF(8)
    default: return fail(VM_EINVAL, "conv3x3_first_softmax_f32: cin %d", cin);
  }
#undef VM_SMF
  return check_launch("conv3x3_first_softmax_f32");
}

}  // namespace vm
