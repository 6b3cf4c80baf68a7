// Weight packing of the 3x3 convs: HWIO f32 filters -> the K-granule layout of conv3x3.hip's header comment, one
// filter (vm_conv3x3_pack_weights) or a batch of forward and flipped packs (vm_conv3x3_pack_weights_batch).
#include "conv_dispatch.h"

namespace vm {

// ================================================================ weight packing
// HWIO f32 [3][3][cin][cout] (unet.py:15 / the VGG npy layout) -> [cout_pad][K_pad] in the compute dtype,
// K in granule order (see the header comment).
template <typename T>
__global__ void pack_weights(const float* w, int cin, int cout, ConvArgs g) {
  constexpr int GE = 64 / sizeof(T);
  T* out = reinterpret_cast<T*>(const_cast<void*>(g.w));
  const long total = (long)g.cout_pad * g.K_pad;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i / g.K_pad);
    const int k = (int)(i - (long)co * g.K_pad);
    int tap, c;
    k_to_tap<GE>(g, k, tap, c);
    float v = 0.f;
    if (co < cout && tap < 9 && c < cin) v = w[((long)tap * cin + c) * cout + co];
    st_elem<T>(out + i, v);
  }
}

constexpr int PACK_MAX_JOBS = 48;
struct PackBatch {
  int n;
  vm_pack_job j[PACK_MAX_JOBS];
  int K_pad[PACK_MAX_JOBS], cout_pad[PACK_MAX_JOBS], cin_pad[PACK_MAX_JOBS];
};

// job blockIdx.y: k_to_tap's decode of the conv geometry (as pack_weights), value from the (flipped) source filter
__global__ void pack_weights_batch(PackBatch b) {
  const vm_pack_job& j = b.j[blockIdx.y];
  const bool bf = j.dtype == VM_BF16;
  const int GE = bf ? 32 : 16;
  ConvArgs g{};
  g.cin_pad = b.cin_pad[blockIdx.y];
  g.K9 = 9 * g.cin_pad;
  g.chunk_major = g.cin_pad % GE == 0;
  g.ng = g.chunk_major ? g.K9 / GE : 0;
  const int K_pad = b.K_pad[blockIdx.y];
  const long total = (long)b.cout_pad[blockIdx.y] * K_pad;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i / K_pad);
    const int k = (int)(i - (long)co * K_pad);
    int tap, c;
    if (bf) k_to_tap<32>(g, k, tap, c);
    else k_to_tap<16>(g, k, tap, c);
    float v = 0.f;
    if (tap < 9 && co < j.cout && c < j.cin) {
      if (!j.flip) {
        if (co < j.w_cout && c < j.w_cin) v = j.w[((long)tap * j.w_cin + c) * j.w_cout + co];
      } else if (c < j.w_cout && co < j.w_cin) {
        v = j.w[((long)(8 - tap) * j.w_cin + co) * j.w_cout + c];
      }
    }
    if (bf) reinterpret_cast<uint16_t*>(j.packed)[i] = f2bf(v);
    else reinterpret_cast<float*>(j.packed)[i] = v;
  }
}

// the forward packs of chunk-major bf16 filters (every conv of the UNetImage / UNetVideo training re-pack): a block
// transposes one (granule, 64-output-channel) tile through LDS, so the source filter is read along cout (256-byte
// runs; pack_weights_batch's one element per thread read it with a w_cout stride) and each packed row receives 64
// contiguous bytes; zero padding (cin / cout past the filter, the K_pad tail granule) as pack_weights_batch, and the
// same RNE rounding: bit-identical
__global__ __launch_bounds__(256) void pack_weights_tiled(PackBatch b) {
  const int jb = blockIdx.y;
  const vm_pack_job& j = b.j[jb];
  const int K_pad = b.K_pad[jb], ngr = K_pad / 32, ng = 9 * b.cin_pad[jb] / 32, ncot = b.cout_pad[jb] / 64;
  const int t = blockIdx.x;
  if (t >= ngr * ncot) return;
  const int gr = t % ngr, co0 = (t / ngr) * 64;
  __shared__ float tile[32][65];
  const int tid = threadIdx.x;
  if (gr < ng) {
    const int cc = gr / 9, tap = gr - cc * 9;
    for (int e = tid; e < 32 * 64; e += 256) {
      const int ci = e >> 6, coj = e & 63;
      const int c = cc * 32 + ci, co = co0 + coj;
      float v = 0.f;
      if (co < j.cout && c < j.cin && co < j.w_cout && c < j.w_cin) v = j.w[((long)tap * j.w_cin + c) * j.w_cout + co];
      tile[ci][coj] = v;
    }
  }
  __syncthreads();
  const int coj = tid >> 2, ch = tid & 3;
  float f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = gr < ng ? tile[ch * 8 + k][coj] : 0.f;
  *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(j.packed) + (long)(co0 + coj) * K_pad + gr * 32 + ch * 8) =
      Chunk<uint16_t>::pack(f);
}

// the flipped (data-gradient) packs of chunk-major bf16 filters: a lane fills one 16-byte run of 8 packed channels,
// whose sources w[8 - tap][co][c .. c + 7] are 8 consecutive floats (the filter's contiguous cout axis), where
// pack_weights_batch decoded and stored one element per thread; same zero padding, same RNE rounding: bit-identical
__global__ __launch_bounds__(256) void pack_weights_flip8(PackBatch b) {
  const int jb = blockIdx.y;
  const vm_pack_job& j = b.j[jb];
  const int K_pad = b.K_pad[jb], ng = 9 * b.cin_pad[jb] / 32, kq8 = K_pad / 8;
  const long total = (long)b.cout_pad[jb] * kq8;
  for (long q = blockIdx.x * 256L + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int co = (int)(q / kq8), kq = (int)(q - (long)co * kq8);
    const int gr = kq >> 2, c0 = (kq & 3) * 8;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (gr < ng && co < j.cout && co < j.w_cin) {
      const int cc = gr / 9, tap = gr - cc * 9;
      const float* src = j.w + ((long)(8 - tap) * j.w_cin + co) * j.w_cout;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = cc * 32 + c0 + k;
        if (c < j.cin && c < j.w_cout) f[k] = src[c];
      }
    }
    *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(j.packed) + (long)co * K_pad + kq * 8) =
        Chunk<uint16_t>::pack(f);
  }
}

}  // namespace vm

using namespace vm;

extern "C" size_t vm_conv3x3_packed_bytes(int cin, int cout, int dtype) {
  if (cin <= 0 || cout <= 0 || (dtype != VM_F32 && dtype != VM_BF16 && dtype != VM_F16)) return 0;
  PackGeom g = geom(cin, cout, dtype);
  return (size_t)g.cout_pad * g.K_pad * elem_bytes(dtype);
}

extern "C" int vm_conv3x3_pack_weights(const float* w_hwio, int cin, int cout, int dtype, void* packed, void* stream) {
  if (!w_hwio || !packed || cin <= 0 || cout <= 0) return fail(VM_EINVAL, "pack_weights: bad argument");
  if (dtype != VM_F32 && dtype != VM_BF16 && dtype != VM_F16) return fail(VM_EINVAL, "pack_weights: dtype %d", dtype);
  PackGeom g = geom(cin, cout, dtype);
  ConvArgs a{};
  fill_geom(a, g);
  a.w = packed;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for((long)g.cout_pad * g.K_pad, 256);
  if (dtype == VM_BF16) hipLaunchKernelGGL(pack_weights<uint16_t>, dim3(grid), dim3(256), 0, st, w_hwio, cin, cout, a);
  else if (dtype == VM_F16) hipLaunchKernelGGL(pack_weights<f16_t>, dim3(grid), dim3(256), 0, st, w_hwio, cin, cout, a);
  else hipLaunchKernelGGL(pack_weights<float>, dim3(grid), dim3(256), 0, st, w_hwio, cin, cout, a);
  return check_launch("pack_weights");
}

extern "C" int vm_conv3x3_pack_weights_batch(int njobs, const vm_pack_job* jobs, void* stream) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return fail(VM_EINVAL, "pack_weights_batch: bad argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int i = 0; i < njobs; ++i) {
    const vm_pack_job& j = jobs[i];
    if (!j.w || !j.packed || j.cin <= 0 || j.cout <= 0 || j.w_cin <= 0 || j.w_cout <= 0 ||
        (j.dtype != VM_F32 && j.dtype != VM_BF16))
      return fail(VM_EINVAL, "pack_weights_batch: bad job %d", i);
  }
  // chunk-major bf16 packs: forward ones to the tiled transpose (pack_weights_tiled), flipped ones 8 channels per
  // lane (pack_weights_flip8); the rest element-wise.  kind 0 element-wise, 1 tiled, 2 flip8
  for (int tiled = 0; tiled < 3; ++tiled) {
    PackBatch b{};
    long mx = 1;
    auto flush = [&]() -> int {
      if (!b.n) return VM_OK;
      if (tiled == 1)
        hipLaunchKernelGGL(pack_weights_tiled, dim3((unsigned)mx, b.n), dim3(256), 0, st, b);
      else if (tiled == 2)
        hipLaunchKernelGGL(pack_weights_flip8, dim3(grid_for(mx, 256, 1024), b.n), dim3(256), 0, st, b);
      else
        hipLaunchKernelGGL(pack_weights_batch, dim3(grid_for(mx, 256, 256), b.n), dim3(256), 0, st, b);
      const int rc = check_launch("pack_weights_batch");
      b.n = 0;
      mx = 1;
      return rc;
    };
    for (int i = 0; i < njobs; ++i) {
      const vm_pack_job& j = jobs[i];
      const PackGeom g = geom(j.cin, j.cout, j.dtype);
      const bool vec = g_opt.pack_tiled && j.dtype == VM_BF16 && g.chunk_major &&
                       reinterpret_cast<uintptr_t>(j.packed) % 16 == 0;
      const int kind = !vec ? 0 : j.flip ? 2 : 1;
      if (kind != tiled) continue;
      b.j[b.n] = j;
      b.K_pad[b.n] = g.K_pad;
      b.cout_pad[b.n] = g.cout_pad;
      b.cin_pad[b.n] = g.cin_pad;
      const long t = tiled == 1 ? (long)(g.K_pad / 32) * (g.cout_pad / 64)
                     : tiled == 2 ? (long)g.cout_pad * (g.K_pad / 8) : (long)g.cout_pad * g.K_pad;
      if (t > mx) mx = t;
      if (++b.n == PACK_MAX_JOBS) {
        const int rc = flush();
        if (rc) return rc;
      }
    }
    const int rc = flush();
    if (rc) return rc;
  }
  return VM_OK;
}
