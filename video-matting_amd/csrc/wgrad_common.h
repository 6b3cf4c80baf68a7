// What the weight-gradient units share (wgrad.hip: FMA kernel, reductions, routing, entry points; wgrad_mfma.hip,
// wgrad_taps.hip, wgrad_wide.hip: one MFMA family each, kernel templates next to the launchers that instantiate them):
// the MFMA kernels' argument block, LDS image swizzle and fragment read, and the host functions called across units.
#pragma once

#include <initializer_list>

#include "train_common.h"

namespace vm {
namespace trn {

constexpr int WM_TW = 32, WM_PW = WM_TW + 2;
// patch pixels of a TH x 32 tile with its halo, and the image rows allocated for them (a multiple of 16, so the row
// swizzle stays in range)
template <int TH>
constexpr int wm_ppix() { return (TH + 2) * WM_PW; }
template <int TH>
constexpr int wm_prows() { return (wm_ppix<TH>() + 15) / 16 * 16; }

struct WgArgs {
  const uint16_t* x;  // bf16 input view base (pixel 0, channel coff applied)
  int n, h, w, cin, xcs, x_src_c;  // x_src_c > 0: channel c lives in source c / x_src_c at + x_src_stride elements
  long x_src_stride;
  const float* dy;  // f32 output-gradient view base (coff applied)
  int cout, dcs;
  float* part;      // [gridDim.x][9][cin][cout]
  int tiles_h, tiles_w;
  long ntiles;
};

// byte offset of 32-byte piece c (16 bf16 channels) of image row r, rows of RB bytes (32, 64 or 128)
template <int RB>
__device__ __forceinline__ int wm_off(int r, int c) {
  if constexpr (RB == 32) return 32 * (r ^ (((r >> 3) & 1) << 2));
  else if constexpr (RB == 64) return 64 * r + 32 * (c ^ ((r >> 3) & 1));
  else return 128 * r + 32 * (c ^ ((r >> 1) & 1) ^ (((r >> 3) & 1) << 1));
}

typedef short v4s __attribute__((ext_vector_type(4)));

// the 16x16x32 operand fragment whose k rows are image rows rk(0..7) (8 consecutive pixels of one image row band),
// columns = 16-channel piece c: two transposed 4-row reads
template <int RB>
__device__ __forceinline__ bf16x8 wm_frag(const char* img, int r0, int c, int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3;
  typedef __attribute__((address_space(3))) v4s* lp;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + wm_off<RB>(r0 + q, c) + 8 * p));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(img + wm_off<RB>(r0 + 4 + q, c) + 8 * p));
  v4s v[2] = {lo, hi};
  return __builtin_bit_cast(bf16x8, v);
}

// ---------------------------------------------------------------- host side (options: wgrad.hip's wgrad_options)
extern long g_wgrad_mfma_pipe, g_wgrad_dma, g_wgrad_dma_cfg, g_wgrad_wide_pipe, g_wgrad_wide_cs, g_wgrad_wide_dbuf,
    g_wgrad_wide_target;

void launch_wgrad_reduce(const float* part, int rows, long S, float* dw, hipStream_t st);
long wgrad_rows(int n, int h, int w, int cin, int cout, int cc);
int wgrad_lds_once(const char* what, std::initializer_list<const void*> kerns, int lds, int& attr_dev);
int launch_wgrad_grid(const void* kern, int lds, int th, int cib, int& attr_dev, int& resident, WgArgs& a, float* dw,
                      hipStream_t st, void (*launch)(dim3, int, hipStream_t, const WgArgs&));
// wgrad_mfma.hip, wgrad_taps.hip: the (nci, nco) / (nci, nt) tiling on th-row tiles (4 or 8); the LDS-DMA form if it is ok
int launch_wgrad_mfma_tiled(WgArgs& a, int nci, int nco, int th, float* dw, hipStream_t st);
int launch_wgrad_taps(WgArgs& a, int nci, int nt, int th, float* dw, hipStream_t st);
bool wgrad_dma_ok(const WgArgs& a);
int launch_wgrad_taps_dma(WgArgs& a, float* dw, hipStream_t st);
constexpr int WW_TARGET_BLOCKS = 512;  // ~2 resident blocks per CU: one round; the partials stay <= 75 MB
long wgrad_wide_gx(int n, int h, int w, int cin, int cout, bool f32, long target = WW_TARGET_BLOCKS);
int launch_wgrad_wide(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, hipStream_t st);
int launch_wgrad_wide_f32(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, hipStream_t st);

// the view fields every weight-gradient args struct (WgArgs, WwArgs, WfArgs) starts from: bases with coff applied
template <typename A>
A wgrad_args(const vm_tensor* x, const vm_tensor* dy, void* work) {
  A a{};
  a.x = reinterpret_cast<decltype(a.x)>(reinterpret_cast<const char*>(x->ptr) + (long)x->coff * elem_bytes(x->dtype));
  a.n = x->n; a.h = x->h; a.w = x->w; a.cin = x->c; a.xcs = x->cstride;
  a.dy = reinterpret_cast<decltype(a.dy)>(reinterpret_cast<const char*>(dy->ptr) + (long)dy->coff * elem_bytes(dy->dtype));
  a.cout = dy->c; a.dcs = dy->cstride; a.part = reinterpret_cast<float*>(work);
  return a;
}

// launch_wgrad_grid for kernel K; its LDS-attribute device and chip-wide resident blocks are cached per instantiation
template <void (*K)(WgArgs)>
int launch_wgrad_grid_k(int lds, int th, int cib, WgArgs& a, float* dw, hipStream_t st) {
  static int attr_dev = -1, resident = 0;
  return launch_wgrad_grid(reinterpret_cast<const void*>(K), lds, th, cib, attr_dev, resident, a, dw, st,
                           [](dim3 g, int l, hipStream_t s, const WgArgs& x) {
                             hipLaunchKernelGGL(K, g, dim3(256), l, s, x); });
}

// runtime value -> template parameter: f(std::integral_constant<int, X>) for the listed X equal to v, else the last X
template <int X, int... Xs, typename F>
int dispatch(int v, F&& f) {
  if constexpr (sizeof...(Xs) == 0) return f(std::integral_constant<int, X>{});
  else return v == X ? f(std::integral_constant<int, X>{}) : dispatch<Xs...>(v, f);
}

}  // namespace trn
}  // namespace vm
