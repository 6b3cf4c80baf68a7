// The folded 2x resize + 3x3 conv (unet.py:44-63 upconv_concat): the phase-filter fold, the border pass that recomputes
// the frame's outer ring, and the vm_conv3x3_up2x* entry points (bf16, split-fp16 x3 and head-split forms), which run
// the folded conv itself on the patch kernel (conv_patch.hip).
#include "conv_border.h"
#include "conv_dispatch.h"

namespace vm {

// ================================================================ folded 2x resize (unet.py:44-63 upconv_concat)
// conv3x3(resize2x(x)) with TF1 legacy bilinear (scale 0.5) is linear in x: resized row 2i = x[i], row 2i+1 =
// (x[i] + x[i+1]) / 2.  So output pixel (2i+a, 2j+b) is a 3x3 conv of the LOW-RES frame at (i, j) with a phase
// filter W'_ab[u][v] = sum_{kh,kw} R_a[u][kh] R_b[v][kw] W[kh][kw], u,v in {-1,0,+1}:
//   R_0 = [[.5,0,0],[.5,1,.5],[0,0,.5]]  (rows u, columns kh)      R_1 = [[0,0,0],[1,.5,0],[0,.5,1]]
// Output channel p*cout + co of the folded conv is phase p = 2a+b of channel co.  Exact in the interior and, with
// the low-res frame replicated past its bottom/right edge, at output rows/columns 2H-2; output row/column 0 and
// 2H-1 / 2W-1 see the resized image's zero padding instead and are recomputed by conv3x3_up2x_border.
__global__ void fold_up2x_weights(const float* w, int cin, int cout, float* wu) {
  const long total = 9L * cin * cout;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % cout);
    const long r = i / cout;
    const int ci = (int)(r % cin);
    const int tap = (int)(r / cin), u = tap / 3, v = tap % 3;  // low-res tap (u, v) = offset (u-1, v-1)
    constexpr float R[2][3][3] = {{{.5f, 0.f, 0.f}, {.5f, 1.f, .5f}, {0.f, 0.f, .5f}},
                                  {{0.f, 0.f, 0.f}, {1.f, .5f, 0.f}, {0.f, .5f, 1.f}}};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int pa = p >> 1, pb = p & 1;
      double s = 0.0;
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) {
          const float c = R[pa][u][kh] * R[pb][v][kw];
          if (c != 0.f) s += (double)c * (double)w[((long)(kh * 3 + kw) * cin + ci) * cout + co];
        }
      wu[((long)tap * cin + ci) * (4L * cout) + (long)p * cout + co] = (float)s;
    }
  }
}

// The border pass as a kernel of its own (conv_border.h has the body): block (x, y) = the 16 border pixels from 16 x,
// output channels 64 y .. +63; BD_KS 4-wave groups split the granules
template <int BD_KS, bool SPL = false>  // granule split of the border pass (waves = 4 x BD_KS)
__global__ __launch_bounds__(256 * BD_KS) void conv3x3_up2x_border(BorderArgs a) {
  __shared__ __attribute__((aligned(16))) char stg[BD_KS * 2 * BORDER_STG];  // [split][buffer][tap][pixel][32 ch]
  __shared__ __attribute__((aligned(16))) float red[BD_KS * 16 * 64];        // [split][pixel][channel] partial sums
  up2x_border_body<BD_KS, SPL, false>(a, stg, red, (int)threadIdx.x, (long)blockIdx.x * 16, (int)blockIdx.y * 64);
}

}  // namespace vm

using namespace vm;

extern "C" int vm_conv3x3_fold_up2x_weights(const float* w_hwio, int cin, int cout, float* w_up_hwio, void* stream) {
  if (!w_hwio || !w_up_hwio || cin <= 0 || cout <= 0) return fail(VM_EINVAL, "fold_up2x: bad argument");
  hipLaunchKernelGGL(fold_up2x_weights, dim3(grid_for(9L * cin * cout, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), w_hwio, cin, cout, w_up_hwio);
  return check_launch("fold_up2x_weights");
}

// One call of a folded upconv (vm_conv3x3_up2x*), checked by its entry point: the arguments every form has, then the
// optional ones
struct UpCall {
  const vm_tensor* x;
  const void* packed_up;
  const void* packed;
  int cin, cout;
  const float* bias;
  const float* scale;
  const float* shift;
  int act;
  vm_tensor* y;
  void* stream;
  const float* head_w = nullptr;  // head split (ConvArgs::hd): conv1_5's HWIO f32 filter, ours at head_coff
  int head_cin = 0, head_coff = 0;
  float* partial = nullptr;       // ... its per-tap partials [pixel][12]; store_y = 0 leaves y unwritten
  int store_y = 1;
  int ysplit = 0;                 // > 0: the split-fp16 x3 form (x = [l, h] slabs, y split at this slab)
  int* overflow = nullptr;
};

static thread_local int g_last_bfuse = 0;  // vm_conv3x3_last_border_fused

extern "C" int vm_conv3x3_last_border_fused(void) { return g_last_bfuse; }

// the folded conv on the patch kernel (interior and, replicated, the far edges), then the border pass (or, with
// border_fuse, both in the folded kernel's launch)
static int up2x_impl(const UpCall& c) {
  const vm_tensor *x = c.x, *y = c.y;
  const bool spl = c.ysplit > 0;
  const char* name = spl ? "conv3x3_up2x_split3" : "conv3x3_up2x";
  const PackGeom g = geom(c.cin, 4 * c.cout, x->dtype), g1 = geom(c.cin, c.cout, x->dtype);
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  ConvArgs a{};
  BorderArgs b{};
  a.x = b.x = x->ptr; a.x_cstride = b.x_cstride = x->cstride; a.x_coff = b.x_coff = x->coff;
  a.H = b.H = x->h; a.W = b.W = x->w; b.nframes = x->n;
  a.M = (long)x->n * x->h * x->w;
  fill_geom(a, g);
  a.w = c.packed_up; a.cout = 4 * c.cout;
  b.w = c.packed; b.K_pad = g1.K_pad; b.cout = c.cout; b.nch = g1.cin_pad / 32;
  a.bias = b.bias = c.bias; a.scale = b.scale = c.scale; a.shift = b.shift = c.shift; a.act = b.act = c.act;
  a.y = b.y = y->ptr; a.y_cstride = b.y_cstride = y->cstride; a.y_coff = b.y_coff = y->coff;
  a.y_dtype = spl ? VM_F32 : y->dtype;  // split: f32 staging, split stores (ConvArgs::ysplit)
  a.y_vec = 1;
  a.up = 1; a.up_cout = c.cout;
  a.hd = b.hd = c.partial; a.hw = b.hw = c.head_w; a.hw_cin = b.hw_cin = c.head_cin; a.hw_coff = b.hw_coff = c.head_coff;
  a.y_skip = b.y_skip = c.store_y ? 0 : 1;
  if (spl) {
    a.ysplit = b.ysplit = c.ysplit; a.ovf = b.ovf = c.overflow;
    a.f16 = 1; a.xalias = b.xs = x->c / 2; a.ksplit = 1;
  }
  if (!patch_ok(a, 2)) return fail(VM_EUNSUPPORTED, "%s: shape not supported by the patch kernel", name);
  // border_fuse: the folded kernel's launch may take the border pass along (ConvArgs::bfuse says whether it did)
  a.bwant = spl ? 0 : (int)g_opt.border_fuse;
  a.bw = b.w; a.bK_pad = b.K_pad; a.bframes = x->n;
  const int rc = dispatch_patch(a, st);
  if (rc != VM_OK) return rc;
  g_last_bfuse = a.bfuse;
  if (a.bfuse) return VM_OK;
  const int OH = 2 * x->h, OW = 2 * x->w;
  b.nb = 2 * OW + 2 * (OH - 2);
  const long nblk = ((long)x->n * b.nb + 15) / 16;
  if (nblk > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "%s: too many border pixels", name);
  const dim3 grid((unsigned)nblk, c.cout / 64);
  if (spl) hipLaunchKernelGGL((conv3x3_up2x_border<4, true>), grid, dim3(1024), 0, st, b);
  else if (g_opt.border_ks == 4) hipLaunchKernelGGL(conv3x3_up2x_border<4>, grid, dim3(1024), 0, st, b);
  else if (g_opt.border_ks == 2) hipLaunchKernelGGL(conv3x3_up2x_border<2>, grid, dim3(512), 0, st, b);
  else hipLaunchKernelGGL(conv3x3_up2x_border<1>, grid, dim3(256), 0, st, b);
  return check_launch(spl ? "conv3x3_up2x_border(split)" : "conv3x3_up2x_border");
}

// the bf16 form's checks (vm_conv3x3_up2x_nhwc, and vm_conv3x3_up2x_head_nhwc after its own)
static int up2x_bf16(const UpCall& c) {
  const vm_tensor *x = c.x, *y = c.y;
  const int cin = c.cin, cout = c.cout;
  if (!valid_tensor(x) || !valid_tensor(y) || !c.packed_up || !c.packed)
    return fail(VM_EINVAL, "conv3x3_up2x: invalid tensor/weights");
  if (cin <= 0 || cout <= 0 || x->c != cin || y->c != cout)
    return fail(VM_EINVAL, "conv3x3_up2x: channel mismatch x.c=%d cin=%d y.c=%d cout=%d", x->c, cin, y->c, cout);
  if (y->n != x->n || y->h != 2 * x->h || y->w != 2 * x->w)
    return fail(VM_EINVAL, "conv3x3_up2x: output must be [%d,%d,%d,%d]", x->n, 2 * x->h, 2 * x->w, cout);
  if (c.act < VM_ACT_NONE || c.act > VM_ACT_SOFTMAX) return fail(VM_EINVAL, "conv3x3_up2x: act %d", c.act);
  const bool xvec = view16_ok(x) && x->coff + geom(cin, 4 * cout, x->dtype).cin_pad <= x->cstride;
  if (x->dtype != VM_BF16 || y->dtype != VM_BF16 || cout % 64 || !xvec || !view16_ok(y) || c.act == VM_ACT_SOFTMAX ||
      g_opt.conv_kernel == 1 || g_opt.conv_kernel == 2)
    return fail(VM_EUNSUPPORTED, "conv3x3_up2x: folded resize needs the bf16 patch kernel (cout %% 64 == 0, "
                                 "16-byte channel views)");
  return up2x_impl(c);
}

extern "C" int vm_conv3x3_up2x_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin, int cout,
                                    const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                                    void* stream) {
  return up2x_bf16({x, packed_up, packed, cin, cout, bias, scale, shift, act, y, stream});
}

extern "C" int vm_conv3x3_up2x_split3_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin,
                                           int cout, const float* bias, const float* scale, const float* shift, int act,
                                           vm_tensor* y, int y_slab, int* overflow, void* stream) {
  if (!valid_tensor(x, true) || !valid_tensor(y, true) || !packed_up || !packed)
    return fail(VM_EINVAL, "conv3x3_up2x_split3: invalid tensor/weights");
  const int S = x->c / 2;
  if (x->dtype != VM_F16 || y->dtype != VM_F16 || x->c % 64 || cin != 3 * S || y->c != cout)
    return fail(VM_EINVAL, "conv3x3_up2x_split3: fp16 views, x = [l, h] slabs of S %% 32 == 0 channels, cin = 3 S "
                           "(x.c=%d cin=%d y.c=%d cout=%d)", x->c, cin, y->c, cout);
  if (y->n != x->n || y->h != 2 * x->h || y->w != 2 * x->w)
    return fail(VM_EINVAL, "conv3x3_up2x_split3: output must be [%d,%d,%d,%d]", x->n, 2 * x->h, 2 * x->w, cout);
  if (act < VM_ACT_NONE || act >= VM_ACT_SOFTMAX) return fail(VM_EINVAL, "conv3x3_up2x_split3: act %d", act);
  const int ys = y_slab > 0 ? y_slab : y->cstride / 2;
  const bool xvec = view16_ok(x) && x->coff + x->c <= x->cstride;
  if (cout % 64 || !xvec || !split3_view_ok(y, ys, cout) || !g_opt.up_skip || g_opt.conv_kernel == 1 || g_opt.conv_kernel == 2)
    return fail(VM_EUNSUPPORTED, "conv3x3_up2x_split3: cout %% 64 == 0, 16-byte channel views, the split layout");
  UpCall c{x, packed_up, packed, cin, cout, bias, scale, shift, act, y, stream};
  c.ysplit = ys;
  c.overflow = overflow;
  return up2x_impl(c);
}

extern "C" int vm_conv3x3_up2x_head_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin,
                                         int cout, const float* bias, const float* scale, const float* shift, int act,
                                         vm_tensor* y, const float* head_w, int head_cin, int head_coff, float* partial,
                                         int store_y, void* stream) {
  if (!head_w || !partial || cout != 64 || head_cin <= 0 || head_coff < 0 || head_coff + cout > head_cin)
    return fail(VM_EINVAL, "conv3x3_up2x_head: head filter [3,3,%d,1] with the conv's %d channels at %d", head_cin, cout,
                head_coff);
  // the partials come from the patch kernel's register epilogue (64-channel row-slot tilings)
  if (!g_opt.patch_repi || g_opt.patch_cfg || g_opt.rows_up || !g_opt.up_skip)
    return fail(VM_EUNSUPPORTED, "conv3x3_up2x_head: needs the patch kernel's register epilogue");
  return up2x_bf16({x, packed_up, packed, cin, cout, bias, scale, shift, act, y, stream, head_w, head_cin, head_coff,
                    partial, store_y});
}
