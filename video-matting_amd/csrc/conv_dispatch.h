// Host side of the 3x3 conv translation units (conv3x3.hip and every conv_*.hip): the tuning options (vm_set_option),
// the call and filter-geometry structs, and the launchers through which one file's routing reaches the kernels of
// another.
#pragma once

#include "conv_common.h"

namespace vm {

// Tuning options of the conv kernels (vm_set_option; the table in conv3x3.hip holds every key's accepted values).
// One instance, defined in conv3x3.hip.  The study-only fields exist in every build (one layout for every translation
// unit); only the study build's table has keys for them.
struct ConvOptions {
  // conv_kernel 0 = auto, 1 = register-staged only, 2 = LDS-DMA whenever legal;
  // conv_min_tiles = smallest grid (in 256-wide output tiles) for which auto picks the LDS-DMA kernel;
  // glds_rb = K-step bytes of the 256x256 LDS-DMA tile (64: 4-slot ring, 128: 2-slot).
  long conv_kernel = 0;
  long conv_min_tiles = 128;
  long glds_rb = 128;
  long head_kernel = 0;
  long head_th = 16;  // conv3x3_head_mfma tile height for the bf16 128-channel head (8 or 16)
  long patch_cfg = 0;
  long softmax_abl = 0;    // (study build) conv3x3_first_softmax_f32 timing ablations
  long patch_rowslot = 1;  // (study build) 0 = the per-tap-barrier dispatch of r01 (A/B runs)
  long patch_ablate = 0;   // (study build) timing experiments on the default patch tiling
  long rows_kernel = 1;        // conv_rows.hip: 0 = off, 1 = auto (grid size), 8 / 16 = forced tile height
  long rows_min_blocks = 400;
  long rows_up = 0;            // 1: the folded upconvs too
  long rows_min_cin = 64;      // r04 A/B: conv2_1 (cin 64, 2040 blocks) +0.3 % on rows<16>; below 64 the
                               // 2-blocks-per-CU patch kernel hides prologue/epilogue better
  // rows<16> bf16: 1 = at a tile's end output rows 0 and 1 (bias / act / pack, their pool) are finished and stored
  // between the last step's two barriers, waves 0-3 before and waves 4-7 behind their MFMAs of input rows 4 and 5, and
  // only rows 2 and 3 after the step; 0 = the whole epilogue after the step's last barrier (A/B, and the reference of
  // tests/test_gpu_rows_retire.py).  Same-box A/B of the 1080p forward: +1.0 % (profiles/rows_retire_ab.txt)
  long rows_retire = 1;
  long rows_ablate = 0;  // (study build) rows<16> tail epilogue: 1 = skipped, 2 = arithmetic kept, nothing written
  long src_span_limit = 0x7ffffff0L;  // split-source byte span the 32-bit offset kernels take (option
                                      // "src_span_limit" lowers it for the fallback tests)
  long pair_strip = 1;  // vm_conv3x3_pair_first*: 1 = the strip-walking kernel (conv_pair.hip) where it applies
  long pair_kernel = 0;  // vm_conv3x3_pair_first_nhwc: 0 = persistent weights-resident kernel when cout == 64,
                         // 1 = streaming patch kernel
  long pair_xin_wide = 1;  // pair kernel, f32 frames with >= 4 channels: two 16-byte loads per pixel (XIN 2)
  long pair_strip_abl = 0;  // study build: timing-only ablations (1 no conv1_1 MFMAs, 2 no conv1_2 MFMAs, 4 no row
                            // barrier, 8 no input DMA, 16 no conv1_2 epilogue; garbage results)
  long pair_strip_pin = 1;  // 1: conv1_2's LDS reads pinned 2 ahead of its MFMAs; 0: left to the scheduler (A/B)
  long conv_prio = 0;  // ConvArgs::prio for the 8-wave conv kernels (patch, persistent patch, row-stationary)

  long border_ks = 1;  // folded-upconv border pass: granule split (1, 2 or 4 wave groups per block)
  // the border pass inside the folded kernel's own launch (ConvArgs::bfuse): 0 = a launch of its own, 1 = the
  // streaming folded kernel takes it (as its first blocks), 2 = the persistent one too (as the blocks after its
  // walkers).  Same-box A/B of the 1080p forward against the separate pass: 1 = +0.4 %, 2 = +1.4..1.7 %
  long border_fuse = 2;
  long up_skip_mask = 3;  // folded upconvs: which zero taps are skipped (1 = kernel row, 2 = column, 3 = both)
  long patch_repi = 1;  // patch kernel: register epilogue (bf16 outputs, no packed frames) where the tiling allows
  // channel-banded patch tiles (ConvArgs::cband): 0 off, 1 folded upconvs, 2 all.  Off: measured on upconv_2 (9.4 MB
  // folded filter) 0.261 -> 0.312 ms and on the L5 convs 0.053 -> 0.057 ms (same box, bench.py --option cband=0|1|2):
  // every XCD then reads the whole input from the Infinity Cache, which costs more than the weight stream it saves
  long cband = 0;
  long cband_bytes = 4L << 20;   // ... for filters of at least this many bytes (an XCD's L2)
  // grouped tile order (ConvArgs::ngroup): this many output tiles per group for filters of >= cband_bytes (0: off) —
  // the XCD working set is ngroup filter slices instead of the whole filter; the input is read tiles_n / ngroup times.
  // Off: same-box A/B (gpurun_out/r6g_ab.log, profiles/r06g_ngroup_ab.log) bf16 forward 2.967 -> 2.993..3.010 ms for
  // ngroup 2..8, f16x3 10.04 -> 10.01..10.04 ms: the re-streamed filter slices come from the Infinity Cache
  long ngroup = 0;
  long pack_tiled = 1;  // 0 = every pack job on the element-wise pack_weights_batch (A/B)
  long up_skip = 1;  // 0 runs the folded upconvs without the zero-tap skipping (A/B)
  // persistent row-slot patch kernel (conv3x3_patch_persist): a resident grid of 8 XCD bands x J walkers, on grids of
  // >= persist_rounds full rounds of items (a shorter walk gains no prologue overlap and its last round is ragged)
  long patch_persist = 1;
  long persist_rounds = 2;
  long persist_up_rounds = 6;
  long persist_all = 0;  // (A/B) every plain grid of >= persist_rounds rounds
  long persist_rot = 0;  // (A/B) walker rotation: 0 = folded upconvs only, 1 = all, 2 = none
  long persist_half = 1;  // (A/B) halfskip walk for frames whose last tile column is <= 16 px (ConvArgs::halfskip)
  long splitk_tiles = 512;  // patch-kernel split-K: grids under this many 4 x 32 pixel x 64 channel tiles (splitk_plan)
  // packed frames (ConvArgs::vstride): a batch of narrow frames tiled as one virtual image (plan_packed_frames)
  long pack_frames = 1;

  long thin_kernel = 1;  // narrow-cout convs (conv3x3_thin)
  long narrowin_kernel = 1;  // narrow-input convs (conv3x3_narrowin)
  // thin split-K plan: below 1024 blocks of 8 x 32 pixels, split the 32-channel chunks over ~thin_blocks (512) blocks
  long thin_th = 8, thin_blocks = 512;
  long thin_rounds = 1;  // persistent grid: at most this many resident rounds of blocks (0: one block per tile)
  // the LDS-DMA thin kernel (conv3x3_thin_dma): 0 off; 1 = 8-row tiles, 3-slot ring; 2 = 4-row tiles, 4 slots;
  // 3 = 4-row tiles, 3 slots; 4 = 8-row tiles, 2 slots.  A resident grid of thin_dma_rounds x blocks per CU x CUs
  long thin_dma = 0, thin_dma_rounds = 1;
  long thin_rowreuse = 1;  // conv3x3_thin: thin_chunk's row reuse (0: the r03 tap-major loop)
  long thin_twalk = 1;     // conv3x3_thin: XCD-banded tile walk (ConvArgs::twalk; 0: round-robin)

  long softmax_kernel = 6;  // 0: the generic kernels' softmax epilogue, 1: conv3x3_first_softmax, 2: its NT form,
                            // 3 / 4: plain / NT with the per-wave LDS transpose (whole-pixel stores), 5: 4 with
                            // LDS weights, 6: wave-private strips (conv3x3_first_softmax_strip, default)
  long softmax_blocks = 2048;  // persistent grid of conv3x3_first_softmax*
  // the pipelined f32 refine kernel's variant: 0 the r03 kernel; 1 pipelined; 2 its 4-waves-per-SIMD build; 3 NT
  // stores; 4 / 5 LDS-transposed whole-pixel stores, NT / through L2; 6 the row-ring form
  // (conv3x3_first_softmax_f32r); 7 split-bf16 x6
  long softmax_f32p = 4;
};
extern ConvOptions g_opt;

// name of the kernel the last conv call on this thread launched, spelled as rocprofv3 reports it
// (bench.py matches its per-launch PMC traffic by this name); defined in conv3x3.hip
extern thread_local char g_last_kernel[128];

// geometry of a packed filter (vm_conv3x3_pack_weights; the K layout of conv3x3.hip's header comment)
struct PackGeom {
  int cin_pad, ge, K9, K_pad, cout_pad, chunk_major, ng;
};

inline PackGeom geom(int cin, int cout, int dtype) {
  PackGeom g;
  g.ge = 64 / elem_bytes(dtype);
  g.cin_pad = (cin + 7) / 8 * 8;
  g.K9 = 9 * g.cin_pad;
  g.chunk_major = g.cin_pad % g.ge == 0;
  g.ng = g.chunk_major ? g.K9 / g.ge : 0;
  g.K_pad = (g.K9 + 2 * g.ge - 1) / (2 * g.ge) * (2 * g.ge);  // whole 128-byte steps
  g.cout_pad = (cout + 63) / 64 * 64;
  return g;
}

inline void fill_geom(ConvArgs& a, const PackGeom& g) {
  a.cin_pad = g.cin_pad;
  a.K9 = g.K9;
  a.chunk_major = g.chunk_major;
  a.ng = g.ng;
  a.K_pad = g.K_pad;
  a.cout_pad = g.cout_pad;
}

// split-fp16 x3 output of vm_conv3x3_split3_nhwc (ConvArgs::ysplit / psplit / ovf)
struct SplitOut {
  int yslab, pslab;
  int* ovf;
};

// One conv call as the C entry points hand it to conv_impl: the arguments every entry point has, then the optional ones
struct ConvCall {
  const vm_tensor* x;
  const void* packed;
  int cin, cout;
  const float* bias;
  const float* scale;
  const float* shift;
  int act;
  vm_tensor* y;
  void* stream;
  const vm_tensor* yp = nullptr;  // fused 2x2/2 SAME max-pool output
  float* y2 = nullptr;            // cout == 1: sigmoid of the pre-activation value (HeadArgs::y2)
  int nsrc = 0;                   // > 1: split sources, x the view of source 0, source s at s * src_stride elements
  long src_stride = 0;
  void* work = nullptr;           // split-K workspace (vm_conv3x3_workspace_bytes)
  size_t work_bytes = 0;
  const float* head_part = nullptr;  // cout == 1: HeadArgs::part
  const float* y_acc = nullptr;      // cout == 1: HeadArgs::yacc
  const SplitOut* so = nullptr;      // split-fp16 x3 output
};

// a split-fp16 view (vm_conv3x3_split3_nhwc, vm_conv3x3_up2x_split3_nhwc): c channels inside the first of two (or
// three) slabs of slab % 8 == 0 channels, 16-byte aligned
inline bool split3_view_ok(const vm_tensor* t, int slab, int c) {
  return t->dtype == VM_F16 && view16_ok(t) && slab > 0 && slab % 8 == 0 && t->coff + c <= slab && 2 * slab <= t->cstride;
}

// conv_patch.hip (called from conv_impl, dispatch_mfma and conv_up2x.hip); a kernel is launched from its own unit only
bool patch_ok(const ConvArgs& a, size_t tsize);
int dispatch_patch(ConvArgs& a, hipStream_t st);
int splitk_plan(long n, int h, int w, int cin_pad, int cout);
int launch_splitk_reduce(const ConvArgs& a, hipStream_t st);  // a.part's a.ksplit partial sums -> a.y (conv_thin.hip too)
int launch_patch_first(ConvArgs& a, hipStream_t st);  // the FIRST patch kernel: conv_pair.hip's streaming fallback
// conv_thin.hip (called from conv_impl and vm_conv3x3_workspace_bytes)
bool thin_ok(int dt, const PackGeom& g, int cout, int x_src_c, int act, const vm_tensor* x);
bool narrowin_ok(const ConvArgs& a, const PackGeom& g, int cout, int act, const vm_tensor* x, const vm_tensor* y);
int launch_narrowin(ConvArgs& a, long n, const PackGeom& g, hipStream_t st);
int thin_splitk_plan(long n, int h, int w, int cin_pad);
int dispatch_thin(ConvArgs& a, long n, hipStream_t st);
// launchers defined in conv_rows.hip (called from dispatch_patch)
bool rows_ok(const ConvArgs& a);
int launch_rows(ConvArgs& a, hipStream_t st, int cfg);
// launchers defined in conv_first.hip (dispatch_mfma decides when they apply)
int launch_first(ConvArgs& a, hipStream_t st);
int launch_first_softmax(ConvArgs& a, hipStream_t st);
int launch_first_softmax_f32(ConvArgs& a, int cin, hipStream_t st);
// conv_head.hip: conv_impl's cout == 1 route (tile choice, head_th, head_kernel)
int dispatch_head(const ConvCall& c, const PackGeom& g, int xalias, long M, hipStream_t st);

}  // namespace vm
