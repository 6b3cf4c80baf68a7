/*
 * vmatting.h — C ABI of the MI355X (gfx950) per-frame alpha-matting path.
 *
 * Drop-in boundary for the hot path of tangih/video-matting.  The reference is
 * TensorFlow-1.x graph code: its "FFI" is the TF op set reached through
 * sess.run (train.py:81,330).  Each entry point below replaces the TF/OpenCV
 * op(s) the reference's model builders and flow helpers call, cited per
 * function.  A Python host (video-matting_amd/vmatting/_lib.py) binds this with
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers owned by the caller (e.g. from
 *     torch.Tensor.data_ptr() on ROCm); nothing is allocated inside a call.
 *   - Activations are NHWC views (vm_tensor): element (n,h,w,c) lives at
 *     ptr + ((n*H + h)*W + w)*cstride + coff + c, in elements of `dtype`.
 *     A channel slice of a wider buffer (coff, cstride) is how a tf.concat is
 *     expressed without a copy (unet.py:62, unet_simple.py:41, small.py:22).
 *   - `stream` is a hipStream_t (void* here so the header needs no HIP include);
 *     every call is asynchronous on it and is capturable into a hipGraph.
 *   - Return value: VM_OK (0) or a negative VM_E* code; vm_last_error() gives a
 *     per-thread message.  No exception crosses the ABI.
 *   - Thread-safety: reentrant; calls on different streams may run concurrently.
 */
#ifndef VMATTING_H
#define VMATTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when an existing entry point's signature, a struct layout or an enum value changes; entry points that are
 * only added leave it alone (an older host still finds everything it binds). */
#define VM_ABI_VERSION 1

enum vm_dtype {
  VM_F32 = 0,
  VM_BF16 = 1,
  VM_U8 = 2,
  VM_F64 = 3, /* loader outputs only */
  VM_F16 = 4  /* IEEE half: the split-fp16 x3 conv operands only (vm_split3h_nhwc, vm_conv3x3_ex_nhwc, head_acc) */
};

enum vm_act {
  VM_ACT_NONE = 0,
  VM_ACT_RELU = 1,     /* tf.nn.relu            (unet.py:96 ...)            */
  VM_ACT_SIGMOID = 2,  /* tf.nn.sigmoid         (unet.py:145,205)           */
  VM_ACT_SOFTMAX = 3   /* tf.nn.softmax, last axis (refine.py:31)           */
};

enum vm_status {
  VM_OK = 0,
  VM_EINVAL = -1,        /* bad argument / shape mismatch (TF: ValueError at build) */
  VM_EUNSUPPORTED = -2,  /* valid but not supported by this build                    */
  VM_EHIP = -3,          /* HIP runtime error                                        */
  VM_EINDEX = -4         /* data-dependent index error (flow.correct_alpha IndexError) */
};

typedef struct vm_tensor {
  void* ptr;
  int32_t n, h, w, c;     /* logical shape                                  */
  int32_t cstride, coff;  /* channel stride of the pixel row / first channel */
  int32_t dtype;          /* enum vm_dtype                                   */
} vm_tensor;

int vm_abi_version(void);
const char* vm_last_error(void);
/* Process-wide tuning knobs (no reference counterpart; TF picks kernels itself):
 *   "conv_kernel"    0 = auto (default: patch kernel when legal, else by shape), 1 = register-staged MFMA kernel
 *                    only, 2 = LDS-DMA kernel when legal, 3 = patch-reuse kernel when legal (bf16, cin % 32 == 0,
 *                    bf16 output, no softmax)
 *   "patch_cfg"      patch-kernel tiling override (0 = dispatcher's choice; 19, 22, 25, 30 = one of the tilings it
 *                    picks); the other sweep tilings and the timing-only ablations ("patch_ablate", "patch_rowslot",
 *                    "pair_kernel" 10..18, garbage results) exist only in the study build (`make study`), never here
 *   "up_skip"        folded 2x upconvs: 1 = skip the exact-zero taps of the odd phases' filters (25 of 36 taps run,
 *                    bit-identical, default), 0 = run all 36
 *   "src_span_limit" byte span of split sources the 32-bit-offset conv kernels take (default 0x7ffffff0; wider
 *                    spans return VM_EUNSUPPORTED and the caller materialises the concat); lowered by tests
 *   "conv_min_tiles" grid size (256-wide output tiles) from which auto uses the LDS-DMA kernel (default 128)
 *   "glds_rb"        K-step bytes of the 256x256 LDS-DMA tile: 128 (2-slot ring, default) or 64 (4-slot)
 *   "head_kernel"    cout == 1 convs: 0 = MFMA tap-GEMM kernel (default), 1 = generic per-pixel kernel,
 *                    2 = register-strip kernel
 *   "softmax_kernel" cin <= 8 -> 64 conv + softmax (refine.py conv4): 0 = generic kernels' epilogue; bf16: 1 =
 *                    conv3x3_first_softmax (register stores), 2 = its nontemporal form, 3 / 4 = per-wave LDS transpose
 *                    with whole-pixel plain / nontemporal stores, 5 = 4 with the weights in LDS, 6 = wave-private
 *                    strips, no per-tile block barrier (default); f32: any value but 0 = conv3x3_first_softmax_f32
 *   "softmax_blocks" persistent grid of the conv3x3_first_softmax kernels (default 2048)
 *   "pair_xin_wide"  pair kernel, f32 frames with 4..8 channels: 1 = two 16-byte loads per pixel (default),
 *                    0 = one dword load per channel
 *   "pair_strip"     first pair: 1 = strip-walking kernel where it applies (default), 0 = tile kernels
 *   "patch_repi"     patch kernel register epilogue: 1 (default) / 0 = LDS-staged epilogue
 *   "patch_persist"  1 = persistent row-slot patch kernel where the round policy says it pays (default), 0 = off
 *   "persist_rounds", "persist_up_rounds"  its minimum rounds of items for plain convs (default 2) and folded
 *                    upconvs (default 6); 0 = any grid (tests)
 *   "persist_all"    1 = every plain grid of >= persist_rounds rounds (A/B); "persist_rot" 0 = walkers rotate
 *                    through the output tiles for folded upconvs only (default), 1 = always, 2 = never
 *   "rows_kernel", "rows_min_blocks", "rows_min_cin", "rows_up"  row-stationary kernel dispatch (1, 400, 128, 0)
 *   "rows_retire"    row-stationary kernel (bf16, 16-row tiles): 1 = a tile's output rows 0 and 1 are finished and
 *                    stored inside its last step, beside the other wave's MFMAs (default), 0 = the whole epilogue
 *                    after the step (bit-identical)
 *   "border_ks"      folded-upconv border pass granule split: 1 (default), 2 or 4
 *   "border_fuse"    the border pass in extra blocks of the folded kernel's own launch instead of a launch of its
 *                    own: 0 = off, 1 = in the streaming folded kernel, 2 = in the persistent one too (default;
 *                    bit-identical; split-K, the split-fp16 form and the row-stationary kernel keep the separate pass)
 *   The patch / row-stationary / persistent / strip choices and "up_skip" are bit-identical (every output keeps its
 *   MFMA sequence); "conv_kernel", "head_kernel" and "softmax_kernel" pick kernels with another f32 summation order
 *   (within the stated tolerances). */
int vm_set_option(const char* key, long value);
/* Name of the conv kernel the calling thread's last vm_conv3x3_nhwc launched, spelled the way
 * rocprofv3 reports it (e.g. "vm::conv3x3_mfma<unsigned short, 128, 128>"); "" before the first call.
 * Used to attribute per-kernel profiler counters (bench.py); no reference counterpart. */
const char* vm_conv3x3_last_kernel(void);
/* 1 if the calling thread's last vm_conv3x3_up2x*_nhwc ran its border pass inside the folded kernel's launch
 * ("border_fuse"), 0 if it launched the border kernel.  For tests and profiles; no reference counterpart. */
int vm_conv3x3_last_border_fused(void);

/* ---------------------------------------------------------------- 3x3 convolution
 * Replaces tf.nn.conv2d(x, w, [1,1,1,1], 'SAME') + tf.nn.bias_add + the activation /
 * inference batch-norm that follows it:
 *   unet.py:35-42 (new_conv), 44-63 (upconv conv), 65-74 (conv_layer);
 *   unet_simple.py:19-27, 30-42, 98-107; small.py:13-34; refine.py:18-25.
 * y = act((conv(x, w) + bias) * scale + shift) per output channel; bias/scale/shift
 * may be NULL (f32 device arrays of length cout).  Weights are first packed from
 * TF's HWIO f32 layout into the kernel's [cout_pad][K_pad] layout (K ordered channel-chunk-major:
 * the 9 taps of each 128-byte channel chunk are consecutive, so shared input rows stay L2-resident).
 * Computes in x->dtype (bf16 -> MFMA 16x16x32 bf16, f32 -> exact-f32 MFMA 16x16x4),
 * accumulates in f32.  cout == 1 dispatches the memory-bound head kernel.
 * act == VM_ACT_SOFTMAX needs cout <= 128 (whole channel row in one tile).
 */
size_t vm_conv3x3_packed_bytes(int cin, int cout, int dtype);
int vm_conv3x3_pack_weights(const float* w_hwio, int cin, int cout, int dtype, void* packed, void* stream);

/* Many packs in ONE launch (the optimizer step re-packs every trainable filter, train.py:302-304).  A job packs the
 * conv geometry (cin, cout, dtype) from an f32 HWIO source filter of (w_cin, w_cout) channels, zero outside it
 * (a cout-padded narrow conv); flip = 1 packs the data-gradient filter of that source instead (spatially flipped,
 * in/out transposed: cin = the source's output channels (padded), cout = its input channels). */
typedef struct vm_pack_job {
  const float* w;
  void* packed;
  int32_t cin, cout, dtype, flip, w_cin, w_cout;
} vm_pack_job;
int vm_conv3x3_pack_weights_batch(int njobs, const vm_pack_job* jobs, void* stream);
int vm_conv3x3_nhwc(const vm_tensor* x, const void* packed, int cin, int cout, const float* bias,
                    const float* scale, const float* shift, int act, vm_tensor* y, void* stream);
/* The same conv over the channel concat of nsrc sources (unet_simple.py:153-168's per-level concat of the three
 * towers, tower-major in HBM so the towers run as one batch): x is the [n,h,w,c_src] view of source 0, source s
 * lies src_stride elements further; cin = nsrc * x->c, and x->c must be whole 64-byte granules. */
/* vm_conv3x3_nhwc / vm_conv3x3_sources_nhwc with a caller workspace: small-grid bf16 convs with a long K loop
 * (the deep levels of unet_simple's towers and heads) split their channel granules over ~1024 blocks and reduce the
 * f32 partial sums in a fixed order (deterministic).  nsrc 0/1 = one source.  work: vm_conv3x3_workspace_bytes. */
size_t vm_conv3x3_workspace_bytes(const vm_tensor* x, int cin, int cout);
int vm_conv3x3_ex_nhwc(const vm_tensor* x, int nsrc, long src_stride, const void* packed, int cin, int cout,
                       const float* bias, const float* scale, const float* shift, int act, vm_tensor* y, void* work,
                       size_t work_bytes, void* stream);
int vm_conv3x3_sources_nhwc(const vm_tensor* x, int nsrc, long src_stride, const void* packed, int cin, int cout,
                            const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                            void* stream);
/* Same conv, and additionally the 2x2/2 SAME max-pool of its output written to ypool
 * ([n, ceil(h/2), ceil(w/2), cout], same dtype) — replaces the conv_layer + max_pool pairs
 * unet.py:170-187 (conv1_2/pool1 ... conv4_3/pool4; max_pool at unet.py:32-33).
 * Only the bf16 patch kernel fuses pooling: other cases return VM_EUNSUPPORTED and the caller runs
 * vm_conv3x3_nhwc + vm_maxpool2x2_same_nhwc instead. */
int vm_conv3x3_pool_nhwc(const vm_tensor* x, const void* packed, int cin, int cout, const float* bias,
                         const float* scale, const float* shift, int act, vm_tensor* y, vm_tensor* ypool,
                         void* stream);

/* cout == 1 head conv, y = act(conv(x, w) + bias ...), and optionally alpha = sigmoid of the pre-activation value
 * (f32, contiguous [n*h*w]) from the same pass — unet.py:203-205 (conv1_5 = self.conv1_3 logits, then
 * tf.nn.sigmoid -> self.output; unet_simple.py:142, small.py:49-50).  alpha may be NULL. */
int vm_conv3x3_head_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias, const float* scale,
                         const float* shift, int act, vm_tensor* y, float* alpha, void* stream);

/* The same cout == 1 head over one channel chunk of its input, adding y_acc (f32, contiguous [n*h*w], e.g. the
 * previous chunk's y) to the pre-activation: a head over more channels than one MFMA head tile holds, chunk by chunk
 * (the split-bf16 x6 path's conv1_5 over 6 x 128 channels, unet.py:203-205).  cin <= 256 (bf16). */
int vm_conv3x3_head_acc_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias, const float* y_acc,
                             vm_tensor* y, float* alpha, void* stream);
/* The same with the per-channel affine of vm_conv3x3_nhwc: pre-activation = (conv + y_acc + bias) * scale + shift
 * (y_acc may be NULL) — the split-fp16 x3 path's conv1_5, whose fp16 filter parts are pre-scaled by a power of two
 * that the last chunk's scale undoes (exactly) before the sigmoid (unet.py:203-205).  x may be VM_F16 (cin <= 256), or a two-slab
 * split-fp16 view [l, h] of 128-channel slabs with cin 384 (read as [l, h, h]; conv1_5 of the f16x3 forward). */
int vm_conv3x3_head_acc_ex_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias, const float* scale,
                                const float* shift, const float* y_acc, vm_tensor* y, float* alpha, void* stream);

/* Two chained convs whose 64-channel intermediate never leaves the chip: y = act2(conv3x3(relu(conv3x3(x, w1) + bias1),
 * w2) + bias2 ...), optionally with the fused 2x2 SAME max-pool of y into ypool (NULL = none) — replaces
 * unet.py:170-172 (conv1_1 -> conv1_2 -> pool1; conv_layer at :65-74) and the VGG towers' first pair
 * (unet_simple.py:60-62).  x: [n,h,w,cin1 <= 8], either a bf16 view whose 8-element pixel row from coff is
 * readable (the channels >= cin1 meet zero weights) or the caller's f32 frame itself (any channel stride; rounded
 * to bf16 on load, which replaces the vm_convert_nhwc pass); packed1 = vm_conv3x3_pack_weights(cin1, 64, bf16),
 * packed2 = (64, cout2, bf16).  bf16 compute only: an f32 y returns VM_EUNSUPPORTED and the caller runs the two
 * convs separately. */
int vm_conv3x3_pair_first_nhwc(const vm_tensor* x, const void* packed1, int cin1, const float* bias1,
                               const void* packed2, int cout2, const float* bias2, const float* scale2,
                               const float* shift2, int act2, vm_tensor* y, vm_tensor* ypool, void* stream);

/* The pair with conv1_1's own output kept too (mid: bf16 [n,h,w,64] view, 16-byte aligned channel chunks) — the
 * training towers (unet_simple.py:60-62), whose select convs read conv1_1 (unet_simple.py:160-168).
 * VM_EUNSUPPORTED when the strip-walking kernel cannot take the case (the caller runs the two convs). */
int vm_conv3x3_pair_first_mid_nhwc(const vm_tensor* x, const void* packed1, int cin1, const float* bias1,
                                   const void* packed2, int cout2, const float* bias2, const float* scale2,
                                   const float* shift2, int act2, vm_tensor* y, vm_tensor* ypool, vm_tensor* mid,
                                   void* stream);

/* The pair kernel with the head split (unet.py:170-172 + 203-205): conv1_5 over cat1 = [up, skip] is linear in
 * its input channels, so the skip half's share is taken where conv1_2's output is made.  Besides y/ypool the pair
 * kernel writes partial[pixel][12] (f32, n*h*w*12 floats): taps 0..8 of sum_c y[pixel][c] * head_w[tap][head_coff+c]
 * (head_w = conv1_5's HWIO f32 filter [3,3,head_cin,1], bf16-rounded like the packed head; 9..11 = 0).  store_y = 0
 * leaves y unwritten (only the pool and the partials leave the chip).  vm_conv3x3_head_partial_nhwc then runs the
 * head over the other channels (x = the up half, packed for that many channels) and adds
 * sum_tap partial[pixel + offset(tap)][tap] (zero outside the frame) before bias / act / alpha. */
int vm_conv3x3_pair_first_head_nhwc(const vm_tensor* x, const void* packed1, int cin1, const float* bias1,
                                    const void* packed2, int cout2, const float* bias2, const float* scale2,
                                    const float* shift2, int act2, vm_tensor* y, vm_tensor* ypool,
                                    const float* head_w, int head_cin, int head_coff, float* partial, int store_y,
                                    void* stream);
int vm_conv3x3_head_partial_nhwc(const vm_tensor* x, const void* packed, int cin, const float* bias,
                                 const float* scale, const float* shift, int act, vm_tensor* y, float* alpha,
                                 const float* partial, void* stream);

/* tf.image.resize_images(x, [2h, 2w]) (TF-1 legacy bilinear, exact 2x) followed by the 3x3 SAME conv, without
 * materialising the resized tensor — unet.py:44-63 (upconv_concat: resize_images at :58, conv2d at :60) for the
 * levels whose skip tensor is exactly twice the input's size.  Bilinear 2x is linear, so every output pixel
 * (2i+a, 2j+b) is a 3x3 conv of the low-res frame at (i, j) with one of four "phase" filters:
 * vm_conv3x3_fold_up2x_weights folds the HWIO f32 filter [3,3,cin,cout] into [3,3,cin,4*cout] (channel
 * p*cout + co = phase p = 2a+b of channel co); pack that with vm_conv3x3_pack_weights(cin, 4*cout) as packed_up
 * and the plain filter as packed.  The frame border (output rows 0 and 2h-1, columns 0 and 2w-1), where the
 * resized image's zero padding breaks the folding, is recomputed from packed the unfused way.
 * x: low-res [n,h,w,cin]; y: [n,2h,2w,cout].  bf16 only (f32 callers use resize + conv3x3: VM_EUNSUPPORTED),
 * cout % 64 == 0, 16-byte aligned channel views.  Numerics: the folded filter is rounded to bf16 instead of the
 * resized activations (same bf16 tolerance class as the unfused path). */
int vm_conv3x3_fold_up2x_weights(const float* w_hwio, int cin, int cout, float* w_up_hwio, void* stream);
int vm_conv3x3_up2x_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin, int cout,
                         const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                         void* stream);

/* The folded upconv with the head split (unet.py:200-205: upconv_4 -> cat1 -> conv1_5): besides y (store_y = 0
 * leaves it unwritten) the conv writes partial[pixel][12] of its [n,2h,2w] output (f32): taps 0..8 of
 * sum_c y[pixel][c] * head_w[tap][head_coff + c] over the conv's bf16 outputs (head_w = conv1_5's HWIO f32 filter
 * [3,3,head_cin,1], bf16-rounded like a packed head; taps 9..11 zero), the frame border included (from the border
 * pass's values).  cout == 64; VM_EUNSUPPORTED when a kernel-selection option rules out the patch kernel's register
 * epilogue (the caller then stores y and runs vm_conv3x3_head_partial_nhwc). */
/* The folded upconv of the split-fp16 x3 path (unet.py:44-63 at f32 accuracy): x is the low-res split input [l, h]
 * (VM_F16, S = x.c / 2 channels per slab, S % 32 == 0), packed_up the fp16 parts [Wh', Wl', Wh'] (cin = 3 S) of the
 * folded filter of vm_conv3x3_fold_up2x_weights (pre-scaled by 2^t), packed the plain filter's parts at the same
 * scale (the border pass: the resize of x = h + l in f32, split again); y = act((conv + bias) * scale + shift) in f32,
 * written split as vm_conv3x3_split3_nhwc writes it ([n, 2h, 2w, cout], cout % 64 == 0, slab y_slab). */
int vm_conv3x3_up2x_split3_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin, int cout,
                                const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                                int y_slab, int* overflow, void* stream);
int vm_conv3x3_up2x_head_nhwc(const vm_tensor* x, const void* packed_up, const void* packed, int cin, int cout,
                              const float* bias, const float* scale, const float* shift, int act, vm_tensor* y,
                              const float* head_w, int head_cin, int head_coff, float* partial, int store_y,
                              void* stream);

/* conv1_5 + sigmoid from two partial sets (unet.py:203-205 with both halves of cat1 taken where they were made,
 * vm_conv3x3_up2x_head_nhwc and vm_conv3x3_pair_first_head_nhwc): logits[p] = bias[0] + sum_tap (pa[p + off(tap)][tap]
 * + pb[p + off(tap)][tap]) (zero outside the frame), alpha[p] = sigmoid(logits[p]).  pa, pb: f32 [n*h*w][12];
 * logits: f32 [n,h,w,1] view or NULL; alpha: contiguous f32 [n*h*w] or NULL. */
int vm_conv3x3_head_from_partials(const float* pa, const float* pb, int n, int h, int w, const float* bias,
                                  vm_tensor* logits, float* alpha, void* stream);

/* tf.nn.max_pool(ksize 2, stride 2, 'SAME') — unet.py:32-33, unet_simple.py:95-96, small.py:40,42 */
int vm_maxpool2x2_same_nhwc(const vm_tensor* x, vm_tensor* y, void* stream);

/* tf.image.resize_images(x, [H, W]) TF-1.x bilinear legacy — unet.py:58, unet_simple.py:33, small.py:17 */
int vm_resize_bilinear_tf1_nhwc(const vm_tensor* x, vm_tensor* y, void* stream);

/* dtype / channel-padding copy with optional per-channel affine and activation
 * (packs the caller's f32 [N,H,W,7] frame into the compute layout; loader.py:76-78 mean/shift
 * can be folded in via shift).  Channels >= x->c of y are zero-filled. */
int vm_convert_nhwc(const vm_tensor* x, vm_tensor* y, const float* scale, const float* shift, int act, void* stream);
/* A HIP stream created with a full CU mask (hipExtStreamCreateWithCUMask), for the trainers' side streams (the
 * filter gradients beside the data-gradient chain, train.py:37-52 / 288-304): a plain stream shares one of the
 * process's hardware queues, possibly the caller's, which serialises the two.  vm_stream_destroy releases it. */
int vm_stream_create_masked(void** stream);
int vm_stream_destroy(void* stream);
/* One wave spinning for `microseconds` of the device wall clock on `stream`: the trainers' probe for a side stream
 * that runs beside theirs (a plain stream may share the caller's hardware queue). */
int vm_spin(int microseconds, void* stream);
/* Split-bf16 x6 operand of an f32 activation (no reference counterpart: the operand format of the split-bf16 conv
 * path, which evaluates unet.py's tf.nn.conv2d (unet.py:39,60,70) at f32 accuracy on bf16 MFMA).  x (f32 view,
 * x.c channels) -> three bf16 parts h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), written as six slabs
 * [l, m, h, m, h, h] at channel p*S + y.coff + c of y (bf16, S = y.cstride / 6; y.c >= x.c, the extra channels 0).
 * A conv over the 6*S channels with the filter parts [h, m, l, h, m, h] stacked along cin is the sum of the six
 * cross products down to 2^-16 of the leading one.  y_pool (optional, same layout at ceil(h/2) x ceil(w/2)): the
 * split of tf.nn.max_pool 2x2 SAME (unet.py:33) of x, from the same pass. */
int vm_split6_nhwc(const vm_tensor* x, vm_tensor* y, vm_tensor* y_pool, void* stream);
/* Split-fp16 x3 operand of an f32 activation (no reference counterpart: the operand format of the split-fp16 conv path,
 * which evaluates unet.py's tf.nn.conv2d (unet.py:39,60,70) at f32 accuracy in three fp16 MFMA products).  x (f32
 * view) -> h = fp16(x), l = fp16(x - h) (RNE; 22 significant bits), written as slabs [l, h] at channel p*S + y.coff + c
 * of y (VM_F16; S = slab, or y.cstride / 2 when slab <= 0; y.c >= x.c, the extra channels 0), and a third slab [h]
 * at 2*S + y.coff + c when the pixel row holds it (3*S <= y.cstride).  A conv over [l, h, h] with the filter parts
 * [Wh, Wl, Wh] stacked along cin is l*Wh + h*Wl + h*Wh; vm_conv3x3_ex_nhwc / split3 read a two-slab view (x.c = 2S,
 * cin = 3S, S % 32 == 0) as [l, h, h], so h is stored once.  y_pool (optional, same layout at ceil(h/2) x ceil(w/2)):
 * the split of tf.nn.max_pool 2x2 SAME (unet.py:33) of x from the same pass.  overflow (device int, may be NULL): set
 * to 1 when some |x| >= 65520 (fp16's range; the split is then invalid). */
int vm_split3h_nhwc(const vm_tensor* x, vm_tensor* y, vm_tensor* y_pool, int slab, int* overflow, void* stream);
/* tf.image.resize_images(x, [y.h, y.w]) TF-1 legacy bilinear (unet.py:58) of an f32 activation, written as its
 * split-fp16 x3 operand (the vm_split3h_nhwc layout of y, slab / overflow as there) without the f32 resized tensor;
 * the same float32 arithmetic as vm_resize_bilinear_tf1_nhwc, so bit-identical to that resize followed by the split.
 * 16-byte aligned views, c % 8 == 0 (the split-fp16 path's upconv_concat inputs, unet.py:44-63). */
int vm_resize_split3h_nhwc(const vm_tensor* x, vm_tensor* y, int slab, int* overflow, void* stream);
/* The split-fp16 x3 conv with the split of its output fused into the epilogue (no f32 round trip): x is an fp16 split
 * input (slabs [l, h] read as [l, h, h], or three stored slabs; cin = 3 x its channels) and packed its fp16 filter
 * parts; y = act((conv + bias) * scale + shift) is computed in f32 as vm_conv3x3_nhwc does, then written split as
 * vm_split3h_nhwc writes it: slabs [l, h] (+ [h] where 3 * y_slab <= y.cstride) of y (VM_F16, cout % 8 == 0 channels
 * at y.coff inside the first slab) at slab distance y_slab (<= 0: y.cstride / 2);
 * ypool (optional, same layout, pool_slab) receives the split of tf.nn.max_pool 2x2 SAME (unet.py:33) of y.  overflow
 * (device int, may be NULL) is set when some |y| >= 65520.  work / work_bytes: vm_conv3x3_workspace_bytes (split-K on
 * small grids; not with ypool). */
int vm_conv3x3_split3_nhwc(const vm_tensor* x, const void* packed, int cin, int cout, const float* bias,
                           const float* scale, const float* shift, int act, vm_tensor* y, int y_slab, vm_tensor* ypool,
                           int pool_slab, int* overflow, void* work, size_t work_bytes, void* stream);

/* tf.contrib.layers.batch_norm(is_training=True): batch mean / biased variance over N,H,W
 * (unet_simple.py:25,41; small.py:22,32).  work: vm_bn_workspace_bytes(x) bytes of device scratch. */
size_t vm_bn_workspace_bytes(const vm_tensor* x);
int vm_bn_stats_nhwc(const vm_tensor* x, float* mean, float* var, void* work, void* stream);
/* y = act((x - mean) * rsqrt(var + eps) * gamma + beta); y may alias x. NULL mean/var = 0/1. */
int vm_bn_apply_nhwc(const vm_tensor* x, vm_tensor* y, const float* mean, const float* var, const float* gamma,
                     const float* beta, float eps, int act, void* stream);

/* tf.nn.softmax over channels — refine.py:31 */
int vm_softmax_lastdim_nhwc(const vm_tensor* x, vm_tensor* y, void* stream);

/* reader.create_composite_image (reader.py:72-79): out = a*fg + (1-a)*bg on channels 0..2 (channels >= 3: bg),
 * over `pixels` pixels of `cn` interleaved channels.  fg/bg: img_dtype VM_U8 / VM_F32 / VM_F64; alpha: one
 * VM_F32 / VM_F64 value per pixel; out: VM_F32 / VM_F64.  Computed in float64 (numpy's promotion), rounded to
 * out_dtype, so a VM_F64 output is bit-identical to the reference's numpy expression. */
int vm_composite_image(const void* fg, const void* bg, int img_dtype, const void* alpha, int alpha_dtype,
                       long pixels, int cn, void* out, int out_dtype, void* stream);

/* flow.warp_img (flow.py:9-18): out[y,x] = bilinear(img, x + flow[y,x,0], y + flow[y,x,1]),
 * cv2.remap INTER_LINEAR / BORDER_CONSTANT 0.  mode 0 = OpenCV 1/32-pixel fixed point, 1 = exact.
 * img [ih,iw] f32, flow [h,w,2] f32, out [h,w] f32.  Batched over `n` frames (contiguous). */
int vm_remap_bilinear_f32(const float* img, int ih, int iw, const float* flow, int h, int w, int n, float* out,
                          int mode, void* stream);
/* flow.warp_bgr (flow.py:21-33): uint8 [ih,iw,cn] HWC, OpenCV 15-bit fixed-point weights. */
int vm_remap_bilinear_u8(const uint8_t* img, int ih, int iw, int cn, const float* flow, int h, int w, uint8_t* out,
                         void* stream);

/* flow.correct_alpha (flow.py:36-65): forward/backward consistency; alpha [h,w] f32 zeroed IN PLACE
 * where the round-trip error > thresh.  promote 0 = numpy-1.x float64 index arithmetic, 1 = numpy-2
 * float32.  *err_flag (device int, zeroed by the caller) is set when an index falls below -dim
 * (the reference's IndexError); the host turns that into VM_EINDEX. */
int vm_fb_consistency(const float* backward, const float* forward, int h, int w, float* alpha, float thresh,
                      int promote, int* err_flag, void* stream);

/* BASELINE config 3 in one pass (flow.py:69-77 chain, refine.py:27 input): per pixel
 *   alpha_w = warp_img(prev_alpha, backward)      (as vm_remap_bilinear_f32 mode 0, flow.py:9-18)
 *   correct_alpha(backward, forward, alpha_w)     (as vm_fb_consistency, flow.py:36-65, threshold thresh)
 *   out[pixel] = [cmp B, G, R, alpha, alpha_w, 0, 0, 0]   (the RefineNet input, Cin 5 padded to 8)
 * prev_alpha / alpha [h,w] f32, backward / forward [h,w,2] f32, cmp [h,w,3] f32 (BGR - VGG_MEAN), out [h,w,8]
 * in out_dtype (VM_F32 or VM_BF16), warped [h,w] f32 or NULL.  *err_flag (zeroed by the caller) is set where
 * the reference raises IndexError; the output is then undefined. */
int vm_temporal_refine_input(const float* prev_alpha, const float* backward, const float* forward, const float* cmp,
                             const float* alpha, int h, int w, float thresh, int promote, void* out, int out_dtype,
                             float* warped, int* err_flag, void* stream);

/* train.py:14-28,42-47 loss: out[0] = mean(0.5*charb(pred,gt) + 0.5*charb(composite(raw_fg,bg,pred), cmp)),
 * out[1] = mean alpha loss, out[2] = mean compositional loss.  pred/gt [n,h,w,1], others [n,h,w,3] f32.
 * work: vm_loss_workspace_bytes(n*h*w) bytes. */
size_t vm_loss_workspace_bytes(long pixels);
int vm_matting_loss(const float* pred, const float* gt, const float* raw_fg, const float* bg, const float* cmp,
                    long pixels, float* out, void* work, void* stream);

/* ---------------------------------------------------------------- training-sample loader
 * Replaces the per-pixel part of loader.py's sample builders after decoding: load_and_crop (loader.py:39-85),
 * simple_load_crop (:119-157), video_load_crop (:285-330) and their batch loops get_batch / simple_batch /
 * video_batch (:93-116, 160-171, 333-345) — get_padded_img canvases (:10-36), crops, flow.warp_img of the
 * previous alpha (:291-293), cv2.resize(INTER_LINEAR) of fg / alpha / warped alpha / bg to the network size
 * (:70-73, 146-148, 316-319), reader.create_composite_image and the VGG_MEAN subtraction (:75-77).
 * The random draws stay on the host (same np.random calls, same order); the host passes their outcome as
 * window maps.  One axis of a padded + cropped source: resize-source index u in [0, n) is canvas index
 * t = u + off; the canvas holds image data on [lo, hi) at image index t + shift, zeros elsewhere. */
typedef struct vm_crop_axis {
  int32_t n, off, lo, hi, shift;
} vm_crop_axis;

typedef struct vm_loader_sample {
  const uint8_t* fg;   /* foreground BGRA u8 [fg_h, fg_w, 4] (reader.read_fg_img: BGR + alpha), 4-byte aligned */
  const uint8_t* prev; /* previous frame BGRA u8 [prev_h, prev_w, 4] (its alpha is warped) or NULL */
  const float* flow;   /* backward flow f32 [fg_h, fg_w, 2] (reader.read_flow), 8-byte aligned, or NULL */
  const uint8_t* bg;   /* background BGR u8 [bg_h, bg_w, 3] (cv2.imread) */
  int32_t fg_h, fg_w, prev_h, prev_w, bg_h, bg_w;
  vm_crop_axis fg_rows, fg_cols, bg_rows, bg_cols;
  int32_t mirror;      /* get_batch rd_mirror: flip this sample's outputs left-right (loader.py:105-109) */
  int32_t reserved;
} vm_loader_sample;

enum vm_loader_plane { VM_LOADER_CMP = 0, VM_LOADER_BG = 1, VM_LOADER_LABEL = 2, VM_LOADER_WARPED = 3,
                       VM_LOADER_FG = 4 };

/* Output planes [n, out_h, out_w, *] (NULL = not produced); element (i, y, x, k) of plane p is at
 * ptr[p][((i*out_h + y)*out_w + x)*pixstride[p] + k].  cmp, bg: 3 channels, mean-subtracted; label: 1 channel
 * (alpha); warped: 3 identical channels (loader.py:293); fg: 3 channels, the resized raw foreground. */
typedef struct vm_loader_outputs {
  void* ptr[5];
  int32_t pixstride[5];
  int32_t reserved;
} vm_loader_outputs;

/* samples: HOST array of n descriptors whose image pointers are device pointers; validated, then uploaded into
 * work (device, vm_loader_workspace_bytes(n) bytes) on `stream`.  dtype VM_F32 or VM_F64 (float64 = the
 * reference's values bit for bit).  Output size (out_h, out_w) = (input_size[1], input_size[0]). */
size_t vm_loader_workspace_bytes(int n);
int vm_loader_compose(const vm_loader_sample* samples, int n, int out_h, int out_w, int dtype,
                      const vm_loader_outputs* out, void* work, void* stream);

/* ---------------------------------------------------------------- augmentation
 * tps.py (thin-plate-spline warp) and augmentation.py (augment's per-pixel work).  The TPS coefficient solve
 * (tps._make_warp's 28x28 pinv, tps.py:110-115) and the np.random draws stay on the host, as in the reference;
 * the per-pixel evaluation, resampling and colour work run here. */

/* tps._make_inverse_warp's grid evaluation (tps.py:41-51 with tps._calculate_f, tps.py:100-108):
 * grid[c][i][j] = a1_c + ax_c*x_i + ay_c*y_j + sum_k w_kc * U(|(x_i, y_j) - P_k|), U(r) = (r*r)*log(r) (0 below
 * 1e-100, tps.py:80-81), x_i = i*x_step + x_lo, y_j = j*y_step + y_lo (np.mgrid).  points [npts,2] and coeffs
 * [npts+3,2] (w_k rows, then a1, ax, ay) are DEVICE f64; grid is DEVICE f64 [2, nx, ny]. */
int vm_tps_grid(const double* points, const double* coeffs, int npts, int nx, int ny, double x_lo, double x_step,
                double y_lo, double y_step, double* grid, void* stream);

/* The inverse map tps.warp_images samples with.  upsample = 0 (approximate_grid == 1): the grid is the map and the
 * output is nx x ny.  upsample = 1: the output is (x_span+1) x (y_span+1) (x_span = x_max - x_min) and each pixel's
 * map is the bilinear upsampling of tps.py:55-74 with x_steps = (x_max - x_min) / approximate_grid. */
typedef struct vm_tps_map {
  const double* grid;
  int32_t nx, ny;
  int32_t upsample;
  int32_t x_span, y_span;
  int32_t reserved;
  double x_steps, y_steps;
} vm_tps_map;

/* tps.warp_images' resampling (tps.py:34): scipy.ndimage.map_coordinates(plane, map, order) with mode 'constant'
 * (cval 0) on `cn` interleaved planes.  img [ih, iw, cn] and out [oh, ow, cn] of dtype VM_U8 / VM_F32 / VM_F64
 * (integer outputs round as scipy does: (type)(t + 0.5)).  order 0 or 1. */
int vm_tps_sample(const vm_tps_map* map, const void* img, int ih, int iw, int cn, int dtype, int order, void* out,
                  void* stream);

/* cv2.warpAffine(src, M, (w, h)) with INTER_LINEAR, BORDER_CONSTANT 0 (augmentation.py:58-61): m is the FORWARD
 * 2x3 matrix (HOST, 6 doubles), inverted in double as warpAffine does.  src [ih, iw, cn], dst [h, w, cn], dtype
 * VM_U8 (15-bit fixed-point weights), VM_F32 or VM_F64 (float table weights). */
int vm_warp_affine(const void* src, int ih, int iw, int cn, int dtype, const double* m, void* dst, int h, int w,
                   void* stream);
/* augmentation.warp_image without its TPS part (augmentation.py:59-63): cv2.warpAffine by the integer translation
 * [[1,0,tu],[0,1,tv]] to (w, h), then cv2.warpAffine by m (the forward getRotationMatrix2D, inverted as warpAffine
 * does) to (w, h) — fused into one pass, bit-identical to the two vm_warp_affine calls (the translation's fixed-point
 * fraction is zero, so its output is src shifted with zero fill).  lut (optional, u8 BGR only): then
 * change_illumination (augmentation.py:86-98, 133-134) with that S/V map, as vm_change_illumination_u8. */
int vm_warp_image(const void* src, int ih, int iw, int cn, int dtype, int tu, int tv, const double* m,
                  const uint8_t* lut, void* dst, int h, int w, void* stream);

/* augmentation.change_illumination (augmentation.py:86-98): cvtColor BGR2HSV (uint8, hrange 180), S and V through
 * lut (HOST, 256 bytes: lut[u] = uint8(255 * clip(a * (u/255.)**b + c, 0, 1)), built by the caller with the
 * reference's float64 arithmetic), cvtColor HSV2BGR.  bgr / out: device uint8 [pixels, 3]. */
int vm_change_illumination_u8(const uint8_t* bgr, long pixels, const uint8_t* lut, uint8_t* out, void* stream);

/* augmentation.object_size / fg_center (augmentation.py:10-20): stats (device int64[3]) = number of nonzero
 * alpha pixels, sum of their row indices, sum of their column indices.  alpha [h, w] VM_F64 / VM_F32 / VM_U8. */
int vm_nonzero_stats(const void* alpha, int h, int w, int dtype, long long* stats, void* stream);

/* augmentation.augmentation's BGRA frame (augmentation.py:154-155, 162-163): out[p] = [fg B, G, R,
 * uint8(255. * alpha[p])] (the product in the alpha's precision, f64 / f32, truncated like numpy's astype). */
int vm_bgra_u8(const uint8_t* fg, const void* alpha, int alpha_dtype, long pixels, uint8_t* out, void* stream);

/* augmentation.augment (augmentation.py:101-135) for a batch of samples in four launches per 4 samples (the
 * config-5 pipeline, vmatting.augmentation.augment_many): per sample the TPS lattice of tps._make_inverse_warp
 * (output region (0, 0, h, w), approximate_grid 2), ONE resampling pass for the fg planes and the alpha through its
 * upsampled map (tps.warp_images, order 1), the fused translate + similarity warps (vm_warp_image) of the background
 * (its own size, camera motion) and of the resampled fg / alpha (object motion), and change_illumination with the
 * sample's S/V map on fg and bg (the fg and alpha object-motion warps share one pass, which can also write the
 * BGRA frame).  Bit-identical to the per-sample entry points.  The np.random draws, the TPS solve
 * and the maps stay on the host (the caller's), as in vm_tps_grid / vm_warp_image. */
typedef struct vm_augment_job {
  const uint8_t* fg;        /* [h, w, 3] u8 BGR (device) */
  const uint8_t* bg;        /* [bg_h, bg_w, 3] u8 BGR */
  const double* alpha;      /* [h, w] f64 */
  const double* tps_points; /* [npts, 2] f64 (device): the deformed landmarks, the reverse map's from-points */
  const double* tps_coeffs; /* [npts + 3, 2] f64 (device): their solve, tps._make_warp (pinv(L) @ [landmarks; 0]) */
  void* scratch;            /* vm_augment_scratch_bytes(h, w) device bytes (lattice, resampled fg and alpha) */
  uint8_t* new_fg;          /* [h, w, 3] u8 */
  uint8_t* new_bg;          /* [bg_h, bg_w, 3] u8 */
  double* new_alpha;        /* [h, w] f64 */
  uint8_t* new_bgra;        /* optional [h, w, 4] u8: the augmented frame as augmentation.augmentation writes it
                             * (augmentation.py:162-163, vm_bgra_u8 of new_fg and new_alpha); NULL: not written */
  int32_t h, w, bg_h, bg_w, npts;
  int32_t tu_bg, tv_bg, tu_fg, tv_fg;
  int32_t reserved;
  double m_bg[6];           /* the forward getRotationMatrix2D matrices (host values), inverted as warpAffine does */
  double m_fg[6];
  uint8_t lut[256];         /* change_illumination's S/V map (augmentation.py:89-95), shared by fg and bg */
} vm_augment_job;
size_t vm_augment_scratch_bytes(int h, int w);
int vm_augment_batch(const vm_augment_job* jobs, int n, void* stream);

/* vm_bgra_u8 for n (fg u8 [px, 3], f64 alpha [px]) pairs (host arrays of device pointers) in one launch per 8. */
int vm_bgra_u8_batch(const uint8_t* const* fg, const double* const* alpha, const long* pixels, uint8_t* const* out,
                     int n, void* stream);

/* vm_nonzero_stats for n f64 alphas (host arrays of device pointers and sizes) in one launch per 8: stats is device
 * int64 [n][3] (count, row-index sum, column-index sum per alpha). */
int vm_nonzero_stats_batch(const double* const* alphas, const int* h, const int* w, int n, long long* stats,
                           void* stream);

/* data.trimap_from_matte (data.py:37-67; the reference uses dilate 1, crop 3): trimap u8 [h, w] from a float64
 * matte [h, w] (device), 255 / 0 where the matte is exactly 1 / 0, 128 elsewhere and — reproducing the reference's
 * raster-order overwrites — on 1-pixels (0-pixels) with a non-0/1 pixel later in raster order within crop (dilate)
 * in the max-norm.  dilate, crop <= 8. */
int vm_trimap_from_matte(const double* matte, int h, int w, int dilate, int crop, uint8_t* trimap, void* stream);

/* ---------------------------------------------------------------- training step (config 5)
 * Backward of train.py's loss through UNetSimple's trainable layers and tf.train.AdamOptimizer
 * (train.py:288-343 video_procedure, 176-227 simple_procedure; unet_simple.py:19-42,116-142).  Gradients are f32;
 * forward activations (x, y views) may be f32 or bf16. */

/* dL/dlogits for alpha = sigmoid(logits) (unet_simple.py:142) under train.py:294-298's loss
 * (regular_l1 train.py:21-28, composite :14-18); pred/gt [P], raw_fg/bg/cmp [P,3] f32 device; dlogits [P]. */
int vm_matting_loss_backward(const float* pred, const float* gt, const float* raw_fg, const float* bg, const float* cmp,
                             long pixels, float* dlogits, void* stream);

/* Workspace of vm_bn_backward_nhwc for a c-channel view. */
size_t vm_bn_backward_workspace_bytes(int channels);

/* Gradient of tf.contrib.layers.batch_norm(is_training=True) (unet_simple.py:25,41) w.r.t. its input x, gamma and
 * beta, given dy (f32) = dL/d(BN output); y (optional) = the relu output that followed the BN (unet_simple.py:120-141:
 * tf.nn.relu(new_conv(...))), so g = dy * (y > 0).  mean/var: the batch statistics the forward normalised with.
 * x == NULL: only dbeta = sum(g) (a bias gradient: the channel sum of dy).  dx / dgamma / dbeta may be NULL. */
int vm_bn_backward_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* y, const float* mean,
                        const float* var, const float* gamma, float eps, vm_tensor* dx, float* dgamma, float* dbeta,
                        void* work, void* stream);
/* The same with dx2 (optional, may be NULL): a second copy of dx in dx2's dtype (the bf16 operand of the
 * data-gradient conv in the bf16 training path, written in the same pass); dbias (optional, needs x): the
 * gradient of a bias added before the BN (new_conv's conv bias, unet_simple.py:23-25) = sum of dx over the
 * pixels, from the same double sums (zero in exact arithmetic). */
int vm_bn_backward_ex_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* y, const float* mean,
                           const float* var, const float* gamma, float eps, vm_tensor* dx, vm_tensor* dx2,
                           float* dgamma, float* dbeta, float* dbias, void* work, void* stream);

/* The input-gradient pass of vm_bn_backward_ex_nhwc alone, with the two channel sums given: sum_g = sum(g),
 * sum_gx = sum(g * xhat) over `count` pixels.  SyncBN (DDP with statistics over the global batch, the single-device
 * reference's unet_simple.py:25,41 normalisation): each replica takes its local sums (vm_bn_backward_ex_nhwc with
 * dx NULL), all-reduces them, and applies them here with count = all replicas' pixels. */
int vm_bn_backward_apply_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* y, const float* mean,
                              const float* var, const float* gamma, float eps, const float* sum_g,
                              const float* sum_gx, long count, vm_tensor* dx, vm_tensor* dx2, void* stream);

/* tf.nn.relu gradient: dx = dy * (y > 0); dx f32. */
int vm_relu_backward_nhwc(const vm_tensor* dy, const vm_tensor* y, vm_tensor* dx, void* stream);
/* The same with an optional second (e.g. bf16) copy of dx. */
int vm_relu_backward_ex_nhwc(const vm_tensor* dy, const vm_tensor* y, vm_tensor* dx, vm_tensor* dx2, void* stream);
/* The same over a decoder level's concat in one pass (upconv_concat, unet_simple.py:30-42): channels [0, split) of
 * the gradient go to dx_lo [n,h,w,split] (f32: the select convs' already-masked gradients, read densely by their
 * BN backward), channels [split, c) to dx [n,h,w,c-split] and optionally dx2 (the upconv's).  0 < split < c, or
 * split 0 with dx_lo NULL (= vm_relu_backward_ex_nhwc). */
int vm_relu_backward_split_nhwc(const vm_tensor* dy, const vm_tensor* y, int split, vm_tensor* dx_lo, vm_tensor* dx,
                                vm_tensor* dx2, void* stream);

/* Adjoint of vm_maxpool2x2_same_nhwc (tf.nn.max_pool 2x2/2 SAME: small.py:40,42; unet.py:32-33): x is the pool's
 * input [n,h,w,c] (any dtype), dy its output gradient [n,ceil(h/2),ceil(w/2),c]; dx [n,h,w,c] (f32 or bf16)
 * = add + the window gradient at the window's first maximum in row-major order (TF MaxPoolGrad's tie rule), 0
 * elsewhere.  add (optional, may alias dx): a gradient reaching x by another path (small.py:20's skip concat). */
int vm_maxpool2x2_backward_nhwc(const vm_tensor* x, const vm_tensor* dy, const vm_tensor* add, vm_tensor* dx,
                                void* stream);

/* The front end of a relu conv's backward (train.py training_procedure through unet.py's y = relu(conv(x) + b),
 * :35-42,65-74): dz = (y > 0) * g written as dz (e.g. the bf16 copy the filter / data-gradient convs read) and the
 * bias gradient dbias[c] = sum_p dz (f64 partials, fixed-order fold) from one pass.  g = dy (+ add) when dy is y's
 * shape; when dy is the 2x2 SAME pool's shape, g = add (optional) + tf.nn.max_pool's adjoint of dy (the window's
 * first maximum of y in row-major order, TF MaxPoolGrad) — the skip half of an [up, skip] concat (unet.py:62) and its
 * pool in one pass.  dy / add f32; y any dtype; work = vm_relu_backward_bias_workspace_bytes(c). */
size_t vm_relu_backward_bias_workspace_bytes(int channels);
int vm_relu_backward_bias_nhwc(const vm_tensor* dy, const vm_tensor* y, const vm_tensor* add, vm_tensor* dz,
                               float* dbias, void* work, void* stream);

/* Adjoint of vm_resize_bilinear_tf1_nhwc (tf.image.resize_images, unet_simple.py:33): dy [n,oh,ow,c] (f32 or bf16
 * view) -> dx contiguous f32 [n,ih,iw,c] (overwritten). */
int vm_resize_bilinear_tf1_backward(const vm_tensor* dy, float* dx, int ih, int iw, void* stream);
/* The same with dx a dense view [n,ih,iw,c]: f32, or bf16 (c % 4 == 0; each f32 sum rounded once to nearest even). */
int vm_resize_bilinear_tf1_backward_nhwc(const vm_tensor* dy, vm_tensor* dx, void* stream);

/* Workspace of vm_conv3x3_wgrad_nhwc (per-block partial filter gradients, <= 64 MiB). */
size_t vm_conv3x3_wgrad_workspace_bytes(int n, int h, int w, int cin, int cout);

/* Weight gradient of the 3x3 SAME conv (tf.nn.conv2d, unet_simple.py:23,35): dw[3][3][cin][cout] (HWIO, f32) +=
 * sum over pixels of x (view, cin = x->c) patch x dy (f32 view [n,h,w,cout]); cout <= 48.  Accumulates;
 * deterministic (fixed-order two-pass sum through ``work``). */
int vm_conv3x3_wgrad_nhwc(const vm_tensor* x, const vm_tensor* dy, float* dw, void* work, void* stream);
/* The weight gradient with options: x_src_c > 0 reads x as x->c / x_src_c sources of x_src_c channels each,
 * source s at x_src_stride elements from the view base (the frozen towers' features stored tower-major,
 * unet_simple.py:153-168's concat); mode 0 = the exact-f32 FMA kernel above, mode 1 = MFMA with bf16 operands
 * (x a bf16 view of 16-byte channel chunks, dy rounded to bf16 on load, f32 sums; the bf16 training path).
 * cout <= 48; dw += result; work: vm_conv3x3_wgrad_ex_workspace_bytes(..., mode) bytes. */
size_t vm_conv3x3_wgrad_ex_workspace_bytes(int n, int h, int w, int cin, int cout, int mode);
int vm_conv3x3_wgrad_ex_nhwc(const vm_tensor* x, int x_src_c, long x_src_stride, const vm_tensor* dy, float* dw,
                             void* work, int mode, void* stream);

/* The data-gradient filter of a 3x3 SAME conv: w_flipped[kh][kw][co][ci] = w[2-kh][2-kw][ci][co]; dx is then
 * vm_conv3x3_nhwc(dy, pack(w_flipped)). */
int vm_conv3x3_flip_weights(const float* w_hwio, int cin, int cout, float* w_flipped, void* stream);

/* tf.train.AdamOptimizer's ApplyAdam (train.py:302-304) over n f32 values, g = grad * grad_scale:
 * m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); var -= m * lr_t / (sqrt(v) + eps), with the caller's
 * lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t). */
int vm_adam_tf(float* var, float* m, float* v, const float* grad, long n, float lr_t, float beta1, float beta2,
               float eps, float grad_scale, void* stream);

/* ---------------------------------------------------------------- inference on a decoded clip
 * The network input from decoded uint8 frames in one pass (the reference's inference feed, loader.py:45,75-78):
 *   cmp     uint8 [n,h,w,3] BGR composite, bg uint8 [nb,h,w,3] BGR background with nb == n, or nb == 1 for one
 *           static plate shared by every frame, trimap uint8 [n,h,w] or NULL
 *   out     view [n,h,w,C], C = 7 with a trimap (UNetVideo) or 6 without (UNetImage); n, h, w are read from it
 * out channel c < 3 = f32((double)cmp - VGG_MEAN[c]), 3 + c the same of bg, VGG_MEAN = (103.939, 116.779, 123.68);
 * channel 6 = f32((double)trimap / 255.0 - 0.5): the float64 subtraction rounded to f32 once, as the reference feeds
 * it.  out dtype VM_F32 (any channel offset / stride) or VM_BF16: the round-to-nearest-even bf16 of those f32 values
 * in 16-byte aligned 8-channel pixels (coff 0, cstride 8; channels C..7 are written as zero), which is the bf16 frame
 * vm_conv3x3_pair_first*_nhwc reads.  4 pixels per thread (dword loads, 16-byte stores) when the planes are 4-byte
 * aligned and the f32 view is dense, else one pixel per thread.  No TF counterpart (feed_dict preprocessing). */
int vm_frames_from_u8(const uint8_t* cmp, const uint8_t* bg, const uint8_t* trimap, int nb, vm_tensor* out,
                      void* stream);

/* alpha f32 [pixels] -> 8- or 16-bit matte: q = (T)min(max(rintf(alpha * M), 0), M), M = 255.f (bits 8, uint8 out) or
 * 65535.f (bits 16, uint16 out); f32 product, ties to even, NaN -> 0. */
int vm_matte_quantize(const float* alpha, long pixels, int bits, void* out, void* stream);

/* The matte applied.  The composite is C = a F + (1 - a) B and the background B is known (it is a model input), so
 * the foreground layer and the frame over another plate N, C + (1 - a)(N - B), follow per pixel.
 *   alpha f32 [n,h,w]; cmp uint8 [n,h,w,3] BGR; bg uint8 [nb,h,w,3], nb == n or 1 (one static plate)
 *   mode VM_COMPOSE_OVER: out uint8 [n,h,w,3] BGR, new_bg uint8 [nn,h,w,3] required, nn == n or 1
 *   mode VM_COMPOSE_STRAIGHT, VM_COMPOSE_PREMUL: out uint8 [n,h,w,4] BGRA, new_bg NULL and nn 0
 * Arithmetic, all float64, nothing contracted, one rounding at the end: fin(v) = (uint8) rint(min(max(v, 0), 255)),
 * ties to even; q = the 8-bit matte of vm_matte_quantize; c, b, nw the bytes of cmp, bg, new_bg, per BGR channel:
 *   OVER      a = (double)alpha clamped to [0,1], NaN -> 0;  out = fin(c + (1 - a) * (nw - b))
 *   PREMUL    out = fin(c - ((255 - q) * b) / 255), A = q: the layer a F with a = q / 255, the stored alpha
 *   STRAIGHT  q == 0: B = G = R = 0; else out = fin(b + ((c - b) * 255) / q), A = q (the reference's foreground
 *             files: data.create_bgra, reader.read_fg_img)
 * (255 - q) b and (c - b) 255 are exact, so each layer value has one rounding division.  Traffic per pixel: 4 B alpha
 * + 3 B cmp + 3 B bg read (a static plate is re-read from cache), + 3 B new plate for OVER, 3 or 4 B written: 13 - 16
 * B, HBM-bound.  4 pixels per thread (one 16-byte alpha load, 3 dwords per uint8 plane, one 16-byte BGRA or three
 * dword BGR stores) when alpha is 16-byte, the uint8 planes 4-byte, a BGRA out 16-byte and a BGR out 4-byte aligned;
 * else one pixel per thread.  No TF counterpart (the reference composites forward only, reader.py:72-79). */
#define VM_COMPOSE_OVER 0
#define VM_COMPOSE_STRAIGHT 1
#define VM_COMPOSE_PREMUL 2
int vm_matte_compose(const float* alpha, const uint8_t* cmp, const uint8_t* bg, int nb, const uint8_t* new_bg, int nn,
                     int n, int h, int w, int mode, uint8_t* out, void* stream);

/* The video model's feed in one pass: everything UNetSimple reads for the recurrence of train.py:346-366 at inference,
 *   alpha[t] = create_model(cmp[t], bg[t], warp_img(alpha[t-1], backward[t]), phase False)   (unet_simple.py:148-152),
 * from a decoded clip.  n, h, w are read from `cat`.
 *   cmp        uint8 [n,h,w,3] BGR; bg uint8 [nb,h,w,3], nb == n or nb == 1 (one static plate); values
 *              f32((double)u - VGG_MEAN[c]) as vm_frames_from_u8
 *   prev_alpha f32 [n,h,w], backward f32 [n,h,w,2]: a = warp_img(prev_alpha, backward), bit-identical to
 *              vm_remap_bilinear_f32 mode 0
 *   forward    f32 [n,h,w,2] or NULL; when given, correct_alpha(backward, forward, a) per frame, bit-identical to
 *              vm_fb_consistency (thresh, promote 0 / 1); *err_flag (device int, zeroed by the caller, required with
 *              forward) is set where the reference raises IndexError, and the output is then undefined
 *   towers     view [3n,h,w,3], VM_BF16 or VM_F32, cstride 8, coff 0, 16-byte aligned: frame t*n + i is tower t of
 *              frame i; tower 0 = cmp, 1 = bg, 2 = [a, a, a]; channels 3..7 are written as zero
 *   cat        view [n,h,w,9] of the same dtype, coff 0, cstride >= 16, 16-byte aligned pixels: channels 0..8 =
 *              [cmp B,G,R, bg B,G,R, a, a, a], channels 9..15 are written as zero, channels from 16 on are not touched
 *   warped     f32 [n,h,w] receiving a, or NULL (it must not alias prev_alpha)
 * bf16 values are the round-to-nearest-even of the f32 values (what vm_convert_nhwc writes).  One pixel per thread:
 * every output pixel is whole 16-byte stores, adjacent lanes write adjacent pixels, and the uint8 planes need no
 * alignment.  No TF counterpart (feed_dict preprocessing + the loader's warp). */
int vm_clip_feed(const uint8_t* cmp, const uint8_t* bg, int nb, const float* prev_alpha, const float* backward,
                 const float* forward, float thresh, int promote, vm_tensor* towers, vm_tensor* cat, float* warped,
                 int* err_flag, void* stream);

/* ---------------------------------------------------------------- dense two-frame optical flow
 * The flow vm_clip_feed consumes, estimated from two decoded frames instead of read from .flo files (the reference
 * computes none: no counterpart there).  estimate(cur, prev) = f with cur(x, y) ~ prev(x + f[..,0], y + f[..,1]): the
 * "backward" flow of a frame into the one before it, reader.read_flow layout; the forward flow is estimate(prev, cur).
 * Coarse-to-fine Horn-Schunck with warping and Jacobi sweeps, all f32, nothing contracted, in exactly this order:
 *   grey      g = f32(29 B + 150 G + 77 R) / 256.f
 *   pyramid   level 0 = g; level k+1 = ((a00 + a01) + (a10 + a11)) * 0.25f over 2x2 of level k, ceil sizes, the last
 *             row / column replicated; a level is added while fewer than `levels` exist and min(h_k, w_k) / 2 >= 8
 *   smooth    afterwards each level once by [1/4 1/2 1/4], horizontally r = (l + r) * 0.25f + c * 0.5f, then vertically
 *             the same on the result, replicate borders (levels are built from the unsmoothed level below)
 *   bilinear  x clamped to [0, w-1], y to [0, h-1]; x0 = floor, x1 = min(x0 + 1, w - 1); top = p00 + fx * (p01 - p00),
 *             bot likewise, top + fy * (bot - top)
 *   level     flow = 0 at the coarsest, else 2.f * bilinear(coarser flow, ((x - 0.5f) * 0.5f, (y - 0.5f) * 0.5f))
 *   warp      `warps` times per level, (u0, v0) the flow at its start: Iw = bilinear(prev_k, (x + u0, y + v0));
 *             Ix, Iy = (next - previous) * 0.5f of Iw, replicate borders; It = Iw - cur_k;
 *             den = (alpha * alpha + Ix * Ix) + Iy * Iy
 *   sweep     `iters` times per warp, Jacobi (u and v both from the previous iterate, replicate borders):
 *             ub = ((up + down) + (left + right)) * (1 / 6.f) + ((ul + ur) + (dl + dr)) * (1 / 12.f), vb likewise;
 *             r = (Ix * (ub - u0) + Iy * (vb - v0)) + It; q = r / den; u = ub - Ix * q, v = vb - Iy * q
 * tests/flow_est_ref.py restates this in numpy; the kernels match it bit for bit.  The sweeps run FT = 4 per launch
 * on LDS tiles (csrc/flow_est.hip; vm_set_option "flow_blocked" 0: one sweep per launch, the same bits).
 *   cur, prev  uint8 [h,w,3] BGR;  flow f32 [h,w,2], 8-byte aligned
 *   work       vm_flow_estimate_workspace_bytes(h, w, levels) bytes, 16-byte aligned
 * No allocation and no synchronisation inside: the calls can be captured in a graph.  VM_EINVAL for NULL pointers,
 * h or w < 16, levels / warps / iters < 1, alpha <= 0 or NaN (checked before any HIP call); the size queries return 0
 * for such shapes.
 * The split form shares work between calls: vm_flow_pyramid writes one frame's smoothed levels (vm_flow_pyramid_bytes,
 * 16-byte aligned; the levels' order and offsets are the library's own) and vm_flow_from_pyramids estimates from two
 * of them; both take the same workspace as vm_flow_estimate, which is vm_flow_pyramid twice and then
 * vm_flow_from_pyramids.  The two directions of one frame pair share both pyramids, consecutive pairs share one. */
size_t vm_flow_estimate_workspace_bytes(int h, int w, int levels);
int vm_flow_estimate(const uint8_t* cur, const uint8_t* prev, int h, int w, int levels, int warps, int iters,
                     float alpha, float* flow, void* work, void* stream);
size_t vm_flow_pyramid_bytes(int h, int w, int levels);
int vm_flow_pyramid(const uint8_t* frame, int h, int w, int levels, float* pyr, void* work, void* stream);
int vm_flow_from_pyramids(const float* cur, const float* prev, int h, int w, int levels, int warps, int iters,
                          float alpha, float* flow, void* work, void* stream);

/* ---------------------------------------------------------------- trimap propagation by optical flow
 * One key-frame trimap carried along a clip by the flows vm_clip_feed consumes (the reference takes a trimap per frame
 * and propagates none: no counterpart there).  propagate(prev, flow, grow) = out:
 *   prev  uint8 [h,w]: 255 is foreground, 0 background, every other value unknown
 *   flow  f32 [h,w,2], reader.read_flow layout, 8-byte aligned: the backward flow of the new frame
 *   out   uint8 [h,w], only the values 0, 128, 255; it must not be prev
 * For output pixel (x, y): xs = f32(x) + flow[y,x,0], ys = f32(y) + flow[y,x,1] (one f32 add each).  Unless
 * 0 <= xs <= w - 1 and 0 <= ys <= h - 1 (so also for NaN and infinities) out = 128.  Else x0 = floor(xs),
 * x1 = x0 + (xs > x0), y0 and y1 likewise: the pixels the bilinear warp touches (one for an integer target, so a zero
 * flow is the identity).  Over the window of rows y0 - grow .. y1 + grow and columns x0 - grow .. x1 + grow, clipped to
 * the image: out = 255 if every pixel of prev in it is foreground, 0 if every one is background, 128 otherwise.  A label
 * survives only where the warp is unambiguous, and grow (0..8) widens the unknown band by that many pixels per step to
 * absorb flow error.  tests/trimap_prop_ref.py restates this in numpy; the kernels match it byte for byte.
 * Two launches (csrc/trimap_prop.hip): a class map of prev into `work` (per pixel whether its (2 grow + 1)^2 window is
 * all foreground / all background, as bit rows: 0.25 B per pixel; skipped for grow == 0), then a gather that reads 8 B
 * of flow and writes 1 B per pixel.
 *   work  vm_trimap_propagate_workspace_bytes(h, w, grow) bytes, 16-byte aligned; 0 bytes for grow == 0, and then
 *         work may be NULL
 * No allocation and no synchronisation inside: the call can be captured in a graph.  VM_EINVAL for h or w < 1 (or
 * h * w beyond 2^31 - 4097), grow outside 0..8, a NULL pointer, out == prev or a misaligned flow / work (checked before
 * any HIP call); the size query returns 0 for such arguments. */
size_t vm_trimap_propagate_workspace_bytes(int h, int w, int grow);
int vm_trimap_propagate(const uint8_t* prev, const float* flow, int h, int w, int grow, uint8_t* out, void* work,
                        void* stream);

/* ---------------------------------------------------------------- trimaps from the background plate
 * The background is a model input, so a trimap can be derived from the frame's difference to it instead of painted
 * (the reference derives its trimaps from ground-truth mattes, data.trimap_from_matte: a certain core plus a narrow
 * unknown band; no counterpart for inference).  trimap_from_plate(cmp, bg, lo, hi, r_bg, r_fg) = out, per frame, all
 * integer:
 *   cmp   uint8 [n,h,w,3] BGR; bg uint8 [nb,h,w,3], nb == n or nb == 1 (one static plate), as vm_frames_from_u8
 *   d     d(x, y) = sum over c of (cmp_c - bg_c)^2, int32
 *   D     D(x, y) = the sum of d over the 3 x 3 neighbourhood, coordinates clamped to the image (replicated border,
 *         always 9 terms)
 *   B0    D <= 9 lo^2;  F0: D >= 9 hi^2.  lo and hi are colour distances in levels, 0 <= lo < hi <= 442 (both bounds
 *         fit int32; 3 * 255^2 < 442^2)
 *   B     B(x, y) holds when every pixel of the (2 r_bg + 1)^2 window around it, clipped to the image, is in B0; F the
 *         same with r_fg and F0.  Pixels outside the image do not erode.  Radii 0..32
 *   out   uint8 [n,h,w]: 255 where F, 0 where B, 128 elsewhere (lo < hi: the two exclude each other); it must not
 *         overlap cmp or bg
 * What this is not: it has no shadow or exposure model (a shadow on the plate or a gain change is a difference like
 * any other; vm_trimap_from_plate_shadow below tolerates cast shadows, and vm_plate_gain_fit / vm_plate_gain_apply
 * further down match the plate's exposure to the frame before this call).  It cannot tell a translucent high-contrast pixel from an opaque one, so r_fg must exceed the width of
 * the soft edge.  Foreground that matches the plate over an area wider than 2 r_bg + 1 is labelled background.
 * tests/trimap_plate_ref.py restates the definition in numpy; the kernels match it byte for byte.
 * Two launches for all n frames (csrc/trimap_plate.hip): the candidates B0 and F0 as bit rows into `work` (0.25 B per
 * pixel), then the two erosions and the result bytes.
 *   work  vm_trimap_from_plate_workspace_bytes(n, h, w) bytes, 16-byte aligned
 * No allocation, no atomics and no synchronisation inside: the call can be captured in a graph.  VM_EINVAL for a NULL
 * pointer, n, h or w < 1 (or n * h * w beyond 2^31 - 1), nb not 1 or n, lo / hi / a radius out of range or lo >= hi,
 * out overlapping cmp or bg, or a misaligned work (checked before any HIP call); the size query returns 0 for such
 * shapes. */
size_t vm_trimap_from_plate_workspace_bytes(int n, int h, int w);
int vm_trimap_from_plate(const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int lo, int hi, int r_bg,
                         int r_fg, uint8_t* out, void* work, void* stream);

/* The same trimap with a distance that tolerates cast shadows: the brightness / chromaticity split of Horprasert et
 * al. (1999).  A shadowed background pixel is the plate's colour scaled by a factor below 1, so where the frame's
 * pixel lies close to the line through the plate's colour, and the factor is one a shadow may have, the distance to
 * that line replaces the distance to the plate itself.  trimap_from_plate_shadow(cmp, bg, lo, hi, r_bg, r_fg, floor,
 * ceil, dark) = out is trimap_from_plate with d' in place of d; per pixel, with I = cmp's three bytes and E = bg's, all
 * integer:
 *   d         sum over c of (I_c - E_c)^2, as above
 *   ee, ie, ii   sum over c of E_c^2, of I_c E_c, of I_c^2
 *   cross     ii ee - ie^2: >= 0 (Cauchy-Schwarz), up to about 3.8e10, so 64 bits
 *   in range  ee >= max(3 dark^2, 1)  and  floor ee <= 256 ie <= ceil ee
 *   d'        cross / ee rounded down where in range, d elsewhere.  cross / ee is the squared distance of I from the
 *             line through E, so d' <= d everywhere
 *   floor     1..256: the least share of the light, in 1/256, that a shadow may leave (128)
 *   ceil      256..512, floor <= ceil: the most; above 256 a highlight passes too (256)
 *   dark      0..255: the plate's mean level below which its chromaticity is not trusted (32)
 * The box sum D of d', the thresholds, the erosions and the labels are those of vm_trimap_from_plate, and so are the
 * buffers, the workspace size and the two launches (SHADOW instantiation of the candidates kernel: the quotient is an
 * f32 reciprocal estimate settled by an integer remainder, exact).  tests/plate_shadow_ref.py restates it in numpy; the
 * kernels match it byte for byte.  The values in brackets are the wrappers' defaults: those of a numpy prototype,
 * untuned on real footage.  On its synthetic scene (tests/plate_shadow_ref.py, 20 seeds) a soft shadow that keeps 0.8
 * or 0.6 of the light has none of its core labelled 0 by vm_trimap_from_plate, and at 0.6 up to 476 background pixels
 * per frame labelled 255; with d' 0.72-0.84 of the core is labelled 0, no pixel with alpha > 0 is labelled 0 and none
 * with alpha < 1 is labelled 255.
 * What this is not: a per-pixel colour test, so a subject that is a darker version of the plate's own hue passes as
 * shadow and is labelled background (a dark-grey shirt on a light-grey wall, any grey on any grey: a 110-grey square
 * on a flat 180-grey plate is labelled 0 throughout; vm_trimap_fill_enclosed repairs only an enclosed one).  There is
 * no smoothness or texture test of the light ratio and no temporal test.  A shadow deeper than floor, or within noise
 * of it, falls back to d, and one such pixel costs its whole (2 r_bg + 3)^2 neighbourhood (with floor 128 a 0.6
 * shadow holds; a 0.45 shadow with floor 100 mostly does not).  Plate pixels darker than dark get no tolerance.  Only
 * the trimap changes: the model still sees the shadowed frame against the unshadowed plate, and a composite onto a new
 * plate carries the shadow additively (cmp - bg), not as a multiplicative shadow pass.
 * VM_EINVAL as vm_trimap_from_plate, and for floor, ceil or dark out of range (floor <= 256 <= ceil by their ranges). */
int vm_trimap_from_plate_shadow(const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int lo, int hi,
                                int r_bg, int r_fg, int floor, int ceil, int dark, uint8_t* out, void* work,
                                void* stream);

/* ---------------------------------------------------------------- connected components, and enclosed background
 * components_label(mask, value, connectivity) = labels, per frame:
 *   mask     uint8 [n,h,w] at any byte address; a pixel is set iff its byte equals value (0..255)
 *   labels   int32 [n,h,w], 4-byte aligned, not overlapping mask: for a set pixel the smallest row-major index y w + x
 *            within its own frame among the pixels of its 4- or 8-connected component, -1 for every other pixel
 * The labels array is the working storage (no workspace).  A union-find with parents that only ever decrease
 * (csrc/components.hip states the invariant): the result is canonical, it does not depend on the order of the atomics.
 * Three launches (two where the frame is one 64 x 32 tile), no allocation, no synchronisation, no host read-back: the
 * call can be captured in a graph.
 *
 * trimap_fill_enclosed(trimap, max_area) = out, per frame, all integer: the automatic trimap's background label is a
 * hard claim, and foreground that matches the plate over a wide area gets it; such a hole does not reach the frame.
 *   Z        the pixels whose byte is 0, and their 4-connected components (4, so that the background does not leak
 *            through a diagonal gap of an 8-connected subject)
 *   enclosed a component none of whose pixels has y in {0, h - 1} or x in {0, w - 1}
 *   out      uint8 [n,h,w]: 128 on the pixels of every enclosed component of at most max_area pixels (max_area == 0: of
 *            any area); everywhere else the input byte, whatever it is (only == 0 is ever tested).  h < 3 or w < 3:
 *            nothing is enclosed, the call is a copy
 *   out == trimap (the same pointer) fills in place; any other overlap of out, trimap and work is refused.  trimap and
 *            out may sit at any byte address
 *   work     vm_trimap_fill_enclosed_workspace_bytes(n, h, w) = 8 n h w bytes, 16-byte aligned: the labels, and an
 *            int32 per pixel that holds the component's border flag and area at its root.  The call initialises what
 *            it reads: the workspace's contents before it do not matter
 * What this is not: a hole that reaches the frame's border is not filled, and a legitimate enclosed gap (between arm
 * and body) becomes unknown as well.  tests/trimap_fill_ref.py restates both definitions in numpy by a breadth-first
 * flood; the kernels match it exactly.
 * Four launches (one copy for h < 3 or w < 3), the area sums only with max_area > 0.  VM_EINVAL for a NULL pointer, n, h
 * or w < 1 (or n * h * w beyond 2^31 - 1), value outside 0..255, connectivity other than 4 or 8, max_area < 0, a
 * misaligned labels or work, or a forbidden overlap (checked before any HIP call); the size query returns 0 for such
 * shapes. */
int vm_components_label(const uint8_t* mask, int n, int h, int w, int value, int connectivity, int32_t* labels,
                        void* stream);
size_t vm_trimap_fill_enclosed_workspace_bytes(int n, int h, int w);
int vm_trimap_fill_enclosed(const uint8_t* trimap, int n, int h, int w, int max_area, uint8_t* out, void* work,
                            void* stream);

/* ---------------------------------------------------------------- the background plate from the clip itself
 * Every model takes the clean background plate; a shot without one can estimate it, if the camera is locked off and the
 * subject moves, as the per-pixel temporal median of a sample of its frames (the reference has no counterpart: its
 * backgrounds are given).  plate_from_samples(samples) = (plate, spread), all integer:
 *   samples  uint8 [n,h,w,3], contiguous, 1 <= n <= VM_PLATE_MAX_SAMPLES
 *   sorted   for every byte position p of a frame (h * w * 3 of them) s_0 <= ... <= s_{n-1}: the n sample bytes at p
 *   plate    uint8 [h,w,3]: plate[p] = s_m, m = (n - 1) / 2 (integer division).  The lower median, per channel, nothing
 *            averaged: every output byte occurred in the samples.  np.sort(samples, 0)[m]
 *   spread   uint8 [h,w] or NULL: spread[y,x] = max over the pixel's three bytes of (s_hi - s_lo), lo = (n - 1) / 4,
 *            hi = n - 1 - lo: the interquantile range, large where the subject covered the pixel in a good share of the
 *            samples or where the shot is noisy, that is, where the plate is not to be trusted
 *   n == 1   plate = samples[0], spread = 0
 * Consequences: a pixel that the subject covers in at most (n - 1) / 2 samples and that shows one value in all others
 * gets that value, whatever covered it; covered in at most (n - 1) / 4 samples, its spread is 0 as well.
 * What this is not: it needs a locked-off camera; a pixel covered in more than half the samples gets the subject's
 * colour (spread shows it); there is no exposure or flicker compensation (vm_plate_gain_fit matches a finished plate
 * to a frame; the samples themselves are taken as they are).
 * tests/plate_ref.py restates the definition in numpy; the kernel matches it byte for byte.
 * One launch (csrc/plate.hip): a thread per dword of the frame, the n samples of its 4 bytes in registers through a
 * sorting network.  samples, plate and spread may sit at any byte address.  No byte outside plate[0 : h*w*3] and
 * spread[0 : h*w] is written.
 * No workspace, no allocation, no atomics and no synchronisation inside: the call can be captured in a graph.
 * VM_EINVAL for a NULL samples or plate, n outside 1..64, h or w < 1, n * h * w * 3 beyond 2^31 - 1, or plate / spread
 * overlapping samples or each other (checked before any HIP call). */
#define VM_PLATE_MAX_SAMPLES 64
int vm_plate_from_samples(const uint8_t* samples, int n, int h, int w, uint8_t* plate, uint8_t* spread, void* stream);

/* ---------------------------------------------------------------- matting metrics of a matte against ground truth
 * The per-frame metrics of Rhemann et al. (SAD, MSE, gradient error) over the trimap's unknown region and the temporal
 * metrics of Erofeev et al. (dtSSD, MESSDdt) as per-frame sums; the figures follow from the sums on the host (the
 * reference scores nothing but its training loss: no counterpart there).  Connectivity error is not computed.
 *   pred, gt    [n,h,w], each VM_F32 or VM_U8, independently
 *   trimap      uint8 [n,h,w] or NULL
 *   prev_pred, prev_gt  [h,w] with the dtypes of pred and gt, or both NULL: the frame before frame 0 of this call
 *   backward    f32 [n,h,w,2] or NULL, reader.read_flow layout, 8-byte aligned: frame j's flow into frame j - 1, what
 *               vm_clip_feed and vm_trimap_propagate consume
 *   stats       f64 [n,8], 8-byte aligned;  grad_map f32 [n,h,w] or NULL
 * Per pixel everything is f32, nothing contracted, IEEE division and sqrt:
 *   unit value  U(q) = (float)q / 255.f of a uint8, U(v) = min(max(v, 0), 1) of an f32 with NaN -> 0 (vm_matte_compose's
 *               clamp); a = U(pred), g = U(gt)
 *   region R_j  with a trimap the pixels of frame j whose trimap byte is neither 0 nor 255 (vm_trimap_propagate's
 *               "unknown"); without one every pixel
 *   terms       d = a - g; sad = |d|; sse = d * d
 *   gradient    Gaussian first-derivative filters, sigma 1.4, radius 4 (9 x 9), replicated borders.  Taps for i = -4..4:
 *               g_i = exp(-i^2 / (2 sigma^2)), d_i = -i g_i, G = g / sqrt(sum g^2), D = d / sqrt(sum d^2), computed in
 *               float64 and rounded to f32:
 *                 G = 0.010715649f 0.0639064f 0.22881863f 0.4918805f 0.63481766f 0.4918805f 0.22881863f 0.0639064f
 *                     0.010715649f
 *                 D = 0.04329901f 0.19367121f 0.46229678f 0.49688867f +0.0f -0.49688867f -0.46229678f -0.19367121f
 *                     -0.04329901f
 *               a 1-D pass is acc = 0; for k = -4..4 ascending: acc = acc + tap[k] * v[clamped index + k];
 *               gx = vertical_G(horizontal_D(x)), gy = vertical_D(horizontal_G(x)), m(x) = sqrtf(gx * gx + gy * gy);
 *               grad = (m(a) - m(g))^2.  The filters read neighbours outside the region; only the sum is restricted.
 *   temporal    for frame j >= 1 against frame j - 1 of the same arrays, for frame 0 against prev_* (without prev_* all
 *               three temporal entries of frame 0 are 0); (a', g') the previous frame's unit values:
 *               dt = ((a - a') - (g - g'))^2, summed over R_j
 *   MESSDdt     only with backward b: xs = f32(x) + b[0], ys = f32(y) + b[1]; a pixel takes part only if 0 <= xs <= w - 1
 *               and 0 <= ys <= h - 1 (NaN and infinities drop out).  e' = (a' - g')^2 at x0 = floor(xs),
 *               x1 = min(x0 + 1, w - 1), y likewise; fx = xs - x0, fy = ys - y0; top = e'00 + fx * (e'01 - e'00), bot
 *               likewise, e^ = top + fy * (bot - top) (vm_flow_estimate's bilinear); me = |sse - e^| summed over the
 *               pixels of R_j that take part, and they are counted
 *   sums        float64, every f32 term converted before it is added; per-block partials and a fold in a fixed order, no
 *               atomics: the same inputs give the same bits on every run
 * stats row j: [0] pixels in R_j, [1] sum sad, [2] sum sse, [3] sum grad, [4] sum dt, [5] sum me, [6] pixels that took
 * part in [5], [7] 0; entries 4 - 6 are 0 where they do not apply.  grad_map receives grad of every pixel, whatever its
 * region.  Figures: SAD = [1], MSE = [2] / [0], Grad = [3], dtSSD = sqrt([4] / [0]), MESSDdt = [5] / [6] (published
 * tables usually quote SAD / 1000, MSE * 1000 and Grad / 1000).  tests/score_ref.py restates all of this in numpy; the
 * kernel's counts and grad_map equal it exactly and each sum is the restatement's f32 terms added in f64.
 * One fused launch over 64 x 16 tiles with a 4-pixel halo in LDS, then a fold (csrc/score.hip); 16-byte f32 / dword
 * uint8 loads when the plane is so aligned and w is a multiple of 4, else element by element, the same bits.
 *   work  vm_matte_score_workspace_bytes(n, h, w) bytes, 8-byte aligned
 * No allocation and no synchronisation inside: the call can be captured in a graph.  VM_EINVAL for a NULL pred / gt /
 * stats / work, n, h or w < 1 (or more than 2^23 tiles), a dtype other than VM_F32 / VM_U8, only one of prev_pred /
 * prev_gt, a misaligned backward / stats / work or an f32 plane off 4 bytes (checked before any HIP call); the size
 * query returns 0 for such shapes. */
size_t vm_matte_score_workspace_bytes(int n, int h, int w);
int vm_matte_score(const void* pred, int pred_dtype, const void* gt, int gt_dtype, const uint8_t* trimap,
                   const void* prev_pred, const void* prev_gt, const float* backward, int n, int h, int w,
                   double* stats, float* grad_map, void* work, void* stream);

/* ---------------------------------------------------------------- guided matte upsampling
 * A frame larger than the model should see (2160 x 3840) is reduced by s = 2, 3 or 4, the model runs on the reduced
 * frame, and its matte is carried back up by a guided filter steered by the full-resolution frame (He & Sun, "Fast
 * Guided Filter"; the reference has no counterpart, it runs at the frames' size).  With hm = ceil(h / s) and
 * wm = ceil(w / s), three calls (csrc/guided.hip); tests/guided_ref.py restates each in numpy.
 *
 * frames_reduce_u8(src, s, kind) = dst, all integer:
 *   src   uint8 [n,h,w,c] at any byte address; dst uint8 [n,hm,wm,c], not overlapping src
 *   block output pixel (Y, X) stands for the input pixels y in [s Y, min(h, s Y + s)), x in [s X, min(w, s X + s)):
 *         cnt of them, fewer in the ragged last row and column
 *   VM_REDUCE_MEAN (c == 3)    per byte (2 sum + cnt) / (2 cnt) in integers: the block's mean, halves rounded up
 *   VM_REDUCE_TRIMAP (c == 1)  the block's byte if all cnt bytes agree, else 128: a reduced 0 or 255 is still a hard
 *                              claim about every pixel it stands for
 * One thread makes 12 (mean) or 16 (trimap) output bytes; it reads every input row of its blocks as aligned dwords
 * shifted into place, whatever the row's address, and stores dwords where the output row is 4-byte aligned.  Only the
 * ragged last blocks of a row go byte by byte.
 *
 * guided_coeffs(g, p, r, eps) = ab: the linear model p ~ a . I + b around every low-resolution pixel
 *   g     uint8 [n,hm,wm,3], the reduced frame; I = g / 255.  p f32 [n,hm,wm], the model's matte, 4-byte aligned
 *   r     1..8: windows are (2 r + 1)^2, clipped to the image (N pixels; the image may be smaller than the window)
 *   eps   1e-5 .. 1
 *   Sigma = mean(I I^T) - mean(I) mean(I)^T + eps 1_3;  c = mean(I p) - mean(I) mean(p);  a = Sigma^-1 c;
 *   b = mean(p) - a . mean(I);  (a, b) rounded to f32 once; ab = the mean of (a, b) over the same clipped window,
 *   summed in f64, rounded to f32 once
 *   ab    f32 [n,hm,wm,4] = (a_0, a_1, a_2, b), 16-byte aligned
 *   work  vm_guided_workspace_bytes(n, hm, wm) bytes, 16-byte aligned: the unaveraged (a, b)
 * The guide's moments (sums of bytes and of byte products) and N S_II - S_I S_I^T are exact integers; the moments with
 * p and the 3 x 3 solve (L D L^T) are f64.  Sigma's conditioning is at most (0.75 + eps) / eps, which is what the
 * lower bound on eps is for: the f64 error stays orders of magnitude below an f32 ulp, so ab differs from the f64
 * restatement by the two f32 roundings only.  Two launches over 32 x 8 tiles staged in LDS with their r-pixel halo;
 * each thread sums its window directly ((2 r + 1)^2 taps: the low-resolution side is a quarter of the pixels or less).
 *
 * guided_apply(ab, cmp, s) = alpha, f32 operation by operation, nothing contracted:
 *   cmp   uint8 [n,h,w,3] at any byte address; alpha f32 [n,h,w], 4-byte aligned
 *   fy = (f32(y) + 0.5f) / f32(s) - 0.5f clamped to [0, hm - 1]; y0 = floor(fy), y1 = min(y0 + 1, hm - 1), ty = fy - y0;
 *   x likewise.  lerp(u, v, t) = u + t * (v - u).  Per component of (a, b):
 *   m = lerp(lerp(ab[y0,x0], ab[y0,x1], tx), lerp(ab[y1,x0], ab[y1,x1], tx), ty): horizontally first
 *   q = ((m_0 * I_0 + m_1 * I_1) + m_2 * I_2) + m_3, I_c = f32(cmp_c) / 255.0f;  alpha = min(max(q, 0), 1) (NaN -> 0)
 * Traffic per pixel: 3 B read, 4 B written, and 16 / s^2 B of ab.  A lane owns 4 consecutive pixels of a column strip
 * (the frame's 12 bytes as aligned dwords shifted into place, one 16-byte store where the row allows it) and walks 16
 * rows; the fx weights are computed once per lane, the fy weights once per block, and a texel row is read and
 * interpolated horizontally once per wave and strip, not per pixel.
 * No allocation and no synchronisation inside any of the three: they can be captured in a graph.  VM_EINVAL for a NULL
 * pointer, n, h or w < 1 (or 4 n h w beyond 2^31 - 1), s outside 2..4, an unknown kind or the wrong c for it, r or eps
 * out of range (NaN included), a misaligned p / ab / work / alpha, or an output that overlaps an input (checked before
 * any HIP call); the size query returns 0 for such shapes. */
#define VM_REDUCE_MEAN 0
#define VM_REDUCE_TRIMAP 1
int vm_frames_reduce_u8(const uint8_t* src, int n, int h, int w, int c, int scale, int kind, uint8_t* dst,
                        void* stream);
size_t vm_guided_workspace_bytes(int n, int hm, int wm);
int vm_guided_coeffs(const uint8_t* guide, const float* p, int n, int hm, int wm, int r, double eps, float* ab,
                     void* work, void* stream);
int vm_guided_apply(const float* ab, const uint8_t* cmp, int n, int h, int w, int scale, float* alpha, void* stream);

/* ---------------------------------------------------------------- the plate's exposure matched to the frame
 * Everything driven by the background (the model's input, the plate trimap, the compose modes) takes the plate and the
 * frame to be shot at one exposure; auto-exposure, lamp flicker or a plate shot earlier shift the whole frame by 10 - 25 %.
 * One gain per frame and colour channel is fitted between frame and plate and the plate is scaled by it (the reference
 * has no counterpart: its backgrounds are the composites' own).  All integer.  Per frame i and channel c, with
 * a = cmp[i,y,x,c] and b = bg[i or 0,y,x,c]:
 *   cmp      uint8 [n,h,w,3] BGR; bg uint8 [nb,h,w,3], nb == n or nb == 1 (one static plate), as vm_frames_from_u8
 *   valid    16 <= b <= 250, a <= 250 and t = 64 a + (b >> 1) < 255 b: a dark plate byte carries no ratio, a clipped byte
 *            a false one, and the last condition keeps the clamp bin 255 out of the histogram
 *   bin      q = t / b (integer division), 0..254: the ratio a / b to the nearest 1/64
 *   H, S     H[q] counts the valid pixels; S[q] = H[q - 1] + H[q] + H[q + 1], H[-1] = H[255] = 0
 *   mode     q0 = the smallest q in 16..254 at which S is largest (no valid pixel: 16).  The mode and not a least-squares
 *            fit over everything: the subject's pixels are outliers of any size
 *   inlier   valid and |64 a - q0 b| <= band b;  band 1..16
 *   sums     over the inliers, int64: cnt, N = sum a b, D = sum b b
 *   gain     int32 [n,3], Q12: G = (4096 N + (D >> 1)) / D if cnt * min_share >= h w, else 4096 (the identity);
 *            min_share 1..4096.  G lies within 64 (q0 -+ band), so G <= 17281
 *   support  int32 [n,3]: cnt in both cases; a small support says the fit is not to be trusted
 *   apply    out uint8 [n,h,w,3]: out = min(255, (G[i,c] b + 2048) >> 12).  Gains outside 0 .. 2^20 are taken as the nearer
 *            end (for G >= 0 that changes no result and G b stays within 32 bits)
 * What this is not: one multiplicative gain per channel and frame - no offset, no shadows, no vignetting or local change;
 * a clipped region gets no match; the fit fails where the subject and not the background is the largest population of
 * one ratio, or where too little of the plate lies within 16..250 (support shows it; below h w / min_share the gain is the
 * identity).  tests/plate_gain_ref.py restates the definition in numpy; the kernels match it exactly.
 * vm_plate_gain_fit is four launches for all n frames (csrc/plate_gain.hip): it zeroes the part of `work` it uses, adds
 * per-block LDS histograms into it, finds each frame's modes and adds the inlier sums, and finishes the quotients;
 * integer atomics only, so the result does not depend on their order.  vm_plate_gain_apply is one launch.
 *   work     vm_plate_gain_workspace_bytes(n) bytes, 16-byte aligned; the call initialises what it reads of it
 * cmp, bg and out may sit at any byte address; gain and support are 4-byte aligned.  No allocation, no synchronisation
 * and no host read-back inside: the calls can be captured in a graph.  VM_EINVAL for a NULL pointer, n, h or w < 1,
 * n * h * w * 3 beyond 2^31 - 1, nb not 1 or n, band or min_share out of range, out overlapping bg or gain, or a misaligned
 * gain / support / work (checked before any HIP call); the size query returns 0 for n < 1. */
size_t vm_plate_gain_workspace_bytes(int n);
int vm_plate_gain_fit(const uint8_t* cmp, const uint8_t* bg, int nb, int n, int h, int w, int band, int min_share,
                      int32_t* gain, int32_t* support, void* work, void* stream);
int vm_plate_gain_apply(const uint8_t* bg, int nb, const int32_t* gain, int n, int h, int w, uint8_t* out, void* stream);

/* ---------------------------------------------------------------- the plate's position matched to the frame
 * Everything driven by the background takes the plate and the frame to be registered pixel for pixel; a bumped tripod, a
 * handheld plate, lens breathing or a slow pan move the plate by a fraction of a pixel up to a few pixels, and on a textured
 * background half a pixel is enough to switch the plate trimap off.  One affine map and one photometric gain per frame
 * are fitted between the grey pyramids (vm_flow_pyramid) of the frame and of the plate, and the plate is resampled through
 * the map (the reference has no counterpart).  Per frame i:
 *   cmp_pyr  f32: frame i's pyramid starts at cmp_pyr + i cmp_stride (floats; at least vm_flow_pyramid_bytes / 4);
 *            bg_pyr likewise with bg_stride, nb == n or nb == 1 (one plate pyramid for all frames; bg_stride is not read);
 *            both of [h,w] frames at `levels`, levels k = 0 .. K of h_k x w_k pixels, I_k and P_k
 *   model    p0..p5 and g, deviations from the identity in centred level-0 pixels xc = x - (w - 1) / 2, yc = y - (h - 1) / 2:
 *            frame pixel (x, y) sees the plate at X = x + ((p0 xc + p1 yc) + p2), Y = y + ((p3 xc + p4 yc) + p5), and
 *            grey(frame) ~ g grey(plate there).  g is a nuisance parameter that lets the fit work on a frame shot at another
 *            exposure: it is reported and never applied (vm_plate_gain_fit does that per channel afterwards)
 *   start    p = 0; g = f32(sum I_K / sum P_K) (f64 sums and quotient) if sum P_K > 0, else 1
 *   step     `iters` times per level, from K down to 0, all per-pixel terms f32, nothing contracted.  For level pixel (x, y),
 *            s = 2^k: X0 = (x + 0.5f) s - 0.5f, Y0 likewise, xc = X0 - (w - 1) 0.5f, yc = Y0 - (h - 1) 0.5f, (X, Y) as above
 *            from (X0, Y0), level position xl = (X + 0.5f) / s - 0.5f, yl likewise;  inside = 0 <= xl <= w_k - 1 and
 *            0 <= yl <= h_k - 1;  B = vm_flow_estimate's bilinear of P_k (coordinates clamped): Pw = B(xl, yl),
 *            Gx = ((B(xl + 1, yl) - B(xl - 1, yl)) 0.5f) / s, Gy likewise;  r = I_k - g Pw;  a = g Gx, b = g Gy;
 *            J = (a xc, a yc, a, b xc, b yc, b, Pw);  inlier = inside and |r| <= tol;  close = inside and |r| <= tol 0.25f
 *   sums     over the inliers, f64, each term one f32 product widened: the 28 J_u J_v (u <= v), the 7 J_u r; count of the
 *            inliers, and of the close pixels
 *   solve    if count min_share >= h_k w_k: (J^T J) d = J^T r by Gaussian elimination without pivoting in f64; a pivot that
 *            is not positive ends it.  Solved: p_u = f32(f64(p_u) + d_u), g likewise.  Otherwise the step changes nothing
 *   support  int32 [n]: the close count of the last step, or 0 where that step met a pivot that is not positive (a plate
 *            without texture has nothing to fit).  The close pixels and not the inliers: two unrelated images leave 33 - 48 %
 *            of their pixels within 16 grey levels but only about 10 % within 4, a fitted background nearly all of its own
 *   result   params f32 [n,8] = (p0..p5, g, 0); the identity (0 .. 0, 1, 0) instead if support min_share < h w, if a
 *            parameter is not finite, or if one of the frame's four corners (-+ (w - 1) / 2, -+ (h - 1) / 2) is displaced by
 *            more than f32(min(h, w)) / f32(reach) pixels (dx dx + dy dy <= lim lim must hold).  The corner limit guards
 *            against a diverged fit; it does not promise that every divergence ends outside it
 *   apply    out uint8 [n,h,w,3]: per pixel (X, Y) as above with (X0, Y0) = (x, y); out = clamp(rint(B(bg[i or 0]))) per
 *            channel on the bytes as f32, coordinates clamped to the plate (replicate border).  Identity parameters
 *            reproduce the plate byte for byte
 * What this is not: one global affine map per frame - no parallax, no rolling shutter, no lens distortion; a textureless
 * plate has nothing to fit and gets the identity (support shows it); the strip that leaves the plate is replicated border
 * and will not match the frame; the truncated weight needs the coarsest level to see the motion, so a shift well beyond
 * a coarsest-level pixel (2^K pixels) is outside the fit's basin: it ends at the identity or, rarely, at a wrong map within
 * `reach` (at 64 x 96, K = 2, shifts of 3.5 and 12.5 pixels do; tests/test_plate_align_host.py); the defaults are untuned on
 * real footage.
 * tests/plate_align_ref.py restates the definition in numpy; vm_plate_align_apply matches it bit for bit, the fit up to the
 * order of its f64 sums.  The kernels' order is fixed (csrc/plate_align.hip: per lane in f64 registers, a wave-64 shuffle
 * tree, the four waves in LDS, the blocks' partials in `work` added in index order; no floating-point atomics; the blocks per
 * frame depend on the level's size only), so two runs give the same bits and a batch of n what n single calls give.
 * vm_plate_align_fit is 1 + 2 levels iters launches for all n frames, vm_plate_align_apply one.
 *   work     vm_plate_align_workspace_bytes(n, h, w, levels) bytes, 16-byte aligned; the call initialises what it reads
 * bg and out may sit at any byte address; pyramids, params and support are 4-byte aligned.  No allocation, no synchronisation
 * and no host read-back inside: the calls can be captured in a graph.  VM_EINVAL for a NULL pointer, n < 1, h or w < 16
 * (apply: < 1) or beyond 32768, n h w 3 beyond 2^31 - 1, levels < 1, nb not 1 or n, iters outside 1..64, tol <= 0 or not
 * finite, min_share outside 1..4096, reach outside 1..1024, a stride below one pyramid, a misaligned pyramid / params /
 * support / work, or out overlapping bg or params (checked before any HIP call); the size query returns 0 for such shapes. */
size_t vm_plate_align_workspace_bytes(int n, int h, int w, int levels);
int vm_plate_align_fit(const float* cmp_pyr, long cmp_stride, const float* bg_pyr, long bg_stride, int nb, int n, int h,
                       int w, int levels, int iters, float tol, int min_share, int reach, float* params, int32_t* support,
                       void* work, void* stream);
int vm_plate_align_apply(const uint8_t* bg, int nb, const float* params, int n, int h, int w, uint8_t* out, void* stream);

/* ---------------------------------------------------------------- flow-compensated temporal matte filter
 * A model that mattes every frame on its own leaves mattes that shimmer along soft edges (vm_matte_score's dtSSD and
 * MESSDdt measure it).  This is a post-filter on the model's output: frame j's matte is pulled towards the previous
 * *filtered* matte, sampled where the backward flow says the pixel came from, and two gates close the pull where it would
 * smear a real change (the reference has no counterpart).  All f32, one operation per step, nothing contracted.  Frame j
 * has alpha[j] (the model's matte), cmp[j], backward[j] (frame j at (x, y) ~ frame j - 1 at (x + u, y + v), (u, v) =
 * backward[j,y,x]), the previous filtered matte s' and the previous frame cmp'.  With unit(v) = vm_matte_score's clamp to
 * [0,1] (NaN -> 0), per pixel (x, y):
 *   a        unit(alpha[j,y,x])
 *   target   xs = (float)x + u, ys = (float)y + v;  inside = 0 <= xs <= w - 1 and 0 <= ys <= h - 1 (false for NaN);
 *            outside, the target is (0, 0)
 *   taps     x0 = floor(xs), x1 = min(x0 + 1, w - 1), fx = xs - x0, and the same in y: vm_matte_score's bilinear
 *            convention;  sample(v) = top + fy (bot - top), top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10)
 *   p        sample(unit(s'))  (s' is a filtered matte, which unit leaves as it is; a caller's prev_alpha is clamped)
 *   d        max over the 3 channels of |(float)cmp[j,y,x,ch] - sample((float)cmp'[...,ch])|
 *   k        unit(1 - d inv_tol) * unit(1 - |a - p| inv_jump), and 0 where not inside;  inv_tol = 1.0f / tol and
 *            inv_jump = 1.0f / jump, divided once on the host in f32
 *   out      s = unit(a + (strength k) (p - a))
 *   weight   k
 * A frame with nothing before it (frame 0 without prev_*) gets s = a and weight 0.  The n frames are processed in
 * order, one launch each (csrc/matte_smooth.hip): frame 0 reads (prev_alpha, prev_cmp), frame j >= 1 reads (out[j - 1],
 * cmp[j - 1]); backward[0] is not read without a predecessor.
 *   alpha    f32 [n,h,w];  cmp uint8 [n,h,w,3];  backward f32 [n,h,w,2] (reader.read_flow layout)
 *   prev_alpha, prev_cmp   f32 [h,w], uint8 [h,w,3]: the frame before frame 0; both NULL: there is none
 *   strength 0 <= strength < 1: the share of the previous matte where both gates are open
 *   tol      > 0, finite, in grey levels: the colour difference at which the photometric gate is shut
 *   jump     > 0, finite, in matte units: the matte difference at which the jump gate is shut
 *   out      f32 [n,h,w]; may be exactly `alpha` (in place: a thread reads only its own pixel of alpha[j])
 *   weight   f32 [n,h,w] or NULL: where the filter held back
 * What this is not: it is one-sided and recursive - one frame of history, no look-ahead, so it lags rather than centres;
 * it detects no cuts (a cut is only caught by the photometric gate, pixel by pixel); the gate is colour-based, so a
 * flicker where subject and background share a colour passes through it, and a wrong flow between equal colours smears;
 * it is no substitute for a recurrent model.  Its effect was measured on a synthetic clip only (tests/matte_smooth_ref.py,
 * DESIGN 3.4n): nothing is known about a trained model's mattes on real footage, and the defaults are untuned.
 * cmp and prev_cmp may sit at any byte address; the f32 arrays are 4-byte aligned.  No workspace, no allocation, no
 * synchronisation: the call can be captured in a graph.  VM_EINVAL for a NULL alpha / cmp / backward / out, exactly one
 * of prev_alpha / prev_cmp, n, h or w < 1, n * h * w * 3 beyond 2^31 - 1, strength, tol or jump out of range (NaN
 * included), a misaligned f32 pointer, out overlapping an input other than being alpha itself, or weight overlapping
 * an input or out (checked before any HIP call). */
int vm_matte_smooth(const float* alpha, const uint8_t* cmp, const float* backward, const float* prev_alpha,
                    const uint8_t* prev_cmp, int n, int h, int w, float strength, float tol, float jump, float* out,
                    float* weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VMATTING_H */
