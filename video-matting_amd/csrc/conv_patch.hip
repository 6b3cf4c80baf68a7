// The patch kernels of the 3x3 conv (bf16 / fp16, chunk-major K; conv3x3.hip's header has the GEMM view and K layout):
// the streaming kernel conv3x3_patch with its FIRST (conv1_1 fused in), folded-upconv and split-K forms, the persistent
// row-slot kernel conv3x3_patch_persist, the split-K reduction, and their routing (dispatch_patch), which also reaches
// the row-stationary kernel of conv_rows.hip.
#include "conv_border.h"
#include "conv_dispatch.h"

namespace vm {

// ================================================================ patch kernel (bf16, chunk-major K)
// 2-D output tile of 8 x 32 pixels.  Per 64-byte channel granule the (8+2) x (32+2) input patch is DMA'd to
// LDS ONCE and serves all 9 taps: the MFMA pixel fragments of tap (dh, dw) are the patch rows shifted by
// (dh+1)*34 + dw+1, so the input costs 1.33x its bytes per granule instead of 9x.  Weights stream per tap
// (granule order cc*9+tap is exactly the chunk-major packing) through an S-slot ring.  LDS-DMA with the
// 64-byte-row XOR swizzle applied at the source (conflict-free fragment reads for any start row); counted
// vmcnt per wave + one barrier per step; dummy (out-of-range) pieces past the end keep the counts uniform.
template <int BN, int WM, int WN, int S, int TH_ = 8, int G_ = 1>
struct PatchCfg {
  static constexpr int G = G_;                               // taps per weight-ring slot (one barrier per slot)
  static constexpr int TH = TH_, TW = 32, BM = TH * TW;
  static constexpr int PW = TW + 2, PPIX = (TH + 2) * PW;  // 340 patch pixels
  static constexpr int NW = WM * WN, NT = 64 * NW;
  static constexpr int XP = (PPIX + 15) / 16;                // 22 DMA pieces per patch
  static constexpr int XPW = (XP + NW - 1) / NW;             // max X pieces per wave
  static constexpr int PB = XP * 1024;
  static constexpr int WP = BN / 16;                         // DMA pieces per weight slot
  static constexpr int WPW = (WP + NW - 1) / NW;
  static constexpr int WSLOT = BN * 64;
  static constexpr int TPM = BM / WM, TPN = BN / WN;
  static constexpr int FP = TPM / 16, FC = TPN / 16;
  static constexpr int SR = 64 * 2 + 16;                    // epilogue staging row (one 64-channel slab, bf16)
  static constexpr int SR32 = 64 * 4 + 16;                  // the same slab in f32 (f32 output views)
  static constexpr int EPI = BM * SR32;
  static constexpr int MAIN = 2 * PB + S * G * WSLOT;
  static constexpr int LDS = MAIN > EPI ? MAIN : EPI;
  static constexpr int IW = TW + 4, IPIX = (TH + 4) * IW;   // FIRST: 8-channel input patch (16 B per pixel)
  static constexpr int LDS_FIRST = MAIN + IPIX * 16 > EPI ? MAIN + IPIX * 16 : EPI;
  // register epilogue (vm_set_option "patch_repi"): a wave's pixel fragments must cover 2 whole rows so the fused
  // 2x2 pool pairs rows inside the wave; 32-pixel waves of 8 x 32 / 4 x 32 tiles (TH == WM) are remapped to 2 rows x
  // 16 pixels (wave pair 2k, 2k+1 = rows 2k, 2k+1), 64-pixel waves already hold 2 rows x 32 pixels.  Either way every
  // output pixel keeps its MFMA sequence, so results do not depend on the mapping.
  static constexpr bool REMAP = TPM == 32 && TW == 32 && WM % 2 == 0 && TH == WM;
  static constexpr bool REPI_OK = G == 3 && (REMAP || TPM == 64);
  static constexpr int PSTEP = REMAP ? 1 : 2;  // pixel fragment of the row below fragment fp (pool partner)
  // folded upconvs: the border pass can run in extra blocks of the launch (ConvArgs::bfuse), one 4-wave group per 256
  // threads, each staging in its own slice of the main pipeline's LDS
  static constexpr bool BFUSE_OK = REPI_OK && NT % 256 == 0 && MAIN >= NT / 256 * BORDER_LDS;
  __device__ static int prow(int wm, int fp) { return REMAP ? 2 * (wm >> 1) + fp : (wm * TPM + fp * 16) / TW; }
  __device__ static int pcol(int wm, int fp) { return REMAP ? 16 * (wm & 1) : (wm * TPM + fp * 16) % TW; }
  __device__ static int tpix(int wm, int fp) { return prow(wm, fp) * TW + pcol(wm, fp); }  // first tile pixel
  static_assert(TPN % 64 == 0, "whole 64-channel epilogue slabs per wave column");
  static_assert(TPM % 32 == 0 || TPM == 16, "pixel fragments stay inside one patch row");
  static_assert(G == 1 || G == 3, "a slot holds one tap or one kernel row");
  static_assert(G == 1 ? (S >= 3 && S <= 9) : (S >= 2 && S <= 4), "ring depth (the X group is counted in at most one window)");
};

// First conv (cin <= 8 -> 64 channels, + bias + relu) of the patch pixels, for the FIRST patch kernel.  The 8-channel
// input patch (TH+4) x (TW+4) is staged at ip; 16-pixel fragments of the (TH+2) x (TW+2) patch are spread over the
// waves; a 32-deep K-step covers 4 taps x 8 channels (tap-major packing k = tap*8 + c, like conv3x3_first).
template <class C>
__device__ __forceinline__ void first_layer_patch(const ConvArgs& a, char* smem, int pb, char* ip, int n, int r0, int c0,
                                                  int wave, int lane, int tid) {
  using T = uint16_t;
  const int H = a.H, W = a.W;
  const T* x8 = reinterpret_cast<const T*>(a.x) + a.x_coff;
  const float* xf = reinterpret_cast<const float*>(a.x) + a.x_coff;
  for (int i = tid; i < C::IPIX; i += C::NT) {
    const int ir = i / C::IW, ic = i - ir * C::IW;
    const int h = r0 - 2 + ir, w = c0 - 2 + ic;
    uint4 v = make_uint4(0, 0, 0, 0);
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
      const long pix = (((long)n * H + h) * W + w) * (long)a.x_cstride;
      if (a.x_f32) {  // the caller's f32 frame (loader.py:76-78 layout), rounded to bf16 like vm_convert_nhwc
        // (measured: one pixel per lane beats a coalesced channel-pair sweep, whose extra LDS stores cost more)
        float f[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = c < a.x_c ? xf[pix + c] : 0.f;
        v = Chunk<T>::pack(f);
      } else {
        v = *reinterpret_cast<const uint4*>(x8 + pix);
      }
    }
    *reinterpret_cast<uint4*>(ip + i * 16) = v;
  }
  const int col = lane & 15, q = lane >> 4;
  const T* w1 = reinterpret_cast<const T*>(a.w1);
  uint4 wf[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) wf[j][fc] = *reinterpret_cast<const uint4*>(w1 + (fc * 16 + col) * 128 + j * 32 + q * 8);
  float b1[4][4];
#pragma unroll
  for (int fc = 0; fc < 4; ++fc)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) b1[fc][jj] = a.bias1 ? a.bias1[fc * 16 + 4 * q + jj] : 0.f;
  __syncthreads();
  constexpr int NF = (C::PPIX + 15) / 16;
  for (int f = wave; f < NF; f += C::NW) {
    const int p = f * 16 + col;
    const int pr = p / C::PW, pc = p - pr * C::PW;
    f32x4 acc[4];
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) acc[fc] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int tap = 4 * j + q;
      uint4 bv = make_uint4(0, 0, 0, 0);
      if (tap < 9 && p < C::PPIX) bv = *reinterpret_cast<const uint4*>(ip + ((pr + tap / 3) * C::IW + pc + tap % 3) * 16);
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) mma16<T>(wf[j][fc], bv, acc[fc]);
    }
    const int h = r0 - 1 + pr, w = c0 - 1 + pc;
    const bool inside = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
    if (p < C::PPIX) {
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        float v[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) v[jj] = inside ? fmaxf(acc[fc][jj] + b1[fc][jj], 0.f) : 0.f;
        uint2 pk;
        pk.x = bf16x2_bits(v[0], v[1]);
        pk.y = bf16x2_bits(v[2], v[3]);
        // channel fc*16 + 4q: granule fc/2, 16-byte chunk (fc&1)*2 + q/2, half q&1
        *reinterpret_cast<uint2*>(smem + (fc >> 1) * pb + swz<64>(p, (fc & 1) * 2 + (q >> 1)) + (q & 1) * 8) = pk;
      }
    }
  }
  __syncthreads();
}

// FIRST: the conv's 64-channel input is itself conv3x3(x8) + bias + relu of an 8-channel frame (unet.py:170-171,
// conv1_1 -> conv1_2): the prologue evaluates that first conv on the (TH+2) x (TW+2) patch straight into the two
// granule buffers (zero outside the frame = the second conv's SAME padding), so the 64-channel activation never
// touches HBM; the main loop then streams only weights.
// UPSKIP: the folded-upconv instantiation (vm_conv3x3_up2x_nhwc), which skips its phase filters' zero taps
// MT: the MFMA operand type (uint16_t = bf16; f16_t = the split-fp16 forward's fp16 parts, same data path)
template <int BN, int WM, int WN, int S, int TH, int MINB, int UNR, bool PF, int ABL, bool FIRST, int G = 1,
          bool UPSKIP = false, typename MT = uint16_t>
__global__ __launch_bounds__(64 * WM * WN)
__attribute__((amdgpu_waves_per_eu((UPSKIP || G > 1) && MINB * WM * WN < 16 ? 4 : MINB * WM * WN / 4)))  // <= 128 VGPRs
void conv3x3_patch(ConvArgs a) {
  using C = PatchCfg<BN, WM, WN, S, TH, G>;
  using T = uint16_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = C::NW, NT = C::NT, FP = C::FP, FC = C::FC, XPW = C::XPW, WPW = C::WPW;
  // the folded upconv's border pass in this launch (ConvArgs::bfuse): the first a.bblocks blocks run it and leave, the
  // rest are the tiles.  First, not last: beside the conv's blocks a border block's latency chain takes about two
  // tile times, which a greedy fill absorbs when it starts with the launch and which sticks out of the launch's end
  // when it starts with the last round of tiles (measured)
  constexpr bool BFUSE = UPSKIP && !FIRST && std::is_same<MT, uint16_t>::value && C::BFUSE_OK;
  [[maybe_unused]] int bid = 0;  // BFUSE: the tile block index
  if constexpr (BFUSE) {
    bid = (int)blockIdx.x;
    if (a.bfuse) {
      if (__builtin_expect(bid < a.bblocks, 0)) {  // (out of line: the tile path keeps its code layout)
        up2x_border_fused<NT>(a, smem, bid);
        return;
      }
      bid -= a.bblocks;
    }
  }
  // (the other instantiations read blockIdx.x as ever: their code is unchanged)
  auto bx = [&]() -> unsigned {
    if constexpr (BFUSE) return (unsigned)bid;
    else return blockIdx.x;
  };

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (a.prio && NW == 8 && wave >= 4) __builtin_amdgcn_s_setprio(1);
  const int wm = wave % WM, wn = wave / WM;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int VW = a.vstride ? a.vW : W;  // packed frames: one virtual image (n = 0), ConvArgs::vstride
  const int th = (H + C::TH - 1) / C::TH, tw = (VW + C::TW - 1) / C::TW;
  int st, nt;
  if (a.cband) {  // channel-banded: XCD b % 8 owns output tiles [xcd * cband, +cband) over every pixel tile
    const int i = bx() >> 3;
    st = i / a.cband;
    nt = (bx() & 7) * a.cband + (i - st * a.cband);
  } else if (a.ngroup) {  // grouped: ngroup output tiles x every pixel tile, group after group (XCD ranges within)
    const int t = xcd_tile(bx(), a.tiles_total);
    const int per = (a.tiles_total / a.tiles_n) * a.ngroup, gi = t / per, r = t - gi * per;
    st = r / a.ngroup;
    nt = gi * a.ngroup + (r - st * a.ngroup);
  } else {
    const int t = xcd_tile(bx(), a.tiles_total);
    st = t / a.tiles_n;
    nt = t - st * a.tiles_n;
  }
  const int n = st / (th * tw), srem = st - n * th * tw;
  const int r0 = (srem / tw) * C::TH, c0 = (srem - (srem / tw) * tw) * C::TW;
  const int n0 = nt * BN;
  // pixel offset (in pixels, from row r0 of the tile's frame / of frame 0 when packed) of tile pixel (pr, pc) of
  // the output; ok says whether it is a real output pixel
  auto out_pix = [&](int pr, int pc, bool& ok) {
    const int v = c0 + pc;
    if (a.vstride) {
      const int f = v / a.vstride, x = v - f * a.vstride;
      ok = r0 + pr < H && x < W && v < VW;
      return (f * H + pr) * W + x;
    }
    ok = r0 + pr < H && v < W;
    return pr * W + pc;
  };

  const T* xb = reinterpret_cast<const T*>(a.x) + a.x_coff + ((long)n * H + r0 - 1) * (long)W * cs;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(xb), 0, 0x7ffffff0, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, n0);

  // DMA geometry: piece k fills 16 LDS rows (4 lanes x 16 B per row); the lane filling physical chunk lpos of
  // row r fetches logical chunk swz(r, lpos)
  const int lrow = lane >> 2, lpos = lane & 3;
  int xoff[XPW];
  int x_n = 0;
#pragma unroll
  for (int i = 0; i < XPW && !FIRST; ++i) {
    const int piece = wave + i * NW;
    const int row = piece * 16 + lrow;
    const int lq = (swz<64>(row, lpos) - row * 64) >> 4;
    const int pr = row / C::PW, pc = row - pr * C::PW;
    int h = r0 - 1 + pr, w = c0 - 1 + pc;
    if (a.up) {  // folded 2x resize: past the bottom/right edge the low-res frame is replicated (TF1 clamp)
      h = min(h, H - 1);
      w = min(w, W - 1);
    }
    bool ok = row < C::PPIX && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)VW;
    int pix = (h - r0 + 1) * W + w;
    if (a.vstride && ok) {  // virtual column -> (frame, column); the two columns past a frame read as zero
      const int f = w / a.vstride, x = w - f * a.vstride;
      ok = x < W;
      pix = (f * H + h - r0 + 1) * W + x;
    }
    xoff[i] = ok ? (pix * cs + lq * 8) * 2 : OOB;
    if (piece < C::XP) ++x_n;
  }
  int woff[WPW];
  int w_n = 0;
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int piece = wave + i * NW;
    const int row = piece * 16 + lrow;
    const int lq = (swz<64>(row, lpos) - row * 64) >> 4;
    woff[i] = (row * a.K_pad + lq * 8) * 2;
    if (piece < C::WP) ++w_n;
  }
  const int nch_all = a.cin_pad / 32;
  const int ksp = a.ksplit > 1 ? a.ksplit : 1;
  const int per_split = (nch_all + ksp - 1) / ksp;  // host: every split non-empty
  const int cc_beg = (int)blockIdx.y * per_split;
  const int nch = min(nch_all, cc_beg + per_split), nsteps = nch * 9;  // end granule / step of this split
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  const uint32_t wring = lds0 + 2 * C::PB;

  auto issue_x = [&](int cc, int buf) {
    if constexpr (FIRST) return;
    const bool real = cc < nch;
#pragma unroll
    for (int i = 0; i < XPW; ++i)
      if (wave + i * NW < C::XP)
        glds16(xrs, lds0 + buf * C::PB + (wave + i * NW) * 1024, real ? xoff[i] + (int)src_chan(a, cc * 32) * 2 : OOB);
  };
  auto issue_w = [&](int s, int slot) {  // ring step s = taps s*G .. s*G+G-1 (chunk-major K: consecutive 64 B)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool real = s * G + g < nsteps;
#pragma unroll
      for (int i = 0; i < WPW; ++i)
        if (wave + i * NW < C::WP)
          glds16(wrs, wring + (slot * G + g) * C::WSLOT + (wave + i * NW) * 1024, real ? woff[i] + (s * G + g) * 64 : OOB);
    }
  };

  int boff[FC], abase[FP];
#pragma unroll
  for (int f = 0; f < FC; ++f) boff[f] = 2 * C::PB + swz<64>(wn * C::TPN + f * 16 + (lane & 15), lane >> 4);
#pragma unroll
  for (int f = 0; f < FP; ++f) {
    abase[f] = C::prow(wm, f) * C::PW + C::pcol(wm, f) + (lane & 15);
  }
  const int ck = lane >> 4;

  f32x4 acc[FC][FP];
#pragma unroll
  for (int i = 0; i < FC; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto frags = [&](uint4 (&av)[FC], uint4 (&bv)[FP], int slot, int buf, int tap) {
    const char* wp = smem + (slot * G + (G == 1 ? 0 : tap % G)) * C::WSLOT;
    const char* xp = smem + buf * C::PB;
#pragma unroll
    for (int f = 0; f < FC; ++f) av[f] = *reinterpret_cast<const uint4*>(wp + boff[f]);
    const int toff = (tap / 3) * C::PW + tap % 3;
#pragma unroll
    for (int f = 0; f < FP; ++f) {
      int row = abase[f] + toff;
      if constexpr (FC * FP >= 16) asm volatile("" : "+v"(row));  // recompute per step: no 9-tap address table
      bv[f] = *reinterpret_cast<const uint4*>(xp + swz<64>(row, ck));
    }
  };
  // counted DMA wait, then lgkmcnt(0): this wave's fragment reads of the ring slot / patch buffer that the DMAs
  // issued right after the barrier refill must have returned before the barrier — the MFMAs consuming them may be
  // scheduled past it (seen in the 4 x 32 folded-upconv instantiation: under a second process on the GPU the refill
  // overtook a queued ds_read about once per 100 frames)
  auto sync = [&](int n) {
    wait_vm(n);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // folded 2x resize: the TF1 legacy upsampling makes an odd output row (phase a = 1) a blend of low-res rows i and
  // i+1 only, so its phase filter's kernel row 0 (offset -1) is exactly zero; likewise kernel column 0 for odd
  // output columns (b = 1).  A block whose channels are one phase skips those taps' fragment reads and MFMAs:
  // phases (0,0) / (0,1) / (1,0) / (1,1) run 9 / 6 / 6 / 4 of the 9 taps (25 of 36, bit-identical: the skipped
  // products are exact zeros).  The weight DMA and the barriers keep their schedule: the folded convs are
  // latency-bound on that ring, and a variant that also dropped the zero rows from the ring (shorter prefetch cover)
  // measured 1.3 % slower on the whole forward, this one 0.3 % faster (same-box A/B, tools/ab_unet.py).
  const int up_phase = UPSKIP && a.up && n0 / a.up_cout == (n0 + BN - 1) / a.up_cout ? n0 / a.up_cout : 0;
  const bool skip_r0 = (up_phase >> 1) != 0 && (a.upmask & 1), skip_c0 = (up_phase & 1) != 0 && (a.upmask & 2);

  if constexpr (G > 1) {
    // one ring slot = one kernel row (G = 3 taps): one barrier per row; inside the row the fragments of tap g+1 are
    // read while tap g's MFMAs run (same slot and patch, no synchronisation needed)
    static_assert(!PF && !FIRST, "row-slot pipeline: plain configuration only");
    constexpr int R = 9 / G;
    issue_x(cc_beg, cc_beg & 1);
#pragma unroll
    for (int j = 0; j < S - 1; ++j) issue_w(cc_beg * R + j, j);
    int slot = 0;
    for (int cc = cc_beg; cc < nch; ++cc) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = cc * R + r;
        // in flight after W(k): S-2 younger row slots, plus the next patch when it was issued inside that window
        // timing ablations (results are garbage): ABL&4 no synchronisation, ABL&8 barrier without the DMA wait,
        // ABL&2 no DMA, ABL&1 no MFMA
        if constexpr (ABL & 8) {
          asm volatile("" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
        } else if constexpr (!(ABL & 4)) {
          sync((S - 2) * G * w_n + ((r >= 1 && r <= S - 2) ? x_n : 0));
        }
        if constexpr (!(ABL & 2)) {
          if (r == 0) issue_x(cc + 1, (cc + 1) & 1);
          int ns = slot + S - 1;
          ns -= ns >= S ? S : 0;
          issue_w(k + S - 1, ns);
        }
        if (!(UPSKIP && skip_r0 && r == 0)) {  // (a folded upconv's zero kernel row: no reads, no MFMAs)
          uint4 av[2][FC], bv[2][FP];
          frags(av[0], bv[0], slot, cc & 1, r * G);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            if (g + 1 < G) frags(av[(g + 1) & 1], bv[(g + 1) & 1], slot, cc & 1, r * G + g + 1);
            if constexpr (ABL & 1) {
#pragma unroll
              for (int fc = 0; fc < FC; ++fc) asm volatile("" ::"v"(av[g & 1][fc].x), "v"(av[g & 1][fc].w));
#pragma unroll
              for (int fp = 0; fp < FP; ++fp) asm volatile("" ::"v"(bv[g & 1][fp].x), "v"(bv[g & 1][fp].w));
            } else if (!(UPSKIP && skip_c0 && g == 0)) {  // (its zero kernel column: no MFMAs)
#pragma unroll
              for (int fc = 0; fc < FC; ++fc)
#pragma unroll
                for (int fp = 0; fp < FP; ++fp) mma16<MT>(av[g & 1][fc], bv[g & 1][fp], acc[fc][fp]);
            }
          }
        }
        // schedule experiments (ABL 16 / 32): pin the order of the row's fragment reads and MFMAs
        if constexpr (ABL & 16) {  // all reads of tap g+1 issued ahead of tap g's MFMAs
          __builtin_amdgcn_sched_group_barrier(0x100, FC + FP, 0);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            if (g + 1 < G) __builtin_amdgcn_sched_group_barrier(0x100, FC + FP, 0);
            __builtin_amdgcn_sched_group_barrier(0x8, FC * FP, 0);
          }
        } else if constexpr (ABL & 32) {  // tap g+1's reads spread one per MFMA of tap g
          __builtin_amdgcn_sched_group_barrier(0x100, FC + FP, 0);
#pragma unroll
          for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < FC * FP; ++i) {
              __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
              if (g + 1 < G && i < FC + FP) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        }
        slot = slot + 1 == S ? 0 : slot + 1;
      }
    }
  } else if constexpr (PF) {
    // fragments of step s+1 are read right after the barrier of step s, while step s's MFMAs run; the ring
    // holds S steps (slot s%S is refilled with step s+S once every wave has its step-s fragments in registers)
    issue_x(0, 0);
    issue_x(1, 1);
#pragma unroll
    for (int j = 0; j < S; ++j) issue_w(j, j);
    sync((S - 1) * w_n);
    uint4 av[FC], bv[FP];
    frags(av, bv, 0, 0, 0);
    int slot = 0;
    for (int cc = 0; cc < nch; ++cc) {
#pragma unroll UNR
      for (int tap = 0; tap < 9; ++tap) {
        const int s = cc * 9 + tap;
#pragma unroll
        for (int fc = 0; fc < FC; ++fc)
#pragma unroll
          for (int fp = 0; fp < FP; ++fp) mma16<MT>(av[fc], bv[fp], acc[fc][fp]);
        if (s + 1 < nsteps) {
          // in flight after W(s+1): S-2 younger weight steps, plus the patch issued at the end of the last chunk
          sync((S - 2) * w_n + ((tap <= S - 2 && cc >= 1) ? x_n : 0));
          issue_w(s + S, slot);
          if (tap == 8) issue_x(cc + 2, cc & 1);
          slot = slot + 1 == S ? 0 : slot + 1;
          frags(av, bv, slot, tap == 8 ? (cc + 1) & 1 : cc & 1, tap == 8 ? 0 : tap + 1);
        }
      }
    }
  } else {
    issue_x(0, 0);
#pragma unroll
    for (int j = 0; j < S - 1; ++j) issue_w(j, j);
    if constexpr (FIRST) first_layer_patch<C>(a, smem, C::PB, smem + C::MAIN, n, r0, c0, wave, lane, tid);
    int slot = 0;
    for (int cc = 0; cc < nch; ++cc) {
#pragma unroll UNR
      for (int tap = 0; tap < 9; ++tap) {
        const int s = cc * 9 + tap;
        // in flight after W(s): S-2 younger weight slots, plus the next patch when it was issued inside the window
        if constexpr (!(ABL & 4)) sync((S - 2) * w_n + ((tap >= 1 && tap <= S - 2) ? x_n : 0));
        if constexpr (!(ABL & 2)) {
          if (tap == 0) issue_x(cc + 1, (cc + 1) & 1);
          int ns = slot + S - 1;
          ns -= ns >= S ? S : 0;
          issue_w(s + S - 1, ns);
        }
        uint4 av[FC], bv[FP];
        frags(av, bv, slot, cc & 1, tap);
        if constexpr (!(ABL & 1)) {  // (no zero-tap skipping here: it made this pipeline spill)
#pragma unroll
          for (int fc = 0; fc < FC; ++fc)
#pragma unroll
            for (int fp = 0; fp < FP; ++fp) mma16<MT>(av[fc], bv[fp], acc[fc][fp]);
        } else {  // keep the fragment reads alive without the MFMAs
#pragma unroll
          for (int fc = 0; fc < FC; ++fc) asm volatile("" ::"v"(av[fc].x), "v"(av[fc].w));
#pragma unroll
          for (int fp = 0; fp < FP; ++fp) asm volatile("" ::"v"(bv[fp].x), "v"(bv[fp].w));
        }
        if constexpr (FC * FP >= 32) __builtin_amdgcn_sched_barrier(0);  // no cross-tap hoisting: registers
        slot = slot + 1 == S ? 0 : slot + 1;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // epilogue: one 64-channel slab per wave column, bf16 staged, 16-byte buffer stores (masked by OOB offsets)
  // a.up (folded 2x resize, vm_conv3x3_up2x_nhwc): output channel n0+sl*64+c is phase p = (a,b) of channel
  // c' = (n0+sl*64) - p*up_cout + c, stored at full-res pixel (2*h+a, 2*w+b) of the [N,2H,2W,up_cout] view
  const int ycs2 = a.y_cstride * 2;
  const int YW = a.up ? 2 * W : W;
  T* yb = reinterpret_cast<T*>(a.y) + a.y_coff +
          (a.up ? (((long)n * 2 * H + 2 * r0) * YW + 2 * c0) : (((long)n * H + r0) * W + (a.vstride ? 0 : c0))) *
              (long)a.y_cstride;
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yb, 0, 0x7ffffff0, 0x00020000);
  constexpr int SPW = C::TPN / 64;  // 64-channel slabs per wave column
  const bool splitk = a.ksplit > 1;
  if (a.y_dtype == VM_F32 || splitk) {
    // f32 output (the training step's pre-BN buffers, unet_simple.py:19-27) or a split-K partial: f32 slab staging,
    // 4 channels per 16-byte store; no fused pool / folded resize on this path (host-checked)
    const int ycs = splitk ? a.cout : a.y_cstride;
    const long pix0 = ((long)n * H + r0) * W + (a.vstride ? 0 : c0);
    float* yf = splitk ? a.part + (long)blockIdx.y * a.M * a.cout + pix0 * ycs
                       : reinterpret_cast<float*>(a.y) + a.y_coff + pix0 * ycs;
    const __amdgpu_buffer_rsrc_t yfr = __builtin_amdgcn_make_buffer_rsrc(yf, 0, 0x7ffffff0, 0x00020000);
    const int ycs4 = ycs * 4;
    // split-fp16 x3 output (ConvArgs::ysplit): the same f32 staging, then 8 channels per thread split into [l, h, h]
    const bool ysp = a.ysplit > 0 && !splitk;
    // (a folded upconv's split output: [N, 2H, 2W] pixels from (2 r0, 2 c0), as the bf16 epilogues' yb)
    uint16_t* ys = reinterpret_cast<uint16_t*>(a.y) + a.y_coff +
                   (a.up ? ((long)n * 2 * H + 2 * r0) * YW + 2 * c0 : pix0) * (long)a.y_cstride;
    const __amdgpu_buffer_rsrc_t ysr = __builtin_amdgcn_make_buffer_rsrc(ys, 0, 0x7ffffff0, 0x00020000);
    bool ovf = false;
    for (int sl = 0; sl < BN / 64; ++sl) {
      const int cb = n0 + sl * 64;
      __syncthreads();
      if (wn == sl / SPW) {
#pragma unroll
        for (int fc = 0; fc < FC; ++fc) {
          if (fc / 4 != sl % SPW) continue;
          const int col = (fc % 4) * 16 + 4 * (lane >> 4);
          // (a folded upconv, split output only: the slab is one phase of up_cout channels, ConvArgs::up)
          const int uph = a.up ? cb / a.up_cout : 0;
          const int cbp = cb - uph * a.up_cout, ccap = a.up ? a.up_cout : a.cout;
          float mul[4], add[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int co = min(cbp + col + j, ccap - 1);
            const float sc = (a.scale && !splitk) ? a.scale[co] : 1.f;
            mul[j] = sc;
            add[j] = splitk ? 0.f : (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
          }
#pragma unroll
          for (int fp = 0; fp < FP; ++fp) {
            const int row = C::tpix(wm, fp) + (lane & 15);
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[j] = fmaf(acc[fc][fp][j], mul[j], add[j]);
              if (!splitk && a.act == VM_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
              else if (!splitk && a.act == VM_ACT_SIGMOID) v[j] = sigmoid_precise(v[j]);
            }
            *reinterpret_cast<float4*>(smem + row * C::SR32 + col * 4) = make_float4(v[0], v[1], v[2], v[3]);
          }
        }
      }
      __syncthreads();
      if (ysp) {
        const int S2 = a.ysplit * 2;
        const bool y3 = 3 * a.ysplit <= a.y_cstride;  // the third slab [h again] where the pixel row holds it
#pragma unroll
        for (int it = 0; it < C::BM * 8 / NT; ++it) {
          const int idx = it * NT + tid;
          const int rr = idx >> 3, cq = idx & 7;
          const float4 d0 = *reinterpret_cast<const float4*>(smem + rr * C::SR32 + cq * 32);
          const float4 d1 = *reinterpret_cast<const float4*>(smem + rr * C::SR32 + cq * 32 + 16);
          const float v[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
          const int pr = rr / C::TW, pc = rr % C::TW;
          bool ok;
          int pix = out_pix(pr, pc, ok);
          const int uph = a.up ? cb / a.up_cout : 0;
          const int cbp = cb - uph * a.up_cout;  // (the phase's own channel, a.up)
          ok = ok && cbp + cq * 8 < (a.up ? a.up_cout : a.cout);
          if (a.up) pix = (2 * pr + (uph >> 1)) * YW + 2 * pc + (uph & 1);
          uint4 hv, lv;
          const bool o = split3h_chunk(v, hv, lv);
          ovf |= ok && o;
          const int off = ok ? pix * ycs2 + (cbp + cq * 8) * 2 : OOB;
          const int off1 = ok ? off + S2 : OOB, off2 = ok ? off + 2 * S2 : OOB;
          typedef __attribute__((ext_vector_type(4))) unsigned u4_t;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, lv), ysr, off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, hv), ysr, off1, 0, 0);
          if (y3) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, hv), ysr, off2, 0, 0);
        }
        if (a.py) {
          // the split of the fused 2x2 SAME max-pool (unet.py:32-33) of the staged f32 slab, as the bf16 path's
          // pool: tiles start on even rows / columns, taps past the frame edge never win
          const int PH = (H + 1) >> 1, PW = (W + 1) >> 1;
          const int pr0 = r0 >> 1, pc0 = c0 >> 1;
          uint16_t* pbs = reinterpret_cast<uint16_t*>(a.py) + a.py_coff +
                          (((long)n * PH + pr0) * PW + (a.vstride ? 0 : pc0)) * (long)a.py_cstride + n0;
          const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pbs, 0, 0x7ffffff0, 0x00020000);
          const int P2 = a.psplit * 2;
          constexpr int PTW = C::TW / 2, PITEMS = C::BM / 4 * 8;
#pragma unroll
          for (int it = 0; it < (PITEMS + NT - 1) / NT; ++it) {
            const int idx = it * NT + tid;
            if (idx >= PITEMS) break;
            const int pp = idx >> 3, cq = idx & 7;
            const int pr = pp / PTW, pc = pp % PTW;
            const int rr = 2 * pr * C::TW + 2 * pc;
            bool in;
            const int fpix = out_pix(2 * pr, 2 * pc, in);
            const int fx = fpix % W;
            const bool vh = r0 + 2 * pr + 1 < H, vw = a.vstride ? fx + 1 < W : c0 + 2 * pc + 1 < W;
            auto ld8 = [&](int r, float* f) {
              const float4 q0 = *reinterpret_cast<const float4*>(smem + r * C::SR32 + cq * 32);
              const float4 q1 = *reinterpret_cast<const float4*>(smem + r * C::SR32 + cq * 32 + 16);
              f[0] = q0.x; f[1] = q0.y; f[2] = q0.z; f[3] = q0.w; f[4] = q1.x; f[5] = q1.y; f[6] = q1.z; f[7] = q1.w;
            };
            float m[8], f[8];
            ld8(rr, m);
            if (vw) {
              ld8(rr + 1, f);
#pragma unroll
              for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
            }
            if (vh) {
              ld8(rr + C::TW, f);
#pragma unroll
              for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
            }
            if (vh && vw) {
              ld8(rr + C::TW + 1, f);
#pragma unroll
              for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
            }
            int ppix = pr * PW + pc;
            bool ok = pr0 + pr < PH && pc0 + pc < PW;
            if (a.vstride) {
              ok = in;
              ppix = ((fpix / W - 2 * pr) / H * PH + pr) * PW + fx / 2;
            }
            ok = ok && n0 + sl * 64 + cq * 8 < a.cout;
            uint4 hv, lv;
            split3h_chunk(m, hv, lv);
            const int off = ok ? (ppix * a.py_cstride + sl * 64 + cq * 8) * 2 : OOB;
            typedef __attribute__((ext_vector_type(4))) unsigned u4_t;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, lv), prs, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, hv), prs, ok ? off + P2 : OOB, 0, 0);
            if (3 * a.psplit <= a.py_cstride)
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, hv), prs, ok ? off + 2 * P2 : OOB, 0, 0);
          }
        }
        continue;
      }
#pragma unroll
      for (int it = 0; it < C::BM * 16 / NT; ++it) {
        const int idx = it * NT + tid;
        const int rr = idx >> 4, cq = idx & 15;
        const uint4 d = *reinterpret_cast<const uint4*>(smem + rr * C::SR32 + cq * 16);
        const int pr = rr / C::TW, pc = rr % C::TW;
        bool ok;
        const int pix = out_pix(pr, pc, ok);
        ok = ok && cb + cq * 4 < a.cout;
        const int off = ok ? pix * ycs4 + (cb + cq * 4) * 4 : OOB;
        if (splitk || a.y_vec) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d),
                                                 yfr, off, 0, 0);
        } else {  // a view whose channel offset / stride is not a multiple of 4 (up1[..., 6:30]): dword stores
          __builtin_amdgcn_raw_buffer_store_b32(d.x, yfr, off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(d.y, yfr, off + 4, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(d.z, yfr, off + 8, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(d.w, yfr, off + 12, 0, 0);
        }
      }
    }
    if (ovf && a.ovf) *a.ovf = 1;  // a plain vector store: any writer's 1 is the answer
    return;
  }
  if constexpr (C::REPI_OK) {
    if (a.repi && !a.vstride) {
      // register epilogue: bias / affine / act in registers, chunk_pair turns each pair of 16-channel fragments' lane
      // quads into whole 16-byte chunks stored straight from the lane (no staging, no block barrier); the fused pool
      // takes the row below from the wave's partner fragment and the column partner through DPP quad_perm [1,0,3,2]
      const int col = lane & 15, ckq = lane >> 4;
      const int c16 = (ckq & 1) ? 2 + (ckq >> 1) : ckq >> 1;
      const int PH = (H + 1) >> 1, PWo = (W + 1) >> 1;
      T* pb = a.py ? reinterpret_cast<T*>(a.py) + a.py_coff +
                         (((long)n * PH + (r0 >> 1)) * PWo + (c0 >> 1)) * (long)a.py_cstride + n0
                   : nullptr;
      const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pb, 0, 0x7ffffff0, 0x00020000);
      // head split (a.hd, vm_conv3x3_up2x_head_nhwc): the wave holds all 64 channels of its pixels (one phase of the
      // folded upconv), so conv1_5's per-tap shares of them are 2 MFMAs on the bf16 outputs, as in the pair kernels:
      // A rows = the 9 taps, k ordered like the lane's output channels (2kk + j/4)*16 + 4q + j%4
      constexpr bool HEADOK = FC == 4 && BN == 64;
      // every global load of the epilogue (per-channel constants of all FC fragments, the head filter) is issued
      // here, before any is used, so the block waits for one round trip instead of one per channel group
      const int ccap = a.up ? a.up_cout : a.cout;
      float mul[FC][4], add[FC][4];
#pragma unroll
      for (int f = 0; f < FC; ++f) {
        const int chb = n0 + wn * C::TPN + (f & ~1) * 16;
        const int cb = chb - (a.up ? chb / a.up_cout : 0) * a.up_cout;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = min(cb + (f & 1) * 16 + 4 * ckq + j, ccap - 1);
          const float sc = a.scale ? a.scale[co] : 1.f;
          mul[f][j] = sc;
          add[f][j] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);  // (as the staged epilogue)
        }
      }
      float hwv[2][8];
      if (HEADOK && a.hd) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int hc = (2 * kk + j / 4) * 16 + 4 * ckq + j % 4;
            hwv[kk][j] = col < 9 ? a.hw[col * a.hw_cin + a.hw_coff + hc] : 0.f;
          }
      }
      uint4 hb[FP][2];  // head split: the B operands (bf16 outputs) of each fragment's 2 head MFMAs, used at the end
#pragma unroll
      for (int g2 = 0; g2 < FC / 2; ++g2) {
        const int chb = n0 + wn * C::TPN + g2 * 32;  // first block channel of this 32-channel group
        const int phase = a.up ? chb / a.up_cout : 0;
        const int cb = chb - phase * a.up_cout;
        const int rex = ring_row(a, phase), cex = ring_col(a, phase);
        float v[FP][2][4];
#pragma unroll
        for (int fp = 0; fp < FP; ++fp) {
          uint2 pk[2];
#pragma unroll
          for (int f = 0; f < 2; ++f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float t = fmaf(acc[2 * g2 + f][fp][j], mul[2 * g2 + f][j], add[2 * g2 + f][j]);
              if (a.act == VM_ACT_RELU) t = fmaxf(t, 0.f);
              else if (a.act == VM_ACT_SIGMOID) t = sigmoid_precise(t);
              v[fp][f][j] = t;
            }
            pk[f].x = bf16x2_bits(v[fp][f][0], v[fp][f][1]);
            pk[f].y = bf16x2_bits(v[fp][f][2], v[fp][f][3]);
          }
          hb[fp][g2] = make_uint4(pk[0].x, pk[0].y, pk[1].x, pk[1].y);
          const uint4 d = chunk_pair(pk[0], pk[1]);
          const int tr = C::prow(wm, fp), tc = C::pcol(wm, fp) + col;
          bool ok = r0 + tr < H && c0 + tc < W && cb + c16 * 8 < ccap && !a.y_skip;
          // (fused border pass: the ring belongs to the border blocks; the store is issued all the same)
          if constexpr (BFUSE) ok = ok && r0 + tr != rex && c0 + tc != cex;
          const int pix = a.up ? (2 * tr + (phase >> 1)) * YW + 2 * tc + (phase & 1) : tr * W + tc;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d),
                                                 yrs, ok ? pix * ycs2 + (cb + c16 * 8) * 2 : OOB, 0, 0);
        }
        if (a.py) {  // tiles start on even rows/columns: every 2x2 window lies inside the tile (host: no a.up)
#pragma unroll
          for (int fp = 0; fp < FP; ++fp) {
            if (C::prow(wm, fp) & 1) continue;  // (compile-time per fp: the top row of each window)
            const int tr = C::prow(wm, fp), tc = C::pcol(wm, fp) + col;
            const bool v0 = r0 + tr < H && c0 + tc < W, v1 = r0 + tr + 1 < H && c0 + tc < W;
            float m[2][4];
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float t = v0 ? v[fp][f][j] : -INFINITY;
                if (v1) t = fmaxf(t, v[fp + C::PSTEP][f][j]);
                const float u = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0xB1, 0xF, 0xF, false));
                m[f][j] = fmaxf(t, u);
              }
            uint2 q2[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
              q2[f].x = bf16x2_bits(m[f][0], m[f][1]);
              q2[f].y = bf16x2_bits(m[f][2], m[f][3]);
            }
            const uint4 d = chunk_pair(q2[0], q2[1]);
            const int pr = tr >> 1, pc = tc >> 1;
            const int chl = wn * C::TPN + g2 * 32 + c16 * 8;  // channel relative to n0
            const bool pok = (col & 1) == 0 && v0 && (r0 >> 1) + pr < PH && (c0 >> 1) + pc < PWo && n0 + chl < a.cout;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d),
                                                   prs, pok ? ((pr * PWo + pc) * a.py_cstride + chl) * 2 : OOB, 0, 0);
          }
        }
      }
      if constexpr (HEADOK) {
        if (a.hd) {
          // the head's shares, last: the filter loads issued at the top of the epilogue had the whole epilogue to land.
          // A fragments: rows = taps (9 of 16), k = 8q + j <-> channel (2kk + j/4)*16 + 4q + j%4
          uint4 hwf[2];
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            hwf[kk] = make_uint4(bf16x2_bits(hwv[kk][0], hwv[kk][1]),
                                 bf16x2_bits(hwv[kk][2], hwv[kk][3]),
                                 bf16x2_bits(hwv[kk][4], hwv[kk][5]),
                                 bf16x2_bits(hwv[kk][6], hwv[kk][7]));
          const int phase = a.up ? (n0 + wn * C::TPN) / a.up_cout : 0;
          const int YH = a.up ? 2 * H : H;
          const int hrex = ring_row(a, phase), hcex = ring_col(a, phase);
#pragma unroll
          for (int fp = 0; fp < FP; ++fp) {
            f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
            mma16<T>(hwf[0], hb[fp][0], d);
            mma16<T>(hwf[1], hb[fp][1], d);
            const int tr = C::prow(wm, fp), tc = C::pcol(wm, fp) + col;
            bool hok = ckq < 3 && r0 + tr < H && c0 + tc < W;
            if constexpr (BFUSE) hok = hok && r0 + tr != hrex && c0 + tc != hcex;  // (fused border pass: not the ring)
            if (hok) {
              const int yy = a.up ? 2 * (r0 + tr) + (phase >> 1) : r0 + tr;
              const int xx = a.up ? 2 * (c0 + tc) + (phase & 1) : c0 + tc;
              *reinterpret_cast<f32x4*>(a.hd + (((long)n * YH + yy) * YW + xx) * 12 + 4 * ckq) = d;
            }
          }
        }
      }
      return;
    }
  }
  for (int sl = 0; sl < BN / 64; ++sl) {
    const int phase = a.up ? (n0 + sl * 64) / a.up_cout : 0;
    const int cb = n0 + sl * 64 - phase * a.up_cout;  // first (per-phase) output channel of the slab
    const int ccap = a.up ? a.up_cout : a.cout;
    __syncthreads();
    if (wn == sl / SPW) {
#pragma unroll
      for (int fc = 0; fc < FC; ++fc) {
        if (fc / 4 != sl % SPW) continue;
        const int col = (fc % 4) * 16 + 4 * (lane >> 4);
        float mul[4], add[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = min(cb + col + j, ccap - 1);
          const float sc = a.scale ? a.scale[co] : 1.f;
          mul[j] = sc;
          add[j] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
        }
#pragma unroll
        for (int fp = 0; fp < FP; ++fp) {
          const int row = C::tpix(wm, fp) + (lane & 15);
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = fmaf(acc[fc][fp][j], mul[j], add[j]);
            if (a.act == VM_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
            else if (a.act == VM_ACT_SIGMOID) v[j] = sigmoid_precise(v[j]);
          }
          uint2 pk;
          pk.x = bf16x2_bits(v[0], v[1]);
          pk.y = bf16x2_bits(v[2], v[3]);
          *reinterpret_cast<uint2*>(smem + row * C::SR + col * 2) = pk;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < C::BM * 8 / NT; ++it) {
      const int idx = it * NT + tid;
      const int rr = idx >> 3, cq = idx & 7;
      const uint4 d = *reinterpret_cast<const uint4*>(smem + rr * C::SR + cq * 16);
      const int pr = rr / C::TW, pc = rr % C::TW;
      bool ok;
      int pix = out_pix(pr, pc, ok);
      ok = ok && cb + cq * 8 < ccap;
      if (a.up) pix = (2 * pr + (phase >> 1)) * YW + 2 * pc + (phase & 1);
      const int off = ok ? pix * ycs2 + (cb + cq * 8) * 2 : OOB;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), yrs,
                                             off, 0, 0);
    }
    if (a.py) {
      // fused tf.nn.max_pool 2x2/2 SAME (unet.py:32-33) of the staged slab: tiles start on even rows/columns,
      // so every window lies inside the tile; taps past the frame edge are skipped (never win)
      // (packed frames: W even, so frames start on even virtual columns and every window is inside one frame)
      const int PH = (H + 1) >> 1, PW = (W + 1) >> 1;
      const int pr0 = r0 >> 1, pc0 = c0 >> 1;
      T* pb = reinterpret_cast<T*>(a.py) + a.py_coff +
              (((long)n * PH + pr0) * PW + (a.vstride ? 0 : pc0)) * (long)a.py_cstride + n0;
      const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pb, 0, 0x7ffffff0, 0x00020000);
      constexpr int PTW = C::TW / 2, PITEMS = C::BM / 4 * 8;
#pragma unroll
      for (int it = 0; it < (PITEMS + NT - 1) / NT; ++it) {
        const int idx = it * NT + tid;
        if (idx >= PITEMS) break;
        const int pp = idx >> 3, cq = idx & 7;
        const int pr = pp / PTW, pc = pp % PTW;
        const int rr = 2 * pr * C::TW + 2 * pc;
        bool in;
        const int fpix = out_pix(2 * pr, 2 * pc, in);  // the window's top-left output pixel
        const int fx = fpix % W;                        // its frame column (even)
        const bool vh = r0 + 2 * pr + 1 < H, vw = a.vstride ? fx + 1 < W : c0 + 2 * pc + 1 < W;
        float m[8], f[8];
        Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + rr * C::SR + cq * 16), m);
        if (vw) {
          Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + (rr + 1) * C::SR + cq * 16), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
        }
        if (vh) {
          Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + (rr + C::TW) * C::SR + cq * 16), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
        }
        if (vh && vw) {
          Chunk<T>::unpack(*reinterpret_cast<const uint4*>(smem + (rr + C::TW + 1) * C::SR + cq * 16), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
        }
        int ppix = pr * PW + pc;
        bool ok = pr0 + pr < PH && pc0 + pc < PW;
        if (a.vstride) {  // pooled pixel (frame, pr0 + pr, fx / 2)
          ok = in;
          ppix = ((fpix / W - 2 * pr) / H * PH + pr) * PW + fx / 2;
        }
        ok = ok && n0 + sl * 64 + cq * 8 < a.cout;
        const int off = ok ? (ppix * a.py_cstride + sl * 64 + cq * 8) * 2 : OOB;
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, Chunk<T>::pack(m)), prs, off, 0, 0);
      }
    }
  }
}

// ================================================================ persistent row-slot patch kernel
// The G = 3 patch pipeline above with the tile loop inside the kernel (vm_set_option "patch_persist"): a resident
// grid of 8 x J blocks; block b lives on XCD b % 8 and walks the (pixel tile, 64-channel output tile) items of its
// XCD's band of pixel tiles [lo, hi): round `it` hands walker j the item it*J + j, so the walkers of a round cover
// all output tiles of adjacent pixel tiles (the input patch is fetched from HBM about once per XCD) and, J being a
// multiple of the output tile count, each walker keeps one output tile.  A folded upconv's phases run 9 / 6 / 6 / 4
// taps, so there (ConvArgs::prot) walker j takes item it*J + (j + it) % J instead and cycles through the phases:
// a fixed phase per walker leaves the 9-tap walkers as the tail.  The DMA stream (input granules, weight row slots) runs on
// across tile boundaries: the next item's first granule and weight rows are issued during the current one's last
// steps and land while it finishes its MFMAs and its register epilogue, so an item pays no prologue latency.  The
// per-channel affine of every output channel and the head filter fragments are staged in LDS once per block (the
// epilogue then has no global load, whose vmcnt wait would drain the prefetch).  Every output pixel keeps the
// non-persistent kernel's MFMA sequence and epilogue arithmetic: results are bit-identical.
template <int BN, int WM, int WN, int S, int TH, int MINB, bool UPSKIP>
__global__ __launch_bounds__(64 * WM * WN)
__attribute__((amdgpu_waves_per_eu(MINB * WM * WN < 16 ? 4 : MINB * WM * WN / 4)))  // <= 128 VGPRs
void conv3x3_patch_persist(ConvArgs a) {
  using C = PatchCfg<BN, WM, WN, S, TH, 3>;
  using T = uint16_t;
  static_assert(BN == 64 && WN == 1 && C::REPI_OK && C::FC == 4, "64-channel output tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NW = C::NW, NT = C::NT, FP = C::FP, FC = C::FC, XPW = C::XPW, WPW = C::WPW, R = 3, G = 3;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (a.prio && wave >= 4) __builtin_amdgcn_s_setprio(1);
  const int wm = wave;
  const int H = a.H, W = a.W, cs = a.x_cstride;
  const int th = (H + C::TH - 1) / C::TH, tw = (W + C::TW - 1) / C::TW;
  // the folded upconv's border pass in this launch (ConvArgs::bfuse): the a.bblocks blocks past the walkers run it
  constexpr bool BFUSE = UPSKIP && C::BFUSE_OK;
  if constexpr (BFUSE) {
    const int nwalk = (int)gridDim.x - a.bblocks;
    if (__builtin_expect((int)blockIdx.x >= nwalk, 0)) {  // (out of line: the walkers keep their code layout)
      up2x_border_fused<NT>(a, smem, (int)blockIdx.x - nwalk);
      return;
    }
  }
  const int tn = a.tiles_n, sp = a.tiles_total / tn, CT = tn * BN;
  const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3,
            J = BFUSE ? ((int)gridDim.x - a.bblocks) >> 3 : (int)(gridDim.x >> 3);
  const int lo = (int)((long)xcd * sp / 8), hi = (int)((long)(xcd + 1) * sp / 8);
  const int nitem = (hi - lo) * tn;
  int it = 0, q = jw;
  if (q >= nitem) return;  // (before any barrier: the block has no work)
  // band-local pixel tile i -> pixel tile; with halfskip the band's last-column tiles (s % tw == tw - 1; [0, s) holds
  // s / tw of them) come after its other tiles, in order
  const int nhalf = a.halfskip ? hi / tw - lo / tw : 0, nfull = hi - lo - nhalf;
  auto band_tile = [&](int i) __attribute__((always_inline)) {
    if (!a.halfskip) return lo + i;
    if (i < nfull) {
      const int g = lo - lo / tw + i;  // the g-th tile off the last column
      return g + g / (tw - 1);
    }
    return (lo / tw + i - nfull) * tw + tw - 1;
  };
  // round r's item of walker jw: prot 1 rotates the walkers over the output tiles, prot 2 reverses the order of the
  // walker groups (tn walkers, one per output tile) in odd rounds, so the walkers that end a round late start the
  // next one early (each walker keeps its output tile)
  auto item_of = [&](int r) __attribute__((always_inline)) {
    if (a.prot == 1) return r * J + (jw + r) % J;
    if (a.prot == 2 && (r & 1)) return r * J + J - tn - jw + 2 * (jw % tn);
    return r * J + jw;
  };

  // per-block constants in LDS: mul[CT], add[CT] (f32, output channel order), then the head A fragments [lane][2]
  char* kc = smem + C::MAIN;
  const int ccap = a.up ? a.up_cout : a.cout;
  for (int c = tid; c < CT; c += NT) {
    const int chb = c & ~31;  // (the register epilogue's 32-channel group base and phase)
    const int cb = chb - (a.up ? chb / a.up_cout : 0) * a.up_cout;
    const int co = min(cb + (c & 31), ccap - 1);
    const float sc = a.scale ? a.scale[co] : 1.f;
    reinterpret_cast<float*>(kc)[c] = sc;
    reinterpret_cast<float*>(kc)[CT + c] = (a.bias ? a.bias[co] : 0.f) * sc + (a.shift ? a.shift[co] : 0.f);
  }
  char* kh = kc + CT * 8;
  const int col = lane & 15, ckq = lane >> 4;
  if (a.hd && tid < 64) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      float hv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int hc = (2 * kk + j / 4) * 16 + 4 * ckq + j % 4;
        hv[j] = col < 9 ? a.hw[col * a.hw_cin + a.hw_coff + hc] : 0.f;
      }
      *reinterpret_cast<uint4*>(kh + (lane * 2 + kk) * 16) =
          make_uint4(bf16x2_bits(hv[0], hv[1]),
                     bf16x2_bits(hv[2], hv[3]),
                     bf16x2_bits(hv[4], hv[5]),
                     bf16x2_bits(hv[6], hv[7]));
    }
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t wrs = w_rsrc<T>(a, 0);  // (item weights at n0 * K_pad * 2 bytes: host-checked)
  const int lrow = lane >> 2, lpos = lane & 3;
  int woff[WPW];
  int w_n = 0;
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int piece = wave + i * NW;
    const int row = piece * 16 + lrow;
    const int lq = (swz<64>(row, lpos) - row * 64) >> 4;
    woff[i] = (row * a.K_pad + lq * 8) * 2;
    if (piece < C::WP) ++w_n;
  }
  int x_n = 0;
#pragma unroll
  for (int i = 0; i < XPW; ++i)
    if (wave + i * NW < C::XP) ++x_n;

  // input DMA state of the tile whose granules are being fetched (switches to the next tile at the last granule)
  __amdgpu_buffer_rsrc_t xrs;
  int xoff[XPW];
  auto set_xtile = [&](int s) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int lrow = ln >> 2, lpos = ln & 3;
    const int n = s / (th * tw), srem = s - n * th * tw;
    const int r0 = (srem / tw) * C::TH, c0 = (srem - (srem / tw) * tw) * C::TW;
    const T* xb = reinterpret_cast<const T*>(a.x) + a.x_coff + ((long)n * H + r0 - 1) * (long)W * cs;
    xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(xb), 0, 0x7ffffff0, 0x00020000);
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int row = (wave + i * NW) * 16 + lrow;
      const int lq = (swz<64>(row, lpos) - row * 64) >> 4;
      const int pr = row / C::PW, pc = row - pr * C::PW;
      int h = r0 - 1 + pr, w = c0 - 1 + pc;
      if (a.up) {  // folded 2x resize: the low-res frame's edge is replicated (as conv3x3_patch)
        h = min(h, H - 1);
        w = min(w, W - 1);
      }
      const bool ok = row < C::PPIX && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      xoff[i] = ok ? (((h - r0 + 1) * W + w) * cs + lq * 8) * 2 : OOB;
    }
  };
  const int nch = a.cin_pad / 32, nsr = nch * R;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  const uint32_t wring = lds0 + 2 * C::PB;
  auto issue_x = [&](int cc, int buf, bool real) {
#pragma unroll
    for (int i = 0; i < XPW; ++i)
      if (wave + i * NW < C::XP)
        glds16(xrs, lds0 + buf * C::PB + (wave + i * NW) * 1024, real ? xoff[i] + (int)src_chan(a, cc * 32) * 2 : OOB);
  };
  auto issue_w = [&](int s, int slot, bool real, int wb) {  // wb: the item's weight byte offset
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < WPW; ++i)
        if (wave + i * NW < C::WP)
          glds16(wrs, wring + (slot * G + g) * C::WSLOT + (wave + i * NW) * 1024,
                 real ? woff[i] + wb + (s * G + g) * 64 : OOB);
  };

  int boff[FC], abase[FP];
#pragma unroll
  for (int f = 0; f < FC; ++f) boff[f] = 2 * C::PB + swz<64>(f * 16 + (lane & 15), lane >> 4);
#pragma unroll
  for (int f = 0; f < FP; ++f) abase[f] = C::prow(wm, f) * C::PW + C::pcol(wm, f) + (lane & 15);
  const int ck = lane >> 4;
  auto frags = [&](uint4 (&av)[FC], uint4 (&bv)[FP], int slot, int buf, int tap) {
    const char* wp = smem + (slot * G + tap % G) * C::WSLOT;
    const char* xp = smem + buf * C::PB;
#pragma unroll
    for (int f = 0; f < FC; ++f) av[f] = *reinterpret_cast<const uint4*>(wp + boff[f]);
    const int toff = (tap / 3) * C::PW + tap % 3;
#pragma unroll
    for (int f = 0; f < FP; ++f) bv[f] = *reinterpret_cast<const uint4*>(xp + swz<64>(abase[f] + toff, ck));
  };
  // counted DMA wait, then lgkmcnt(0): this wave's fragment reads of the ring slot / patch buffer that the DMAs
  // issued right after the barrier refill must have returned before the barrier — the MFMAs consuming them may be
  // scheduled past it (seen in the 4 x 32 folded-upconv instantiation: under a second process on the GPU the refill
  // overtook a queued ds_read about once per 100 frames)
  auto sync = [&](int n) {
    wait_vm(n);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  // stores of one epilogue (counted into the first waits of the next tile: they are younger than the weight rows
  // issued before it); the head's conditional stores are not counted (waiting longer is safe)
  int e_st = 2 * FP;
  if (a.py) {
#pragma unroll
    for (int fp = 0; fp < FP; ++fp) e_st += (C::prow(wm, fp) & 1) ? 0 : 2;
  }

  const int ycs2 = a.y_cstride * 2;
  const int YW = a.up ? 2 * W : W;
  const int PH = (H + 1) >> 1, PWo = (W + 1) >> 1;
  auto epilogue = [&](const f32x4 (&acc)[FC][FP], int s, int n0) {
    // lane-derived values from an opaque copy of the lane id: recomputed per tile instead of held across the loop
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int col = ln & 15, ckq = ln >> 4;
    const int n = s / (th * tw), srem = s - n * th * tw;
    const int r0 = (srem / tw) * C::TH, c0 = (srem - (srem / tw) * tw) * C::TW;
    T* yb = reinterpret_cast<T*>(a.y) + a.y_coff +
            (a.up ? (((long)n * 2 * H + 2 * r0) * YW + 2 * c0) : (((long)n * H + r0) * W + c0)) * (long)a.y_cstride;
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yb, 0, 0x7ffffff0, 0x00020000);
    const int c16 = (ckq & 1) ? 2 + (ckq >> 1) : ckq >> 1;
    T* pb = a.py ? reinterpret_cast<T*>(a.py) + a.py_coff +
                       (((long)n * PH + (r0 >> 1)) * PWo + (c0 >> 1)) * (long)a.py_cstride + n0
                 : nullptr;
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pb, 0, 0x7ffffff0, 0x00020000);
    f32x4 dh[FP];  // head split: conv1_5's per-tap partials, accumulated over the two 32-channel groups
#pragma unroll
    for (int fp = 0; fp < FP; ++fp) dh[fp] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g2 = 0; g2 < FC / 2; ++g2) {
      const int chb = n0 + g2 * 32;
      const int phase = a.up ? chb / a.up_cout : 0;
      const int cb = chb - phase * a.up_cout;
      const int rex = ring_row(a, phase), cex = ring_col(a, phase);
      float v[FP][2][4];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const float4 m4 = *reinterpret_cast<const float4*>(kc + (n0 + (2 * g2 + f) * 16 + 4 * ckq) * 4);
        const float4 a4 = *reinterpret_cast<const float4*>(kc + (CT + n0 + (2 * g2 + f) * 16 + 4 * ckq) * 4);
        const float mul[4] = {m4.x, m4.y, m4.z, m4.w}, add[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int fp = 0; fp < FP; ++fp)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float t = fmaf(acc[2 * g2 + f][fp][j], mul[j], add[j]);
            if (a.act == VM_ACT_RELU) t = fmaxf(t, 0.f);
            else if (a.act == VM_ACT_SIGMOID) t = sigmoid_precise(t);
            v[fp][f][j] = t;
          }
      }
#pragma unroll
      for (int fp = 0; fp < FP; ++fp) {
        uint2 pk[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          pk[f].x = bf16x2_bits(v[fp][f][0], v[fp][f][1]);
          pk[f].y = bf16x2_bits(v[fp][f][2], v[fp][f][3]);
        }
        if (a.hd)  // (the same two MFMAs, in the same order, as the register epilogue's head split)
          mma16<T>(*reinterpret_cast<const uint4*>(kh + (ln * 2 + g2) * 16),
                   make_uint4(pk[0].x, pk[0].y, pk[1].x, pk[1].y), dh[fp]);
        const uint4 d = chunk_pair(pk[0], pk[1]);
        const int tr = C::prow(wm, fp), tc = C::pcol(wm, fp) + col;
        bool ok = r0 + tr < H && c0 + tc < W && cb + c16 * 8 < ccap && !a.y_skip;
        // (fused border pass: the ring belongs to the border blocks; the store is issued, and counted, all the same)
        if constexpr (BFUSE) ok = ok && r0 + tr != rex && c0 + tc != cex;
        const int pix = a.up ? (2 * tr + (phase >> 1)) * YW + 2 * tc + (phase & 1) : tr * W + tc;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d), yrs,
                                               ok ? pix * ycs2 + (cb + c16 * 8) * 2 : OOB, 0, 0);
      }
      if (a.py) {
#pragma unroll
        for (int fp = 0; fp < FP; ++fp) {
          if (C::prow(wm, fp) & 1) continue;
          const int tr = C::prow(wm, fp), tc = C::pcol(wm, fp) + col;
          const bool v0 = r0 + tr < H && c0 + tc < W, v1 = r0 + tr + 1 < H && c0 + tc < W;
          float m[2][4];
#pragma unroll
          for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float t = v0 ? v[fp][f][j] : -INFINITY;
              if (v1) t = fmaxf(t, v[fp + C::PSTEP][f][j]);
              const float u = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0xB1, 0xF, 0xF, false));
              m[f][j] = fmaxf(t, u);
            }
          uint2 q2[2];
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            q2[f].x = bf16x2_bits(m[f][0], m[f][1]);
            q2[f].y = bf16x2_bits(m[f][2], m[f][3]);
          }
          const uint4 d = chunk_pair(q2[0], q2[1]);
          const int pr = tr >> 1, pc = tc >> 1;
          const int chl = g2 * 32 + c16 * 8;
          const bool pok = (col & 1) == 0 && v0 && (r0 >> 1) + pr < PH && (c0 >> 1) + pc < PWo && n0 + chl < a.cout;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, d),
                                                 prs, pok ? ((pr * PWo + pc) * a.py_cstride + chl) * 2 : OOB, 0, 0);
        }
      }
    }
    if (a.hd) {
      const int phase = a.up ? n0 / a.up_cout : 0;
      const int YH = a.up ? 2 * H : H;
      const int hrex = ring_row(a, phase), hcex = ring_col(a, phase);
#pragma unroll
      for (int fp = 0; fp < FP; ++fp) {
        const f32x4 d = dh[fp];
        const int tr = C::prow(wm, fp), tc = C::pcol(wm, fp) + col;
        bool hok = ckq < 3 && r0 + tr < H && c0 + tc < W;
        if constexpr (BFUSE) hok = hok && r0 + tr != hrex && c0 + tc != hcex;  // (fused border pass: not the ring)
        if (hok) {  // (uncounted stores: waiting longer is safe)
          const int yy = a.up ? 2 * (r0 + tr) + (phase >> 1) : r0 + tr;
          const int xx = a.up ? 2 * (c0 + tc) + (phase & 1) : c0 + tc;
          *reinterpret_cast<f32x4*>(a.hd + (((long)n * YH + yy) * YW + xx) * 12 + 4 * ckq) = d;
        }
      }
    }
  };

  const int wstep = a.K_pad * 2 * BN;  // weight bytes of one output tile
  int st = band_tile(q / tn), n0 = (q % tn) * BN;
  set_xtile(st);
  int gcnt = 0;  // granules issued so far (input buffer parity)
  issue_x(0, 0, true);
#pragma unroll
  for (int j = 0; j < S - 1; ++j) issue_w(j, j, j < nsr, (q % tn) * wstep);
  int slot = 0;
  bool first = true;
  for (;;) {
    const int qn = item_of(it + 1);
    const bool more = qn < nitem;
    const int stn = more ? band_tile(qn / tn) : st, wbn = more ? (qn % tn) * wstep : 0, wb = (n0 / BN) * wstep;
    // a last-column tile of a halfskip frame: the right-half waves' pixels are all outside it (stores masked as ever)
    const bool idle = a.halfskip && (wm & 1) && st % tw == tw - 1;
    const int up_phase = UPSKIP && a.up && n0 / a.up_cout == (n0 + BN - 1) / a.up_cout ? n0 / a.up_cout : 0;
    const bool skip_r0 = (up_phase >> 1) != 0 && (a.upmask & 1), skip_c0 = (up_phase & 1) != 0 && (a.upmask & 2);
    f32x4 acc[FC][FP];
#pragma unroll
    for (int i = 0; i < FC; ++i)
#pragma unroll
      for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cc = 0; cc < nch; ++cc) {
      const int buf = gcnt & 1;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = cc * R + r;
        int nw = (S - 2) * G * w_n + ((r >= 1 && r <= S - 2) ? x_n : 0);
        if (!first && k < S - 1) nw += e_st;
        sync(nw);
        if (r == 0) {
          if (cc + 1 < nch) {
            issue_x(cc + 1, buf ^ 1, true);
          } else {  // the next item's first granule (a dummy past the walk's end)
            if (more && stn != st) set_xtile(stn);
            issue_x(0, buf ^ 1, more);
          }
        }
        int ws = k + S - 1;
        if (ws < nsr) {
          issue_w(ws, slot + S - 1 - (slot + S - 1 >= S ? S : 0), true, wb);
        } else {
          issue_w(ws - nsr, slot + S - 1 - (slot + S - 1 >= S ? S : 0), more, wbn);
        }
        if (!(UPSKIP && skip_r0 && r == 0) && !idle) {
          uint4 av[2][FC], bv[2][FP];
          frags(av[0], bv[0], slot, buf, r * G);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            if (g + 1 < G) frags(av[(g + 1) & 1], bv[(g + 1) & 1], slot, buf, r * G + g + 1);
            if (!(UPSKIP && skip_c0 && g == 0)) {
#pragma unroll
              for (int fc = 0; fc < FC; ++fc)
#pragma unroll
                for (int fp = 0; fp < FP; ++fp) mma16<T>(av[g & 1][fc], bv[g & 1][fp], acc[fc][fp]);
            }
          }
        }
        slot = slot + 1 == S ? 0 : slot + 1;
      }
      ++gcnt;
    }
    epilogue(acc, st, n0);
    if (!more) break;
    ++it;
    q = qn;
    st = stn;
    n0 = (qn % tn) * BN;
    first = false;
  }
}

// ================================================================ split-K reduction
// out[p][c] = act((sum_s part[s][p][c]) * scale + bias*scale + shift), the splits summed in order (deterministic);
// one thread per 4 output channels of a pixel
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int ks, long M, int cout,
                                                            const float* bias, const float* scale, const float* shift,
                                                            int act, void* y, int y_dtype, int ycs, int ycoff,
                                                            int ysplit = 0, int* ovf = nullptr) {
  const int c4 = (cout + 3) / 4;
  const long total = M * c4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long p = i / c4;
    const int c = (int)(i - p * c4) * 4;
    float4 s = *reinterpret_cast<const float4*>(part + p * cout + c);
    for (int k = 1; k < ks; ++k) {
      const float4 t = *reinterpret_cast<const float4*>(part + (long)k * M * cout + p * cout + c);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c + j >= cout) break;
      const float sc = scale ? scale[c + j] : 1.f;
      float t = fmaf(v[j], sc, (bias ? bias[c + j] : 0.f) * sc + (shift ? shift[c + j] : 0.f));
      if (act == VM_ACT_RELU) t = fmaxf(t, 0.f);
      else if (act == VM_ACT_SIGMOID) t = sigmoid_precise(t);
      const long o = p * ycs + ycoff + c + j;
      if (ysplit > 0) {  // split-fp16 x3 output (ConvArgs::ysplit): [l, h, h] at 0, ysplit, 2 * ysplit
        const _Float16 h = (_Float16)t;
        const _Float16 l = (_Float16)(t - (float)h);
        uint16_t* yo = reinterpret_cast<uint16_t*>(y) + o;
        yo[0] = __builtin_bit_cast(uint16_t, l);
        yo[ysplit] = __builtin_bit_cast(uint16_t, h);
        if (3 * ysplit <= ycs) yo[2 * ysplit] = __builtin_bit_cast(uint16_t, h);
        if (!(fabsf(t) < 65520.f) && ovf) *ovf = 1;
      } else if (y_dtype == VM_F32) {
        reinterpret_cast<float*>(y)[o] = t;
      } else {
        reinterpret_cast<uint16_t*>(y)[o] = f2bf(t);
      }
    }
  }
}

int launch_splitk_reduce(const ConvArgs& a, hipStream_t st) {
  const long work = a.M * ((a.cout + 3) / 4);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid_for(work, 256)), dim3(256), 0, st, a.part, a.ksplit, a.M, a.cout,
                     a.bias, a.scale, a.shift, a.act, a.y, a.y_dtype, a.y_cstride, a.y_coff, a.ysplit, a.ovf);
  return check_launch("splitk_reduce");
}

// ================================================================ launchers and routing
// the border blocks a folded kernel of nt threads adds to its grid (ConvArgs::bfuse): one 4-wave group per 16
// border pixels x 64 output channels, nt / 256 groups per block; left off where the grid would not fit
static void plan_border_fuse(ConvArgs& a, int nt) {
  a.bfuse = a.bblocks = 0;
  // (the border blocks address the low-res frame with 32-bit element offsets)
  if (!a.up || !a.bw || a.up_cout % 64 || (long)a.H * a.W * a.x_cstride + a.cin_pad > 0x7fffffffL) return;
  const long nb = 4L * a.W + 2 * (2L * a.H - 2);
  const long groups = (a.bframes * nb + 15) / 16 * (a.up_cout / 64), per = nt / 256;
  const long blocks = (groups + per - 1) / per;
  if (blocks <= 0 || a.tiles_total + blocks > 0x7fffffffL) return;
  a.bfuse = 1;
  a.bblocks = (int)blocks;
}

template <int BN, int WM, int WN, int S, int TH = 8, int MINB = 1, int UNR = 9, bool PF = false, int ABL = 0,
          bool FIRST = false, int G = 1, bool UPSKIP = false>
static int launch_patch(ConvArgs& a, hipStream_t st) {
  using C = PatchCfg<BN, WM, WN, S, TH, G>;
  static_assert(!(FIRST && PF), "FIRST uses the plain pipeline");
  constexpr int lds = FIRST ? C::LDS_FIRST : C::LDS;
  // fp16 operands (ConvArgs::f16, the split-fp16 forward): the same tiling on v_mfma_f32_16x16x32_f16
  constexpr bool F16_OK = !FIRST && ABL == 0;
  const bool f16 = F16_OK && a.f16;
  if (a.f16 && !F16_OK) return fail(VM_EUNSUPPORTED, "conv3x3_patch: no fp16 instantiation of this tiling");
  static bool attr_set = false, attr16_set = false;
  if (!(f16 ? attr16_set : attr_set)) {
    const void* fn = f16 ? reinterpret_cast<const void*>(
                               &conv3x3_patch<BN, WM, WN, S, TH, MINB, UNR, PF, ABL, FIRST, G, UPSKIP, f16_t>)
                         : reinterpret_cast<const void*>(
                               &conv3x3_patch<BN, WM, WN, S, TH, MINB, UNR, PF, ABL, FIRST, G, UPSKIP>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return fail(VM_EHIP, "hipFuncSetAttribute(patch): %s", hipGetErrorString(e));
    (f16 ? attr16_set : attr_set) = true;
  }
  const long N = a.M / ((long)a.H * a.W);
  const long sp = a.vstride ? ((a.H + C::TH - 1) / C::TH) * (long)((a.vW + C::TW - 1) / C::TW)
                            : N * ((a.H + C::TH - 1) / C::TH) * ((a.W + C::TW - 1) / C::TW);
  a.tiles_n = (a.cout + BN - 1) / BN;
  a.bfuse = a.bblocks = 0;
  a.repi = (int)g_opt.patch_repi;
  a.upmask = (int)g_opt.up_skip_mask;
  a.prio = (int)g_opt.conv_prio;
  if (sp * a.tiles_n > 0x7fffffffL) return fail(VM_EUNSUPPORTED, "conv3x3: too many tiles");
  a.tiles_total = (int)(sp * a.tiles_n);
  // channel-banded tile order (ConvArgs::cband) for weight-heavy layers: the whole filter exceeds an XCD's 4 MB L2
  // and its output tiles split evenly over the 8 XCDs.  cband option: 0 off, 1 folded upconvs, 2 any such layer
  const long wbytes = (long)a.cout_pad * a.K_pad * 2;
  a.cband = (g_opt.cband >= (a.up ? 1 : 2)) && !FIRST && BN == 64 && a.tiles_n % 8 == 0 && wbytes >= g_opt.cband_bytes
                ? a.tiles_n / 8 : 0;
  a.ngroup = !a.cband && g_opt.ngroup > 0 && a.tiles_n > g_opt.ngroup && a.tiles_n % g_opt.ngroup == 0 && wbytes >= g_opt.cband_bytes
                 ? (int)g_opt.ngroup : 0;
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_patch<%d, %d, %d, %d, %d, %d, %d, %s, %d, %s, %d, %s%s>",
           BN, WM, WN, S, TH, MINB, UNR, PF ? "true" : "false", ABL, FIRST ? "true" : "false", G,
           UPSKIP ? "true" : "false", f16 ? ", vm::f16_t" : "");
  if constexpr (UPSKIP && !FIRST && C::BFUSE_OK) {
    if (a.bwant >= 1 && !f16 && a.repi && !a.vstride && a.ksplit <= 1 && a.y_dtype == VM_BF16) plan_border_fuse(a, C::NT);
  }
  const dim3 grid(a.tiles_total + a.bblocks, a.ksplit > 1 ? a.ksplit : 1);
  if constexpr (F16_OK) {
    if (f16) {
      hipLaunchKernelGGL((conv3x3_patch<BN, WM, WN, S, TH, MINB, UNR, PF, ABL, FIRST, G, UPSKIP, f16_t>), grid,
                         dim3(C::NT), lds, st, a);
      return check_launch("conv3x3_patch");
    }
  }
  hipLaunchKernelGGL((conv3x3_patch<BN, WM, WN, S, TH, MINB, UNR, PF, ABL, FIRST, G, UPSKIP>), grid, dim3(C::NT), lds,
                     st, a);
  return check_launch("conv3x3_patch");
}

// conv1_1 -> conv1_2 in the streaming kernel (a.w1 / a.bias1): 4 x 32 px tiles for grids under 512 blocks
int launch_patch_first(ConvArgs& a, hipStream_t st) {
  const long sp = a.M / ((long)a.H * a.W) * ((a.H + 7) / 8) * ((a.W + 31) / 32);
  if (sp * ((a.cout + 63) / 64) < 512) return launch_patch<64, 4, 1, 6, 4, 1, 9, false, 0, true>(a, st);
  return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 0, true>(a, st);
}

// persistent row-slot patch kernel (conv3x3_patch_persist): a resident grid of 8 XCD bands x J walkers, on grids of
// >= g_opt.persist_rounds full rounds of items (a shorter walk gains no prologue overlap and its last round is ragged);
// the callers check persist_ok, then persist_launch returns 1 when the grid is too small (the caller falls back)
static bool persist_ok(const ConvArgs& a) {
  return g_opt.patch_persist && g_opt.patch_repi && a.ksplit <= 1 && !a.vstride && a.y_dtype == VM_BF16 &&
         (!a.up || a.up_cout % 32 == 0) && (long)a.cout_pad * a.K_pad * 2 < 0x7fff0000L;
}
template <int BN, int WM, int WN, int S, int TH, int MINB, bool UPSKIP>
static int launch_patch_persist(ConvArgs& a, hipStream_t st) {
  using C = PatchCfg<BN, WM, WN, S, TH, 3>;
  const int tn = (a.cout + BN - 1) / BN;
  const int lds = C::MAIN + tn * BN * 8 + 2048;  // + per-channel affine of every output tile + head fragments
  constexpr int lds_max = 160 * 1024 / (160 * 1024 / C::MAIN);  // as many blocks per CU as the streaming kernel
  if (lds > lds_max) return 1;
  const void* fn = reinterpret_cast<const void*>(&conv3x3_patch_persist<BN, WM, WN, S, TH, MINB, UPSKIP>);
  static int dev_seen = -1, per_cu = 0, n_cu = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != dev_seen) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, C::NT, lds_max);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return fail(VM_EHIP, "conv3x3_patch_persist: %s", hipGetErrorString(e));
    dev_seen = dev;
  }
  const long N = a.M / ((long)a.H * a.W);
  const long sp = N * ((a.H + C::TH - 1) / C::TH) * ((a.W + C::TW - 1) / C::TW);
  const long resident = (long)per_cu * n_cu;
  // where it pays (same-box A/B per layer of the 1080p forward, 2 blocks per CU = 512 resident): a folded upconv
  // (phases of 9 / 6 / 6 / 4 taps, rotated over the walkers) needs >= g_opt.persist_up_rounds rounds of items to even
  // out (upconv_3 / upconv_4, 8 / 16 rounds: -3 % / -18 %; upconv_2, 4 rounds: +13 %); a plain conv gains on grids of
  // 2..3 rounds (conv4_x, conv5 of 1024 / 512 channels: -2..-3 %) and on the 2-granule K loop (conv2_1: -9 %), and
  // loses a little on 4..8 rounds of 4..8 granules (conv2_2, conv3_2, conv3_3: +2..+3 %)
  const long items = sp * tn;
  bool use;
  if (a.up) use = items >= g_opt.persist_up_rounds * resident;
  else use = items >= g_opt.persist_rounds * resident && (items < 3 * resident || a.cin_pad <= 64 || g_opt.persist_rounds == 0 ||
                                                        g_opt.persist_all);
  if (sp < 8 || resident < 8 || !use || items > 0x7fffffffL) return 1;
  a.tiles_n = tn;
  a.prot = g_opt.persist_rot == 0 ? (a.up ? 1 : 0) : g_opt.persist_rot == 1 ? 1 : 0;
  // a last tile column of <= 16 frame columns (135 x 240: 7.5 tiles) costs half a tile: walk those tiles last and
  // serpentine the rounds, so the 2.125 rounds of items of the conv4 level end after ~2.2 tile times instead of 3
  const long J_ = resident / 8;
  a.halfskip = g_opt.persist_half && C::REMAP && a.W % C::TW != 0 && a.W % C::TW <= 16 && a.W > C::TW;
  if (a.halfskip && !a.prot && J_ % tn == 0) a.prot = 2;
  a.repi = 1;
  a.prio = (int)g_opt.conv_prio;
  a.upmask = (int)g_opt.up_skip_mask;
  a.tiles_total = (int)(sp * tn);
  const long J = resident / 8;  // walkers per XCD band (every band has >= 2 rounds of items)
  snprintf(g_last_kernel, sizeof g_last_kernel, "vm::conv3x3_patch_persist<%d, %d, %d, %d, %d, %d, %s>", BN, WM, WN, S,
           TH, MINB, UPSKIP ? "true" : "false");
  if constexpr (UPSKIP && C::BFUSE_OK) {
    if (a.bwant >= 2) plan_border_fuse(a, C::NT);
  }
  hipLaunchKernelGGL((conv3x3_patch_persist<BN, WM, WN, S, TH, MINB, UPSKIP>), dim3((unsigned)(8 * J + a.bblocks)),
                     dim3(C::NT), lds, st, a);
  return check_launch("conv3x3_patch_persist");
}

// a shipped tiling: the folded-upconv instantiation (zero phase taps skipped, row-slot pipeline G = 3) for a.up,
// else the plain one
template <int BN, int WM, int WN, int S, int TH = 8, int MINB = 1, int UNR = 9, bool PF = false, int ABL = 0,
          bool FIRST = false, int G = 1>
static int launch_patch_up(ConvArgs& a, hipStream_t st) {
  if (G > 1 && a.up && g_opt.up_skip) return launch_patch<BN, WM, WN, S, TH, MINB, UNR, PF, ABL, FIRST, G, (G > 1)>(a, st);
  return launch_patch<BN, WM, WN, S, TH, MINB, UNR, PF, ABL, FIRST, G, false>(a, st);
}

// split-K plan of a patch-kernel conv: small grids (under g_opt.splitk_tiles 4 x 32 pixel x 64 channel tiles) with a
// long K loop split the channel granules so that ~1024 blocks run; 1 = no split.  Deterministic in the geometry,
// so vm_conv3x3_workspace_bytes and the launch agree.
int splitk_plan(long n, int h, int w, int cin_pad, int cout) {
  const long tiles = n * ((h + 3) / 4) * ((w + 31) / 32) * ((cout + 63) / 64);
  const int nch = cin_pad / 32;
  if (tiles >= g_opt.splitk_tiles || nch < 4 || tiles <= 0) return 1;
  int ks = (int)((1024 + tiles - 1) / tiles);
  if (ks > nch / 2) ks = nch / 2;
  if (ks < 2) return 1;
  const int per = (nch + ks - 1) / ks;
  return (nch + per - 1) / per;  // every split non-empty
}

bool patch_ok(const ConvArgs& a, size_t tsize) {
  // bf16 output (16-byte aligned view), or f32 output without the fused pool / folded resize (cout multiple of 4;
  // dword stores when the view is not 16-byte aligned)
  const bool yok = a.y_dtype == VM_BF16 ? (a.cout & 7) == 0 && a.y_vec
                                        : (a.y_dtype == VM_F32 && (!a.py || a.ysplit) && (!a.up || a.ysplit) &&
                                           (a.cout & 3) == 0);
  return tsize == 2 && a.chunk_major && a.cin_pad % 32 == 0 && yok && a.act != VM_ACT_SOFTMAX &&
         (a.x_src_c <= 0 || a.x_src_c % 32 == 0);
}

// packed frames (ConvArgs::vstride): a batch of narrow frames tiled as one virtual image when that saves >= 10 % of
// the column tiles (8 x 320^2 training crops: the 80 / 40 / 20-wide tower levels, 3 / 2 / 1 tiles per frame -> 2.6
// / 1.3 / 0.7).  Results are bit-identical (every output keeps its K loop); only which pixels share a block changes.
// Off for the folded upconvs, odd widths under a fused pool, and where the batch's 32-bit byte offsets would wrap.
static void plan_packed_frames(ConvArgs& a) {
  a.vstride = a.vW = 0;
  const long N = a.M / ((long)a.H * a.W);
  if (!g_opt.pack_frames || a.up || N < 2 || (a.py && (a.W & 1))) return;
  const long plain = N * ((a.W + 31) / 32), packed = (N * (a.W + 2) + 31) / 32;
  if (packed * 10 > plain * 9 || N * (a.W + 2) > 0x7fffffffL) return;
  const long lim = 0x7ffffff0L;
  long xspan = a.M * a.x_cstride * 2;
  if (a.x_src_c > 0) xspan += (long)(a.cin_pad / a.x_src_c - 1) * a.x_src_stride * 2;
  const long yspan = a.ksplit > 1 ? a.M * a.cout * 4 : a.M * a.y_cstride * (a.y_dtype == VM_F32 ? 4 : 2);
  const long pspan = a.py ? N * ((a.H + 1) / 2) * ((a.W + 1) / 2) * a.py_cstride * 2 : 0;
  if (xspan >= lim || yspan >= lim || pspan >= lim) return;
  a.vstride = a.W + 2;
  a.vW = (int)(N * (a.W + 2));
}

int dispatch_patch(ConvArgs& a, hipStream_t st) {
  plan_packed_frames(a);
  if (a.ksplit > 1) {  // split-K: the 4 x 32-pixel row-slot config, then the fixed-order reduction
    int rc = launch_patch<64, 4, 1, 2, 4, 2, 9, false, 0, false, 3>(a, st);
    return rc ? rc : launch_splitk_reduce(a, st);
  }
#ifdef VM_STUDY
  switch (g_opt.patch_ablate) {  // timing experiments on the default tiling (results are garbage)
    case 1: return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 1>(a, st);
    case 2: return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 2>(a, st);
    case 3: return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 3>(a, st);
    case 4: return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 4>(a, st);
    case 6: return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 6>(a, st);
    case 7: return launch_patch<64, 8, 1, 6, 8, 1, 9, false, 7>(a, st);
    // the same ablations on the row-slot default (64 x 8 waves, 2-slot ring of kernel rows)
    case 11: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 1, false, 3>(a, st);
    case 12: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 2, false, 3>(a, st);
    case 14: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 4, false, 3>(a, st);
    case 16: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 6, false, 3>(a, st);
    case 18: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 8, false, 3>(a, st);
    case 19: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 5, false, 3>(a, st);
    case 20: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 16, false, 3>(a, st);
    case 21: return launch_patch<64, 8, 1, 2, 8, 1, 9, false, 32, false, 3>(a, st);
    case 22: return launch_patch<64, 8, 1, 2, 8, 2, 9, false, 16, false, 3>(a, st);
    default: break;
  }
#endif
  switch (g_opt.patch_cfg) {
    // the tilings the dispatcher below picks (the only ones in the shipped library)
    case 19: return launch_patch_up<64, 8, 1, 3, 8, 1, 9, false, 0, false, 3>(a, st);
    case 22: return launch_patch_up<64, 8, 1, 2, 8, 1, 9, false, 0, false, 3>(a, st);
    case 25: return launch_patch_up<64, 4, 1, 2, 4, 2, 9, false, 0, false, 3>(a, st);
    case 30: return launch_patch_up<128, 4, 2, 3, 8, 2>(a, st);
#ifdef VM_STUDY
    // study build only (make study): every tiling of the r01/r02 sweeps (scripts/sweep.sh, scripts/conv_study.sh)
    case 1: return launch_patch<64, 4, 1, 6>(a, st);
    case 2: return launch_patch<128, 2, 2, 6>(a, st);
    case 3: return launch_patch<128, 4, 2, 4>(a, st);
    case 4: return launch_patch<128, 4, 2, 6>(a, st);
    case 5: return launch_patch<64, 8, 1, 6>(a, st);
    case 6: return launch_patch<64, 8, 1, 6, 8, 1, 9, true>(a, st);
    case 7: return launch_patch<64, 8, 1, 4, 8, 1, 9, true>(a, st);
    case 8: return launch_patch<128, 4, 1, 4, 8, 2>(a, st);
    case 9: return launch_patch<128, 2, 2, 4, 8, 2>(a, st);
    case 10: return launch_patch<256, 4, 2, 3, 8, 1>(a, st);
    case 11: return launch_patch<64, 8, 1, 6, 4>(a, st);
    case 12: return launch_patch<64, 4, 1, 6, 4>(a, st);
    case 13: return launch_patch<128, 4, 1, 4, 8, 2, 9, true>(a, st);
    case 14: return launch_patch<128, 4, 1, 5, 8, 2, 9, true>(a, st);
    case 15: return launch_patch<128, 4, 1, 6, 8, 2, 9, false>(a, st);
    // 16 x 32 px tiles: half the weight-stream DMA per pixel of the 8 x 32 tiles
    case 16: return launch_patch<64, 8, 1, 6, 16>(a, st);
    case 17: return launch_patch<128, 8, 1, 4, 16>(a, st);
    case 18: return launch_patch<128, 4, 2, 4, 16>(a, st);
    // one barrier per kernel row (3 taps per ring slot), tap g+1's fragments read under tap g's MFMAs
    case 20: return launch_patch<64, 4, 1, 3, 8, 2, 9, false, 0, false, 3>(a, st);
    case 21: return launch_patch<128, 4, 1, 2, 4, 2, 9, false, 0, false, 3>(a, st);
    case 23: return launch_patch<128, 8, 1, 2, 8, 1, 9, false, 0, false, 3>(a, st);
    case 24: return launch_patch<128, 4, 2, 2, 8, 1, 9, false, 0, false, 3>(a, st);
    // one 8 x 32 px patch shared by 256 output channels (8 waves of 64 px x 128 channels, one block per CU)
    case 26: return launch_patch<256, 4, 2, 2, 8, 1, 9, false, 0, false, 3>(a, st);
    // 64 px x 64 channel wave tiles, 4 waves (two 256 px x 64 channel blocks per CU)
    case 27: return launch_patch<64, 4, 1, 2, 8, 2, 9, false, 0, false, 3>(a, st);
    // 16 x 32 px tiles on 16 waves of 32 px x 64 channels (1024 threads, one block per CU): half the weight DMA per MFMA
    case 28: return launch_patch<64, 16, 1, 2, 16, 1, 9, false, 0, false, 3>(a, st);
    case 29: return launch_patch<64, 16, 1, 3, 16, 1, 9, false, 0, false, 3>(a, st);
    // 64 px x 64 channel wave tiles at 4 waves per SIMD, 4-slot ring
    case 31: return launch_patch<128, 4, 2, 4, 8, 2>(a, st);
#endif
    default: break;
  }
  // row-stationary kernel (conv_rows.hip) on grids of >= g_opt.rows_min_blocks 16 x 32 px x 64 channel blocks (one block
  // per CU: ~4 full rounds); rows_kernel 8 / 16 forces that tile height wherever it is legal
  if (g_opt.rows_kernel && rows_ok(a)) {
    if (g_opt.rows_kernel == 8 || g_opt.rows_kernel == 16) {  // forced: per-frame tiles (the rows kernel does not pack)
      a.vstride = a.vW = 0;
      return launch_rows(a, st, (int)g_opt.rows_kernel);
    }
    const long N16 = a.M / ((long)a.H * a.W);
    const long blocks16 = N16 * ((a.H + 15) / 16) * ((a.W + 31) / 32) * ((a.cout + 63) / 64);
    // measured in the 1080p forward (scripts/opt_ab.sh, bench.py --layers --option rows_min_*): a win for cin >= 256
    // on >= 400 blocks (conv3_4, conv2_3, conv3_2, conv3_3: -3..-4 %) and for cin 128 on >= 800 blocks (conv2_2,
    // conv3_1: -2..-3 %; r03: whole forward +1.0 % same-box); a loss for the folded upconvs (8-byte phase-scattered
    // stores), cin 64 (conv2_1: the persistent patch kernel is faster)
    // ... and only where its 16-row tiles waste no more rows than the patch kernel's 8-row ones (the training
    // towers' 40 x 40 level: 48 of 40 rows vs 40, measured 612 vs ~800 TFLOP/s)
    const bool rows_fit = ((a.H + 15) / 16) * 16 <= ((a.H + 7) / 8) * 8 + a.H / 32;
    if ((!a.up || g_opt.rows_up) && !a.vstride && rows_fit && blocks16 >= g_opt.rows_min_blocks && a.cin_pad >= g_opt.rows_min_cin &&
        (a.cin_pad >= 2 * g_opt.rows_min_cin || blocks16 >= 2 * g_opt.rows_min_blocks))
      return launch_rows(a, st, 16);
  }
  // measured per layer inside the UNetVideo 1080p forward (scripts/sweep.sh, profiles/r01_patch_cfg_sweep.txt):
  // 8 waves of 32 px x 64 channels with one barrier per kernel row (3 taps per ring slot) everywhere, except
  // 4 waves of 64 px x 128 channels (2 blocks per CU, one barrier per tap) for cin >= 512, cout >= 128 on grids
  // of >= ~2 full rounds of blocks, a 3-slot ring for the largest grids, 4 x 32 px tiles for grids under 2 rounds.
  // Same-box A/B of the whole forward (bench.py --option patch_rowslot=0|1): 292.4 -> 306.8 frames/s
  const long N = a.M / ((long)a.H * a.W);
  const long sp = a.vstride ? ((a.H + 7) / 8) * (long)((a.vW + 31) / 32) : N * ((a.H + 7) / 8) * ((a.W + 31) / 32);
  const long blocks64 = sp * ((a.cout + 63) / 64);
#ifdef VM_STUDY
  if (!g_opt.patch_rowslot) {
    if (a.cout >= 128 && a.cin_pad >= 256 && sp * ((a.cout + 127) / 128) >= 1000)
      return launch_patch<128, 4, 1, 4, 8, 2>(a, st);
    if (blocks64 < 512) return launch_patch<64, 4, 1, 6, 4>(a, st);
    return launch_patch<64, 8, 1, 6>(a, st);
  }
#endif
  // (a folded upconv takes the row-slot configs below, whose instantiation skips its phases' zero taps)
  if (!(a.up && g_opt.up_skip) && a.cout >= 128 && a.cin_pad >= 512 && sp * ((a.cout + 127) / 128) >= 1000) {
    // fp16 operands (the split x3 forward's upconv_2 / _3, K = 3 x cin): the 3-slot 64-channel ring measured faster
    // (same box, patch_cfg 19 vs auto: 0.759 / 0.803 -> 0.732 / 0.754 ms, profiles/r06k_f16x3_patch_cfg_ab.log)
    if (a.f16) return launch_patch_up<64, 8, 1, 3, 8, 1, 9, false, 0, false, 3>(a, st);
    return launch_patch_up<128, 4, 2, 3, 8, 2>(a, st);  // 64 px x 64 channel waves, 4 per SIMD (r02: -5% vs 4x1)
  }
  if (persist_ok(a)) {  // the same tilings, persistent (2-slot ring: the LDS also holds the block's constants)
    const bool sk = a.up && g_opt.up_skip;
    int rc = 1;
    if (blocks64 >= 512)
      rc = sk ? launch_patch_persist<64, 8, 1, 2, 8, 1, true>(a, st) : launch_patch_persist<64, 8, 1, 2, 8, 1, false>(a, st);
    else
      rc = sk ? launch_patch_persist<64, 4, 1, 2, 4, 2, true>(a, st) : launch_patch_persist<64, 4, 1, 2, 4, 2, false>(a, st);
    if (rc != 1) return rc;
  }
  // the 3-slot ring for the largest grids and for the folded upconvs the persistent kernel leaves (upconv_2: its
  // zero-tap phases are latency-bound on the ring, a deeper prefetch measured -2 %)
  if (blocks64 >= 8000 || (a.up && g_opt.up_skip && blocks64 >= 512))
    return launch_patch_up<64, 8, 1, 3, 8, 1, 9, false, 0, false, 3>(a, st);
  if (blocks64 < 512) return launch_patch_up<64, 4, 1, 2, 4, 2, 9, false, 0, false, 3>(a, st);  // L5: 4 x 32 px tiles
  return launch_patch_up<64, 8, 1, 2, 8, 1, 9, false, 0, false, 3>(a, st);
}

}  // namespace vm
