// pwbwd.hip — the backward of a 1x1 conv and the BatchNorm after it, in one pass (bf16).
//
// Reference: slim.conv2d(.., [1, 1]) + slim.batch_norm (conv_blocks.py:263-294 expand /
// project, catch_net.py:301-304 head 1x1s); TF runs FusedBatchNormGrad, then
// Conv2DBackpropInput and Conv2DBackpropFilter, each a separate pass over the tensors.
//
// Unfused (rod_bn_bwd + rod_conv_fwd(mode 1) + rod_conv_wgrad) the [M, Cout] gradient dy is
// written once and read three times.  Here a block streams its chunk of rows, 64 at a time:
//   1. loads dz and the pre-BatchNorm y, forms dy = coef0*(g - coef1 - yhat*coef2) in
//      registers (rod_bn_bwd_apply's arithmetic, rounded to bf16) and stages it in LDS;
//      loads the conv input rows (BatchNorm-apply prologue when the input was Pending);
//   2. dW += dy^T . a  (16x16x32 bf16 MFMA, both operands read transposed with
//      ds_read_b64_tr_b16; the bias gradient is a ones column appended to a);
//      dx  = dy . W    (W = wt1 [Cin][Cout] held in LDS for the whole launch);
//   3. stages dx in LDS and writes whole 16-byte row segments.
// dW / db partials per block go to fp32 slabs summed in f64 in fixed order (slab_sum), so the
// result is deterministic.  Bytes per row: 2*Cout*2 (dz, y) + Cin*2 (x) + Cin*2 (dx).
//
// The kernel is latency-bound on its synchronous 64-row steps, so occupancy is what it runs
// on: the wave index is made scalar (readfirstlane: tile indices and their divisions in
// SGPRs), per-step offsets are recomputed from an opaque copy of the thread index instead of
// being hoisted as loop invariants, dz / y are batched two (not four) 16-byte loads deep, and
// the 7 coefficient fields are read four channels at a time.  The expand shapes went from
// 1-2 to 3 waves per SIMD: tools/pwbwd_bench.py 4715 -> 3326 us over its eight shapes,
// outputs bit-identical.
//
// The arithmetic the three kernels of this file share — the gate and dy (pb_dy1), the lane
// constants, the input prologue, the MFMA tiles, the wave-ordered tails and the 32-row tile
// bookkeeping — is stated once in pwbwd_common.h; this file keeps what differs: which rows a
// thread owns, what is in flight when, and the launch plans.
#include "rod_common.h"
#include "pwbwd_common.h"

namespace rod {

constexpr int PB_BM = 64;    // rows per step (4 waves x 16 rows of dx)
constexpr int PB_CF = 8;     // per-channel coefficient fields in the LDS table

struct PwBwdArgs {
  const bf16_t* dz;
  const bf16_t* y;
  const bf16_t* x;
  const bf16_t* wt1;
  bf16_t* dx;
  float* partw;  // [nblk][Cout][Cin]
  float* partb;  // [nblk][Cout] or NULL
  const float *mean, *rstd, *gamma, *beta, *coef;
  const float *xmean, *xrstd, *xgamma, *xbeta;
  int act, xact;
  long M, chunk;
  int Cin, Cout, kd, nci, nco, nxt;
  bf16_t* dyp = nullptr;   // rod_pw_bwd_gred_dyp: the BatchNorm-backward output rows [M][Cout] (dx not written)
  const bf16_t* wt0 = nullptr;   // RC (ABI 23): the forward weights [Cout][Cin]; y is recomputed, never read
};

template <int NX, int WT>
__global__ void __launch_bounds__(256) pw_bwd_kernel(PwBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Cin = a.Cin, Cout = a.Cout;
  const int CCH = Cout / 8, XCH = Cin / 8;
  const int LDD = a.kd + 8;           // 16-byte aligned rows, 8-byte aligned transposed reads
  const int LDX = a.nci * 16 + 8;
  // coefficient tables field-major ([PB_CF][Cout], [2][Cin]): a thread reads its chunk's 8
  // channels of a field as two 16-byte LDS reads, neighbouring lanes on neighbouring chunks
  float* ctab = (float*)smem;                                  // [PB_CF][Cout]
  float* xtab = ctab + (long)Cout * PB_CF;                     // [2][Cin]
  bf16_t* Ds = (bf16_t*)(xtab + 2 * Cin);                      // [64][LDD]   dy
  bf16_t* Xs = Ds + PB_BM * LDD;                               // [64][LDX]   a | 1 ; dx staging
  bf16_t* Ws = Xs + PB_BM * LDX;                               // [nxt*16][LDD] wt1
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: tile indices in SGPRs
  const bool prox = a.xmean != nullptr;
  const bool has_bias = a.partb != nullptr;
  const float ghi = pb_gate_hi(a.act), glo = pb_gate_lo(a.act);

  for (int c = tid; c < Cout; c += 256) {   // fields 2..6: sc, sh, a, k1, k0 (0, 1, 7: mean, rstd, 0)
    float* t = ctab + c;
    t[0] = a.mean[c];
    t[Cout] = a.rstd[c];
    pb_bn_d1(a.mean, a.rstd, a.gamma, a.beta, a.coef, Cout, c, t[2 * Cout], t[3 * Cout], t[4 * Cout], t[5 * Cout],
             t[6 * Cout]);
    t[7 * Cout] = 0.f;
  }
  if (prox) {
    for (int c = tid; c < Cin; c += 256) {
      float sc, sh;
      bn_affine(a.xmean, a.xrstd, a.xgamma, a.xbeta, c, sc, sh);
      xtab[c] = sc;
      xtab[Cin + c] = sh;
    }
  }
  // zero padding: dy columns >= Cout, a columns >= Cin, the whole W image (Ds | Xs | Ws are
  // contiguous, every row a multiple of 16 bytes)
  pb_lds_zero(Ds, (PB_BM * LDD + PB_BM * LDX + a.nxt * 16 * LDD) / 8, tid);
  __syncthreads();
  if (a.dx) pb_load_wt1(Ws, LDD, a.wt1, Cin, Cout, tid);

  const long mb = (long)blockIdx.x * a.chunk;
  const long me = mb + a.chunk < a.M ? mb + a.chunk : a.M;

  f32x4 accw[WT];
#pragma unroll
  for (int i = 0; i < WT; ++i) accw[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntile = a.nco * a.nci;
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;

  for (long m0 = mb; m0 < me; m0 += PB_BM) {
    __syncthreads();  // the previous step's readers of Ds / Xs are done
    // The thread index passes through an opaque copy each step, so the per-thread LDS / global
    // offsets below are recomputed in the loop (a few VALU ops) instead of being hoisted out of
    // it as loop invariants — each hoisted offset held a VGPR for the whole kernel and together
    // they cost two thirds of the occupancy.
    int tid_l = tid;
    asm volatile("" : "+v"(tid_l));
    const int tid = tid_l;
    const int g = (tid & 63) >> 4, li = tid & 15, q = li >> 2, p = li & 3;
    // ---- 1. dy = BatchNorm backward of (dz, y) -> Ds; a -> Xs ----------------------------
    // the conv-input rows are loaded first so their latency overlaps the dz / y loads
    constexpr int XR = NX / 2 > 0 ? NX / 2 : 1;   // 64 * Cin/8 chunks / 256 threads <= NX/2
    const int xtot = PB_BM * XCH;
    bf16x8 xr[XR];
#pragma unroll
    for (int k = 0; k < XR; ++k) {
      const int idx = tid + k * 256;
      const int r = idx / XCH, cc = idx - r * XCH;
      if (idx < xtot && m0 + r < me) xr[k] = *(const bf16x8*)(a.x + (m0 + r) * Cin + cc * 8);
    }
    const int tot = PB_BM * CCH;
    for (int base = tid; base < tot; base += 512) {
      bf16x8 dv[2], yv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = base + u * 256;
        const int r = idx / CCH, cc = idx - r * CCH;
        const long m = m0 + r;
        if (idx < tot && m < me) {
          dv[u] = *(const bf16x8*)(a.dz + m * Cout + cc * 8);
          yv[u] = *(const bf16x8*)(a.y + m * Cout + cc * 8);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = base + u * 256;
        if (idx >= tot) continue;
        const int r = idx / CCH, cc = idx - r * CCH;
        const long m = m0 + r;
        bf16x8 o;
        if (m < me) {
          // two halves of 4 channels: 7 coefficient fields x 4 live at a time
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x4 f[7];
#pragma unroll
            for (int k = 2; k < 7; ++k) f[k] = *(const f32x4*)(ctab + k * Cout + cc * 8 + 4 * h);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const int j = 4 * h + jj;
              o[j] = (bf16_t)pb_dy1(PbGate{ghi, glo}, f[2][jj], f[3][jj], f[4][jj], f[5][jj], f[6][jj], dv[u][j], yv[u][j]);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (bf16_t)0.f;
        }
        *(bf16x8*)(Ds + r * LDD + cc * 8) = o;
      }
    }
#pragma unroll
    for (int k = 0; k < XR; ++k) {
      const int idx = tid + k * 256;
      if (idx >= xtot) continue;
      const int r = idx / XCH, cc = idx - r * XCH;
      bf16x8 v = xr[k];
      if (m0 + r < me) {
        if (prox) {
          float xsc[8], xsh[8];
          pb_ld8(xtab + cc * 8, xsc);
          pb_ld8(xtab + Cin + cc * 8, xsh);
          v = pb_xpro(v, xsc, xsh, a.xact, true);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (bf16_t)0.f;
      }
      *(bf16x8*)(Xs + r * LDX + cc * 8) = v;
    }
    if (has_bias && tid < PB_BM) Xs[tid * LDX + Cin] = (bf16_t)(m0 + tid < me ? 1.f : 0.f);
    __syncthreads();
    // ---- 2a. dW (+ db) += dy^T . [a | 1] over the 64 rows ----------------------------------
#pragma unroll
    for (int i = 0; i < WT; ++i) {
      const int t = wave + 4 * i;
      if (t >= ntile) continue;
      const int ct = t / a.nci, it = t - ct * a.nci;
#pragma unroll
      for (int ks = 0; ks < PB_BM / 32; ++ks)
        pb_dw_tile(Ds + ks * 32 * LDD, LDD, Xs + ks * 32 * LDX, LDX, ct, it, tid & 63, accw[i]);
    }
    if (!a.dx) continue;
    // ---- 2b. dx = dy . W for this wave's 16 rows -------------------------------------------
    // (pb_dx_half's loop with the run-time k depth and tile count of this kernel's plan)
    f32x4 accx[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) accx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.kd / 32; ++s) {
      const bf16x8 fa = *(const bf16x8*)(Ds + (wave * 16 + li) * LDD + s * 32 + 8 * g);
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        if (j >= a.nxt) continue;
        const bf16x8 fb = *(const bf16x8*)(Ws + (j * 16 + li) * LDD + s * 32 + 8 * g);
        accx[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, accx[j], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done reading Xs (dW) before it becomes the dx stage
    // ---- 3. dx -> Xs -> 16-byte row segments ------------------------------------------------
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      if (j >= a.nxt) continue;
      const int col = j * 16 + li;
      if (col < Cin) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(wave * 16 + 4 * g + r) * LDX + col] = (bf16_t)accx[j][r];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < PB_BM * XCH; idx += 256) {
      const int r = idx / XCH, cc = idx - r * XCH;
      const long m = m0 + r;
      if (m < me) *(bf16x8*)(a.dx + m * Cin + cc * 8) = *(const bf16x8*)(Xs + r * LDX + cc * 8);
    }
  }
  // ---- partial dW / db of this block ------------------------------------------------------
  float* pw = a.partw + (long)blockIdx.x * Cout * Cin;
#pragma unroll
  for (int i = 0; i < WT; ++i) {
    const int t = wave + 4 * i;
    if (t >= ntile) continue;
    const int ct = t / a.nci, it = t - ct * a.nci;
    const int ci = it * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = ct * 16 + 4 * g + r;
      if (co >= Cout) continue;
      if (ci < Cin) pw[(long)co * Cin + ci] = accw[i][r];
      else if (has_bias && ci == Cin) a.partb[(long)blockIdx.x * Cout + co] = accw[i][r];
    }
  }
}


// =====================================================================================
// Streaming form (the expand shapes 16->96 and 24->144 without bias): every wave works on
// its own 32-row tiles with no block barrier inside the row loop — the 64-row block-synchronous
// steps above leave the memory system idle while all four waves sit in their MFMA phase.
//   * lane constants: a lane owns ONE 8-channel chunk cc of dz / y (lanes = RG row groups x
//     COUT/8 chunks) for the whole launch, so its BatchNorm-backward constants (sc, sh, a, k1,
//     k0 of 8 channels) sit in registers — no per-element coefficient reads from LDS;
//   * per 16-row half: dz / y / x arrive by buffer loads from a per-tile resource (rows past M
//     read 0, their dx stores are dropped), dy = bn_bwd_apply (rounded to bf16, the arithmetic of
//     the block kernel) goes to this wave's LDS tile, then the NEXT half's loads are issued into
//     the same registers before the MFMA work of this one (one half in flight per wave, no extra
//     registers);
//   * dx = dy . W for the half (A fragments straight from the dy rows, W staged once per block),
//     staged through a wave-private LDS slot and written as 16-byte row segments;
//   * after the second half, dW += dy^T . x over the 32 rows (both operands read transposed,
//     ds_read_b64_tr_b16, as above);
//   * at the end the four waves' dW add in wave order in LDS (one partial per block, slab_sum).
// dx is the block kernel's bit for bit (same dy, same MFMA k order); dW sums its rows in another
// grouping (fp32, within the float64 bounds of tests/test_gpu_pwbwd.py).
// =====================================================================================
template <int CIN, int COUT>
struct PbsGeo {
  // CW channels per lane chunk: 4 (8-byte loads) where the chunks tile 64 lanes into whole rows
  // without waste (96: 2 row groups x 24 chunks, 16 rows in 8 steps, 20 constant registers
  // instead of 40), else 8
  static constexpr int CW = (64 / (COUT / 4)) * (COUT / 4) >= 48 && 16 % (64 / (COUT / 4)) == 0 ? 4 : 8;
  static constexpr int CCH = COUT / CW, RG = 64 / CCH, JN = (16 + RG - 1) / RG;
  static constexpr int KT = (COUT + 31) / 32, KD = KT * 32, LDD = KD + 8;
  static constexpr int NCO = COUT / 16, XCH = CIN / 8, NCI = (CIN + 15) / 16, LDX = NCI * 16 + 8;
  static constexpr int LDC = CIN + 8;
  static constexpr int WREG = 32 * LDD + 32 * LDX + 16 * LDC;    // bf16 elements per wave
  static constexpr int WS = NCI * 16 * LDD;                       // wt1 image (bf16 elements)
  static constexpr int XT = 3 * CIN * 2;                          // input-prologue table (bf16 slots)
  static constexpr int LDW = 40;                                  // RC: forward weight rows, k zero-padded to 32
  static constexpr int WF = COUT * LDW;                           // RC: forward weight image (bf16 elements)
  static constexpr size_t lds(bool rc = false) {
    const size_t main = (size_t)(WS + XT + 4 * WREG + (rc ? WF : 0)) * 2;
    const size_t red = (size_t)(WS + XT + (rc ? WF : 0)) * 2 + (size_t)COUT * NCI * 16 * 4 +
                       (size_t)4 * 16 * 2 * CIN * 4;
    return main > red ? main : red;
  }
};

template <int CW> struct PbsVec;
template <> struct PbsVec<4> { typedef bf16x4 T; };
template <> struct PbsVec<8> { typedef bf16x8 T; };

// XG (with the input prologue): also the input BatchNorm's backward sums over (dx, x) — the
// expand conv of a block whose input is the previous block's project output (linear BatchNorm):
// that BatchNorm's gradient is this dx, so its rod_bn_bwd_reduce pass is not needed
// (rod_pw_bwd_gred on the expand shapes); part blockIdx.x of [nblk][2][CIN]
// XL: the input BatchNorm is linear (act NONE; the project output chained into an expand) —
// its prologue and sums compile without the activation (a runtime branch costs the XG form
// 12 VGPRs and a wave per SIMD).
// RC (ABI 23, rod_pw_bwd_rc / rod_pw_bwd_gred_rc): the pre-BatchNorm y = x_act . W^T is not read
// but recomputed per 16-row half from the conv input already staged for the weight gradient — the
// forward's MFMA (v_mfma_f32_16x16x32_bf16, k zero-padded to 32) with the operands swapped, so the
// lane holds 4 consecutive channels of one row, rounded to bf16 once: the stored y bit for bit.
// It is written into the half's dy rows in LDS, where each lane reads its chunk and overwrites it
// with dy in place (the same lane reads and writes an element).  Saves the M x COUT y stream (the
// expanded tensor of an inverted-residual block: 1.42 GB at 720p b8 for 16 -> 96).
// Occupancy: the 16 -> 96 forms at 3 waves per SIMD — 120-168 VGPRs and no AGPRs, no spills
// (unbounded: 156 + 24 AGPRs, 2 waves), so the 768-block grid is resident at once: block 1's
// recomputing gred form 568.5 -> 557.8 us; the 24 -> 144 forms (200-250 + 72-76 AGPRs, 1 wave)
// measured slower at 2 waves (306 -> 321-327 us) and stay unbounded (profiles/r6_pwbwd_bounds_ab.txt).
template <int CIN, int COUT, bool PRO, bool DX, bool XG = false, bool XL = false, bool RC = false>
__global__ void __launch_bounds__(256, CIN == 16 ? 3 : 1) pw_bwd_stream_kernel(PwBwdArgs a, long ntiles, float* __restrict__ xparts) {
  using G = PbsGeo<CIN, COUT>;
  static_assert(!XG || (PRO && DX), "the input sums need the prologue and dx");
  static_assert(!RC || CIN <= 32, "the recompute is one k step");
  constexpr int CW = G::CW, CCH = G::CCH, RG = G::RG, JN = G::JN, KT = G::KT, LDD = G::LDD, NCO = G::NCO,
                XCH = G::XCH, NCI = G::NCI, LDX = G::LDX, LDC = G::LDC;
  typedef typename PbsVec<CW>::T VT;
  static_assert(COUT % 16 == 0 && CIN % 8 == 0 && 16 * XCH <= 64, "streaming pw_bwd geometry");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ws = (bf16_t*)smem;                                   // [NCI*16][LDD]: wt1 rows (ci), k = co
  float* xtab = (float*)(Ws + G::WS);                           // [3][CIN]: input prologue scale, shift, mean
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bf16_t* Ds = Ws + G::WS + G::XT + wave * G::WREG;             // [32][LDD]  dy of the tile
  bf16_t* Xs = Ds + 32 * LDD;                                   // [32][LDX]  conv input of the tile
  bf16_t* Cx = Xs + 32 * LDX;                                   // [16][LDC]  dx staging
  bf16_t* Wf = Ws + G::WS + G::XT + 4 * G::WREG;                // RC: [COUT][LDW] forward weights
  // zero everything once (dy columns >= COUT, x columns >= CIN stay 0), then the weights
  pb_lds_zero(smem, (G::WS + G::XT + 4 * G::WREG + (RC ? G::WF : 0)) / 8, tid);
  __syncthreads();
  if constexpr (DX) pb_load_wt1(Ws, LDD, a.wt1, CIN, COUT, tid);
  if constexpr (PRO) {
    for (int c = tid; c < CIN; c += 256) {
      bn_affine(a.xmean, a.xrstd, a.xgamma, a.xbeta, c, xtab[c], xtab[CIN + c]);
      xtab[2 * CIN + c] = a.xmean[c];
    }
  }
  if constexpr (RC) {
    for (int i = tid; i < COUT * (CIN / 8); i += 256) {
      const int co = i / (CIN / 8), k8 = i - co * (CIN / 8);
      *(bf16x8*)(Wf + co * G::LDW + k8 * 8) = *(const bf16x8*)(a.wt0 + (long)co * CIN + k8 * 8);
    }
  }
  __syncthreads();

  // ---- lane constants ---------------------------------------------------------------------
  float xsg[XG ? 8 : 1] = {}, xsgx[XG ? 8 : 1] = {};   // XG: sums of g and g*(x - mean), this lane's chunk
  const int rg = lane / CCH, cc = lane - (lane / CCH) * CCH;
  const bool dact = rg < RG;
  PbBnD<CW> bd;
  bd.init(a.mean, a.rstd, a.gamma, a.beta, a.coef, COUT, dact ? cc * CW : 0);
  const float ghi = pb_gate_hi(a.act), glo = pb_gate_lo(a.act);
  const int xr = lane / XCH, xc = lane - (lane / XCH) * XCH;
  const bool xact = lane < 16 * XCH;
  // lane offset of chunk j inside a half (bytes): vd0 + j * RG rows; ROD_OOB: no row there
  const unsigned vd0 = dact ? (unsigned)((rg * COUT + cc * CW) * 2) : ROD_OOB;
  auto vdj = [&](int j) -> unsigned { return pb_lane_off<JN, RG>(vd0, rg, j, COUT * 2); };
  const unsigned vx = xact ? (unsigned)((xr * CIN + xc * 8) * 2) : ROD_OOB;
  const long M = a.M;
  auto rsrc_rows = [&](const void* base, long row0, int rowbytes) { return pb_rsrc_rows(base, M, row0, rowbytes); };

  f32x4 accw[NCO][NCI];
#pragma unroll
  for (int i = 0; i < NCO; ++i)
#pragma unroll
    for (int j = 0; j < NCI; ++j) accw[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const long wstride = (long)gridDim.x * 4;
  long t = (long)blockIdx.x * 4 + wave;
  VT dzv[JN], yv[RC ? 1 : JN];
  bf16x8 xv;
  {   // the first half (t >= ntiles: an empty resource, the loads return 0)
    const rsrc_t rdz = rsrc_rows(a.dz, t * 32, COUT * 2);
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      dzv[j] = buf_ld<VT>(rdz, vdj(j), 0u);
      if constexpr (!RC) yv[j] = buf_ld<VT>(rsrc_rows(a.y, t * 32, COUT * 2), vdj(j), 0u);
    }
    xv = buf_ld<bf16x8>(rsrc_rows(a.x, t * 32, CIN * 2), vx, 0u);
  }
  for (; t < ntiles; t += wstride) {
    const long row0 = t * 32;
    // not unrolled: the reloads land in the registers just consumed (unrolled, the compiler
    // double-buffers them: +32 VGPRs)
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      // ---- dy = BatchNorm backward of (dz, y) -> Ds; x (+ prologue) -> Xs ------------------
      // each chunk's registers are reloaded with the NEXT half's chunk as soon as they are
      // consumed, so this wave keeps loads in flight through its VALU work as well
      // (RC: x first, then y recomputed from it into the dy rows, then dy over it in place)
      const long rown = (h == 0 ? t : t + wstride) * 32;
      const rsrc_t ndz = rsrc_rows(a.dz, rown, COUT * 2);
      const unsigned nso = (unsigned)((1 - h) * 16 * COUT * 2);
      auto dy_rows = [&]() {
        const rsrc_t ny = rsrc_rows(a.y, rown, COUT * 2);
#pragma unroll
        for (int j = 0; j < JN; ++j) {
          const int r = rg + RG * j;
          const bool rok = dact && (JN * RG == 16 || r < 16);
          bf16_t* dp = Ds + (h * 16 + (rok ? r : 0)) * LDD + cc * CW;
          VT yj4;
          if constexpr (RC) yj4 = *(const VT*)dp;
          else yj4 = yv[j];
          const VT o = bd.dy(PbGate{ghi, glo}, dzv[j], yj4);
          dzv[j] = buf_ld<VT>(ndz, vdj(j), nso);
          if constexpr (!RC) yv[j] = buf_ld<VT>(ny, vdj(j), nso);
          if (rok) *(VT*)dp = o;
        }
      };
      if constexpr (!RC) dy_rows();
      const bf16x8 xcur = xv;   // XG: the raw x of this half, for the sums at the dx write-back
      {
        bf16x8 v = xv;
        if constexpr (PRO) {
          const bool rok = row0 + h * 16 + xr < M;   // rows past M stay 0 (not act(shift))
          float xsc[8], xsh[8];
          pb_ld8(xtab + xc * 8, xsc);
          pb_ld8(xtab + CIN + xc * 8, xsh);
          if constexpr (XL) v = pb_xpro_linear(v, xsc, xsh, rok);   // linear input BatchNorm: packed pairs
          else v = pb_xpro(v, xsc, xsh, a.xact, rok);
        }
        xv = buf_ld<bf16x8>(rsrc_rows(a.x, rown, CIN * 2), vx, (unsigned)((1 - h) * 16 * CIN * 2));
        if (xact) *(bf16x8*)(Xs + (h * 16 + xr) * LDX + xc * 8) = v;
      }
      __builtin_amdgcn_wave_barrier();
      if constexpr (RC) {
        // y^T of this half from its x rows and the forward weights, into the half's dy rows
        pb_rc_y_half<NCO, CIN>(Xs + h * 16 * LDX, LDX, Wf, G::LDW, Ds + h * 16 * LDD, LDD, lane);
        __builtin_amdgcn_wave_barrier();
        dy_rows();
        __builtin_amdgcn_wave_barrier();
      }
      if constexpr (DX) {
        // ---- dx = dy . W for the 16 rows of this half -> Cx -> 16-byte row segments ---------
        f32x4 accx[NCI];
        pb_dx_half<KT, NCI>(Ds + h * 16 * LDD, Ws, LDD, lane, accx);
#pragma unroll
        for (int j = 0; j < NCI; ++j) {
          const int col = j * 16 + li;
          if (col < CIN) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Cx[(4 * g + r) * LDC + col] = (bf16_t)accx[j][r];
          }
        }
        __builtin_amdgcn_wave_barrier();
        const rsrc_t rdx = rsrc_rows(a.dx, row0, CIN * 2);
        const bf16x8 ov = *(const bf16x8*)(Cx + (xact ? xr : 0) * LDC + xc * 8);
        buf_st(ov, rdx, vx, (unsigned)(h * 16 * CIN * 2));
        if constexpr (XG) {
          if (xact && row0 + h * 16 + xr < M) {
            // the constants are read from the LDS table per element, not held in registers
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float mu = xtab[2 * CIN + xc * 8 + e];
              if constexpr (XL) pb_xsum_linear((float)ov[e], (float)xcur[e], mu, xsg[e], xsgx[e]);   // the project's: g = dx
              else gred_acc((float)ov[e], (float)xcur[e], xtab[xc * 8 + e], xtab[CIN + xc * 8 + e], mu, 1.f, a.xact,
                            xsg[e], xsgx[e]);
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    // ---- dW += dy^T . x over the tile's 32 rows ---------------------------------------------
    pb_dw_tiles<NCO, NCI>(Ds, LDD, Xs, LDX, lane, accw);
    __builtin_amdgcn_wave_barrier();   // the next tile's dy / x writes stay after these reads
  }
  // ---- the block's dW: the four waves add in wave order -> part blockIdx.x -----------------
  float* red = (float*)(smem + (size_t)(G::WS + G::XT) * 2);   // [COUT][NCI*16]
  constexpr int LR = NCI * 16;
  __syncthreads();
  pb_dw_wave_sum<NCO, NCI>(red, LR, wave, lane, accw);
  float* pw = a.partw + (long)blockIdx.x * COUT * CIN;
  for (int i = tid; i < COUT * CIN; i += 256) {
    const int co = i / CIN, ci = i - co * CIN;
    pw[i] = red[co * LR + ci];
  }
  if constexpr (XG) {   // waves, then the 16 row lanes of each chunk, added in a fixed order
    float* gbuf = red + COUT * LR;                                // [4][16][2][CIN]
    if (xact) pb_xsum_stage(gbuf, 16, CIN, wave, xr, xc * 8, xsg, xsgx);
    __syncthreads();
    float* xp = xparts + (long)blockIdx.x * 2 * CIN;
    for (int i = tid; i < 2 * CIN; i += 256) {
      const int k = i / CIN, c = i - k * CIN;
      xp[i] = pb_xsum_col(gbuf, 16, CIN, k, c, a.xrstd[c]);
    }
  }
}


// =====================================================================================
// Project form with the input BatchNorm's backward sums (rod_pw_bwd_gred).  The conv input is
// x_p = act_x(BN_x(x)) with x the raw depthwise output; the block's backward needs, besides
// dx / dW, BN_x's backward sums over (dx, x) — which this kernel forms from the x it already
// reads for the weight gradient and the dx it writes.  Cout is small (16..64) and Cin large, so
// the grid splits Cin into groups of NW columns (blockIdx.y): a group re-reads only dz / y (4*Cout
// bytes a row) and owns its columns of x, dx, dW and the sums.  Per wave, 32-row tiles in two
// 16-row halves, no block barrier in the row loop:
//   * dy: a lane owns one 4-channel chunk of dz / y (constants in registers), reloaded with the
//     next half's chunk as soon as it is consumed; rows past M give dy = 0;
//   * x: a lane owns one 8-column chunk of the group (BN_x constants in registers) for RGX row
//     groups; x_p = act_x(BN_x(x)) (bf16) goes to LDS for the weight gradient, the raw x stays
//     in registers for the sums; the next half's x is loaded into a second register set at the
//     start of each half (the first form loaded it after the sums: 2.5 TB/s on 96->24);
//   * dx = dy . W for the half (A fragments from the dy rows in LDS, W's group rows in LDS),
//     staged in LDS, written by the x lanes, which add g and g*xhat of their chunk as they write;
//   * after the second half dW += dy^T . x_p over the 32 rows (transposed LDS reads);
//   * at the end the waves' dW and sums add in a fixed order -> part blockIdx.x.
// =====================================================================================
template <int COUT, int NW>
struct PbgGeo {
  static constexpr int CCH = COUT / 4, RG = 64 / CCH, JN = (16 + RG - 1) / RG;
  static constexpr int KT = (COUT + 31) / 32, KD = KT * 32, LDD = KD + 8;
  static constexpr int NCO = (COUT + 15) / 16;
  static constexpr int XCH = NW / 8, RGX = 64 / XCH, JX = (16 + RGX - 1) / RGX, NWT = NW / 16;
  static constexpr int LDX = NW + 8;
  static constexpr int WREG = 32 * LDD + 32 * LDX + 16 * LDX;     // bf16 elements per wave
  static constexpr int WS = NW * LDD;                              // the group's wt1 rows
  static constexpr int RED = NCO * 16 * NW + 4 * RGX * 2 * NW;     // fp32 end-of-launch buffer
  static constexpr size_t lds() {
    const size_t main = (size_t)(WS + 4 * WREG) * 2;
    const size_t red = (size_t)WS * 2 + (size_t)RED * 4;
    return main > red ? main : red;
  }
};

// FAST: the block's activations (linear output BatchNorm, ReLU6 input BatchNorm) at compile
// time, channel pairs as packed fp32 ops; otherwise both activations at run time, per element
// DYP (rod_pw_bwd_gred_dyp): dy written by column group 0, dx not stored — a template argument so
// the two entries are separate kernels in a trace / PMC pass (rod/roofline.py ENTRY_KERNELS)
template <int COUT, int NW, bool FAST, bool DYP = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) pw_bwd_gred_kernel(PwBwdArgs a, long ntiles, float* __restrict__ xparts) {
  using G = PbgGeo<COUT, NW>;
  constexpr int CCH = G::CCH, RG = G::RG, JN = G::JN, KT = G::KT, LDD = G::LDD, NCO = G::NCO, XCH = G::XCH,
                RGX = G::RGX, JX = G::JX, NWT = G::NWT, LDX = G::LDX;
  static_assert(COUT % 8 == 0 && NW % 16 == 0 && RG * CCH <= 64 && RGX * XCH <= 64, "gred pw_bwd geometry");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Cin = a.Cin;
  const int n0 = blockIdx.y * NW;                               // this group's first column
  bf16_t* Ws = (bf16_t*)smem;                                   // [NW][LDD]: wt1 rows n0.., k = co
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bf16_t* Ds = Ws + G::WS + wave * G::WREG;                     // [32][LDD]  dy of the tile
  bf16_t* Xs = Ds + 32 * LDD;                                   // [32][LDX]  x_p of the tile
  bf16_t* Cx = Xs + 32 * LDX;                                   // [16][LDX]  dx staging
  pb_lds_zero(smem, (G::WS + 4 * G::WREG) / 8, tid);
  __syncthreads();
  pb_load_wt1(Ws, LDD, a.wt1 + (long)n0 * COUT, NW, COUT, tid);
  __syncthreads();

  // ---- lane constants: dy chunk (4 channels of Cout) and x chunk (8 columns of the group) ----
  const int rg = lane / CCH, cc = lane - (lane / CCH) * CCH;
  const bool dact = rg < RG;
  PbBnD<4> bd;
  bd.init(a.mean, a.rstd, a.gamma, a.beta, a.coef, COUT, dact ? cc * 4 : 0);
  const float ghi = pb_gate_hi(a.act), glo = pb_gate_lo(a.act);
  const int rx = lane / XCH, xc = lane - (lane / XCH) * XCH;
  const bool xact = rx < RGX;
  // sgx sums g*(x - mean); the rstd factor is applied once per column at the end
  float xsc[8], xsh[8], xmu[8], sg[8], sgx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = n0 + (xact ? xc * 8 : 0) + e;
    bn_affine(a.xmean, a.xrstd, a.xgamma, a.xbeta, c, xsc[e], xsh[e]);
    xmu[e] = a.xmean[c];
    sg[e] = sgx[e] = 0.f;
  }
  // FAST: the same constants as register pairs (packed operands without pair-building moves)
  pb_f2 ca2[2], k12[2], k02[2], xsc2[4], xsh2[4], xmu2[4];
  if constexpr (FAST) {
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      ca2[h2] = pb_f2{bd.ca[2 * h2], bd.ca[2 * h2 + 1]};
      k12[h2] = pb_f2{bd.k1[2 * h2], bd.k1[2 * h2 + 1]};
      k02[h2] = pb_f2{bd.k0[2 * h2], bd.k0[2 * h2 + 1]};
    }
#pragma unroll
    for (int h2 = 0; h2 < 4; ++h2) {
      xsc2[h2] = pb_f2{xsc[2 * h2], xsc[2 * h2 + 1]};
      xsh2[h2] = pb_f2{xsh[2 * h2], xsh[2 * h2 + 1]};
      xmu2[h2] = pb_f2{xmu[2 * h2], xmu[2 * h2 + 1]};
    }
  }
  pb_f2 sg2[4] = {}, sgx2[4] = {};
  const unsigned vd0 = dact ? (unsigned)((rg * COUT + cc * 4) * 2) : ROD_OOB;
  auto vdj = [&](int j) -> unsigned { return pb_lane_off<JN, RG>(vd0, rg, j, COUT * 2); };
  const unsigned vx0 = xact ? (unsigned)((rx * Cin + xc * 8) * 2) : ROD_OOB;
  auto vxj = [&](int j) -> unsigned { return pb_lane_off<JX, RGX>(vx0, rx, j, Cin * 2); };
  const long M = a.M;
  // dz / y rows [row0, +32) of Cout channels; x / dx rows of this group's columns
  auto rsrc_d = [&](const void* base, long row0) { return pb_rsrc_rows(base, M, row0, COUT * 2); };
  auto rsrc_x = [&](const void* base, long row0) { return pb_rsrc_cols(base, M, row0, Cin, n0, NW); };

  f32x4 accw[NCO][NWT];
#pragma unroll
  for (int i = 0; i < NCO; ++i)
#pragma unroll
    for (int j = 0; j < NWT; ++j) accw[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const long wstride = (long)gridDim.x * 4;
  long t = (long)blockIdx.x * 4 + wave;
  bf16x4 dzv[JN], yv[JN];
  bf16x8 xv[JX];
  {
    const rsrc_t rdz = rsrc_d(a.dz, t * 32), ry = rsrc_d(a.y, t * 32), rxx = rsrc_x(a.x, t * 32);
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      dzv[j] = buf_ld<bf16x4>(rdz, vdj(j), 0u);
      yv[j] = buf_ld<bf16x4>(ry, vdj(j), 0u);
    }
#pragma unroll
    for (int j = 0; j < JX; ++j) xv[j] = buf_ld<bf16x8>(rxx, vxj(j), 0u);
  }
  for (; t < ntiles; t += wstride) {
    const long row0 = t * 32;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const long rown = (h == 0 ? t : t + wstride) * 32;
      // the next half's x, in flight through this whole half (xv is needed until its sums)
      bf16x8 xn[JX];
      {
        const rsrc_t nx = rsrc_x(a.x, rown);
        const unsigned nso = (unsigned)((1 - h) * 16 * Cin * 2);
#pragma unroll
        for (int j = 0; j < JX; ++j) xn[j] = buf_ld<bf16x8>(nx, vxj(j), nso);
      }
      // ---- dy -> Ds (rows past M: 0); the next half's dz / y chunks reload as consumed --------
      {
        const rsrc_t ndz = rsrc_d(a.dz, rown), ny = rsrc_d(a.y, rown);
        const unsigned nso = (unsigned)((1 - h) * 16 * COUT * 2);
        // dyp (column group 0 only; other blocks and rows past M: the empty / range-checked resource)
        const rsrc_t rdp = DYP && blockIdx.y == 0 ? rsrc_d(a.dyp, row0) : rod_rsrc(a.dz, 0u);
        const unsigned dpso = (unsigned)(h * 16 * COUT * 2);
#pragma unroll
        for (int j = 0; j < JN; ++j) {
          const int r = rg + RG * j;
          const bool rok = row0 + h * 16 + r < M;
          bf16x4 o;
          if constexpr (FAST) {   // linear output BatchNorm: g = dz; dy = fma(a, dz, fma(k1, y, k0))
            const u32x2_t yu = __builtin_bit_cast(u32x2_t, yv[j]), du = __builtin_bit_cast(u32x2_t, dzv[j]);
            u32x2_t ou;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              const pb_f2 dy2 = pb_dy_pair_linear(ca2[h2], k12[h2], k02[h2], pb_unpack(du[h2]), pb_unpack(yu[h2]));
              ou[h2] = rok ? pb_round(dy2) : 0u;
            }
            o = __builtin_bit_cast(bf16x4, ou);
          } else {
            const bf16x4 zero4 = {};
            o = rok ? bd.dy(PbGate{ghi, glo}, dzv[j], yv[j]) : zero4;
          }
          dzv[j] = buf_ld<bf16x4>(ndz, vdj(j), nso);
          yv[j] = buf_ld<bf16x4>(ny, vdj(j), nso);
          buf_st(o, rdp, vdj(j), dpso);   // dropped unless the dyp form (empty resource)
          if (dact && (JN * RG == 16 || r < 16)) *(bf16x4*)(Ds + (h * 16 + r) * LDD + cc * 4) = o;
        }
      }
      // ---- x_p = act_x(BN_x(x)) -> Xs (rows past M: 0) -------------------------------------
#pragma unroll
      for (int j = 0; j < JX; ++j) {
        const int r = rx + RGX * j;
        const bool rok = row0 + h * 16 + r < M;
        bf16x8 v;
        if constexpr (FAST) v = pb_xpro_relu6(xv[j], xsc2, xsh2, rok);   // ReLU6 input BatchNorm, packed
        else v = pb_xpro(xv[j], xsc, xsh, a.xact, rok);
        if (xact && (JX * RGX == 16 || r < 16)) *(bf16x8*)(Xs + (h * 16 + r) * LDX + xc * 8) = v;
      }
      __builtin_amdgcn_wave_barrier();
      // ---- dx = dy . W for the half -> Cx; written by the x lanes with the BN_x sums ------------
      {
        f32x4 accx[NWT];
        pb_dx_half<KT, NWT>(Ds + h * 16 * LDD, Ws, LDD, lane, accx);
#pragma unroll
        for (int j = 0; j < NWT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) Cx[(4 * g + r) * LDX + j * 16 + li] = (bf16_t)accx[j][r];
        __builtin_amdgcn_wave_barrier();
        const rsrc_t rdx = !DYP ? rsrc_x(a.dx, row0) : rod_rsrc(a.x, 0u);   // dyp form: dx not stored
        const unsigned so = (unsigned)(h * 16 * Cin * 2);
#pragma unroll
        for (int j = 0; j < JX; ++j) {
          const int r = rx + RGX * j;
          const bool rok = row0 + h * 16 + r < M && xact && (JX * RGX == 16 || r < 16);
          const bf16x8 dv = *(const bf16x8*)(Cx + (r < 16 ? r : 0) * LDX + xc * 8);
          buf_st(dv, rdx, vxj(j), so);
          if (rok) {
            // FAST: g = dx where 0 < z < 6; sums of g and g*(x - mean), in pairs
            if constexpr (FAST) pb_xsum_relu6(dv, xv[j], xsc2, xsh2, xmu2, sg2, sgx2);
            else {
#pragma unroll
              for (int e = 0; e < 8; ++e)
                gred_acc((float)dv[e], (float)xv[j][e], xsc[e], xsh[e], xmu[e], 1.f, a.xact, sg[e], sgx[e]);
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int j = 0; j < JX; ++j) xv[j] = xn[j];
    }
    // ---- dW += dy^T . x_p over the tile's 32 rows -------------------------------------------
    pb_dw_tiles<NCO, NWT>(Ds, LDD, Xs, LDX, lane, accw);
    __builtin_amdgcn_wave_barrier();
  }
  // ---- end: dW (waves in order) and the BN_x sums (waves, then row groups, in order) -------
  float* red = (float*)(smem + (size_t)G::WS * 2);              // [NCO*16][NW]
  float* gbuf = red + NCO * 16 * NW;                            // [4][RGX][2][NW]
  __syncthreads();
  if constexpr (FAST) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sg[e] = sg2[e >> 1][e & 1];
      sgx[e] = sgx2[e >> 1][e & 1];
    }
  }
  if (xact) pb_xsum_stage(gbuf, RGX, NW, wave, rx, xc * 8, sg, sgx);
  pb_dw_wave_sum<NCO, NWT>(red, NW, wave, lane, accw);
  float* pw = a.partw + (long)blockIdx.x * COUT * Cin;
  for (int i = tid; i < COUT * NW; i += 256) {
    const int co = i / NW, c = i - co * NW;
    pw[(long)co * Cin + n0 + c] = red[co * NW + c];
  }
  float* xp = xparts + (long)blockIdx.x * 2 * Cin;
  for (int i = tid; i < 2 * NW; i += 256) {
    const int k = i / NW, c = i - k * NW;
    xp[(long)k * Cin + n0 + c] = pb_xsum_col(gbuf, RGX, NW, k, c, a.xrstd[n0 + c]);
  }
}

// the group width of the gred form for (Cin, Cout); 0: not taken
static int pw_bwd_gred_nw(int Cin, int Cout) {
  if (!(Cout == 16 || Cout == 24 || Cout == 32 || Cout == 64)) return 0;
  // Cout 64 at 48 columns spills under the 3-waves/SIMD bound (168 VGPRs); 32 columns fit (162)
  if (Cout == 64) return Cin % 32 == 0 ? 32 : 0;
  // 32-column groups wherever Cin allows (tools/pwgred_bench.py: 96->24 289 -> 256 us, 192->32
  // 139 -> 121 us against 48: no idle row group, 4 waves / SIMD), 48 for Cin = 144
  if (Cin % 32 == 0) return 32;
  if (Cin % 48 == 0) return 48;
  return 0;
}
static int pw_bwd_gred_rowblocks(long M, int Cin, int nw) {
  const long ntiles = cdivl(M, 32);
  const int groups = Cin / nw;
  const long want = std::max<long>(1, 768 / groups);   // ~3 resident blocks per CU over all groups
  return (int)std::max<long>(1, std::min<long>(cdivl(ntiles, 4), want));
}

struct PwBwdPlan {
  int kd, nci, nco, nxt, nx, wt, nblk;
  long chunk;
  size_t lds;
};

// the streaming kernel's shapes (expand convs without bias)
static bool pw_bwd_stream_ok(int Cin, int Cout, bool bias) {
  // 32->192 stays on the block kernel: 248 VGPRs (2 waves / SIMD), measured slower (168 vs 152 us)
  return !bias && ((Cin == 16 && Cout == 96) || (Cin == 24 && Cout == 144));
}
// blocks of the streaming launch: 3 per CU (the register budget of the 16->96 form), at most one
// 4-wave group per 4 tiles
static int pw_bwd_stream_blocks(long M) {
  const long ntiles = cdivl(M, 32);
  return (int)std::max<long>(1, std::min<long>(cdivl(ntiles, 4), 3L * 256));
}

static bool pw_bwd_ok(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0 || Cin % 8 || Cout % 8 || Cin > 192 || Cout > 512) return false;
  const int nco = cdiv(Cout, 16), nci = cdiv(Cin + 1, 16);
  return nco * nci <= 64;
}

static PwBwdPlan pw_bwd_plan(long M, int Cin, int Cout, bool bias) {
  PwBwdPlan p;
  p.kd = cdiv(Cout, 32) * 32;
  p.nco = cdiv(Cout, 16);
  p.nci = cdiv(Cin + (bias ? 1 : 0), 16);
  p.nxt = cdiv(Cin, 16);
  p.nx = p.nxt <= 2 ? 2 : p.nxt <= 4 ? 4 : p.nxt <= 8 ? 8 : 12;
  const int per = cdiv(p.nco * p.nci, 4);
  p.wt = per <= 4 ? 4 : per <= 6 ? 6 : per <= 8 ? 8 : 16;
  p.lds = (size_t)Cout * PB_CF * 4 + (size_t)Cin * 2 * 4 +
          ((size_t)PB_BM * (p.kd + 8) + (size_t)PB_BM * (p.nci * 16 + 8) + (size_t)p.nxt * 16 * (p.kd + 8)) * 2;
  // two rounds of the 3 resident blocks per CU (measured: 768 / 1024 / 1280 / 1536 / 2048 /
  // 3072 blocks -> 3471 / 3722 / 3572 / 3326 / 3531 / 3519 us over tools/pwbwd_bench.py)
  const long steps = cdivl(M, PB_BM);
  p.nblk = (int)std::max<long>(1, std::min<long>(steps, 1536));
  p.chunk = cdivl(steps, p.nblk) * PB_BM;
  p.nblk = (int)cdivl(M, p.chunk);
  return p;
}

// the arguments every form takes; the launch-specific fields (partb / chunk / kd .. nxt of the
// block kernel's plan, dyp, wt0) stay 0 / NULL and are set by name where a form uses them
static PwBwdArgs pb_args(const void* dz, const void* y, const void* x, const void* wt1, void* dx, float* partw,
                         const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* coef, int act, const float* xmean, const float* xrstd, const float* xgamma,
                         const float* xbeta, int xact, long M, int Cin, int Cout) {
  PwBwdArgs a{};
  a.dz = (const bf16_t*)dz, a.y = (const bf16_t*)y, a.x = (const bf16_t*)x, a.wt1 = (const bf16_t*)wt1;
  a.dx = (bf16_t*)dx, a.partw = partw;
  a.mean = mean, a.rstd = rstd, a.gamma = gamma, a.beta = beta, a.coef = coef, a.act = act;
  a.xmean = xmean, a.xrstd = xrstd, a.xgamma = xgamma, a.xbeta = xbeta, a.xact = xact;
  a.M = M, a.Cin = Cin, a.Cout = Cout;
  return a;
}

// the pointer checks of both run functions, in two steps so that each keeps its place among the
// entry's own checks: `have` is the entry's list of required pointers
static int pb_check_ptrs(const char* who, bool have, const void* wt0) {
  ROD_CHECK_ARG(have, "%s: NULL argument", who);
  ROD_CHECK_ARG((((uintptr_t)wt0) & 15) == 0, "%s_rc: wt0 must be 16-byte aligned", who);
  return 0;
}
static int pb_check_align(const char* who, const void* dz, const void* y, const void* x, const void* wt1,
                          const void* dx, const void* dyp) {
  ROD_CHECK_ARG(((((uintptr_t)dz) | ((uintptr_t)y) | ((uintptr_t)x) | ((uintptr_t)wt1) | ((uintptr_t)dx) |
                  ((uintptr_t)dyp)) & 15) == 0,
                "%s: tensors must be 16-byte aligned", who);
  return 0;
}

}  // namespace rod

using namespace rod;

extern "C" {

int rod_pw_bwd_supported(int Cin, int Cout, int dtype) { return dtype == ROD_BF16 && pw_bwd_ok(Cin, Cout) ? 1 : 0; }

size_t rod_pw_bwd_workspace(long M, int Cin, int Cout) {
  if (!pw_bwd_ok(Cin, Cout) || M <= 0) return 0;
  const PwBwdPlan p = pw_bwd_plan(M, Cin, Cout, true);
  const size_t blk = pw_bwd_stream_ok(Cin, Cout, false) ? (size_t)std::max(p.nblk, pw_bwd_stream_blocks(M)) : p.nblk;
  return blk * Cout * (Cin + 1) * sizeof(float) + 64;
}

int rod_pw_bwd_rc_supported(long M, int Cin, int Cout, int dtype) {
  return dtype == ROD_BF16 && M > 0 && pw_bwd_ok(Cin, Cout) && pw_bwd_stream_ok(Cin, Cout, false) ? 1 : 0;
}

static int pw_bwd_run(const void* dz, const void* y, const void* wt0, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int act, const float* coef, const void* x,
                      const float* xmean, const float* xrstd, const float* xgamma, const float* xbeta, int xact,
                      const void* wt1, void* dx, float* dw, float* db, void* workspace, long M, int Cin, int Cout,
                      int dtype, void* stream) {
  ROD_CHECK_ARG(dtype == ROD_BF16, "rod_pw_bwd: bf16 only");
  ROD_CHECK_ARG(M > 0 && pw_bwd_ok(Cin, Cout), "rod_pw_bwd: unsupported shape M=%ld Cin=%d Cout=%d", M, Cin, Cout);
  if (const int e = pb_check_ptrs("rod_pw_bwd", dz && (y || wt0) && mean && rstd && coef && x && dw && workspace, wt0))
    return e;
  ROD_CHECK_ARG(!wt0 || (!db && rod_pw_bwd_rc_supported(M, Cin, Cout, dtype)),
                "rod_pw_bwd_rc: the recompute form takes the streaming shapes (16 -> 96, 24 -> 144) without bias");
  ROD_CHECK_ARG(!dx || wt1, "rod_pw_bwd: dx needs wt1");
  ROD_CHECK_ARG(!xmean || xrstd, "rod_pw_bwd: bad input prologue");
  if (const int e = pb_check_align("rod_pw_bwd", dz, y, x, wt1, dx, nullptr)) return e;
  const PwBwdPlan p = pw_bwd_plan(M, Cin, Cout, db != nullptr);
  ROD_CHECK_ARG(p.lds <= 160 * 1024, "rod_pw_bwd: LDS plan too large");
  hipStream_t s = ROD_STREAM(stream);
  float* partw = (float*)workspace;
  if (pw_bwd_stream_ok(Cin, Cout, db != nullptr)) {
    const int nblk = pw_bwd_stream_blocks(M);
    PwBwdArgs a = pb_args(dz, y, x, wt1, dx, partw, mean, rstd, gamma, beta, coef, act, xmean, xrstd, xgamma, xbeta,
                          xact, M, Cin, Cout);
    a.wt0 = (const bf16_t*)wt0;
    const long ntiles = cdivl(M, 32);
    // PR: input prologue, DXF: dx wanted, XL: the prologue without an activation (built for
    // either PR, selected only with it), RCF: y recomputed from wt0
    auto go = [&](auto CI, auto CO) {
      sel_bool(xmean != nullptr, [&](auto PR) {
        sel_bool(dx != nullptr, [&](auto DXF) {
          sel_bool(PR && xact == ROD_ACT_NONE, [&](auto XL) {
            sel_bool(wt0 != nullptr, [&](auto RCF) {
              const size_t lds = PbsGeo<CI, CO>::lds(RCF);
              launch_lds(pw_bwd_stream_kernel<CI, CO, PR, DXF, false, XL, RCF>, dim3(nblk), dim3(256), lds, s, a,
                         ntiles, nullptr);
            });
          });
        });
      });
    };
    if (Cin == 16 && Cout == 96) go(int_c<16>{}, int_c<96>{});
    else if (Cin == 24 && Cout == 144) go(int_c<24>{}, int_c<144>{});
    else ROD_CHECK_ARG(false, "rod_pw_bwd: no streaming kernel for Cin=%d Cout=%d", Cin, Cout);
    slab_sum(partw, dw, nblk, (long)Cout * Cin, s);
    return check_launch("rod_pw_bwd");
  }
  float* partb = db ? partw + (size_t)p.nblk * Cout * Cin : nullptr;
  PwBwdArgs a = pb_args(dz, y, x, wt1, dx, partw, mean, rstd, gamma, beta, coef, act, xmean, xrstd, xgamma, xbeta, xact,
                        M, Cin, Cout);
  a.partb = partb, a.chunk = p.chunk, a.kd = p.kd, a.nci = p.nci, a.nco = p.nco, a.nxt = p.nxt;
  // p.nx is 2 / 4 / 8 / 12 A tiles and p.wt 4 / 6 / 8 / 16 weight tiles per wave (pw_bwd_plan)
  const bool hit = sel_int<2, 4, 8, 12>(p.nx, [&](auto NX) {
    return sel_int<4, 6, 8, 16>(p.wt, [&](auto WT) {
      launch_lds(pw_bwd_kernel<NX, WT>, dim3(p.nblk), dim3(256), p.lds, s, a);
    });
  });
  ROD_CHECK_ARG(hit, "rod_pw_bwd: no kernel for nx=%d wt=%d", p.nx, p.wt);
  slab_sum(partw, dw, p.nblk, (long)Cout * Cin, s);
  if (db) slab_sum(partb, db, p.nblk, (long)Cout, s);
  return check_launch("rod_pw_bwd");
}

int rod_pw_bwd(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma,
               const float* beta, int act, const float* coef, const void* x, const float* xmean, const float* xrstd,
               const float* xgamma, const float* xbeta, int xact, const void* wt1, void* dx, float* dw, float* db,
               void* workspace, long M, int Cin, int Cout, int dtype, void* stream) {
  ROD_CHECK_ARG(y, "rod_pw_bwd: NULL y");
  return pw_bwd_run(dz, y, nullptr, mean, rstd, gamma, beta, act, coef, x, xmean, xrstd, xgamma, xbeta, xact, wt1, dx,
                    dw, db, workspace, M, Cin, Cout, dtype, stream);
}

int rod_pw_bwd_rc(const void* dz, const void* wt0, const float* mean, const float* rstd, const float* gamma,
                  const float* beta, int act, const float* coef, const void* x, const float* xmean, const float* xrstd,
                  const float* xgamma, const float* xbeta, int xact, const void* wt1, void* dx, float* dw,
                  void* workspace, long M, int Cin, int Cout, int dtype, void* stream) {
  ROD_CHECK_ARG(wt0, "rod_pw_bwd_rc: NULL wt0");
  return pw_bwd_run(dz, nullptr, wt0, mean, rstd, gamma, beta, act, coef, x, xmean, xrstd, xgamma, xbeta, xact, wt1,
                    dx, dw, nullptr, workspace, M, Cin, Cout, dtype, stream);
}


// expand shapes the gred entry takes (the streaming kernel with the input sums): 16 -> 96 only
// (168 VGPRs, 3 waves / SIMD); 24 -> 144 would need 268 (1 wave), and its input is usually also a
// residual source, whose gradient is a sum the sums could not be handed to anyway
static bool pw_bwd_xg_ok(int Cin, int Cout) { return Cin == 16 && Cout == 96 && pw_bwd_stream_ok(Cin, Cout, false); }

long rod_pw_bwd_gred_parts(long M, int Cin, int Cout, int dtype) {
  if (dtype == ROD_BF16 && M > 0 && pw_bwd_xg_ok(Cin, Cout)) return pw_bwd_stream_blocks(M);
  const int nw = dtype == ROD_BF16 && M > 0 ? pw_bwd_gred_nw(Cin, Cout) : 0;
  return nw ? pw_bwd_gred_rowblocks(M, Cin, nw) : 0;
}

size_t rod_pw_bwd_gred_workspace(long M, int Cin, int Cout) {
  if (M > 0 && pw_bwd_xg_ok(Cin, Cout)) return (size_t)pw_bwd_stream_blocks(M) * Cout * Cin * sizeof(float) + 64;
  const int nw = M > 0 ? pw_bwd_gred_nw(Cin, Cout) : 0;
  return nw ? (size_t)pw_bwd_gred_rowblocks(M, Cin, nw) * Cout * Cin * sizeof(float) + 64 : 0;
}

static int pw_bwd_gred_run(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, int act, const float* coef, const void* x, const float* xmean,
                           const float* xrstd, const float* xgamma, const float* xbeta, int xact, const void* wt1,
                           void* dx, void* dyp, float* dw, float* xparts, void* workspace, long M, int Cin, int Cout,
                           int dtype, void* stream, const void* wt0 = nullptr) {
  const bool sexp = dtype == ROD_BF16 && M > 0 && pw_bwd_xg_ok(Cin, Cout) && !dyp;
  const int nw = dtype == ROD_BF16 && M > 0 && !sexp ? pw_bwd_gred_nw(Cin, Cout) : 0;
  ROD_CHECK_ARG(nw || sexp, "rod_pw_bwd_gred: unsupported shape M=%ld Cin=%d Cout=%d dtype=%d", M, Cin, Cout,
                dtype);
  ROD_CHECK_ARG(!wt0 || sexp, "rod_pw_bwd_gred_rc: the recompute form takes the 16 -> 96 expand only");
  if (const int e = pb_check_ptrs("rod_pw_bwd_gred", dz && (y || wt0) && mean && rstd && coef && x && xmean && xrstd &&
                                  dw && xparts && workspace, wt0))
    return e;
  ROD_CHECK_ARG((dx != nullptr) != (dyp != nullptr) && wt1,
                "rod_pw_bwd_gred: wt1 and exactly one of dx / dyp required (the sums are over dx)");
  if (const int e = pb_check_align("rod_pw_bwd_gred", dz, y, x, wt1, dx, dyp)) return e;
  ROD_CHECK_ARG(M * Cin * 2 < (1L << 31) && M * Cout * 2 < (1L << 31), "rod_pw_bwd_gred: tensor over 2 GiB");
  hipStream_t s = ROD_STREAM(stream);
  float* partw = (float*)workspace;
  if (sexp) {   // an expand shape: the streaming kernel with the input BatchNorm's sums
    const int nb = pw_bwd_stream_blocks(M);
    PwBwdArgs a = pb_args(dz, y, x, wt1, dx, partw, mean, rstd, gamma, beta, coef, act, xmean, xrstd, xgamma, xbeta,
                          xact, M, Cin, Cout);
    a.wt0 = (const bf16_t*)wt0;
    const long nt = cdivl(M, 32);
    // sexp: 16 -> 96 only (pw_bwd_xg_ok)
    sel_bool(xact == ROD_ACT_NONE, [&](auto XL) {
      sel_bool(wt0 != nullptr, [&](auto RCF) {
        const size_t lds = PbsGeo<16, 96>::lds(RCF);
        launch_lds(pw_bwd_stream_kernel<16, 96, true, true, true, XL, RCF>, dim3(nb), dim3(256), lds, s, a, nt, xparts);
      });
    });
    slab_sum(partw, dw, nb, (long)Cout * Cin, s);
    return check_launch("rod_pw_bwd_gred");
  }
  const int nblk = pw_bwd_gred_rowblocks(M, Cin, nw);
  PwBwdArgs a = pb_args(dz, y, x, wt1, dx, partw, mean, rstd, gamma, beta, coef, act, xmean, xrstd, xgamma, xbeta, xact,
                        M, Cin, Cout);
  a.dyp = (bf16_t*)dyp;
  const long ntiles = cdivl(M, 32);
  const dim3 grid(nblk, Cin / nw);
  // the inverted-residual block's case takes the packed form; at 48 columns it measured slower
  // (144->24: 569 vs 433 us), so there the per-element form runs
  const bool fast = act == ROD_ACT_NONE && xact == ROD_ACT_RELU6 && nw == 32;
  // Cout 16 / 24 / 32 / 64 in groups of nw = 32 or 48 columns (pw_bwd_gred_nw); 48 columns take
  // neither Cout 64 nor the packed form, so those are not built
  const bool hit = sel_int<16, 24, 32, 64>(Cout, [&](auto CO) {
    return sel_int<32, 48>(nw, [&](auto NW) {
      return sel_bool(fast, [&](auto F) {
        constexpr int co = decltype(CO)::value, nwc = decltype(NW)::value;
        constexpr bool f = decltype(F)::value;
        if constexpr (nwc == 48 && (co == 64 || f)) {
          return false;
        } else {
          sel_bool(dyp != nullptr, [&](auto D) {
            launch_lds(pw_bwd_gred_kernel<co, nwc, f, D>, grid, dim3(256), PbgGeo<co, nwc>::lds(), s, a, ntiles,
                       xparts);
          });
          return true;
        }
      });
    });
  });
  ROD_CHECK_ARG(hit, "rod_pw_bwd_gred: no kernel for Cout=%d nw=%d", Cout, nw);
  slab_sum(partw, dw, nblk, (long)Cout * Cin, s);
  return check_launch("rod_pw_bwd_gred");
}

int rod_pw_bwd_gred(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, int act, const float* coef, const void* x, const float* xmean,
                    const float* xrstd, const float* xgamma, const float* xbeta, int xact, const void* wt1,
                    void* dx, float* dw, float* xparts, void* workspace, long M, int Cin, int Cout, int dtype,
                    void* stream) {
  ROD_CHECK_ARG(dx, "rod_pw_bwd_gred: dx required");
  return pw_bwd_gred_run(dz, y, mean, rstd, gamma, beta, act, coef, x, xmean, xrstd, xgamma, xbeta, xact, wt1, dx,
                         nullptr, dw, xparts, workspace, M, Cin, Cout, dtype, stream);
}

int rod_pw_bwd_gred_dyp(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int act, const float* coef, const void* x, const float* xmean,
                        const float* xrstd, const float* xgamma, const float* xbeta, int xact, const void* wt1,
                        void* dyp, float* dw, float* xparts, void* workspace, long M, int Cin, int Cout, int dtype,
                        void* stream) {
  ROD_CHECK_ARG(dyp, "rod_pw_bwd_gred_dyp: dyp required");
  return pw_bwd_gred_run(dz, y, mean, rstd, gamma, beta, act, coef, x, xmean, xrstd, xgamma, xbeta, xact, wt1,
                         nullptr, dyp, dw, xparts, workspace, M, Cin, Cout, dtype, stream);
}

int rod_pw_bwd_gred_rc(const void* dz, const void* wt0, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, int act, const float* coef, const void* x, const float* xmean,
                       const float* xrstd, const float* xgamma, const float* xbeta, int xact, const void* wt1,
                       void* dx, float* dw, float* xparts, void* workspace, long M, int Cin, int Cout, int dtype,
                       void* stream) {
  ROD_CHECK_ARG(dx && wt0, "rod_pw_bwd_gred_rc: dx and wt0 required");
  return pw_bwd_gred_run(dz, nullptr, mean, rstd, gamma, beta, act, coef, x, xmean, xrstd, xgamma, xbeta, xact, wt1,
                         dx, nullptr, dw, xparts, workspace, M, Cin, Cout, dtype, stream, wt0);
}

}  // extern "C"
