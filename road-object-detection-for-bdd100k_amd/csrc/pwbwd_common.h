// pwbwd_common.h — the one copy of the fused 1x1 backward's arithmetic, shared by the three kernels
// of pwbwd.hip (pw_bwd_kernel, pw_bwd_stream_kernel, pw_bwd_gred_kernel) and the BNB loader of
// stem_wgrad_kernel (gemm.hip).
//
// dx is bit-identical to the unfused chain (tests/test_gpu_pwbwd.py) because every kernel forms dy
// with ONE operation sequence, pb_dy1 below, and runs the MFMA in the same k order.  The
// per-element, packed-linear and packed-ReLU6 forms stay deliberately distinct.
// Everything is __forceinline__ on the caller's registers and LDS pointers; these kernels run on
// occupancy (profiles/pwbwd_share_resources.md; DESIGN.md §5 lists any site kept inline).
#pragma once
#include "rod_common.h"

namespace rod {

// ---- activation gate and dy ---------------------------------------------------------------------
// act_grad(z, act) as one select chain: z > 0 ? (z < hi ? 1 : 0) : lo — the same {0, 0.2, 1}
// factors (NaN -> lo, as the compare-based forms give) without a per-element switch
struct PbGate {
  float ghi, glo;
};
// Callers hold the two values as plain floats for the launch and build the PbGate at the call: held
// as an object across the row loop it changed pw_bwd_stream_kernel's schedule (24 -> 144 with the
// ReLU6 prologue: 172 to 154 VGPRs and 328 to 349 us at 720p b8).
__device__ __forceinline__ float pb_gate_hi(int act) { return act == ROD_ACT_RELU6 ? 6.f : INFINITY; }
__device__ __forceinline__ float pb_gate_lo(int act) {
  return act == ROD_ACT_LEAKY ? 0.2f : act == ROD_ACT_NONE ? 1.f : 0.f;
}
// dy of one element, unrounded: the caller rounds to bf16 and masks rows past M.  (dz, y) come in
// as stored and are widened here, y first: widened at the call site pw_bwd_kernel<2, 4> took 106
// VGPRs instead of 104 and lost its fourth wave per SIMD.
__device__ __forceinline__ float pb_dy1(const PbGate& gt, float sc, float sh, float ca, float k1, float k0, bf16_t dz,
                                        bf16_t y) {
  const float yj = (float)y;
  const float z = fmaf(yj, sc, sh);
  const float g = (float)dz * (z > 0.f ? (z < gt.ghi ? 1.f : 0.f) : gt.glo);
  return bn_bwd_apply1<bf16_t>(ca, g, k1, k0, 0.f, yj);
}

// one channel's constants: the forward affine (for the gate) and the folded backward coefficients
__device__ __forceinline__ void pb_bn_d1(const float* mean, const float* rstd, const float* gamma, const float* beta,
                                         const float* coef, int Cout, int c, float& sc, float& sh, float& ca,
                                         float& k1, float& k0) {
  bn_affine(mean, rstd, gamma, beta, c, sc, sh);
  ca = coef[c];
  bn_bwd_k_fold(ca, mean[c], rstd[c], coef[Cout + c], coef[2 * Cout + c], k1, k0);
}

// lane constants: CW consecutive channels from c0, in registers for the whole launch
template <int CW>
struct PbBnD {
  float sc[CW], sh[CW], ca[CW], k1[CW], k0[CW];
  __device__ __forceinline__ void init(const float* mean, const float* rstd, const float* gamma, const float* beta,
                                       const float* coef, int Cout, int c0) {
#pragma unroll
    for (int e = 0; e < CW; ++e) pb_bn_d1(mean, rstd, gamma, beta, coef, Cout, c0 + e, sc[e], sh[e], ca[e], k1[e], k0[e]);
  }
  // dy of the lane's chunk (V: bf16x4 / bf16x8 of CW elements), rounded, unmasked
  template <typename V>
  __device__ __forceinline__ V dy(const PbGate& gt, const V& dz, const V& y) const {
    V o;
#pragma unroll
    for (int e = 0; e < CW; ++e) o[e] = (bf16_t)pb_dy1(gt, sc[e], sh[e], ca[e], k1[e], k0[e], dz[e], y[e]);
    return o;
  }
};

typedef float pb_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 pb_b2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pb_f2 pb_unpack(unsigned u) {   // bf16 pair (low, high) -> fp32 pair
  return pb_f2{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}
__device__ __forceinline__ unsigned pb_round(pb_f2 v) {    // one v_cvt_pk_bf16_f32 (RNE per element)
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, pb_b2));
}
// ReLU6 gradient gate (0 < z < 6; NaN -> closed) as one unsigned compare on the bits
__device__ __forceinline__ bool pb_relu6_open(float z) { return __builtin_bit_cast(unsigned, z) - 1u < 0x40BFFFFFu; }

// packed-linear dy of a channel pair (linear output BatchNorm: g = dz), unrounded:
// fma(a, dz, fma(k1, y, k0)) — pb_dy1 with the gate at 1
__device__ __forceinline__ pb_f2 pb_dy_pair_linear(pb_f2 ca2, pb_f2 k12, pb_f2 k02, pb_f2 d2, pb_f2 y2) {
  return __builtin_elementwise_fma(ca2, d2, __builtin_elementwise_fma(k12, y2, k02));
}

// ---- input prologue: x_p = act_x(BN_x(x)), rounded to bf16; rows past M stay 0 (not act(shift)) --
// 8 fp32 constants of a chunk from an LDS (or global) table, as two 16-byte reads
__device__ __forceinline__ void pb_ld8(const float* p, float (&v)[8]) {
  const f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = lo[e];
    v[4 + e] = hi[e];
  }
}
__device__ __forceinline__ bf16x8 pb_xpro(const bf16x8& x, const float (&sc)[8], const float (&sh)[8], int xact,
                                          bool rok) {
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = rok ? (bf16_t)act_fwd(fmaf((float)x[e], sc[e], sh[e]), xact) : (bf16_t)0.f;
  return v;
}
// linear input BatchNorm (xact NONE), packed pairs
__device__ __forceinline__ bf16x8 pb_xpro_linear(const bf16x8& x, const float (&sc)[8], const float (&sh)[8], bool rok) {
  const u32x4_t u = __builtin_bit_cast(u32x4_t, x);
  u32x4_t o;
#pragma unroll
  for (int h2 = 0; h2 < 4; ++h2) {
    const pb_f2 z2 = __builtin_elementwise_fma(pb_unpack(u[h2]), pb_f2{sc[2 * h2], sc[2 * h2 + 1]},
                                               pb_f2{sh[2 * h2], sh[2 * h2 + 1]});
    o[h2] = rok ? pb_round(z2) : 0u;
  }
  return __builtin_bit_cast(bf16x8, o);
}
// ReLU6 input BatchNorm, packed pairs (constants as register pairs)
__device__ __forceinline__ bf16x8 pb_xpro_relu6(const bf16x8& x, const pb_f2 (&sc2)[4], const pb_f2 (&sh2)[4], bool rok) {
  const u32x4_t xu = __builtin_bit_cast(u32x4_t, x);
  u32x4_t vu;
#pragma unroll
  for (int h2 = 0; h2 < 4; ++h2) {
    const pb_f2 z2 = __builtin_elementwise_fma(pb_unpack(xu[h2]), sc2[h2], sh2[h2]);
    const pb_f2 t2 = {act_t<ROD_ACT_RELU6>(z2.x), act_t<ROD_ACT_RELU6>(z2.y)};
    vu[h2] = rok ? pb_round(t2) : 0u;
  }
  return __builtin_bit_cast(bf16x8, vu);
}

// ---- the input BatchNorm's backward sums over (dx, x): sg += g, sgx += g*(x - mean) --------------
// (the rstd factor is applied once per column at the end: pb_xsum_col).  The per-element form is
// gred_acc(dx, x, sc, sh, mu, rs = 1, xact, sg, sgx) of rod_common.h; the two below are its
// linear (g = dx) and packed-ReLU6 siblings.
__device__ __forceinline__ void pb_xsum_linear(float dx, float x, float mu, float& sg, float& sgx) {
  sg += dx;
  sgx = fmaf(dx, x - mu, sgx);
}
__device__ __forceinline__ void pb_xsum_relu6(const bf16x8& dx, const bf16x8& x, const pb_f2 (&sc2)[4],
                                              const pb_f2 (&sh2)[4], const pb_f2 (&mu2)[4], pb_f2 (&sg2)[4],
                                              pb_f2 (&sgx2)[4]) {
  const u32x4_t du = __builtin_bit_cast(u32x4_t, dx), xu = __builtin_bit_cast(u32x4_t, x);
#pragma unroll
  for (int h2 = 0; h2 < 4; ++h2) {
    const pb_f2 x2 = pb_unpack(xu[h2]), d2 = pb_unpack(du[h2]);
    const pb_f2 z2 = __builtin_elementwise_fma(x2, sc2[h2], sh2[h2]);
    const pb_f2 g2 = {pb_relu6_open(z2.x) ? d2.x : 0.f, pb_relu6_open(z2.y) ? d2.y : 0.f};
    sg2[h2] += g2;
    sgx2[h2] = __builtin_elementwise_fma(g2, x2 - mu2[h2], sgx2[h2]);
  }
}
// a lane's 8 columns of (sg, sgx) -> staging [4 waves][RGX row groups][2][NC columns]
__device__ __forceinline__ void pb_xsum_stage(float* gbuf, int RGX, int NC, int wave, int rx, int c0,
                                              const float (&sg)[8], const float (&sgx)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    gbuf[((wave * RGX + rx) * 2 + 0) * NC + c0 + e] = sg[e];
    gbuf[((wave * RGX + rx) * 2 + 1) * NC + c0 + e] = sgx[e];
  }
}
// column c of sum k (0: g, 1: g*(x - mean), scaled by xrstd): waves, then row groups, in order
__device__ __forceinline__ float pb_xsum_col(const float* gbuf, int RGX, int NC, int k, int c, float xrstd) {
  float s = 0.f;
  for (int w = 0; w < 4; ++w)
    for (int r = 0; r < RGX; ++r) s += gbuf[((w * RGX + r) * 2 + k) * NC + c];
  return k ? s * xrstd : s;
}

// ---- MFMA pieces (v_mfma_f32_16x16x32_bf16) ------------------------------------------------------
// a transposed operand fragment: rows [8g + q, +4] x 4 columns at p (p already holds the lane's
// 8g + q row and 4p column offset), two ds_read_b64_tr_b16
__device__ __forceinline__ bf16x8 pb_tr_frag(const bf16_t* p, int ld) {
  const bf16x4 lo = lds_tr_read(p), hi = lds_tr_read(p + 4 * ld);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// acc += dy^T . x of one 16 (co) x 16 (ci) tile over the 32 rows at Ds / Xs (the row base is the
// caller's: the block kernel steps it through its 64 rows)
__device__ __forceinline__ void pb_dw_tile(const bf16_t* Ds, int LDD, const bf16_t* Xs, int LDX, int ct, int it,
                                           int lane, f32x4& acc) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const bf16x8 fa = pb_tr_frag(Ds + (8 * g + q) * LDD + ct * 16 + 4 * p, LDD);
  const bf16x8 fb = pb_tr_frag(Xs + (8 * g + q) * LDX + it * 16 + 4 * p, LDX);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
}
// all NCO x NT tiles of a wave's 32-row tile, the dy fragment read once per co tile
template <int NCO, int NT>
__device__ __forceinline__ void pb_dw_tiles(const bf16_t* Ds, int LDD, const bf16_t* Xs, int LDX, int lane,
                                            f32x4 (&accw)[NCO][NT]) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
  for (int ct = 0; ct < NCO; ++ct) {
    const bf16x8 fa = pb_tr_frag(Ds + (8 * g + q) * LDD + ct * 16 + 4 * p, LDD);
#pragma unroll
    for (int it = 0; it < NT; ++it) {
      const bf16x8 fb = pb_tr_frag(Xs + (8 * g + q) * LDX + it * 16 + 4 * p, LDX);
      accw[ct][it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, accw[ct][it], 0, 0, 0);
    }
  }
}
// accx = dy . W for 16 rows: drow = the half's dy rows, wrow = the wt1 image, both [..][LDD] with
// k = co along the row; KT k steps of 32, NT column tiles of 16
template <int KT, int NT>
__device__ __forceinline__ void pb_dx_half(const bf16_t* drow, const bf16_t* wrow, int LDD, int lane,
                                           f32x4 (&accx)[NT]) {
  const int g = lane >> 4, li = lane & 15;
#pragma unroll
  for (int j = 0; j < NT; ++j) accx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KT; ++s) {
    const bf16x8 fa = *(const bf16x8*)(drow + li * LDD + s * 32 + 8 * g);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16x8 fb = *(const bf16x8*)(wrow + (j * 16 + li) * LDD + s * 32 + 8 * g);
      accx[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, accx[j], 0, 0, 0);
    }
  }
}
// RC: y^T of a 16-row half, tile by tile: A = forward weight rows (16 channels x k), B = the half's
// x_p rows (k x 16 rows), k zero-padded to 32 (one step, CIN <= 32); lane (g, li) gets channels
// 16ct + 4g .. +3 of row li, rounded to bf16 once — the stored y — and writes them into the dy rows
template <int NCO, int CIN>
__device__ __forceinline__ void pb_rc_y_half(const bf16_t* xrow, int LDX, const bf16_t* Wf, int LDW, bf16_t* drow,
                                             int LDD, int lane) {
  const int g = lane >> 4, li = lane & 15;
  const bf16x8 zero8 = {};
  const bf16x8 fb = 8 * g < CIN ? *(const bf16x8*)(xrow + li * LDX + 8 * g) : zero8;
#pragma unroll
  for (int ct = 0; ct < NCO; ++ct) {
    const bf16x8 fw = 8 * g < CIN ? *(const bf16x8*)(Wf + (ct * 16 + li) * LDW + 8 * g) : zero8;
    const f32x4 yt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fb, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    const bf16x4 yb = {(bf16_t)yt[0], (bf16_t)yt[1], (bf16_t)yt[2], (bf16_t)yt[3]};
    *(bf16x4*)(drow + li * LDD + ct * 16 + 4 * g) = yb;
  }
}

// ---- tails --------------------------------------------------------------------------------------
// the block's dW: its four waves add their accumulators in wave order into red [NCO*16][LR]
// (block-wide: every wave calls it; red may alias the row buffers, retired by the caller's barrier)
template <int NCO, int NT>
__device__ __forceinline__ void pb_dw_wave_sum(float* red, int LR, int wave, int lane, const f32x4 (&accw)[NCO][NT]) {
  const int g = lane >> 4, li = lane & 15;
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* d = red + (ct * 16 + 4 * g + r) * LR + it * 16 + li;
            *d = w == 0 ? accw[ct][it][r] : *d + accw[ct][it][r];
          }
    }
    __syncthreads();
  }
}

// ---- tile bookkeeping (32-row tiles behind buffer resources) --------------------------------------
__device__ __forceinline__ long pb_rows_of(long M, long row0) { return row0 < M ? (M - row0 < 32 ? M - row0 : 32) : 0; }
// whole rows [row0, min(row0 + 32, M)) of rowbytes each (row0 >= M: an empty resource, loads give 0)
__device__ __forceinline__ rsrc_t pb_rsrc_rows(const void* base, long M, long row0, int rowbytes) {
  return rod_rsrc((const char*)base + (row0 < M ? row0 : 0) * rowbytes, (unsigned)(pb_rows_of(M, row0) * rowbytes));
}
// the same rows of one column group: nw bf16 columns from n0 of rows ld elements long
__device__ __forceinline__ rsrc_t pb_rsrc_cols(const void* base, long M, long row0, int ld, int n0, int nw) {
  const long r = pb_rows_of(M, row0);
  return rod_rsrc((const char*)base + ((row0 < M ? row0 : 0) * ld + n0) * 2, r > 0 ? (unsigned)(((r - 1) * ld + nw) * 2) : 0u);
}
// lane offset (bytes) of chunk j inside a 16-row half: a lane of row group rg owns rows rg + RG*j,
// j < JN; v0 is its offset at j = 0 (ROD_OOB for an idle lane) and rowbytes the row pitch.  Where
// the groups tile the half exactly there is no row to drop and the compare goes away.
template <int JN, int RG>
__device__ __forceinline__ unsigned pb_lane_off(unsigned v0, int rg, int j, int rowbytes) {
  if constexpr (JN * RG == 16) return v0 + (unsigned)(j * RG * rowbytes);
  else return rg + RG * j < 16 ? v0 + (unsigned)(j * RG * rowbytes) : ROD_OOB;
}
// zero n8 16-byte chunks of LDS (dy columns >= Cout and x columns >= Cin then stay 0)
__device__ __forceinline__ void pb_lds_zero(void* smem, int n8, int tid) {
  for (int i = tid; i < n8; i += 256) {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.f;
    ((bf16x8*)smem)[i] = z;
  }
}
// the wt1 image: rows [0, rows) of wt1 ([..][Cout], starting at the caller's first row) -> Ws [rows][LDD]
__device__ __forceinline__ void pb_load_wt1(bf16_t* Ws, int LDD, const bf16_t* wt1, int rows, int Cout, int tid) {
  const int cch = Cout / 8;
  for (int i = tid; i < rows * cch; i += 256) {
    const int ci = i / cch, cc = i - ci * cch;
    *(bf16x8*)(Ws + ci * LDD + cc * 8) = *(const bf16x8*)(wt1 + (long)ci * Cout + cc * 8);
  }
}

}  // namespace rod
