// dwfused_common.h — the one copy of what the four fused depthwise backward kernels share:
// dw3x3_bwd_fused2_kernel (stride 1, and its PW form), dw3x3_bwd_fused_s2_kernel (stride 2, fp32,
// scalar), dw3x3_bwd_fused_s2p_kernel (stride 2, bf16, packed) in depthwise.hip and
// dw3x3_bwd_fused_rc_kernel (stride 2, bf16, expand recomputed) in dwrc.hip.  They evaluate the
// same per-element expressions in the same order; a rounding or gating change is made here once.
// Everything is __forceinline__ and works on the caller's registers
// (profiles/dwfused_share_resources.md); fused2 keeps its own grouped epilogue.
//
// Per element, with channel pairs as packed fp32 ops (v_pk_fma / v_pk_mul / v_pk_add):
//   x   = round_T(act_e(fma(ye, sc_e, sh_e)))                      DwfBnE::x_of — BN_e prologue
//   dy  = round_T(fma(a, gate_d(z_d, dz), fma(k1, yd [- m], k0)))  DwfBnD::dy_of — bn_bwd_apply1<T>,
//         z_d = fma(yd, sc_d, sh_d); the caller masks and rounds
//   dx  = one v_cvt_pk_bf16_f32 per pair, the rounded value read back by a shift / mask (dwf_dx_pair)
//   g   = gate_e(z_e, dx_rounded), sg += g, sgx = fma(g, fma(ye, rstd_e, -mean_e * rstd_e), sgx)
//         DwfBnE::sum — z_e is the prologue's own pre-activation of the same element
// The activation gradients are specialised (gate2: ReLU6 as one compare + select on the bits,
// else the run-time act_grad chain).
#pragma once
#include "dw_common.h"

namespace rod {

// channel v of a per-thread constant held as pairs (the scalar fp32 kernel's reads)
template <int VP>
__device__ __forceinline__ float dwf_lane(const dw_f2 (&a)[VP], int v) { return a[v >> 1][v & 1]; }

// the nine filter taps of channels c .. c + 2 VP - 1 as pairs
template <int VP>
__device__ __forceinline__ void dwf_taps(const float* w, int C, int c, dw_f2 (&wr)[9][VP]) {
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int h = 0; h < VP; ++h) wr[k][h] = dw_f2{w[k * C + c + 2 * h], w[k * C + c + 2 * h + 1]};
}

// bn_affine for the adjacent channels c, c + 1 as a pair.  Both channels' values are loaded before
// either is used, so that the set-up's loads merge into pair loads issued together (loaded one
// channel at a time, each waits for the one before it: a latency chain the small maps feel).
__device__ __forceinline__ void dwf_affine2(const float* mean, const float* rstd, const float* gamma,
                                            const float* beta, int c, dw_f2& sc, dw_f2& sh) {
  const dw_f2 mu = dw_f2{mean[c], mean[c + 1]}, rs = dw_f2{rstd[c], rstd[c + 1]};
  sc = gamma ? rs * dw_f2{gamma[c], gamma[c + 1]} : rs;
  sh = (beta ? dw_f2{beta[c], beta[c + 1]} : dw_f2{0.f, 0.f}) - mu * sc;
}

// BN_e: the BatchNorm + activation between the producer's ye and the depthwise input x.
// PACT: -1 no prologue (x = ye), ROD_ACT_RELU6 the inlined form, else the run-time activation;
// RED: also BN_e's backward sums over (dx, ye).
template <int VP, int PACT, bool RED>
struct DwfBnE {
  dw_f2 psc[VP], psh[VP], ers[VP], enb[VP];   // z = fma(ye, psc, psh); yhat = fma(ye, ers, enb)
  int pact = 0;
  __device__ __forceinline__ void init(const BnPro& pro, int c) {
    if constexpr (PACT >= 0) {
      pact = pro.act;
#pragma unroll
      for (int h = 0; h < VP; ++h) {
        dwf_affine2(pro.mean, pro.rstd, pro.gamma, pro.beta, c + 2 * h, psc[h], psh[h]);
        if constexpr (RED) {
          ers[h] = dw_f2{pro.rstd[c + 2 * h], pro.rstd[c + 2 * h + 1]};
          enb[h] = dw_f2{-pro.mean[c + 2 * h] * ers[h].x, -pro.mean[c + 2 * h + 1] * ers[h].y};
        }
      }
    }
  }
  // pair h of x from the raw ye pair, rounded to T; with RED the pre-activation z (the gradient
  // gate of this element) is left in `gate`
  template <typename T>
  __device__ __forceinline__ dw_f2 x_of(int h, dw_f2 yr, dw_f2& gate, T) const {
    if constexpr (PACT >= 0) {
      const dw_f2 z = f2fma(yr, psc[h], psh[h]);
      dw_f2 t;
      if constexpr (PACT == ROD_ACT_RELU6) t = dw_f2{act_t<ROD_ACT_RELU6>(z.x), act_t<ROD_ACT_RELU6>(z.y)};
      else t = dw_f2{act_fwd(z.x, pact), act_fwd(z.y, pact)};
      if constexpr (RED) gate = z;
      return round2(t, T{});
    } else {
      return yr;
    }
  }
  // BN_e's partial sums from the rounded dx pair; `on` = false adds zeros (a column off the map)
  __device__ __forceinline__ void sum(int h, dw_f2& sg, dw_f2& sgx, dw_f2 gate, dw_f2 dxr, dw_f2 yr,
                                      bool on = true) const {
    const dw_f2 g = on ? gate2<PACT>(gate, dxr, pact) : dw_f2{0.f, 0.f};
    sg += g;
    sgx = f2fma(g, f2fma(yr, ers[h], enb[h]), sgx);
  }
};

// BN_d: the BatchNorm + activation after the depthwise, whose backward apply forms dy from
// (dz, yd).  BACT: ROD_ACT_RELU6 inlined, else the run-time activation.
template <typename T, int VP, int BACT>
struct DwfBnD {
  dw_f2 dsc[VP], dsh[VP], da[VP], k1[VP], k0[VP], m[VP];   // k1 / k0 / m: bn_bwd_k's triple
  int act;
  __device__ __forceinline__ void init(const DwBwdBn& bd, int C, int c) {
    act = bd.act;
#pragma unroll
    for (int h = 0; h < VP; ++h) {
      const int c0 = c + 2 * h;
      float k10, k00, k11, k01, m0, m1;
      dwf_affine2(bd.mean, bd.rstd, bd.gamma, bd.beta, c0, dsc[h], dsh[h]);
      const dw_f2 mu = dw_f2{bd.mean[c0], bd.mean[c0 + 1]}, rs = dw_f2{bd.rstd[c0], bd.rstd[c0 + 1]};
      const dw_f2 mg = dw_f2{bd.coef[C + c0], bd.coef[C + c0 + 1]}, mgx = dw_f2{bd.coef[2 * C + c0], bd.coef[2 * C + c0 + 1]};
      da[h] = dw_f2{bd.coef[c0], bd.coef[c0 + 1]};
      bn_bwd_k<T>(da[h].x, mu.x, rs.x, mg.x, mgx.x, k10, k00, m0);
      bn_bwd_k<T>(da[h].y, mu.y, rs.y, mg.y, mgx.y, k11, k01, m1);
      k1[h] = dw_f2{k10, k11};
      k0[h] = dw_f2{k00, k01};
      m[h] = dw_f2{m0, m1};   // bf16 storage: the folded form, m unused
    }
  }
  // the BatchNorm-backward apply of pair h (bn_bwd_apply1<T>, pairwise), unrounded
  __device__ __forceinline__ dw_f2 dy_of(int h, dw_f2 yv, dw_f2 zv) const {
    const dw_f2 z = f2fma(yv, dsc[h], dsh[h]);
    const dw_f2 g = gate2<BACT>(z, zv, act);
    const dw_f2 yc = sizeof(T) == 4 ? yv - m[h] : yv;
    return f2fma(da[h], g, f2fma(k1[h], yc, k0[h]));
  }
};

// dx pair h into the output pack (bf16: one v_cvt_pk_bf16_f32), and the pair as stored — rounded,
// back in fp32 by a shift / mask — which BN_e's sums take
template <typename T, int V>
__device__ __forceinline__ void dwf_dx_pair(PackV<T, V>& o, int h, dw_f2 a) {
  if constexpr (sizeof(T) == 2) {
    const dw_b2 b = __builtin_convertvector(a, dw_b2);
    o.v[2 * h] = b.x;
    o.v[2 * h + 1] = b.y;
  } else {
    o.set(2 * h, a.x);
    o.set(2 * h + 1, a.y);
  }
}
template <typename T, int V>
__device__ __forceinline__ dw_f2 dwf_dx_stored(const PackV<T, V>& o, int h) {
  return dw_f2{o.get(2 * h), o.get(2 * h + 1)};
}

// Thread and block position in the tile plan: thread (p, cvb) = column p of the tile (one halo
// column each side), channel vector cvb of the block's group; block = (column tile ct, channel
// group cg, strip, image n) after the XCD remap.
template <int V>
struct DwfPos {
  int tid, CVb, P, p, cvb, strip, n, cg, ct, c, li, ri;
  __device__ __forceinline__ void init(const DwTile& tl) {
    constexpr int TB = 1024 / V;
    tid = threadIdx.x;
    CVb = tl.CVb * (4 / V), P = tl.P;
    p = tid / CVb, cvb = tid - (tid / CVb) * CVb;
    int bx;
    xcd_block(bx, strip, n);
    cg = bx % tl.cgroups, ct = bx / tl.cgroups;
    c = (cg * CVb + cvb) * V;
    li = tid >= CVb ? tid - CVb : tid, ri = tid + CVb < TB ? tid + CVb : tid;   // LDS neighbours
  }
  __device__ __forceinline__ long part(const DwTile& tl) const { return ((long)n * tl.strips + strip) * tl.coltiles + ct; }
};

// Stride-2 thread geometry and prefetch ring.  Thread (p, cvb) owns dy column b and the dx / x
// column pair (ci0, ci0 + 1), ci0 = 2b - pl; step q handles dy row a = a0 - 1 + q and the x / dx
// rows 2a - pt, 2a + 1 - pt.  The tiled map is (A, B): every a / b with a dx row / column (dy rows
// >= Ho read as zero).  Every load is issued (rows / columns clamped into the map, uses masked by
// okd / okx) and every dx store too (offset ROD_OOB or the empty resource where nothing is to be
// written), so no memory operation sits under a branch and the ring's wait counts stay exact.
// YE: the kernel loads ye (the recompute kernel forms it instead and takes only the masks).
template <typename T, int V, int D, bool YE = true>
struct DwfS2 {
  typedef PackV<T, V> PK;
  int H, pt, A, B, a0, a1, dlo, dhi;
  bool comp, cokd, cok0, cok1;
  rsrc_t rye, rdx, rnull, rdz, ryd;
  unsigned vod, vox0, vox1, vst0, vst1, rsx, rsd;
  // ring slot k: dy (dz, yd) of row a, x (ye) at rows 2a-pt, 2a+1-pt x columns ci0, ci0+1
  PK rz[D], ry[D], rx[YE ? D : 1][4];
  bool okd[D], okx[D][4];

  __device__ __forceinline__ void init(const DwfPos<V>& at, const T* ye, const T* dz, const T* yd, T* dx,
                                       const DwTile& tl, int H_, int W, int C, int pt_, int pl, int Ho, int Wo) {
    H = H_, pt = pt_;
    const int b = at.ct * tl.TWo + at.p - 1;
    const int ci0 = 2 * b - pl;
    A = ((H - 1 + pt) >> 1) + 1, B = ((W - 1 + pl) >> 1) + 1;
    comp = at.p >= 1 && at.p <= at.P - 2 && b < B;
    cokd = at.p < at.P && b >= 0 && b < Wo;
    cok0 = at.p < at.P && ci0 >= 0 && ci0 < W;
    cok1 = at.p < at.P && ci0 + 1 >= 0 && ci0 + 1 < W;
    a0 = at.strip * tl.RB;
    a1 = a0 + tl.RB < A ? a0 + tl.RB : A;
    const unsigned es = sizeof(T);
    const int n = at.n, c = at.c;
    if constexpr (YE) rye = rod_rsrc(ye + (long)n * H * W * C, (unsigned)((long)H * W * C * es));
    rdx = rod_rsrc(dx + (long)n * H * W * C, (unsigned)((long)H * W * C * es));
    rnull = rod_rsrc(dx + (long)n * H * W * C, 0u);
    rdz = rod_rsrc(dz + (long)n * Ho * Wo * C, (unsigned)((long)Ho * Wo * C * es));
    ryd = rod_rsrc(yd + (long)n * Ho * Wo * C, (unsigned)((long)Ho * Wo * C * es));
    const int bc = b < 0 ? 0 : (b >= Wo ? Wo - 1 : b);
    const int x0c = ci0 < 0 ? 0 : (ci0 >= W ? W - 1 : ci0), x1c = ci0 + 1 < 0 ? 0 : (ci0 + 1 >= W ? W - 1 : ci0 + 1);
    vod = (unsigned)(((long)bc * C + c) * es);
    vox0 = (unsigned)(((long)x0c * C + c) * es), vox1 = (unsigned)(((long)x1c * C + c) * es);
    vst0 = comp && cok0 ? vox0 : ROD_OOB, vst1 = comp && cok1 ? vox1 : ROD_OOB;
    rsx = (unsigned)(W * C * es), rsd = (unsigned)(Wo * C * es);
    dlo = a0 - 1 > 0 ? a0 - 1 : 0;
    dhi = a1 - 1 < Ho - 1 ? a1 - 1 : Ho - 1;
  }
  __device__ __forceinline__ int steps() const { return a1 - a0 + 2; }
  // load step q into ring slot k
  __device__ __forceinline__ void issue(int k, int q) {
    const int a = a0 - 1 + q;
    okd[k] = cokd && a >= dlo && a <= dhi;
    const int ac = a < dlo ? dlo : (a > dhi ? dhi : a);
    rz[k].bload(rdz, vod, (unsigned)ac * rsd);
    ry[k].bload(ryd, vod, (unsigned)ac * rsd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hh = 2 * a - pt + (i >> 1);
      const bool rowok = a >= a0 && (i < 2 ? a <= a1 : a < a1) && hh >= 0 && hh < H;
      okx[k][i] = rowok && ((i & 1) ? cok1 : cok0);
      if constexpr (YE) {
        const int hc = hh < 0 ? 0 : (hh >= H ? H - 1 : hh);
        rx[k][i].bload(rye, (i & 1) ? vox1 : vox0, (unsigned)hc * rsx);
      }
    }
  }
  // the prologue issues the slots in order (slot 0 first), so that the loop header's wait for
  // slot 0 is the same count on entry as around the back-edge
  __device__ __forceinline__ void prime() {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      issue(k, k);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // dx position i (row hh = 2a-pt + (i >> 1), column ci0 + (i & 1)): dropped off the strip / map
  __device__ __forceinline__ void store(const PK& pk, int i, bool hok, int hh) const {
    pk.bstore(hok ? rdx : rnull, (i & 1) ? vst1 : vst0, (unsigned)(hok ? hh : 0) * rsx);
  }
};

// Epilogue of the packed stride-2 kernels: the nine filter accumulators and (RED) the BN_e sums
// staged into `red`, one barrier, dw_colsum_emit.  (fused2 has its own grouped form.)
template <int V, bool RED>
__device__ __forceinline__ void dwf_epilogue(float* red, const dw_f2 (&fa)[9][V / 2], const dw_f2 (&sg)[V / 2],
                                             const dw_f2 (&sgx)[V / 2], bool comp, const DwfPos<V>& at, float* slab,
                                             float* gparts, long part, int C) {
  constexpr int VP = V / 2, TB = 1024 / V;
  auto stage = [&](const dw_f2 (&a)[VP], int qk) {
#pragma unroll
    for (int h = 0; h < VP; ++h) {
      red[(qk * TB + at.tid) * V + 2 * h] = comp ? a[h].x : 0.f;
      red[(qk * TB + at.tid) * V + 2 * h + 1] = comp ? a[h].y : 0.f;
    }
  };
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 9; ++k) stage(fa[k], k);
  if constexpr (RED) {
    stage(sg, 9);
    stage(sgx, 10);
  }
  __syncthreads();
  dw_colsum_emit<V>(red, 0, RED ? 11 : 9, TB, at.CVb * V, at.CVb, at.P, slab, gparts, part, C, at.cg);
}

// host: what the fused entries share around their launch
struct DwFusedPlan {
  DwTile t;
  dim3 grid;
  BnPro pv;
  DwBwdBn bd;
  float* slab;
};
// the tile plan over the (A, B) map in 4-channel units, its grid, both BatchNorms, the filter slab
inline DwFusedPlan dw_fused_plan(int N, int A, int B, int C, const float* pro_mean, const float* pro_rstd,
                                 const float* pro_gamma, const float* pro_beta, int pro_act, const float* bn_mean,
                                 const float* bn_rstd, const float* bn_gamma, const float* bn_beta, int bn_act,
                                 const float* coef, void* workspace) {
  DwFusedPlan f;
  f.t = dw_tile(N, A, B, C, 1, 4);
  f.grid = dim3(f.t.coltiles * f.t.cgroups, f.t.strips, N);
  f.pv = BnPro{pro_mean, pro_rstd, pro_gamma, pro_beta, pro_act};
  f.bd = DwBwdBn{bn_mean, bn_rstd, bn_gamma, bn_beta, coef, bn_act};
  f.slab = (float*)workspace;
  return f;
}
// after the launch: its status, then the fixed-order sum of the per-part filter slabs into dw
inline int dw_fused_finish(const char* what, const float* slab, float* dw, int N, const DwTile& t, int C,
                           hipStream_t s) {
  const int rc = check_launch(what);
  if (rc) return rc;
  slab_sum(slab, dw, (int)((long)N * t.strips * t.coltiles), 9L * C, s);
  return check_launch(what);
}

}  // namespace rod
