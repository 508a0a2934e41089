// bnstat_common.h — the one copy of the BatchNorm partial-statistics arithmetic shared by the
// seven kernels that write a parts slab for rod_bn_finalize: bn_stats_kernel (batchnorm.hip), the
// STATS epilogues of conv_fwd_kernel, pw_stream_kernel and stem_fwd_mfma_kernel (gemm.hip), the
// direct depthwise forward and dw_lx_body (depthwise.hip) and the recompute forward (dwrc.hip).
//
// The slab contract: [nparts][3][C] of (count, mean, M2) per part and channel, part-major so that
// a producer block writes its 3*C values contiguously.  The statistics are those of the value AS
// STORED (rounded to the output type), a part with count 0 is ignored by the merge and carries
// mean = M2 = 0, and the counts of a channel sum to the number of rows.
//
// Every producer accumulates pivot-shifted sums s1 = sum(x - piv), s2 = sum((x - piv)^2) in fp32
// (StatAcc), so that s2 - s1^2/n does not cancel; they differ in where the pivot comes from, how
// the sums become (n, mean, M2) — three finishes, each a fixed operation sequence — and how the
// partials of a block are combined — two Chan steps.  The forms are deliberately distinct
// (DESIGN.md §5): a rounding-level change to the parts moves the full-size training tests, so a
// change is made here once and re-measured.  Everything is __forceinline__ and works on the
// caller's registers (profiles/bnstat_share_resources.md).  Three sites write these operations out
// instead, in the same order, because the calls cost registers or time there: the two
// depthwise forwards of depthwise.hip (accumulate, stat_finish_inv and their merges; dw_lx_body's
// is stat_block_merge_runs line for line) and pw_stream_kernel's pivot.  Change them together.
#pragma once
#include "rod_common.h"

namespace rod {

__device__ __forceinline__ void store_stat_part(float* slab, int C, long part, int c, float n, float mean, float m2) {
  float* p = slab + part * 3 * C + c;
  p[0] = n;
  p[C] = mean;
  p[2 * C] = m2;
}

// fp32 Chan merge of (n, mean, M2) accumulators
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float meanb, float m2b) {
  if (nb == 0.f) return;
  if (n == 0.f) {
    n = nb;
    mean = meanb;
    m2 = m2b;
    return;
  }
  const float nt = n + nb;
  const float d = meanb - mean;
  mean = fmaf(d, nb / nt, mean);
  m2 = m2 + m2b + d * d * (n * nb / nt);
  n = nt;
}

// conv_fwd_kernel's merge of its wave strips, in strip order: the mean moves by a rounded product
// and a rounded sum (no fmaf: one bit away from chan_merge), empty strips are skipped and the
// first strip is never empty unless all are.
__device__ __forceinline__ void chan_merge_strip(float& n, float& mean, float& m2, float nb, float meanb, float m2b) {
  if (nb <= 0.f) return;
  const float nn = n + nb;
  const float d = meanb - mean;
  mean = mean + d * (nb / nn);
  m2 = m2 + m2b + d * d * (n * nb / nn);
  n = nn;
}

// Pivot-shifted sums of V channels (or V columns) of one thread.
template <int V>
struct StatAcc {
  float piv[V], s1[V], s2[V];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int v = 0; v < V; ++v) piv[v] = s1[v] = s2[v] = 0.f;
  }
  // pivot set by the caller
  __device__ __forceinline__ void add(int v, float x) {
    const float d = x - piv[v];
    s1[v] += d;
    s2[v] = fmaf(d, d, s2[v]);
  }
  // pivot = the thread's first value
  __device__ __forceinline__ void add(int v, float x, bool first) {
    if (first) piv[v] = x;
    add(v, x);
  }
};

// ---- finishes: shifted sums -> (mean, M2) -------------------------------------------------------
// depthwise form: nr values of one thread, scaled by the reciprocal (nr = 0: an idle thread, 0 0)
__device__ __forceinline__ void stat_finish_inv(int nr, float piv, float s1, float s2, float& mean, float& m2) {
  const float inv = nr > 0 ? 1.f / (float)nr : 0.f;
  const float dm = s1 * inv;
  mean = piv + dm;
  m2 = nr > 0 ? fmaxf(s2 - s1 * dm, 0.f) : 0.f;
}
// MFMA form: a column of a ROWS-row tile; a full tile scales exactly, a partial one divides
template <int ROWS>
__device__ __forceinline__ void stat_finish_tile(bool full, float n, float piv, float s1, float s2, float& mean,
                                                 float& m2) {
  static_assert((ROWS & (ROWS - 1)) == 0, "the tile's rows must be a power of two");
  const float dm = full ? s1 * (1.0f / ROWS) : (n > 0.f ? s1 / n : 0.f);
  mean = piv + dm;
  m2 = fmaxf(s2 - s1 * dm, 0.f);
}
// f64 form: the fp32 sums (or their f64 totals) finished in double, rounded once
__device__ __forceinline__ void stat_finish_f64(double nb, double piv, double s1, double s2, float& mean, float& m2) {
  const double q = s2 - s1 * s1 / nb;
  mean = (float)(piv + s1 / nb);
  m2 = (float)(q > 0.0 ? q : 0.0);
}

// ---- MFMA columns: a column of a 16x16 tile lives in lanes l, l^16, l^32, l^48 (rows 4(l>>4)+r) ---
// pivot of a column: the mean of the first (up to) 8 of the `left` valid rows of the 16-row tile
// whose four values per lane are v[0..3]; the same value in all four lanes of the column
template <typename R>
__device__ __forceinline__ float mfma_col_pivot(const R& v, int lane, int left) {
  const int lg = lane >> 4;
  float p = 0.f;
  if (lg < 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (lg * 4 + r < left) p += v[r];
  }
  p += __shfl_xor(p, 16, 64);
  p = __shfl(p, lane & 15, 64);
  // 8 rows: an exact scaling
  return left >= 8 ? p * 0.125f : (left > 0 ? p / (float)left : 0.f);
}
// the four lane groups' sums of a column, in every lane of it
__device__ __forceinline__ void mfma_col_reduce(float& s1, float& s2) {
  s1 += __shfl_xor(s1, 16, 64);
  s2 += __shfl_xor(s2, 16, 64);
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
}

// ---- per-thread form: the threads of a channel combined through LDS ------------------------------
// LDS floats of the block merge below (256 threads)
constexpr int stat_stage_floats(int V) { return 256 * (2 * V + 1); }
constexpr int stat_runs_floats(int V) { return stat_stage_floats(V) + 3 * 512; }

// every thread's (n, mean, M2) of its nr values -> lds as mean[256][V], M2[256][V], n[256]
template <int V>
__device__ __forceinline__ void stat_stage(float* lds, int tid, int nr, const StatAcc<V>& a) {
  float* sm = lds;
  float* sq = sm + 256 * V;
#pragma unroll
  for (int v = 0; v < V; ++v) stat_finish_inv(nr, a.piv[v], a.s1[v], a.s2[v], sm[tid * V + v], sq[tid * V + v]);
  sq[256 * V + tid] = (float)nr;
  __syncthreads();
}

// Column-tile kernels (the recompute forward; dw_lx_body holds the same text inline): thread p * CVb + cvb holds column p of
// channel vector cvb.  Per channel, Chan merge over the P columns in two levels (runs of 8 columns,
// then the runs, each in column order: serial depth ~8 + P/8 rather than P) -> channels
// c0 .. c0 + CVb*V - 1 of `part`.  lds (stat_runs_floats(V)) may alias the kernel's row buffers:
// the leading barrier retires them.
template <int V>
__device__ __forceinline__ void stat_block_merge_runs(float* lds, int tid, int nr, const StatAcc<V>& a, int CVb,
                                                      int P, float* parts, int C, long part, int c0) {
  __syncthreads();
  stat_stage<V>(lds, tid, nr, a);
  const float *sm = lds, *sq = sm + 256 * V, *sn = sq + 256 * V;
  float* l1n = lds + stat_stage_floats(V);
  float* l1m = l1n + 512;
  float* l1q = l1m + 512;
  const int Cc = CVb * V;
  const int nrun = (P + 7) / 8;
  for (int e = tid; e < Cc * nrun; e += 256) {
    const int ch = e % Cc, run = e / Cc;
    const int cve = ch / V, v = ch - cve * V;
    float pn = 0.f, pm = 0.f, pq = 0.f;
    for (int pp = run * 8; pp < run * 8 + 8 && pp < P; ++pp) {
      const int t2 = pp * CVb + cve;
      chan_merge(pn, pm, pq, sn[t2], sm[t2 * V + v], sq[t2 * V + v]);
    }
    l1n[e] = pn;
    l1m[e] = pm;
    l1q[e] = pq;
  }
  __syncthreads();
  for (int ch = tid; ch < Cc; ch += 256) {
    float pn = 0.f, pm = 0.f, pq = 0.f;
    for (int run = 0; run < nrun; ++run) chan_merge(pn, pm, pq, l1n[run * Cc + ch], l1m[run * Cc + ch], l1q[run * Cc + ch]);
    store_stat_part(parts, C, part, c0 + ch, pn, pm, pq);
  }
}

}  // namespace rod
