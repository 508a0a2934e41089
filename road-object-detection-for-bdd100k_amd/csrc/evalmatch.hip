// evalmatch.hip — rod_match_detections (ABI 28): TP/FP matching of the score-ordered detections
// of every (image, class) against the image's ground truth (reference
// utils/tf_extended/bboxes.py:246-334, bboxes_matching) at T IoU thresholds in one launch;
// rod_match_detections_area (ABI 31): the same matching reported for R object-area ranges.
//
// The reference walks the detections in score order and keeps a "ground truth already matched"
// bit per box.  The ground truth a detection competes for is the first argmax of its IoU over
// the same-label boxes: no threshold and no matching state enters it.  The matched bit of box
// idx, seen by detection i at threshold t, is "some i' < i has idx_i' == idx, is not difficult
// and matches at t" — so detection i is the TP of box idx at t exactly when it is the FIRST
// detection in score order with (idx_i == idx && nd_i && match_it).  That is one integer min
// per (box, threshold): no sequential loop.
//
// One workgroup of 256 threads per (image b, class slot c):
//   stage    the image's g = gt_count[b] boxes, labels and difficult flags in LDS;
//   phase 1  thread tid takes detections i = tid, tid + 256, ... (N <= 1024: at most 4, kept in
//            registers) and scans the g boxes — every lane reads the same LDS address, a
//            broadcast — keeping (best_jac, idx), first maximum;
//   phase 2  first[g][T] (LDS, INT_MAX): atomicMin(first[idx][t], i) for every t with
//            nd && match; barrier; tp_it = first[idx][t] == i.  Integer min is
//            order-independent: the output is deterministic.
// IoU: jaccard_eval (box_common.h) = oracle.post.bboxes_jaccard_one, one fp32 operation at a time
// (the build is -ffp-contract=off), the division of nms.hip (IEEE `/`).
//
// Area ranges (the AREA instantiation).  Phases 1 and 2 do not depend on the range: a detection
// competes for its argmax ground truth whether that box is in the range or not.  A range only
// decides what the final store reports: ground truth outside it is ignored (a detection matched
// to it is neither TP nor FP), and an unmatched detection is an FP only if its own area is inside.
// The stage phase leaves one byte per ground-truth row in LDS, bit r = "area in range r"; each
// thread keeps the same byte for its detections; only the final store loops over r.
#include <limits.h>

#include "box_common.h"

namespace rod {

constexpr int EM_T = 256;        // threads per workgroup
constexpr int EM_MAXN = 1024;    // detections per (image, class)
constexpr int EM_PER = EM_MAXN / EM_T;
constexpr int EM_MAXG = 512;     // ground-truth rows per image
constexpr int EM_MAXT = 16;      // thresholds (bits of the masks)
constexpr int EM_MAXR = 8;       // area ranges (bits of the per-row range byte)

static size_t em_pad16(int G) { return ((size_t)G + 15) & ~(size_t)15; }
// dynamic LDS: boxes [G] float4 | labels [G] int | first [G*T] int | difficult [G] bytes
// (padded to 16) | AREA only: in-range bits [G] bytes
static size_t em_lds_bytes(int G, int T, bool area = false) {
  return (size_t)G * (16 + 4 + 4 * T) + em_pad16(G) + 16 + (area ? em_pad16(G) : 0);
}

// bit r = in_r(a) = !(a < lo_r) && !(a >= hi_r): [lo, hi), a NaN area is inside every range
__device__ __forceinline__ int area_range_bits(float a, const float* __restrict__ ranges, int R) {
  int bits = 0;
  for (int r = 0; r < R; ++r)
    if (!(a < ranges[2 * r]) && !(a >= ranges[2 * r + 1])) bits |= 1 << r;
  return bits;
}

// AREA = false: rod_match_detections, outputs [B,C,N] / [B,C]; area_ranges and R are not read.
// AREA = true: rod_match_detections_area, outputs [R,B,C,N] / [R,B,C] (B = gridDim.y).
template <bool AREA>
__global__ void __launch_bounds__(EM_T) match_detections_kernel(
    const float* __restrict__ det_boxes, const int32_t* __restrict__ gt_labels, const float* __restrict__ gt_boxes,
    const uint8_t* __restrict__ gt_difficult, const int32_t* __restrict__ gt_count,
    const float* __restrict__ thresholds, const float* __restrict__ area_ranges, int R, int C, int N, int G, int T,
    int first_label, int32_t* __restrict__ tp_mask, int32_t* __restrict__ fp_mask, int32_t* __restrict__ n_gt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char em_lds[];
  __shared__ int cnt[AREA ? EM_MAXR : 1];
  f32x4* gbox = (f32x4*)em_lds;
  int* glab = (int*)(gbox + G);
  int* first = glab + G;
  unsigned char* gdiff = (unsigned char*)(first + (size_t)G * T);
  unsigned char* grange = gdiff + (((size_t)G + 15) & ~(size_t)15);  // AREA only

  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int label = first_label + c;
  const int g = min(max(gt_count[b], 0), G);  // rows >= g are padding: never read
  const long row = (long)b * C + c;
  const int all_bits = (int)((1u << T) - 1u);

  if (tid < (AREA ? R : 1)) cnt[tid] = 0;
  for (int j = tid; j < g; j += EM_T) {
    const f32x4 q = *(const f32x4*)(gt_boxes + ((long)b * G + j) * 4);
    gbox[j] = q;
    glab[j] = gt_labels[(long)b * G + j];
    gdiff[j] = gt_difficult ? (gt_difficult[(long)b * G + j] ? 1 : 0) : 0;
    if constexpr (AREA) grange[j] = (unsigned char)area_range_bits((q[2] - q[0]) * (q[3] - q[1]), area_ranges, R);
  }
  for (int q = tid; q < g * T; q += EM_T) first[q] = INT_MAX;
  __syncthreads();

  if constexpr (AREA) {
    for (int j = tid; j < g; j += EM_T) {
      if (glab[j] != label || gdiff[j]) continue;
      for (int r = 0; r < R; ++r)
        if (grange[j] >> r & 1) atomicAdd(&cnt[r], 1);
    }
  } else {
    int mine = 0;
    for (int j = tid; j < g; j += EM_T) mine += (glab[j] == label && !gdiff[j]) ? 1 : 0;
    if (mine) atomicAdd(&cnt[0], mine);
  }

  // phase 1: (best_jac, idx) of this thread's detections
  float bj[EM_PER];
  int bi[EM_PER];
  int drange[EM_PER];  // AREA only: the detection's own in-range bits
#pragma unroll
  for (int k = 0; k < EM_PER; ++k) {
    const int i = tid + k * EM_T;
    bj[k] = 0.f;
    bi[k] = 0;
    drange[k] = 0;
    if (i >= N || (!AREA && g == 0)) continue;
    const f32x4 r = *(const f32x4*)(det_boxes + (row * N + i) * 4);
    const float area_det = (r[2] - r[0]) * (r[3] - r[1]);
    if constexpr (AREA) {
      drange[k] = area_range_bits(area_det, area_ranges, R);
      if (g == 0) continue;
    }
    float best = -1.f;  // every jac is >= 0: box 0 always takes the first comparison
    int idx = 0;
    for (int j = 0; j < g; ++j) {
      const float jac = jaccard_eval(gbox[j], r, area_det, glab[j] == label);
      if (jac > best) {  // strict: the first maximum wins
        best = jac;
        idx = j;
      }
    }
    bj[k] = best;
    bi[k] = idx;
  }

  // phase 2: the first detection in score order that matches box idx at threshold t
  int mbits[EM_PER];
#pragma unroll
  for (int k = 0; k < EM_PER; ++k) {
    const int i = tid + k * EM_T;
    mbits[k] = 0;
    if (i >= N || g == 0 || gdiff[bi[k]]) continue;
    int m = 0;
    for (int t = 0; t < T; ++t)
      if (bj[k] > thresholds[t]) {
        m |= 1 << t;
        atomicMin(&first[bi[k] * T + t], i);
      }
    mbits[k] = m;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EM_PER; ++k) {
    const int i = tid + k * EM_T;
    if (i >= N) continue;
    int tp = 0, fp = all_bits;  // g == 0: FP in every bit
    if (g > 0) {
      const bool nd = !gdiff[bi[k]];
      for (int t = 0; t < T; ++t)
        if ((mbits[k] >> t & 1) && first[bi[k] * T + t] == i) tp |= 1 << t;
      fp = nd ? (all_bits & ~tp) : 0;
    }
    if constexpr (AREA) {
      // tp / fp above are the all-range answer; nd = false left both 0.  Matched bits (mbits)
      // count only if the ground truth is in range r, unmatched bits only if the detection is.
      const long plane = (long)gridDim.y * C * N;
      const int gin = g > 0 ? grange[bi[k]] : 0;
      const int unmatched = fp & ~mbits[k];
      for (int r = 0; r < R; ++r) {
        const bool g_in = gin >> r & 1, d_in = drange[k] >> r & 1;
        tp_mask[r * plane + row * N + i] = g_in ? tp : 0;
        fp_mask[r * plane + row * N + i] = (g_in ? (fp & mbits[k]) : 0) | (d_in ? unmatched : 0);
      }
    } else {
      tp_mask[row * N + i] = tp;
      fp_mask[row * N + i] = fp;
    }
  }
  if constexpr (AREA) {
    if (tid < R) n_gt[(long)tid * gridDim.y * C + row] = cnt[tid];
  } else {
    if (tid == 0) n_gt[row] = cnt[0];
  }
}

}  // namespace rod

using namespace rod;

extern "C" {

int rod_match_detections(const float* det_scores, const float* det_boxes, const int32_t* gt_labels,
                         const float* gt_boxes, const uint8_t* gt_difficult, const int32_t* gt_count,
                         const float* thresholds, int B, int C, int N, int G, int T, int first_label, int32_t* tp_mask,
                         int32_t* fp_mask, int32_t* n_gt, void* stream) {
  (void)det_scores;  // no decision reads the scores: the detections arrive in score order
  ROD_CHECK_ARG(B > 0 && C > 0, "rod_match_detections: bad shape");
  ROD_CHECK_ARG(T >= 1 && T <= EM_MAXT, "rod_match_detections: T must be in [1, %d], got %d", EM_MAXT, T);
  ROD_CHECK_ARG(N >= 1 && N <= EM_MAXN, "rod_match_detections: N must be in [1, %d], got %d", EM_MAXN, N);
  ROD_CHECK_ARG(G >= 0 && G <= EM_MAXG, "rod_match_detections: G must be in [0, %d], got %d", EM_MAXG, G);
  ROD_CHECK_ARG(B <= 65535, "rod_match_detections: B too large");
  ROD_CHECK_ARG(thresholds != nullptr, "rod_match_detections: thresholds is NULL");
  ROD_CHECK_ARG(det_boxes && gt_count && tp_mask && fp_mask && n_gt, "rod_match_detections: NULL argument");
  ROD_CHECK_ARG(G == 0 || (gt_labels && gt_boxes), "rod_match_detections: NULL ground truth with G > 0");
  launch_lds(match_detections_kernel<false>, dim3(C, B), dim3(EM_T), em_lds_bytes(G, T), ROD_STREAM(stream), det_boxes,
             gt_labels, gt_boxes, gt_difficult, gt_count, thresholds, (const float*)nullptr, 0, C, N, G, T, first_label,
             tp_mask, fp_mask, n_gt);
  return check_launch("rod_match_detections");
}

int rod_match_detections_area(const float* det_scores, const float* det_boxes, const int32_t* gt_labels,
                              const float* gt_boxes, const uint8_t* gt_difficult, const int32_t* gt_count,
                              const float* thresholds, const float* area_ranges, int B, int C, int N, int G, int T,
                              int R, int first_label, int32_t* tp_mask, int32_t* fp_mask, int32_t* n_gt,
                              void* stream) {
  (void)det_scores;
  ROD_CHECK_ARG(B > 0 && C > 0, "rod_match_detections_area: bad shape");
  ROD_CHECK_ARG(T >= 1 && T <= EM_MAXT, "rod_match_detections_area: T must be in [1, %d], got %d", EM_MAXT, T);
  ROD_CHECK_ARG(N >= 1 && N <= EM_MAXN, "rod_match_detections_area: N must be in [1, %d], got %d", EM_MAXN, N);
  ROD_CHECK_ARG(G >= 0 && G <= EM_MAXG, "rod_match_detections_area: G must be in [0, %d], got %d", EM_MAXG, G);
  ROD_CHECK_ARG(R >= 1 && R <= EM_MAXR, "rod_match_detections_area: R must be in [1, %d], got %d", EM_MAXR, R);
  ROD_CHECK_ARG(B <= 65535, "rod_match_detections_area: B too large");
  ROD_CHECK_ARG(thresholds != nullptr, "rod_match_detections_area: thresholds is NULL");
  ROD_CHECK_ARG(area_ranges != nullptr, "rod_match_detections_area: area_ranges is NULL");
  ROD_CHECK_ARG(det_boxes && gt_count && tp_mask && fp_mask && n_gt, "rod_match_detections_area: NULL argument");
  ROD_CHECK_ARG(G == 0 || (gt_labels && gt_boxes), "rod_match_detections_area: NULL ground truth with G > 0");
  launch_lds(match_detections_kernel<true>, dim3(C, B), dim3(EM_T), em_lds_bytes(G, T, true), ROD_STREAM(stream),
             det_boxes, gt_labels, gt_boxes, gt_difficult, gt_count, thresholds, area_ranges, R, C, N, G, T,
             first_label, tp_mask, fp_mask, n_gt);
  return check_launch("rod_match_detections_area");
}

}  // extern "C"
