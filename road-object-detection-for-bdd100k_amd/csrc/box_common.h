// box_common.h — the arithmetic the detection-side kernels share (targets.hip, detect.hip,
// loss.hip, nms.hip, evalmatch.hip): the level table, box decode / conversion, the IoU forms and
// the row softmax.  Every file that includes this is compiled with -ffp-contract=off, and every
// helper is ONE fixed sequence of rounded fp32 operations: two kernels that call the same helper
// agree bit for bit, which is what the oracle-pinned tests rely on.  The IoU forms differ from one
// another in operation order and guards ON PURPOSE (each restates another reference function):
// they stay separate functions.
#pragma once
#include "rod_common.h"

namespace rod {

// ---- levels ------------------------------------------------------------------------------
// Anchors of one image are the levels' anchors concatenated: level l owns [off[l], off[l+1]).
constexpr int MAXL = 8;
struct Levels {
  int off[MAXL + 1];
  float thr[MAXL];  // per-level positive threshold (0 where the entry takes none)
  int L;
};

// lvl_off [L+1] (and thr [L], or NULL) are host arrays
static inline int fill_levels(Levels& lv, const int* lvl_off, const float* thr, int L, int A) {
  ROD_CHECK_ARG(lvl_off, "levels: lvl_off is a host array and must be given");
  ROD_CHECK_ARG(L >= 1 && L <= MAXL, "levels: L=%d out of range [1,%d]", L, MAXL);
  lv.L = L;
  for (int i = 0; i <= MAXL; ++i) lv.off[i] = i <= L ? lvl_off[i] : A;
  for (int i = 0; i < MAXL; ++i) lv.thr[i] = (thr && i < L) ? thr[i] : 0.f;
  ROD_CHECK_ARG(lv.off[0] == 0 && lv.off[L] == A, "levels: offsets must span [0, A]");
  for (int i = 0; i < L; ++i) ROD_CHECK_ARG(lv.off[i] <= lv.off[i + 1], "levels: offsets must be monotone");
  return 0;
}

// the level that owns anchor a (the last one whose offset is <= a: empty levels own nothing)
__device__ __forceinline__ int level_of(const Levels& lv, int a) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < MAXL; ++k)
    if (k < lv.L && a >= lv.off[k]) l = k;
  return l;
}

// ---- boxes -------------------------------------------------------------------------------
// A box is four floats, centre form (cy, cx, h, w) or corner form (ymin, xmin, ymax, xmax); the
// helpers index their arguments, so an f32x4, a float[4] and a pointer into LDS all serve.

// decode_locations_one_layer (net_tools.py:182-234): bboxes_cy = off * anchor_h + anchor_cy,
// bboxes_h = exp(off) * anchor_h.  az is the centre-form anchor.
template <typename A, typename O>
__device__ __forceinline__ f32x4 decode_center(const A& az, const O& o) {
  return f32x4{o[0] * az[2] + az[0], o[1] * az[3] + az[1], exp_cr(o[2]) * az[2], exp_cr(o[3]) * az[3]};
}
// its backward: d wrt the offsets from d wrt the decoded centre box z = decode_center(az, o)
template <typename A>
__device__ __forceinline__ f32x4 decode_center_bwd(const f32x4& d, const A& az, const f32x4& z) {
  return f32x4{d[0] * az[2], d[1] * az[3], d[2] * z[2], d[3] * z[3]};
}
// centerBboxes_2_cornerBboxes (common_tools.py:30-33)
template <typename Z>
__device__ __forceinline__ f32x4 center_to_corner(const Z& z) {
  return f32x4{z[0] - z[2] / 2.f, z[1] - z[3] / 2.f, z[0] + z[2] / 2.f, z[1] + z[3] / 2.f};
}
// cornerBboxes_2_centerBboxes (common_tools.py:38-56)
template <typename C>
__device__ __forceinline__ f32x4 corner_to_center(const C& c) {
  return f32x4{(c[0] + c[2]) / 2.f, (c[1] + c[3]) / 2.f, c[2] - c[0], c[3] - c[1]};
}

// ---- IoU 1: the reference's jaccard (net_tools.py:254-266) -----------------------------------
// Anchor matching, the ODM targets and the box loss.  No guard: 0/0 is NaN as in the reference.
// vol_anchors = (xmax - xmin) * (ymax - ymin) (254); the gt's volume the other way round (265).
template <typename C>
__device__ __forceinline__ float vol_anchor(const C& c) { return (c[3] - c[1]) * (c[2] - c[0]); }
template <typename C>
__device__ __forceinline__ float vol_gt(const C& c) { return (c[2] - c[0]) * (c[3] - c[1]); }
struct Jaccard {
  float ihr, iwr;  // height / width of the intersection before max(., 0)
  float ih, iw;    // after
  float inter, uni, iou;
};
// a: the anchor (or predicted) box, always the first operand of min / max; g: the gt box
template <typename CA, typename CG>
__device__ __forceinline__ Jaccard jaccard_ref_parts(const CA& a, float vol_a, const CG& g, float vol_g) {
  Jaccard j;
  j.ihr = fminf(a[2], g[2]) - fmaxf(a[0], g[0]);
  j.iwr = fminf(a[3], g[3]) - fmaxf(a[1], g[1]);
  j.ih = fmaxf(j.ihr, 0.f);
  j.iw = fmaxf(j.iwr, 0.f);
  j.inter = j.ih * j.iw;
  j.uni = vol_a - j.inter + vol_g;  // (vol_anchors - inter_vol) + vol_gt
  j.iou = j.inter / j.uni;
  return j;
}
template <typename CA, typename CG>
__device__ __forceinline__ float jaccard_ref(const CA& a, float vol_a, const CG& g, float vol_g) {
  return jaccard_ref_parts(a, vol_a, g, vol_g).iou;
}
// Backward of jaccard_ref wrt the centre form (cy, cx, h, w) of a = center_to_corner(z), given the
// caller's d / d inter (d_I) and d / d vol_a (d_area).  TF's gradient rules: maximum -> its first
// argument when x >= y, minimum -> when x <= y (a is the first argument), max(., 0) passes at >= 0.
// ENC adds the terms of an enclosing box max(a, g) - min(a, g) of upstream d_eh / d_ew (the GIoU
// family); without it nothing is added, not even a zero (x + 0 would turn a -0 into +0).
template <bool ENC, typename CA, typename CG>
__device__ __forceinline__ f32x4 jaccard_ref_bwd(const CA& a, const CG& g, const Jaccard& j, float d_I,
                                                 float d_area, float d_eh = 0.f, float d_ew = 0.f) {
  const float d_ih = j.ihr >= 0.f ? d_I * j.iw : 0.f;
  const float d_iw = j.iwr >= 0.f ? d_I * j.ih : 0.f;
  float d_y1 = a[2] <= g[2] ? d_ih : 0.f, d_y0 = a[0] >= g[0] ? -d_ih : 0.f;
  float d_x1 = a[3] <= g[3] ? d_iw : 0.f, d_x0 = a[1] >= g[1] ? -d_iw : 0.f;
  if constexpr (ENC) {
    d_y1 += a[2] >= g[2] ? d_eh : 0.f;
    d_y0 += a[0] <= g[0] ? -d_eh : 0.f;
    d_x1 += a[3] >= g[3] ? d_ew : 0.f;
    d_x0 += a[1] <= g[1] ? -d_ew : 0.f;
  }
  const float ah = a[2] - a[0], aw = a[3] - a[1];
  d_x1 += d_area * ah;
  d_x0 -= d_area * ah;
  d_y1 += d_area * aw;
  d_y0 -= d_area * aw;
  // corner -> centre: y0 = cy - h/2, y1 = cy + h/2
  return f32x4{d_y0 + d_y1, d_x0 + d_x1, (d_y1 - d_y0) / 2.f, (d_x1 - d_x0) / 2.f};
}

// ---- IoU 2: tf.image.non_max_suppression (bboxes.py:182) --------------------------------------
// Differs from jaccard_ref: corners are min/max-normalised first, 0 when either area is <= 0,
// union = area_i + area_j - inter.
__device__ __forceinline__ float tf_iou(const float* bi, const float* bj) {
  const float ymin_i = fminf(bi[0], bi[2]), xmin_i = fminf(bi[1], bi[3]);
  const float ymax_i = fmaxf(bi[0], bi[2]), xmax_i = fmaxf(bi[1], bi[3]);
  const float ymin_j = fminf(bj[0], bj[2]), xmin_j = fminf(bj[1], bj[3]);
  const float ymax_j = fmaxf(bj[0], bj[2]), xmax_j = fmaxf(bj[1], bj[3]);
  const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
  const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
  if (area_i <= 0.f || area_j <= 0.f) return 0.f;
  const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
  const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
  const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
  return inter / (area_i + area_j - inter);
}

// ---- IoU 3: bboxes_jaccard of the evaluation matcher (tf_extended/bboxes.py:246-334) ---------
// Differs from both: union = (-inter + area_gt) + area_det, 0 unless the union is > 0, and a pair
// with no intersection or another label is exactly 0 without the division (0 / union, iou * 0).
// q: the gt box, the first operand of min / max; r: the detection, area_det its area.
__device__ __forceinline__ float jaccard_eval(const f32x4& q, const f32x4& r, float area_det, bool same_label) {
  const float h = fmaxf(fminf(q[2], r[2]) - fmaxf(q[0], r[0]), 0.f);
  const float w = fmaxf(fminf(q[3], r[3]) - fmaxf(q[1], r[1]), 0.f);
  const float inter = h * w;
  if (!(inter > 0.f && same_label)) return 0.f;
  const float area_g = (q[2] - q[0]) * (q[3] - q[1]);
  const float uni = (-inter + area_g) + area_det;
  return uni > 0.f ? inter / uni : 0.f;
}
// (A fourth form, the crop-overlap score of the augmentation, lives with its only user in
// augment.hip.)

// ---- row softmax -------------------------------------------------------------------------
// e[k] = exp(x[k] - max x), s = sum e in index order: p[k] = e[k] / s is slim.softmax
// (predict.py:128) and the loss's predictions (net_tools.py:571), which must agree.
template <typename T>
__device__ __forceinline__ void row_softmax(const T* __restrict__ x, int K, float* e, float& m, float& s) {
  m = to_f32(x[0]);
  for (int k = 1; k < K; ++k) m = fmaxf(m, to_f32(x[k]));
  s = 0.f;
  for (int k = 0; k < K; ++k) {
    e[k] = exp_cr(to_f32(x[k]) - m);
    s += e[k];
  }
}

}  // namespace rod
