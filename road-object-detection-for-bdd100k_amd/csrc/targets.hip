// targets.hip — anchor matching (JACCARD_BIGGER), the masked smooth-L1 loss and the opt-in
// IoU-family box loss.
//
// Bit-exactness: this file is compiled with -ffp-contract=off (Makefile), so every
// expression below rounds after each operation exactly like the reference's chain of
// separate TF float32 ops; transcendental functions are correctly rounded (exp_cr/log_cr)
// and the oracle uses the same definition.
#include <math.h>

#include "box_common.h"

namespace rod {

// One workgroup per (anchor block, image).  The image's centre-form GT boxes are staged
// in LDS together with their corner form and area.
// NN = false: JACCARD_BIGGER (net_tools.py:382-421): argmax IoU, positive if >= the level's
// threshold.  NN = true: NEAREST_NEIGHBOR (net_tools.py:354-380): argmin over the boxes of
// sum(encode(anchor, box)^2) (tf.argmin, first minimum), every anchor positive.
template <bool NN>
__global__ void __launch_bounds__(256) match_anchors_kernel(const float* __restrict__ anc_corner,
                                                            const float* __restrict__ anc_center, Levels li,
                                                            const float* __restrict__ gt, const int* __restrict__ gt_lbl,
                                                            const int* __restrict__ gt_n, float* __restrict__ out_off,
                                                            float* __restrict__ out_cbox, int* __restrict__ out_lbl,
                                                            int* __restrict__ out_pos, int A, int G) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* gc = sm;              // [G][4] corner after round trip
  float* gz = sm + 4 * G;      // [G][4] centre (cy, cx, h, w)
  float* gv = sm + 8 * G;      // [G] volume
  int* gl = (int*)(sm + 9 * G);  // [G] label
  __shared__ int poison[8];    // per-channel count of non-finite encodings (0..3 offsets, 4..7 centre)

  const int b = blockIdx.y;
  int n = gt_n[b];
  if (n > G) n = G;
  if (threadIdx.x < 8) poison[threadIdx.x] = 0;
  __syncthreads();
  for (int g = threadIdx.x; g < n; g += blockDim.x) {
    // center_bboxes[i] = (cy, cx, h, w) (train.py:109 already converted them)
    const float* p = gt + ((long)b * G + g) * 4;
    const float cy = p[0], cx = p[1], h = p[2], w = p[3];
    const f32x4 c = center_to_corner(p);  // the corner form jaccard takes (net_tools.py:323, 398)
    gc[g * 4 + 0] = c[0]; gc[g * 4 + 1] = c[1]; gc[g * 4 + 2] = c[2]; gc[g * 4 + 3] = c[3];
    gz[g * 4 + 0] = cy; gz[g * 4 + 1] = cx; gz[g * 4 + 2] = h; gz[g * 4 + 3] = w;
    gv[g] = vol_gt(c);
    gl[g] = gt_lbl[(long)b * G + g];
    // every box contributes mask*encode(box) to every anchor (net_tools.py:340-342): a
    // non-finite encoding turns 0*x into NaN for all anchors (kept for parity).
    if (!isfinite(cy)) atomicAdd(&poison[0], 1);
    if (!isfinite(cx)) atomicAdd(&poison[1], 1);
    if (!(h > 0.f) || isinf(h)) atomicAdd(&poison[2], 1);
    if (!(w > 0.f) || isinf(w)) atomicAdd(&poison[3], 1);
    if (!isfinite(cy)) atomicAdd(&poison[4], 1);
    if (!isfinite(cx)) atomicAdd(&poison[5], 1);
    if (!isfinite(h)) atomicAdd(&poison[6], 1);
    if (!isfinite(w)) atomicAdd(&poison[7], 1);
  }
  __syncthreads();

  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A) return;
  const int lvl = level_of(li, a);

  const f32x4 ac = *(const f32x4*)(anc_corner + (long)a * 4);
  const float vol_a = vol_anchor(ac);

  float best = 0.f;
  int idx = 0;
  if constexpr (NN) {
    const f32x4 az = *(const f32x4*)(anc_center + (long)a * 4);
    for (int g = 0; g < n; ++g) {
      const float o0 = (gz[g * 4 + 0] - az[0]) / az[2], o1 = (gz[g * 4 + 1] - az[1]) / az[3];
      const float o2 = log_cr(gz[g * 4 + 2] / az[2]), o3 = log_cr(gz[g * 4 + 3] / az[3]);
      // reduce_sum over the 4 offsets, in index order (parity unpinned vs Eigen's order)
      const float d = ((o0 * o0 + o1 * o1) + o2 * o2) + o3 * o3;
      if (g == 0 || d < best) {
        best = d;
        idx = g;
      }
    }
  } else {
    for (int g = 0; g < n; ++g) {
      const float iou = jaccard_ref(ac, vol_a, gc + g * 4, gv[g]);
      if (g == 0 || iou > best) {  // tf.argmax: first maximal index wins
        best = iou;
        idx = g;
      }
    }
  }
  // tf.greater_equal (net_tools.py:406); NEAREST_NEIGHBOR: pos_mask = ones (net_tools.py:375)
  const bool pos = n > 0 && (NN || best >= li.thr[lvl]);

  const long o = (long)b * A + a;
  float off[4] = {0.f, 0.f, 0.f, 0.f}, cb[4] = {0.f, 0.f, 0.f, 0.f};
  int lab = 0;
  if (pos) {
    const f32x4 az = *(const f32x4*)(anc_center + (long)a * 4);
    const float cy = gz[idx * 4 + 0], cx = gz[idx * 4 + 1], h = gz[idx * 4 + 2], w = gz[idx * 4 + 3];
    off[0] = (cy - az[0]) / az[2];          // encode_locations_one_layer (net_tools.py:174-177)
    off[1] = (cx - az[1]) / az[3];
    off[2] = log_cr(h / az[2]);
    off[3] = log_cr(w / az[3]);
    cb[0] = cy; cb[1] = cx; cb[2] = h; cb[3] = w;
    lab = gl[idx];
  }
  // NaN poisoning of the masked sum (see above): with P poisoned boxes on a channel, the
  // anchor's sum is NaN unless its own matched box is the single poisoned one.
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int P = poison[c];
    if (P > 0) {
      const bool mine = pos && !isfinite(off[c]);
      if (!(mine && P == 1)) off[c] = __builtin_nanf("");
    }
    const int Q = poison[4 + c];
    if (Q > 0) {
      const bool mine = pos && !isfinite(cb[c]);
      if (!(mine && Q == 1)) cb[c] = __builtin_nanf("");
    }
  }
  f32x4 vo = {off[0], off[1], off[2], off[3]};
  f32x4 vc = {cb[0], cb[1], cb[2], cb[3]};
  *(f32x4*)(out_off + o * 4) = vo;
  *(f32x4*)(out_cbox + o * 4) = vc;
  out_lbl[o] = lab;
  out_pos[o] = pos ? 1 : 0;
}

// ---------------------------------------------------------------- smooth L1
// grid: x over (image, anchor-in-level) pairs of one level, y = level.
template <typename T>
__global__ void __launch_bounds__(256) smoothl1_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                       const int* __restrict__ mask, Levels li, float inv_scale,
                                                       T* __restrict__ grad, float* __restrict__ grad_t,
                                                       float* __restrict__ slab, int B, int A, int nbx) {
  __shared__ float red[4];
  const int l = blockIdx.y;
  const int Al = li.off[l + 1] - li.off[l];
  const long total = (long)B * Al;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float s = 0.f;
  if (t < total) {
    const int b = (int)(t / Al);
    const int a = li.off[l] + (int)(t - (long)b * Al);
    const long o = (long)b * A + a;
    const float m = (float)mask[o];
    float gv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = to_f32(pred[o * 4 + c]);
      const float d = (target[o * 4 + c] - x) * m;       // (y - x) * mask
      const float ad = fabsf(d);
      const float mn = fminf(ad, 1.f);
      s += 0.5f * ((ad - 1.f) * mn + ad);                // smooth_l1 (net_tools.py:486-489)
      gv[c] = -m * fminf(fmaxf(d, -1.f), 1.f) * inv_scale;  // d/dx of the above / scale
    }
    if (grad) {
#pragma unroll
      for (int c = 0; c < 4; ++c) grad[o * 4 + c] = from_f32<T>(gv[c]);
    }
    if (grad_t) {  // d/d target = -d/d pred (the ODM target depends on refine_out, 471)
#pragma unroll
      for (int c = 0; c < 4; ++c) grad_t[o * 4 + c] = -gv[c];
    }
  }
  s = warp_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) slab[(long)l * nbx + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// weight: 1 for the smooth-L1 losses (1 * x is x bit for bit), the loss weight of rod_box_iou_loss
__global__ void level_sum_finalize_kernel(const float* __restrict__ slab, int nbx, int L, float weight, float scale,
                                          float* __restrict__ out) {
  // one 256-thread block: strided partial sums per level, fixed-order tree in LDS
  __shared__ double red[MAXL][256];
  for (int l = 0; l < L; ++l) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nbx; i += 256) s += (double)slab[(long)l * nbx + i];
    red[l][threadIdx.x] = s;
  }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int l = 0; l < L; ++l) red[l][threadIdx.x] += red[l][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  float total = 0.f;  // refine_loss = 0.; refine_loss += layer_loss (net_tools.py:505-515)
  for (int l = 0; l < L; ++l) {
    out[l] = weight * (float)red[l][0] / scale;  // reduce_sum(...) / bs
    total = total + out[l];
  }
  out[L] = total;
}

// ---------------------------------------------------------------- IoU-family box loss (ABI 27)
// The four components of one row as ONE vector: 16 bytes (fp32) or 8 bytes (bf16); VEC = false
// (a pointer off that alignment) loads and stores them one by one.
template <typename T> struct Row4;
template <> struct Row4<float> { typedef f32x4 V; };
template <> struct Row4<bf16_t> { typedef bf16x4 V; };
template <typename T, bool VEC>
__device__ __forceinline__ void load_row4(const T* __restrict__ p, float (&o)[4]) {
  if constexpr (VEC) {
    const typename Row4<T>::V v = *(const typename Row4<T>::V*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (float)v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = to_f32(p[k]);
  }
}
template <typename T, bool VEC>
__device__ __forceinline__ void store_row4(T* __restrict__ p, const float (&g)[4]) {
  if constexpr (VEC) {
    typename Row4<T>::V v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = from_f32<T>(g[k]);
    *(typename Row4<T>::V*)p = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = from_f32<T>(g[k]);
  }
}
__device__ __forceinline__ float atan_cr(float x) { return (float)atan((double)x); }

// IoU / GIoU / DIoU / CIoU loss of the box the ODM predicts, decode(anchor, refine_out + det_out),
// against the matched centre box, and its gradient wrt the summed offsets in the same pass (the
// formula is in include/rod.h, rod_box_iou_loss).  Grid as smoothl1_kernel: x over (image,
// anchor-in-level) pairs of one level, y = level.  A row off the mask loads det_pos alone.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) box_iou_loss_kernel(const float* __restrict__ anc_center,
                                                           const T* __restrict__ refine_out,
                                                           const T* __restrict__ det_out,
                                                           const float* __restrict__ cbox,
                                                           const int* __restrict__ det_pos, Levels li, int kind,
                                                           float gscale, T* __restrict__ grad,
                                                           float* __restrict__ slab, int B, int A, int nbx) {
  __shared__ float red[4];
  const int l = blockIdx.y;
  const int Al = li.off[l + 1] - li.off[l];
  const long total = (long)B * Al;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float rl = 0.f;
  if (t < total) {
    const int b = (int)(t / Al);
    const int a = li.off[l] + (int)(t - (long)b * Al);
    const long o = (long)b * A + a;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (det_pos[o] != 0) {
      float az[4], gz[4], s[4], sb[4];
      load_row4<float, VEC>(anc_center + (long)a * 4, az);
      load_row4<float, VEC>(cbox + o * 4, gz);
      load_row4<T, VEC>(refine_out + o * 4, s);
      load_row4<T, VEC>(det_out + o * 4, sb);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = s[k] + sb[k];  // refine_out + det_out, as rod_decode
      // the predicted box and its IoU, by the helpers rod_decode and rod_det_targets call
      const f32x4 z = decode_center(az, s);
      const f32x4 pc = center_to_corner(z), gc = center_to_corner(gz);
      const Jaccard j = jaccard_ref_parts(pc, vol_anchor(pc), gc, vol_gt(gc));
      const float I = j.inter, U = j.uni, iou = j.iou;
      rl = 1.f - iou;
      const float q = I / (U * U);
      float d_I = -(1.f / U + q), d_ap = q;  // d(1 - iou) / d(I, area of the prediction)
      float d_eh = 0.f, d_ew = 0.f, d_cy = 0.f, d_cx = 0.f, d_h = 0.f, d_w = 0.f;
      if (kind != 0) {
        // the enclosing box: height, width, area C, squared diagonal c2
        const float eh = fmaxf(pc[2], gc[2]) - fminf(pc[0], gc[0]), ew = fmaxf(pc[3], gc[3]) - fminf(pc[1], gc[1]);
        if (kind == 1) {
          const float C = eh * ew;
          rl = rl + (C - U) / C;
          const float invC = 1.f / C, dC = U / (C * C);
          d_I = d_I + invC;
          d_ap = d_ap - invC;
          d_eh = dC * ew;
          d_ew = dC * eh;
        } else {
          const float c2 = eh * eh + ew * ew;
          const float dy = z[0] - gz[0], dx = z[1] - gz[1];
          const float rho2 = dy * dy + dx * dx;
          rl = rl + rho2 / c2;
          const float d_c2 = -(rho2 / (c2 * c2)), ir = 1.f / c2;
          d_eh = d_c2 * (2.f * eh);
          d_ew = d_c2 * (2.f * ew);
          d_cy = ir * (2.f * dy);
          d_cx = ir * (2.f * dx);
          if (kind == 3) {
            const float k4 = 0.40528473456935109f;  // 4 / pi^2
            const float h = z[2], w = z[3];
            const float dat = atan_cr(gz[3] / gz[2]) - atan_cr(w / h);
            const float v = k4 * (dat * dat);
            const float alpha = v == 0.f ? 0.f : v / ((1.f - iou) + v);  // a constant in the gradient
            rl = rl + alpha * v;
            const float tv = alpha * ((2.f * k4) * dat), hw2 = h * h + w * w;
            d_w = -(tv * (h / hw2));
            d_h = tv * (w / hw2);
          }
        }
      }
      const f32x4 dj = jaccard_ref_bwd<true>(pc, gc, j, d_I, d_ap, d_eh, d_ew);
      const f32x4 dz = {d_cy + dj[0], d_cx + dj[1], d_h + dj[2], d_w + dj[3]};
      const f32x4 go = decode_center_bwd(dz, az, z);
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = go[k] * gscale;
    }
    if (grad) store_row4<T, VEC>(grad + o * 4, g);
  }
  rl = warp_sum(rl);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = rl;
  __syncthreads();
  if (threadIdx.x == 0) slab[(long)l * nbx + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------- box conversions
// common_tools.py:16-35 / 38-56 on [..., 4] fp32 tensors
__global__ void boxes_convert_kernel(const float* __restrict__ in, float* __restrict__ out, long n, int to_center) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f32x4 v = *(const f32x4*)(in + i * 4);
  *(f32x4*)(out + i * 4) = to_center ? corner_to_center(v) : center_to_corner(v);
}

// dst[r, c] = src[r, c] for a rows x cols block with independent row strides (bytes)
template <int WB>
__global__ void copy2d_kernel(const char* __restrict__ src, long sld, char* __restrict__ dst, long dld, long rows,
                              long chunks) {
  // flattened (row, chunk) grid-stride: efficient for many short rows (channel concat)
  const long total = rows * chunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / chunks, c = (i - r * chunks) * WB;
    if constexpr (WB == 16) *(f32x4*)(dst + r * dld + c) = *(const f32x4*)(src + r * sld + c);
    else if constexpr (WB == 4) *(float*)(dst + r * dld + c) = *(const float*)(src + r * sld + c);
    else dst[r * dld + c] = src[r * sld + c];
  }
}

// both matching entries: NN picks the kernel and makes thr optional
template <bool NN>
static int match_anchors(const char* who, const float* anc_corner, const float* anc_center, const int* lvl_off,
                         const float* thr, int L, const float* gt, const int* gt_lbl, const int* gt_n, float* out_off,
                         float* out_cbox, int* out_lbl, int* out_pos, int B, int A, int G, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0 && G > 0, "%s: bad shape B=%d A=%d G=%d", who, B, A, G);
  ROD_CHECK_ARG(G <= 4096, "%s: G=%d exceeds 4096", who, G);
  ROD_CHECK_ARG(NN || thr, "%s: thr is a host array and must be given", who);
  Levels li;
  if (int rc = fill_levels(li, lvl_off, thr, L, A)) return rc;
  size_t lds = (size_t)G * 10 * sizeof(float);
  hipLaunchKernelGGL(match_anchors_kernel<NN>, dim3(cdiv(A, 256), B), dim3(256), lds, ROD_STREAM(stream), anc_corner,
                     anc_center, li, gt, gt_lbl, gt_n, out_off, out_cbox, out_lbl, out_pos, A, G);
  return check_launch(who);
}

}  // namespace rod

using namespace rod;

extern "C" {

int rod_match_anchors(const float* anc_corner, const float* anc_center, const int* lvl_off, const float* thr, int L,
                      const float* gt, const int* gt_lbl, const int* gt_n, float* out_off, float* out_cbox,
                      int* out_lbl, int* out_pos, int B, int A, int G, void* stream) {
  return match_anchors<false>("rod_match_anchors", anc_corner, anc_center, lvl_off, thr, L, gt, gt_lbl, gt_n, out_off,
                              out_cbox, out_lbl, out_pos, B, A, G, stream);
}

int rod_match_anchors_nn(const float* anc_corner, const float* anc_center, const int* lvl_off, int L, const float* gt,
                         const int* gt_lbl, const int* gt_n, float* out_off, float* out_cbox, int* out_lbl,
                         int* out_pos, int B, int A, int G, void* stream) {
  return match_anchors<true>("rod_match_anchors_nn", anc_corner, anc_center, lvl_off, nullptr, L, gt, gt_lbl, gt_n,
                             out_off, out_cbox, out_lbl, out_pos, B, A, G, stream);
}

static int smoothl1_nbx(int B, const Levels& li) {
  long mx = 1;
  for (int l = 0; l < li.L; ++l) mx = std::max<long>(mx, (long)B * (li.off[l + 1] - li.off[l]));
  return cdiv(mx, 256);
}

size_t rod_smoothl1_workspace(int B, int A) {
  // at most A*B/256 + MAXL blocks per level, MAXL levels
  return (size_t)(cdivl((long)B * A, 256) + 1) * MAXL * sizeof(float);
}

int rod_smoothl1_masked(const void* pred, const float* target, const int* mask, const int* lvl_off, int L,
                        float scale, float* loss_lvl, void* grad, float* grad_target, void* workspace, int B, int A,
                        int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0, "rod_smoothl1_masked: bad shape");
  ROD_CHECK_ARG(scale != 0.f, "rod_smoothl1_masked: scale must be non-zero");
  ROD_CHECK_ARG(workspace && loss_lvl, "rod_smoothl1_masked: workspace/loss_lvl NULL");
  Levels li;
  if (int rc = fill_levels(li, lvl_off, nullptr, L, A)) return rc;
  const int nbx = smoothl1_nbx(B, li);
  const float inv = 1.0f / scale;
  hipStream_t s = ROD_STREAM(stream);
  auto run = [&](auto tt) {
    typedef decltype(tt) T;
    hipLaunchKernelGGL(smoothl1_kernel<T>, dim3(nbx, L), dim3(256), 0, s, (const T*)pred, target, mask, li, inv,
                       (T*)grad, grad_target, (float*)workspace, B, A, nbx);
  };
  ROD_CHECK_ARG(sel_dtype(dtype, run), "rod_smoothl1_masked: unsupported dtype code %d", dtype);
  hipLaunchKernelGGL(level_sum_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, nbx, L, 1.f, scale,
                     loss_lvl);
  return check_launch("rod_smoothl1_masked");
}

size_t rod_box_iou_loss_workspace(int B, int A) { return rod_smoothl1_workspace(B, A); }

int rod_box_iou_loss(const float* anc_center, const void* refine_out, const void* det_out, const float* cbox,
                     const int* det_pos, const int* lvl_off, int L, int kind, float weight, float scale,
                     float* loss_lvl, void* grad, void* workspace, int B, int A, int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0, "rod_box_iou_loss: B and A must be > 0, got B=%d A=%d", B, A);
  ROD_CHECK_ARG(kind >= 0 && kind <= 3, "rod_box_iou_loss: kind must be 0 (IoU), 1 (GIoU), 2 (DIoU) or 3 (CIoU), got %d",
                kind);
  ROD_CHECK_ARG(scale != 0.f, "rod_box_iou_loss: scale must be non-zero");
  ROD_CHECK_ARG(weight >= 0.f && weight <= 3.402823466e38f, "rod_box_iou_loss: weight must be finite and >= 0, got %g",
                (double)weight);
  ROD_CHECK_ARG(dtype == ROD_F32 || dtype == ROD_BF16, "rod_box_iou_loss: unsupported dtype code %d", dtype);
  Levels li;
  if (int rc = fill_levels(li, lvl_off, nullptr, L, A)) return rc;
  ROD_CHECK_ARG(anc_center && refine_out && det_out && cbox && det_pos,
                "rod_box_iou_loss: anc_center/refine_out/det_out/cbox/det_pos NULL");
  ROD_CHECK_ARG(workspace && loss_lvl, "rod_box_iou_loss: workspace/loss_lvl NULL");
  const int nbx = smoothl1_nbx(B, li);
  const float gscale = weight / scale;
  hipStream_t s = ROD_STREAM(stream);
  // one vector per row: 16 bytes (fp32 offsets) or 8 (bf16); the fp32 tables always 16
  const uintptr_t am = dtype == ROD_F32 ? 15 : 7;
  const bool vec = ((((uintptr_t)refine_out | (uintptr_t)det_out | (uintptr_t)grad) & am) |
                    (((uintptr_t)anc_center | (uintptr_t)cbox) & 15)) == 0;
  sel_dtype(dtype, [&](auto tt) {
    typedef decltype(tt) T;
    sel_bool(vec, [&](auto v) {
      hipLaunchKernelGGL((box_iou_loss_kernel<T, decltype(v)::value>), dim3(nbx, L), dim3(256), 0, s, anc_center,
                         (const T*)refine_out, (const T*)det_out, cbox, det_pos, li, kind, gscale, (T*)grad,
                         (float*)workspace, B, A, nbx);
    });
  });
  hipLaunchKernelGGL(level_sum_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, nbx, L, weight,
                     scale, loss_lvl);
  return check_launch("rod_box_iou_loss");
}

int rod_boxes_convert(const float* in, float* out, long n_boxes, int to_center, void* stream) {
  ROD_CHECK_ARG(n_boxes >= 0, "rod_boxes_convert: n < 0");
  ROD_CHECK_ARG((((uintptr_t)in | (uintptr_t)out) & 15) == 0, "rod_boxes_convert: buffers must be 16B aligned");
  if (n_boxes == 0) return 0;
  hipLaunchKernelGGL(boxes_convert_kernel, dim3(cdivl(n_boxes, 256)), dim3(256), 0, ROD_STREAM(stream), in, out,
                     n_boxes, to_center);
  return check_launch("rod_boxes_convert");
}

int rod_copy2d(const void* src, long src_ld_bytes, void* dst, long dst_ld_bytes, long rows, long cols_bytes,
               void* stream) {
  ROD_CHECK_ARG(rows >= 0 && cols_bytes >= 0, "rod_copy2d: bad extent");
  if (rows == 0 || cols_bytes == 0) return 0;
  const uintptr_t al = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)src_ld_bytes | (uintptr_t)dst_ld_bytes |
                       (uintptr_t)cols_bytes;
  hipStream_t s = ROD_STREAM(stream);
  const int wb = (al & 15) == 0 ? 16 : ((al & 3) == 0 ? 4 : 1);
  const long chunks = cols_bytes / wb;
  const int grid = (int)std::min<long>(cdivl(rows * chunks, 256), 8192);
  sel_int<16, 4, 1>(wb, [&](auto WB) {
    hipLaunchKernelGGL(copy2d_kernel<WB>, dim3(grid), dim3(256), 0, s, (const char*)src, src_ld_bytes, (char*)dst,
                       dst_ld_bytes, rows, chunks);
  });
  return check_launch("rod_copy2d");
}

}  // extern "C"
