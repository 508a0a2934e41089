// loss.hip — det_clf_loss classification part with global hard-negative mining
// (reference utils/net_tools.py:551-615), entirely on the device (no host sync):
//
//   p = softmax(logits) per row; nvalue = p[0] on negatives, 1 on positives      (571-575)
//   k = min(int32(3 * n_pos) + B, n_neg)                                          (578-581)
//   thr = k-th smallest nvalue  (exact 4 x 8-bit radix select on the f32 bits)   (583-584)
//   negatives kept: neg && nvalue < thr  (strict)                                  (587)
//   iou factor per (image, level): ((iou-mean)/sqrt(var+1e-8) - min) / (max+1e-8), ^4 (590-600)
//   pos_loss = sum CE(label) * pos * iouf / bs;  neg_loss = sum CE(0) * negmask / bs (605-613)
//   clf_loss = neg_loss / 2 + pos_loss                                             (615)
// plus d clf_loss / d logits.  Row layout: [B, A] anchors (levels concatenated per image).
//
// Opt-in alternative (rod_softmax_focal, not in the reference): focal loss over every row in one
// pass, without the selection and without the IoU factor; semantics in include/rod.h.
#include <math.h>

#include "box_common.h"

namespace rod {

constexpr int HNM_K = 16;  // max classes

// state words (int): [0] k  [1] prefix bits  [2] remaining rank  [3] n_pos  [4] n_neg  [5] n_neg_sel
// float outputs (8): pos_loss, neg_loss, clf_loss, max_hard_pred, n_pos, k, n_neg_selected, 0
struct HnmWs {
  float* nval;       // [R]
  float* gstat;      // [B*L][4]: mean, sd, zmin, den
  unsigned* hist;    // [256]
  int* state;        // [8]
  int* cnt_slab;     // [nb][2]
  double* loss_slab; // [nb][3]
};

template <typename T>
__global__ void __launch_bounds__(256) hnm_rows_kernel(const T* __restrict__ logits, const int* __restrict__ pos,
                                                       long R, int K, float* __restrict__ nval,
                                                       int* __restrict__ cnt_slab) {
  __shared__ int red[2][4];
  int np = 0, nn = 0;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    float e[HNM_K], m, s;
    row_softmax(logits + r * K, K, e, m, s);
    const bool p = pos[r] != 0;
    nval[r] = p ? 1.f : e[0] / s;  // tf.where(nmask, predictions[:, 0], 1. - fnmask)
    np += p ? 1 : 0;
    nn += p ? 0 : 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    np += __shfl_xor(np, o, 64);
    nn += __shfl_xor(nn, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = np;
    red[1][threadIdx.x >> 6] = nn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt_slab[blockIdx.x * 2 + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    cnt_slab[blockIdx.x * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ void hnm_count_kernel(const int* __restrict__ cnt_slab, int nb, int B, int* __restrict__ state,
                                 unsigned* __restrict__ hist) {
  __shared__ int s[2][256];
  int np = 0, nn = 0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    np += cnt_slab[2 * i];
    nn += cnt_slab[2 * i + 1];
  }
  s[0][threadIdx.x] = np;
  s[1][threadIdx.x] = nn;
  hist[threadIdx.x] = 0u;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s[0][threadIdx.x] += s[0][threadIdx.x + w];
      s[1][threadIdx.x] += s[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float n_pos = (float)s[0][0];
    int k = (int)(3.0f * n_pos) + B;          // tf.cast(negative_ratio * n_positives, tf.int32) + bs
    k = min(k, s[1][0]);                       // tf.minimum(n_neg, max_neg_entries)
    state[0] = k;
    state[1] = 0;                              // prefix
    state[2] = k;                              // rank (1-based) still to locate
    state[3] = s[0][0];
    state[4] = s[1][0];
  }
}

// histogram of digit `shift` among values whose higher digits equal the prefix
__global__ void __launch_bounds__(256) radix_hist_kernel(const float* __restrict__ v, long R, int shift,
                                                         const int* __restrict__ state, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned prefix = (unsigned)state[1];
  const unsigned hmask = shift >= 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
  if (state[0] > 0) {
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
      const unsigned b = __float_as_uint(v[r]);
      if ((b & hmask) == (prefix & hmask)) atomicAdd(&h[(b >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// pick the bucket holding the remaining rank; fix the digit; clear the histogram
__global__ void radix_scan_kernel(int shift, int* __restrict__ state, unsigned* __restrict__ hist) {
  if (threadIdx.x == 0 && state[0] > 0) {
    unsigned rank = (unsigned)state[2];
    unsigned acc = 0;
    int d = 0;
    for (; d < 256; ++d) {
      if (acc + hist[d] >= rank) break;
      acc += hist[d];
    }
    if (d > 255) d = 255;
    state[1] = (int)((unsigned)state[1] | ((unsigned)d << shift));
    state[2] = (int)(rank - acc);
  }
  __syncthreads();
  hist[threadIdx.x] = 0u;
}

// per (image, level) group: mean, sd = sqrt(var + 1e-8), zmin, den = max(z') + 1e-8
__global__ void __launch_bounds__(256) iou_group_kernel(const float* __restrict__ iou, Levels lv, int A,
                                                        float* __restrict__ gstat) {
  __shared__ double sd[256];
  __shared__ float smin[256], smax[256];
  const int g = blockIdx.x;
  const int b = g / lv.L, l = g - b * lv.L;
  const long r0 = (long)b * A + lv.off[l];
  const int n = lv.off[l + 1] - lv.off[l];
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float u = iou[r0 + i];
    s += (double)u;
    mn = fminf(mn, u);
    mx = fmaxf(mx, u);
  }
  sd[threadIdx.x] = s;
  smin[threadIdx.x] = mn;
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sd[threadIdx.x] += sd[threadIdx.x + w];
      smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + w]);
      smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + w]);
    }
    __syncthreads();
  }
  const float mean = (float)(sd[0] / (double)n);  // tf.nn.moments mean
  const float umin = smin[0], umax = smax[0];
  __syncthreads();
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = iou[r0 + i] - mean;
    v += (double)(d * d);                          // squared_difference(x, mean)
  }
  sd[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sd[threadIdx.x] += sd[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float var = (float)(sd[0] / (double)n);
    const float sdev = sqrtf(var + 1e-8f);
    const float zmin = (umin - mean) / sdev;       // reduce_min of the standardised values
    const float zmax = (umax - mean) / sdev + (0.f - zmin);
    gstat[g * 4 + 0] = mean;
    gstat[g * 4 + 1] = sdev;
    gstat[g * 4 + 2] = zmin;
    gstat[g * 4 + 3] = zmax + 1e-8f;
  }
}

__device__ __forceinline__ float iou_factor(float u, const float* gs) {
  const float z = (u - gs[0]) / gs[1];
  const float zz = z + (0.f - gs[2]);  // iou += 0. - reduce_min(iou)
  const float w = zz / gs[3];          // iou /= reduce_max(iou) + 1e-8
  return powf(w, 4.f);                 // tf.pow(iou, 4)
}

template <typename T>
__global__ void __launch_bounds__(256) hnm_loss_kernel(const T* __restrict__ logits, const int* __restrict__ lbl,
                                                       const int* __restrict__ pos, const float* __restrict__ iou,
                                                       const float* __restrict__ nval, const float* __restrict__ gstat,
                                                       const int* __restrict__ state, Levels lv, long R, int A,
                                                       int K, float inv_bs, T* __restrict__ grad,
                                                       double* __restrict__ slab) {
  __shared__ double red[3][4];
  const float thr = state[0] > 0 ? __uint_as_float((unsigned)state[1]) : 0.f;  // max_hard_pred
  double sp = 0.0, sn = 0.0, cn = 0.0;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    float e[HNM_K], m, s;
    const T* x = logits + r * K;
    row_softmax(x, K, e, m, s);
    const bool p = pos[r] != 0;
    const bool ng = !p && nval[r] < thr;  // logical_and(nmask, nvalues < max_hard_pred)
    const int a = (int)(r % A);
    const int b = (int)(r / A);
    const int l = level_of(lv, a);
    const float lse = log_cr(s);
    const int lab = lbl[r];
    float wp = 0.f, wn = 0.f;
    if (p) {
      const float f = iou_factor(iou[r], gstat + (b * lv.L + l) * 4);
      const float ce = lse - (to_f32(x[lab]) - m);   // sparse softmax xent (label)
      sp += (double)(ce * f);                        // pos_loss * fpmask * iou_factor
      wp = f * inv_bs;
    } else {
      // iou factor is still multiplied in the reference (times fpmask = 0)
    }
    if (ng) {
      const float ce0 = lse - (to_f32(x[0]) - m);    // no_classes = 0 on negatives
      sn += (double)ce0;
      cn += 1.0;
      wn = 0.5f * inv_bs;                            // clf_loss = neg_loss / 2 + pos_loss
    }
    if (grad) {
      for (int k = 0; k < K; ++k) {
        const float pk = e[k] / s;
        float g = 0.f;
        if (p) g += wp * (pk - (k == lab ? 1.f : 0.f));
        if (ng) g += wn * (pk - (k == 0 ? 1.f : 0.f));
        grad[r * K + k] = from_f32<T>(g);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sp += __shfl_xor(sp, o, 64);
    sn += __shfl_xor(sn, o, 64);
    cn += __shfl_xor(cn, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sp;
    red[1][threadIdx.x >> 6] = sn;
    red[2][threadIdx.x >> 6] = cn;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int j = 0; j < 3; ++j) slab[blockIdx.x * 3 + j] = red[j][0] + red[j][1] + red[j][2] + red[j][3];
}

__global__ void hnm_finalize_kernel(const double* __restrict__ slab, int nb, const int* __restrict__ state,
                                    float bs, float* __restrict__ out) {
  __shared__ double s[3][256];
  double a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    a += slab[i * 3];
    b += slab[i * 3 + 1];
    c += slab[i * 3 + 2];
  }
  s[0][threadIdx.x] = a;
  s[1][threadIdx.x] = b;
  s[2][threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int j = 0; j < 3; ++j) s[j][threadIdx.x] += s[j][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float pos_loss = (float)s[0][0] / bs;  // tf.div(reduce_sum(...), bs)
    const float neg_loss = (float)s[1][0] / bs;
    out[0] = pos_loss;
    out[1] = neg_loss;
    out[2] = neg_loss / 2.f + pos_loss;
    out[3] = state[0] > 0 ? __uint_as_float((unsigned)state[1]) : 0.f;
    out[4] = (float)state[3];
    out[5] = (float)state[0];
    out[6] = (float)s[2][0];
    out[7] = 0.f;
  }
}

// data-parallel split (rod_hnm_*): the per-rank counts, then k from the all-reduced counts
__global__ void hnm_sum_counts_kernel(const int* __restrict__ cnt_slab, int nb, int* __restrict__ counts) {
  __shared__ int s[2][256];
  int np = 0, nn = 0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    np += cnt_slab[2 * i];
    nn += cnt_slab[2 * i + 1];
  }
  s[0][threadIdx.x] = np;
  s[1][threadIdx.x] = nn;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s[0][threadIdx.x] += s[0][threadIdx.x + w];
      s[1][threadIdx.x] += s[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] = s[0][0];
    counts[1] = s[1][0];
  }
}
__global__ void hnm_begin_kernel(const int* __restrict__ counts, int B, int* __restrict__ state,
                                 unsigned* __restrict__ hist) {
  hist[threadIdx.x] = 0u;
  if (threadIdx.x == 0) {
    int k = (int)(3.0f * (float)counts[0]) + B;  // the same arithmetic as hnm_count_kernel
    k = min(k, counts[1]);
    state[0] = k;
    state[1] = 0;
    state[2] = k;
    state[3] = counts[0];
    state[4] = counts[1];
    state[5] = state[6] = state[7] = 0;
  }
}

// d clf_loss / d iou through the IoU focal factor (net_tools.py:590-607), the path that
// exists when refine_out is trained (train.py fix_refine=False; the reference applies no
// stop-gradient).  One block per (image, level) group, f64 sums, TF's gradient rules:
//   pos_loss = sum CE*pos*f / bs, f = w^4, w = zz/den, den = max(zz) + 1e-8, zz = z - min(z),
//   z = (u - mean)/sqrt(var + 1e-8) with tf.nn.moments (variance of stop_gradient(mean));
//   reduce_min / reduce_max split their gradient evenly over the tied elements.
// Recomputes the forward statistics with iou_group_kernel's exact float operations so the
// tie tests select the same elements.  g_iou [B*A] fp32 is written (0 for no gradient).
template <typename T>
__global__ void __launch_bounds__(256) iou_factor_bwd_kernel(const T* __restrict__ logits, const int* __restrict__ lbl,
                                                             const int* __restrict__ pos, const float* __restrict__ iou,
                                                             Levels lv, int A, int K, float inv_bs,
                                                             float* __restrict__ g_iou) {
  __shared__ double sd[4][256];
  __shared__ float smin[256], smax[256];
  const int g = blockIdx.x;
  const int b = g / lv.L, l = g - b * lv.L;
  const long r0 = (long)b * A + lv.off[l];
  const int n = lv.off[l + 1] - lv.off[l];
  const int tid = threadIdx.x;
  auto block_sum = [&](double v0, double v1, double v2, double v3, double (&o)[4]) {
    __syncthreads();
    sd[0][tid] = v0;
    sd[1][tid] = v1;
    sd[2][tid] = v2;
    sd[3][tid] = v3;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w)
        for (int j = 0; j < 4; ++j) sd[j][tid] += sd[j][tid + w];
      __syncthreads();
    }
    for (int j = 0; j < 4; ++j) o[j] = sd[j][0];
  };
  // forward statistics (iou_group_kernel)
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < n; i += 256) {
    const float u = iou[r0 + i];
    s += (double)u;
    mn = fminf(mn, u);
    mx = fmaxf(mx, u);
  }
  smin[tid] = mn;
  smax[tid] = mx;
  double o4[4];
  block_sum(s, 0.0, 0.0, 0.0, o4);
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      smin[tid] = fminf(smin[tid], smin[tid + w]);
      smax[tid] = fmaxf(smax[tid], smax[tid + w]);
    }
    __syncthreads();
  }
  const float mean = (float)(o4[0] / (double)n);
  const float umin = smin[0], umax = smax[0];
  double v = 0.0;
  for (int i = tid; i < n; i += 256) {
    const float d = iou[r0 + i] - mean;
    v += (double)(d * d);
  }
  block_sum(v, 0.0, 0.0, 0.0, o4);
  const float var = (float)(o4[0] / (double)n);
  const float sdev = sqrtf(var + 1e-8f);
  const float zmin = (umin - mean) / sdev;
  const float zzmax = (umax - mean) / sdev + (0.f - zmin);
  const float den = zzmax + 1e-8f;
  // pass A: a_i = dL/dw_i = G_i * 4 w^3 (G_i = CE_i * pos_i / bs) -> g_iou (scratch);
  // sums a*zz (den), tie counts of max(zz) and min(z)
  double saz = 0.0, cmax = 0.0, cmin = 0.0;
  for (int i = tid; i < n; i += 256) {
    const long r = r0 + i;
    const float u = iou[r];
    const float z = (u - mean) / sdev;
    const float zz = z + (0.f - zmin);
    const float w = zz / den;
    float a = 0.f;
    if (pos[r] != 0) {
      const T* x = logits + r * K;
      float e[HNM_K], m, se;
      row_softmax(x, K, e, m, se);
      const float ce = log_cr(se) - (to_f32(x[lbl[r]]) - m);
      a = ce * inv_bs * (4.f * powf(w, 3.f));
    }
    g_iou[r] = a;
    saz += (double)a * (double)zz;
    cmax += zz == zzmax ? 1.0 : 0.0;
    cmin += z == zmin ? 1.0 : 0.0;
  }
  block_sum(saz, cmax, cmin, 0.0, o4);
  const double dden = -o4[0] / ((double)den * (double)den);
  const double tmax = dden / o4[1];   // reduce_max: split over the ties
  const double ncmin = o4[2];
  // pass B: dzz_i = a_i/den + [zz_i max] tmax; sum dzz (-> d min(z))
  double sdzz = 0.0;
  for (int i = tid; i < n; i += 256) {
    const long r = r0 + i;
    const float u = iou[r];
    const float z = (u - mean) / sdev;
    const float zz = z + (0.f - zmin);
    double dzz = (double)g_iou[r] / (double)den + (zz == zzmax ? tmax : 0.0);
    g_iou[r] = (float)dzz;
    sdzz += dzz;
  }
  block_sum(sdzz, 0.0, 0.0, 0.0, o4);
  const double tmin = -o4[0] / ncmin;   // d min(z) = -sum dzz, split over the ties
  // pass C: g_i = dL/dz_i; sums g and g*(u - mean)
  double sg = 0.0, sgu = 0.0;
  for (int i = tid; i < n; i += 256) {
    const long r = r0 + i;
    const float u = iou[r];
    const float z = (u - mean) / sdev;
    const double gi = (double)g_iou[r] + (z == zmin ? tmin : 0.0);
    g_iou[r] = (float)gi;
    sg += gi;
    sgu += gi * (double)(u - mean);
  }
  block_sum(sg, sgu, 0.0, 0.0, o4);
  // z = (u - mean)/s, s = sqrt(var + 1e-8), var = mean((u - stop_gradient(mean))^2)
  const double sd_ = (double)sdev;
  const double dsdev = -o4[1] / (sd_ * sd_);
  const double cmean = -o4[0] / sd_ / (double)n;
  for (int i = tid; i < n; i += 256) {
    const long r = r0 + i;
    const double gi = (double)g_iou[r];
    const double du = gi / sd_ + cmean + dsdev * (double)(iou[r] - mean) / ((double)n * sd_);
    g_iou[r] = (float)du;
  }
}

static int hnm_blocks(long R) { return (int)std::min<long>(cdivl(R, 256), 2048); }

static HnmWs carve(void* ws, long R, int B, int L, int nb) {
  char* p = (char*)ws;
  auto take = [&](size_t n) {
    char* r = p;
    p += (n + 255) & ~(size_t)255;
    return r;
  };
  HnmWs w;
  w.nval = (float*)take(R * sizeof(float));
  w.gstat = (float*)take((size_t)B * L * 4 * sizeof(float));
  w.hist = (unsigned*)take(256 * sizeof(unsigned));
  w.state = (int*)take(8 * sizeof(int));
  w.cnt_slab = (int*)take((size_t)nb * 2 * sizeof(int));
  w.loss_slab = (double*)take((size_t)nb * 3 * sizeof(double));
  return w;
}

// ---- focal loss (include/rod.h, ABI 26): count -> loss -> finalize ----------------------------
// workspace: [0, 256) counts2 of the single-process form, then the loss slab [nb][2] fp64
constexpr int FOCAL_ROWS = 256;  // rows per block pass = threads per block

// counts2 += (positives, negatives) of pos[0, R): 16-byte loads between a scalar head and tail,
// one pair of integer atomics per block (integer sums: the order does not matter)
__global__ void __launch_bounds__(256) focal_count_kernel(const int* __restrict__ pos, long R,
                                                          int* __restrict__ counts2) {
  __shared__ int red[2][4];
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const long h = (long)(((16 - ((uintptr_t)pos & 15)) & 15) / 4);  // pos is 4-byte aligned
  const long head = h < R ? h : R;
  const long nv = (R - head) / 4;
  const long tail0 = head + nv * 4;
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long gs = (long)gridDim.x * blockDim.x;
  int np = 0, nn = 0;
  if (g < head) {
    np += pos[g] != 0;
    nn += pos[g] == 0;
  }
  for (long v = g; v < nv; v += gs) {
    const i32x4 p = *(const i32x4*)(pos + head + v * 4);
    const int c = (p[0] != 0) + (p[1] != 0) + (p[2] != 0) + (p[3] != 0);
    np += c;
    nn += 4 - c;
  }
  if (tail0 + g < R) {  // at most 3 elements
    np += pos[tail0 + g] != 0;
    nn += pos[tail0 + g] == 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    np += __shfl_xor(np, o, 64);
    nn += __shfl_xor(nn, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = np;
    red[1][threadIdx.x >> 6] = nn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int bp = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const int bn = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (bp) atomicAdd(&counts2[0], bp);
    if (bn) atomicAdd(&counts2[1], bn);
  }
}

// A block pass handles FOCAL_ROWS consecutive rows = one contiguous span of n <= 256 K elements.
// The span is copied between global memory and LDS with 16-byte vectors; `buf` is the LDS array
// already shifted by the span's misalignment (in elements) so that a 16-byte aligned global
// address is a 16-byte aligned LDS address.  The elements before the first and after the last
// aligned vector of the span go one at a time.
template <typename T>
__device__ __forceinline__ int span_mis(const T* g) {
  return (int)(((uintptr_t)g / sizeof(T)) % Vec16<T>::N);
}
template <typename T, bool IN>
__device__ __forceinline__ void span_copy(T* g, T* buf, int mis, int n) {
  constexpr int VN = Vec16<T>::N;
  const int head = min(n, (VN - mis) % VN);
  const int nv = (n - head) / VN;
  const int tail0 = head + nv * VN;
  const int tid = threadIdx.x;
  if (tid < head) {
    if constexpr (IN) buf[tid] = g[tid];
    else g[tid] = buf[tid];
  }
  for (int v = tid; v < nv; v += FOCAL_ROWS) {
    Vec16<T> x;
    if constexpr (IN) {
      x.load(g + head + v * VN);
      x.store(buf + head + v * VN);
    } else {
      x.load(buf + head + v * VN);
      x.store_out(g + head + v * VN);
    }
  }
  if (tail0 + tid < n) {
    if constexpr (IN) buf[tail0 + tid] = g[tail0 + tid];
    else g[tail0 + tid] = buf[tail0 + tid];
  }
}

template <typename T, bool GRAD>
__global__ void __launch_bounds__(256) focal_loss_kernel(const T* __restrict__ logits, const int* __restrict__ lbl,
                                                         const int* __restrict__ pos,
                                                         const int* __restrict__ counts2, float alpha, float gamma,
                                                         long R, int K, T* __restrict__ grad,
                                                         double* __restrict__ slab) {
  constexpr int VN = Vec16<T>::N;
  __shared__ __attribute__((aligned(16))) T sm[FOCAL_ROWS * HNM_K + VN];
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const float norm = (float)max(counts2[0], 1);
  const long nrb = (R + FOCAL_ROWS - 1) / FOCAL_ROWS;
  double sp = 0.0, sn = 0.0;
  for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const long r0 = rb * FOCAL_ROWS;
    const int rows = R - r0 < FOCAL_ROWS ? (int)(R - r0) : FOCAL_ROWS;
    const long e0 = r0 * K;
    const int n = rows * K;
    const int mis = span_mis(logits + e0);
    span_copy<T, true>(const_cast<T*>(logits) + e0, sm + mis, mis, n);
    __syncthreads();
    float e[HNM_K];
    float coef = 0.f, q = 0.f;
    int t = 0;
    if (tid < rows) {
      const T* x = sm + mis + tid * K;
      const bool p = pos[r0 + tid] != 0;
      t = p ? lbl[r0 + tid] : 0;
      float m = to_f32(x[0]);
#pragma unroll
      for (int k = 0; k < HNM_K; ++k)
        if (k < K) {
          e[k] = to_f32(x[k]);
          m = fmaxf(m, e[k]);
        }
      float s = 0.f, et = 0.f, dt = 0.f;
#pragma unroll
      for (int k = 0; k < HNM_K; ++k)
        if (k < K) {
          const float d = e[k] - m;
          e[k] = exp_cr(d);
          s += e[k];
          if (k == t) {
            et = e[k];
            dt = d;
          }
        }
      q = (s - et) / s;
      const float pt = et / s;
      const float lp = dt - log_cr(s);
      const float a = p ? alpha : 1.f - alpha;
      const float w = gamma == 0.f ? 1.f : (q == 0.f ? 0.f : powf(q, gamma));
      const float fl = -(a * w * lp);
      if (p) sp += (double)fl;
      else sn += (double)fl;
      if constexpr (GRAD) {
        const float t1 = (gamma > 0.f && q > 0.f) ? gamma * (w / q) * pt * lp : 0.f;
        coef = a * (t1 - w) / norm;
#pragma unroll
        for (int k = 0; k < HNM_K; ++k)
          if (k < K) e[k] = e[k] / s;  // p_k
      }
    }
    if constexpr (GRAD) {
      const int misg = span_mis(grad + e0);
      __syncthreads();  // every row has been read: the buffer now takes the gradient
      if (tid < rows) {
        T* gx = sm + misg + tid * K;
#pragma unroll
        for (int k = 0; k < HNM_K; ++k)
          if (k < K) gx[k] = from_f32<T>((k == t ? q : -e[k]) * coef);
      }
      __syncthreads();
      span_copy<T, false>(grad + e0, sm + misg, misg, n);
    }
    __syncthreads();  // before the next pass overwrites the buffer
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sp += __shfl_xor(sp, o, 64);
    sn += __shfl_xor(sn, o, 64);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sp;
    red[1][tid >> 6] = sn;
  }
  __syncthreads();
  if (tid == 0)
    for (int j = 0; j < 2; ++j) slab[blockIdx.x * 2 + j] = red[j][0] + red[j][1] + red[j][2] + red[j][3];
}

__global__ void focal_finalize_kernel(const double* __restrict__ slab, int nb, const int* __restrict__ counts2,
                                      float* __restrict__ out) {
  __shared__ double s[2][256];
  double a = 0, b = 0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    a += slab[i * 2];
    b += slab[i * 2 + 1];
  }
  s[0][threadIdx.x] = a;
  s[1][threadIdx.x] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int j = 0; j < 2; ++j) s[j][threadIdx.x] += s[j][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int norm = max(counts2[0], 1);
    const float pos_loss = (float)(s[0][0] / (double)norm);
    const float neg_loss = (float)(s[1][0] / (double)norm);
    out[0] = pos_loss;
    out[1] = neg_loss;
    out[2] = pos_loss + neg_loss;
    out[3] = 0.f;
    out[4] = (float)counts2[0];
    out[5] = 0.f;
    out[6] = (float)counts2[1];
    out[7] = (float)norm;
  }
}

static int focal_check(const char* who, int B, int A, int K, float alpha, float gamma) {
  ROD_CHECK_ARG(B > 0 && A > 0, "%s: B and A must be > 0 (got B %d, A %d)", who, B, A);
  ROD_CHECK_ARG(K >= 2 && K <= HNM_K, "%s: K must be in 2..16 (got %d)", who, K);
  ROD_CHECK_ARG(isfinite(gamma) && gamma >= 0.f, "%s: gamma must be finite and >= 0 (got %g)", who, (double)gamma);
  ROD_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha must be in [0, 1] (got %g)", who, (double)alpha);
  return 0;
}

static int focal_count(const int* det_pos, int* counts2, long R, hipStream_t s) {
  hipError_t e = hipMemsetAsync(counts2, 0, 2 * sizeof(int), s);
  if (e != hipSuccess) {
    set_error("rod_focal_count: hipMemsetAsync: %s", hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(focal_count_kernel, dim3(hnm_blocks(cdivl(R, 4))), dim3(256), 0, s, det_pos, R, counts2);
  return 0;
}

static void focal_loss(const void* logits, const int* det_lbl, const int* det_pos, const int* counts2, float alpha,
                       float gamma, float* out, void* grad, double* slab, long R, int K, int dtype, hipStream_t s) {
  const int nb = hnm_blocks(R);
  sel_dtype(dtype, [&](auto tag) {
    typedef decltype(tag) T;
    sel_bool(grad != nullptr, [&](auto g) {
      hipLaunchKernelGGL((focal_loss_kernel<T, decltype(g)::value>), dim3(nb), dim3(256), 0, s, (const T*)logits,
                         det_lbl, det_pos, counts2, alpha, gamma, R, K, (T*)grad, slab);
    });
  });
  hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, s, slab, nb, counts2, out);
}

}  // namespace rod

using namespace rod;

extern "C" {

size_t rod_softmax_ce_hnm_workspace(int B, int A, int L) {
  const long R = (long)B * A;
  const int nb = hnm_blocks(R);
  return ((R * 4 + 255) & ~255L) + (((long)B * L * 16 + 255) & ~255L) + 1024 + 256 + (((long)nb * 8 + 255) & ~255L) +
         (((long)nb * 24 + 255) & ~255L) + 256;
}

int rod_softmax_ce_hnm(const void* logits, const int* det_lbl, const int* det_pos, const float* iou,
                       const int* lvl_off, int L, float bs, float* out, void* grad, void* workspace, int B, int A,
                       int K, int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0 && K > 1 && K <= HNM_K, "rod_softmax_ce_hnm: bad shape (K <= 16)");
  Levels lv;
  if (int rc = fill_levels(lv, lvl_off, nullptr, L, A)) return rc;
  ROD_CHECK_ARG(workspace && out, "rod_softmax_ce_hnm: workspace/out NULL");
  const long R = (long)B * A;
  const int nb = hnm_blocks(R);
  HnmWs w = carve(workspace, R, B, L, nb);
  hipStream_t s = ROD_STREAM(stream);
  const float inv_bs = 1.0f / bs;
  auto run = [&](auto tt) {
    typedef decltype(tt) T;
    hipLaunchKernelGGL(hnm_rows_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)logits, det_pos, R, K, w.nval,
                       w.cnt_slab);
    hipLaunchKernelGGL(hnm_count_kernel, dim3(1), dim3(256), 0, s, w.cnt_slab, nb, B, w.state, w.hist);
    for (int shift = 24; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(256), 0, s, w.nval, R, shift, w.state, w.hist);
      hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(256), 0, s, shift, w.state, w.hist);
    }
    hipLaunchKernelGGL(iou_group_kernel, dim3(B * L), dim3(256), 0, s, iou, lv, A, w.gstat);
    hipLaunchKernelGGL(hnm_loss_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)logits, det_lbl, det_pos, iou, w.nval,
                       w.gstat, w.state, lv, R, A, K, inv_bs, (T*)grad, w.loss_slab);
    hipLaunchKernelGGL(hnm_finalize_kernel, dim3(1), dim3(256), 0, s, w.loss_slab, nb, w.state, bs, out);
  };
  ROD_CHECK_ARG(sel_dtype(dtype, run), "rod_softmax_ce_hnm: unsupported dtype code %d", dtype);
  return check_launch("rod_softmax_ce_hnm");
}

int rod_iou_factor_bwd(const void* logits, const int* det_lbl, const int* det_pos, const float* iou,
                       const int* lvl_off, int L, float bs, float* g_iou, int B, int A, int K, int dtype,
                       void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0 && K > 1 && K <= HNM_K && g_iou, "rod_iou_factor_bwd: bad arguments");
  Levels lv;
  if (int rc = fill_levels(lv, lvl_off, nullptr, L, A)) return rc;
  auto run = [&](auto tt) {
    typedef decltype(tt) T;
    hipLaunchKernelGGL(iou_factor_bwd_kernel<T>, dim3(B * L), dim3(256), 0, ROD_STREAM(stream), (const T*)logits,
                       det_lbl, det_pos, iou, lv, A, K, 1.0f / bs, g_iou);
  };
  ROD_CHECK_ARG(sel_dtype(dtype, run), "rod_iou_factor_bwd: unsupported dtype code %d", dtype);
  return check_launch("rod_iou_factor_bwd");
}

// ---- data-parallel split: per-rank rows, exchange points are counts[2] and hist[256] ----
size_t rod_hnm_workspace(int B, int A, int L) { return rod_softmax_ce_hnm_workspace(B, A, L); }

int rod_hnm_rows(const void* logits, const int* det_pos, void* workspace, int* counts, int B, int A, int K, int L,
                 int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0 && K > 1 && K <= HNM_K && workspace && counts, "rod_hnm_rows: bad arguments");
  const long R = (long)B * A;
  const int nb = hnm_blocks(R);
  HnmWs w = carve(workspace, R, B, L, nb);
  hipStream_t s = ROD_STREAM(stream);
  auto run = [&](auto tt) {
    typedef decltype(tt) T;
    hipLaunchKernelGGL(hnm_rows_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)logits, det_pos, R, K, w.nval,
                       w.cnt_slab);
  };
  ROD_CHECK_ARG(sel_dtype(dtype, run), "rod_hnm_rows: unsupported dtype code %d", dtype);
  hipLaunchKernelGGL(hnm_sum_counts_kernel, dim3(1), dim3(256), 0, s, w.cnt_slab, nb, counts);
  return check_launch("rod_hnm_rows");
}

int rod_hnm_begin(const int* counts, int B_global, int* state, unsigned* hist, void* stream) {
  ROD_CHECK_ARG(counts && state && hist && B_global > 0, "rod_hnm_begin: bad arguments");
  hipLaunchKernelGGL(hnm_begin_kernel, dim3(1), dim3(256), 0, ROD_STREAM(stream), counts, B_global, state, hist);
  return check_launch("rod_hnm_begin");
}

int rod_hnm_radix_hist(const void* workspace, int B, int A, int L, int shift, const int* state, unsigned* hist,
                       void* stream) {
  ROD_CHECK_ARG(workspace && state && hist && (shift == 0 || shift == 8 || shift == 16 || shift == 24),
                "rod_hnm_radix_hist: bad arguments");
  const long R = (long)B * A;
  const int nb = hnm_blocks(R);
  HnmWs w = carve((void*)workspace, R, B, L, nb);
  hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(256), 0, ROD_STREAM(stream), w.nval, R, shift, state, hist);
  return check_launch("rod_hnm_radix_hist");
}

int rod_hnm_radix_scan(int shift, int* state, unsigned* hist, void* stream) {
  ROD_CHECK_ARG(state && hist, "rod_hnm_radix_scan: bad arguments");
  hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(256), 0, ROD_STREAM(stream), shift, state, hist);
  return check_launch("rod_hnm_radix_scan");
}

int rod_hnm_loss(const void* logits, const int* det_lbl, const int* det_pos, const float* iou, const int* lvl_off,
                 int L, float bs, const int* state, float* out, void* grad, void* workspace, int B, int A, int K,
                 int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0 && K > 1 && K <= HNM_K, "rod_hnm_loss: bad shape (K <= 16)");
  Levels lv;
  if (int rc = fill_levels(lv, lvl_off, nullptr, L, A)) return rc;
  ROD_CHECK_ARG(workspace && out && state, "rod_hnm_loss: workspace/out/state NULL");
  const long R = (long)B * A;
  const int nb = hnm_blocks(R);
  HnmWs w = carve(workspace, R, B, L, nb);
  hipStream_t s = ROD_STREAM(stream);
  auto run = [&](auto tt) {
    typedef decltype(tt) T;
    hipLaunchKernelGGL(iou_group_kernel, dim3(B * L), dim3(256), 0, s, iou, lv, A, w.gstat);
    hipLaunchKernelGGL(hnm_loss_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)logits, det_lbl, det_pos, iou, w.nval,
                       w.gstat, state, lv, R, A, K, 1.0f / bs, (T*)grad, w.loss_slab);
    hipLaunchKernelGGL(hnm_finalize_kernel, dim3(1), dim3(256), 0, s, w.loss_slab, nb, state, bs, out);
  };
  ROD_CHECK_ARG(sel_dtype(dtype, run), "rod_hnm_loss: unsupported dtype code %d", dtype);
  return check_launch("rod_hnm_loss");
}

// ---- focal loss: the opt-in alternative to everything above (semantics: include/rod.h) ----
size_t rod_softmax_focal_workspace(int B, int A) {
  return 256 + (((size_t)hnm_blocks((long)B * A) * 2 * sizeof(double) + 255) & ~(size_t)255);
}

int rod_focal_count(const int* det_pos, void* workspace, int* counts2, int B, int A, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0, "rod_focal_count: B and A must be > 0 (got B %d, A %d)", B, A);
  ROD_CHECK_ARG(det_pos && workspace && counts2, "rod_focal_count: det_pos/workspace/counts2 NULL");
  if (int rc = focal_count(det_pos, counts2, (long)B * A, ROD_STREAM(stream))) return rc;
  return check_launch("rod_focal_count");
}

int rod_focal_loss(const void* logits, const int* det_lbl, const int* det_pos, const int* counts2, float alpha,
                   float gamma, float* out, void* grad, void* workspace, int B, int A, int K, int dtype,
                   void* stream) {
  if (int rc = focal_check("rod_focal_loss", B, A, K, alpha, gamma)) return rc;
  ROD_CHECK_ARG(dtype == ROD_F32 || dtype == ROD_BF16, "rod_focal_loss: unsupported dtype code %d", dtype);
  ROD_CHECK_ARG(logits && det_lbl && det_pos && counts2 && out && workspace,
                "rod_focal_loss: logits/det_lbl/det_pos/counts2/out/workspace NULL");
  focal_loss(logits, det_lbl, det_pos, counts2, alpha, gamma, out, grad, (double*)((char*)workspace + 256),
             (long)B * A, K, dtype, ROD_STREAM(stream));
  return check_launch("rod_focal_loss");
}

int rod_softmax_focal(const void* logits, const int* det_lbl, const int* det_pos, float alpha, float gamma,
                      float* out, void* grad, void* workspace, int B, int A, int K, int dtype, void* stream) {
  if (int rc = focal_check("rod_softmax_focal", B, A, K, alpha, gamma)) return rc;
  ROD_CHECK_ARG(dtype == ROD_F32 || dtype == ROD_BF16, "rod_softmax_focal: unsupported dtype code %d", dtype);
  ROD_CHECK_ARG(logits && det_lbl && det_pos && out && workspace,
                "rod_softmax_focal: logits/det_lbl/det_pos/out/workspace NULL");
  int* counts2 = (int*)workspace;
  if (int rc = focal_count(det_pos, counts2, (long)B * A, ROD_STREAM(stream))) return rc;
  focal_loss(logits, det_lbl, det_pos, counts2, alpha, gamma, out, grad, (double*)((char*)workspace + 256),
             (long)B * A, K, dtype, ROD_STREAM(stream));
  return check_launch("rod_softmax_focal");
}

}  // extern "C"
