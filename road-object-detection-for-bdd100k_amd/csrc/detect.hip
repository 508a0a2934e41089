// detect.hip — deconvolution-pyramid helpers and the ODM (det) target path.
//
//   legacy bilinear resize   tf.image.resize_images(BILINEAR, align_corners=False), TF1
//                            scaling src = dst * (in/out) (catch_net.py:207; tf_image.py:275)
//   depth-to-space 2x2       conv2d_transpose(k=2, s=2, SAME) = 1x1 GEMM [M, i_c] x [i_c, 4 f_c]
//                            followed by this scatter (catch_net.py:196); cropping of odd outputs
//   add                      ADD merge (catch_net.py:269), refine_out + det_out (predict.py:132)
//   decode                   decode_locations_one_layer (net_tools.py:182-234) [+ centre->corner]
//   det targets              det_groundtruth (net_tools.py:431-475)
//   softmax                  slim.softmax over the class axis (predict.py:128)
// Compiled with -ffp-contract=off: each expression rounds per op like the TF op chain.
#include <math.h>

#include "box_common.h"

namespace rod {

// ---------------------------------------------------------------- legacy bilinear
struct Lerp {
  int lo, hi;
  float f;
};
__device__ __forceinline__ Lerp legacy_lerp(int o, float scale, int n_in) {
  const float in = (float)o * scale;  // LegacyScaler: out * scale, no half-pixel offset
  const float fl = floorf(in);
  Lerp r;
  r.lo = max((int)fl, 0);
  r.hi = min((int)ceilf(in), n_in - 1);
  r.f = in - fl;
  return r;
}

template <typename T>
__global__ void resize_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho,
                                  int Wo, float sy, float sx) {
  const long total = (long)N * Ho * Wo * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long t = i / C;
    const int xo = (int)(t % Wo);
    t /= Wo;
    const int yo = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const Lerp ly = legacy_lerp(yo, sy, H), lx = legacy_lerp(xo, sx, W);
    const T* b = x + (long)n * H * W * C + c;
    const float tl = to_f32(b[((long)ly.lo * W + lx.lo) * C]);
    const float tr = to_f32(b[((long)ly.lo * W + lx.hi) * C]);
    const float bl = to_f32(b[((long)ly.hi * W + lx.lo) * C]);
    const float br = to_f32(b[((long)ly.hi * W + lx.hi) * C]);
    const float top = tl + (tr - tl) * lx.f;  // compute_lerp (resize_bilinear_op.cc)
    const float bot = bl + (br - bl) * lx.f;
    y[i] = from_f32<T>(top + (bot - top) * ly.f);
  }
}

// ResizeBilinearGrad as a gather: every input pixel sums the weights of the output pixels
// whose lo/hi taps land on it (deterministic; no atomics).
template <typename T>
__global__ void resize_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C, int Ho,
                                  int Wo, float sy, float sx) {
  const long total = (long)N * H * W * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long t = i / C;
    const int xi = (int)(t % W);
    t /= W;
    const int yi = (int)(t % H);
    const int n = (int)(t / H);
    // output rows whose taps can touch yi: in = yo*sy in (yi-1, yi+1]
    const int y_lo = max(0, (int)floorf((float)(yi - 1) / sy) - 1);
    const int y_hi = min(Ho - 1, (int)ceilf((float)(yi + 1) / sy) + 1);
    const int x_lo = max(0, (int)floorf((float)(xi - 1) / sx) - 1);
    const int x_hi = min(Wo - 1, (int)ceilf((float)(xi + 1) / sx) + 1);
    float acc = 0.f;
    for (int yo = y_lo; yo <= y_hi; ++yo) {
      const Lerp ly = legacy_lerp(yo, sy, H);
      float wy = 0.f;
      if (ly.lo == yi) wy += 1.f - ly.f;
      if (ly.hi == yi) wy += ly.f;
      if (wy == 0.f) continue;
      for (int xo = x_lo; xo <= x_hi; ++xo) {
        const Lerp lx = legacy_lerp(xo, sx, W);
        float wx = 0.f;
        if (lx.lo == xi) wx += 1.f - lx.f;
        if (lx.hi == xi) wx += lx.f;
        if (wx == 0.f) continue;
        acc = fmaf(to_f32(dy[(((long)n * Ho + yo) * Wo + xo) * C + c]), wy * wx, acc);
      }
    }
    dx[i] = from_f32<T>(acc);
  }
}

// ---------------------------------------------------------------- deconv scatter / gather
// out[n, 2i+a, 2j+b, f] = z[n, i, j, (a*2+b)*F + f]   (rows/cols beyond Ho/Wo cropped)
template <typename T>
__global__ void d2s_kernel(const T* __restrict__ z, T* __restrict__ out, int N, int h, int w, int F, int Ho, int Wo,
                           int ldo) {
  const long total = (long)N * Ho * Wo * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    long t = i / F;
    const int xo = (int)(t % Wo);
    t /= Wo;
    const int yo = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const int a = yo & 1, b = xo & 1;
    out[(((long)n * Ho + yo) * Wo + xo) * ldo + f] =
        z[(((long)n * h + (yo >> 1)) * w + (xo >> 1)) * 4 * F + (a * 2 + b) * F + f];
  }
}

template <typename T>
__global__ void s2d_kernel(const T* __restrict__ dout, T* __restrict__ dz, int N, int h, int w, int F, int Ho, int Wo,
                           int ldo) {
  const long total = (long)N * h * w * 4 * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i % (4 * F));
    long t = i / (4 * F);
    const int j = (int)(t % w);
    t /= w;
    const int ii = (int)(t % h);
    const int n = (int)(t / h);
    const int ab = q / F, f = q - ab * F;
    const int yo = 2 * ii + (ab >> 1), xo = 2 * j + (ab & 1);
    dz[i] = (yo < Ho && xo < Wo) ? dout[(((long)n * Ho + yo) * Wo + xo) * ldo + f] : (T)0.f;
  }
}

template <typename T>
__global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ c, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    c[i] = from_f32<T>(to_f32(a[i]) + to_f32(b[i]));
}

// ---------------------------------------------------------------- decode
// out = decode(anchor, a (+ b)), centre form or corner form, fp32 [B, A, 4]
template <typename T>
__global__ void decode_kernel(const float* __restrict__ anc_center, const T* __restrict__ oa,
                              const T* __restrict__ ob, float* __restrict__ out, long BA, int A, int to_corner) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < BA; i += (long)gridDim.x * blockDim.x) {
    const int a = (int)(i % A);
    const f32x4 az = *(const f32x4*)(anc_center + (long)a * 4);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = to_f32(oa[i * 4 + k]);
      if (ob) o[k] = o[k] + to_f32(ob[i * 4 + k]);  // refine_out + det_out (predict.py:132)
    }
    const f32x4 z = decode_center(az, o);
    *(f32x4*)(out + i * 4) = to_corner ? center_to_corner(z) : z;
  }
}

// ---------------------------------------------------------------- det targets
template <typename T>
__global__ void det_targets_kernel(const float* __restrict__ anc_center, const T* __restrict__ refine_out,
                                   const float* __restrict__ refine_gt, const float* __restrict__ cbox,
                                   const int* __restrict__ label, const int* __restrict__ refine_pos, Levels lv,
                                   float* __restrict__ det_gt, int* __restrict__ det_pos, int* __restrict__ det_lbl,
                                   float* __restrict__ iou_out, long BA, int A) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < BA; i += (long)gridDim.x * blockDim.x) {
    const int a = (int)(i % A);
    const int l = level_of(lv, a);
    const f32x4 az = *(const f32x4*)(anc_center + (long)a * 4);
    float ro[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ro[k] = to_f32(refine_out[i * 4 + k]);
    // adjusted anchor = corner(decode(anchor, refine_out))   (net_tools.py:459-460)
    const f32x4 ac = center_to_corner(decode_center(az, ro));
    // gt corner (net_tools.py:463)
    const f32x4 gc = center_to_corner(*(const f32x4*)(cbox + i * 4));
    const float iou = jaccard_ref(ac, vol_anchor(ac), gc, vol_gt(gc));
    const int pos = (iou >= lv.thr[l] ? 1 : 0) * refine_pos[i];  // net_tools.py:468-469
    const float pm = (float)pos;
    const f32x4 rg = *(const f32x4*)(refine_gt + i * 4);
    f32x4 dg;
#pragma unroll
    for (int k = 0; k < 4; ++k) dg[k] = (rg[k] - ro[k]) * pm;  // (offset_gt - refine_out) * mask
    *(f32x4*)(det_gt + i * 4) = dg;
    det_pos[i] = pos;
    det_lbl[i] = label[i] * pos;
    iou_out[i] = iou;
  }
}

// Backward of det_targets wrt refine_out (train.py fix_refine=False; no stop-gradient in the
// reference): det_gt = (refine_gt - refine_out)*pos (net_tools.py:471) gives -g_det_gt*pos;
// iou = jaccard(corner(decode(anchor, refine_out)), corner(cbox)) (459-465) gives the chain
// below with TF's gradient rules (maximum -> the first argument when x >= y, minimum -> when
// x <= y, max(., 0) passes at >= 0).  The forward is recomputed with det_targets_kernel's
// exact operations.
template <typename T>
__global__ void det_targets_bwd_kernel(const float* __restrict__ anc_center, const T* __restrict__ refine_out,
                                       const float* __restrict__ cbox, const int* __restrict__ det_pos,
                                       const float* __restrict__ g_det_gt, const float* __restrict__ g_iou,
                                       T* __restrict__ g_ro, long BA, int A) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < BA; i += (long)gridDim.x * blockDim.x) {
    const int a = (int)(i % A);
    const f32x4 az = *(const f32x4*)(anc_center + (long)a * 4);
    float ro[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ro[k] = to_f32(refine_out[i * 4 + k]);
    const f32x4 z = decode_center(az, ro);
    const f32x4 ac = center_to_corner(z);
    const f32x4 gc = center_to_corner(*(const f32x4*)(cbox + i * 4));
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    const float G = g_iou ? g_iou[i] : 0.f;
    if (G != 0.f) {
      const Jaccard j = jaccard_ref_parts(ac, vol_anchor(ac), gc, vol_gt(gc));
      const float q = G * j.inter / (j.uni * j.uni);
      const float d_inter = G / j.uni + q;  // d iou/d inter, with union = vol_a - inter + vol_g
      const f32x4 go = decode_center_bwd(jaccard_ref_bwd<false>(ac, gc, j, d_inter, -q), az, z);
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = go[k];
    }
    if (g_det_gt) {
      const float pm = (float)det_pos[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] -= g_det_gt[i * 4 + k] * pm;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) g_ro[i * 4 + k] = from_f32<T>(g[k]);
  }
}

// ---------------------------------------------------------------- softmax over K classes
template <typename T>
__global__ void softmax_kernel(const T* __restrict__ logits, float* __restrict__ probs, long rows, int K) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long)gridDim.x * blockDim.x) {
    float e[16], m, s;
    row_softmax(logits + r * K, K, e, m, s);
    for (int k = 0; k < K; ++k) probs[r * K + k] = e[k] / s;
  }
}

static int ew_grid(long n) { return (int)std::min<long>(cdivl(n, 256), 8192); }

// one grid-stride launch of 256-thread blocks over n items
template <typename... P, typename... A>
static void ew_launch(void (*kern)(P...), long n, void* stream, A... args) {
  hipLaunchKernelGGL(kern, dim3(ew_grid(n)), dim3(256), 0, ROD_STREAM(stream), args...);
}
// the tail of every entry here: launch(T{}) for the dtype code's storage type T, then the launch check
template <typename F>
static int ew_entry(const char* who, int dtype, F&& launch) {
  ROD_CHECK_ARG(sel_dtype(dtype, launch), "%s: unsupported dtype code %d", who, dtype);
  return check_launch(who);
}

}  // namespace rod

using namespace rod;

extern "C" {

int rod_resize_bilinear(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int dtype,
                        void* stream) {
  ROD_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0, "rod_resize_bilinear: bad shape");
  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;  // CalculateResizeScale, no align_corners
  const long n = (long)N * Ho * Wo * C;
  return ew_entry("rod_resize_bilinear", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(resize_fwd_kernel<T>, n, stream, (const T*)x, (T*)y, N, H, W, C, Ho, Wo, sy, sx);
  });
}

int rod_resize_bilinear_bwd(const void* dy, void* dx, int N, int H, int W, int C, int Ho, int Wo, int dtype,
                            void* stream) {
  ROD_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0, "rod_resize_bilinear_bwd: bad shape");
  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
  const long n = (long)N * H * W * C;
  return ew_entry("rod_resize_bilinear_bwd", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(resize_bwd_kernel<T>, n, stream, (const T*)dy, (T*)dx, N, H, W, C, Ho, Wo, sy, sx);
  });
}

int rod_depth_to_space2(const void* z, void* out, int N, int h, int w, int F, int Ho, int Wo, int ldo, int dtype,
                        void* stream) {
  ROD_CHECK_ARG(N > 0 && h > 0 && w > 0 && F > 0, "rod_depth_to_space2: bad shape");
  ROD_CHECK_ARG(Ho <= 2 * h && Wo <= 2 * w && Ho > 2 * h - 2 && Wo > 2 * w - 2, "rod_depth_to_space2: bad crop");
  if (ldo == 0) ldo = F;
  const long n = (long)N * Ho * Wo * F;
  return ew_entry("rod_depth_to_space2", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(d2s_kernel<T>, n, stream, (const T*)z, (T*)out, N, h, w, F, Ho, Wo, ldo);
  });
}

int rod_space_to_depth2(const void* dout, void* dz, int N, int h, int w, int F, int Ho, int Wo, int ldo, int dtype,
                        void* stream) {
  ROD_CHECK_ARG(N > 0 && h > 0 && w > 0 && F > 0, "rod_space_to_depth2: bad shape");
  ROD_CHECK_ARG(Ho <= 2 * h && Wo <= 2 * w, "rod_space_to_depth2: bad crop");
  if (ldo == 0) ldo = F;
  const long n = (long)N * h * w * 4 * F;
  return ew_entry("rod_space_to_depth2", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(s2d_kernel<T>, n, stream, (const T*)dout, (T*)dz, N, h, w, F, Ho, Wo, ldo);
  });
}

int rod_add(const void* a, const void* b, void* c, long n, int dtype, void* stream) {
  ROD_CHECK_ARG(n >= 0, "rod_add: n < 0");
  if (n == 0) return 0;
  return ew_entry("rod_add", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(add_kernel<T>, n, stream, (const T*)a, (const T*)b, (T*)c, n);
  });
}

int rod_decode(const float* anc_center, const void* off_a, const void* off_b, float* out, int B, int A, int to_corner,
               int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0, "rod_decode: bad shape");
  const long BA = (long)B * A;
  return ew_entry("rod_decode", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(decode_kernel<T>, BA, stream, anc_center, (const T*)off_a, (const T*)off_b, out, BA, A, to_corner);
  });
}

int rod_det_targets(const float* anc_center, const void* refine_out, const float* refine_gt, const float* cbox,
                    const int* label, const int* refine_pos, const int* lvl_off, const float* thr, int L,
                    float* det_gt, int* det_pos, int* det_lbl, float* iou, int B, int A, int dtype, void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0, "rod_det_targets: bad shape");
  ROD_CHECK_ARG(thr, "rod_det_targets: thr is a host array and must be given");
  Levels lv;
  if (int rc = fill_levels(lv, lvl_off, thr, L, A)) return rc;
  const long BA = (long)B * A;
  return ew_entry("rod_det_targets", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(det_targets_kernel<T>, BA, stream, anc_center, (const T*)refine_out, refine_gt, cbox, label, refine_pos,
              lv, det_gt, det_pos, det_lbl, iou, BA, A);
  });
}

int rod_det_targets_bwd(const float* anc_center, const void* refine_out, const float* cbox, const int* det_pos,
                        const float* g_det_gt, const float* g_iou, void* g_refine_out, int B, int A, int dtype,
                        void* stream) {
  ROD_CHECK_ARG(B > 0 && A > 0 && g_refine_out, "rod_det_targets_bwd: bad arguments");
  const long BA = (long)B * A;
  return ew_entry("rod_det_targets_bwd", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(det_targets_bwd_kernel<T>, BA, stream, anc_center, (const T*)refine_out, cbox, det_pos, g_det_gt, g_iou,
              (T*)g_refine_out, BA, A);
  });
}

int rod_softmax(const void* logits, float* probs, long rows, int K, int dtype, void* stream) {
  ROD_CHECK_ARG(rows >= 0 && K > 0 && K <= 16, "rod_softmax: bad shape (K <= 16)");
  if (rows == 0) return 0;
  return ew_entry("rod_softmax", dtype, [&](auto tt) {
    typedef decltype(tt) T;
    ew_launch(softmax_kernel<T>, rows, stream, (const T*)logits, probs, rows, K);
  });
}

}  // extern "C"
