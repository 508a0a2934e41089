// api.hip — error reporting, version, and small elementwise entry points.
#include <float.h>
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "rod_common.h"

namespace rod {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------- slab reduction
// block = CB columns x (256/CB) slab lanes; each lane keeps 4 independent f64 partials
// (4 loads in flight), then a fixed-order LDS combine.  CB is chosen so that short rows
// with many slabs (filter gradients: n = 9*C, thousands of parts) still fill the chip.
template <int CB>
__global__ void __launch_bounds__(256) slab_sum_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                       int nslab, long n) {
  constexpr int L = 256 / CB;
  __shared__ double red[L][CB + 1];
  const int tx = threadIdx.x % CB, ty = threadIdx.x / CB;
  const long i = (long)blockIdx.x * CB + tx;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (i < n) {
    int b = ty;
    for (; b + 3 * L < nslab; b += 4 * L) {
      s0 += (double)slab[(long)b * n + i];
      s1 += (double)slab[(long)(b + L) * n + i];
      s2 += (double)slab[(long)(b + 2 * L) * n + i];
      s3 += (double)slab[(long)(b + 3 * L) * n + i];
    }
    for (; b < nslab; b += L) s0 += (double)slab[(long)b * n + i];
  }
  red[ty][tx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ty == 0 && i < n) {
    double t = 0.0;
    for (int k = 0; k < L; ++k) t += red[k][tx];
    out[i] = (float)t;
  }
}

// Deferred slab sums (rod_slab_defer / rod_slab_flush).  A training step's parameter-gradient
// entries (conv / depthwise / fused-pointwise weight gradients, bias column sums) each end in a
// slab_sum of a few microseconds, ~115 launches per step whose only consumers are the optimizer
// and the data-parallel reducer.  While deferral is on, those sums are queued on the host and
// rod_slab_flush runs them as ONE batched launch per SLAB_BATCH jobs, each job with the exact
// block geometry and summation order of its own launch (bit-identical outputs).  The jobs are
// passed by value in the kernel arguments, so a flush is capturable in a HIP graph.
struct SlabJob {
  const float* slab;
  float* out;
  long n;
  int nslab;
  int cb;   // columns per block (4, 8 or 32): as slab_sum would have launched it
  int vec;  // 4: each thread sums 4 adjacent columns with 16-byte loads (n % 4 == 0, aligned slab)
};
constexpr int SLAB_BATCH = 32;
struct SlabBatch {
  SlabJob job[SLAB_BATCH];
  int first[SLAB_BATCH + 1];  // first block of each job; first[cnt] = grid size
  int cnt;
};

// vec == 4: a thread owns 4 adjacent columns (one 16-byte load per slab row instead of four
// 4-byte ones: 4x the bytes in flight per load instruction); every column keeps the thread row
// ty, the four chains and the block's ty-order combine of the scalar form (bit-identical sums)
__global__ void __launch_bounds__(256) slab_sum_batch_kernel(SlabBatch b) {
  __shared__ double red[1088];  // [L][VW * CB + 1] for L = 256 / CB, CB in {4, 8, 32}, VW in {1, 4}
  int e = 0;
  while (e + 1 < b.cnt && (int)blockIdx.x >= b.first[e + 1]) ++e;
  const SlabJob j = b.job[e];
  const int CB = j.cb, L = 256 / CB;
  const int tx = threadIdx.x % CB, ty = threadIdx.x / CB;
  if (j.vec == 4) {
    const int RW = 4 * CB + 1;
    const long i0 = (long)(blockIdx.x - b.first[e]) * CB * 4 + tx * 4;
    const long n = j.n;
    double s[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) s[c][v] = 0.0;
    if (i0 < n) {
      int k = ty;
      for (; k + 3 * L < j.nslab; k += 4 * L) {
        f32x4 a[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = *(const f32x4*)(j.slab + (long)(k + c * L) * n + i0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int v = 0; v < 4; ++v) s[c][v] += (double)a[c][v];
      }
      for (; k < j.nslab; k += L) {
        const f32x4 a = *(const f32x4*)(j.slab + (long)k * n + i0);
#pragma unroll
        for (int v = 0; v < 4; ++v) s[0][v] += (double)a[v];
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) red[ty * RW + tx * 4 + v] = (s[0][v] + s[1][v]) + (s[2][v] + s[3][v]);
    __syncthreads();
    if (ty == 0 && i0 < n) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        double t = 0.0;
        for (int k = 0; k < L; ++k) t += red[k * RW + tx * 4 + v];
        j.out[i0 + v] = (float)t;
      }
    }
    return;
  }
  const long i = (long)(blockIdx.x - b.first[e]) * CB + tx;
  const long n = j.n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (i < n) {
    int k = ty;
    for (; k + 3 * L < j.nslab; k += 4 * L) {
      s0 += (double)j.slab[(long)k * n + i];
      s1 += (double)j.slab[(long)(k + L) * n + i];
      s2 += (double)j.slab[(long)(k + 2 * L) * n + i];
      s3 += (double)j.slab[(long)(k + 3 * L) * n + i];
    }
    for (; k < j.nslab; k += L) s0 += (double)j.slab[(long)k * n + i];
  }
  red[ty * (CB + 1) + tx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ty == 0 && i < n) {
    double t = 0.0;
    for (int k = 0; k < L; ++k) t += red[k * (CB + 1) + tx];
    j.out[i] = (float)t;
  }
}

// process-wide, not thread-local: PyTorch runs the backward of custom autograd Functions on its
// per-device worker thread, not on the thread that calls rod_slab_defer / rod_slab_flush
static std::atomic<bool> g_slab_defer{false};
static std::mutex g_slab_mu;
static std::vector<SlabJob>* g_slab_jobs = nullptr;

int slab_cb(int nslab, long n) {
  if (n >= 256L * 32 || nslab <= 64) return 32;
  if (n >= 256L * 8) return 8;
  return 4;
}

void slab_sum(const float* slab, float* out, int nslab, long n, hipStream_t s, bool deferrable) {
  if (n <= 0) return;
  const int cb = slab_cb(nslab, n);
  if (deferrable && g_slab_defer.load()) {
    std::lock_guard<std::mutex> lk(g_slab_mu);
    if (!g_slab_jobs) g_slab_jobs = new std::vector<SlabJob>();
    const int vec = n % 4 == 0 && ((uintptr_t)slab & 15) == 0 ? 4 : 1;
    g_slab_jobs->push_back(SlabJob{slab, out, n, nslab, cb, vec});
    return;
  }
  if (cb == 32)
    hipLaunchKernelGGL(slab_sum_kernel<32>, dim3(cdivl(n, 32)), dim3(256), 0, s, slab, out, nslab, n);
  else if (cb == 8)
    hipLaunchKernelGGL(slab_sum_kernel<8>, dim3(cdivl(n, 8)), dim3(256), 0, s, slab, out, nslab, n);
  else
    hipLaunchKernelGGL(slab_sum_kernel<4>, dim3(cdivl(n, 4)), dim3(256), 0, s, slab, out, nslab, n);
}

int const_channel_blocks(int CV, long total, int target) {
  // smallest block count step s with (s*256) % CV == 0
  int g = CV, b = 256;
  while (b) { int t = g % b; g = b; b = t; }  // gcd(CV, 256)
  const int step = CV / g;
  long want = std::min<long>(target, cdivl(total, 256));
  long blocks = std::max<long>(1, cdivl(want, step)) * step;
  return (int)blocks;
}

// ---------------------------------------------------------------- kernels
template <typename T>
__global__ void normalize_image_kernel(const uint8_t* __restrict__ img, T* __restrict__ out, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const float k = 2.0f / 255.0f;  // (2.0 / 255.0) * imgs - 1.0, train.py:126 (f32 graph)
  if (i + 3 < n) {
    uchar4 v = *(const uchar4*)(img + i);
    out[i + 0] = from_f32<T>(k * (float)v.x - 1.0f);
    out[i + 1] = from_f32<T>(k * (float)v.y - 1.0f);
    out[i + 2] = from_f32<T>(k * (float)v.z - 1.0f);
    out[i + 3] = from_f32<T>(k * (float)v.w - 1.0f);
  } else {
    for (; i < n; ++i) out[i] = from_f32<T>(k * (float)img[i] - 1.0f);
  }
}

template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ src, D* __restrict__ dst, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = from_f32<D>(to_f32(src[i]));
}

// tf.clip_by_value = minimum(maximum(g, -clip), clip) with Eigen's scalar max/min
// (a < b ? b : a / b < a ? b : a): a NaN gradient stays NaN and poisons the variable, as in TF.
__device__ __forceinline__ float clip_tf(float g, float clip) {
  return g != g ? g : fminf(fmaxf(g, -clip), clip);
}

__global__ void sgd_clip_kernel(float* __restrict__ p, const float* __restrict__ g, long n, float lr,
                                float clip) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (; i < n; i += stride) {
    if (i + 3 < n) {
      f32x4 pv = *(f32x4*)(p + i);
      f32x4 gv = *(const f32x4*)(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float c = clip_tf(gv[j], clip);               // tf.clip_by_value
        pv[j] = pv[j] - lr * c;                       // ApplyGradientDescent: var -= alpha * delta
      }
      *(f32x4*)(p + i) = pv;
    } else {
      for (long k = i; k < n; ++k) p[k] = p[k] - lr * clip_tf(g[k], clip);
    }
  }
}

// ---- momentum SGD over the flat buffer (rod_sgd_momentum; the formula and its order are the
// contract in include/rod.h; -ffp-contract=off keeps every line one rounded operation).
// One thread per group of 4 elements per pass: one flag byte, three 16-byte loads, two 16-byte
// stores.  A group without ROD_OPT_TRAINABLE costs its flag byte only.
// EMA (rod_sgd_momentum_ema): the shadow e follows the p just written, e = e - rate * (e - p) in
// three rounded operations; one more 16-byte load and store per trainable group.  EMA = false
// never reads e or rate_p (both NULL there) and is the kernel rod_sgd_momentum always launched.
template <bool EMA>
__global__ void __launch_bounds__(256) sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ e,
                                                           const uint8_t* __restrict__ flags, long ngroups,
                                                           const float* __restrict__ lr_p,
                                                           const float* __restrict__ scale_p,
                                                           const float* __restrict__ rate_p, float mu, float wd,
                                                           float clip, int nesterov) {
  const float lr = *lr_p;
  const float scale = scale_p ? *scale_p : 1.0f;
  float rate = 0.0f;
  if constexpr (EMA) rate = *rate_p;
  long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; q < ngroups; q += stride) {
    const unsigned f = flags[q];
    if (!(f & ROD_OPT_TRAINABLE)) continue;
    const long i = q * 4;
    f32x4 pv = *(f32x4*)(p + i);
    const f32x4 gv = *(const f32x4*)(g + i);
    f32x4 mv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (m) mv = *(f32x4*)(m + i);
    f32x4 ev = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (EMA) ev = *(f32x4*)(e + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float d = gv[j];
      if (scale_p) d = d * scale;                    // global-norm clip (scale from rod_grad_sqnorm)
      d = clip_tf(d, clip);                          // tf.clip_by_value
      if (f & ROD_OPT_DECAY) d = d + wd * pv[j];
      const float mj = m ? mu * mv[j] + d : d;
      const float u = nesterov ? d + mu * mj : mj;
      pv[j] = pv[j] - lr * u;
      mv[j] = mj;
      if constexpr (EMA) {
        float t = ev[j] - pv[j];                       // tf.train.ExponentialMovingAverage:
        t = rate * t;                                  // variable -= (1 - decay) * (variable - value)
        ev[j] = ev[j] - t;
      }
    }
    *(f32x4*)(p + i) = pv;
    if (m) *(f32x4*)(m + i) = mv;
    if constexpr (EMA) *(f32x4*)(e + i) = ev;
  }
}

// ---- sum of squares of the trainable gradient (rod_grad_sqnorm): the partition is a function
// of n alone (stride SQN_PARTS * 256 groups whatever the grid), every sum has a fixed order.
constexpr int SQN_PARTS = 1024;

__device__ __forceinline__ float block_tree_sum(float v, float* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] = red[t] + red[t + w];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(256) grad_sqnorm_parts_kernel(const float* __restrict__ g,
                                                                const uint8_t* __restrict__ flags, long ngroups,
                                                                float* __restrict__ parts) {
  __shared__ float red[256];
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (long)SQN_PARTS * 256) {
    if (!(flags[q] & ROD_OPT_TRAINABLE)) continue;
    const f32x4 v = *(const f32x4*)(g + q * 4);
    s0 = s0 + v[0] * v[0];
    s1 = s1 + v[1] * v[1];
    s2 = s2 + v[2] * v[2];
    s3 = s3 + v[3] * v[3];
  }
  const float s = block_tree_sum((s0 + s1) + (s2 + s3), red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) grad_sqnorm_final_kernel(const float* __restrict__ parts, int nparts,
                                                                float clip_norm, float* __restrict__ scale) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  float a[SQN_PARTS / 256];
#pragma unroll
  for (int k = 0; k < SQN_PARTS / 256; ++k) a[k] = t + 256 * k < nparts ? parts[t + 256 * k] : 0.0f;
  static_assert(SQN_PARTS == 1024, "stage 2 pairs four parts per thread");
  const float s = block_tree_sum((a[0] + a[1]) + (a[2] + a[3]), red);
  if (t == 0) {
    const float norm = sqrtf(s);
    const float r = clip_norm / fmaxf(norm, FLT_MIN);
    // a NaN or Inf gradient poisons the update (fmaxf / fminf would drop the NaN)
    *scale = !(norm <= FLT_MAX) ? __builtin_nanf("") : (r < 1.0f ? r : 1.0f);
  }
}

}  // namespace rod

using namespace rod;

extern "C" {

int rod_abi_version(void) { return ROD_ABI_VERSION; }
const char* rod_last_error(void) { return rod::g_err; }

int rod_normalize_image(const void* img_u8, void* out, long n, int out_dtype, void* stream) {
  ROD_CHECK_ARG(n >= 0, "rod_normalize_image: n < 0");
  if (n == 0) return 0;
  ROD_CHECK_ARG(((uintptr_t)img_u8 & 3) == 0, "rod_normalize_image: input must be 4-byte aligned");
  int blocks = cdiv(cdivl(n, 4), 256);
  auto run = [&](auto tag) {
    typedef decltype(tag) T;
    hipLaunchKernelGGL(normalize_image_kernel<T>, dim3(blocks), dim3(256), 0, ROD_STREAM(stream),
                       (const uint8_t*)img_u8, (T*)out, n);
  };
  ROD_CHECK_ARG(sel_dtype(out_dtype, run), "rod_normalize_image: unsupported dtype code %d", out_dtype);
  return check_launch("rod_normalize_image");
}

int rod_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream) {
  ROD_CHECK_ARG(n >= 0, "rod_cast: n < 0");
  if (n == 0) return 0;
  int blocks = (int)std::min<long>(cdivl(n, 256), 8192);
  hipStream_t s = ROD_STREAM(stream);
  if (src_dtype == ROD_F32 && dst_dtype == ROD_BF16)
    hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3(blocks), dim3(256), 0, s, (const float*)src,
                       (bf16_t*)dst, n);
  else if (src_dtype == ROD_BF16 && dst_dtype == ROD_F32)
    hipLaunchKernelGGL((cast_kernel<bf16_t, float>), dim3(blocks), dim3(256), 0, s, (const bf16_t*)src,
                       (float*)dst, n);
  else if (src_dtype == ROD_F32 && dst_dtype == ROD_F32)
    hipLaunchKernelGGL((cast_kernel<float, float>), dim3(blocks), dim3(256), 0, s, (const float*)src,
                       (float*)dst, n);
  else if (src_dtype == ROD_BF16 && dst_dtype == ROD_BF16)
    hipLaunchKernelGGL((cast_kernel<bf16_t, bf16_t>), dim3(blocks), dim3(256), 0, s,
                       (const bf16_t*)src, (bf16_t*)dst, n);
  else {
    set_error("rod_cast: bad dtype pair %d -> %d", src_dtype, dst_dtype);
    return ROD_EINVAL;
  }
  return check_launch("rod_cast");
}

int rod_slab_defer(int on) { return g_slab_defer.exchange(on != 0) ? 1 : 0; }

int rod_slab_pending(void) {
  std::lock_guard<std::mutex> lk(g_slab_mu);
  return g_slab_jobs ? (int)g_slab_jobs->size() : 0;
}

static int slab_launch(std::vector<SlabJob>& jobs, hipStream_t s) {
  for (size_t k0 = 0; k0 < jobs.size(); k0 += SLAB_BATCH) {
    SlabBatch b{};
    b.cnt = (int)std::min<size_t>(SLAB_BATCH, jobs.size() - k0);
    long blocks = 0;
    for (int e = 0; e < b.cnt; ++e) {
      b.job[e] = jobs[k0 + e];
      b.first[e] = (int)blocks;
      blocks += cdivl(b.job[e].n, (long)b.job[e].cb * b.job[e].vec);
    }
    b.first[b.cnt] = (int)blocks;
    ROD_CHECK_ARG(blocks < (1L << 31), "rod_slab_flush: batch too large");
    hipLaunchKernelGGL(slab_sum_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, b);
    const int rc = check_launch("rod_slab_flush");
    if (rc) return rc;
  }
  return 0;
}

int rod_slab_flush(void* stream) {
  hipStream_t s = ROD_STREAM(stream);
  std::vector<SlabJob> jobs;
  {
    std::lock_guard<std::mutex> lk(g_slab_mu);
    if (!g_slab_jobs || g_slab_jobs->empty()) return 0;
    jobs.swap(*g_slab_jobs);
  }
  return slab_launch(jobs, s);
}

int rod_slab_flush_range(const void* lo, const void* hi, void* stream) {
  hipStream_t s = ROD_STREAM(stream);
  ROD_CHECK_ARG((const char*)lo <= (const char*)hi, "rod_slab_flush_range: lo > hi");
  std::vector<SlabJob> jobs;
  {
    std::lock_guard<std::mutex> lk(g_slab_mu);
    if (!g_slab_jobs || g_slab_jobs->empty()) return 0;
    std::vector<SlabJob> keep;
    for (const SlabJob& j : *g_slab_jobs) {
      const char* o = (const char*)j.out;
      const bool in = o >= (const char*)lo && o + j.n * sizeof(float) <= (const char*)hi;
      (in ? jobs : keep).push_back(j);
    }
    g_slab_jobs->swap(keep);
  }
  return jobs.empty() ? 0 : slab_launch(jobs, s);
}

int rod_sgd_clip(float* param, const float* grad, long n, float lr, float clip, void* stream) {
  ROD_CHECK_ARG(n >= 0, "rod_sgd_clip: n < 0");
  ROD_CHECK_ARG(((uintptr_t)param & 15) == 0 && ((uintptr_t)grad & 15) == 0,
                "rod_sgd_clip: buffers must be 16-byte aligned");
  if (n == 0) return 0;
  int blocks = (int)std::min<long>(cdivl(cdivl(n, 4), 256), 4096);
  hipLaunchKernelGGL(sgd_clip_kernel, dim3(blocks), dim3(256), 0, ROD_STREAM(stream), param, grad, n,
                     lr, clip);
  return check_launch("rod_sgd_clip");
}

size_t rod_grad_sqnorm_workspace(void) { return SQN_PARTS * sizeof(float); }

int rod_grad_sqnorm(const float* grad, const unsigned char* flags, long n, float clip_norm, float* scale,
                    void* workspace, void* stream) {
  ROD_CHECK_ARG(n >= 0 && n % 4 == 0, "rod_grad_sqnorm: n must be a non-negative multiple of 4");
  ROD_CHECK_ARG(((uintptr_t)grad & 15) == 0, "rod_grad_sqnorm: grad must be 16-byte aligned");
  ROD_CHECK_ARG(clip_norm > 0.0f, "rod_grad_sqnorm: clip_norm must be > 0");
  ROD_CHECK_ARG(scale != nullptr && workspace != nullptr && ((uintptr_t)workspace & 3) == 0,
                "rod_grad_sqnorm: scale and a 4-byte aligned workspace are required");
  ROD_CHECK_ARG(n == 0 || (grad != nullptr && flags != nullptr), "rod_grad_sqnorm: grad and flags are required");
  hipStream_t s = ROD_STREAM(stream);
  const long ngroups = n / 4;
  const int nparts = (int)std::min<long>(cdivl(ngroups, 256), SQN_PARTS);
  if (nparts > 0) {
    hipLaunchKernelGGL(grad_sqnorm_parts_kernel, dim3(nparts), dim3(256), 0, s, grad, (const uint8_t*)flags,
                       ngroups, (float*)workspace);
    const int rc = check_launch("rod_grad_sqnorm");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, nparts,
                     clip_norm, scale);
  return check_launch("rod_grad_sqnorm");
}

int rod_sgd_momentum(float* param, const float* grad, float* mom, const unsigned char* flags, long n,
                     const float* lr, const float* scale, float mu, float wd, float clip, int nesterov,
                     void* stream) {
  ROD_CHECK_ARG(n >= 0 && n % 4 == 0, "rod_sgd_momentum: n must be a non-negative multiple of 4");
  ROD_CHECK_ARG(((uintptr_t)param & 15) == 0 && ((uintptr_t)grad & 15) == 0 && ((uintptr_t)mom & 15) == 0,
                "rod_sgd_momentum: buffers must be 16-byte aligned");
  ROD_CHECK_ARG(lr != nullptr, "rod_sgd_momentum: lr (device pointer) is required");
  ROD_CHECK_ARG(mom != nullptr || mu == 0.0f, "rod_sgd_momentum: mu != 0 needs the momentum buffer");
  ROD_CHECK_ARG(!(clip < 0.0f) && clip == clip, "rod_sgd_momentum: clip must be >= 0 (+inf disables it)");
  if (n == 0) return 0;
  ROD_CHECK_ARG(param != nullptr && grad != nullptr && flags != nullptr,
                "rod_sgd_momentum: param, grad and flags are required");
  const long ngroups = n / 4;
  int blocks = (int)std::min<long>(cdivl(ngroups, 256), 4096);
  hipLaunchKernelGGL(sgd_momentum_kernel<false>, dim3(blocks), dim3(256), 0, ROD_STREAM(stream), param, grad, mom,
                     (float*)nullptr, (const uint8_t*)flags, ngroups, lr, scale, (const float*)nullptr, mu, wd, clip,
                     nesterov);
  return check_launch("rod_sgd_momentum");
}

int rod_sgd_momentum_ema(float* param, const float* grad, float* mom, float* ema, const unsigned char* flags,
                         long n, const float* lr, const float* scale, const float* ema_rate, float mu, float wd,
                         float clip, int nesterov, void* stream) {
  ROD_CHECK_ARG(n >= 0 && n % 4 == 0, "rod_sgd_momentum_ema: n must be a non-negative multiple of 4");
  ROD_CHECK_ARG(((uintptr_t)param & 15) == 0 && ((uintptr_t)grad & 15) == 0 && ((uintptr_t)mom & 15) == 0 &&
                    ((uintptr_t)ema & 15) == 0,
                "rod_sgd_momentum_ema: buffers must be 16-byte aligned");
  ROD_CHECK_ARG(ema != nullptr && ema_rate != nullptr,
                "rod_sgd_momentum_ema: ema and ema_rate (device pointer) are required");
  ROD_CHECK_ARG(lr != nullptr, "rod_sgd_momentum_ema: lr (device pointer) is required");
  ROD_CHECK_ARG(mom != nullptr || mu == 0.0f, "rod_sgd_momentum_ema: mu != 0 needs the momentum buffer");
  ROD_CHECK_ARG(!(clip < 0.0f) && clip == clip, "rod_sgd_momentum_ema: clip must be >= 0 (+inf disables it)");
  if (n == 0) return 0;
  ROD_CHECK_ARG(param != nullptr && grad != nullptr && flags != nullptr,
                "rod_sgd_momentum_ema: param, grad and flags are required");
  const long ngroups = n / 4;
  int blocks = (int)std::min<long>(cdivl(ngroups, 256), 4096);
  hipLaunchKernelGGL(sgd_momentum_kernel<true>, dim3(blocks), dim3(256), 0, ROD_STREAM(stream), param, grad, mom,
                     ema, (const uint8_t*)flags, ngroups, lr, scale, ema_rate, mu, wd, clip, nesterov);
  return check_launch("rod_sgd_momentum_ema");
}

}  // extern "C"
