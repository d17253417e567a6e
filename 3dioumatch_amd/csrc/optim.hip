// 3dioumatch_amd/csrc/optim.hip -- the optimizer step of the train scripts on one flat buffer.
//
// What it replaces: optimizer.step() of torch.optim.Adam(net.parameters(), lr, weight_decay)
// (pretrain.py:186 / :289, train.py:201 / :339) and, in the semi-supervised stage, the EMA update
// of the teacher that follows it (train.py:232-236 update_ema_variables).  The detector's
// parameters live in one flat buffer (votenet/step.py), so the whole update is one pass:
// read p, g, m, v (and the teacher), write p, m, v (and the teacher) -- 28 bytes per parameter
// instead of the ~15 element-wise kernels of the for-each implementation.
//
// The arithmetic is that of torch's Adam (no amsgrad, not maximize):
//     g'  = g * grad_scale + weight_decay * p          (g * grad_scale is also written back)
//     m   = m + (g' - m) * (1 - beta1);   v = beta2 * v + (1 - beta2) * g' * g'
//     p   = p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// with t = step + 1; the step counter and the learning rate are device scalars, so a captured
// HIP graph of this launch replays with the current values.
#include "common.h"
#include <math.h>

namespace {

// elements of the gradient one workgroup of adam_grad_sq_kernel sums: 256 lanes x 4 float4 loads
constexpr long long kGuardSpan = 4096;

// guarded entry, first launch: partials[b] = sum over the span b of ((double)(float)(g * grad_scale))^2.
// In-lane sums in element order, then a fixed-order tree over the 256 lanes: the grouping depends
// on n alone, no atomics, so two launches on equal inputs give equal bits.
__global__ void __launch_bounds__(256)
adam_grad_sq_kernel(long long n, const float *__restrict__ g, float grad_scale,
                    double *__restrict__ partials) {
  __shared__ double lanes[256];
  const long long base = (long long)blockIdx.x * kGuardSpan;
  double acc = 0.0;
  auto add = [&](float x) {
    const double d = (double)(x * grad_scale);
    acc += d * d;
  };
  for (int j = 0; j < 4; ++j) {
    const long long i4 = base + ((long long)j * 256 + threadIdx.x) * 4;
    if (i4 + 3 < n) {
      const float4 gg = *reinterpret_cast<const float4 *>(g + i4);
      add(gg.x); add(gg.y); add(gg.z); add(gg.w);
    } else {
      for (long long i = i4; i < n; ++i) add(g[i]);  // the tail: one lane, at most 3 elements
    }
  }
  lanes[threadIdx.x] = acc;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) lanes[threadIdx.x] += lanes[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = lanes[0];
}

// t = ++step, and the two scalars every parameter needs.  guard == NULL: one lane.  Guarded: one
// wave first adds the partial sums in a fixed order and lane 0 writes the verdict
// (guard[0] = gradient norm, [1] = clip coefficient, [2] = 1 if the step is skipped, [3] += [2]);
// a skipped step leaves step and scratch alone.
__global__ void __launch_bounds__(64)
adam_prepare_kernel(float *__restrict__ step, const float *__restrict__ lr, double beta1,
                    double beta2, float *__restrict__ scratch, const float *__restrict__ loss,
                    double max_norm, double *__restrict__ guard,
                    const double *__restrict__ partials, int nparts) {
  if (guard) {
    __shared__ double lanes[64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) acc += partials[i];
    lanes[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 32; half > 0; half >>= 1) {
      if ((int)threadIdx.x < half) lanes[threadIdx.x] += lanes[threadIdx.x + half];
      __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double s = lanes[0];
    // squares of finite floats cannot overflow this sum: s is non-finite exactly when an element is
    const bool ok = isfinite(s) && (loss == nullptr || isfinite(loss[0]));
    const double norm = sqrt(s);
    guard[0] = norm;
    guard[1] = max_norm > 0.0 ? fmin(1.0, max_norm / (norm + 1e-6)) : 1.0;  // clip_grad_norm_
    guard[2] = ok ? 0.0 : 1.0;
    guard[3] += ok ? 0.0 : 1.0;
    if (!ok) return;
  } else if (threadIdx.x != 0) {
    return;
  }
  const float t = step[0] + 1.f;
  step[0] = t;
  const double bc1 = 1.0 - pow(beta1, (double)t);
  const double bc2 = 1.0 - pow(beta2, (double)t);
  scratch[0] = (float)((double)lr[0] / bc1);  // step size
  scratch[1] = (float)sqrt(bc2);
}

// guard == NULL: the plain update.  Otherwise the verdict of adam_prepare_kernel: a skipped step
// writes nothing, an applied one uses (g * grad_scale) * clip.
__global__ void __launch_bounds__(256)
adam_update_kernel(long long n, float *__restrict__ p, float *__restrict__ g,
                   float *__restrict__ m, float *__restrict__ v,
                   const float *__restrict__ scratch, float beta1, float beta2, float one_m_beta1,
                   float one_m_beta2, float eps, float weight_decay, float grad_scale,
                   float *__restrict__ ema,
                   const float *__restrict__ ema_weight, const double *__restrict__ guard) {
  float clip = 1.f;
  if (guard) {
    if (guard[2] != 0.0) return;
    clip = (float)guard[1];
  }
  const float step_size = scratch[0], bc2_sqrt = scratch[1];
  const float w = ema ? ema_weight[0] : 0.f;
  const bool rewrite = grad_scale != 1.f || clip != 1.f;
  auto one = [&](float &pp, float &gg, float &mm, float &vv) {
    gg = (gg * grad_scale) * clip;  // (x * 1.f is x: clip == 1 is the unguarded arithmetic)
    float gd = gg;
    if (weight_decay != 0.f) gd = gd + weight_decay * pp;
    mm = mm + (gd - mm) * one_m_beta1;
    vv = beta2 * vv + (one_m_beta2 * gd) * gd;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp = pp - step_size * (mm / denom);
  };
  const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 + 3 < n) {
    float4 pp = *reinterpret_cast<float4 *>(p + i4);
    float4 gg = *reinterpret_cast<const float4 *>(g + i4);
    float4 mm = *reinterpret_cast<float4 *>(m + i4), vv = *reinterpret_cast<float4 *>(v + i4);
    one(pp.x, gg.x, mm.x, vv.x); one(pp.y, gg.y, mm.y, vv.y);
    one(pp.z, gg.z, mm.z, vv.z); one(pp.w, gg.w, mm.w, vv.w);
    if (rewrite)  // leave the mean behind where the sum was (p.grad of the modules)
      *reinterpret_cast<float4 *>(g + i4) = gg;
    *reinterpret_cast<float4 *>(p + i4) = pp;
    *reinterpret_cast<float4 *>(m + i4) = mm;
    *reinterpret_cast<float4 *>(v + i4) = vv;
    if (ema) {  // teacher <- teacher + (student - teacher) * (1 - alpha)
      float4 tt = *reinterpret_cast<float4 *>(ema + i4);
      tt.x = tt.x + w * (pp.x - tt.x); tt.y = tt.y + w * (pp.y - tt.y);
      tt.z = tt.z + w * (pp.z - tt.z); tt.w = tt.w + w * (pp.w - tt.w);
      *reinterpret_cast<float4 *>(ema + i4) = tt;
    }
  } else {
    for (long long i = i4; i < n; ++i) {
      float pp = p[i], gg = g[i], mm = m[i], vv = v[i];
      one(pp, gg, mm, vv);
      if (rewrite) g[i] = gg;
      p[i] = pp; m[i] = mm; v[i] = vv;
      if (ema) ema[i] = ema[i] + w * (pp - ema[i]);
    }
  }
}

// the launches of both entry points; guard == NULL: the unguarded pair
int adam_launch(long long n, float *p, float *g, float *m, float *v, float *step, const float *lr,
                double beta1, double beta2, double eps, double weight_decay, double grad_scale,
                float *ema, const float *ema_weight, float *scratch, const float *loss,
                double max_norm, double *guard, double *partials, hipStream_t stream) {
  const int nparts = guard ? pn2_ceil_div(n, kGuardSpan) : 0;
  if (guard)
    hipLaunchKernelGGL(adam_grad_sq_kernel, dim3((unsigned)nparts), dim3(256), 0, stream, n, g,
                       (float)grad_scale, partials);
  hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(guard ? 64 : 1), 0, stream, step, lr, beta1,
                     beta2, scratch, loss, max_norm, guard, partials, nparts);
  hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)pn2_ceil_div(n, 1024LL)), dim3(256), 0, stream, n,
                     p, g, m, v, scratch, (float)beta1, (float)beta2, (float)(1.0 - beta1),
                     (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)grad_scale, ema,
                     ema_weight, guard);
  return pn2_launch_status();
}

// Behind a guarded update: the verdict applied to the state a step writes OUTSIDE the update, in its
// forward passes (the BatchNorm buffers, one byte arena: votenet/step.py flatten_buffers).  Applied
// (guard[2] == 0): shadow <- state, the state is the last good one.  Skipped: state <- shadow.  Both
// directions in one kernel, so a captured launch serves either verdict.  One 16-byte load and one
// 16-byte store per lane; guard is only read.
__global__ void __launch_bounds__(256)
guard_state_sync_kernel(long long nvec, uint4 *state, uint4 *shadow, const double *__restrict__ guard) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const bool skipped = guard[2] != 0.0;
  const uint4 *src = skipped ? shadow : state;
  uint4 *dst = skipped ? state : shadow;
  dst[i] = src[i];
}

}  // namespace

// One Adam step on flat buffers of n floats (16-byte aligned); step (1 float, the count of steps
// taken so far; incremented), lr (1 float) and ema_weight (1 float, = 1 - alpha) live on the
// device; scratch: 2 floats.  ema == NULL: no teacher update.  The hyper-parameters arrive as
// doubles (Python floats): 1 - beta is rounded to fp32 once, as torch does.
PN2_API int votenet_adam_step(long long n, float *p, float *g, float *m, float *v, float *step,
                              const float *lr, double beta1, double beta2, double eps,
                              double weight_decay, double grad_scale, float *ema,
                              const float *ema_weight, float *scratch, void *stream_) {
  if (n <= 0) return 0;
  if (!p || !g || !m || !v || !step || !lr || !scratch || (ema && !ema_weight))
    return (int)hipErrorInvalidValue;
  return adam_launch(n, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale, ema,
                     ema_weight, scratch, nullptr, 0.0, nullptr, nullptr, (hipStream_t)stream_);
}

PN2_API int votenet_adam_guard_span(void) { return (int)kGuardSpan; }

PN2_API int votenet_adam_guard_partials(long long n) {
  return n <= 0 ? 0 : pn2_ceil_div(n, kGuardSpan);
}

// votenet_adam_step behind a device-side verdict: the step is applied only when every scaled
// gradient element and *loss (NULL: not looked at) are finite, with the gradient clipped to
// max_norm (<= 0: not clipped); otherwise nothing but guard is written.  guard: 4 doubles the caller
// zeroed once; partials: votenet_adam_guard_partials(n) doubles.  No host synchronisation.
PN2_API int votenet_adam_step_guarded(long long n, float *p, float *g, float *m, float *v,
                                      float *step, const float *lr, double beta1, double beta2,
                                      double eps, double weight_decay, double grad_scale, float *ema,
                                      const float *ema_weight, float *scratch, const float *loss,
                                      double max_norm, double *guard, double *partials,
                                      void *stream_) {
  if (n <= 0) return 0;
  if (!p || !g || !m || !v || !step || !lr || !scratch || (ema && !ema_weight) || !guard || !partials)
    return (int)hipErrorInvalidValue;
  return adam_launch(n, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale, ema,
                     ema_weight, scratch, loss, max_norm, guard, partials, (hipStream_t)stream_);
}

// The verdict of votenet_adam_step_guarded (guard[2], read on the device) applied to nbytes of state
// that the step's forward passes wrote: applied -> shadow <- state, skipped -> state <- shadow.  One
// launch on `stream`, behind the guarded update; nbytes a multiple of 16, both pointers 16-byte
// aligned, the two ranges disjoint.  guard is not written.
PN2_API int votenet_guard_state_sync(long long nbytes, void *state, void *shadow, const double *guard,
                                     void *stream_) {
  if (nbytes == 0) return 0;
  if (nbytes < 0 || nbytes % 16 != 0 || !state || !shadow || !guard ||
      (uintptr_t)state % 16 != 0 || (uintptr_t)shadow % 16 != 0)
    return (int)hipErrorInvalidValue;
  const long long nvec = nbytes / 16;
  const long long blocks = (nvec + 255) / 256;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(guard_state_sync_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream_, nvec, (uint4 *)state, (uint4 *)shadow, guard);
  return pn2_launch_status();
}
