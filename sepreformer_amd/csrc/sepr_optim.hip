// Optimizer step of the reference training loop (engine.py:76-77: clip_grad_norm_(max_norm) + AdamW.step) as THREE launches over
// the whole model, whatever its number of parameter tensors (Base: 1 312):
//   opt_sqsum_kernel   sum of squares of the flat gradient buffer, 1 024 block partials in double (fixed order, no atomics)
//   opt_prep_kernel    one block: total norm, clip coefficient, step counter += 1, the bias corrections of this step
//   opt_adamw_kernel   one block per 1 024 elements of one tensor (block table), decoupled weight decay + Adam update
// sepr_adamw_step_guarded is the same three launches with one difference: a non-finite total norm skips the step (scal[5] = 1, the
// counter, parameters and moments untouched) instead of poisoning the weights; with a finite norm its arithmetic is sepr_adamw_step's.
// The prepare and the update kernel are templates on the guard: sepr_adamw_step launches the <false, false> instantiations, whose code is
// what the two kernels compiled to before the guard existed.
// sepr_adamw_step_ema is the guarded step that also keeps an exponential moving average of the parameters (the second template
// argument): the prepare kernel leaves 1 - d_t in scal[6], the update kernel folds the parameter value it has just stored into the
// flat `ema` buffer (36 bytes per parameter instead of 28).  sepr_adamw_swap exchanges the parameters with such a buffer, bitwise.
// run_ledger_kernel folds a step's loss parts and optimizer scalars into the float64 run ledger the training loop reads once per
// log interval (no per-step host synchronisation).
// torch's route is one multi_tensor_apply launch per ~36 tensors (37 launches for the update, 12 for the norms, 37 for the clip
// scaling: 1.8 ms per step at 14.7 M parameters = 260 GB/s); these three stream the 14.7 M x 28 bytes once (~0.15 ms).
// Arithmetic = torch's fused AdamW (fused_adam_utils.cuh adam_math, decoupled weight decay): fp32 per element, the bias corrections
// from pow() in double; the clip coefficient is min(1, max_norm / (norm + 1e-6)) applied to the gradient inside the update.
#include "sepr_common.h"
#include <math.h>

namespace sepr {
namespace {
constexpr int OPT_TPB = 256;
constexpr int OPT_BLOCK = 1024;       // elements per block of the update kernel (one float4 per thread)
constexpr int OPT_PARTS = 1024;       // block partials of the norm

__global__ __launch_bounds__(OPT_TPB) void opt_sqsum_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
  __shared__ double sh[OPT_TPB / 64];
  // block b owns the contiguous range [b * per, (b + 1) * per): the partial of a block does not depend on the grid
  const long long per = ((n + OPT_PARTS - 1) / OPT_PARTS + 3) / 4 * 4;
  const long long beg = (long long)blockIdx.x * per;
  const long long end = beg + per < n ? beg + per : n;
  double acc = 0.0;
  for (long long i = beg + 4LL * threadIdx.x; i < end; i += 4LL * OPT_TPB) {
    if (i + 3 < end) {
      const float4 v = ld4(g + i);
      acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    } else {
      for (long long j = i; j < end; ++j) acc += (double)g[j] * g[j];
    }
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// scal[0] = total norm, [1] = clip coefficient, [2] = lr / bias_correction1, [3] = sqrt(bias_correction2), [4] = lr * weight_decay,
// [5] (guard only) = 1 when the step is skipped for a non-finite total norm, else 0, [6] (EMA only) = 1 - d_t, the weight of the new
// parameter value in the moving average of this step
__device__ __forceinline__ bool opt_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

template <bool GUARD, bool EMA>
__global__ __launch_bounds__(OPT_TPB) void opt_prep_kernel(const double* __restrict__ part, int with_norm, float max_norm, const float* __restrict__ lr,
                                                          double beta1, double beta2, float weight_decay, double* __restrict__ step,
                                                          float* __restrict__ scal, double ema_decay, double ema_warmup) {
  __shared__ double sh[OPT_TPB];
  double acc = 0.0;
  if (with_norm)
    for (int i = threadIdx.x; i < OPT_PARTS; i += OPT_TPB) acc += part[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = OPT_TPB / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(sh[0]);
  if (GUARD) {
    // sepr_adamw_step_guarded: a non-finite total norm skips the step - the counter stays, the update kernel returns on scal[5]
    const bool bad = opt_nonfinite(norm);
    scal[5] = bad ? 1.0f : 0.0f;
    if (bad) {
      scal[0] = norm;
      return;
    }
  }
  float clip = 1.0f;
  if (with_norm && max_norm > 0.f) {
    clip = max_norm / (norm + 1e-6f);
    // torch.clamp(max = 1) semantics of clip_grad_norm_: a non-finite norm gives a NaN coefficient that reaches EVERY gradient element
    // (the step then poisons the weights visibly, as with torch, instead of applying the finite elements unclipped)
    clip = !(clip >= 1.0f) ? clip : 1.0f;
  }
  const double t = *step + 1.0;
  *step = t;
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  const float l = *lr;
  scal[0] = norm;
  scal[1] = clip;
  scal[2] = (float)((double)l / bc1);
  scal[3] = (float)sqrt(bc2);
  scal[4] = l * weight_decay;
  if (EMA) {
    // the decay of step t: ema_decay, ramped in as (1 + t) / (warmup + t) while that is smaller (trainer.ema_decay_at states it on the host)
    double d = ema_decay;
    if (ema_warmup > 0.0) {
      const double r = (1.0 + t) / (ema_warmup + t);
      d = r < d ? r : d;
    }
    scal[6] = (float)(1.0 - d);
  }
}

struct OptTables {
  float* const* params;           // [ntensors]
  const long long* grad_off;      // [ntensors] element offset of the tensor's gradient in the flat gradient buffer
  const long long* state_off;     // [ntensors] element offset of its moments in exp_avg / exp_avg_sq
  const int* numel;               // [ntensors]
  const int2* blocks;             // [nblocks] (tensor, first element)
};

template <bool GUARD, bool EMA>
__global__ __launch_bounds__(OPT_TPB) void opt_adamw_kernel(const OptTables t, const float* __restrict__ grads, float* __restrict__ exp_avg,
                                                           float* __restrict__ exp_avg_sq, const float* __restrict__ scal, float omb1,
                                                           float beta2, float omb2, float eps, float* __restrict__ ema) {
#pragma clang fp contract(off)
  if (GUARD && scal[5] != 0.0f) return;                       // skipped step: parameters and moments stay as they are
  const int2 b = t.blocks[blockIdx.x];
  const int ti = b.x;
  const int n = t.numel[ti];
  const int e0 = b.y + 4 * threadIdx.x;
  if (e0 >= n) return;
  float* __restrict__ p = t.params[ti] + e0;
  const float* __restrict__ g = grads + t.grad_off[ti] + e0;
  const long long so = t.state_off[ti] + e0;
  const float clip = scal[1], step_size = scal[2], bc2_sqrt = scal[3], lr_wd = scal[4];
  const int cnt = n - e0 < 4 ? n - e0 : 4;
  float pv[4], gv[4], mv[4], vv[4];
  if (cnt == 4) {       // every slice starts 16-byte aligned (parameter allocations, 64-element gradient and state slots)
    const float4 p4 = ld4(p), g4 = ld4(g), m4 = ld4(exp_avg + so), v4 = ld4(exp_avg_sq + so);
    pv[0] = p4.x; pv[1] = p4.y; pv[2] = p4.z; pv[3] = p4.w;
    gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
    mv[0] = m4.x; mv[1] = m4.y; mv[2] = m4.z; mv[3] = m4.w;
    vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
  } else {
    for (int e = 0; e < cnt; ++e) { pv[e] = p[e]; gv[e] = g[e]; mv[e] = exp_avg[so + e]; vv[e] = exp_avg_sq[so + e]; }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e >= cnt) break;
    const float gr = gv[e] * clip;
    float pr = pv[e];
    pr -= lr_wd * pr;                                         // decoupled weight decay
    const float m = mv[e] + omb1 * (gr - mv[e]);              // lerp(exp_avg, grad, 1 - beta1)
    const float v = beta2 * vv[e] + omb2 * gr * gr;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    pr -= step_size * m / denom;
    pv[e] = pr; mv[e] = m; vv[e] = v;
  }
  if (cnt == 4) {
    st4(p, make_float4(pv[0], pv[1], pv[2], pv[3]));
    st4(exp_avg + so, make_float4(mv[0], mv[1], mv[2], mv[3]));
    st4(exp_avg_sq + so, make_float4(vv[0], vv[1], vv[2], vv[3]));
  } else {
    for (int e = 0; e < cnt; ++e) { p[e] = pv[e]; exp_avg[so + e] = mv[e]; exp_avg_sq[so + e] = vv[e]; }
  }
  if (EMA) {
    // e += (1 - d_t) (p - e) with p the value stored above, from its register: three rounded operations (no contraction in this kernel)
    const float w = scal[6];
    float* __restrict__ ea = ema + so;
    if (cnt == 4) {
      float4 e4 = ld4(ea);
      e4.x = e4.x + w * (pv[0] - e4.x);
      e4.y = e4.y + w * (pv[1] - e4.y);
      e4.z = e4.z + w * (pv[2] - e4.z);
      e4.w = e4.w + w * (pv[3] - e4.w);
      st4(ea, e4);
    } else {
      for (int e = 0; e < cnt; ++e) {
        const float ev = ea[e];
        ea[e] = ev + w * (pv[e] - ev);
      }
    }
  }
}

// sepr_adamw_swap: one block per 1 024 elements of one tensor, over the update's block table; parameter and shadow slot trade places
__global__ __launch_bounds__(OPT_TPB) void opt_swap_kernel(const OptTables t, float* __restrict__ shadow) {
  const int2 b = t.blocks[blockIdx.x];
  const int ti = b.x;
  const int n = t.numel[ti];
  const int e0 = b.y + 4 * threadIdx.x;
  if (e0 >= n) return;
  float* __restrict__ p = t.params[ti] + e0;
  float* __restrict__ q = shadow + t.state_off[ti] + e0;
  if (n - e0 >= 4) {
    const float4 a = ld4(p), c = ld4(q);
    st4(p, c);
    st4(q, a);
  } else {
    for (int e = 0; e < n - e0; ++e) {
      const float a = p[e];
      p[e] = q[e];
      q[e] = a;
    }
  }
}

// Run ledger (include/sepr.h SEPR_LEDGER_*): one thread folds one step into float64 slots, in fixed order, with plain stores.
__global__ void run_ledger_kernel(const float* __restrict__ parts, int nparts, const float* __restrict__ scal, double* __restrict__ led) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (scal && scal[5] != 0.0f) {
    led[SEPR_LEDGER_SKIPPED] += 1.0;
    return;
  }
  led[SEPR_LEDGER_STEPS] += 1.0;
  bool bad = false;
  for (int i = 0; i < nparts; ++i) {
    const float v = parts[i];
    bad |= opt_nonfinite(v);
    led[SEPR_LEDGER_PART_SUM + i] += (double)v;
    led[SEPR_LEDGER_PART_SUM + nparts + i] = (double)v;       // the last step's parts
  }
  if (bad) led[SEPR_LEDGER_NONFINITE] += 1.0;
  if (scal) {
    const double gn = (double)scal[0];
    led[SEPR_LEDGER_GNORM_SUM] += gn;
    if (gn > led[SEPR_LEDGER_GNORM_MAX]) led[SEPR_LEDGER_GNORM_MAX] = gn;
    if (scal[1] < 1.0f) led[SEPR_LEDGER_CLIPPED] += 1.0;
  }
}
}  // namespace
}  // namespace sepr

using namespace sepr;

extern "C" int sepr_adamw_block_elems(void) { return OPT_BLOCK; }
extern "C" size_t sepr_adamw_workspace(void) { return OPT_PARTS * sizeof(double); }

static int adamw_step_impl(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                           double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                           float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream, bool guard, float* ema = nullptr,
                           double ema_decay = 0.0, double ema_warmup = 0.0) {
  if (!t || !t->params || !t->grad_off || !t->state_off || !t->numel || !t->blocks || t->nblocks <= 0 || !grads || grads_numel <= 0 ||
      !exp_avg || !exp_avg_sq || !step || !lr || !scal)
    return SEPR_EINVAL;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(grads) & 15) || (reinterpret_cast<uintptr_t>(exp_avg) & 15) || (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15))
    return SEPR_EINVAL;
  if (ema && (!guard || (reinterpret_cast<uintptr_t>(ema) & 15) || !(ema_decay >= 0.0 && ema_decay < 1.0))) return SEPR_EINVAL;
  const int with_norm = (guard || max_norm > 0.0) ? 1 : 0;      // the guard judges the total norm, so it always runs the norm pass
  if (with_norm && (!ws || ws_bytes < sepr_adamw_workspace())) return SEPR_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(ws);
  if (with_norm) hipLaunchKernelGGL(opt_sqsum_kernel, dim3(OPT_PARTS), dim3(OPT_TPB), 0, s, grads, grads_numel, part);
  const float wd = (float)weight_decay;
  if (ema)
    hipLaunchKernelGGL((opt_prep_kernel<true, true>), dim3(1), dim3(OPT_TPB), 0, s, part, with_norm, (float)max_norm, lr, beta1, beta2, wd, step, scal, ema_decay, ema_warmup);
  else if (guard)
    hipLaunchKernelGGL((opt_prep_kernel<true, false>), dim3(1), dim3(OPT_TPB), 0, s, part, with_norm, (float)max_norm, lr, beta1, beta2, wd, step, scal, 0.0, 0.0);
  else
    hipLaunchKernelGGL((opt_prep_kernel<false, false>), dim3(1), dim3(OPT_TPB), 0, s, part, with_norm, (float)max_norm, lr, beta1, beta2, wd, step, scal, 0.0, 0.0);
  OptTables k;
  k.params = t->params; k.grad_off = t->grad_off; k.state_off = t->state_off; k.numel = t->numel;
  k.blocks = reinterpret_cast<const int2*>(t->blocks);
  float* const no_ema = nullptr;
  if (ema)
    hipLaunchKernelGGL((opt_adamw_kernel<true, true>), dim3(t->nblocks), dim3(OPT_TPB), 0, s, k, grads, exp_avg, exp_avg_sq, scal, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, ema);
  else if (guard)
    hipLaunchKernelGGL((opt_adamw_kernel<true, false>), dim3(t->nblocks), dim3(OPT_TPB), 0, s, k, grads, exp_avg, exp_avg_sq, scal, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, no_ema);
  else
    hipLaunchKernelGGL((opt_adamw_kernel<false, false>), dim3(t->nblocks), dim3(OPT_TPB), 0, s, k, grads, exp_avg, exp_avg_sq, scal, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, no_ema);
  SEPR_CHECK_LAUNCH("adamw step kernels");
  return SEPR_OK;
}

extern "C" int sepr_adamw_step(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                               double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                               float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  return adamw_step_impl(t, grads, grads_numel, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, max_norm, scal, ws, ws_bytes, stream, false);
}

extern "C" int sepr_adamw_step_guarded(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                                       double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                       float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  return adamw_step_impl(t, grads, grads_numel, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, max_norm, scal, ws, ws_bytes, stream, true);
}

extern "C" int sepr_adamw_step_ema(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                                   double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                   float* ema, double ema_decay, double ema_warmup, float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  if (!ema) return SEPR_EINVAL;
  return adamw_step_impl(t, grads, grads_numel, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, max_norm, scal, ws, ws_bytes, stream, true,
                         ema, ema_decay, ema_warmup);
}

extern "C" int sepr_adamw_swap(const sepr_adamw_tables* t, float* shadow, sepr_stream_t stream) {
  if (!t || !t->params || !t->state_off || !t->numel || !t->blocks || t->nblocks <= 0 || !shadow) return SEPR_EINVAL;
  if (reinterpret_cast<uintptr_t>(shadow) & 15) return SEPR_EINVAL;
  OptTables k;
  k.params = t->params; k.grad_off = t->grad_off; k.state_off = t->state_off; k.numel = t->numel;
  k.blocks = reinterpret_cast<const int2*>(t->blocks);
  hipLaunchKernelGGL(opt_swap_kernel, dim3(t->nblocks), dim3(OPT_TPB), 0, static_cast<hipStream_t>(stream), k, shadow);
  SEPR_CHECK_LAUNCH("adamw swap kernel");
  return SEPR_OK;
}

extern "C" int sepr_run_ledger_doubles(int nparts) { return nparts >= 1 && nparts <= SEPR_LEDGER_MAX_PARTS ? SEPR_LEDGER_PART_SUM + 2 * nparts : 0; }

extern "C" int sepr_run_ledger_update(const float* parts, int nparts, const float* opt_scal, double* ledger, int ledger_doubles,
                                      sepr_stream_t stream) {
  if (!parts || !ledger || nparts < 1 || nparts > SEPR_LEDGER_MAX_PARTS || ledger_doubles < sepr_run_ledger_doubles(nparts)) return SEPR_EINVAL;
  if (reinterpret_cast<uintptr_t>(ledger) & 7) return SEPR_EINVAL;
  hipLaunchKernelGGL(run_ledger_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), parts, nparts, opt_scal, ledger);
  SEPR_CHECK_LAUNCH("run ledger kernel");
  return SEPR_OK;
}
