// Frame activity on the device (contracts in include/sepr.h): the energy of every frame of every row, which frames of a
// row count as active, and what a channel emits in the frames of each class.
//
//   frame_energy_kernel   one wave per (row, frame): lane l adds the squares of the samples 4 q .. 4 q + 3 of the frame for q = l, l + 64, ... in
//                         ascending order from +0.0, in float64 (the square of a float32 value is exact in it), then the lanes by butterfly.  Four
//                         frames per workgroup, the rows on grid.y: one launch for all rows.  A frame whose first sample is 16-byte aligned is
//                         read with one float4 load per four samples that all lie below T, element by element otherwise - the same additions.
//   act_scan_kernel       one workgroup per row: the maximum of the row's energies (order-free: a zero of either sign counts as +0.0, a NaN is
//                         never taken), the threshold, then raw[f] = e[f] > thr counted into a prefix table cnt[f + 1] = #{f' <= f : raw[f']} in
//                         the workspace - 256 frames a step by ballot and popcount, the waves' counts through LDS, the carry in a register.
//   act_dilate_kernel     one thread per (row, frame): active = cnt[min(nF, f + hang + 1)] - cnt[max(0, f - hang)] > 0.
//   class_sums_kernel     one workgroup per (channel, class), written as segsnr_value_kernel of sepr_conversation.hip is: thread i takes the
//                         frames i, i + 256, ... in order and adds those of its class, a wave adds its lanes by butterfly, the four wave sums are
//                         kept in the workspace and added in wave order.  The two counts travel the same way: sums of ones are exact.
// No atomics; nothing depends on the launch order of workgroups: results are bit-identical from run to run.  The class table is device memory and a
// class byte is used as cls & 3, so it indexes nothing outside out.
#include <cmath>

#include "sepr_common.h"

namespace sepr {
namespace {
constexpr int FA_TPB = 256;
constexpr int FA_WAVES = FA_TPB / 64;
constexpr int FA_MAX_CH = 8;
constexpr int FA_MAX_FRAMES = 1 << 30;

template <bool VEC>
__global__ __launch_bounds__(FA_TPB) void frame_energy_kernel(const float* __restrict__ x, long long T, long long ld, int frame, long long nF,
                                                              double* __restrict__ e) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long long f = (long long)blockIdx.x * FA_WAVES + (threadIdx.x >> 6);
  if (f >= nF) return;                                             // the whole wave leaves; the kernel has no barrier
  const long long t0 = f * frame;
  const int n = T - t0 < frame ? (int)(T - t0) : frame;            // 1 .. frame valid samples: t0 < T because f < nF
  const float* __restrict__ p = x + (long long)blockIdx.y * ld + t0;
  double acc = 0.0;
  for (int i = 4 * lane; i < n; i += 256) {
    if (VEC && i + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      acc += (double)v.x * (double)v.x;
      acc += (double)v.y * (double)v.y;
      acc += (double)v.z * (double)v.z;
      acc += (double)v.w * (double)v.w;
    } else {
      for (int k = i; k < n && k < i + 4; ++k) acc += (double)p[k] * (double)p[k];
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) e[(long long)blockIdx.y * nF + f] = acc;
}

__device__ __forceinline__ double fa_max(double a, double b) { return b > a ? b : a; }      // a NaN b is never taken

__global__ __launch_bounds__(FA_TPB) void act_scan_kernel(const double* __restrict__ e, int nF, double ratio, double floor_,
                                                          double* __restrict__ level, int* __restrict__ cnt) {
#pragma clang fp contract(off)
  __shared__ double redm[FA_WAVES];
  __shared__ int redn[FA_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ er = e + (long long)blockIdx.x * nF;
  int* __restrict__ cr = cnt + (long long)blockIdx.x * ((long long)nF + 1);
  double m = -INFINITY;
  for (int f = tid; f < nF; f += FA_TPB) m = fa_max(m, er[f] + 0.0);          // -0.0 + 0.0 = +0.0: the maximum has one bit pattern
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fa_max(m, __shfl_xor(m, o, 64));
  if (lane == 0) redm[wave] = m;
  __syncthreads();
  m = fa_max(fa_max(fa_max(redm[0], redm[1]), redm[2]), redm[3]);
  const double t = m * ratio;
  const double thr = t > floor_ ? t : floor_;
  if (tid == 0) {
    level[blockIdx.x] = m;
    cr[0] = 0;
  }
  int carry = 0;
  for (int base = 0; base < nF; base += FA_TPB) {
    const int f = base + tid;
    const bool raw = f < nF && er[f] > thr;
    const unsigned long long b = __ballot(raw);
    const int incl = __popcll(b & ((1ull << lane) - 1ull)) + (raw ? 1 : 0);
    if (lane == 0) redn[wave] = __popcll(b);
    __syncthreads();
    const int w0 = redn[0], w1 = redn[1], w2 = redn[2], w3 = redn[3];
    if (f < nF) cr[f + 1] = carry + (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0) + incl;
    carry += w0 + w1 + w2 + w3;
    __syncthreads();                                               // redn is rewritten by the next step
  }
}

__global__ __launch_bounds__(FA_TPB) void act_dilate_kernel(const int* __restrict__ cnt, int nF, int hang, unsigned char* __restrict__ active) {
  const int f = blockIdx.x * FA_TPB + threadIdx.x;
  if (f >= nF) return;
  const int* __restrict__ cr = cnt + (long long)blockIdx.y * ((long long)nF + 1);
  const long long hi = (long long)f + hang + 1;
  const int lo = f > hang ? f - hang : 0;
  active[(long long)blockIdx.y * nF + f] = cr[hi < nF ? (int)hi : nF] - cr[lo] > 0 ? 1 : 0;
}

__global__ __launch_bounds__(FA_TPB) void class_sums_kernel(const double* __restrict__ e_est, const double* __restrict__ e_mix,
                                                            const unsigned char* __restrict__ active, const unsigned char* __restrict__ cls, int nF,
                                                            double* __restrict__ out, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4][FA_WAVES];
  const int c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const long long row = (long long)c * nF;
  double q[4] = {0.0, 0.0, 0.0, 0.0};                             // frames, active frames, sum e_est, sum e_mix
  for (int f = tid; f < nF; f += FA_TPB) {
    if ((cls[row + f] & 3) != k) continue;
    q[0] += 1.0;
    q[1] += active[row + f] ? 1.0 : 0.0;
    q[2] += e_est[row + f];
    q[3] += e_mix[f];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double s = wave_sum_d(q[j]);
    if ((tid & 63) == 0) red[j][tid >> 6] = s;
  }
  __syncthreads();
  if (tid < 4) {
    const long long o = ((long long)c * 4 + k) * 4 + tid;
    out[o] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
#pragma unroll
    for (int w = 0; w < FA_WAVES; ++w) part[o * FA_WAVES + w] = red[tid][w];
  }
}

struct ActLayout {
  int* cnt;                              // [rows][nF + 1]: raw-active frames before each frame
  ActLayout(Arena& a, int rows, int nF) { cnt = a.of<int>((size_t)rows * ((size_t)nF + 1)); }
};
struct ClsLayout {
  double* part;                          // [C][4][4][4]: the wave sums of every (channel, class, quantity), in wave order
  ClsLayout(Arena& a, int C) { part = a.f64((size_t)C * 4 * 4 * FA_WAVES); }
};
}  // namespace
}  // namespace sepr

extern "C" int sepr_frame_energy_fwd(const float* x, int rows, long long T, long long ld, int frame, double* e, sepr_stream_t stream) {
  using namespace sepr;
  if (!x || !e || rows < 1 || rows > 65535 || T < 1 || T > (1LL << 36) || ld < T) return SEPR_EINVAL;
  if (frame < 32 || frame > 4096 || frame % 4 != 0) return SEPR_EINVAL;
  if (reinterpret_cast<uintptr_t>(x) % 4 != 0 || reinterpret_cast<uintptr_t>(e) % 8 != 0) return SEPR_EINVAL;
  const long long nF = (T + frame - 1) / frame;
  const dim3 grid((unsigned)cdiv(nF, FA_WAVES), (unsigned)rows);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (reinterpret_cast<uintptr_t>(x) % 16 == 0 && ld % 4 == 0)      // every frame of every row starts on 16 bytes: frame is a multiple of 4
    hipLaunchKernelGGL(frame_energy_kernel<true>, grid, dim3(FA_TPB), 0, st, x, T, ld, frame, nF, e);
  else
    hipLaunchKernelGGL(frame_energy_kernel<false>, grid, dim3(FA_TPB), 0, st, x, T, ld, frame, nF, e);
  SEPR_CHECK_LAUNCH("frame energy kernel");
  return SEPR_OK;
}

extern "C" long long sepr_frame_activity_bytes(int rows, int nF) {
  using namespace sepr;
  if (rows < 1 || rows > 65535 || nF < 1 || nF > FA_MAX_FRAMES) return 0;
  return (long long)layout_bytes<ActLayout>(rows, nF);
}

extern "C" int sepr_frame_activity_fwd(const double* e, int rows, int nF, double ratio, double floor, int hang, unsigned char* active, double* level,
                                       void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!e || !active || !level || rows < 1 || rows > 65535 || nF < 1 || nF > FA_MAX_FRAMES || hang < 0) return SEPR_EINVAL;
  if (!(ratio >= 0.0 && std::isfinite(ratio)) || !(floor >= 0.0 && std::isfinite(floor))) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(level)) % 8 != 0) return SEPR_EINVAL;
  Arena arena(ws, ws_bytes);
  const ActLayout lay(arena, rows, nF);
  if (!arena.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(act_scan_kernel, dim3((unsigned)rows), dim3(FA_TPB), 0, st, e, nF, ratio, floor, level, lay.cnt);
  hipLaunchKernelGGL(act_dilate_kernel, dim3((unsigned)cdiv(nF, FA_TPB), (unsigned)rows), dim3(FA_TPB), 0, st, lay.cnt, nF, hang, active);
  SEPR_CHECK_LAUNCH("frame activity kernels");
  return SEPR_OK;
}

extern "C" long long sepr_frame_class_sums_bytes(int C, int nF) {
  using namespace sepr;
  if (C < 1 || C > FA_MAX_CH || nF < 1 || nF > FA_MAX_FRAMES) return 0;
  return (long long)layout_bytes<ClsLayout>(C);
}

extern "C" int sepr_frame_class_sums_fwd(const double* e_est, const double* e_mix, const unsigned char* active, const unsigned char* cls, int C,
                                         int nF, double* out, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!e_est || !e_mix || !active || !cls || !out || C < 1 || C > FA_MAX_CH || nF < 1 || nF > FA_MAX_FRAMES) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(e_est) | reinterpret_cast<uintptr_t>(e_mix) | reinterpret_cast<uintptr_t>(out)) % 8 != 0) return SEPR_EINVAL;
  Arena arena(ws, ws_bytes);
  const ClsLayout lay(arena, C);
  if (!arena.ok_need()) return SEPR_EWORKSPACE;
  hipLaunchKernelGGL(class_sums_kernel, dim3((unsigned)C, 4), dim3(FA_TPB), 0, static_cast<hipStream_t>(stream), e_est, e_mix, active, cls, nF,
                     out, lay.part);
  SEPR_CHECK_LAUNCH("frame class sums kernel");
  return SEPR_OK;
}
