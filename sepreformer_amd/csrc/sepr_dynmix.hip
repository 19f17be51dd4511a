// Dynamic mixing from a device-resident corpus: the training batch of the reference's *_DM_* data sets
// (models/SepReformer_Large_DM_*/dataset.py::_dynamic_mixing + _collate) built by ONE launch from a plan table.
//
// The corpus is two contiguous buffers - int16 utterances (PCM16 files as they are on disk) and float32 utterances - with one
// int64 table of cumulative element counts: utterance u < N16 is buf16[off[u] .. off[u + 1]), utterance u >= N16 is
// buf32[off[u] - off[N16] .. off[u + 1] - off[N16]).
//   energy_part_kernel / energy_finish_kernel   sum of squares per utterance, once at load: int64 for int16 utterances (exact, so
//                        independent of the order), float64 in a fixed order for float32 utterances; per-workgroup partials and a
//                        finishing pass, no atomics;
//   dynmix_kernel        one thread per eight output samples of one example: every term is eight consecutive samples from an
//                        arbitrary start, read as aligned 16-byte loads from the aligned-down address and realigned in registers
//                        (v_alignbyte for the odd int16 starts), scaled by two separately rounded multiplies, summed in term
//                        order; float4 stores of the mixture and the S target rows, zeros from n[b] on.
// Nothing here depends on the launch order of workgroups: results are bit-identical from run to run.
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr int DM_TPB = 256;        // threads per workgroup of the mixing kernel
constexpr int DM_PER = 8;          // output samples per thread
constexpr int EN_TPB = 256;        // threads per workgroup of the energy kernel = samples per chunk
constexpr int EN_PARTS = 8;        // workgroups (partials) per utterance: workgroup p takes the chunks c = p, p + 8, ...

struct DmRows {
  float* p[3];
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint4 ldu4(const void* p) { return *reinterpret_cast<const uint4*>(p); }

// eight consecutive int16 samples from element e (any parity) of buf as floats s * 2^-15 (exact).  Two aligned 16-byte loads at
// the aligned-down element e & ~7; pad = the buffer's element count rounded up to 8 (allocated), so no load leaves the buffer.
__device__ __forceinline__ void load8_i16(const short* __restrict__ buf, long long e, long long pad, float out[8]) {
  const long long a0 = e & ~7LL;
  const uint4 lo = ldu4(buf + a0);
  const uint4 hi = a0 + 8 < pad ? ldu4(buf + a0 + 8) : make_uint4(0u, 0u, 0u, 0u);
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const int sh = (int)(e & 7), ds = sh >> 1;
  unsigned u[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) u[k] = ds == 0 ? w[k] : (ds == 1 ? w[k + 1] : (ds == 2 ? w[k + 2] : w[k + 3]));
  const bool odd = sh & 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned d = odd ? __builtin_amdgcn_alignbyte(u[k + 1], u[k], 2) : u[k];
    out[2 * k] = (float)(short)(d & 0xffffu) * 3.0517578125e-05f;
    out[2 * k + 1] = (float)((int)d >> 16) * 3.0517578125e-05f;
  }
}

// eight consecutive float32 samples from element e (any) of buf: three aligned 16-byte loads at e & ~3; pad = the element count
// rounded up to 4.
__device__ __forceinline__ void load8_f32(const float* __restrict__ buf, long long e, long long pad, float out[8]) {
  const long long a0 = e & ~3LL;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 q0 = ldu4(buf + a0);
  const uint4 q1 = a0 + 4 < pad ? ldu4(buf + a0 + 4) : z;
  const uint4 q2 = a0 + 8 < pad ? ldu4(buf + a0 + 8) : z;
  const unsigned w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
  const int sh = (int)(e & 3);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = __uint_as_float(sh == 0 ? w[k] : (sh == 1 ? w[k + 1] : (sh == 2 ? w[k + 2] : w[k + 3])));
}

struct DmCorpus {
  const short* buf16;
  const float* buf32;
  const long long* off;
  long long total16, total32;
  int N16, N;
};

// (sample * norm) * gain of term j of the example on samples t0 .. t0 + 7.  The table is not trusted: the utterance index, the start
// and the element position are clamped, so whatever it holds no read leaves the corpus buffers.
__device__ __forceinline__ void term_value(const DmCorpus& c, int utt, int start, float norm, float gain, int t0, float v[8]) {
#pragma clang fp contract(off)
  const int u = utt < 0 ? 0 : (utt >= c.N ? c.N - 1 : utt);
  const long long o0 = c.off[u], len = c.off[u + 1] - o0;
  const long long st = clampll(start, 0, len > 0 ? len : 0);
  float x[8];
  if (u < c.N16) {
    load8_i16(c.buf16, clampll(o0 + st + t0, 0, c.total16 - 1), (c.total16 + 7) & ~7LL, x);
  } else {
    load8_f32(c.buf32, clampll(o0 - c.off[c.N16] + st + t0, 0, c.total32 - 1), (c.total32 + 3) & ~3LL, x);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float a = x[i] * norm;       // two roundings, as numpy's `samps *= norm_factor` followed by `gain * samps`
    v[i] = a * gain;
  }
}

__device__ __forceinline__ void store8(float* __restrict__ row, const float v[8], int t0, int n, bool second) {
  float m[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = t0 + i < n ? v[i] : 0.f;
  st4(row, make_float4(m[0], m[1], m[2], m[3]));
  if (second) st4(row + 4, make_float4(m[4], m[5], m[6], m[7]));
}

template <int S>
__global__ __launch_bounds__(DM_TPB) void dynmix_kernel(DmCorpus c, const int* __restrict__ term_utt, const int* __restrict__ term_start,
                                                        const float* __restrict__ term_norm, const float* __restrict__ term_gain,
                                                        const int* __restrict__ nlen, int M, int Tmax, float* __restrict__ mix, DmRows src) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int t0 = (blockIdx.x * DM_TPB + threadIdx.x) * DM_PER;
  if (t0 >= Tmax) return;
  const bool second = t0 + 4 < Tmax;                               // Tmax is a multiple of 4, not of 8
  int n = nlen[b];
  n = n < 0 ? 0 : (n > Tmax ? Tmax : n);
  const long long row = (long long)b * Tmax + t0;
  float acc[8], keep[S][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (t0 >= n) {                                                   // the zero fill of pad_sequence
    store8(mix + row, acc, t0, n, second);
#pragma unroll
    for (int s = 0; s < S; ++s) store8(src.p[s] + row, acc, t0, n, second);
    return;
  }
  const int NT = M + S, j0 = b * NT;
#pragma unroll
  for (int m = 0; m < S + 1; ++m) {
    if (m < M) {
      float v[8];
      term_value(c, term_utt[j0 + m], term_start[j0 + m], term_norm[j0 + m], term_gain[j0 + m], t0, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = acc[i] + v[i];         // ((0 + t0) + t1) + ...: Python's sum(), then `+ noise`
      if (m < S) {
#pragma unroll
        for (int i = 0; i < 8; ++i) keep[m][i] = v[i];
      }
    }
  }
  store8(mix + row, acc, t0, n, second);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int jm = j0 + s, jt = j0 + M + s;
    const bool same = term_utt[jt] == term_utt[jm] && term_start[jt] == term_start[jm] &&
                      __float_as_uint(term_norm[jt]) == __float_as_uint(term_norm[jm]) &&
                      __float_as_uint(term_gain[jt]) == __float_as_uint(term_gain[jm]);
    if (same) {                                                    // WSJ0 / WHAM: the target IS the mixture term - computed once
      store8(src.p[s] + row, keep[s], t0, n, second);
    } else {
      float v[8];
      term_value(c, term_utt[jt], term_start[jt], term_norm[jt], term_gain[jt], t0, v);
      store8(src.p[s] + row, v, t0, n, second);
    }
  }
}

// partial sum of squares of utterance u = blockIdx.x over the chunks p, p + EN_PARTS, ... (p = blockIdx.y) of EN_TPB samples
__global__ __launch_bounds__(EN_TPB) void energy_part_kernel(DmCorpus c, long long* __restrict__ part) {
#pragma clang fp contract(off)
  const int u = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const bool is16 = u < c.N16;
  const long long total = is16 ? c.total16 : c.total32;
  const long long o0 = clampll(c.off[u] - (is16 ? 0 : c.off[c.N16]), 0, total);
  const long long len = clampll(c.off[u + 1] - c.off[u], 0, total - o0);
  __shared__ long long red[EN_TPB / 64];
  long long ai = 0;
  double ad = 0.0;
  for (long long i = (long long)p * EN_TPB + tid; i < len; i += (long long)EN_PARTS * EN_TPB) {
    if (is16) {
      const long long s = c.buf16[o0 + i];
      ai += s * s;
    } else {
      const double s = (double)c.buf32[o0 + i];
      ad += s * s;                                                 // the product of two float32 is exact in float64
    }
  }
  if (is16) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ai += __shfl_xor(ai, o, 64);
  } else {
    ai = __double_as_longlong(wave_sum_d(ad));
  }
  if ((tid & 63) == 0) red[tid >> 6] = ai;
  __syncthreads();
  if (tid == 0) {
    long long r;
    if (is16) {
      r = ((red[0] + red[1]) + red[2]) + red[3];
    } else {
      r = __double_as_longlong(((__longlong_as_double(red[0]) + __longlong_as_double(red[1])) + __longlong_as_double(red[2])) +
                               __longlong_as_double(red[3]));
    }
    part[(long long)u * EN_PARTS + p] = r;
  }
}

__global__ __launch_bounds__(256) void energy_finish_kernel(const long long* __restrict__ part, int N16, int N, long long* __restrict__ ss16,
                                                            double* __restrict__ ss32) {
#pragma clang fp contract(off)
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= N) return;
  const long long* q = part + (long long)u * EN_PARTS;
  if (u < N16) {
    long long r = 0;
#pragma unroll
    for (int p = 0; p < EN_PARTS; ++p) r += q[p];
    ss16[u] = r;
  } else {
    double r = 0.0;
#pragma unroll
    for (int p = 0; p < EN_PARTS; ++p) r += __longlong_as_double(q[p]);
    ss32[u - N16] = r;
  }
}

// the argument checks the two entries share; 0 = fine
int corpus_args_bad(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N) {
  if (!offsets || N < 1 || N16 < 0 || N16 > N) return 1;
  if (N16 > 0 && (!buf16 || total16 < 1)) return 1;
  if (N > N16 && (!buf32 || total32 < 1)) return 1;
  if (total16 < 0 || total32 < 0) return 1;
  if ((reinterpret_cast<uintptr_t>(buf16) | reinterpret_cast<uintptr_t>(buf32)) % 16 != 0) return 1;      // aligned 16-byte loads
  return 0;
}
}  // namespace
}  // namespace sepr

extern "C" size_t sepr_corpus_energy_workspace(int N) {
  using namespace sepr;
  if (N < 1) return 0;
  return align_up((size_t)N * EN_PARTS * sizeof(long long));
}

extern "C" int sepr_corpus_energy(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                                  int N16, int N, long long* ss16, double* ss32, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (corpus_args_bad(buf16, total16, buf32, total32, offsets, N16, N)) return SEPR_EINVAL;
  if ((N16 > 0 && !ss16) || (N > N16 && !ss32)) return SEPR_EINVAL;
  if (!ws || ws_bytes < sepr_corpus_energy_workspace(N)) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DmCorpus c = {buf16, buf32, offsets, total16, total32, N16, N};
  long long* part = static_cast<long long*>(ws);
  hipLaunchKernelGGL(energy_part_kernel, dim3((unsigned)N, EN_PARTS), dim3(EN_TPB), 0, st, c, part);
  hipLaunchKernelGGL(energy_finish_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, part, N16, N, ss16, ss32);
  SEPR_CHECK_LAUNCH("corpus energy kernels");
  return SEPR_OK;
}

extern "C" int sepr_dynmix_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                               int N16, int N, const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain,
                               const int* n, int B, int M, int S, int Tmax, float* mix, float* const* src, sepr_stream_t stream) {
  using namespace sepr;
  if (corpus_args_bad(buf16, total16, buf32, total32, offsets, N16, N)) return SEPR_EINVAL;
  if (!term_utt || !term_start || !term_norm || !term_gain || !n || !mix || !src) return SEPR_EINVAL;
  if (B < 1 || B > 65535 || S < 2 || S > 3 || M < S || M > S + 1 || Tmax < 4 || Tmax % 4 != 0) return SEPR_EINVAL;
  DmRows rows = {{nullptr, nullptr, nullptr}};
  uintptr_t al = reinterpret_cast<uintptr_t>(mix);
  for (int s = 0; s < S; ++s) {
    if (!src[s]) return SEPR_EINVAL;
    rows.p[s] = src[s];
    al |= reinterpret_cast<uintptr_t>(src[s]);
  }
  if (al % 16 != 0) return SEPR_EINVAL;                            // float4 stores
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DmCorpus c = {buf16, buf32, offsets, total16, total32, N16, N};
  const dim3 grid((unsigned)cdiv(Tmax, DM_TPB * DM_PER), (unsigned)B);
  if (S == 2)
    hipLaunchKernelGGL((dynmix_kernel<2>), grid, dim3(DM_TPB), 0, st, c, term_utt, term_start, term_norm, term_gain, n, M, Tmax, mix, rows);
  else
    hipLaunchKernelGGL((dynmix_kernel<3>), grid, dim3(DM_TPB), 0, st, c, term_utt, term_start, term_norm, term_gain, n, M, Tmax, mix, rows);
  SEPR_CHECK_LAUNCH("dynmix kernel");
  return SEPR_OK;
}
