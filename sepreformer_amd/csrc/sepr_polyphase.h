// The rational-ratio converter, stated once for the launches that run it: sepr_resample_fwd, sepr_streambank_convert and the
// speed forms of the dynamic-mixing launch.
//   y[n] = float32( sum_{j < K} double(tap[(n M) mod L][j]) * double(x[floor(n M / L) - Hh + j]) ),   Hh = (K - 2) / 2,   x = 0 outside [0, T)
// Taps and samples are float32, so every product is exact in float64; the products are summed in float64 from 0.0 in the order j = 0 .. K - 1 and
// the sum is rounded once.  A tile of consecutive outputs from n0 reads the input span [b0 - Hh, b0 - Hh + pp_span), b0 = floor(n0 M / L), staged in
// LDS as doubles and zero-extended by predicate; output n reads K doubles from d = floor(n M / L) - b0 on against column n mod L of the [K][L] device
// table (resample.device_table).  A kernel that keeps a text of its own for a piece says so at the place (docs/HISTORY.md, "The converter stated once").
#pragma once
#include "sepr_common.h"

namespace sepr {
constexpr int PP_MAX_NC = 16;                    // converters one launch takes (include/sepr.h)
constexpr size_t PP_MAX_LDS = 64 * 1024;         // dynamic LDS of a workgroup: the span limit of sepr_resample_fwd and sepr_streambank_convert

// input samples a tile of `tile` consecutive outputs reads
__host__ __device__ inline long long pp_span(int tile, int L, int M, int K) { return ((long long)(tile - 1) * M) / L + K + 1; }

// ceil(T L / M): the outputs of T > 0 input samples (the caller keeps T L inside 64 bits)
__host__ __device__ inline long long pp_out_len(long long T, int L, int M) { return (T * L + M - 1) / M; }

struct ConvSet {
  const float* taps[PP_MAX_NC];                  // [K][L], column q = the tap row of phase (q M) mod L (resample.device_table)
  int L[PP_MAX_NC], M[PP_MAX_NC], K[PP_MAX_NC];
  int NC;
};

// what an entry asks of its converters beyond L, M >= 1 and K even, K >= 2: the policies differ (include/sepr.h) and stay apart, the loop is one
struct ConvPolicy {
  int tile;                                      // outputs per tile of the entry's kernel
  int min_nc;
  long long max_doubles;                         // > 0: the span may not exceed it
  size_t max_bytes;                              // > 0: the span as doubles, with the tap row of an L = 1 converter beside it, may not exceed it
  bool aligned;                                  // tap pointers are 4-byte aligned
  bool repeat_last;                              // the entries from NC on repeat the last one (else they stay as the caller left them)
};

// the converter arguments of an entry, checked against its policy and copied into cv; false = refuse
inline bool pp_fill(const float* const* taps, const int* L, const int* M, const int* K, int NC, const ConvPolicy& p, ConvSet& cv) {
  if (NC < p.min_nc || NC > PP_MAX_NC) return false;
  if (NC > 0 && (!taps || !L || !M || !K)) return false;
  cv.NC = NC;
  for (int k = 0; k < (p.repeat_last && NC > 0 ? PP_MAX_NC : NC); ++k) {
    const int c = k < NC ? k : NC - 1;
    if (!taps[c] || (p.aligned && reinterpret_cast<uintptr_t>(taps[c]) % 4 != 0)) return false;
    if (L[c] < 1 || M[c] < 1 || K[c] < 2 || K[c] % 2 != 0) return false;
    const long long span = pp_span(p.tile, L[c], M[c], K[c]);
    if (p.max_doubles > 0 && span > p.max_doubles) return false;
    if (p.max_bytes > 0 && (span > 0x7fffffffLL || (size_t)(span + (L[c] == 1 ? K[c] : 0)) * sizeof(double) > p.max_bytes)) return false;
    cv.taps[k] = taps[c];
    cv.L[k] = L[c];
    cv.M[k] = M[c];
    cv.K[k] = K[c];
  }
  return true;
}

// output n reads a span staged from input sample b0 - Hh on from d = pp_base(n) - b0 (0 .. (tile - 1) M / L + 1 inside its tile), column pp_phase(n)
__device__ __forceinline__ long long pp_base(long long n, int L, int M) { return (n * M) / L; }
__device__ __forceinline__ int pp_phase(long long n, int L) { return (int)(n % L); }
// d clamped into [0, lim], lim = span - K the highest window base inside the staged span: for kernels whose n comes from an untrusted table
__device__ __forceinline__ int pp_window(long long n, int L, int M, long long b0, int lim) {
  const long long d = pp_base(n, L, M) - b0;
  return (int)(d < 0 ? 0 : (d > lim ? lim : d));
}

// xs[i] = src(g0 + i, i) for i < count, zero where g0 + i lies outside [0, T): all TPB threads of the workgroup, no barrier.  src(g, i) is the
// sample g as a double; it is called inside [0, T) only.
template <int TPB, class Src>
__device__ __forceinline__ void pp_stage(double* __restrict__ xs, int count, long long g0, long long T, Src src) {
  for (int i = threadIdx.x; i < count; i += TPB) {
    const long long g = g0 + i;
    xs[i] = (g >= 0 && g < T) ? src(g, i) : 0.0;
  }
}

// acc[i] = sum_{j < K} double(tq[i][j * stride]) * xp[i][j] for NI interleaved chains, j ascending, each from 0.0
template <int NI, int UNROLL, class TapT, class StrideT>
__device__ __forceinline__ void pp_chain(const TapT* const (&tq)[NI], StrideT stride, const double* const (&xp)[NI], int K, double (&acc)[NI]) {
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = 0.0;
#pragma unroll UNROLL
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = fma((double)tq[i][j * stride], xp[i][j], acc[i]);
  }
}
}  // namespace sepr
