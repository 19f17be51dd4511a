// Sample-rate conversion of whole recordings: the converter of sepr_polyphase.h - which states the filter, the span rule,
// the window, the staging loop and the fma chain - one thread per output sample, one workgroup per tile of RS_TILE consecutive outputs of ONE
// recording (grid.y = recording): the tile's input span is staged once in LDS, zero-extended at both ends of the recording - a tile never reads
// another recording's samples.  L = 1 (integer decimation): every output uses the same tap row, kept in LDS as doubles and read as a
// broadcast.  L > 1: the table arrives transposed and in output order, [K][L] indexed by n mod L, so consecutive lanes read
// consecutive taps of a table that stays in L2.  No atomics, nothing depends on the launch order: bit-identical from run to run,
// and a recording's result does not depend on what else is in the call.
#include "sepr_polyphase.h"

namespace sepr {
namespace {
constexpr int RS_TILE = 256;
constexpr int RS_MAX_R = 65535;                  // grid.y

template <bool ONE>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const float* __restrict__ x, const long long* __restrict__ in_off,
                                                           float* __restrict__ y, const long long* __restrict__ out_off,
                                                           const float* __restrict__ taps, int L, int M, int K) {
  extern __shared__ double rs_lds[];
  const int r = blockIdx.y, tid = threadIdx.x;
  const long long xo = in_off[r], T = in_off[r + 1] - xo, yo = out_off[r], N = out_off[r + 1] - yo;
  const long long n0 = (long long)blockIdx.x * RS_TILE;
  if (n0 >= N) return;                                              // the grid is as wide as the longest recording
  const int Hh = (K - 2) / 2, span = (int)pp_span(RS_TILE, L, M, K), Lq = ONE ? 1 : L;   // (L = 1 as a constant: no division)
  const long long b0 = pp_base(n0, Lq, M);
  double* xs = rs_lds;
  double* ts = rs_lds + span;
  pp_stage<RS_TILE>(xs, span, b0 - Hh, T, [&](long long g, int) { return (double)x[xo + g]; });
  if (ONE)
    for (int j = tid; j < K; j += RS_TILE) ts[j] = (double)taps[j];
  __syncthreads();
  const long long n = n0 + tid;
  if (n >= N) return;
  const double* const xp[1] = {xs + (int)(pp_base(n, Lq, M) - b0)};  // n M in 64 bits; 0 <= b - b0 <= (RS_TILE - 1) M / L + 1
  double acc[1] = {0.0};
  if (ONE) {   // its own text, not pp_chain: through the template this instantiation takes two more instructions (docs/HISTORY.md)
#pragma unroll 8
    for (int j = 0; j < K; ++j) acc[0] = fma(ts[j], xp[0][j], acc[0]);
  } else {
    const float* const tq[1] = {taps + pp_phase(n, L)};
    pp_chain<1, 8>(tq, (long long)L, xp, K, acc);
  }
  y[yo + n] = (float)acc[0];
}
struct ResampleWs {   // device copies of in_offset and out_offset [R + 1]
  long long *ioff, *ooff;
  ResampleWs(Arena& a, int R) { ioff = a.of<long long>((size_t)(R + 1)); ooff = a.of<long long>((size_t)(R + 1)); }
};
}  // namespace
}  // namespace sepr

extern "C" long long sepr_resample_out_len(long long T, int L, int M) {
  if (T < 1 || L < 1 || M < 1 || T > (1LL << 62) / L) return 0;
  return sepr::pp_out_len(T, L, M);
}

extern "C" size_t sepr_resample_workspace(int R) {
  using namespace sepr;
  if (R < 1 || R > RS_MAX_R) return 0;
  return layout_bytes<ResampleWs>(R);
}

extern "C" int sepr_resample_fwd(const float* x, const long long* in_offset, float* y, const long long* out_offset, int R,
                                 const float* taps, int L, int M, int K, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!x || !in_offset || !y || !out_offset || !taps) return SEPR_EINVAL;
  if (R < 1 || R > RS_MAX_R || L < 1 || M < 1 || K < 2 || K % 2 != 0) return SEPR_EINVAL;
  const long long span = pp_span(RS_TILE, L, M, K);
  const size_t lds = (size_t)(span + (L == 1 ? K : 0)) * sizeof(double);
  if (span > 0x7fffffffLL || lds > PP_MAX_LDS) return SEPR_EINVAL;                                       // ratio beyond one tile's LDS
  if (in_offset[0] != 0 || out_offset[0] != 0) return SEPR_EINVAL;
  long long nmax = 0;
  for (int r = 0; r < R; ++r) {
    const long long T = in_offset[r + 1] - in_offset[r], N = out_offset[r + 1] - out_offset[r];
    if (T < 1 || N < 1 || N != sepr_resample_out_len(T, L, M)) return SEPR_EINVAL;
    if (N > (1LL << 62) / M) return SEPR_EINVAL;                    // n * M stays inside 64 bits
    nmax = N > nmax ? N : nmax;
  }
  const long long tiles = (nmax + RS_TILE - 1) / RS_TILE;
  if (tiles > 0x7fffffffLL) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  const ResampleWs k(ar, R);
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(k.ioff, in_offset, (size_t)(R + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(k.ooff, out_offset, (size_t)(R + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    set_hip_error(e, "resample setup");
    return SEPR_EHIP;
  }
  const dim3 grid((unsigned)tiles, (unsigned)R);
  if (L == 1)
    hipLaunchKernelGGL((resample_kernel<true>), grid, dim3(RS_TILE), lds, st, x, k.ioff, y, k.ooff, taps, L, M, K);
  else
    hipLaunchKernelGGL((resample_kernel<false>), grid, dim3(RS_TILE), lds, st, x, k.ioff, y, k.ooff, taps, L, M, K);
  SEPR_CHECK_LAUNCH("resample kernel");
  return SEPR_OK;
}
