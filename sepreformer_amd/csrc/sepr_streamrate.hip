// Sample-rate conversion inside the stream bank: the converter of sepr_polyphase.h - sepr_resample_fwd's filter, span rule,
// window and fma chain, the same code and so the same bits - computed a span of outputs at a time for A rows of one hop, each row with its own
// converter, reading from and writing to rings.
//
// The taps are (double)taps[j][n mod L] of the [K][L] device table for every L - at L = 1 column 0 is the tap row itself, the value
// resample_kernel<true> keeps in LDS - so one code path serves both; a table of up to 4096 taps that fits beside the span is widened into LDS
// once per tile (every L = 1 converter inside the span limit, and the small upsampling tables), a larger one is read from global memory as
// resample_kernel<false> reads it.  What is this file's own is the addressing: source sample t lies at src + base + (t - origin) mod cap,
// output n goes to dst + base + (n - origin) mod cap, and the row's converter, span of outputs [n0, n1) and T_known come from a DEVICE table.
// One workgroup per tile of SR_TILE consecutive outputs of ONE row (grid.y = row), a tile never reads another row's samples.  No atomics,
// nothing depends on the launch order: bit-identical from run to run.
//
// stream_carry_kernel moves the last `hist` emitted samples of every track of the hop's streams to the front of their rows, after the
// conversion that read the old history has run (a launch of its own: the order of two launches on one stream is the whole synchronisation).
#include "sepr_polyphase.h"

namespace sepr {
namespace {
constexpr int SR_TILE = 256;
constexpr int SR_MAX_A = 65535;                  // grid.y
constexpr int SR_COLS = 10;                      // include/sepr.h: the convert table's columns
constexpr int SR_STEP_COLS = 6;                  // sepr_streambank_step's table, whose slot column the carry reads

constexpr long long SR_TAPS_LDS = 4096;          // a table of up to this many taps is staged in LDS beside the span, as doubles

// a small table is read by every wave of the launch: from global memory its few cache lines are what the launch waits for
__host__ __device__ inline bool sr_taps_in_lds(int L, int M, int K) {
  const long long n = (long long)K * L;
  return n <= SR_TAPS_LDS && (size_t)(pp_span(SR_TILE, L, M, K) + n) * sizeof(double) <= PP_MAX_LDS;
}

// (t - origin) mod cap in [0, cap), for any t and origin (the difference wraps in unsigned arithmetic instead of overflowing)
__device__ __forceinline__ long long ring_at(long long t, long long origin, long long cap) {
  const long long m = (long long)((unsigned long long)t - (unsigned long long)origin) % cap;
  return m < 0 ? m + cap : m;
}

__global__ __launch_bounds__(SR_TILE) void stream_convert_kernel(const float* __restrict__ src, long long src_elems, float* __restrict__ dst,
                                                                 long long dst_elems, const long long* __restrict__ table, long long nmax,
                                                                 const ConvSet cv) {
  extern __shared__ double sr_lds[];
  const int a = blockIdx.y, tid = threadIdx.x;
  const long long* row = table + (long long)a * SR_COLS;
  // the table is not trusted: every value that forms an address or a trip count is clamped into range
  const long long cr = row[0];
  // (the row is the workgroup's: through readfirstlane the converter's L, M, K and table pointer are scalars, as they are in resample_kernel)
  const int ci = __builtin_amdgcn_readfirstlane((int)(cr < 0 ? 0 : (cr >= cv.NC ? cv.NC - 1 : cr)));
  const int L = cv.L[ci], M = cv.M[ci], K = cv.K[ci];
  const float* __restrict__ taps = cv.taps[ci];
  const long long nlim = (1LL << 62) / M;                           // n M stays inside 64 bits
  long long n0 = row[1], n1 = row[2];
  n0 = n0 < 0 ? 0 : (n0 > nlim ? nlim : n0);
  n1 = n1 < 0 ? 0 : (n1 > nlim ? nlim : n1);
  n1 = n1 - n0 > nmax ? n0 + nmax : n1;                             // the grid is as wide as nmax outputs
  const long long T = row[3];
  const long long sbase = row[4], sorg = row[5], scap = row[6], dbase = row[7], dorg = row[8], dcap = row[9];
  const long long t0 = n0 + (long long)blockIdx.x * SR_TILE;
  if (t0 >= n1) return;
  if (scap < 1 || sbase < 0 || sbase > src_elems - scap || dcap < 1 || dbase < 0 || dbase > dst_elems - dcap) return;
  const int Hh = (K - 2) / 2, span = (int)pp_span(SR_TILE, L, M, K);
  const long long b0 = pp_base(t0, L, M);
  double* xs = sr_lds;
  const long long g0 = b0 - Hh;
  const long long p0 = ring_at(g0, sorg, scap);
  // its own staging loop, not pp_stage: with the ring position under the predicate the one-row launch measured 0.9 us longer (docs/HISTORY.md)
  for (int i = tid; i < span; i += SR_TILE) {
    const long long g = g0 + i;
    long long p = p0 + i;                                           // a ring at least a span long wraps at most once inside a tile
    if (p >= scap) p -= scap;
    if (p >= scap) p %= scap;
    xs[i] = (g >= 0 && g < T) ? (double)src[sbase + p] : 0.0;
  }
  const bool staged = sr_taps_in_lds(L, M, K);
  double* ts = sr_lds + span;
  if (staged)
    for (int i = tid; i < K * L; i += SR_TILE) ts[i] = (double)taps[i];
  __syncthreads();
  const long long n = t0 + tid;
  if (n >= n1) return;
  const double* const xp[1] = {xs + (int)(pp_base(n, L, M) - b0)};  // n M in 64 bits; 0 <= b - b0 <= (SR_TILE - 1) M / L + 1
  const int q = pp_phase(n, L);
  double acc[1];
  if (staged) {                                                     // the same doubles, widened once per tile instead of once per use
    const double* const tq[1] = {ts + q};
    pp_chain<1, 8>(tq, L, xp, K, acc);
  } else {
    const float* const tq[1] = {taps + q};
    pp_chain<1, 8>(tq, (long long)L, xp, K, acc);
  }
  dst[dbase + ring_at(n, dorg, dcap)] = (float)acc[0];
}

// rows [slot][S] of `row_len` floats: [0, hist) <- [hist, 2 hist) for the slot of every row of the step table
__global__ __launch_bounds__(SR_TILE) void stream_carry_kernel(float* __restrict__ buf, const long long* __restrict__ table, int slots, int S,
                                                               int hist, long long row_len) {
  const int a = blockIdx.y / S, s = blockIdx.y % S, q = 4 * (blockIdx.x * SR_TILE + threadIdx.x);
  if (q >= hist) return;
  long long slot = table[(long long)a * SR_STEP_COLS];
  slot = slot < 0 ? 0 : (slot >= slots ? slots - 1 : slot);
  float* r = buf + (slot * S + s) * row_len;
  st4(r + q, ld4(r + hist + q));                                    // hist is a multiple of 4 and 2 hist <= row_len: the halves are disjoint
}
}  // namespace
}  // namespace sepr

extern "C" int sepr_streambank_convert(const float* src, long long src_elems, float* dst, long long dst_elems, const long long* table, int A,
                                       long long nmax, const float* const* conv_taps, const int* conv_L, const int* conv_M,
                                       const int* conv_K, int NC, sepr_stream_t stream) {
  using namespace sepr;
  if (!src || !dst || !table || !conv_taps || !conv_L || !conv_M || !conv_K) return SEPR_EINVAL;
  if (A < 1 || A > SR_MAX_A || src_elems < 1 || dst_elems < 1 || nmax < 1) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 != 0) return SEPR_EINVAL;
  if (reinterpret_cast<uintptr_t>(table) % 8 != 0) return SEPR_EINVAL;
  // at least one converter, aligned tables, a ratio inside one tile's LDS (sepr_resample_fwd's limit); the unused entries repeat the last one
  ConvSet cv;
  if (!pp_fill(conv_taps, conv_L, conv_M, conv_K, NC, {SR_TILE, 1, 0, PP_MAX_LDS, true, true}, cv)) return SEPR_EINVAL;
  size_t lds = 0;
  for (int k = 0; k < NC; ++k) {
    const long long tab = sr_taps_in_lds(cv.L[k], cv.M[k], cv.K[k]) ? (long long)cv.K[k] * cv.L[k] : 0;
    const size_t need = (size_t)(pp_span(SR_TILE, cv.L[k], cv.M[k], cv.K[k]) + tab) * sizeof(double);
    lds = need > lds ? need : lds;
  }
  const long long tiles = (nmax + SR_TILE - 1) / SR_TILE;
  if (tiles > 0x7fffffffLL) return SEPR_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(stream_convert_kernel, dim3((unsigned)tiles, (unsigned)A), dim3(SR_TILE), lds, st, src, src_elems, dst, dst_elems, table,
                     nmax, cv);
  SEPR_CHECK_LAUNCH("stream convert kernel");
  return SEPR_OK;
}

extern "C" int sepr_streambank_carry(float* buf, long long buf_elems, const long long* step_table, int A, int slots, int S, int hist,
                                     long long row_len, sepr_stream_t stream) {
  using namespace sepr;
  if (!buf || !step_table) return SEPR_EINVAL;
  if (A < 1 || slots < 1 || slots > (1 << 20) || S < 1 || S > 3 || (long long)A * S > SR_MAX_A) return SEPR_EINVAL;
  if (hist < 4 || hist % 4 != 0 || row_len % 4 != 0 || row_len < 2LL * hist || row_len > (1LL << 40)) return SEPR_EINVAL;
  if (buf_elems < (long long)slots * S * row_len) return SEPR_EINVAL;
  if (reinterpret_cast<uintptr_t>(buf) % 16 != 0 || reinterpret_cast<uintptr_t>(step_table) % 8 != 0) return SEPR_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(stream_carry_kernel, dim3((unsigned)((hist / 4 + SR_TILE - 1) / SR_TILE), (unsigned)(A * S)), dim3(SR_TILE), 0, st, buf,
                     step_table, slots, S, hist, row_len);
  SEPR_CHECK_LAUNCH("stream carry kernel");
  return SEPR_OK;
}
