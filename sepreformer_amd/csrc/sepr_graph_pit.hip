// Graph-PIT on the device (contracts in include/sepr.h): which target row of a conversation window goes on which output
// channel, and the channels' targets assembled from the rows.
//
//   gp_moment_kernel    one workgroup per (example, moment): a moment is the dot product of two rows - or of a row and ones - over an interval, in
//                       float64 on exact float32 inputs, written as segsnr_value_kernel of sepr_conversation.hip is: thread i adds the samples
//                       i, i + 256, ... of the interval in order, a wave adds its lanes by butterfly, the four wave sums are added in wave order.  An
//                       empty interval stores 0 and exits at once.  A row is never read outside its clamped span.
//   gp_search_kernel    one workgroup per example: the moments into LDS, then the C^L colourings of the L live rows spread over the threads - thread i
//                       takes the colourings i, i + 256, ... in lexicographic order, each evaluated whole from the small tables - and the minimum
//                       with its first index reduced in a fixed order (lanes by butterfly under a total order, then the four waves in wave order).
//   gp_assemble_kernel  one thread per four samples of an example: the rows of each colour added in ascending row order from +0.0, one float4
//                       store per channel.  A row that covers the four samples is read with one aligned float4 load (the samples start at a multiple
//                       of 4 of a 16-byte aligned row), one that covers some of them element by element under the span's mask.
// No atomics; nothing depends on the launch order of workgroups: results are bit-identical from run to run.  The span, adjacency and colour tables are
// device memory and are not trusted: every value read from one is clamped, so a bad table gives wrong values but no access outside a buffer.
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr int GP_TPB = 256;
constexpr int GP_MAX_C = 3;
constexpr int GP_MAX_U = 8;
constexpr int GP_MAX_PAIRS = GP_MAX_U * (GP_MAX_U - 1) / 2;

struct GpEst { const float* p[GP_MAX_C]; };
struct GpRows { const float* p[GP_MAX_U]; };
struct GpOut { float* p[GP_MAX_C]; };

// the moments of one example, in this order: se_c, ee_c [C]; st_u, tt_u [U]; et_cu [C][U]; tv_uv, u < v in lexicographic order [U (U - 1) / 2]
__host__ __device__ __forceinline__ int gp_moments(int C, int U) { return 2 * C + 2 * U + C * U + U * (U - 1) / 2; }
__host__ __device__ __forceinline__ int gp_pair(int u, int v, int U) { return u * (2 * U - u - 1) / 2 + (v - u - 1); }      // u < v

__device__ __forceinline__ const float* gp_pick(const GpEst& e, int c) {
  const float* p = e.p[0];
#pragma unroll
  for (int k = 1; k < GP_MAX_C; ++k) p = k == c ? e.p[k] : p;
  return p;
}
__device__ __forceinline__ const float* gp_pick(const GpRows& r, int u) {
  const float* p = r.p[0];
#pragma unroll
  for (int k = 1; k < GP_MAX_U; ++k) p = k == u ? r.p[k] : p;
  return p;
}

// the span of row u of example b under clamps: on into [0, T], off into [on, T]
__device__ __forceinline__ void gp_span(const int* __restrict__ spans, int b, int u, int U, int T, int& on, int& off) {
  const int* s = spans + ((long long)b * U + u) * 2;
  const int a = s[0], e = s[1];
  on = a < 0 ? 0 : (a > T ? T : a);
  off = e < on ? on : (e > T ? T : e);
}

__global__ __launch_bounds__(GP_TPB) void gp_moment_kernel(GpEst est, GpRows rows, const int* __restrict__ spans, int C, int U, int T,
                                                           double* __restrict__ mom) {
#pragma clang fp contract(off)
  __shared__ double red[GP_TPB / 64];
  const int b = blockIdx.y, tid = threadIdx.x, M = gp_moments(C, U);
  int m = blockIdx.x;
  double* __restrict__ dst = mom + (long long)b * M + m;
  const float* x = nullptr;
  const float* y = nullptr;                            // nullptr: ones
  int lo = 0, hi = T;
  if (m < 2 * C) {                                     // se_c, ee_c over all T
    x = gp_pick(est, m < C ? m : m - C);
    y = m < C ? nullptr : x;
  } else if ((m -= 2 * C) < 2 * U) {                   // st_u, tt_u over the span of u
    const int u = m < U ? m : m - U;
    x = gp_pick(rows, u);
    y = m < U ? nullptr : x;
    gp_span(spans, b, u, U, T, lo, hi);
  } else if ((m -= 2 * U) < C * U) {                   // et_cu over the span of u
    const int c = m / U, u = m - c * U;
    x = gp_pick(est, c);
    y = gp_pick(rows, u);
    gp_span(spans, b, u, U, T, lo, hi);
  } else {                                             // tv_uv over the intersection of the two spans
    m -= C * U;
    int u = 0;
    while (u < U - 2 && m >= U - 1 - u) m -= U - 1 - u, ++u;
    const int v = u + 1 + (m < U - 2 - u ? m : U - 2 - u);
    x = gp_pick(rows, u);
    y = gp_pick(rows, v);
    int lo2, hi2;
    gp_span(spans, b, u, U, T, lo, hi);
    gp_span(spans, b, v, U, T, lo2, hi2);
    lo = lo > lo2 ? lo : lo2;
    hi = hi < hi2 ? hi : hi2;
  }
  if (hi <= lo) {                                      // workgroup-uniform: an empty interval
    if (tid == 0) *dst = 0.0;
    return;
  }
  x += (long long)b * T;
  double a = 0.0;
  if (y) {
    y += (long long)b * T;
    for (int i = lo + tid; i < hi; i += GP_TPB) a += (double)x[i] * (double)y[i];      // the product of two float32 values is exact in float64
  } else {
    for (int i = lo + tid; i < hi; i += GP_TPB) a += (double)x[i];
  }
  a = block_sum_d(a, red);                            // every thread is here: the one return above is workgroup-uniform
  if (tid == 0) *dst = a;
}

// the tables of one example in LDS, and the colouring they are evaluated under
struct GpTables {
  double se[GP_MAX_C], ee[GP_MAX_C], st[GP_MAX_U], tt[GP_MAX_U], et[GP_MAX_C][GP_MAX_U], tv[GP_MAX_PAIRS];
  unsigned adj[GP_MAX_U];                              // symmetric, no self loops, live rows only
  int live[GP_MAX_U];                                  // the rows with a non-empty span, ascending
  int L, count;                                        // live rows; C^L colourings
};

// colouring idx in lexicographic order of (col(live[0]), .., col(live[L - 1])): live[0] is the most significant digit.  cols holds 2 bits per row.
__device__ __forceinline__ unsigned gp_decode(const GpTables& tb, int C, int idx) {
  unsigned cols = 0;
  for (int k = tb.L - 1; k >= 0; --k) {
    const int q = idx / C;
    cols |= (unsigned)(idx - q * C) << (2 * tb.live[k]);
    idx = q;
  }
  return cols;
}

__device__ __forceinline__ bool gp_valid(const GpTables& tb, int U, unsigned cols) {
  for (int k = 0; k < tb.L; ++k) {
    const int u = tb.live[k];
    const unsigned cu = (cols >> (2 * u)) & 3u;
    unsigned a = tb.adj[u];
    while (a) {
      const int v = __ffs(a) - 1;
      a &= a - 1;
      if (((cols >> (2 * v)) & 3u) == cu) return false;
    }
  }
  return true;
}

// E and D of a colouring (include/sepr.h): per colour the rows in ascending order, the pairs in lexicographic order
__device__ __forceinline__ void gp_energy(const GpTables& tb, int C, int U, int T, unsigned cols, double& E, double& D) {
#pragma clang fp contract(off)
  const double dT = (double)T;
  double e = 0.0, d = 0.0;
  for (int c = 0; c < C; ++c) {
    double Sy = 0.0, tts = 0.0, cross = 0.0, ets = 0.0;
    for (int k = 0; k < tb.L; ++k) {
      const int u = tb.live[k];
      if ((int)((cols >> (2 * u)) & 3u) != c) continue;
      Sy += tb.st[u];
      tts += tb.tt[u];
      ets += tb.et[c][u];
      for (int j = k + 1; j < tb.L; ++j) {
        const int v = tb.live[j];
        if ((int)((cols >> (2 * v)) & 3u) == c) cross += tb.tv[gp_pair(u, v, U)];
      }
    }
    const double yy = (tts + 2.0 * cross) - Sy * Sy / dT;
    const double eet = tb.ee[c] - tb.se[c] * tb.se[c] / dT;
    const double ey = ets - tb.se[c] * Sy / dT;
    e += (eet - 2.0 * ey) + yy;
    d += yy;
  }
  E = e > 0.0 ? e : 0.0;
  D = d;
}

struct GpBest {
  double E;
  int idx;                                             // INT_MAX: no valid colouring seen
};
// a total order on (valid, E, idx): the lower E, then the lower index
__device__ __forceinline__ GpBest gp_better(GpBest a, GpBest b) {
  if (b.idx == 0x7fffffff) return a;
  if (a.idx == 0x7fffffff) return b;
  return (b.E < a.E || (b.E == a.E && b.idx < a.idx)) ? b : a;
}

__global__ __launch_bounds__(GP_TPB) void gp_search_kernel(const double* __restrict__ mom, const int* __restrict__ spans,
                                                           const unsigned* __restrict__ adj, int C, int U, int T, double eps, double tau,
                                                           int* __restrict__ col, double* __restrict__ value, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ GpTables tb;
  __shared__ GpBest red[GP_TPB / 64];
  const int b = blockIdx.x, tid = threadIdx.x, M = gp_moments(C, U);
  const double* __restrict__ m = mom + (long long)b * M;
  if (tid < M) {
    const double v = m[tid];
    int k = tid;
    if (k < C) tb.se[k] = v;
    else if ((k -= C) < C) tb.ee[k] = v;
    else if ((k -= C) < U) tb.st[k] = v;
    else if ((k -= U) < U) tb.tt[k] = v;
    else if ((k -= U) < C * U) tb.et[k / U][k % U] = v;
    else tb.tv[k - C * U] = v;
  }
  if (tid == 0) {
    int L = 0, count = 1;
    unsigned livemask = 0;
    for (int u = 0; u < U; ++u) {
      int on, off;
      gp_span(spans, b, u, U, T, on, off);
      if (off > on) tb.live[L++] = u, livemask |= 1u << u, count *= C;
    }
    for (int u = 0; u < U; ++u) {                      // symmetric closure on the live rows: an edge if either side names it
      unsigned a = adj[(long long)b * U + u];
      for (int v = 0; v < U; ++v) a |= ((adj[(long long)b * U + v] >> u) & 1u) << v;
      tb.adj[u] = ((livemask >> u) & 1u) ? (a & livemask & ~(1u << u)) : 0u;
    }
    tb.L = L, tb.count = count;
  }
  __syncthreads();
  GpBest best = {0.0, 0x7fffffff};
  for (int idx = tid; idx < tb.count; idx += GP_TPB) {   // ascending: a later colouring must be strictly better
    const unsigned cols = gp_decode(tb, C, idx);
    if (!gp_valid(tb, U, cols)) continue;
    double E, D;
    gp_energy(tb, C, U, T, cols, E, D);
    if (best.idx == 0x7fffffff || E < best.E) best.E = E, best.idx = idx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    GpBest other;
    other.E = __shfl_xor(best.E, o, 64);
    other.idx = __shfl_xor(best.idx, o, 64);
    best = gp_better(best, other);
  }
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    best = gp_better(gp_better(gp_better(red[0], red[1]), red[2]), red[3]);
    const bool found = best.idx != 0x7fffffff;
    const unsigned cols = found ? gp_decode(tb, C, best.idx) : 0u;
    for (int u = 0; u < U; ++u) col[(long long)b * U + u] = (int)((cols >> (2 * u)) & 3u);
    status[b] = found ? 0 : 1;
    if (found) {
      double E, D;
      gp_energy(tb, C, U, T, cols, E, D);
      value[b] = 10.0 * log10((E + tau * D + eps) / (D + eps));
    } else {
      value[b] = __longlong_as_double(0x7ff8000000000000LL);
    }
  }
}

__global__ __launch_bounds__(GP_TPB) void gp_assemble_kernel(GpRows rows, const int* __restrict__ spans, const int* __restrict__ col, int C, int U,
                                                             int T, int tiles, GpOut out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x / tiles;
  const int t0 = ((blockIdx.x - b * tiles) * GP_TPB + threadIdx.x) * 4;          // T is a multiple of 4: the four samples are all below it or none is
  if (t0 >= T) return;
  float acc[GP_MAX_C][4];
#pragma unroll
  for (int c = 0; c < GP_MAX_C; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.f;
  for (int u = 0; u < U; ++u) {                                                  // ascending rows: ((+0.0 + t_u1) + t_u2) + ... per colour
    int on, off;
    gp_span(spans, b, u, U, T, on, off);
    if (off <= t0 || on >= t0 + 4) continue;                                     // adding +0.0 to a sum that began at +0.0 changes no bit
    const int cr = col[(long long)b * U + u];
    const int cu = cr < 0 ? 0 : (cr >= C ? C - 1 : cr);
    const float* __restrict__ r = gp_pick(rows, u) + (long long)b * T + t0;
    float x[4];
    if (on <= t0 && off >= t0 + 4) {
      const float4 q = ld4(r);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = (t0 + i >= on && t0 + i < off) ? r[i] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < GP_MAX_C; ++c) {
      if (c == cu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[c][i] = acc[c][i] + x[i];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < GP_MAX_C; ++c) {
    if (c < C) st4(out.p[c] + (long long)b * T + t0, make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]));
  }
}

struct GpLayout {
  double* mom;                           // [B][gp_moments(C, U)]
  GpLayout(Arena& a, int C, int U, int B) { mom = a.f64((size_t)B * (size_t)gp_moments(C, U)); }
};

inline bool gp_shape_ok(int C, int U, int B) { return C >= 1 && C <= GP_MAX_C && U >= 1 && U <= GP_MAX_U && B >= 1 && B <= 65535; }
inline bool gp_len_ok(int T) { return T >= 4 && T % 4 == 0; }
}  // namespace
}  // namespace sepr

extern "C" long long sepr_graph_pit_bytes(int C, int U, int B) {
  using namespace sepr;
  if (!gp_shape_ok(C, U, B)) return 0;
  return (long long)layout_bytes<GpLayout>(C, U, B);
}

extern "C" int sepr_graph_pit_assign(const float* const* est, const float* const* rows, const int* spans, const unsigned* adj, int C, int U, int B,
                                     int T, double eps, double snr_max, int* col, double* value, int* status, void* ws, size_t ws_bytes,
                                     sepr_stream_t stream) {
  using namespace sepr;
  if (!est || !rows || !spans || !adj || !col || !value || !status) return SEPR_EINVAL;
  if (!gp_shape_ok(C, U, B) || !gp_len_ok(T)) return SEPR_EINVAL;
  if (!(eps >= 0.0 && eps <= 1.0) || !(snr_max >= 0.0 && snr_max <= 300.0)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(spans) | reinterpret_cast<uintptr_t>(adj) | reinterpret_cast<uintptr_t>(col) |
       reinterpret_cast<uintptr_t>(status)) % 4 != 0 || reinterpret_cast<uintptr_t>(value) % 8 != 0)
    return SEPR_EINVAL;
  GpEst e = {};
  GpRows r = {};
  for (int c = 0; c < C; ++c) {
    if (!est[c] || reinterpret_cast<uintptr_t>(est[c]) % 4 != 0) return SEPR_EINVAL;
    e.p[c] = est[c];
  }
  for (int c = C; c < GP_MAX_C; ++c) e.p[c] = est[0];
  for (int u = 0; u < U; ++u) {
    if (!rows[u] || reinterpret_cast<uintptr_t>(rows[u]) % 4 != 0) return SEPR_EINVAL;
    r.p[u] = rows[u];
  }
  for (int u = U; u < GP_MAX_U; ++u) r.p[u] = rows[0];
  Arena arena(ws, ws_bytes);
  const GpLayout lay(arena, C, U, B);
  if (!arena.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double tau = pow(10.0, -snr_max / 10.0);
  hipLaunchKernelGGL(gp_moment_kernel, dim3((unsigned)gp_moments(C, U), (unsigned)B), dim3(GP_TPB), 0, st, e, r, spans, C, U, T, lay.mom);
  hipLaunchKernelGGL(gp_search_kernel, dim3((unsigned)B), dim3(GP_TPB), 0, st, lay.mom, spans, adj, C, U, T, eps, tau, col, value, status);
  SEPR_CHECK_LAUNCH("graph-PIT assignment kernels");
  return SEPR_OK;
}

extern "C" int sepr_graph_pit_assemble(const float* const* rows, const int* spans, const int* col, int C, int U, int B, int T, float* const* out,
                                       sepr_stream_t stream) {
  using namespace sepr;
  if (!rows || !spans || !col || !out) return SEPR_EINVAL;
  if (!gp_shape_ok(C, U, B) || !gp_len_ok(T)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(spans) | reinterpret_cast<uintptr_t>(col)) % 4 != 0) return SEPR_EINVAL;
  GpRows r = {};
  GpOut o = {};
  for (int u = 0; u < U; ++u) {
    if (!rows[u] || reinterpret_cast<uintptr_t>(rows[u]) % 16 != 0) return SEPR_EINVAL;      // float4 loads
    r.p[u] = rows[u];
  }
  for (int u = U; u < GP_MAX_U; ++u) r.p[u] = rows[0];
  for (int c = 0; c < C; ++c) {
    if (!out[c] || reinterpret_cast<uintptr_t>(out[c]) % 16 != 0) return SEPR_EINVAL;        // float4 stores
    o.p[c] = out[c];
  }
  for (int c = C; c < GP_MAX_C; ++c) o.p[c] = out[0];
  const int tiles = cdiv(T / 4, GP_TPB);
  if ((long long)tiles * B > 0x7fffffffLL) return SEPR_EINVAL;
  hipLaunchKernelGGL(gp_assemble_kernel, dim3((unsigned)(tiles * B)), dim3(GP_TPB), 0, static_cast<hipStream_t>(stream), r, spans, col, C, U, T,
                     tiles, o);
  SEPR_CHECK_LAUNCH("graph-PIT assemble kernel");
  return SEPR_OK;
}
