// Long-form separation: the boundary alignment and overlap-add of overlapping chunk outputs.
//
// A recording of T samples is cut into Nc = 1 + ceil((T - W) / H) windows of W samples at hop H = W - O (one window when
// T <= W; only the last one is zero-padded past T).  The separator runs the windows as a batch; these kernels put the S
// outputs of every window back together:
//   stitch_stats_kernel  one workgroup per boundary k | k+1 of a recording: C[i][j] = <a_i, b_j>, Ea[i] = <a_i, a_i>,
//                        Eb[j] = <b_j, b_j> in float64 over the O overlap samples (a = the last O samples of chunk k,
//                        b = the first O of chunk k+1), float4 loads, a fixed per-thread order and a fixed tree;
//   stitch_plan_kernel   one wave per recording: each lane scores the S! permutations of one boundary (lexicographic
//                        order, the first maximiser of sum_i |C[i][pi(i)]| / sqrt(Ea[i] Eb[pi(i)] + delta)) and its
//                        least-squares gain ratios; lane 0 then composes the tracks boundary by boundary
//                        (P_{k+1}(s) = pi_k(P_k(s)), g_{k+1}(s) = g_k(s) * ratio_k[P_k(s)]) and writes perm / gain;
//   stitch_ola_kernel    one thread per four output samples: at most two chunks read, sin^2 crossfade over the overlap,
//                        one float4 store.
// Nothing here uses atomics or depends on the launch order of workgroups: results are bit-identical from run to run.
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr double STITCH_DELTA = 1e-20;      // added to Ea * Eb inside the square root of the normalised correlation
constexpr double STITCH_SILENCE = 1e-10;    // gain carried when Ea / O or Eb / O (mean square per sample) is below this
constexpr double STITCH_RHO_MIN = 0.5;      // gain carried when the normalised correlation of the matched pair is below this
constexpr int STITCH_TPB = 256;

__host__ __device__ constexpr int stitch_ns(int S) { return S * S + 2 * S; }

// pi(i) of permutation p in lexicographic order (S = 2: 01 10; S = 3: 012 021 102 120 201 210)
template <int S>
__host__ __device__ constexpr int perm_at(int p, int i) {
  if (S == 2) return i == 0 ? p : 1 - p;
  const int first = p >> 1, lo = first == 0 ? 1 : 0, hi = first == 2 ? 1 : 2;
  return i == 0 ? first : (i == 1 ? ((p & 1) ? hi : lo) : ((p & 1) ? lo : hi));
}

// largest r in [0, R) with coff[r] <= k (coff non-decreasing, coff[0] = 0 <= k)
__device__ __forceinline__ int find_rec_chunk(const int* __restrict__ coff, int R, long long k) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (coff[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// largest r in [0, R) whose output region starts at or before element e: base(r) = S (coff[r] H + r O)
__device__ __forceinline__ int find_rec_out(const int* __restrict__ coff, int R, int S, int H, int O, long long e) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)S * ((long long)coff[mid] * H + (long long)mid * O) <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int S>
__global__ __launch_bounds__(STITCH_TPB) void stitch_stats_kernel(const float* __restrict__ chunks, const int* __restrict__ coff, int R,
                                                                  int W, int O, double* __restrict__ stats) {
  constexpr int NS = stitch_ns(S);
  const int k = blockIdx.x;
  const int r = find_rec_chunk(coff, R, k);
  if (k + 1 >= coff[r + 1]) return;                               // the last chunk of its recording: no boundary
  const int H = W - O, tid = threadIdx.x;
  const float* a = chunks + (long long)k * S * W + H;
  const float* b = chunks + (long long)(k + 1) * S * W;
  double acc[NS];
#pragma unroll
  for (int v = 0; v < NS; ++v) acc[v] = 0.0;
  for (int q = 4 * tid; q < O; q += 4 * STITCH_TPB) {
    float4 av[S], bv[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      av[i] = ld4(a + (long long)i * W + q);
      bv[i] = ld4(b + (long long)i * W + q);
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        double c = acc[i * S + j];
        c = fma((double)av[i].x, (double)bv[j].x, c);
        c = fma((double)av[i].y, (double)bv[j].y, c);
        c = fma((double)av[i].z, (double)bv[j].z, c);
        acc[i * S + j] = fma((double)av[i].w, (double)bv[j].w, c);
      }
      double ea = acc[S * S + i], eb = acc[S * S + S + i];
      ea = fma((double)av[i].x, (double)av[i].x, ea);
      ea = fma((double)av[i].y, (double)av[i].y, ea);
      ea = fma((double)av[i].z, (double)av[i].z, ea);
      acc[S * S + i] = fma((double)av[i].w, (double)av[i].w, ea);
      eb = fma((double)bv[i].x, (double)bv[i].x, eb);
      eb = fma((double)bv[i].y, (double)bv[i].y, eb);
      eb = fma((double)bv[i].z, (double)bv[i].z, eb);
      acc[S * S + S + i] = fma((double)bv[i].w, (double)bv[i].w, eb);
    }
  }
  __shared__ double red[STITCH_TPB / 64][NS];
#pragma unroll
  for (int v = 0; v < NS; ++v) {
    const double w = wave_sum_d(acc[v]);
    if ((tid & 63) == 0) red[tid >> 6][v] = w;
  }
  __syncthreads();
  if (tid < NS) stats[(long long)k * NS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

template <int S>
__global__ __launch_bounds__(64) void stitch_plan_kernel(const double* __restrict__ stats, const int* __restrict__ coff, int O,
                                                         int match_gain, int* __restrict__ perm, float* __restrict__ gain) {
#pragma clang fp contract(off)
  constexpr int NS = stitch_ns(S), NP = S == 2 ? 2 : 6;
  __shared__ int spi[64];
  __shared__ double sratio[64][S];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int k0 = coff[r], nb = coff[r + 1] - k0 - 1;              // boundaries of this recording
  int P[S];
  double g[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    P[s] = s;
    g[s] = 1.0;
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      perm[(long long)k0 * S + s] = s;
      gain[(long long)k0 * S + s] = 1.0f;
    }
  }
  for (int base = 0; base < nb; base += 64) {
    const int kk = base + lane;
    if (kk < nb) {
      const double* st = stats + (long long)(k0 + kk) * NS;
      double C[S * S], Ea[S], Eb[S];
#pragma unroll
      for (int v = 0; v < S * S; ++v) C[v] = st[v];
#pragma unroll
      for (int i = 0; i < S; ++i) {
        Ea[i] = st[S * S + i];
        Eb[i] = st[S * S + S + i];
      }
      double best = 0.0, ratio[S];
      int bp = 0;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        double score = 0.0, rat[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
          const int j = perm_at<S>(p, i);
          const double rho = fabs(C[i * S + j]) / sqrt(Ea[i] * Eb[j] + STITCH_DELTA);
          score += rho;
          const double q = C[i * S + j] / Eb[j];
          const bool carry = !match_gain || Ea[i] / O < STITCH_SILENCE || Eb[j] / O < STITCH_SILENCE || rho < STITCH_RHO_MIN ||
                             !__builtin_isfinite(q);
          rat[i] = carry ? 1.0 : q;
        }
        if (p == 0 || score > best) {                             // ties keep the lexicographically first
          best = score;
          bp = p;
#pragma unroll
          for (int i = 0; i < S; ++i) ratio[i] = rat[i];
        }
      }
      spi[lane] = bp;
#pragma unroll
      for (int i = 0; i < S; ++i) sratio[lane][i] = ratio[i];
    }
    __syncthreads();
    if (lane == 0) {
      const int n = nb - base < 64 ? nb - base : 64;
      for (int l = 0; l < n; ++l) {
        const int p = spi[l];
        const long long o = (long long)(k0 + base + l + 1) * S;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          g[s] = g[s] * sratio[l][P[s]];
          P[s] = perm_at<S>(p, P[s]);
          perm[o + s] = P[s];
          gain[o + s] = (float)g[s];
        }
      }
    }
    __syncthreads();
  }
}

// y of recording r, track s: y + S (coff[r] H + r O) + s (Nc H + O), Nc H + O samples (>= T; zero from T on)
template <int S>
__global__ __launch_bounds__(STITCH_TPB) void stitch_ola_kernel(const float* __restrict__ chunks, const int* __restrict__ coff,
                                                                const int* __restrict__ lens, int R, int W, int O,
                                                                const int* __restrict__ perm, const float* __restrict__ gain,
                                                                float* __restrict__ y, long long nquads) {
#pragma clang fp contract(off)
  const long long qd = (long long)blockIdx.x * STITCH_TPB + threadIdx.x;
  if (qd >= nquads) return;
  const int H = W - O;
  const long long e = 4 * qd;
  const int r = find_rec_out(coff, R, S, H, O, e);
  const int k0 = coff[r], nc = coff[r + 1] - k0, T = lens[r];
  const long long base = (long long)S * ((long long)k0 * H + (long long)r * O), row = (long long)nc * H + O;
  const long long rel = e - base;
  const int s = (int)(rel / row), t0 = (int)(rel - s * row);
  float4 out = zero4();
  if (t0 < T) {
    int k = t0 / H;
    k = k < nc - 1 ? k : nc - 1;
    const int j = t0 - k * H;                                     // a multiple of 4: a quad never straddles a region
    const long long ki = (long long)(k0 + k) * S + s;
    const float gi = gain[ki];
    const float4 ci = ld4(chunks + ((long long)(k0 + k) * S + perm[ki]) * W + j);
    float v[4] = {gi * ci.x, gi * ci.y, gi * ci.z, gi * ci.w};
    if (k > 0 && j < O) {                                         // overlap of boundary k - 1 at offset j
      const long long ko = ki - S;
      const float go = gain[ko];
      const float4 co = ld4(chunks + ((long long)(k0 + k - 1) * S + perm[ko]) * W + H + j);
      const float cin[4] = {ci.x, ci.y, ci.z, ci.w}, cout[4] = {co.x, co.y, co.z, co.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double sn = sin(3.14159265358979323846 * ((double)(j + u) + 0.5) / (2.0 * O));
        const float win = (float)(sn * sn), wout = 1.0f - win;
        v[u] = fmaf(win * gi, cin[u], (wout * go) * cout[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = t0 + u < T ? v[u] : 0.f;
    out = make_float4(v[0], v[1], v[2], v[3]);
  }
  st4(y + e, out);
}
struct StitchWs {
  double* stats;      // [total chunks][stitch_ns(S)] overlap statistics
  int *coff, *lens;   // device copies of chunk_offset [R + 1] and lengths [R]
  StitchWs(Arena& a, int R, int total, int S) {
    stats = a.f64((size_t)total * stitch_ns(S)); coff = a.of<int>((size_t)(R + 1)); lens = a.of<int>((size_t)R);
  }
};
}  // namespace
}  // namespace sepr

extern "C" size_t sepr_stitch_workspace(int R, int total_chunks, int S) {
  using namespace sepr;
  if (S < 2 || S > 3 || R <= 0 || total_chunks < R) return 0;
  return layout_bytes<StitchWs>(R, total_chunks, S);
}

extern "C" int sepr_stitch_fwd(const float* chunks, const int* chunk_offset, const int* lengths, int R, int S, int W, int O,
                               int match_gain, float* y, int* perm, float* gain, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!chunks || !chunk_offset || !lengths || !y || !perm || !gain) return SEPR_EINVAL;
  if (S < 2 || S > 3 || R <= 0 || R > (1 << 30)) return SEPR_EINVAL;
  if (W <= 0 || W % 4 != 0 || O <= 0 || O % 4 != 0 || 2LL * O > W) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(chunks) | reinterpret_cast<uintptr_t>(y)) % 16 != 0) return SEPR_EINVAL;     // float4 access
  const int H = W - O;
  if (chunk_offset[0] != 0) return SEPR_EINVAL;
  for (int r = 0; r < R; ++r) {
    const long long T = lengths[r], nc = (long long)chunk_offset[r + 1] - chunk_offset[r];
    if (T <= 0) return SEPR_EINVAL;
    const long long want = T <= W ? 1 : 1 + (T - W + H - 1) / H;
    if (nc != want) return SEPR_EINVAL;                           // also catches non-monotone offsets (nc >= 1)
  }
  const int total = chunk_offset[R];
  if ((long long)S * ((long long)total * H + (long long)R * O) / 4 > (long long)STITCH_TPB * 0x7fffffffLL) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  const StitchWs k(ar, R, total, S);
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(k.coff, chunk_offset, (size_t)(R + 1) * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(k.lens, lengths, (size_t)R * sizeof(int), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    set_hip_error(e, "stitch setup");
    return SEPR_EHIP;
  }
  const long long nquads = (long long)S * ((long long)total * H + (long long)R * O) / 4;
  const int mg = match_gain ? 1 : 0;
#define SEPR_STITCH_CASE(SS)                                                                                                   \
  case SS:                                                                                                                     \
    if (total > R)                                                                                                             \
      hipLaunchKernelGGL((stitch_stats_kernel<SS>), dim3(total), dim3(STITCH_TPB), 0, st, chunks, k.coff, R, W, O, k.stats);     \
    hipLaunchKernelGGL((stitch_plan_kernel<SS>), dim3(R), dim3(64), 0, st, k.stats, k.coff, O, mg, perm, gain);                  \
    hipLaunchKernelGGL((stitch_ola_kernel<SS>), dim3((unsigned)((nquads + STITCH_TPB - 1) / STITCH_TPB)), dim3(STITCH_TPB), 0, \
                       st, chunks, k.coff, k.lens, R, W, O, perm, gain, y, nquads);                                               \
    break;
  switch (S) {
    SEPR_STITCH_CASE(2)
    SEPR_STITCH_CASE(3)
    default: return SEPR_EINVAL;
  }
#undef SEPR_STITCH_CASE
  SEPR_CHECK_LAUNCH("stitch kernels");
  return SEPR_OK;
}
