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
//   stream_step_kernel   the stream bank: the same stitch one boundary at a time, for streams whose
//                        length is not known yet.  One workgroup per stream of the hop: statistics over the saved tail and the
//                        new window's head (stitch_overlap_stats, shared with stitch_stats_kernel), the decision
//                        (stitch_choose, shared with stitch_plan_kernel), the emission of the samples that became final, and
//                        the new tail, P and float64 g saved in the stream's slot;
//   stream_gather_kernel the [A][W] input of a hop from the streams' rings of pending samples, zero past what was received.
// Nothing here uses atomics or depends on the launch order of workgroups: results are bit-identical from run to run.
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr double STITCH_DELTA = 1e-20;      // added to Ea * Eb inside the square root of the normalised correlation
constexpr double STITCH_SILENCE = 1e-10;    // gain carried when Ea / O or Eb / O (mean square per sample) is below this
constexpr double STITCH_RHO_MIN = 0.5;      // gain carried when the normalised correlation of the matched pair is below this
constexpr int STITCH_TPB = 256;

__host__ __device__ constexpr int stitch_ns(int S) { return S * S + 2 * S; }

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

// The overlap statistics of one boundary, by one workgroup of STITCH_TPB threads: a[i] / b[j] point at the O overlap samples of source i of
// the outgoing window and of source j of the incoming one.  Thread tid takes the quads 4 tid, 4 tid + 1024, ... in one fma chain per
// statistic, then the wave sums and the fixed tree over the four waves.  put(v, value) receives statistic v < NS (C row-major, Ea, Eb) from thread v.
// Both the offline kernel and the stream step call this: a boundary's statistics have one definition and one order.
// RowsA / RowsB say where source i's overlap samples lie: rows(i, q) = the address of sample q of source i.
struct StridedRows {                        // rows of one buffer, ld apart
  const float* p;
  int ld;
  __device__ __forceinline__ const float* operator()(int i, int q) const { return p + (long long)i * ld + q; }
};
template <int S>
struct PointerRows {                        // one pointer per source
  const float* p[S];
  __device__ __forceinline__ const float* operator()(int i, int q) const { return p[i] + q; }
};
template <int S, class RowsA, class RowsB, class Put>
__device__ __forceinline__ void stitch_overlap_stats(RowsA a, RowsB b, int O, int tid, Put put) {
  constexpr int NS = stitch_ns(S);
  double acc[NS];
#pragma unroll
  for (int v = 0; v < NS; ++v) acc[v] = 0.0;
  for (int q = 4 * tid; q < O; q += 4 * STITCH_TPB) {
    float4 av[S], bv[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      av[i] = ld4(a(i, q));
      bv[i] = ld4(b(i, q));
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
  if (tid < NS) put(tid, ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]);
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
  stitch_overlap_stats<S>(StridedRows{a, W}, StridedRows{b, W}, O, tid, [&](int v, double x) { stats[(long long)k * NS + v] = x; });
}

// One boundary's decision from its statistics st = (C row-major, Ea, Eb): the lexicographically first maximiser of the summed normalised
// correlations (-> its index in perm_at's order) and the gain ratio of each outgoing source under it (1 = carried).
template <int S>
__device__ __forceinline__ int stitch_choose(const double* st, int O, int match_gain, double (&ratio)[S]) {
#pragma clang fp contract(off)
  double C[S * S], Ea[S], Eb[S];
#pragma unroll
  for (int v = 0; v < S * S; ++v) C[v] = st[v];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    Ea[i] = st[S * S + i];
    Eb[i] = st[S * S + S + i];
  }
  double best = 0.0;
  int bp = 0;
#pragma unroll
  for (int p = 0; p < perm_count<S>(); ++p) {
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
  return bp;
}

template <int S>
__global__ __launch_bounds__(64) void stitch_plan_kernel(const double* __restrict__ stats, const int* __restrict__ coff, int O,
                                                         int match_gain, int* __restrict__ perm, float* __restrict__ gain) {
#pragma clang fp contract(off)
  constexpr int NS = stitch_ns(S);
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
      double ratio[S];
      const int bp = stitch_choose<S>(stats + (long long)(k0 + kk) * NS, O, match_gain, ratio);
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
// ---- the stream bank: the same stitch, one boundary per launch, its state on the device ---------------------
// A slot's state: the raw last O samples of its latest window (all S sources, un-permuted), its track permutation P and its gains g in
// float64.  One workgroup serves one stream of the launch and does everything for it in order - statistics, decision, emission, save -
// so no other workgroup ever reads a field this one writes (two barriers order the reads of the old tail before its overwrite).
constexpr int STREAM_COLS = 6;              // step table row: slot, k, n_emit, has_window, out offset, track stride (int64)
constexpr int GATHER_COLS = 3;              // gather table row: base of the stream's ring in the store, first sample, samples received

template <int S>
struct StreamWin {
  const float* p[S];                        // source s of the hop's windows: [A][ld]
};

template <int S, class T>
__device__ __forceinline__ T pick(const T (&v)[S], int i) {
  T r = v[0];
#pragma unroll
  for (int s = 1; s < S; ++s) r = i == s ? v[s] : r;
  return r;
}

struct StreamState {
  float* tail;        // [slots][S][O]
  int* P;             // [slots][S]
  double* g;          // [slots][S]
  StreamState(Arena& a, int slots, int S, int O) {
    tail = a.f32((size_t)slots * S * O); P = a.of<int>((size_t)slots * S); g = a.f64((size_t)slots * S);
  }
};

template <int S>
__global__ __launch_bounds__(STITCH_TPB) void stream_step_kernel(StreamWin<S> win, long long ld, const long long* __restrict__ table,
                                                                 int slots, int W, int O, int match_gain, float* __restrict__ out,
                                                                 long long out_elems, int* __restrict__ perm, float* __restrict__ gain,
                                                                 float* tails, int* sP, double* sg) {
#pragma clang fp contract(off)
  constexpr int NS = stitch_ns(S);
  const int a = blockIdx.x, tid = threadIdx.x, H = W - O;
  const long long* row = table + (long long)a * STREAM_COLS;
  // a bad table gives wrong samples, never an access outside the state, the windows or the emission buffer
  long long slot = row[0];
  slot = slot < 0 ? 0 : (slot >= slots ? slots - 1 : slot);
  const bool first = row[1] <= 0, has = row[3] != 0;
  long long ne = row[2];
  const int cap = has ? W : O;
  ne = ne < 0 ? 0 : (ne > cap ? cap : ne);
  const int n_emit = (int)ne, n4 = (n_emit + 3) & ~3;
  const long long off = row[4], ts = row[5];
  const bool emit = off >= 0 && off <= out_elems && ts >= n4 && ts <= out_elems && ((off | ts) & 3) == 0 &&
                    off + (S - 1) * ts + n4 <= out_elems;
  float* tail = tails + slot * S * O;
  const float* w[S];
#pragma unroll
  for (int s = 0; s < S; ++s) w[s] = win.p[s] + (long long)a * ld;
  int Po[S], Pn[S];
  double go[S], gn[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int p = first ? s : sP[slot * S + s];
    Po[s] = p < 0 ? 0 : (p >= S ? S - 1 : p);
    go[s] = first ? 1.0 : sg[slot * S + s];
    Pn[s] = Po[s];
    gn[s] = go[s];
  }
  if (has && !first) {                                            // uniform over the workgroup
    __shared__ double st[NS];
    PointerRows<S> b;
#pragma unroll
    for (int i = 0; i < S; ++i) b.p[i] = w[i];
    stitch_overlap_stats<S>(StridedRows{tail, O}, b, O, tid, [&](int v, double x) { st[v] = x; });
    __syncthreads();
    double ratio[S];
    const int p = stitch_choose<S>(st, O, match_gain, ratio);     // every thread takes the same decision from the same numbers
#pragma unroll
    for (int s = 0; s < S; ++s) {
      gn[s] = go[s] * pick<S>(ratio, Po[s]);
      Pn[s] = perm_at<S>(p, Po[s]);
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      perm[(long long)a * S + s] = Pn[s];
      gain[(long long)a * S + s] = (float)gn[s];
    }
  }
  if (emit) {
    for (int q = 4 * tid; q < n4; q += 4 * STITCH_TPB) {
      const bool fade = has && !first && q < O;                   // O is a multiple of 4: a quad never straddles the overlap's end
      float wi[4] = {1.f, 1.f, 1.f, 1.f};
      if (fade) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double sn = sin(3.14159265358979323846 * ((double)(q + u) + 0.5) / (2.0 * O));
          wi[u] = (float)(sn * sn);
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float gi = (float)gn[s];
        const float4 ci = has ? ld4(pick<S>(w, Pn[s]) + q) : ld4(tail + (long long)Pn[s] * O + q);
        float v[4] = {gi * ci.x, gi * ci.y, gi * ci.z, gi * ci.w};
        if (fade) {
          const float gout = (float)go[s];
          const float4 co = ld4(tail + (long long)Po[s] * O + q);
          const float cin[4] = {ci.x, ci.y, ci.z, ci.w}, cout[4] = {co.x, co.y, co.z, co.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float wout = 1.0f - wi[u];
            v[u] = fmaf(wi[u] * gi, cin[u], (wout * gout) * cout[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = q + u < n_emit ? v[u] : 0.f;
        st4(out + off + s * ts + q, make_float4(v[0], v[1], v[2], v[3]));
      }
    }
  }
  if (!has) return;                                               // the flush form leaves the state as it is
  __syncthreads();                                                // every read of the old tail is done
  for (int q = 4 * tid; q < O; q += 4 * STITCH_TPB) {
#pragma unroll
    for (int s = 0; s < S; ++s) st4(tail + (long long)s * O + q, ld4(w[s] + H + q));
  }
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      sP[slot * S + s] = Pn[s];
      sg[slot * S + s] = gn[s];
    }
  }
}

// x[a][0 .. W) = samples [start, start + W) of the stream whose ring of `cap` samples begins at store + base; zero from `received` on
__global__ __launch_bounds__(STITCH_TPB) void stream_gather_kernel(const float* __restrict__ store, long long store_elems, long long cap,
                                                                   const long long* __restrict__ table, int W, float* __restrict__ x) {
  const int a = blockIdx.y, q = 4 * (blockIdx.x * STITCH_TPB + threadIdx.x);
  if (q >= W) return;
  const long long* row = table + (long long)a * GATHER_COLS;
  const long long base = row[0], start = row[1], recv = row[2];
  const bool ok = base >= 0 && (base & 3) == 0 && base <= store_elems - cap && start >= 0 && (start & 3) == 0;
  float4 v = zero4();
  if (ok) {
    const long long pos = start + q;
    const float4 c = ld4(store + base + pos % cap);              // cap, start and q are multiples of 4: a quad never wraps
    v = make_float4(pos < recv ? c.x : 0.f, pos + 1 < recv ? c.y : 0.f, pos + 2 < recv ? c.z : 0.f, pos + 3 < recv ? c.w : 0.f);
  }
  st4(x + (long long)a * W + q, v);
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

extern "C" long long sepr_streambank_state_bytes(int slots, int S, int O) {
  using namespace sepr;
  if (S < 2 || S > 3 || slots < 1 || slots > (1 << 20) || O <= 0 || O % 4 != 0) return 0;
  return (long long)layout_bytes<StreamState>(slots, S, O);
}

extern "C" int sepr_streambank_step(const float* const* win, long long ld, const long long* table, int A, int slots, int S, int W, int O,
                                    int match_gain, float* out, long long out_elems, int* perm, float* gain, void* state,
                                    size_t state_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!win || !table || !out || !perm || !gain) return SEPR_EINVAL;
  if (S < 2 || S > 3 || A < 1 || slots < 1 || slots > (1 << 20)) return SEPR_EINVAL;
  if (W <= 0 || W % 4 != 0 || O <= 0 || O % 4 != 0 || 2LL * O > W) return SEPR_EINVAL;
  if (ld < W || ld % 4 != 0 || out_elems < 4 || (long long)A * ld > (1LL << 40)) return SEPR_EINVAL;
  for (int s = 0; s < S; ++s)
    if (!win[s] || reinterpret_cast<uintptr_t>(win[s]) % 16 != 0) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(state)) % 16 != 0) return SEPR_EINVAL;     // float4 access
  if (reinterpret_cast<uintptr_t>(table) % 8 != 0) return SEPR_EINVAL;
  Arena ar(state, state_bytes);
  const StreamState k(ar, slots, S, O);
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int mg = match_gain ? 1 : 0;
  if (S == 2) {
    const StreamWin<2> w{{win[0], win[1]}};
    hipLaunchKernelGGL((stream_step_kernel<2>), dim3(A), dim3(STITCH_TPB), 0, st, w, ld, table, slots, W, O, mg, out, out_elems, perm, gain,
                       k.tail, k.P, k.g);
  } else {
    const StreamWin<3> w{{win[0], win[1], win[2]}};
    hipLaunchKernelGGL((stream_step_kernel<3>), dim3(A), dim3(STITCH_TPB), 0, st, w, ld, table, slots, W, O, mg, out, out_elems, perm, gain,
                       k.tail, k.P, k.g);
  }
  SEPR_CHECK_LAUNCH("stream step kernel");
  return SEPR_OK;
}

extern "C" int sepr_streambank_gather(const float* store, long long store_elems, long long cap, const long long* table, int A, int W,
                                      float* x, sepr_stream_t stream) {
  using namespace sepr;
  if (!store || !table || !x) return SEPR_EINVAL;
  if (A < 1 || A > 65535 || W <= 0 || W % 4 != 0 || cap < W || cap % 4 != 0 || store_elems < cap) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(x)) % 16 != 0) return SEPR_EINVAL;       // float4 access
  if (reinterpret_cast<uintptr_t>(table) % 8 != 0) return SEPR_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)((W / 4 + STITCH_TPB - 1) / STITCH_TPB), (unsigned)A), dim3(STITCH_TPB), 0, st,
                     store, store_elems, cap, table, W, x);
  SEPR_CHECK_LAUNCH("stream gather kernel");
  return SEPR_OK;
}
