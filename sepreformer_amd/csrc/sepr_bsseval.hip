// BSS-eval source criteria (SDR / SIR / SAR) on the device, float64 throughout (mir_eval 0.7 bss_eval_sources,
// compute_permutation=True; reference utils/implements/criterions.py:264-289, PIT_SDRi).
//
// mir_eval projects the zero-padded estimate e onto the span of the references delayed by 0..F-1 (F = 512): normal
// equations G c = D with G[(i,a),(j,b)] = R_ij(a-b), R_ij(m) = sum_n s_i[n] s_j[n+m], D[(i,a)] = sum_n s_i[n-a] e[n].
// Every energy it forms is a projection energy, so with G = L L^T only a forward substitution is needed:
//   P_all = ||L^-1 D||^2 (joint Gram), P_j = ||L_jj^-1 D_j||^2 (the j-th diagonal block alone), E = ||e||^2
//   SDR = 10 log10(P_j / (E - P_j)),  SIR = 10 log10(P_j / (P_all - P_j)),  SAR = 10 log10(P_all / (E - P_all)).
// The forward substitution rides inside the factorisation: the right-hand sides are appended to the Gram as extra rows
// (a bordered matrix [G; D^T]), and the right-looking Cholesky turns those rows into (L^-1 D)^T on its own.  The leading
// F x F block of the joint factor is chol(G_00), so P_0 comes from the first F columns of the joint rows.
//
// Launches (all deterministic: fixed-order sums, no float atomics):
//   bss_corr_kernel     lagged correlations, one workgroup per (utterance, job, 256 lags); the whole valid length in
//                       1024-sample LDS windows, one lag per thread;
//   bss_gram_kernel     Toeplitz blocks of the joint Gram, of each G_jj (j >= 1) and the bordering rows;
//   per block step k:   bss_panel_kernel (factor the 64 x 64 diagonal block in LDS, then the panel below it by a
//                       triangular solve) and bss_update_kernel (the trailing update A_ij -= L_ik L_jk^T, one 64 x 64
//                       tile per workgroup, f64 VALU FMA);
//   bss_crit_kernel     energies, dB values, the S! permutation walk, the mixture row.
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr int BSS_F = 512;      // mir_eval's distortion-filter length (fixed in bss_eval_sources)
constexpr int BSS_NB = 64;      // Cholesky block
constexpr int BSS_LAGS = 256;   // lags per correlation workgroup
constexpr int BSS_CH = 1024;    // samples per LDS window of the correlation kernel
constexpr int BSS_LD = BSS_NB + 1;

__host__ __device__ constexpr int bss_np(int S) { return S * (S + 1) / 2; }                  // reference pairs i <= j
__host__ __device__ constexpr long long bss_ncorr(int S) { return (long long)bss_np(S) * 2 * BSS_F + (long long)(S + 1) * S * BSS_F; }
__host__ __device__ constexpr long long bss_mj(int S) { return (long long)(S * BSS_F + BSS_NB) * (S * BSS_F); }   // joint Gram + border
__host__ __device__ constexpr long long bss_ms() { return (long long)(BSS_F + BSS_NB) * BSS_F; }                  // one G_jj + border
__host__ __device__ constexpr long long bss_mats(int S) { return bss_mj(S) + (S - 1) * bss_ms(); }

__device__ __forceinline__ int bss_pair(int i, int j, int S) { return i * S - i * (i - 1) / 2 + (j - i); }   // i <= j

// problem p = b * S + q: q = 0 the joint Gram (S F columns), q >= 1 G_qq (F columns)
__device__ __forceinline__ double* bss_mat(double* mats, int S, int b, int q) {
  return mats + (long long)b * bss_mats(S) + (q == 0 ? 0 : bss_mj(S) + (long long)(q - 1) * bss_ms());
}

// out[l] = sum_{0 <= t < L} u[t] v[t + m0 + l] (v zero outside [0, L)), l < BSS_LAGS
template <int S>
__global__ __launch_bounds__(BSS_LAGS) void bss_corr_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                            const float* __restrict__ mix, const int* __restrict__ lens, int B, int T,
                                                            double* __restrict__ corr) {
  constexpr int NP = bss_np(S), RB = 2 * BSS_F / BSS_LAGS, DB = BSS_F / BSS_LAGS;
  const int b = blockIdx.y, L = lens[b];
  int x = blockIdx.x, m0;
  const float *u, *v;
  double* out = corr + (long long)b * bss_ncorr(S);
  if (x < NP * RB) {
    const int p = x / RB, blk = x % RB;
    int i = 0;
    while (p >= bss_pair(i + 1, i + 1, S) && i + 1 < S) ++i;
    const int j = i + (p - bss_pair(i, i, S));
    u = ref + ((long long)i * B + b) * T;
    v = ref + ((long long)j * B + b) * T;
    m0 = -BSS_F + blk * BSS_LAGS;
    out += (long long)p * 2 * BSS_F + blk * BSS_LAGS;
  } else {
    x -= NP * RB;
    const int job = x / DB, blk = x % DB, r = job / S, i = job % S;
    if (r == S && !mix) return;
    u = ref + ((long long)i * B + b) * T;
    v = r < S ? est + ((long long)r * B + b) * T : mix + (long long)b * T;
    m0 = blk * BSS_LAGS;
    out += (long long)NP * 2 * BSS_F + (long long)job * BSS_F + blk * BSS_LAGS;
  }
  __shared__ double us[BSS_CH];
  __shared__ double vs[BSS_CH + BSS_LAGS];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int t0 = 0; t0 < L; t0 += BSS_CH) {
    for (int q = tid; q < BSS_CH; q += BSS_LAGS) us[q] = t0 + q < L ? (double)u[t0 + q] : 0.0;
    for (int q = tid; q < BSS_CH + BSS_LAGS; q += BSS_LAGS) {
      const int t = t0 + m0 + q;
      vs[q] = (t >= 0 && t < L) ? (double)v[t] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int q = 0; q < BSS_CH; ++q) acc = fma(us[q], vs[q + tid], acc);
    __syncthreads();
  }
  out[tid] = acc;
}

// Gram blocks (lower block triangle, diagonal blocks whole) and the border rows (row n + r = D of right-hand side r:
// the S estimates, then the mixture; zero beyond).  grid (chunks, B * S), grid-stride over the problem's elements.
template <int S>
__global__ __launch_bounds__(256) void bss_gram_kernel(const double* __restrict__ corr, double* __restrict__ mats, int have_mix) {
  constexpr int NP = bss_np(S);
  const int b = blockIdx.y / S, q = blockIdx.y % S;
  const int n = q == 0 ? S * BSS_F : BSS_F;
  const long long tot = (long long)(n + BSS_NB) * n;
  const double* c = corr + (long long)b * bss_ncorr(S);
  double* A = bss_mat(mats, S, b, q);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(e / n), col = (int)(e % n);
    if (col / BSS_NB > row / BSS_NB) continue;                    // upper block triangle: never read
    const int j = q == 0 ? col / BSS_F : q, bb = col % BSS_F;
    double val;
    if (row < n) {
      const int i = q == 0 ? row / BSS_F : q, a = row % BSS_F, m = a - bb;
      val = i <= j ? c[(long long)bss_pair(i, j, S) * 2 * BSS_F + BSS_F + m] : c[(long long)bss_pair(j, i, S) * 2 * BSS_F + BSS_F - m];
    } else {
      const int r = row - n;
      val = (r < S || (r == S && have_mix)) ? c[(long long)NP * 2 * BSS_F + (long long)(r * S + j) * BSS_F + bb] : 0.0;
    }
    A[(long long)row * n + col] = val;
  }
}

// Step k: workgroup x = row block i - k (i in [k, nd]; i = nd is the border).  Every workgroup factors A_kk in LDS (64
// steps, cheaper than a launch); i == k records the pivot flag, i > k solves X L_kk^T = A_ik and overwrites A_ik with X.
template <int S>
__global__ __launch_bounds__(256) void bss_panel_kernel(double* __restrict__ mats, int k, int* __restrict__ flags) {
  const int b = blockIdx.y / S, q = blockIdx.y % S;
  const int n = q == 0 ? S * BSS_F : BSS_F, nd = n / BSS_NB, i = k + blockIdx.x;
  if (k >= nd || i > nd) return;
  double* A = bss_mat(mats, S, b, q);
  __shared__ double Lk[BSS_NB][BSS_LD];
  __shared__ double X[BSS_NB][BSS_LD];
  const int tid = threadIdx.x;
  const long long k0 = (long long)k * BSS_NB, i0 = (long long)i * BSS_NB;
  for (int e = tid; e < BSS_NB * BSS_NB; e += 256) Lk[e / BSS_NB][e % BSS_NB] = A[(k0 + e / BSS_NB) * n + k0 + e % BSS_NB];
  bool bad = false;
  for (int c = 0; c < BSS_NB; ++c) {
    __syncthreads();
    const double piv = Lk[c][c];
    bad |= !(piv > 0.0);                                          // never clamped: the utterance gets status 2
    const double inv = 1.0 / piv;
    for (int e = tid; e < BSS_NB * BSS_NB; e += 256) {
      const int r = e / BSS_NB, p = e % BSS_NB;
      if (p > c && p <= r) Lk[r][p] -= Lk[r][c] * Lk[p][c] * inv;
    }
    __syncthreads();
    if (tid >= c && tid < BSS_NB) Lk[tid][c] = tid == c ? sqrt(piv) : Lk[tid][c] / sqrt(piv);
  }
  __syncthreads();
  if (i == k) {                                                   // L_kk itself is never read again: A_kk stays as it was,
    if (tid == 0 && bad) flags[blockIdx.y] = 1;                   // so the sibling workgroups read an unfactored block
    return;
  }
  for (int e = tid; e < BSS_NB * BSS_NB; e += 256) X[e / BSS_NB][e % BSS_NB] = A[(i0 + e / BSS_NB) * n + k0 + e % BSS_NB];
  for (int c = 0; c < BSS_NB; ++c) {
    __syncthreads();
    if (tid < BSS_NB) X[tid][c] /= Lk[c][c];
    __syncthreads();
    for (int e = tid; e < BSS_NB * BSS_NB; e += 256) {
      const int r = e / BSS_NB, p = e % BSS_NB;
      if (p > c) X[r][p] -= X[r][c] * Lk[p][c];
    }
  }
  __syncthreads();
  for (int e = tid; e < BSS_NB * BSS_NB; e += 256) A[(i0 + e / BSS_NB) * n + k0 + e % BSS_NB] = X[e / BSS_NB][e % BSS_NB];
}

// Step k: A_ij -= L_ik L_jk^T for k < j <= i < nd, and for the border row block i = nd, k < j < nd.
template <int S>
__global__ __launch_bounds__(256) void bss_update_kernel(double* __restrict__ mats, int k) {
  const int b = blockIdx.y / S, q = blockIdx.y % S;
  const int n = q == 0 ? S * BSS_F : BSS_F, nd = n / BSS_NB, m = nd - k - 1;
  if (m <= 0) return;
  const int ntri = m * (m + 1) / 2, idx = blockIdx.x;
  if (idx >= ntri + m) return;
  int i, j;
  if (idx < ntri) {
    int ir = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
    while (ir * (ir + 1) / 2 > idx) --ir;
    while ((ir + 1) * (ir + 2) / 2 <= idx) ++ir;
    i = k + 1 + ir;
    j = k + 1 + (idx - ir * (ir + 1) / 2);
  } else {
    i = nd;
    j = k + 1 + (idx - ntri);
  }
  double* A = bss_mat(mats, S, b, q);
  __shared__ double Li[BSS_NB][BSS_LD];
  __shared__ double Lj[BSS_NB][BSS_LD];
  const int tid = threadIdx.x;
  const long long k0 = (long long)k * BSS_NB, i0 = (long long)i * BSS_NB, j0 = (long long)j * BSS_NB;
  for (int e = tid; e < BSS_NB * BSS_NB; e += 256) {
    const int r = e / BSS_NB, c = e % BSS_NB;
    Li[r][c] = A[(i0 + r) * n + k0 + c];
    Lj[r][c] = A[(j0 + r) * n + k0 + c];
  }
  __syncthreads();
  const int tr = (tid / 16) * 4, tc = (tid % 16) * 4;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
  for (int p = 0; p < BSS_NB; ++p) {
    double x[4], y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      x[a] = Li[tr + a][p];
      y[a] = Lj[tc + a][p];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = fma(x[a], y[c], acc[a][c]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) A[(i0 + tr + a) * n + j0 + tc + c] -= acc[a][c];
}

__device__ __forceinline__ double bss_db(double num, double den) {
  den = den > 0.0 ? den : 0.0;                                    // rounding may leave a tiny negative residual
  return den == 0.0 ? __builtin_huge_val() : 10.0 * log10(num / den);         // mir_eval _safe_db: a zero denominator is +inf
}

template <int S>
__global__ __launch_bounds__(256) void bss_crit_kernel(const float* __restrict__ est, const float* __restrict__ mix,
                                                       const int* __restrict__ lens, int B, int T, const double* __restrict__ corr,
                                                       double* __restrict__ mats, const int* __restrict__ flags, double* __restrict__ sdr,
                                                       double* __restrict__ sir, double* __restrict__ sar, int* __restrict__ perm,
                                                       double* __restrict__ sdr_mix, int* __restrict__ status) {
  constexpr int NR = S + 1;
  __shared__ double red[4];
  const int b = blockIdx.x, L = lens[b], tid = threadIdx.x, nj = S * BSS_F;
  double E[NR], Pall[NR], P[NR][S];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    E[r] = Pall[r] = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) P[r][j] = 0.0;
    if (r == S && !mix) continue;                                 // uniform
    const float* x = r < S ? est + ((long long)r * B + b) * T : mix + (long long)b * T;
    double s = 0.0;
    for (int t = tid; t < L; t += 256) s = fma((double)x[t], (double)x[t], s);
    E[r] = block_sum_d(s, red);
    const double* y = bss_mat(mats, S, b, 0) + (long long)(nj + r) * nj;
    double s0 = 0.0, s1 = 0.0;
    for (int c = tid; c < BSS_F; c += 256) s0 = fma(y[c], y[c], s0);
    for (int c = BSS_F + tid; c < nj; c += 256) s1 = fma(y[c], y[c], s1);
    P[r][0] = block_sum_d(s0, red);
    Pall[r] = P[r][0] + block_sum_d(s1, red);
#pragma unroll
    for (int j = 1; j < S; ++j) {
      const double* yj = bss_mat(mats, S, b, j) + (long long)(BSS_F + r) * BSS_F;
      double sj = 0.0;
      for (int c = tid; c < BSS_F; c += 256) sj = fma(yj[c], yj[c], sj);
      P[r][j] = block_sum_d(sj, red);
    }
  }
  if (tid != 0) return;
  int st = 0;
#pragma unroll
  for (int r = 0; r < NR; ++r) st = (r < S || mix) && E[r] == 0.0 ? 1 : st;
#pragma unroll
  for (int j = 0; j < S; ++j) st = corr[(long long)b * bss_ncorr(S) + (long long)bss_pair(j, j, S) * 2 * BSS_F + BSS_F] == 0.0 ? 1 : st;
  if (!st)
#pragma unroll
    for (int q = 0; q < S; ++q) st = flags[b * S + q] ? 2 : st;
  status[b] = st;
  double vsdr[NR][S], vsir[NR][S], vsar[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    vsar[r] = bss_db(Pall[r], E[r] - Pall[r]);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      vsdr[r][j] = bss_db(P[r][j], E[r] - P[r][j]);
      vsir[r][j] = bss_db(P[r][j], Pall[r] - P[r][j]);
    }
  }
  // itertools.permutations(range(S)) order; the first maximiser of mean_k SIR[popt[k], k] (np.argmax over np.mean)
  double best;
  const int popt = pit_walk_max<S>([&](int p) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < S; ++k) s += vsir[perm_at<S>(p, k)][k];
    return s / S;
  }, best);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const int e = perm_at<S>(popt, k);
    double osdr = vsdr[0][k], osir = vsir[0][k], osar = vsar[0];
#pragma unroll
    for (int r = 1; r < S; ++r) {                                 // row e by selects over constant indices: the tables stay in registers
      osdr = r == e ? vsdr[r][k] : osdr;
      osir = r == e ? vsir[r][k] : osir;
      osar = r == e ? vsar[r] : osar;
    }
    sdr[b * S + k] = st ? nan : osdr;
    sir[b * S + k] = st ? nan : osir;
    sar[b * S + k] = st ? nan : osar;
    perm[b * S + k] = e;
    if (sdr_mix) sdr_mix[b * S + k] = st ? nan : vsdr[S][k];     // identical rows: every SIR ties, popt = identity
  }
}
struct BssWs {   // two blocks, each split with no alignment inside: correlations [B][ncorr] | Gram systems [B][mats]; lengths [B] | a flag per (b, s)
  double *corr, *mats;
  int *lens, *flags;
  BssWs(Arena& a, int S, int B) {
    corr = a.f64((size_t)B * (size_t)(bss_ncorr(S) + bss_mats(S))); mats = corr + (long long)B * bss_ncorr(S);
    lens = a.of<int>((size_t)B * (S + 1)); flags = lens + B;
  }
};
}  // namespace
}  // namespace sepr

extern "C" size_t sepr_bss_eval_workspace(int S, int B, int T) {
  using namespace sepr;
  if (S < 2 || S > 3 || B <= 0 || T < S * BSS_F) return 0;
  return layout_bytes<BssWs>(S, B);
}

extern "C" int sepr_bss_eval_fwd(const float* est, const float* ref, const float* mix, const int* lengths, int S, int B, int T,
                                 double* sdr, double* sir, double* sar, int* perm, double* sdr_mix, int* status, void* ws,
                                 size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!est || !ref || !lengths || !sdr || !sir || !sar || !perm || !status) return SEPR_EINVAL;
  if (S < 2 || S > 3 || B <= 0 || B * S > 65535 || T < S * BSS_F) return SEPR_EINVAL;
  if (!mix && sdr_mix) return SEPR_EINVAL;
  for (int b = 0; b < B; ++b)
    if (lengths[b] < S * BSS_F || lengths[b] > T) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  const BssWs wk(ar, S, B);
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(wk.lens, lengths, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(wk.flags, 0, (size_t)B * S * sizeof(int), st);
  if (e != hipSuccess) {
    set_hip_error(e, "bss_eval setup");
    return SEPR_EHIP;
  }
  const int have_mix = mix ? 1 : 0;
  const int nd = S * BSS_F / BSS_NB;
#define SEPR_BSS_CASE(SS)                                                                                                      \
  case SS: {                                                                                                                   \
    const int nblk = bss_np(SS) * (2 * BSS_F / BSS_LAGS) + (SS + 1) * SS * (BSS_F / BSS_LAGS);                                 \
    hipLaunchKernelGGL((bss_corr_kernel<SS>), dim3(nblk, B), dim3(BSS_LAGS), 0, st, est, ref, mix, wk.lens, B, T, wk.corr);         \
    hipLaunchKernelGGL((bss_gram_kernel<SS>), dim3(256, B * SS), dim3(256), 0, st, wk.corr, wk.mats, have_mix);                     \
    for (int k = 0; k < nd; ++k) {                                                                                             \
      hipLaunchKernelGGL((bss_panel_kernel<SS>), dim3(nd + 1 - k, B * SS), dim3(256), 0, st, wk.mats, k, wk.flags);                 \
      const int m = nd - k - 1;                                                                                                \
      if (m > 0) hipLaunchKernelGGL((bss_update_kernel<SS>), dim3(m * (m + 1) / 2 + m, B * SS), dim3(256), 0, st, wk.mats, k);    \
    }                                                                                                                          \
    hipLaunchKernelGGL((bss_crit_kernel<SS>), dim3(B), dim3(256), 0, st, est, mix, wk.lens, B, T, wk.corr, wk.mats, wk.flags, sdr, sir,   \
                       sar, perm, sdr_mix, status);                                                                            \
  } break;
  switch (S) {
    SEPR_BSS_CASE(2)
    SEPR_BSS_CASE(3)
    default: return SEPR_EINVAL;
  }
#undef SEPR_BSS_CASE
  SEPR_CHECK_LAUNCH("bss_eval kernels");
  return SEPR_OK;
}
