// Permutation-invariant SI-SNR on the device.
//
// reference: utils/implements/criterions.py
//   PIT_SISNR_time.__call__  :191-217   loss  = mean_b min_perm sum_s clamp(-SISNR(est_s, tgt_perm(s)), min=-30)
//   PIT_SISNRi.__call__      :232-260   score = max_perm sum_s (SISNR(est_s, tgt_p(s)) - SISNR(mix, tgt_p(s)))
//   SISNR(a, t) = 20 log10(eps + |alpha t~| / (|a~ - alpha t~| + eps)),  alpha = <a~,t~> / (|t~|^2 + eps),  ~ = zero-mean
//
// Everything above is a function of 2S+1 sums, 2S+1 sums of squares and S*S + S cross sums per utterance, so the
// waveforms are read exactly once (20 B per sample for S = 2; HBM-bound, ~3 us for 32 x 32000 samples):
//   pit_partial_kernel   one workgroup per (4096-sample chunk, utterance): fp64 accumulators, wave butterfly +
//                        LDS combine, fixed order -> bitwise deterministic; partials to the workspace;
//   pit_finalize_kernel  one wave per utterance: sums the chunk partials in chunk order, forms the zero-mean
//                        moments, the S x S SI-SNR matrix and the mixture row, walks the S! permutations.
// fp64 throughout: the residual energy |a~|^2 - 2 alpha <a~,t~> + alpha^2 |t~|^2 cancels ~3 digits at 30 dB, which
// fp32 moments could not afford; with fp64 moments the result is the exact-arithmetic value to ~1e-9 dB (the
// reference's own fp32 evaluation differs from that by up to ~1e-3 dB at high SI-SNR).
//
// Beyond the reference: the source-aggregated, soft-thresholded SDR (sepr_pit_sasdr_*) on the same moment pass, the same
// STFT projection and the same workspaces - a criterion that is defined when a target is silent throughout.
//
// What the eight entries share is stated once: the layout of the moment vector and the zero-mean moments with their clamp (pit_iq_*,
// PitMoments), the fold of the chunk partials (pit_fold_moments), the permutations and the walk over them (perm_at / pit_walk of
// sepr_common.h), the launch of the moment pass (launch_moments), the choice of the S instantiation (dispatch_S) and the forward launches
// of the magnitude forms, which their backward repeats (mag_forward_launches).
#include <type_traits>

#include "sepr_gemm_epi.h"

namespace sepr {

namespace {
constexpr int PIT_TPB = 256, PIT_CHUNK = 4096, PIT_SMAX = 3;
__host__ __device__ constexpr int pit_nchunk(int T) { return (T + PIT_CHUNK - 1) / PIT_CHUNK; }

// The moment vector q of one utterance (and of one chunk of it in the workspace), over the NV = 2S + 1 waveforms v: est_s = s, tgt_k = S + k,
// mix = 2S:  NV sums | NV sums of squares | S x S cross sums est_s . tgt_k, row-major | S cross sums mix . tgt_k
__host__ __device__ constexpr int pit_iq_sum(int S, int v) { return v; }
__host__ __device__ constexpr int pit_iq_sq(int S, int v) { return (2 * S + 1) + v; }
__host__ __device__ constexpr int pit_iq_at(int S, int s, int k) { return 2 * (2 * S + 1) + s * S + k; }
__host__ __device__ constexpr int pit_iq_xt(int S, int k) { return 2 * (2 * S + 1) + S * S + k; }
__host__ __device__ constexpr int pit_nq(int S) { return pit_iq_xt(S, S); }

// The zero-mean moments of an utterance of n samples from its moment vector: x~ = x - mean(x).
template <int S>
struct PitMoments {
  const double* q;
  double n;
  __device__ __forceinline__ double sum(int v) const { return q[pit_iq_sum(S, v)]; }
  __device__ __forceinline__ double mean(int v) const { return sum(v) / n; }
  __device__ __forceinline__ double energy(int v) const {                       // |x~_v|^2
    // sum(x^2) - sum(x)^2/n of a constant (DC-only) signal can cancel to a slightly negative number; the
    // reference subtracts the mean first, so its energies are >= 0: clamp, or sqrt() would return NaN
    const double e = q[pit_iq_sq(S, v)] - sum(v) * sum(v) / n;
    return e > 0.0 ? e : 0.0;
  }
  __device__ __forceinline__ double sum_est(int s) const { return sum(s); }
  __device__ __forceinline__ double sum_tgt(int k) const { return sum(S + k); }
  __device__ __forceinline__ double mean_est(int s) const { return mean(s); }
  __device__ __forceinline__ double mean_tgt(int k) const { return mean(S + k); }
  __device__ __forceinline__ double aa(int s) const { return energy(s); }      // |a~_s|^2
  __device__ __forceinline__ double tt(int k) const { return energy(S + k); }  // |t~_k|^2
  __device__ __forceinline__ double mix_energy() const { return energy(2 * S); }
  __device__ __forceinline__ double at(int s, int k) const { return q[pit_iq_at(S, s, k)] - sum_est(s) * sum_tgt(k) / n; }    // <a~_s, t~_k>
  __device__ __forceinline__ double xt(int k) const { return q[pit_iq_xt(S, k)] - sum(2 * S) * sum_tgt(k) / n; }              // <x~, t~_k>
};

// The chunk partials of utterance b -> its moment vector q[pit_nq(S)] in LDS: thread i sums quantity i in chunk order, so each has one fixed
// order.  Every thread of the workgroup (at least pit_nq(S) of them) calls it; it ends with the barrier after which all of them may read q.
template <int S>
__device__ __forceinline__ void pit_fold_moments(const double* __restrict__ part, int b, int nchunk, double* q) {
  constexpr int NQ = pit_nq(S);
  if (threadIdx.x < NQ) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[((long long)b * nchunk + c) * NQ + threadIdx.x];
    q[threadIdx.x] = s;
  }
  __syncthreads();
}

// sum_s m[s][pi_p(s)]: what every walk below minimises or maximises
template <int S>
__device__ __forceinline__ double perm_cost(const double (&m)[S][S], int p) {
  double c = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) c += m[s][perm_at<S>(p, s)];
  return c;
}
template <int S>
__device__ __forceinline__ void store_perm(int* __restrict__ dst, int p) {
#pragma unroll
  for (int s = 0; s < S; ++s) dst[s] = perm_at<S>(p, s);
}

template <int S>
__global__ __launch_bounds__(PIT_TPB) void pit_partial_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                             const float* __restrict__ mix, int B, int T, int nchunk,
                                                             double* __restrict__ part) {
  constexpr int NV = 2 * S + 1, NQ = pit_nq(S);
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int t0 = chunk * PIT_CHUNK, t1 = min(T, t0 + PIT_CHUNK);
  double q[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) q[i] = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += PIT_TPB) {
    double v[NV];                       // est_0..est_{S-1}, tgt_0..tgt_{S-1}, mix
#pragma unroll
    for (int s = 0; s < S; ++s) {
      v[s] = (double)est[((long long)s * B + b) * T + t];
      v[S + s] = (double)tgt[((long long)s * B + b) * T + t];
    }
    v[2 * S] = mix ? (double)mix[(long long)b * T + t] : 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      q[pit_iq_sum(S, i)] += v[i];
      q[pit_iq_sq(S, i)] = fma(v[i], v[i], q[pit_iq_sq(S, i)]);
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int k = 0; k < S; ++k) q[pit_iq_at(S, s, k)] = fma(v[s], v[S + k], q[pit_iq_at(S, s, k)]);
#pragma unroll
    for (int k = 0; k < S; ++k) q[pit_iq_xt(S, k)] = fma(v[2 * S], v[S + k], q[pit_iq_xt(S, k)]);
  }
  __shared__ double red[PIT_TPB / 64][NQ];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const double s = wave_sum_d(q[i]);
    if (lane == 0) red[w][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    double s = 0.0;
#pragma unroll
    for (int ww = 0; ww < PIT_TPB / 64; ++ww) s += red[ww][threadIdx.x];
    part[((long long)b * nchunk + chunk) * NQ + threadIdx.x] = s;
  }
}

__device__ __forceinline__ double sisnr_db(double aa, double tt, double at, double eps) {
  // aa = |a~|^2, tt = |t~|^2, at = <a~,t~>
  const double alpha = at / (tt + eps);
  const double num = fabs(alpha) * sqrt(tt);
  double res2 = aa - 2.0 * alpha * at + alpha * alpha * tt;
  res2 = res2 > 0.0 ? res2 : 0.0;
  return 20.0 * log10(eps + num / (sqrt(res2) + eps));
}

template <int S>
__global__ __launch_bounds__(64) void pit_finalize_kernel(const double* __restrict__ part, int T, int nchunk, double eps_loss,
                                                         double eps_i, double clamp_min, int have_mix, float* __restrict__ loss,
                                                         int* __restrict__ loss_perm, float* __restrict__ sisnri,
                                                         int* __restrict__ sisnri_perm) {
  const int b = blockIdx.x;
  __shared__ double q[pit_nq(S)];
  pit_fold_moments<S>(part, b, nchunk, q);
  if (threadIdx.x != 0) return;
  const PitMoments<S> m{q, (double)T};
  double aa[S], tt[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    aa[i] = m.aa(i);
    tt[i] = m.tt(i);
  }
  double snr_l[S][S], snr_i[S][S], snr_x[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const double xt = m.xt(k);
    snr_x[k] = have_mix ? sisnr_db(m.mix_energy(), tt[k], xt, eps_i) : 0.0;
  }
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double et = m.at(s, k);
      const double l = -sisnr_db(aa[s], tt[k], et, eps_loss);
      snr_l[s][k] = l < clamp_min ? clamp_min : l;      // torch.clamp(utt_loss, min=-30)
      snr_i[s][k] = sisnr_db(aa[s], tt[k], et, eps_i) - snr_x[k];
    }
  double best_l, best_i;
  const int arg_l = pit_walk_min<S>([&](int p) { return perm_cost<S>(snr_l, p); }, best_l);
  const int arg_i = pit_walk_max<S>([&](int p) { return perm_cost<S>(snr_i, p); }, best_i);
  loss[b] = (float)best_l;
  if (loss_perm) store_perm<S>(loss_perm + b * S, arg_l);
  if (sisnri_perm) store_perm<S>(sisnri_perm + b * S, arg_i);
  if (sisnri) {
#pragma unroll
    for (int s = 0; s < S; ++s) sisnri[b * S + s] = (float)snr_i[s][perm_at<S>(arg_i, s)];
  }
}
// ---- source-aggregated, soft-thresholded SDR: one ratio per utterance over all S sources ----
//   D = sum_k |t~_k|^2,  E_p = sum_s |e~_s - t~_p(s)|^2,  loss = min_p 10 log10((E_p + tau D + eps) / (D + eps)),  tau = 10^(-snr_max / 10)
// Not scale-invariant, no per-pair division by |t~_k|^2: a silent target costs nothing to state.  The time form takes its pair energies
// from the moments (sasdr_pairs), the magnitude form from stft_pair_kernel's sums with unit scales; the walk, the value and the
// gradient coefficient below serve both.
// |e~_s - t~_k|^2 for every pair and D, from the one-pass moments.  A bit-equal pair gives exactly 0 (the three moments are then the same
// fp64 number); cancellation below 0 is clamped as the energies are.
template <int S>
__device__ __forceinline__ void sasdr_pairs(const PitMoments<S>& m, double (&res)[S][S], double& D) {
  double aa[S], tt[S];
  D = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    aa[i] = m.aa(i);
    tt[i] = m.tt(i);
    D += tt[i];
  }
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double at = m.at(s, k);
      const double r = (aa[s] - 2.0 * at) + tt[k];
      res[s][k] = r > 0.0 ? r : 0.0;
    }
}
// the permutation a backward was handed, clamped into range: res[][] is indexed by it
template <int S>
__device__ __forceinline__ void load_perm_clamped(const int* __restrict__ src, int (&pk)[S]) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int k = src[i];
    pk[i] = k < 0 ? 0 : (k >= S ? S - 1 : k);
  }
}
template <int S>
__device__ __forceinline__ double sasdr_energy(const double (&res)[S][S], const int* __restrict__ pk) {   // E of the permutation pk[0..S)
  double e = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) e += res[s][pk[s]];
  return e;
}
// the first minimiser of E_p (the denominator does not depend on p) -> its index; E of it in `best`
template <int S>
__device__ __forceinline__ int sasdr_walk(const double (&res)[S][S], double& best) {
  return pit_walk_min<S>([&](int p) { return perm_cost<S>(res, p); }, best);
}
__device__ __forceinline__ double sasdr_db(double E, double D, double tau, double eps) {
  return 10.0 * log10((E + tau * D + eps) / (D + eps));
}
// d loss / d (e~_s - t~_p(s)) = sasdr_coef * (e~_s - t~_p(s)); the same number for every source of the utterance, no clamp branch
__device__ __forceinline__ double sasdr_coef(double E, double D, double tau, double eps) {
  return (20.0 / log(10.0)) / (E + tau * D + eps);
}

template <int S>
__global__ __launch_bounds__(64) void sasdr_finalize_kernel(const double* __restrict__ part, int T, int nchunk, double eps, double tau,
                                                           float* __restrict__ loss, int* __restrict__ perm) {
  const int b = blockIdx.x;
  __shared__ double q[pit_nq(S)];
  pit_fold_moments<S>(part, b, nchunk, q);
  if (threadIdx.x != 0) return;
  double res[S][S], D, E;
  sasdr_pairs<S>(PitMoments<S>{q, (double)T}, res, D);
  const int arg = sasdr_walk<S>(res, E);
  loss[b] = (float)sasdr_db(E, D, tau, eps);
  if (perm) store_perm<S>(perm + b * S, arg);
}
}  // namespace

struct PitWs {   // the chunks' fp64 partial moments; the backward adds four coefficients per (b, s)
  double* part;
  float* coef;
  PitWs(Arena& a, int S, int B, int T, bool bwd) {
    part = a.f64((size_t)B * pit_nchunk(T) * pit_nq(S));
    coef = bwd ? a.f32((size_t)B * S * 4) : nullptr;
  }
};
size_t pit_workspace_bytes(int S, int B, int T) {
  if (S < 1 || S > PIT_SMAX || B <= 0 || T <= 0) return 0;
  return layout_bytes<PitWs>(S, B, T, false);
}

namespace {
// f(std::integral_constant<int, S>) for the S the library is built for: the launches of an entry are written once, as a generic lambda
template <class F>
int dispatch_S(int S, F&& f) {
  static_assert(PIT_SMAX == 3, "one case per S");
  switch (S) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return SEPR_EINVAL;
  }
}
// the moment pass every entry starts with; mix may be null (its moments are then 0)
template <int S>
void launch_moments(const float* est, const float* tgt, const float* mix, int B, int T, double* part, hipStream_t st) {
  const int nchunk = pit_nchunk(T);
  hipLaunchKernelGGL((pit_partial_kernel<S>), dim3(nchunk, B), dim3(PIT_TPB), 0, st, est, tgt, mix, B, T, nchunk, part);
}
}  // namespace

}  // namespace sepr

extern "C" int sepr_pit_sisnr_fwd(const float* est, const float* tgt, const float* mix, int S, int B, int T, double eps_loss,
                                  double eps_i, double clamp_min, float* loss, int* loss_perm, float* sisnri,
                                  int* sisnri_perm, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!est || !tgt || !loss || S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || B > 65535) return SEPR_EINVAL;
  if ((sisnri || sisnri_perm) && !mix) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  double* part = PitWs(ar, S, B, T, false).part;
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int have_mix = mix ? 1 : 0;
  return dispatch_S(S, [&](auto ss) {
    constexpr int SS = decltype(ss)::value;
    launch_moments<SS>(est, tgt, mix, B, T, part, st);
    hipLaunchKernelGGL((pit_finalize_kernel<SS>), dim3(B), dim3(64), 0, st, part, T, pit_nchunk(T), eps_loss, eps_i, clamp_min, have_mix,
                       loss, loss_perm, sisnri, sisnri_perm);
    SEPR_CHECK_LAUNCH("pit_sisnr kernels");
    return SEPR_OK;
  });
}

extern "C" int sepr_pit_sasdr_fwd(const float* est, const float* tgt, int S, int B, int T, double eps, double snr_max, float* loss,
                                  int* perm, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!est || !tgt || !loss || S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || B > 65535) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  double* part = PitWs(ar, S, B, T, false).part;
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double tau = pow(10.0, -snr_max / 10.0);
  return dispatch_S(S, [&](auto ss) {
    constexpr int SS = decltype(ss)::value;
    launch_moments<SS>(est, tgt, nullptr, B, T, part, st);
    hipLaunchKernelGGL((sasdr_finalize_kernel<SS>), dim3(B), dim3(64), 0, st, part, T, pit_nchunk(T), eps, tau, loss, perm);
    SEPR_CHECK_LAUNCH("pit_sasdr kernels");
    return SEPR_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// PIT_SISNR_mag (criterions.py:117-176): the same permutation walk on STFT magnitudes
//   loss(est_s, tgt_k) = -20 log10(eps + |M_k'| / (|M_s - M_k'| + eps)),  M = sqrt(re^2 + im^2 + 1e-10) of the conv-STFT
//   (:74-113, kernel :43-61) of the zero-mean signal, tgt scaled by clamp(<e~,t~> / (|t~|^2 + eps), min = 1e-2) (:155-159),
//   norms over (bins, frames) (:164).
// Four launches: the moment kernel above (means and the S x S scales), stft_prep_kernel (zero-mean, zero-padded copies of
// the 2S waveforms), the STFT itself as ONE f32-MFMA projection (row f of the A operand is x[hop*f : hop*f + N]: an
// overlapping row map with leading dimension = hop, the DFT kernel is the weight) and stft_pair_kernel (fp64 sums of
// M_k'^2 and (M_s - M_k')^2 per (utterance, estimate, target), then the permutation walk).
// ---------------------------------------------------------------------------------------------------------------------
namespace sepr {
int launch_gemm(int pro, int epi, const GemmArgs& a, int site, hipStream_t stream);   // sepr_gemm.hip
namespace {

template <int S>
__global__ __launch_bounds__(64) void mag_scales_kernel(const double* __restrict__ part, int T, int nchunk, double eps,
                                                       float* __restrict__ means, float* __restrict__ scales, int B, int unit /* 1: every scale is 1 (the aggregated form) */) {
  const int b = blockIdx.x;
  __shared__ double q[pit_nq(S)];
  pit_fold_moments<S>(part, b, nchunk, q);
  if (threadIdx.x != 0) return;
  const PitMoments<S> m{q, (double)T};
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) means[i * B + b] = (float)m.mean(i);        // waveform order: est_0.. est_{S-1}, tgt_0..
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double et = m.at(s, k), tt = m.tt(k);
      const double sc = et / (tt + eps);
      scales[(b * S + s) * S + k] = unit ? 1.f : (float)(sc < 1e-2 ? 1e-2 : sc);   // torch.clamp(scale, min=1e-2)
    }
}

__global__ __launch_bounds__(256) void stft_prep_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                       const float* __restrict__ means, int SB, int T, int Tpad,
                                                       float* __restrict__ xz) {
  const int wv = blockIdx.y;                                     // 0 .. 2*S*B - 1
  const float* src = (wv < SB ? est + (long long)wv * T : tgt + (long long)(wv - SB) * T);
  const float mu = means[wv];
  for (int t = blockIdx.x * 256 + threadIdx.x; t < Tpad; t += gridDim.x * 256)
    xz[(long long)wv * Tpad + t] = t < T ? src[t] - mu : 0.f;
}

// N values per thread of a 256-thread workgroup -> their N sums in every thread, the four wave sums taken in pairs, (r0 + r1) + (r2 + r3):
// the order the three kernels below have had from the start (block_sum_d's left-to-right order rounds differently).  One barrier.
template <int N>
__device__ __forceinline__ void pair_block_sums(double (&v)[N], double (&red)[N][4]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum_d(v[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
}

template <int S>
__global__ __launch_bounds__(256) void stft_pair_kernel(const float* __restrict__ C, int ldc, int B, int nfr, int nbin,
                                                       const float* __restrict__ scales, double* __restrict__ sums) {
  // block = (utterance b, estimate s, target k): sums[0] = sum M_k'^2, sums[1] = sum (M_s - M_k')^2
  const int b = blockIdx.x, s = blockIdx.y / S, k = blockIdx.y % S;
  const float sc = scales[(b * S + s) * S + k];
  const float* Ce = C + (long long)(s * B + b) * nfr * ldc;
  const float* Ct = C + (long long)((S + k) * B + b) * nfr * ldc;
  double a[2] = {0.0, 0.0};
  const int total = nfr * nbin;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int f = i / nbin, w = i - f * nbin;
    const float er = Ce[(long long)f * ldc + w], ei = Ce[(long long)f * ldc + nbin + w];
    const float tr = sc * Ct[(long long)f * ldc + w], ti = sc * Ct[(long long)f * ldc + nbin + w];
    const float me = sqrtf(er * er + ei * ei + 1.0e-10f);
    const float ms = sqrtf(tr * tr + ti * ti + 1.0e-10f);
    const double d = (double)me - (double)ms;
    a[0] = fma((double)ms, (double)ms, a[0]);
    a[1] = fma(d, d, a[1]);
  }
  __shared__ double red[2][4];
  pair_block_sums(a, red);
  if (threadIdx.x == 0) {
    double* o = sums + ((long long)(b * S + s) * S + k) * 2;
    o[0] = a[0];
    o[1] = a[1];
  }
}

template <int S>
__global__ __launch_bounds__(64) void mag_finalize_kernel(const double* __restrict__ sums, int B, double eps, float* __restrict__ loss,
                                                         int* __restrict__ perm) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double l[S][S];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double* o = sums + ((long long)(b * S + s) * S + k) * 2;
      l[s][k] = -20.0 * log10(eps + sqrt(o[0]) / (sqrt(o[1]) + eps));
    }
  double best;
  const int arg = pit_walk_min<S>([&](int p) { return perm_cost<S>(l, p); }, best);
  loss[b] = (float)best;
  if (perm) store_perm<S>(perm + b * S, arg);
}

// the aggregated form over the pair sums of unit scales: sums[(b, s, k)] = (sum M_k^2, sum (M_s - M_k)^2); D reads the s = 0 row
template <int S>
__device__ __forceinline__ void sasdr_mag_pairs(const double* __restrict__ sums, int b, double (&res)[S][S], double& D) {
  D = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double* o = sums + ((long long)(b * S + s) * S + k) * 2;
      res[s][k] = o[1];
      if (s == 0) D += o[0];
    }
}
template <int S>
__global__ __launch_bounds__(64) void sasdr_mag_finalize_kernel(const double* __restrict__ sums, int B, double eps, double tau,
                                                               float* __restrict__ loss, int* __restrict__ perm) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double res[S][S], D, E;
  sasdr_mag_pairs<S>(sums, b, res, D);
  const int arg = sasdr_walk<S>(res, E);
  loss[b] = (float)sasdr_db(E, D, tau, eps);
  if (perm) store_perm<S>(perm + b * S, arg);
}

// geometry and workspace of the magnitude loss, carved from `a` (sized by the same code on Arena::sizing())
struct MagPlan {
  int nchunk, NF, Tpad, nfr, ldc;
  double* part;
  float *means, *scales, *xz, *C;
  double* sums;
};
MagPlan mag_plan(Arena& a, int S, int B, int T, int N, int hop) {
  MagPlan p;
  p.nchunk = pit_nchunk(T);
  p.NF = (T + hop - 1) / hop;
  p.Tpad = p.NF * hop;
  p.nfr = p.Tpad >= N ? (p.Tpad - N) / hop + 1 : 0;
  p.ldc = ((N + 2) + 3) / 4 * 4;
  p.part = PitWs(a, S, B, T, false).part;
  p.means = a.f32((size_t)2 * S * B);
  p.scales = a.f32((size_t)B * S * S);
  p.xz = a.f32((size_t)2 * S * B * p.Tpad);
  p.C = a.f32((size_t)2 * S * B * p.nfr * p.ldc);
  p.sums = a.f64((size_t)B * S * S * 2);
  return p;
}
}  // namespace

size_t pit_mag_workspace_bytes(int S, int B, int T, int N, int hop) {
  if (S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || N <= 0 || hop <= 0 || N % 32 != 0 || hop % 4 != 0) return 0;
  Arena a = Arena::sizing();
  mag_plan(a, S, B, T, N, hop);
  return a.need();
}
}  // namespace sepr

extern "C" size_t sepr_pit_sisnr_mag_workspace(int S, int B, int T, int frame_len, int frame_shift) {
  return sepr::pit_mag_workspace_bytes(S, B, T, frame_len, frame_shift);
}

namespace sepr {
namespace {
// The forward quantities of both magnitude criteria, which their backward recomputes launch for launch: moments, scales (`agg`: unit scales)
// and means, the zero-mean padded copies of the 2S waveforms, their STFT as one projection, the pair sums.  `where` names the first
// launch check; the caller makes the one after its own launches.
template <int S>
int mag_forward_launches(const MagPlan& p, const float* est, const float* tgt, int B, int T, const float* dft, int frame_len, int frame_shift,
                         double eps, int agg, const char* where, hipStream_t st) {
  launch_moments<S>(est, tgt, nullptr, B, T, p.part, st);
  hipLaunchKernelGGL((mag_scales_kernel<S>), dim3(B), dim3(64), 0, st, p.part, T, p.nchunk, eps, p.means, p.scales, B, agg);
  const int gx = (p.Tpad + 255) / 256 < 64 ? (p.Tpad + 255) / 256 : 64;
  hipLaunchKernelGGL(stft_prep_kernel, dim3(gx, 2 * S * B), dim3(256), 0, st, est, tgt, p.means, S * B, T, p.Tpad, p.xz);
  SEPR_CHECK_LAUNCH(where);
  {  // STFT: row (waveform, frame f) of A = xz[waveform][hop*f : hop*f + N]; weight = DFT kernel [N+2 (padded to ldc), N]
    GemmArgs a = gemm_args_zero();
    a.M = 2 * S * B * p.nfr; a.N = p.ldc; a.K = frame_len;
    a.A = p.xz; a.lda = frame_shift;
    a.rows_out = p.nfr; a.rows_src = p.NF; a.rows_valid = p.nfr;
    a.W = dft; a.bias = nullptr; a.Y = p.C; a.ldc = p.ldc;
    SEPR_TRY(launch_gemm(PRO_PLAIN, EPI_STORE, a, SEPR_SITE_NONE, st));
  }
  hipLaunchKernelGGL((stft_pair_kernel<S>), dim3(B, S * S), dim3(256), 0, st, p.C, p.ldc, B, p.nfr, frame_len / 2 + 1, p.scales, p.sums);
  return SEPR_OK;
}

// both magnitude criteria: `agg` = 0 the per-pair SI-SNR form, 1 the aggregated form (unit scales, sasdr_mag_finalize_kernel with `tau`)
int mag_fwd(const float* est, const float* tgt, int S, int B, int T, const float* dft, int frame_len, int frame_shift, double eps, int agg,
            double tau, float* loss, int* perm, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  if (!est || !tgt || !dft || !loss || S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || B > 65535) return SEPR_EINVAL;
  if (frame_len <= 0 || frame_len % 32 != 0 || frame_shift <= 0 || frame_shift % 4 != 0) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  const MagPlan p = mag_plan(ar, S, B, T, frame_len, frame_shift);
  if (p.nfr <= 0) return SEPR_EINVAL;                                 // shorter than one frame
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  if ((long long)2 * S * B * p.nfr > 0x7fffffffLL / 8 || (long long)2 * S * B * p.Tpad >= (1LL << 32)) return SEPR_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_S(S, [&](auto ss) {
    constexpr int SS = decltype(ss)::value;
    SEPR_TRY(mag_forward_launches<SS>(p, est, tgt, B, T, dft, frame_len, frame_shift, eps, agg, "pit mag: moments / prep", st));
    if (agg)
      hipLaunchKernelGGL((sasdr_mag_finalize_kernel<SS>), dim3((B + 63) / 64), dim3(64), 0, st, p.sums, B, eps, tau, loss, perm);
    else
      hipLaunchKernelGGL((mag_finalize_kernel<SS>), dim3((B + 63) / 64), dim3(64), 0, st, p.sums, B, eps, loss, perm);
    SEPR_CHECK_LAUNCH("pit mag: pair sums");
    return SEPR_OK;
  });
}
}  // namespace
}  // namespace sepr

extern "C" int sepr_pit_sisnr_mag_fwd(const float* est, const float* tgt, int S, int B, int T, const float* dft, int frame_len,
                                      int frame_shift, double eps, float* loss, int* perm, void* ws, size_t ws_bytes,
                                      sepr_stream_t stream) {
  return sepr::mag_fwd(est, tgt, S, B, T, dft, frame_len, frame_shift, eps, 0, 0.0, loss, perm, ws, ws_bytes, stream);
}
extern "C" int sepr_pit_sasdr_mag_fwd(const float* est, const float* tgt, int S, int B, int T, const float* dft, int frame_len,
                                      int frame_shift, double eps, double snr_max, float* loss, int* perm, void* ws, size_t ws_bytes,
                                      sepr_stream_t stream) {
  return sepr::mag_fwd(est, tgt, S, B, T, dft, frame_len, frame_shift, eps, 1, pow(10.0, -snr_max / 10.0), loss, perm, ws, ws_bytes,
                       stream);
}

// =====================================================================================================================
// Backward of the two training criteria (reference: torch.autograd through criterions.py:148-217)
// =====================================================================================================================
// PIT_SISNR_time.  For estimate a and its permuted target t (zero-mean versions a~, t~):
//   alpha = <a~,t~> / c, c = |t~|^2 + eps;  e = a~ - alpha t~;  P = |alpha| |t~|;  R = |e|;  u = P / (R + eps)
//   loss = clamp(-20 log10(eps + u), min = clamp_min)
//   d loss / d a = g_u [ sign(alpha) |t~| / (c (R + eps)) t~  -  P / ((R + eps)^2 R) (e - (e.t~)/c t~) ],  g_u = -(20 / ln 10) / (eps + u)
// (a linear combination of the zero-mean vectors a~ and t~, so removing the mean is already accounted for); zero where
// the clamp is active.  The moments come from the same one-pass kernel as the forward; the gradient is then one
// element-wise pass: dest = ca (a - mean_a) + ct (t - mean_t).
namespace sepr {
namespace {
template <int S>
__global__ __launch_bounds__(64) void pit_bwd_coef_kernel(const double* __restrict__ part, const int* __restrict__ perm,
                                                         const float* __restrict__ gl, int T, int nchunk, double eps, double clamp_min,
                                                         float* __restrict__ coef /*[B][S][4]: ca, ct, mean_a, mean_t*/) {
  const int b = blockIdx.x;
  __shared__ double q[pit_nq(S)];
  pit_fold_moments<S>(part, b, nchunk, q);
  if (threadIdx.x >= S) return;
  const int s = threadIdx.x, k = perm[b * S + s];
  const PitMoments<S> m{q, (double)T};
  const double aa = m.aa(s), tt = m.tt(k), at = m.at(s, k);
  const double c = tt + eps, alpha = at / c;
  const double P = fabs(alpha) * sqrt(tt);
  double R2 = aa - 2.0 * alpha * at + alpha * alpha * tt;
  R2 = R2 > 0.0 ? R2 : 0.0;
  const double R = sqrt(R2), u = P / (R + eps);
  const double loss = -20.0 * log10(eps + u);
  double ca = 0.0, ct = 0.0;
  if (loss > clamp_min && R > 0.0) {
    const double gu = -(20.0 / log(10.0)) / (eps + u) * (double)gl[b];
    const double et = at - alpha * tt;                                   // e . t~
    const double kt = gu * (alpha >= 0.0 ? 1.0 : -1.0) * sqrt(tt) / (c * (R + eps));   // coefficient of t~ from dP
    const double ke = -gu * P / ((R + eps) * (R + eps) * R);             // coefficient of (e - (e.t~)/c t~) from dR
    ca = ke;                                                             // e = a~ - alpha t~
    ct = kt - ke * alpha - ke * et / c;
  }
  float* o = coef + ((long long)b * S + s) * 4;
  o[0] = (float)ca; o[1] = (float)ct; o[2] = (float)m.mean_est(s); o[3] = (float)m.mean_tgt(k);
}
// the aggregated form's record: ca = k, ct = -k with k = sasdr_coef * gl[b], the two means.  A pair whose energy is exactly 0 in the moments
// (bit-equal signals, two silent rows) gets ca = ct = 0: its gradient is exactly 0, which k a~ - k t~ rounded twice in float32 is not.
template <int S>
__global__ __launch_bounds__(64) void sasdr_bwd_coef_kernel(const double* __restrict__ part, const int* __restrict__ perm,
                                                           const float* __restrict__ gl, int T, int nchunk, double eps, double tau,
                                                           float* __restrict__ coef /*[B][S][4]: ca, ct, mean_a, mean_t*/) {
  const int b = blockIdx.x;
  __shared__ double q[pit_nq(S)];
  pit_fold_moments<S>(part, b, nchunk, q);
  if (threadIdx.x >= S) return;
  const int s = threadIdx.x;
  int pk[S];
  load_perm_clamped<S>(perm + b * S, pk);
  const PitMoments<S> m{q, (double)T};
  double res[S][S], D;
  sasdr_pairs<S>(m, res, D);
  const double k = res[s][pk[s]] > 0.0 ? sasdr_coef(sasdr_energy<S>(res, pk), D, tau, eps) * (double)gl[b] : 0.0;
  float* o = coef + ((long long)b * S + s) * 4;
  o[0] = (float)k; o[1] = (float)-k; o[2] = (float)m.mean_est(s); o[3] = (float)m.mean_tgt(pk[s]);
}
__global__ __launch_bounds__(256) void pit_bwd_apply_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                           const int* __restrict__ perm, const float* __restrict__ coef, int S, int B, int T,
                                                           float* __restrict__ dest) {
  const int sb = blockIdx.y;                 // s * B + b
  const int s = sb / B, b = sb - s * B;
  const float* cf = coef + ((long long)b * S + s) * 4;
  const float ca = cf[0], ct = cf[1], ma = cf[2], mt = cf[3];
  const float* a = est + (long long)sb * T;
  const float* t = tgt + ((long long)perm[b * S + s] * B + b) * T;
  float* o = dest + (long long)sb * T;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < T; i += gridDim.x * 256) o[i] = fmaf(ca, a[i] - ma, ct * (t[i] - mt));
}
}  // namespace
}  // namespace sepr

namespace sepr {
namespace {
// both time criteria: `agg` = 0 the per-pair SI-SNR coefficients (lim = clamp_min), 1 the aggregated form's (lim = tau)
int pit_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, double eps, int agg, double lim,
            float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  if (!est || !tgt || !perm || !gl || !dest || S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || B > 65535) return SEPR_EINVAL;
  const int nchunk = pit_nchunk(T);
  Arena ar(ws, ws_bytes);
  const PitWs k(ar, S, B, T, true);
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  double* part = k.part;
  float* coef = k.coef;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_S(S, [&](auto ss) {
    constexpr int SS = decltype(ss)::value;
    launch_moments<SS>(est, tgt, nullptr, B, T, part, st);
    if (agg)
      hipLaunchKernelGGL((sasdr_bwd_coef_kernel<SS>), dim3(B), dim3(64), 0, st, part, perm, gl, T, nchunk, eps, lim, coef);
    else
      hipLaunchKernelGGL((pit_bwd_coef_kernel<SS>), dim3(B), dim3(64), 0, st, part, perm, gl, T, nchunk, eps, lim, coef);
    const int gx = (T + 255) / 256 < 64 ? (T + 255) / 256 : 64;
    hipLaunchKernelGGL(pit_bwd_apply_kernel, dim3(gx, S * B), dim3(256), 0, st, est, tgt, perm, coef, S, B, T, dest);
    SEPR_CHECK_LAUNCH("pit_sisnr_bwd kernels");
    return SEPR_OK;
  });
}
}  // namespace
}  // namespace sepr

extern "C" int sepr_pit_sisnr_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, double eps,
                                  double clamp_min, float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  return sepr::pit_bwd(est, tgt, perm, gl, S, B, T, eps, 0, clamp_min, dest, ws, ws_bytes, stream);
}
extern "C" int sepr_pit_sasdr_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, double eps,
                                  double snr_max, float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  return sepr::pit_bwd(est, tgt, perm, gl, S, B, T, eps, 1, pow(10.0, -snr_max / 10.0), dest, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// PIT_SISNR_mag backward.  With M_e = |STFT(a~)|, M_s = |STFT(c t~)| (both sqrt(re^2 + im^2 + 1e-10)), c = max(<a~,t~> / (|t~|^2 + eps), 1e-2),
// P = |M_s|_F, R = |M_e - M_s|_F, u = P / (R + eps), loss = -20 log10(eps + u):
//   dL/dM_e = g_u (-P / ((R + eps)^2 R)) (M_e - M_s);   dL/dM_s = g_u [ M_s / (P (R + eps)) + P / ((R + eps)^2 R) (M_e - M_s) ]
//   d re_e = dL/dM_e re_e / M_e (same for im);  dL/dc = sum dL/dM_s c (re_t^2 + im_t^2) / M_s;  dc/da~ = t~ / (|t~|^2 + eps) unless clamped
//   d a~ = STFT^T(d re_e, d im_e) + dL/dc dc/da~;   d a = d a~ - mean(d a~)
// The STFT adjoint is the same projection core with the transposed DFT kernel followed by an overlap-add gather.
// ---------------------------------------------------------------------------------------------------------------------
namespace sepr {
namespace {
struct MagBwdPlan {
  MagPlan f;
  int ldd;      // leading dimension of dC: frame_len + 2 rounded up to a multiple of 32 (K of the adjoint projection)
  float* dC;
  double* dLdc;
  float *fr, *da;
};
MagBwdPlan mag_bwd_plan(Arena& a, int S, int B, int T, int N, int hop) {
  MagBwdPlan p;
  p.f = mag_plan(a, S, B, T, N, hop);
  p.ldd = ((N + 2) + 31) / 32 * 32;
  p.dC = a.f32((size_t)S * B * p.f.nfr * p.ldd);      // d(re, im) of the estimates' STFT
  p.dLdc = a.f64((size_t)S * B * 2);                  // dL/dc partial (one per (s,b)), spare
  p.fr = a.f32((size_t)S * B * p.f.nfr * N);          // adjoint frames before overlap-add
  p.da = a.f32((size_t)S * B * p.f.Tpad);             // d a~ (padded length)
  a.f32((size_t)S * B * 4);                           // (unused: kept so that the size does not move)
  return p;
}

// block = (b, s): pass 1 sums are already in `sums` (P^2, R^2 for every (b, s, k)); this kernel writes dC for the
// estimate s of utterance b against its permuted target and reduces dL/dc
// AGG: the aggregated form (unit scales in `scales`, `tau` its threshold): dL/dM_e = sasdr_coef gl[b] (M_e - M_s), nothing flows to the scale
template <int S, bool AGG>
__global__ __launch_bounds__(256) void stft_pair_bwd_kernel(const float* __restrict__ C, int ldc, int B, int nfr, int nbin,
                                                           const float* __restrict__ scales, const double* __restrict__ sums,
                                                           const int* __restrict__ perm, const float* __restrict__ gl, double eps, double tau,
                                                           float* __restrict__ dC, int ldd, double* __restrict__ dLdc) {
  const int b = blockIdx.x, s = blockIdx.y;
  const int k = perm[b * S + s];
  const float sc = scales[(b * S + s) * S + k];
  float ge, gs1, gs2;                                       // dL/dM_e = ge (M_e - M_s);  dL/dM_s = gs1 M_s + gs2 (M_e - M_s)
  if (AGG) {
    int pk[S];
    load_perm_clamped<S>(perm + b * S, pk);
    double res[S][S], D;
    sasdr_mag_pairs<S>(sums, b, res, D);
    ge = (float)(sasdr_coef(sasdr_energy<S>(res, pk), D, tau, eps) * (double)gl[b]);
    gs1 = gs2 = 0.f;
  } else {
    const double* o = sums + ((long long)(b * S + s) * S + k) * 2;
    const double P = sqrt(o[0]), R = sqrt(o[1]);
    const double u = P / (R + eps);
    const double gu = -(20.0 / log(10.0)) / (eps + u) * (double)gl[b];
    const double kR = (R > 0.0) ? P / ((R + eps) * (R + eps) * R) : 0.0;
    ge = (float)(-gu * kR);
    gs1 = (float)(P > 0.0 ? gu / (P * (R + eps)) : 0.0);
    gs2 = (float)(gu * kR);
  }
  const float* Ce = C + (long long)(s * B + b) * nfr * ldc;
  const float* Ct = C + (long long)((S + k) * B + b) * nfr * ldc;
  float* De = dC + (long long)(s * B + b) * nfr * ldd;
  double acc[1] = {0.0};
  const int total = nfr * nbin;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int f = i / nbin, w = i - f * nbin;
    const float er = Ce[(long long)f * ldc + w], ei = Ce[(long long)f * ldc + nbin + w];
    const float tr = Ct[(long long)f * ldc + w], ti = Ct[(long long)f * ldc + nbin + w];
    const float me = sqrtf(er * er + ei * ei + 1.0e-10f);
    const float t2 = tr * tr + ti * ti;
    // AGG: the expression of `me`, so that a bit-equal pair gives d = 0 and a gradient that is exactly 0
    const float ms = AGG ? sqrtf(tr * tr + ti * ti + 1.0e-10f) : sqrtf(sc * sc * t2 + 1.0e-10f);
    const float d = me - ms;
    const float gme = ge * d;
    De[(long long)f * ldd + w] = gme * er / me;
    De[(long long)f * ldd + nbin + w] = gme * ei / me;
    const float gms = gs1 * ms + gs2 * d;
    acc[0] += (double)(gms * sc * t2 / ms);
  }
  // zero the padding columns of this estimate's rows (the adjoint projection reads ldc columns)
  for (int i = threadIdx.x; i < nfr * (ldd - 2 * nbin); i += 256) {
    const int f = i / (ldd - 2 * nbin), w = i - f * (ldd - 2 * nbin);
    De[(long long)f * ldd + 2 * nbin + w] = 0.f;
  }
  __shared__ double red[1][4];
  pair_block_sums(acc, red);
  if (threadIdx.x == 0) dLdc[b * S + s] = acc[0];
}

// overlap-add gather of the adjoint frames + the scale path: da[t] = sum_{f: 0 <= t - hop f < N} fr[f][t - hop f] + cs t~[t]
template <int S>
__global__ __launch_bounds__(256) void stft_ola_kernel(const float* __restrict__ fr, const float* __restrict__ xz, int B, int nfr, int N,
                                                      int hop, int Tpad, const double* __restrict__ dLdc, const double* __restrict__ part,
                                                      int nchunk, int T, const int* __restrict__ perm, double eps,
                                                      float* __restrict__ da) {
  const int sb = blockIdx.y;
  const int s = sb / B, b = sb - s * B;
  const int k = perm[b * S + s];
  // scale path coefficient: dL/dc * [raw scale >= 1e-2] / (|t~|^2 + eps), by every thread from the folded moments
  __shared__ double q[pit_nq(S)];
  pit_fold_moments<S>(part, b, nchunk, q);
  const PitMoments<S> m{q, (double)T};
  const double tt = m.tt(k), et = m.at(s, k);
  const double raw = et / (tt + eps);
  const float cs = raw >= 1e-2 ? (float)(dLdc[b * S + s] / (tt + eps)) : 0.f;
  const float* f0 = fr + (long long)sb * nfr * N;
  const float* tz = xz + (long long)((S + k) * B + b) * Tpad;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < Tpad; t += gridDim.x * 256) {
    float a = cs * tz[t];
    const int fhi = t / hop < nfr - 1 ? t / hop : nfr - 1;
    for (int f = fhi; f >= 0 && t - hop * f < N; --f) a += f0[(long long)f * N + (t - hop * f)];
    da[(long long)sb * Tpad + t] = a;
  }
}
// dest = da[:T] - mean(da[:T])   (a~ = a - mean(a)); one block per (s, b)
__global__ __launch_bounds__(256) void demean_kernel(const float* __restrict__ da, int Tpad, int T, float* __restrict__ dest) {
  const int sb = blockIdx.x;
  const float* p = da + (long long)sb * Tpad;
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < T; i += 256) s[0] += (double)p[i];
  __shared__ double red[1][4];
  pair_block_sums(s, red);
  const float mean = (float)(s[0] / (double)T);
  float* o = dest + (long long)sb * T;
  for (int i = threadIdx.x; i < T; i += 256) o[i] = p[i] - mean;
}
}  // namespace
}  // namespace sepr

extern "C" size_t sepr_pit_sisnr_mag_bwd_workspace(int S, int B, int T, int frame_len, int frame_shift) {
  using namespace sepr;
  if (S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || frame_len <= 0 || frame_shift <= 0 || frame_len % 32 || frame_shift % 4) return 0;
  Arena a = Arena::sizing();
  mag_bwd_plan(a, S, B, T, frame_len, frame_shift);
  return a.need();
}

namespace sepr {
namespace {
// both magnitude criteria (`agg`, `tau` as in mag_fwd)
int mag_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, const float* dft, const float* dft_t,
            int frame_len, int frame_shift, double eps, int agg, double tau, float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  if (!est || !tgt || !perm || !gl || !dft || !dft_t || !dest || S < 1 || S > PIT_SMAX || B <= 0 || T <= 0 || B > 65535) return SEPR_EINVAL;
  if (frame_len <= 0 || frame_len % 32 != 0 || frame_shift <= 0 || frame_shift % 4 != 0) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  const MagBwdPlan bp = mag_bwd_plan(ar, S, B, T, frame_len, frame_shift);
  const MagPlan& p = bp.f;
  if (p.nfr <= 0) return SEPR_EINVAL;
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_S(S, [&](auto ss) {
    constexpr int SS = decltype(ss)::value;
    const int nbin = frame_len / 2 + 1;
    SEPR_TRY(mag_forward_launches<SS>(p, est, tgt, B, T, dft, frame_len, frame_shift, eps, agg, "pit mag bwd: moments / prep", st));
    if (agg)
      hipLaunchKernelGGL((stft_pair_bwd_kernel<SS, true>), dim3(B, SS), dim3(256), 0, st, p.C, p.ldc, B, p.nfr, nbin, p.scales, p.sums, perm,
                         gl, eps, tau, bp.dC, bp.ldd, bp.dLdc);
    else
      hipLaunchKernelGGL((stft_pair_bwd_kernel<SS, false>), dim3(B, SS), dim3(256), 0, st, p.C, p.ldc, B, p.nfr, nbin, p.scales, p.sums, perm,
                         gl, eps, tau, bp.dC, bp.ldd, bp.dLdc);
    SEPR_CHECK_LAUNCH("pit mag bwd: pair");
    {  // adjoint frames: fr[row][n] = sum_c dC[row][c] K[c][n]  ->  projection with the transposed kernel dft_t [frame_len][ldd] (zero padded)
      GemmArgs a = gemm_args_zero();
      a.M = S * B * p.nfr; a.N = frame_len; a.K = bp.ldd;
      a.A = bp.dC; a.lda = bp.ldd; a.W = dft_t; a.bias = nullptr; a.Y = bp.fr; a.ldc = frame_len;
      SEPR_TRY(launch_gemm(PRO_PLAIN, EPI_STORE, a, SEPR_SITE_NONE, st));
    }
    const int gx = (p.Tpad + 255) / 256 < 64 ? (p.Tpad + 255) / 256 : 64;
    hipLaunchKernelGGL((stft_ola_kernel<SS>), dim3(gx, SS * B), dim3(256), 0, st, bp.fr, p.xz, B, p.nfr, frame_len, frame_shift, p.Tpad,
                       bp.dLdc, p.part, p.nchunk, T, perm, eps, bp.da);
    hipLaunchKernelGGL(demean_kernel, dim3(S * B), dim3(256), 0, st, bp.da, p.Tpad, T, dest);
    SEPR_CHECK_LAUNCH("pit mag bwd: adjoint");
    return SEPR_OK;
  });
}
}  // namespace
}  // namespace sepr

extern "C" int sepr_pit_sisnr_mag_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T,
                                      const float* dft, const float* dft_t, int frame_len, int frame_shift, double eps, float* dest,
                                      void* ws, size_t ws_bytes, sepr_stream_t stream) {
  return sepr::mag_bwd(est, tgt, perm, gl, S, B, T, dft, dft_t, frame_len, frame_shift, eps, 0, 0.0, dest, ws, ws_bytes, stream);
}
// the scale path of stft_ola_kernel reads dL/dc = 0 (gs1 = gs2 = 0 above) and adds exactly 0
extern "C" int sepr_pit_sasdr_mag_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T,
                                      const float* dft, const float* dft_t, int frame_len, int frame_shift, double eps, double snr_max,
                                      float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  return sepr::mag_bwd(est, tgt, perm, gl, S, B, T, dft, dft_t, frame_len, frame_shift, eps, 1, pow(10.0, -snr_max / 10.0), dest, ws,
                       ws_bytes, stream);
}
