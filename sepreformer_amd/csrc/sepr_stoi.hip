// STOI and ESTOI (Taal et al. 2011; Jensen & Taal 2016) on the device, float64 throughout (include/sepr.h
// sepr_stoi_fwd; the float64 numpy restatement is tests/stoi_ref.py).  Evaluation only, no backward.
//
// Per utterance b and reference i the clean signal x = ref[b][i] decides which frames are silent; the S estimates and the mixture are
// compacted with the same frame list, so one reference costs S + 2 spectrogram passes and S + 1 segment walks.
//
// Launches (all deterministic: fixed-order sums, no atomics; every grid is sized by the padded length T):
//   stoi_mask_kernel   one workgroup per (b, i): frame energies (a wave per frame), their maximum, the keep mask, an exclusive scan ->
//                      the list of kept frame indices, kept[b][i], status[b][i];
//   stoi_band_kernel   one workgroup per (b, i, signal, 16 spectral frames): the compacted, re-windowed frames are GATHERED from the
//                      source frames through the kept list (spectral frame m is source frame idx[m] plus the overlapping halves of
//                      idx[m - 1] and idx[m + 1]: a sum of two terms, so no overlap-add buffer, no extra launch, and the same value
//                      whichever order the overlap-add would take); the 256-point transform at the 212 bins the bands cover is a
//                      matrix product against the host-built float64 twiddle table, one bin per thread, 16 frames in registers,
//                      f64 VALU FMA; |X|^2 goes through LDS into the 15 band sums;
//   stoi_seg_kernel    one workgroup per (b, i, processed signal, 16 segments of 30 frames): both measures from the same band values
//                      in LDS, a fixed-order block sum, one pair of partials per workgroup;
//   stoi_final_kernel  one thread per (b, i, processed signal): the partials in workgroup order, the means, "too short".
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NSEG = 30, ST_BANDS = 15;
constexpr int ST_BIN0 = 7, ST_NBIN = 212;          // bins [7, 219) of the 512-point grid at 10 kHz
constexpr int ST_FT = 16;                          // spectral frames per workgroup of stoi_band_kernel
constexpr int ST_SG = 16;                          // segments per workgroup of stoi_seg_kernel
constexpr double ST_EPS = 2.220446049250313e-16;   // 2^-52
constexpr double ST_SHORT = 1e-5;
// bin of linspace(0, 10000, 513) nearest to 150 * 2^((2 b - 1) / 6), b = 0 .. 15: band b covers [ST_EDGE[b], ST_EDGE[b + 1])
__constant__ const int ST_EDGE[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__host__ __device__ inline int st_frames(int T) { return T >= ST_FRAME ? (T - ST_FRAME) / ST_HOP + 1 : 0; }

__global__ __launch_bounds__(256) void stoi_mask_kernel(const float* __restrict__ ref, const int* __restrict__ lens, int S, int T, int Fmax,
                                                        const double* __restrict__ win, double* __restrict__ energy, int* __restrict__ idx,
                                                        int* __restrict__ nk, int* __restrict__ kept, int* __restrict__ status) {
  __shared__ double wmax[4];
  __shared__ int cnt[256];
  const int bi = blockIdx.x, b = bi / S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = min(max(lens[b], 0), T), nF = st_frames(L);
  const float* x = ref + (long long)bi * T;
  double* e = energy + (long long)bi * Fmax;
  int* ix = idx + (long long)bi * Fmax;
  double mx = -__builtin_huge_val();
  for (int k = wave; k < nF; k += 4) {
    const float* f = x + (long long)k * ST_HOP;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = (double)f[lane + 64 * r] * win[lane + 64 * r];
      s = fma(v, v, s);
    }
    s = wave_sum_d(s);
    const double ek = 20.0 * log10(sqrt(s) + ST_EPS);
    if (lane == 0) e[k] = ek;
    mx = fmax(mx, ek);
  }
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();                                                  // also orders the energy stores before the reads below
  mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
  const int per = (nF + 255) / 256, k0 = tid * per, k1 = min(k0 + per, nF);
  int c = 0;
  for (int k = k0; k < k1; ++k) c += (mx - 40.0 - e[k] < 0.0) ? 1 : 0;
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int q = 0; q < 256; ++q) {
      const int v = cnt[q];
      cnt[q] = run;
      run += v;
    }
    nk[bi] = run;
    kept[bi] = run;
    status[bi] = run - 1 < ST_NSEG ? 1 : 0;
  }
  __syncthreads();
  int o = cnt[tid];
  for (int k = k0; k < k1; ++k)
    if (mx - 40.0 - e[k] < 0.0) ix[o++] = k;
}

// signal q of (b, i): 0 the reference itself, 1 .. S estimate q - 1, S + 1 the mixture
__device__ __forceinline__ const float* st_signal(const float* ref, const float* est, const float* mix, int S, int T, int b, int i, int q) {
  if (q == 0) return ref + ((long long)b * S + i) * T;
  if (q <= S) return est + ((long long)b * S + (q - 1)) * T;
  return mix + (long long)b * T;
}

__global__ __launch_bounds__(256) void stoi_band_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                        const float* __restrict__ mix, int S, int T, int Fmax,
                                                        const double* __restrict__ win, const double2* __restrict__ tw,
                                                        const int* __restrict__ idx, const int* __restrict__ nk, double* __restrict__ bands) {
  __shared__ double lds[ST_FRAME * ST_FT];                           // frames [t][f]; afterwards |X|^2 [f][bin]
  const int c = blockIdx.y, bi = c / (S + 2), q = c % (S + 2), b = bi / S, i = bi % S, tid = threadIdx.x;
  const int NS = nk[bi] - 1, m0 = blockIdx.x * ST_FT;
  if (m0 >= NS || (q == S + 1 && !mix)) return;                      // uniform
  const float* x = st_signal(ref, est, mix, S, T, b, i, q);
  const int* ix = idx + (long long)bi * Fmax;
  {
    const int t = tid, th = t < ST_HOP ? t + ST_HOP : t - ST_HOP;    // th: the same sample's offset inside the neighbouring frame
    const double wt = win[t], wh = win[th];
    for (int f = 0; f < ST_FT; ++f) {
      const int m = m0 + f;
      double v = 0.0;
      if (m < NS) {                                                  // m + 1 <= NS = kept - 1 is a kept frame
        v = (double)x[(long long)ix[m] * ST_HOP + t] * wt;
        if (t >= ST_HOP) v += (double)x[(long long)ix[m + 1] * ST_HOP + th] * wh;
        else if (m >= 1) v += (double)x[(long long)ix[m - 1] * ST_HOP + th] * wh;
        v *= wt;
      }
      lds[t * ST_FT + f] = v;
    }
  }
  __syncthreads();
  const int kb = min(tid, ST_NBIN - 1);                              // threads 212 .. 255 repeat the last bin and drop it
  double re[ST_FT], im[ST_FT];
#pragma unroll
  for (int f = 0; f < ST_FT; ++f) re[f] = im[f] = 0.0;
  const double2* twp = tw + kb;
#pragma unroll 2
  for (int t = 0; t < ST_FRAME; ++t) {
    const double2 w = twp[(long long)t * ST_NBIN];
    const double2* fr = reinterpret_cast<const double2*>(lds + t * ST_FT);
#pragma unroll
    for (int f = 0; f < ST_FT; f += 2) {
      const double2 v = fr[f / 2];
      re[f] = fma(v.x, w.x, re[f]);
      im[f] = fma(v.x, w.y, im[f]);
      re[f + 1] = fma(v.y, w.x, re[f + 1]);
      im[f + 1] = fma(v.y, w.y, im[f + 1]);
    }
  }
  __syncthreads();
  if (tid < ST_NBIN) {
#pragma unroll
    for (int f = 0; f < ST_FT; ++f) lds[f * ST_NBIN + tid] = fma(re[f], re[f], im[f] * im[f]);
  }
  __syncthreads();
  if (tid < ST_FT * ST_BANDS) {
    const int f = tid % ST_FT, band = tid / ST_FT, m = m0 + f;
    if (m < NS) {
      double s = 0.0;
      for (int k = ST_EDGE[band] - ST_BIN0; k < ST_EDGE[band + 1] - ST_BIN0; ++k) s += lds[f * ST_NBIN + k];
      bands[((long long)c * ST_BANDS + band) * Fmax + m] = sqrt(s);
    }
  }
}

// 16 consecutive segments (segment m = frames m .. m + 29) of one (reference, processed signal) pair per workgroup.  Row pass: thread
// (segment, band) forms the row's norms and means, STOI's clipped and normalised correlation, and leaves the row statistics ESTOI needs in
// LDS; column pass: thread (segment, column) normalises the 15 row-normalised values of its column and correlates them.  The two sums of
// the 16 segments leave as one pair of partials per workgroup; stoi_final_kernel adds the partials in workgroup order.
__global__ __launch_bounds__(256) void stoi_seg_kernel(int S, int Fmax, int ntiles, int have_mix, const int* __restrict__ nk,
                                                       const double* __restrict__ bands, double* __restrict__ part) {
  constexpr int W = ST_SG + ST_NSEG - 1;                             // frames under the tile's segments
  __shared__ double xs[ST_BANDS][W], ys[ST_BANDS][W];
  __shared__ double stat[4][ST_BANDS][ST_SG];                        // mean x, 1 / (norm x + eps), mean y, 1 / (norm y + eps)
  __shared__ double red[4];
  const int p = blockIdx.y, bi = p / (S + 1), q = p % (S + 1), tid = threadIdx.x;
  const int nseg = nk[bi] - ST_NSEG, m0 = blockIdx.x * ST_SG;        // kept - 1 frames give kept - 30 segments
  if (m0 >= nseg || (q == S && !have_mix)) return;                   // uniform
  const double* xb = bands + (long long)bi * (S + 2) * ST_BANDS * Fmax;
  const double* yb = xb + (long long)(q + 1) * ST_BANDS * Fmax;
  const int nfr = min(W, nseg + ST_NSEG - 1 - m0);                   // frames that exist from m0 on
  for (int e = tid; e < ST_BANDS * W; e += 256) {
    const int j = e / W, f = e % W;
    xs[j][f] = f < nfr ? xb[(long long)j * Fmax + m0 + f] : 0.0;
    ys[j][f] = f < nfr ? yb[(long long)j * Fmax + m0 + f] : 0.0;
  }
  __syncthreads();
  const double clip = 1.0 + 5.623413251903491;                       // 1 + 10^(15 / 20)
  const double inv_n = 1.0 / ST_NSEG, inv_b = 1.0 / ST_BANDS;
  double ds = 0.0, de = 0.0;
  if (tid < ST_SG * ST_BANDS) {
    const int mi = tid % ST_SG, j = tid / ST_SG;
    const double* xr = &xs[j][mi];
    const double* yr = &ys[j][mi];
    double sxx = 0.0, syy = 0.0, sumx = 0.0, sumy = 0.0;
#pragma unroll
    for (int n = 0; n < ST_NSEG; ++n) {
      sxx = fma(xr[n], xr[n], sxx);
      syy = fma(yr[n], yr[n], syy);
      sumx += xr[n];
      sumy += yr[n];
    }
    const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
    const double mean_x = sumx * inv_n, mean_y = sumy * inv_n;
    double sump = 0.0;
#pragma unroll
    for (int n = 0; n < ST_NSEG; ++n) sump += fmin(yr[n] * alpha, xr[n] * clip);
    const double mean_p = sump * inv_n;
    double cxx = 0.0, cyy = 0.0, cpp = 0.0, cxp = 0.0;
#pragma unroll
    for (int n = 0; n < ST_NSEG; ++n) {
      const double a = xr[n] - mean_x, c = fmin(yr[n] * alpha, xr[n] * clip) - mean_p, y = yr[n] - mean_y;
      cxx = fma(a, a, cxx);
      cpp = fma(c, c, cpp);
      cxp = fma(a, c, cxp);
      cyy = fma(y, y, cyy);
    }
    const double nx = sqrt(cxx) + ST_EPS;
    if (m0 + mi < nseg) ds = cxp / (nx * (sqrt(cpp) + ST_EPS));
    stat[0][j][mi] = mean_x;
    stat[1][j][mi] = 1.0 / nx;
    stat[2][j][mi] = mean_y;
    stat[3][j][mi] = 1.0 / (sqrt(cyy) + ST_EPS);
  }
  __syncthreads();
  for (int it = tid; it < ST_SG * ST_NSEG; it += 256) {
    const int mi = it % ST_SG, n = it / ST_SG;
    double a[ST_BANDS], c[ST_BANDS];
    double suma = 0.0, sumc = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
      a[j] = (xs[j][mi + n] - stat[0][j][mi]) * stat[1][j][mi];
      c[j] = (ys[j][mi + n] - stat[2][j][mi]) * stat[3][j][mi];
      suma += a[j];
      sumc += c[j];
    }
    const double ma = suma * inv_b, mc = sumc * inv_b;
    double caa = 0.0, ccc = 0.0, cac = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
      const double u = a[j] - ma, v = c[j] - mc;
      caa = fma(u, u, caa);
      ccc = fma(v, v, ccc);
      cac = fma(u, v, cac);
    }
    if (m0 + mi < nseg) de += cac / ((sqrt(caa) + ST_EPS) * (sqrt(ccc) + ST_EPS));
  }
  ds = block_sum_d(ds, red);
  de = block_sum_d(de, red);
  if (tid == 0) {
    double* o = part + ((long long)p * ntiles + blockIdx.x) * 2;
    o[0] = ds;
    o[1] = de * inv_n;
  }
}

// one thread per (b, i, processed signal): the partials in workgroup order, the two means, or 1e-5 when there is no segment
__global__ __launch_bounds__(64) void stoi_final_kernel(int S, int npairs, int ntiles, int have_mix, const int* __restrict__ nk,
                                                        const double* __restrict__ part, double* __restrict__ stoi,
                                                        double* __restrict__ estoi, double* __restrict__ stoi_mix,
                                                        double* __restrict__ estoi_mix) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= npairs) return;
  const int bi = p / (S + 1), q = p % (S + 1);
  if (q == S && !have_mix) return;
  const int nseg = nk[bi] - ST_NSEG;
  double ds = ST_SHORT, de = ST_SHORT;                               // "too short" (status bit 0, set by stoi_mask_kernel)
  if (nseg > 0) {
    ds = de = 0.0;
    const int nt = (nseg + ST_SG - 1) / ST_SG;                       // <= ntiles
    for (int t = 0; t < nt; ++t) {
      ds += part[((long long)p * ntiles + t) * 2];
      de += part[((long long)p * ntiles + t) * 2 + 1];
    }
    ds /= (double)nseg * ST_BANDS;
    de /= (double)nseg;
  }
  if (q < S) {
    stoi[(long long)bi * S + q] = ds;
    estoi[(long long)bi * S + q] = de;
  } else {
    stoi_mix[bi] = ds;
    estoi_mix[bi] = de;
  }
}

inline int st_tiles(int T) { return st_frames(T) > ST_NSEG ? (st_frames(T) - ST_NSEG + ST_SG - 1) / ST_SG : 0; }
inline bool st_shape_ok(int S, int B, int T) {
  return S >= 2 && S <= 3 && B >= 1 && T >= ST_FRAME && T <= (1 << 30) && (long long)B * S * (S + 2) <= 65535;
}
struct StoiWs {
  double* energy;   // [B S][frames] frame energies of the references
  int *idx, *nk;    // [B S][frames] kept-frame indices, [B S] their counts
  double *bands;    // [B S (S + 2)][bands][frames] one-third-octave envelopes
  double* part;     // [B S (S + 1)][tiles + 1][2] segment partials
  StoiWs(Arena& a, int S, int B, int T) {
    const size_t bs = (size_t)B * S, fr = st_frames(T);
    energy = a.f64(bs * fr); idx = a.of<int>(bs * fr); nk = a.of<int>(bs);
    bands = a.f64(bs * (S + 2) * ST_BANDS * fr); part = a.f64(bs * (S + 1) * (st_tiles(T) + 1) * 2);
  }
};
}  // namespace
}  // namespace sepr

extern "C" size_t sepr_stoi_workspace(int S, int B, int T) {
  using namespace sepr;
  if (!st_shape_ok(S, B, T)) return 0;
  return layout_bytes<StoiWs>(S, B, T);
}

extern "C" int sepr_stoi_fwd(const float* ref, const float* est, const float* mix, const int* lengths, int S, int B, int T,
                             const double* tables, double* stoi, double* estoi, double* stoi_mix, double* estoi_mix, int* kept,
                             int* status, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (!ref || !est || !lengths || !tables || !stoi || !estoi || !kept || !status) return SEPR_EINVAL;
  if (!st_shape_ok(S, B, T)) return SEPR_EINVAL;
  if ((mix == nullptr) != (stoi_mix == nullptr) || (mix == nullptr) != (estoi_mix == nullptr)) return SEPR_EINVAL;
  Arena ar(ws, ws_bytes);
  const StoiWs k(ar, S, B, T);
  if (!ar.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Fmax = st_frames(T), ntiles = st_tiles(T), npairs = B * S * (S + 1);
  const double* win = tables;
  const double2* tw = reinterpret_cast<const double2*>(tables + ST_FRAME);
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(B * S), dim3(256), 0, st, ref, lengths, S, T, Fmax, win, k.energy, k.idx, k.nk, kept, status);
  if (Fmax > 1)
    hipLaunchKernelGGL(stoi_band_kernel, dim3(cdiv(Fmax - 1, ST_FT), B * S * (S + 2)), dim3(256), 0, st, ref, est, mix, S, T, Fmax, win, tw,
                       k.idx, k.nk, k.bands);
  if (ntiles > 0)
    hipLaunchKernelGGL(stoi_seg_kernel, dim3(ntiles, npairs), dim3(256), 0, st, S, Fmax, ntiles, mix ? 1 : 0, k.nk, k.bands, k.part);
  hipLaunchKernelGGL(stoi_final_kernel, dim3(cdiv(npairs, 64)), dim3(64), 0, st, S, npairs, ntiles, mix ? 1 : 0, k.nk, k.part, stoi, estoi, stoi_mix,
                     estoi_mix);
  SEPR_CHECK_LAUNCH("stoi kernels");
  return SEPR_OK;
}
