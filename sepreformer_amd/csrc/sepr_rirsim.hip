// Room impulse responses by the image-source method, simulated on the device: R shoebox rooms -> R responses of N
// samples in ONE call, so that a bank of simulated rooms can be redrawn at every epoch (reverb.RirBank.simulate / resimulate).
//
// The definition (include/sepr.h, sepr_rir_ism_fwd) makes the result independent of the order of summation: every image source adds an
// 81-tap windowed-sinc pulse, read from a table of 33 fractional positions the host built, and every tap goes into the response as the
// INTEGER rint((a v) 2^48).  Integer addition commutes, so the decomposition below - tiles, column splits, LDS atomics, global atomics -
// cannot change a bit, and a numpy restatement that walks the whole cube of images reproduces the sums exactly (tests/rirsim_ref.py).
//   rir_ism_kernel     one workgroup per (response, tile of 256 output samples, one of 8 column splits).  The images that can touch the tile
//                      lie in a spherical shell; threads stride over the (x image, y image) columns that cut the shell's outer sphere, solve
//                      the z-index intervals of the column analytically (widened by one), and apply the exact predicates of the definition
//                      to every image of the interval.  Image offsets are two float64 operations from (k, p), cheaper than a list in LDS;
//                      LDS holds the pulse table (21 KB), the powers of beta (8 KB, a sequential product by one thread while the others
//                      stage the table) and the int64 tile (2 KB), which takes the taps as 64-bit LDS atomic adds and is flushed with
//                      64-bit global atomic adds.  Heavy (late) tiles are dispatched first.
//   rir_finish_kernel  per response: the first maximum of |acc|, then float32(h / peak) or float32(h).
// The rooms table is device memory and not trusted: room sizes, positions and beta are clamped into their contract ranges, every image index
// range, the table row, the power index and every tap position are clamped, so a bad table gives wrong samples and bounded work, never an
// access outside acc, rir, lut or the LDS arrays.
#include "sepr_common.h"

#pragma clang fp contract(off)

namespace sepr {
namespace {
constexpr int RS_HW = 40;                  // half width of a pulse
constexpr int RS_TW = 2 * RS_HW + 1;       // taps of a pulse
constexpr int RS_Q = 32;                   // fractional steps of the pulse table
constexpr int RS_LUT = (RS_Q + 1) * RS_TW;
constexpr double RS_SCALE = 281474976710656.0;        // 2^48
constexpr double RS_FOURPI = 4.0 * 3.141592653589793; // float64(4 pi)
constexpr int RS_W = 256;                  // output samples per tile
constexpr int RS_TPB = 256;
constexpr int RS_SPLIT = 8;                // workgroups that share the columns of one tile
constexpr int RS_NPOW = 1024;              // entries of the table of powers of beta
constexpr int RS_KMAX = 511;               // |k| of any image index: n = |2 k - p| <= 1023
constexpr int RS_MAX_N = 16384;
constexpr double RS_LMIN = 1.5;            // smallest room dimension of the contract

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }   // NaN -> lo
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

struct RsAxis {
  double two_l, c0, c1;                    // 2 L;  s - m (parity 0);  -(s + m) (parity 1): offset(k, p) = k (2 L) + c_p
};

__device__ __forceinline__ RsAxis rs_axis(const double* __restrict__ room, int a) {
#pragma clang fp contract(off)
  const double L = clampd(room[a], RS_LMIN, 1.0e6);
  const double s = clampd(room[3 + a], 0.0, L), m = clampd(room[6 + a], 0.0, L);
  RsAxis x;
  x.two_l = 2.0 * L;
  x.c0 = s - m;
  x.c1 = -(s + m);
  return x;
}

__global__ __launch_bounds__(RS_TPB) void rir_ism_kernel(const double* __restrict__ rooms, int N, double fsc, const double* __restrict__ lut,
                                                         unsigned long long* __restrict__ acc, int ntiles) {
#pragma clang fp contract(off)
  __shared__ double lut_s[RS_LUT];
  __shared__ double bpow[RS_NPOW];
  __shared__ unsigned long long tile[RS_W];
  const int tid = threadIdx.x;
  const int tix = ntiles - 1 - (int)(blockIdx.x / RS_SPLIT), split = (int)(blockIdx.x % RS_SPLIT), r = blockIdx.y;
  const int t0 = tix * RS_W, tend = t0 + RS_W < N ? t0 + RS_W : N;
  const double* __restrict__ room = rooms + (long long)r * 10;
  const RsAxis ax = rs_axis(room, 0), ay = rs_axis(room, 1), az = rs_axis(room, 2);
  const double beta = clampd(room[9], 0.0, 1.0);
  // the shell of the tile: an image touches it iff t0 - HW <= i0 <= tend - 1 + HW; one sample of slack on either side for the search
  const double dhi = (double)(tend + RS_HW + 1) / fsc;
  const double dlo = (double)(t0 - RS_HW - 1 > 0 ? t0 - RS_HW - 1 : 0) / fsc;
  const double i0_lo = (double)(t0 - RS_HW), i0_hi = (double)(tend - 1 + RS_HW);
  const int Kx = (int)fmin((double)RS_KMAX, floor((dhi - ax.c1) / ax.two_l) + 1.0);
  const int Ky = (int)fmin((double)RS_KMAX, floor((dhi - ay.c1) / ay.two_l) + 1.0);
  const int nxe = 2 * (2 * Kx + 1), nye = 2 * (2 * Ky + 1);
  const int ncol = nxe * nye;                                              // <= 2046^2
  if (split * RS_TPB >= ncol) return;                                      // (workgroup-uniform) no column for this split

  for (int i = tid; i < RS_LUT; i += RS_TPB) lut_s[i] = lut[i];
  tile[tid] = 0ull;
  // an image at distance d has at most sqrt(3) d / Lmin + 3 reflections: the powers this tile can need
  const double lmin = 0.5 * fmin(ax.two_l, fmin(ay.two_l, az.two_l));
  const int nlim = (int)fmin((double)(RS_NPOW - 1), floor(1.7320508075688772 * dhi / lmin) + 4.0);
  for (int n = nlim + 1 + tid; n < RS_NPOW; n += RS_TPB) bpow[n] = 0.0;    // never read for a room of the contract
  if (tid == RS_TPB - 1) {                                                 // bpow[n] = bpow[n - 1] * beta: a sequential product, not pow
    double b = 1.0;
    bpow[0] = b;
    for (int n = 1; n <= nlim; ++n) {
      b = b * beta;
      bpow[n] = b;
    }
  }
  __syncthreads();

  const double dhi2 = dhi * dhi, dlo2 = dlo * dlo;
  for (int c = split * RS_TPB + tid; c < ncol; c += RS_SPLIT * RS_TPB) {
    const int ex = c % nxe, ey = c / nxe;
    const int px = ex & 1, kx = (ex >> 1) - Kx, py = ey & 1, ky = (ey >> 1) - Ky;
    const double dx = (double)kx * ax.two_l + (px ? ax.c1 : ax.c0);
    const double dy = (double)ky * ay.two_l + (py ? ay.c1 : ay.c0);
    const double q = dx * dx + dy * dy;
    const double zhi2 = dhi2 - q;
    if (!(zhi2 >= 0.0)) continue;                                          // the column misses the outer sphere
    const double zhi = sqrt(zhi2);
    const double zlo2 = dlo2 - q;
    const double zlo = zlo2 > 0.0 ? sqrt(zlo2) : 0.0;
    const int nxy = iabs(2 * kx - px) + iabs(2 * ky - py);
#pragma unroll 1
    for (int pz = 0; pz < 2; ++pz) {
      const double cz = pz ? az.c1 : az.c0;
      // offsets in [zlo, zhi] and in [-zhi, -zlo], each index interval widened by one; where the two meet they are walked as one
      const int kl = (int)clampd(ceil((zlo - cz) / az.two_l) - 1.0, -(double)RS_KMAX, (double)RS_KMAX);
      const int kh = (int)clampd(floor((zhi - cz) / az.two_l) + 1.0, -(double)RS_KMAX, (double)RS_KMAX);
      const int ml = (int)clampd(ceil((-zhi - cz) / az.two_l) - 1.0, -(double)RS_KMAX, (double)RS_KMAX);
      const int mh = (int)clampd(floor((-zlo - cz) / az.two_l) + 1.0, -(double)RS_KMAX, (double)RS_KMAX);
#pragma unroll 1
      for (int kz = ml; kz <= kh; ++kz) {
        if (kz > mh && kz < kl) kz = kl;                                   // the gap between the two intervals
        const double dz = (double)kz * az.two_l + cz;
        const double d = sqrt(q + dz * dz);
        const double tau = d * fsc;
        const double i0d = floor(tau);
        if (!(i0d >= i0_lo && i0d <= i0_hi)) continue;                     // the exact predicate: the pulse touches [t0, tend)
        int n = nxy + iabs(2 * kz - pz);
        n = n > RS_NPOW - 1 ? RS_NPOW - 1 : n;
        const double a = bpow[n] / (RS_FOURPI * d);
        if (a == 0.0) continue;                                            // every tap would add the integer 0
        const double f = tau - i0d;
        const double fq = f * (double)RS_Q;
        const double kf = floor(fq);
        const double w = fq - kf;
        int kk = (int)kf;
        kk = kk < 0 ? 0 : (kk > RS_Q - 1 ? RS_Q - 1 : kk);
        const int base = (int)i0d - RS_HW - t0;                            // tile index of tap 0: -2 HW .. tend - t0 - 1
        const int j0 = base < 0 ? -base : 0;
        const int j1 = tend - t0 - base < RS_TW ? tend - t0 - base : RS_TW;
        const double* __restrict__ l0 = lut_s + kk * RS_TW;
        for (int j = j0; j < j1; ++j) {
          const double v0 = l0[j], v1 = l0[j + RS_TW];
          const double v = v0 + w * (v1 - v0);
          const double ci = rint((a * v) * RS_SCALE);
          if (fabs(ci) < 4.0e18 && ci != 0.0) atomicAdd(&tile[base + j], (unsigned long long)(long long)ci);
        }
      }
    }
  }
  __syncthreads();
  const unsigned long long v = tile[tid];
  if (t0 + tid < tend && v != 0ull) atomicAdd(acc + (long long)r * N + t0 + tid, v);
}

// first maximum of |acc_r|, then the float32 response
__global__ __launch_bounds__(RS_TPB) void rir_finish_kernel(const long long* __restrict__ acc, int N, float* __restrict__ rir,
                                                            int* __restrict__ peak_idx, int normalise) {
#pragma clang fp contract(off)
  __shared__ unsigned long long red_m[RS_TPB / 64];
  __shared__ int red_i[RS_TPB / 64];
  const int tid = threadIdx.x, r = blockIdx.x;
  const long long* __restrict__ a = acc + (long long)r * N;
  unsigned long long best = 0ull;
  int bidx = N;
  for (int t = tid; t < N; t += RS_TPB) {
    const long long s = a[t];
    const unsigned long long m = s < 0 ? 0ull - (unsigned long long)s : (unsigned long long)s;
    if (m > best) best = m, bidx = t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long om = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bidx, o, 64);
    if (om > best || (om == best && oi < bidx)) best = om, bidx = oi;
  }
  if ((tid & 63) == 0) red_m[tid >> 6] = best, red_i[tid >> 6] = bidx;
  __syncthreads();
  best = red_m[0], bidx = red_i[0];
#pragma unroll
  for (int k = 1; k < RS_TPB / 64; ++k) {
    if (red_m[k] > best || (red_m[k] == best && red_i[k] < bidx)) best = red_m[k], bidx = red_i[k];
  }
  if (best == 0ull) bidx = 0;                                               // an all-zero response: numpy's argmax, and zeros out
  if (tid == 0) peak_idx[r] = bidx;
  const double peak = (double)best / RS_SCALE;
  float* __restrict__ out = rir + (long long)r * N;
  for (int t = tid; t < N; t += RS_TPB) {
    const double h = (double)a[t] / RS_SCALE;
    out[t] = normalise ? (best != 0ull ? (float)(h / peak) : 0.f) : (float)h;
  }
}
}  // namespace
}  // namespace sepr

extern "C" int sepr_rir_ism_fwd(const double* rooms, int R, int N, double fsc, const double* lut, long long* acc, float* rir, int* peak_idx,
                                int normalise, sepr_stream_t stream) {
  using namespace sepr;
  if (!rooms || !lut || !acc || !rir || !peak_idx) return SEPR_EINVAL;
  if (R < 1 || R > 65535 || N < 1 || N > RS_MAX_N || (normalise != 0 && normalise != 1)) return SEPR_EINVAL;
  if (!(fsc > 0.0) || !(fsc < 1.0e12)) return SEPR_EINVAL;
  // the table of powers of beta and the image index range, for the smallest room the kernel admits
  if (!(1.7320508075688772 * (double)(N + RS_HW + 1) / fsc / RS_LMIN + 3.0 < (double)RS_NPOW)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(rooms) | reinterpret_cast<uintptr_t>(lut) | reinterpret_cast<uintptr_t>(acc)) % 8 != 0) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(rir) | reinterpret_cast<uintptr_t>(peak_idx)) % 4 != 0) return SEPR_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = hipMemsetAsync(acc, 0, (size_t)R * N * sizeof(long long), st);
  if (e != hipSuccess) {
    set_hip_error(e, "rir ism memset");
    return SEPR_EHIP;
  }
  const int ntiles = cdiv(N, RS_W);
  hipLaunchKernelGGL(rir_ism_kernel, dim3((unsigned)(ntiles * RS_SPLIT), (unsigned)R), dim3(RS_TPB), 0, st, rooms, N, fsc, lut,
                     reinterpret_cast<unsigned long long*>(acc), ntiles);
  hipLaunchKernelGGL(rir_finish_kernel, dim3((unsigned)R), dim3(RS_TPB), 0, st, acc, N, rir, peak_idx, normalise);
  SEPR_CHECK_LAUNCH("rir ism kernels");
  return SEPR_OK;
}
