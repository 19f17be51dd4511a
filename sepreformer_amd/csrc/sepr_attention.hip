// EGA self-attention over the pooled sequence with the relative-position key bias.
//
// reference: MultiHeadAttention.forward, modules/network.py:103-122 with pos_k from
// RelativePositionalEncoding, modules/module.py:52-57,196-198:
//     scores[i,j] = (q_i . k_j + q_i . pe_k[clamp(i - j, -maxlen, maxlen-1) + maxlen]) / sqrt(dk)
// The reference materialises pos_k as [T',T',dk] (16 MB at T'=500, 85 MB at 1150) and the scores as
// [b,H,T',T'].  Here neither exists:
//   * a workgroup = 64 queries of one (sequence, head) = 4 waves x 16 queries; keys are streamed in
//     64-key LDS tiles (K rows, V transposed, and the 127 consecutive rows i-j of the [2*maxlen, dk]
//     table that the tile can touch - the bias is Toeplitz);
//   * q.k^T and p.v run on the f32 MFMA (v_mfma_f32_16x16x4_f32) in the transposed form
//     S^T[key][query]: a lane then owns ONE query column and 4 keys per 16-key sub-tile, so the softmax
//     statistics are per-lane scalars (two shuffles across the 4 lane groups), the probabilities are
//     already the B operand of the p.v MFMA (no cross-lane movement), and the running output
//     O^T[d][query] is rescaled by a per-lane factor;
//   * the relative-position term is a per-lane VALU dot product of the lane's own q row with 4
//     consecutive band rows (the skewed index i-j does not map onto an MFMA fragment);
//   * exact online softmax (fp32, rescale every sub-tile), masked keys contribute exp(-1e30 - m) = 0.
#include "sepr_pointwise.h"
#include "sepr_train.h"

namespace sepr {

template <int DK>
__global__ __launch_bounds__(256) void relattn_kernel(const float* __restrict__ QKV, float* __restrict__ O, int Tp, int F,
                                                     const float* __restrict__ pe, int maxlen, float inv_sqrt_dk) {
  constexpr int QB = 64, KT = 64;
  constexpr int KS = DK + 4;          // K tile row stride   [KT][KS]
  constexpr int VS = KT + 4;          // V^T row stride      [DK][VS]
  constexpr int PS = DK + 4;          // band row stride     [QB + KT - 1][PS]
  constexpr int NBAND = QB + KT - 1;
  constexpr int NC = DK / 16;         // 16-wide d slices
  __shared__ __attribute__((aligned(16))) float Ks[KT * KS];
  __shared__ __attribute__((aligned(16))) float Vts[DK * VS];
  __shared__ __attribute__((aligned(16))) float pes[NBAND * PS];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ii = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * QB, h = blockIdx.y, seq = blockIdx.z;
  const int ld = 3 * F;
  const float* base = QKV + (long long)seq * Tp * ld + h * DK;
  const int i = i0 + 16 * w + ii;
  const bool active = i < Tp;

  // this lane's query row: full (for the VALU bias) and the MFMA B fragments d = 16c + 4g + r
  float qfull[DK];
  float4 qf[NC];
  {
    const float* qp = base + (long long)(active ? i : Tp - 1) * ld;
#pragma unroll
    for (int d = 0; d < DK; d += 4) {
      const float4 v = ld4(qp + d);
      qfull[d] = v.x * inv_sqrt_dk; qfull[d + 1] = v.y * inv_sqrt_dk;
      qfull[d + 2] = v.z * inv_sqrt_dk; qfull[d + 3] = v.w * inv_sqrt_dk;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float4 v = ld4(qp + 16 * c + 4 * g);
      qf[c] = make_float4(v.x * inv_sqrt_dk, v.y * inv_sqrt_dk, v.z * inv_sqrt_dk, v.w * inv_sqrt_dk);
    }
  }
  f32x4 o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float mrun = -1e30f, lrun = 0.f;

  for (int j0 = 0; j0 < Tp; j0 += KT) {
    __syncthreads();   // previous tile fully consumed
    // ---- stage K rows, V transposed, and the band of the position table --------------------------------
    for (int idx = tid; idx < KT * (DK / 4); idx += 256) {
      const int jj = idx / (DK / 4), c4 = idx % (DK / 4);
      const int j = j0 + jj;
      float4 kv = zero4(), vv = zero4();
      if (j < Tp) {
        const float* kp = base + (long long)j * ld + F + 4 * c4;
        kv = ld4(kp);
        vv = ld4(kp + F);
      }
      st4(Ks + jj * KS + 4 * c4, kv);
      Vts[(4 * c4 + 0) * VS + jj] = vv.x;
      Vts[(4 * c4 + 1) * VS + jj] = vv.y;
      Vts[(4 * c4 + 2) * VS + jj] = vv.z;
      Vts[(4 * c4 + 3) * VS + jj] = vv.w;
    }
    for (int idx = tid; idx < NBAND * (DK / 4); idx += 256) {
      const int rr = idx / (DK / 4), c4 = idx % (DK / 4);
      int rel = i0 - j0 - (KT - 1) + rr;                      // i - j for band row rr
      rel = rel < -maxlen ? -maxlen : (rel > maxlen - 1 ? maxlen - 1 : rel);
      st4(pes + rr * PS + 4 * c4, ld4(pe + (long long)(rel + maxlen) * DK + 4 * c4));
    }
    __syncthreads();

    const int nsub = (Tp - j0 >= KT) ? KT / 16 : (Tp - j0 + 15) / 16;
    for (int jt = 0; jt < nsub; ++jt) {
      // S^T[key = 16 jt + 4g + r][query = ii]
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float4 kf = ld4(Ks + (16 * jt + ii) * KS + 16 * c + 4 * g);
        s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[c].x, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[c].y, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[c].z, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[c].w, s, 0, 0, 0);
      }
      // relative-position bias: band row of (query 16w+ii, key 16jt+4g+r) is (16w+ii) - (16jt+4g+r) + KT-1
      const float* pb = pes + (16 * w + ii - 16 * jt - 4 * g + (KT - 1)) * PS;
      float bias[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* pr = pb - r * PS;
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < DK; d += 4) {
          const float4 p4 = ld4(pr + d);
          acc = fmaf(qfull[d], p4.x, acc);
          acc = fmaf(qfull[d + 1], p4.y, acc);
          acc = fmaf(qfull[d + 2], p4.z, acc);
          acc = fmaf(qfull[d + 3], p4.w, acc);
        }
        bias[r] = acc;
      }
      const int jbase = j0 + 16 * jt + 4 * g;
      float sv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[r] = (jbase + r < Tp) ? s[r] + bias[r] : -1e30f;
      float mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(mrun, mx);
      const float corr = __expf(mrun - mnew);
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = __expf(sv[r] - mnew);
      lrun = lrun * corr + ((p[0] + p[1]) + (p[2] + p[3]));
      mrun = mnew;
      // O^T[d = 16c + 4g + r][query = ii] += V^T[d][key] . P[key][query]
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        o[c][0] *= corr; o[c][1] *= corr; o[c][2] *= corr; o[c][3] *= corr;
        const float4 vf = ld4(Vts + (16 * c + ii) * VS + 16 * jt + 4 * g);
        o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.x, p[0], o[c], 0, 0, 0);
        o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.y, p[1], o[c], 0, 0, 0);
        o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.z, p[2], o[c], 0, 0, 0);
        o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf.w, p[3], o[c], 0, 0, 0);
      }
    }
  }
  float ltot = lrun + __shfl_xor(lrun, 16, 64);
  ltot += __shfl_xor(ltot, 32, 64);
  if (active) {
    const float inv = 1.0f / ltot;
    float* op = O + ((long long)seq * Tp + i) * F + h * DK + 4 * g;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      st4(op + 16 * c, make_float4(o[c][0] * inv, o[c][1] * inv, o[c][2] * inv, o[c][3] * inv));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// bf16x3 form of the same attention for dk = 16 (default arithmetic).  relattn_kernel above is VALU-bound: per 16 keys
// a lane spends 64 FMAs + 16 LDS reads on the relative-position bias against 8 f32 MFMAs (PMC: 74 % VALU-active,
// 31 % MFMA-busy).  Here all three products run on the bf16 MFMA with split operands (hi.hi + hi.lo + lo.hi):
//   * keys are walked 32 at a time; S^T = K q^T is one K=32 MFMA step per 16 keys (dk = 16 fills half of K, the
//     other half of the fragments is zero);
//   * the relative-position term is a THIRD product, P^T[b][query] = band[b] . q for the 47 band rows a
//     (16 queries x 32 keys) block can touch (3 row tiles), skewed through a per-wave LDS scratch:
//     bias(query, key) = P[query][query - key + 31].  9 cheap MFMAs + 3 LDS writes + 8 LDS reads replace 128 FMAs;
//   * O^T += V^T P: the 8 probabilities a lane holds (keys 4g+r of both 16-key halves) are exactly one K=32 B fragment
//     when V^T is read with the matching key-slot order, so PV is 3 MFMAs per 32 keys with no data movement.
// K, V^T and the band are split into bf16 hi/lo planes once per 64-key tile while they are staged into LDS.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int AT_NW = 4;   // 16-query waves per workgroup: 64 queries share every staged K / V / band tile
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split4(const float4 v, bf16x4& h, bf16x4& l) {
  const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const __bf16 hh = (__bf16)x[e];
    h[e] = hh;
    l[e] = (__bf16)(x[e] - (float)hh);
  }
}

// DK = 16 (Base): dk fills half of the K = 32 MFMA step, lane groups 2,3 carry zeros.  DK = 32 (Large): the step is full,
// O^T has two 16-row tiles (two PV accumulators), the staging moves twice the K / V / band rows per thread.
// TRAIN (sepr_train_attn_x3.hip's forward): additionally writes lse[(seq*H + h)*Tp + i] = log sum_j exp(score_ij) - all the
// backward keeps of the probabilities - and applies inverted dropout to the probabilities that multiply V (network.py:121;
// the softmax denominator sums the undropped ones); mask of element (row = (seq*H + h)*Tp + i, key j) = 16-bit half j & 1 of
// sepr_drop_word(dkey, row, j >> 1) >= thr (sepr_train.h).
// NWV stays a template parameter (always AT_NW): it is part of the kernel's symbol name.
template <int DK, bool TRAIN = false, bool BP = false, bool ONE = false, int NWV = AT_NW>
__global__ __launch_bounds__(64 * NWV, DK == 16 ? 4 : 2) void relattn_x3_kernel(const float* __restrict__ QKV, float* __restrict__ O, int Tp, int F,
                                                        const float* __restrict__ pe, int maxlen, float inv_sqrt_dk,
                                                        float* __restrict__ lse = nullptr, unsigned thr = 0u, float dscale = 1.0f,
                                                        unsigned long long seed = 0ull, const unsigned long long* __restrict__ salt = nullptr,
                                                        const unsigned short* __restrict__ pe_planes = nullptr) {
  constexpr bool PACK = false;
#include "sepr_attention_x3_body.h"
}

// Packed-K form of the dk = 16 inference attention (SEPR_ATTN_PACK, default on).  A head has 16 channels, the bf16 MFMA step has K = 32: above,
// lane groups 2,3 multiply zeros, a split product costs three such MFMAs and every K / band fragment is read from LDS twice (hi and lo plane).
// Here the A fragment is [x_hi | x_lo] - ONE read - and the B fragments are [q_hi | q_hi] and [q_lo | q_lo], so two MFMAs give the full
// four-term product: 24 MFMAs and 9 K / band fragment reads per 64-key tile instead of 33 and 18.  The kernel is bound by the LDS, not by the
// matrix pipe: the reads are what pays.  The bias is the accumulator the score MFMAs start from (no add), q carries
// log2(e) so the softmax is exp2 without the per-element multiply, and the K / band / V^T row strides are the conflict-free ones for these
// reads.  Staging, P.V, the online-softmax bookkeeping and the epilogue are the shared body's (sepr_attention_x3_body.h).
template <bool BP>
__global__ __launch_bounds__(64 * AT_NW, 4) void relattn_x3p_kernel(const float* __restrict__ QKV, float* __restrict__ O, int Tp, int F,
                                                                   const float* __restrict__ pe, int maxlen, float inv_sqrt_dk,
                                                                   const unsigned short* __restrict__ pe_planes) {
  constexpr int DK = 16, NWV = AT_NW;
  constexpr bool TRAIN = false, ONE = false, PACK = true;
  float* const lse = nullptr;                                  // the training-only parameters of the shared body, as constants
  const unsigned thr = 0u;
  const float dscale = 1.0f;
  const unsigned long long seed = 0ull;
  const unsigned long long* const salt = nullptr;
#include "sepr_attention_x3_body.h"
}

// train forward on the bf16x3 kernel: O, lse [n*H*Tp]; p > 0: dropout of the probabilities (16-bit generator, site 2)
int launch_relattn_x3_train_fwd(const float* QKV, float* O, float* lse, int n, int Tp, int F, int H, const float* pe_k, int maxlen,
                                float p, unsigned long long seed, const unsigned long long* salt, hipStream_t s, int one) {
  if (n <= 0 || Tp <= 0) return SEPR_OK;
  if (H <= 0 || F % H != 0 || maxlen <= 0 || !pe_k || !lse || n > 65535 || !(p >= 0.f) || !(p < 1.f)) return SEPR_EINVAL;
  const int dk = F / H;
  const dim3 grid((Tp + 63) / 64, H, n);
  const float isd = 1.0f / sqrtf((float)dk);
  const unsigned thr = p > 0.f ? sepr_drop_thr16(p) : 0u;
  const float dscale = p > 0.f ? sepr_drop_scale16(p) : 1.0f;
  const unsigned short* none = nullptr;
  if (dk == 16 && one) hipLaunchKernelGGL((relattn_x3_kernel<16, true, false, true>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, lse, thr, dscale, seed, salt, none);
  else if (dk == 16) hipLaunchKernelGGL((relattn_x3_kernel<16, true, false, false>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, lse, thr, dscale, seed, salt, none);
  else if (dk == 32 && one) hipLaunchKernelGGL((relattn_x3_kernel<32, true, false, true>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, lse, thr, dscale, seed, salt, none);
  else if (dk == 32) hipLaunchKernelGGL((relattn_x3_kernel<32, true, false, false>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, lse, thr, dscale, seed, salt, none);
  else return SEPR_EINVAL;
  SEPR_CHECK_LAUNCH("relattn_x3_kernel<train>");
  return SEPR_OK;
}

int launch_relattn(const float* QKV, float* O, int n, int Tp, int F, int H, const float* pe_k, int maxlen, int x3,
                   hipStream_t s, const void* pe_planes) {
  if (n <= 0 || Tp <= 0) return SEPR_OK;
  if (H <= 0 || F % H != 0 || maxlen <= 0 || !pe_k || n > 65535) return SEPR_EINVAL;
  const int dk = F / H;
  const dim3 grid((Tp + 63) / 64, H, n);
  const float isd = 1.0f / sqrtf((float)dk);
  if (dk == 16 && x3 && knob(SEPR_KNOB_ATTN_PACK) != 0) {
    if (pe_planes)
      hipLaunchKernelGGL((relattn_x3p_kernel<true>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, static_cast<const unsigned short*>(pe_planes));
    else
      hipLaunchKernelGGL((relattn_x3p_kernel<false>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, (const unsigned short*)nullptr);
  } else if (dk == 16 && x3) {
    if (pe_planes)
      hipLaunchKernelGGL((relattn_x3_kernel<16, false, true>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, (float*)nullptr, 0u, 1.0f, 0ull,
                         (const unsigned long long*)nullptr, static_cast<const unsigned short*>(pe_planes));
    else
      hipLaunchKernelGGL((relattn_x3_kernel<16, false, false>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, (float*)nullptr, 0u, 1.0f,
                         0ull, (const unsigned long long*)nullptr, (const unsigned short*)nullptr);
  } else if (dk == 32 && x3) {
    if (pe_planes)
      hipLaunchKernelGGL((relattn_x3_kernel<32, false, true>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, (float*)nullptr, 0u, 1.0f, 0ull,
                         (const unsigned long long*)nullptr, static_cast<const unsigned short*>(pe_planes));
    else
      hipLaunchKernelGGL((relattn_x3_kernel<32, false, false>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd, (float*)nullptr, 0u, 1.0f,
                         0ull, (const unsigned long long*)nullptr, (const unsigned short*)nullptr);
  } else if (dk == 16) {
    hipLaunchKernelGGL((relattn_kernel<16>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd);
  } else if (dk == 32) {
    hipLaunchKernelGGL((relattn_kernel<32>), grid, dim3(256), 0, s, QKV, O, Tp, F, pe_k, maxlen, isd);
  } else {
    return SEPR_EINVAL;
  }
  SEPR_CHECK_LAUNCH("relattn_kernel");
  return SEPR_OK;
}

}  // namespace sepr
