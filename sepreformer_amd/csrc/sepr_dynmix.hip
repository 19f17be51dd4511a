// Dynamic mixing from a device-resident corpus: the training batch of the reference's *_DM_* data sets
// (models/SepReformer_Large_DM_*/dataset.py::_dynamic_mixing + _collate) built by ONE launch from a plan table.
//
// The corpus is two contiguous buffers - int16 utterances (PCM16 files as they are on disk) and float32 utterances - with one
// int64 table of cumulative element counts: utterance u < N16 is buf16[off[u] .. off[u + 1]), utterance u >= N16 is
// buf32[off[u] - off[N16] .. off[u + 1] - off[N16]).
//   energy_part_kernel / energy_finish_kernel   sum of squares per utterance, once at load: int64 for int16 utterances (exact, so
//                        independent of the order), float64 in a fixed order for float32 utterances; per-workgroup partials and a
//                        finishing pass, no atomics;
//   dynmix_kernel<S, F>  the mixing skeleton of the plain and the reverberant launch: zero fill from n[b] on, the M terms scaled by two
//                        separately rounded multiplies and summed in term order, float4 stores of the mixture and the S target rows, a
//                        target that IS its mixture term (every field of the form equal) stored from the kept values.
//     F = PlainForm      (sepr_dynmix_fwd) one thread per eight output samples of one example: every term is eight consecutive samples
//                        from an arbitrary start, read as aligned 16-byte loads from the aligned-down address and realigned in
//                        registers (v_alignbyte for the odd int16 starts).  No LDS, no barrier, a thread past Tmax or n returns early.
//     F = ReverbForm     (sepr_dynmix_reverb_fwd) a term whose rir is an index into the RIR bank is the stored
//                        utterance convolved with the first taps samples of that impulse response, exact float64 products summed in the
//                        order j = 0 .. taps - 1, one rounding.  2048 outputs of one example per workgroup, one output per lane,
//                        transposed through a float tile; the taps are walked in ascending chunks of 1024, each staging its 3071 input
//                        samples and its taps as doubles in LDS, the float64 accumulators staying in registers - so the 32 768-byte LDS
//                        plan does not depend on the response's length.  It holds barriers: no thread returns early, and n, a term's
//                        integer fields and the same-term flag are wave-uniform (readfirstlane) before any branch around a barrier.
//     F = SpeedReverbForm (sepr_dynmix_speed_reverb_fwd, section 5e-5) a term may carry a converter AND a response: the utterance perturbed
//                        first, reverberated second.  The geometry of ReverbForm; per tap chunk the span of the perturbed utterance that the
//                        chunk reaches is converted into LDS as doubles (the converter of sepr_polyphase.h, in passes whose input span fits the
//                        staged doubles), then the FIR loop runs over it.  57 344 bytes of LDS; a term with one of the two takes that
//                        form's code and gives its bits.
//     F = TurnsForm      (sepr_dynmix_turns_fwd, section 5e-6) SpeedReverbForm's term with a turn [on, off): the talker's float32 signal under a
//                        raised-cosine gate BEFORE the response, so the room rings on after the talker stops.  The gate is a parameter of the
//                        four staging paths (NoGate in every other form: their code); a tile or a tap chunk that reaches only closed samples
//                        is skipped.
//   dynmix_speed_kernel  (sepr_dynmix_speed_fwd, section 5e-2) the same batch with speed perturbation, a kernel of its own (docs/HISTORY.md:
//                        as an instance of the skeleton it ran 0.8 to 1.1 us longer per launch at B = 16): a term whose term_conv is a converter
//                        index is the stored utterance through that rational-ratio converter (sepr_polyphase.h).  The
//                        same tile geometry: input span staged in LDS as doubles, outputs converted one per lane, transposed through an
//                        LDS tile of floats.  It shares term_value, scale8, store8 and the launcher.
// Nothing here depends on the launch order of workgroups: results are bit-identical from run to run.
#include "sepr_polyphase.h"

namespace sepr {
namespace {
constexpr int DM_TPB = 256;        // threads per workgroup of the mixing kernel
constexpr int DM_PER = 8;          // output samples per thread
constexpr int EN_TPB = 256;        // threads per workgroup of the energy kernel = samples per chunk
constexpr int EN_PARTS = 8;        // workgroups (partials) per utterance: workgroup p takes the chunks c = p, p + 8, ...

struct DmRows {
  float* p[3];
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint4 ldu4(const void* p) { return *reinterpret_cast<const uint4*>(p); }

// eight consecutive int16 samples from element e (any parity) of buf as floats s * 2^-15 (exact).  Two aligned 16-byte loads at
// the aligned-down element e & ~7; pad = the buffer's element count rounded up to 8 (allocated), so no load leaves the buffer.
__device__ __forceinline__ void load8_i16(const short* __restrict__ buf, long long e, long long pad, float out[8]) {
  const long long a0 = e & ~7LL;
  const uint4 lo = ldu4(buf + a0);
  const uint4 hi = a0 + 8 < pad ? ldu4(buf + a0 + 8) : make_uint4(0u, 0u, 0u, 0u);
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const int sh = (int)(e & 7), ds = sh >> 1;
  unsigned u[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) u[k] = ds == 0 ? w[k] : (ds == 1 ? w[k + 1] : (ds == 2 ? w[k + 2] : w[k + 3]));
  const bool odd = sh & 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned d = odd ? __builtin_amdgcn_alignbyte(u[k + 1], u[k], 2) : u[k];
    out[2 * k] = (float)(short)(d & 0xffffu) * 3.0517578125e-05f;
    out[2 * k + 1] = (float)((int)d >> 16) * 3.0517578125e-05f;
  }
}

// eight consecutive float32 samples from element e (any) of buf: three aligned 16-byte loads at e & ~3; pad = the element count
// rounded up to 4.
__device__ __forceinline__ void load8_f32(const float* __restrict__ buf, long long e, long long pad, float out[8]) {
  const long long a0 = e & ~3LL;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 q0 = ldu4(buf + a0);
  const uint4 q1 = a0 + 4 < pad ? ldu4(buf + a0 + 4) : z;
  const uint4 q2 = a0 + 8 < pad ? ldu4(buf + a0 + 8) : z;
  const unsigned w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
  const int sh = (int)(e & 3);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = __uint_as_float(sh == 0 ? w[k] : (sh == 1 ? w[k + 1] : (sh == 2 ? w[k + 2] : w[k + 3])));
}

struct DmCorpus {
  const short* buf16;
  const float* buf32;
  const long long* off;
  long long total16, total32;
  int N16, N;
};

// (sample * norm) * gain of every form: two roundings, as numpy's `samps *= norm_factor` followed by `gain * samps`
__device__ __forceinline__ void scale8(const float x[8], float norm, float gain, float v[8]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float a = x[i] * norm;
    v[i] = a * gain;
  }
}

// ---- turns: a gate on the talker's float32 signal, before any response ------------------------------------------
// A gate is a parameter of the four staging paths below (term_value, convert_tile, reverb_tile's staged input, speed_reverb_tile's perturbed
// span).  Term time is t = p - start (p the sample's index in the stored or perturbed utterance, so t is the output sample it reaches through tap 0;
// negative in a response's history).  A path rebases the gate once, on scalars, to the term time of its first staged sample - gate.at(base) - and
// then gates sample i of its span with 32-bit arithmetic: gate(y, i).  NoGate is the identity and leaves the code each path had.
struct NoGate {
  static constexpr bool kOn = false;
  __device__ __forceinline__ NoGate at(long long) const { return {}; }
  __device__ __forceinline__ float operator()(float y, int) const { return y; }
};

// the turn [on, off) of one term under the raised-cosine table ramp [RL]:  w(t) = 0 outside the turn, ramp[min(t - on, off - 1 - t)] where that
// is below RL, else 1.  on and off are clamped to [-2^30, 2^30] where the table is read (TurnsForm::cols) and again when the gate is rebased (an end
// 2^30 samples from a span of a few thousand is out of its reach either way), and a span's index i lies within a few thousand of 0: no difference
// overflows 32 bits.  The ramp index lies in [0, RL).  A closed gate SELECTS +0 (never -0, whatever y holds), an open one multiplies once in
// float32, and w = 1 is y itself (y * 1.0f is y).
struct TurnGate {
  static constexpr bool kOn = true;
  int on, off, RL;
  const float* __restrict__ ramp;
  __device__ __forceinline__ TurnGate at(long long base) const {
    return {(int)clampll(on - base, -(1 << 30), 1 << 30), (int)clampll(off - base, -(1 << 30), 1 << 30), RL, ramp};
  }
  __device__ __forceinline__ float operator()(float y, int i) const {
#pragma clang fp contract(off)
    const int d = i - on, e = off - 1 - i;
    if ((d | e) < 0) return 0.f;
    const int m = d < e ? d : e;
    return m < RL ? y * ramp[m] : y;
  }
  // outputs [t_lo, t_hi) of a term under K taps (K = 1 without a response) reach gated samples at t - j, j < K: all of them closed?
  __device__ __forceinline__ bool silent(long long t_lo, long long t_hi, int K) const { return t_lo >= (long long)off + (K - 1) || t_hi <= on; }
};

// (sample * norm) * gain of the stored term (utt, start) on samples t0 .. t0 + 7.  The table is not trusted: the utterance index, the start
// and the element position are clamped, so whatever it holds no read leaves the corpus buffers.
template <class G = NoGate>
__device__ __forceinline__ void term_value(const DmCorpus& c, int utt, int start, float norm, float gain, int t0, float v[8], const G& gate = G{},
                                           int i0 = 0) {                     // i0: the gate's index of sample t0
  const int u = utt < 0 ? 0 : (utt >= c.N ? c.N - 1 : utt);
  const long long o0 = c.off[u], len = c.off[u + 1] - o0;
  const long long st = clampll(start, 0, len > 0 ? len : 0);
  float x[8];
  if (u < c.N16) {
    load8_i16(c.buf16, clampll(o0 + st + t0, 0, c.total16 - 1), (c.total16 + 7) & ~7LL, x);
  } else {
    load8_f32(c.buf32, clampll(o0 - c.off[c.N16] + st + t0, 0, c.total32 - 1), (c.total32 + 3) & ~3LL, x);
  }
  if constexpr (G::kOn) {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = gate(x[i], i0 + i);
  }
  scale8(x, norm, gain, v);
}

__device__ __forceinline__ void store8(float* __restrict__ row, const float v[8], int t0, int n, bool second) {
  float m[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = t0 + i < n ? v[i] : 0.f;
  st4(row, make_float4(m[0], m[1], m[2], m[3]));
  if (second) st4(row + 4, make_float4(m[4], m[5], m[6], m[7]));
}

// ---- the tiled forms: a workgroup makes DS_TILE outputs of one example, one output per lane, through 32 768 bytes of LDS ----------
constexpr int DS_TILE = DM_TPB * DM_PER;   // output samples per workgroup
constexpr int DS_SPAN = 3072;              // doubles of staged input: (DS_TILE - 1) M / L + K + 1 must fit (speeds of about 70 % to 140 %)
constexpr int DR_CHUNK = 1024;             // taps per chunk: the chunk's span DS_TILE + DR_CHUNK - 1 = 3071 doubles fits xs [DS_SPAN]
constexpr int DR_MAX_TAPS = 16384;
static_assert(DS_TILE + DR_CHUNK - 1 <= DS_SPAN, "a chunk's input span must fit the staged doubles");
static_assert(DR_CHUNK * sizeof(double) == DS_TILE * sizeof(float), "the chunk's taps as doubles share the float tile");

struct DsLds {
  double xs[DS_SPAN];                                  // the staged input span
  __attribute__((aligned(16))) double hs[DR_CHUNK];    // a chunk's taps; at the end of a term the tile of DS_TILE floats
};

// one utterance's slice of the corpus buffers.  The table is not trusted: the index is clamped and every staged element position is
// clamped into its buffer, so whatever span is asked for no read leaves the corpus.
struct DmUtt {
  long long T, e0, total;                  // samples of the utterance, its first element in its buffer, the buffer's element count
  bool is16;

  __device__ __forceinline__ DmUtt(const DmCorpus& c, int utt) {
    const int u = utt < 0 ? 0 : (utt >= c.N ? c.N - 1 : utt);
    const long long o0 = c.off[u];
    T = c.off[u + 1] - o0;
    is16 = u < c.N16;
    total = is16 ? c.total16 : c.total32;
    e0 = o0 - (is16 ? 0 : c.off[c.N16]);
  }

  // xs[i] = double(sample g0 + i) for i < count, zero outside [0, T); all threads of the workgroup, no barrier
  __device__ __forceinline__ void stage(const DmCorpus& c, long long g0, int count, double* __restrict__ xs) const {
    pp_stage<DM_TPB>(xs, count, g0, T, [&](long long g, int) {
      const long long e = clampll(e0 + g, 0, total - 1);
      return is16 ? (double)((float)c.buf16[e] * 3.0517578125e-05f) : (double)c.buf32[e];
    });
  }

  // the same under a gate rebased to the term time of sample g0: sample g0 + i is gated as a float32, at index i, and widened after
  template <class G>
  __device__ __forceinline__ void stage(const DmCorpus& c, long long g0, int count, double* __restrict__ xs, const G& gate) const {
    if constexpr (!G::kOn) {
      stage(c, g0, count, xs);
    } else {
      pp_stage<DM_TPB>(xs, count, g0, T, [&](long long g, int i) {
        const long long e = clampll(e0 + g, 0, total - 1);
        return (double)gate(is16 ? (float)c.buf16[e] * 3.0517578125e-05f : c.buf32[e], i);
      });
    }
  }
};

// the tile's outputs from one per lane (thread tid holds t = tile0 + tid + DM_TPB i) to x[0 .. 7] = t0 .. t0 + 7 (t0 = tile0 + 8 tid),
// transposed through the float tile; the caller has made sure that nobody still reads ys.  One barrier.
__device__ __forceinline__ void tile_out8(const double acc[DM_PER], float* __restrict__ ys, float x[8]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < DM_PER; ++i) ys[tid + i * DM_TPB] = (float)acc[i];
  __syncthreads();
  const float4 lo = *reinterpret_cast<const float4*>(ys + tid * DM_PER);
  const float4 hi = *reinterpret_cast<const float4*>(ys + tid * DM_PER + 4);
  x[0] = lo.x, x[1] = lo.y, x[2] = lo.z, x[3] = lo.w, x[4] = hi.x, x[5] = hi.y, x[6] = hi.z, x[7] = hi.w;
}

struct DrBank {
  const float* h;                          // the R impulse responses back to back
  const long long* off;                    // [R + 1] cumulative sample counts
  long long total;
  int R;
};

// the first K of `taps` samples of response r >= 0 at hp; the table is not trusted: both are clamped so that every tap read is inside the bank
struct DrResp {
  int K;
  const float* __restrict__ hp;
  __device__ __forceinline__ DrResp(const DrBank& bk, int r, int taps) {
    const int rr = r >= bk.R ? bk.R - 1 : r;
    const long long h0 = clampll(bk.off[rr], 0, bk.total - 1);
    const long long hl = clampll(bk.off[rr + 1] - h0, 1, bk.total - h0 < DR_MAX_TAPS ? bk.total - h0 : DR_MAX_TAPS);
    K = taps < 1 ? 1 : (taps > (int)hl ? (int)hl : taps);
    hp = bk.h + h0;
  }
};

// outputs t = tile0 .. tile0 + DS_TILE - 1 of term (utt, start) convolved with the first `taps` samples of impulse response r, as
//   y[t] = float32(sum_{j < taps} double(h[j]) * double(x[start + t - j])),   x = 0 outside [0, T) of that utterance,
// left in x8[0 .. 7] for t = t0 .. t0 + 7 of thread tid (t0 = tile0 + 8 tid).  Workgroup-uniform arguments; every thread of the workgroup
// passes every barrier.  Thread tid owns the outputs tid + 256 i: consecutive lanes read consecutive doubles of xs, and the tap is one
// broadcast read.  hs is the taps of a chunk as doubles while the chunks run, the tile of floats at the end.
// The tables are not trusted: r, taps, the utterance and every read position are clamped, so no read leaves the bank or the corpus.
// Under a gate x is the gated utterance; a chunk that reaches only closed samples adds fma(h, +0, acc) = acc and is skipped, as one before the
// utterance is (the turn is workgroup-uniform, so the barriers stay matched).
template <class G = NoGate>
__device__ __forceinline__ void reverb_tile(const DmCorpus& c, const DrBank& bk, int r, int taps, int utt, int start, int tile0, int n,
                                            DsLds& lds, float x8[8], const G& gate = G{}) {
  const int tid = threadIdx.x;
  const DmUtt ut(c, utt);
  const long long st = clampll(start, 0, ut.T > 0 ? ut.T : 0);
  const DrResp rs(bk, r, taps);                                              // r >= 0 here
  const int K = rs.K;
  const float* __restrict__ hp = rs.hp;
  const int left = n - tile0;                                                // > 0: the caller returned for tiles past n
  double acc[DM_PER];
#pragma unroll
  for (int i = 0; i < DM_PER; ++i) acc[i] = 0.0;
  double* __restrict__ hs = lds.hs;
  const double* xp = lds.xs + tid + (DR_CHUNK - 1);
  for (int k0 = 0; k0 < K; k0 += DR_CHUNK) {
    const long long g0 = st + tile0 - k0 - (DR_CHUNK - 1);                  // the utterance index of xs[0]
    // a chunk whose whole span lies before the utterance's first sample adds fma(h, 0, acc) = acc (acc is never -0): it and every
    // later chunk - their spans lie further back still - are skipped without changing a bit
    if (g0 + (DS_TILE + DR_CHUNK - 2) < 0) break;
    const int kc = K - k0 < DR_CHUNK ? K - k0 : DR_CHUNK;
    if constexpr (G::kOn) {                                                  // the chunk's outputs below n, as a term of its own under kc taps
      const long long ta = (long long)tile0 - k0, tb = ta + (left < DS_TILE ? left : DS_TILE);
      if (tb <= gate.on) break;                                              // later chunks reach further back still
      if (gate.silent(ta, tb, kc)) continue;
    }
    __syncthreads();                                                         // the last readers of xs / hs (or of the float tile) are done
    ut.stage(c, g0, DS_TILE + DR_CHUNK - 1, lds.xs, gate.at(g0 - st));
    for (int i = tid; i < kc; i += DM_TPB) hs[i] = (double)hp[k0 + i];
    __syncthreads();
    if (tid < left) {                                                        // (per wave: whole waves past n skip the loop)
#pragma unroll 4
      for (int j = 0; j < kc; ++j) {
        const double hj = hs[j];
#pragma unroll
        for (int i = 0; i < DM_PER; ++i) acc[i] = fma(hj, xp[i * DM_TPB - j], acc[i]);
      }
    }
  }
  __syncthreads();                                                           // hs has been read: it becomes the float tile
  tile_out8(acc, reinterpret_cast<float*>(hs), x8);
}

// outputs t = tile0 .. tile0 + DS_TILE - 1 (below n) of the perturbed utterance of term (utt, start) through converter (tp, L, M, K), left in
// ys[t - tile0]; thread tid then owns ys[8 tid .. 8 tid + 7].  Workgroup-uniform arguments; two barriers.  The table is not trusted:
// whatever it holds, the staging reads stay inside the utterance's slice of the corpus buffers.  A gate acts on the perturbed sample, at its output.
template <class G = NoGate>
__device__ __forceinline__ void convert_tile(const DmCorpus& c, int utt, int start, const float* __restrict__ tp, int L, int M, int K,
                                             int tile0, int n, double* __restrict__ xs, float* __restrict__ ys, const G& gate = G{}) {
  const int tid = threadIdx.x;
  const DmUtt ut(c, utt);
  const long long n0 = (long long)(start < 0 ? 0 : start) + tile0;          // first output of the tile, as an index of the perturbed utterance
  const int Hh = (K - 2) / 2;
  const long long b0 = pp_base(n0, L, M), g0 = b0 - Hh;
  const int span = (int)pp_span(DS_TILE, L, M, K);                           // <= DS_SPAN: the entry refuses any other converter
  ut.stage(c, g0, span, xs);
  __syncthreads();
  const int left = n - tile0;                                                // > 0: the caller returned for tiles past n
  const int lim = span - K;                                                  // highest window base inside the staged span
  double acc[DM_PER] = {};
  const double* xp[DM_PER];
  const float* tq[DM_PER];
#pragma unroll
  for (int i = 0; i < DM_PER; ++i) {
    const long long nn = n0 + tid + i * DM_TPB;
    xp[i] = xs + pp_window(nn, L, M, b0, lim);                               // 0 .. (DS_TILE - 1) M / L + 1
    tq[i] = tp + pp_phase(nn, L);
  }
  if (tid < left) pp_chain<DM_PER, 2>(tq, (long long)L, xp, K, acc);         // (per wave: whole waves past n skip the loop)
#pragma unroll
  for (int i = 0; i < DM_PER; ++i) ys[tid + i * DM_TPB] = gate((float)acc[i], tid + i * DM_TPB);       // the caller rebased the gate to tile0
  __syncthreads();
}

// a term of the speed kernel on samples t0 .. t0 + 7: through its converter when it has one, else term_value
__device__ __forceinline__ void speed_term_value(const DmCorpus& c, const ConvSet& cv, int conv, int utt, int start, float norm, float gain,
                                                 int tile0, int t0, int n, double* xs, float* ys, float v[8]) {
#pragma clang fp contract(off)
  if (conv < 0 || cv.NC < 1) {
    term_value(c, utt, start, norm, gain, t0 < n ? t0 : 0, v);
    return;
  }
  const int k = conv >= cv.NC ? cv.NC - 1 : conv;
  convert_tile(c, utt, start, cv.taps[k], cv.L[k], cv.M[k], cv.K[k], tile0, n, xs, ys);
  const float4 lo = *reinterpret_cast<const float4*>(ys + threadIdx.x * DM_PER);
  const float4 hi = *reinterpret_cast<const float4*>(ys + threadIdx.x * DM_PER + 4);
  const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  scale8(x, norm, gain, v);
}

// The speed launch keeps the body and the code it had before the skeleton (per-lane reads of n and the term fields included: every lane
// reads the same address, which is what keeps its barriers safe).
template <int S>
__global__ __launch_bounds__(DM_TPB) void dynmix_speed_kernel(DmCorpus c, ConvSet cv, const int* __restrict__ term_utt,
                                                              const int* __restrict__ term_start, const float* __restrict__ term_norm,
                                                              const float* __restrict__ term_gain, const int* __restrict__ term_conv,
                                                              const int* __restrict__ nlen, int M, int Tmax, float* __restrict__ mix, DmRows src) {
#pragma clang fp contract(off)
  __shared__ double xs[DS_SPAN];
  __shared__ __attribute__((aligned(16))) float ys[DS_TILE];
  const int b = blockIdx.y;
  const int tile0 = blockIdx.x * DS_TILE;
  const int t0 = tile0 + threadIdx.x * DM_PER;
  const bool live = t0 < Tmax;                                     // no early return for a thread: the conversions hold barriers
  const bool second = t0 + 4 < Tmax;
  int n = nlen[b];
  n = n < 0 ? 0 : (n > Tmax ? Tmax : n);
  const long long row = (long long)b * Tmax + t0;
  float acc[8], keep[S][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (tile0 >= n) {                                                // the whole tile is the zero fill of pad_sequence (workgroup-uniform)
    if (live) {
      store8(mix + row, acc, t0, n, second);
#pragma unroll
      for (int s = 0; s < S; ++s) store8(src.p[s] + row, acc, t0, n, second);
    }
    return;
  }
  const int NT = M + S, j0 = b * NT;
#pragma unroll
  for (int m = 0; m < S + 1; ++m) {
    if (m < M) {
      float v[8];
      const int conv = __builtin_amdgcn_readfirstlane(term_conv[j0 + m]);
      speed_term_value(c, cv, conv, term_utt[j0 + m], term_start[j0 + m], term_norm[j0 + m], term_gain[j0 + m], tile0, t0, n, xs, ys, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = acc[i] + v[i];
      if (m < S) {
#pragma unroll
        for (int i = 0; i < 8; ++i) keep[m][i] = v[i];
      }
    }
  }
  if (live) store8(mix + row, acc, t0, n, second);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int jm = j0 + s, jt = j0 + M + s;
    const int conv = __builtin_amdgcn_readfirstlane(term_conv[jt]);
    const bool same = term_utt[jt] == term_utt[jm] && term_start[jt] == term_start[jm] &&
                      __float_as_uint(term_norm[jt]) == __float_as_uint(term_norm[jm]) &&
                      __float_as_uint(term_gain[jt]) == __float_as_uint(term_gain[jm]) && conv == term_conv[jm];
    if (same) {
      if (live) store8(src.p[s] + row, keep[s], t0, n, second);
    } else {
      float v[8];
      speed_term_value(c, cv, conv, term_utt[jt], term_start[jt], term_norm[jt], term_gain[jt], tile0, t0, n, xs, ys, v);
      if (live) store8(src.p[s] + row, v, t0, n, second);
    }
  }
}

// ---- the forms of a term: what the mixing skeleton below does not share ---------------------------------------------------------
// A form is the kernel's first argument - the corpus and the banks its terms read, side by side as the kernels before it took them - and says
//   kTiled          whether value8 holds barriers: then no thread returns early, n, the term's integer fields and the `same` flag are
//                   wave-uniform (readfirstlane) before any branch around a barrier, and the zero fill is decided per workgroup;
//   Cols, cols()    the columns of term j beyond (utt, start, norm, gain), read from the table's extra columns `col...` (kernel
//                   parameters of their own, where the kernels before had them, so they stay __restrict__ and the reads scalar loads);
//   same(a, b)      whether those columns name the same term;
//   value8(...)     (raw * norm) * gain of the term on samples t0 .. t0 + 7 of this thread: scale8 of its eight raw samples - the
//                   stored ones (term_value) or the chunked FIR filter's tile.
struct PlainForm {
  static constexpr bool kTiled = false;
  DmCorpus c;
  struct Cols {};
  __device__ __forceinline__ static Cols cols(int) { return {}; }
  __device__ __forceinline__ static bool same(Cols, Cols) { return true; }
  __device__ __forceinline__ void value8(int utt, int start, float norm, float gain, Cols, int, int t0, int, float v[8]) const {
    term_value(c, utt, start, norm, gain, t0, v);
  }
};

// the speed entry's corpus and converters for dynmix_launch; its kernel is dynmix_speed_kernel, not an instance of the skeleton
struct SpeedForm {
  DmCorpus c;
  ConvSet cv;
};

// a term whose rir is an index into the bank is the stored utterance under the first taps samples of that response; rir < 0: as stored
struct ReverbForm {
  static constexpr bool kTiled = true;
  DmCorpus c;
  DrBank bk;
  struct Cols {
    int rir, taps;
  };
  __device__ __forceinline__ static Cols cols(const int* __restrict__ term_rir, const int* __restrict__ term_taps, int j) {
    return {__builtin_amdgcn_readfirstlane(term_rir[j]), __builtin_amdgcn_readfirstlane(term_taps[j])};
  }
  __device__ __forceinline__ static bool same(Cols a, Cols b) { return a.rir == b.rir && a.taps == b.taps; }
  __device__ __forceinline__ void value8(int utt, int start, float norm, float gain, Cols t, int tile0, int t0, int n, float v[8]) const {
    if (t.rir < 0) {
      term_value(c, utt, start, norm, gain, t0 < n ? t0 : 0, v);
      return;
    }
    __shared__ DsLds lds;
    float x[8];
    reverb_tile(c, bk, t.rir, t.taps, utt, start, tile0, n, lds, x);
    scale8(x, norm, gain, v);
  }
};

// ---- speed perturbation, then the room ------------------------------------------------------------------------
// 57 344 bytes of LDS: the 32 768 of the two tiled forms before it - which the terms with only a converter (convert_tile) or only a response
// (reverb_tile) use exactly as those forms do - and the perturbed span of a tap chunk as doubles.
struct SrLds {
  DsLds a;                                             // xs: the staged INPUT span of a conversion pass; hs: a chunk's taps, then the float tile
  double ys[DS_SPAN];                                  // the chunk's span of the PERTURBED utterance, float32 values widened
};
static_assert(sizeof(SrLds) <= 57344, "static LDS of the combined form");

// perturbed samples of the positions i = i0 + tid + 256 k (k < NI) below i1 into yd[i]: position i is sample q0 + i >= 0 of the perturbed utterance,
//   y[q] = float32(sum_{j < K} double(tap[(q M) mod L][j]) * x[floor(q M / L) - Hh + j]),
// the window and the chain of sepr_polyphase.h; xs[0] is input sample b0 - Hh and `span` doubles are staged.  No barrier.  Every window base is clamped into
// [0, span - K] (span <= DS_SPAN, K <= span: the entry refuses any other converter) and every phase lies in [0, L): no read leaves xs or the tap table.
// Under a gate - rebased to the term time of position 0 - the float32 perturbed sample is gated before it is widened.
template <int NI, class G = NoGate>
__device__ __forceinline__ void convert_group(const double* __restrict__ xs, int span, long long b0, const float* __restrict__ tp, int L, int M,
                                              int K, long long q0, int i0, int i1, double* __restrict__ yd, const G& gate = G{}) {
  const int tid = threadIdx.x;
  if (i0 + tid >= i1) return;                                                // (per wave: whole waves without a position skip the loop)
  const int lim = span - K;
  double acc[NI];
  const double* xp[NI];
  const float* tq[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int pos = i0 + tid + i * DM_TPB;
    const long long nn = q0 + (pos < i1 ? pos : i0);                        // a lane past i1 converts the group's first position and drops it
    xp[i] = xs + pp_window(nn, L, M, b0, lim);
    tq[i] = tp + pp_phase(nn, L);
  }
  pp_chain<NI, 2>(tq, (long long)L, xp, K, acc);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int pos = i0 + tid + i * DM_TPB;
    if (pos < i1) yd[pos] = (double)gate((float)acc[i], pos);         // the one rounding of the perturbed sample
  }
}

// outputs t = tile0 .. tile0 + DS_TILE - 1 of term (utt, start) perturbed by converter `conv` and then convolved with the first `taps` samples of
// impulse response r:
//   z[t] = float32(sum_{j < taps} double(h[j]) * double(y[start + t - j])),   y = the perturbed utterance, ZERO outside [0, P),
// left in x8 as reverb_tile leaves its outputs.  Workgroup-uniform arguments; every thread of the workgroup passes every barrier.  Per tap chunk
// the span of y that the chunk's kc taps reach - positions DR_CHUNK - kc .. DR_CHUNK + min(n - tile0, DS_TILE) - 2 of ys, not all 3071 - is
// converted in passes of at most W positions, W the most whose input span fits xs (W >= DS_TILE by the entry's check, so at most two passes),
// then reverb_tile's FIR loop runs over ys; the float64 accumulators stay in registers across chunks and passes.
// The tables are not trusted.  conv is clamped to [0, NC - 1], r and taps as in reverb_tile (every tap read inside the bank), the utterance by
// DmUtt (every staged element clamped into its buffer), start into [0, P]; ys is written and read at indices in [DR_CHUNK - kc, DS_TILE +
// DR_CHUNK - 1) only, xs below `span` <= DS_SPAN only.
// Under a gate y is the gated perturbed utterance: a chunk that reaches only closed samples is skipped as in reverb_tile, and of the others only the
// positions inside the turn are converted - the rest are the +0 the gate would select.
template <class G = NoGate>
__device__ __forceinline__ void speed_reverb_tile(const DmCorpus& c, const ConvSet& cv, const DrBank& bk, int conv, int r, int taps, int utt,
                                                  int start, int tile0, int n, SrLds& lds, float x8[8], const G& gate = G{}) {
  const int tid = threadIdx.x;
  const DmUtt ut(c, utt);
  const int ck = conv >= cv.NC ? cv.NC - 1 : conv;                           // conv >= 0 and NC >= 1 here
  const float* __restrict__ tp = cv.taps[ck];
  const int L = cv.L[ck], M = cv.M[ck], Kc = cv.K[ck], Hh = (Kc - 2) / 2;
  const long long P = ut.T > 0 ? pp_out_len(ut.T, L, M) : 0;
  const long long st = clampll(start, 0, P);
  const DrResp rs(bk, r, taps);                                              // r >= 0 here
  const int K = rs.K;
  const float* __restrict__ hp = rs.hp;
  const int left = n - tile0;                                                // > 0: the caller returned for tiles past n
  const int top = (DR_CHUNK - 1) + (left < DS_TILE ? left : DS_TILE);        // positions from here on reach no output below n
  const long long Wl = ((long long)(DS_SPAN - Kc - 1) * L) / M + 1;          // ((W - 1) M) / L + K + 1 <= DS_SPAN
  const int W = Wl > DS_SPAN ? DS_SPAN : (Wl < 1 ? 1 : (int)Wl);
  double acc[DM_PER];
#pragma unroll
  for (int i = 0; i < DM_PER; ++i) acc[i] = 0.0;
  double* __restrict__ hs = lds.a.hs;
  double* __restrict__ ys = lds.ys;
  const double* yp = lds.ys + tid + (DR_CHUNK - 1);
  for (int k0 = 0; k0 < K; k0 += DR_CHUNK) {
    const long long g0 = st + tile0 - k0 - (DR_CHUNK - 1);                  // the index of ys[0] in the perturbed utterance
    // as in reverb_tile: a chunk whose whole span lies before perturbed sample 0 adds fma(h, 0, acc) = acc, and so do all after it
    if (g0 + (DS_TILE + DR_CHUNK - 2) < 0) break;
    const int kc = K - k0 < DR_CHUNK ? K - k0 : DR_CHUNK;
    const int lo = DR_CHUNK - kc;                                            // the FIR loop reads ys[lo ..] only
    int ca = g0 + lo < 0 ? (int)(-g0) : lo;                                  // positions [ca, cb) are converted, the rest of [lo, 3071) is zero:
    const long long pe = P - g0;                                             // before sample 0, from sample P on, or of no use below n
    int cb = pe < top ? (pe < 0 ? 0 : (int)pe) : top;
    const long long tq = g0 - st;                                            // the term time of ys[0]
    const G cg = gate.at(tq);
    if constexpr (G::kOn) {
      const long long ta = (long long)tile0 - k0, tb = ta + (left < DS_TILE ? left : DS_TILE);
      if (tb <= gate.on) break;
      if (gate.silent(ta, tb, kc)) continue;
      ca = (int)clampll(gate.on - tq, ca, DS_SPAN);                          // positions before `on` and from `off` on are closed
      cb = (int)clampll(gate.off - tq, 0, cb);
    }
    __syncthreads();                                                         // the last readers of ys / hs (or of the float tile) are done
    for (int i = lo + tid; i < DS_TILE + DR_CHUNK - 1; i += DM_TPB) {
      if (i < ca || i >= cb) ys[i] = 0.0;
    }
    for (int i = tid; i < kc; i += DM_TPB) hs[i] = (double)hp[k0 + i];
    for (int a = ca; a < cb; a += W) {
      const int e = cb - a > W ? a + W : cb;
      const long long b0 = pp_base(g0 + a, L, M);                             // g0 + a >= 0
      const long long sp = pp_base(g0 + e - 1, L, M) - b0 + Kc;              // <= ((W - 1) M) / L + 1 + K <= DS_SPAN
      const int span = sp > DS_SPAN ? DS_SPAN : (int)sp;
      if (a != ca) __syncthreads();                                          // the pass before has read xs
      ut.stage(c, b0 - Hh, span, lds.a.xs);
      __syncthreads();
      for (int i0 = a; i0 < e; i0 += DS_TILE) {
        if (e - i0 > DS_TILE / 2) {
          convert_group<DM_PER>(lds.a.xs, span, b0, tp, L, M, Kc, g0, i0, e - i0 > DS_TILE ? i0 + DS_TILE : e, ys, cg);
        } else {
          convert_group<DM_PER / 2>(lds.a.xs, span, b0, tp, L, M, Kc, g0, i0, e, ys, cg);
        }
      }
    }
    __syncthreads();
    if (tid < left) {                                                        // reverb_tile's loop, written again: as one function both kernels grow
#pragma unroll 4
      for (int j = 0; j < kc; ++j) {
        const double hj = hs[j];
#pragma unroll
        for (int i = 0; i < DM_PER; ++i) acc[i] = fma(hj, yp[i * DM_TPB - j], acc[i]);
      }
    }
  }
  __syncthreads();                                                           // hs has been read: it becomes the float tile
  tile_out8(acc, reinterpret_cast<float*>(hs), x8);
}

// a term may carry a converter (conv >= 0), a response (rir >= 0), both or neither.  One of the two alone takes the code of the form that has
// only that one (convert_tile, reverb_tile) in the first 32 768 bytes of the LDS, neither takes term_value: each with that form's bits.
// The body the two forms below share.  Under a gate, a tile none of whose outputs below n reaches an open sample - it lies past off + K - 1 or ends at or
// before on - is eight +0 per thread without a load, a conversion or a chunk; the turn and K are workgroup-uniform, so every thread of the
// workgroup leaves here or none does, and scale8 of the zeros keeps the bits the long way round gives.
template <class G>
__device__ __forceinline__ void speed_reverb_value8(const DmCorpus& c, const ConvSet& cv, const DrBank& bk, int utt, int start, float norm, float gain,
                                                    int conv, int rir, int taps, const G& gate, int tile0, int t0, int n, float v[8]) {
  const bool perturbed = conv >= 0 && cv.NC >= 1;
  if constexpr (G::kOn) {
    const int K = rir < 0 ? 1 : DrResp(bk, rir, taps).K;
    const int end = n - tile0 < DS_TILE ? n : tile0 + DS_TILE;
    if (__builtin_amdgcn_readfirstlane(gate.silent(tile0, end, K))) {
      const float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      scale8(x, norm, gain, v);
      return;
    }
  }
  if (!perturbed && rir < 0) {
    term_value(c, utt, start, norm, gain, t0 < n ? t0 : 0, v, gate.at(tile0), t0 - tile0);
    return;
  }
  __shared__ SrLds lds;
  float x[8];
  if (!perturbed) {
    reverb_tile(c, bk, rir, taps, utt, start, tile0, n, lds.a, x, gate);
  } else if (rir < 0) {
    const int k = conv >= cv.NC ? cv.NC - 1 : conv;
    float* ys = reinterpret_cast<float*>(lds.a.hs);
    convert_tile(c, utt, start, cv.taps[k], cv.L[k], cv.M[k], cv.K[k], tile0, n, lds.a.xs, ys, gate.at(tile0));
    const float4 lo = *reinterpret_cast<const float4*>(ys + threadIdx.x * DM_PER);
    const float4 hi = *reinterpret_cast<const float4*>(ys + threadIdx.x * DM_PER + 4);
    x[0] = lo.x, x[1] = lo.y, x[2] = lo.z, x[3] = lo.w, x[4] = hi.x, x[5] = hi.y, x[6] = hi.z, x[7] = hi.w;
  } else {
    speed_reverb_tile(c, cv, bk, conv, rir, taps, utt, start, tile0, n, lds, x, gate);
  }
  scale8(x, norm, gain, v);
}

struct SpeedReverbForm {
  static constexpr bool kTiled = true;
  DmCorpus c;
  ConvSet cv;
  DrBank bk;
  struct Cols {
    int conv, rir, taps;
  };
  __device__ __forceinline__ static Cols cols(const int* __restrict__ term_conv, const int* __restrict__ term_rir,
                                              const int* __restrict__ term_taps, int j) {
    return {__builtin_amdgcn_readfirstlane(term_conv[j]), __builtin_amdgcn_readfirstlane(term_rir[j]),
            __builtin_amdgcn_readfirstlane(term_taps[j])};
  }
  __device__ __forceinline__ static bool same(Cols a, Cols b) { return a.conv == b.conv && a.rir == b.rir && a.taps == b.taps; }
  __device__ __forceinline__ void value8(int utt, int start, float norm, float gain, Cols t, int tile0, int t0, int n, float v[8]) const {
    speed_reverb_value8(c, cv, bk, utt, start, norm, gain, t.conv, t.rir, t.taps, NoGate{}, tile0, t0, n, v);
  }
};

// ---- turn-taking: SpeedReverbForm's term with a turn [on, off), the talker gated before the room --------------------------
// The LDS, the geometry and the code of SpeedReverbForm; the gate rides through the four staging paths.  A bank of R = 0 responses makes every rir none.
constexpr int DT_MAX_RAMP = 4096;
constexpr int DT_FAR = 1 << 30;                         // on and off are clamped to [-DT_FAR, DT_FAR]: (-DT_FAR, DT_FAR) is the open turn

struct TurnsForm {
  static constexpr bool kTiled = true;
  DmCorpus c;
  ConvSet cv;
  DrBank bk;
  const float* ramp;
  int RL;
  struct Cols {
    int conv, rir, taps, on, off;
  };
  __device__ __forceinline__ static int turn_clamp(int v) { return v < -DT_FAR ? -DT_FAR : (v > DT_FAR ? DT_FAR : v); }
  __device__ __forceinline__ static Cols cols(const int* __restrict__ term_conv, const int* __restrict__ term_rir, const int* __restrict__ term_taps,
                                              const int* __restrict__ term_on, const int* __restrict__ term_off, int j) {
    return {__builtin_amdgcn_readfirstlane(term_conv[j]), __builtin_amdgcn_readfirstlane(term_rir[j]),
            __builtin_amdgcn_readfirstlane(term_taps[j]), turn_clamp(__builtin_amdgcn_readfirstlane(term_on[j])),
            turn_clamp(__builtin_amdgcn_readfirstlane(term_off[j]))};
  }
  __device__ __forceinline__ static bool same(Cols a, Cols b) {
    return a.conv == b.conv && a.rir == b.rir && a.taps == b.taps && a.on == b.on && a.off == b.off;
  }
  __device__ __forceinline__ void value8(int utt, int start, float norm, float gain, Cols t, int tile0, int t0, int n, float v[8]) const {
    const TurnGate gate = {t.on, t.off, RL, ramp};
    speed_reverb_value8(c, cv, bk, utt, start, norm, gain, t.conv, bk.R >= 1 ? t.rir : -1, t.taps, gate, tile0, t0, n, v);
  }
};

template <class F>
__device__ __forceinline__ int uniform(int v) {
  return F::kTiled ? __builtin_amdgcn_readfirstlane(v) : v;
}

// The mixing skeleton of every form: one workgroup per DS_TILE samples of one example, one thread per eight.
template <int S, class F, class... Col>
__global__ __launch_bounds__(DM_TPB) void dynmix_kernel(F form, const int* __restrict__ term_utt, const int* __restrict__ term_start,
                                                        const float* __restrict__ term_norm, const float* __restrict__ term_gain,
                                                        const Col* __restrict__... col, const int* __restrict__ nlen, int M, int Tmax,
                                                        float* __restrict__ mix, DmRows src) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int tile0 = blockIdx.x * DS_TILE;
  const int t0 = (blockIdx.x * DM_TPB + threadIdx.x) * DM_PER;
  if (!F::kTiled && t0 >= Tmax) return;
  const bool live = !F::kTiled || t0 < Tmax;                       // a tiled form keeps its threads for the barriers and masks their stores
  const bool second = t0 + 4 < Tmax;                               // Tmax is a multiple of 4, not of 8
  int n = uniform<F>(nlen[b]);
  n = n < 0 ? 0 : (n > Tmax ? Tmax : n);
  const long long row = (long long)b * Tmax + t0;
  float acc[8], keep[S][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if ((F::kTiled ? tile0 : t0) >= n) {                             // the zero fill of pad_sequence; tiled: the whole tile, workgroup-uniform
    if (live) {
      store8(mix + row, acc, t0, n, second);
#pragma unroll
      for (int s = 0; s < S; ++s) store8(src.p[s] + row, acc, t0, n, second);
    }
    return;
  }
  const int NT = M + S, j0 = b * NT;
#pragma unroll
  for (int m = 0; m < S + 1; ++m) {
    if (m < M) {
      float v[8];
      form.value8(uniform<F>(term_utt[j0 + m]), uniform<F>(term_start[j0 + m]), term_norm[j0 + m], term_gain[j0 + m],
                  F::cols(col..., j0 + m), tile0, t0, n, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = acc[i] + v[i];         // ((0 + t0) + t1) + ...: Python's sum(), then `+ noise`
      if (m < S) {
#pragma unroll
        for (int i = 0; i < 8; ++i) keep[m][i] = v[i];
      }
    }
  }
  if (live) store8(mix + row, acc, t0, n, second);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int jm = j0 + s, jt = j0 + M + s;
    const bool same = term_utt[jt] == term_utt[jm] && term_start[jt] == term_start[jm] &&
                      __float_as_uint(term_norm[jt]) == __float_as_uint(term_norm[jm]) &&
                      __float_as_uint(term_gain[jt]) == __float_as_uint(term_gain[jm]) && F::same(F::cols(col..., jt), F::cols(col..., jm));
    if (uniform<F>(same)) {                                        // every field of the form: the target IS the mixture term - computed once
      if (live) store8(src.p[s] + row, keep[s], t0, n, second);
    } else {
      float v[8];
      form.value8(uniform<F>(term_utt[jt]), uniform<F>(term_start[jt]), term_norm[jt], term_gain[jt], F::cols(col..., jt), tile0, t0, n,
                  v);
      if (live) store8(src.p[s] + row, v, t0, n, second);
    }
  }
}

// partial sum of squares of utterance u = blockIdx.x over the chunks p, p + EN_PARTS, ... (p = blockIdx.y) of EN_TPB samples
__global__ __launch_bounds__(EN_TPB) void energy_part_kernel(DmCorpus c, long long* __restrict__ part) {
#pragma clang fp contract(off)
  const int u = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const bool is16 = u < c.N16;
  const long long total = is16 ? c.total16 : c.total32;
  const long long o0 = clampll(c.off[u] - (is16 ? 0 : c.off[c.N16]), 0, total);
  const long long len = clampll(c.off[u + 1] - c.off[u], 0, total - o0);
  __shared__ long long red[EN_TPB / 64];
  long long ai = 0;
  double ad = 0.0;
  for (long long i = (long long)p * EN_TPB + tid; i < len; i += (long long)EN_PARTS * EN_TPB) {
    if (is16) {
      const long long s = c.buf16[o0 + i];
      ai += s * s;
    } else {
      const double s = (double)c.buf32[o0 + i];
      ad += s * s;                                                 // the product of two float32 is exact in float64
    }
  }
  if (is16) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ai += __shfl_xor(ai, o, 64);
  } else {
    ai = __double_as_longlong(wave_sum_d(ad));
  }
  if ((tid & 63) == 0) red[tid >> 6] = ai;
  __syncthreads();
  if (tid == 0) {
    long long r;
    if (is16) {
      r = ((red[0] + red[1]) + red[2]) + red[3];
    } else {
      r = __double_as_longlong(((__longlong_as_double(red[0]) + __longlong_as_double(red[1])) + __longlong_as_double(red[2])) +
                               __longlong_as_double(red[3]));
    }
    part[(long long)u * EN_PARTS + p] = r;
  }
}

__global__ __launch_bounds__(256) void energy_finish_kernel(const long long* __restrict__ part, int N16, int N, long long* __restrict__ ss16,
                                                            double* __restrict__ ss32) {
#pragma clang fp contract(off)
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= N) return;
  const long long* q = part + (long long)u * EN_PARTS;
  if (u < N16) {
    long long r = 0;
#pragma unroll
    for (int p = 0; p < EN_PARTS; ++p) r += q[p];
    ss16[u] = r;
  } else {
    double r = 0.0;
#pragma unroll
    for (int p = 0; p < EN_PARTS; ++p) r += __longlong_as_double(q[p]);
    ss32[u - N16] = r;
  }
}

// the argument checks the two entries share; 0 = fine
int corpus_args_bad(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N) {
  if (!offsets || N < 1 || N16 < 0 || N16 > N) return 1;
  if (N16 > 0 && (!buf16 || total16 < 1)) return 1;
  if (N > N16 && (!buf32 || total32 < 1)) return 1;
  if (total16 < 0 || total32 < 0) return 1;
  if ((reinterpret_cast<uintptr_t>(buf16) | reinterpret_cast<uintptr_t>(buf32)) % 16 != 0) return 1;      // aligned 16-byte loads
  return 0;
}
}  // namespace
}  // namespace sepr

extern "C" size_t sepr_corpus_energy_workspace(int N) {
  using namespace sepr;
  if (N < 1) return 0;
  return align_up((size_t)N * EN_PARTS * sizeof(long long));
}

extern "C" int sepr_corpus_energy(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                                  int N16, int N, long long* ss16, double* ss32, void* ws, size_t ws_bytes, sepr_stream_t stream) {
  using namespace sepr;
  if (corpus_args_bad(buf16, total16, buf32, total32, offsets, N16, N)) return SEPR_EINVAL;
  if ((N16 > 0 && !ss16) || (N > N16 && !ss32)) return SEPR_EINVAL;
  if (!ws || ws_bytes < sepr_corpus_energy_workspace(N)) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DmCorpus c = {buf16, buf32, offsets, total16, total32, N16, N};
  long long* part = static_cast<long long*>(ws);
  hipLaunchKernelGGL(energy_part_kernel, dim3((unsigned)N, EN_PARTS), dim3(EN_TPB), 0, st, c, part);
  hipLaunchKernelGGL(energy_finish_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, part, N16, N, ss16, ss32);
  SEPR_CHECK_LAUNCH("corpus energy kernels");
  return SEPR_OK;
}

namespace sepr {
namespace {
// what the five mixing entries share: the checks of the common arguments, the corpus and the target rows as kernel arguments, the grid,
// the dispatch on S and the launch check.  An entry checks its own arguments BEFORE it calls this and passes them in `form` and `col`;
// every refusal is SEPR_EINVAL, so which check comes first does not show.
template <class F, class... Col>
int dynmix_launch(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N,
                  const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain, const int* n, int B, int M, int S,
                  int Tmax, float* mix, float* const* src, sepr_stream_t stream, F form, const char* what, const Col*... col) {
  if (corpus_args_bad(buf16, total16, buf32, total32, offsets, N16, N)) return SEPR_EINVAL;
  if (!term_utt || !term_start || !term_norm || !term_gain || !n || !mix || !src) return SEPR_EINVAL;
  if (B < 1 || B > 65535 || S < 2 || S > 3 || M < S || M > S + 1 || Tmax < 4 || Tmax % 4 != 0) return SEPR_EINVAL;
  DmRows rows = {{nullptr, nullptr, nullptr}};
  uintptr_t al = reinterpret_cast<uintptr_t>(mix);
  for (int s = 0; s < S; ++s) {
    if (!src[s]) return SEPR_EINVAL;
    rows.p[s] = src[s];
    al |= reinterpret_cast<uintptr_t>(src[s]);
  }
  if (al % 16 != 0) return SEPR_EINVAL;                            // float4 stores
  hipStream_t st = static_cast<hipStream_t>(stream);
  form.c = {buf16, buf32, offsets, total16, total32, N16, N};
  const dim3 grid((unsigned)cdiv(Tmax, DS_TILE), (unsigned)B);
  // `head`: the kernel's leading arguments, its corpus and banks; `col`: term_conv (speed), term_rir and term_taps (reverb), all three (speed-reverb), those and term_on, term_off (turns), none (plain)
  auto go = [&](auto kernel, const auto&... head) {
    hipLaunchKernelGGL(kernel, grid, dim3(DM_TPB), 0, st, head..., term_utt, term_start, term_norm, term_gain, col..., n, M, Tmax, mix, rows);
  };
  if constexpr (__is_same(F, SpeedForm))             // a kernel of its own (see dynmix_speed_kernel) with the argument list it always had
    S == 2 ? go(dynmix_speed_kernel<2>, form.c, form.cv) : go(dynmix_speed_kernel<3>, form.c, form.cv);
  else
    S == 2 ? go(dynmix_kernel<2, F, Col...>, form) : go(dynmix_kernel<3, F, Col...>, form);
  SEPR_CHECK_LAUNCH(what);
  return SEPR_OK;
}

// the converter policy of the speed entries: none is fine, the tile's input span fits the kernel's LDS plan, the entries from NC on stay zero
constexpr ConvPolicy DS_POLICY = {DS_TILE, 0, DS_SPAN, 0, false, false};

// the bank arguments of the reverberant entries, checked and copied into bk; 0 = fine
int bank_bad(const float* rir, long long rir_total, const long long* rir_off, int R, DrBank& bk) {
  if (!rir || !rir_off || R < 1 || rir_total < 1) return 1;
  if (reinterpret_cast<uintptr_t>(rir) % 4 != 0) return 1;
  bk = {rir, rir_off, rir_total, R};
  return 0;
}
}  // namespace
}  // namespace sepr

extern "C" int sepr_dynmix_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                               int N16, int N, const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain,
                               const int* n, int B, int M, int S, int Tmax, float* mix, float* const* src, sepr_stream_t stream) {
  using namespace sepr;
  return dynmix_launch(buf16, total16, buf32, total32, offsets, N16, N, term_utt, term_start, term_norm, term_gain, n, B, M, S, Tmax, mix, src,
                       stream, PlainForm{}, "dynmix kernel");
}

extern "C" int sepr_dynmix_speed_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                                     int N16, int N, const int* term_utt, const int* term_start, const float* term_norm,
                                     const float* term_gain, const int* term_conv, const int* n, int B, int M, int S, int Tmax, float* mix,
                                     float* const* src, const float* const* conv_taps, const int* conv_L, const int* conv_M, const int* conv_K,
                                     int NC, sepr_stream_t stream) {
  using namespace sepr;
  SpeedForm form = {};
  if (!term_conv || !pp_fill(conv_taps, conv_L, conv_M, conv_K, NC, DS_POLICY, form.cv)) return SEPR_EINVAL;
  return dynmix_launch(buf16, total16, buf32, total32, offsets, N16, N, term_utt, term_start, term_norm, term_gain, n, B, M, S, Tmax, mix, src,
                       stream, form, "dynmix speed kernel", term_conv);
}

extern "C" int sepr_dynmix_reverb_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                                      int N16, int N, const int* term_utt, const int* term_start, const float* term_norm,
                                      const float* term_gain, const int* term_rir, const int* term_taps, const int* n, int B, int M, int S,
                                      int Tmax, float* mix, float* const* src, const float* rir, long long rir_total, const long long* rir_off,
                                      int R, sepr_stream_t stream) {
  using namespace sepr;
  ReverbForm form = {};
  if (!term_rir || !term_taps || bank_bad(rir, rir_total, rir_off, R, form.bk)) return SEPR_EINVAL;
  return dynmix_launch(buf16, total16, buf32, total32, offsets, N16, N, term_utt, term_start, term_norm, term_gain, n, B, M, S, Tmax, mix, src,
                       stream, form, "dynmix reverb kernel", term_rir, term_taps);
}

extern "C" int sepr_dynmix_speed_reverb_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                                            int N16, int N, const int* term_utt, const int* term_start, const float* term_norm,
                                            const float* term_gain, const int* term_conv, const int* term_rir, const int* term_taps, const int* n,
                                            int B, int M, int S, int Tmax, float* mix, float* const* src, const float* const* conv_taps,
                                            const int* conv_L, const int* conv_M, const int* conv_K, int NC, const float* rir, long long rir_total,
                                            const long long* rir_off, int R, sepr_stream_t stream) {
  using namespace sepr;
  SpeedReverbForm form = {};
  if (!term_conv || !pp_fill(conv_taps, conv_L, conv_M, conv_K, NC, DS_POLICY, form.cv)) return SEPR_EINVAL;
  if (!term_rir || !term_taps || bank_bad(rir, rir_total, rir_off, R, form.bk)) return SEPR_EINVAL;
  return dynmix_launch(buf16, total16, buf32, total32, offsets, N16, N, term_utt, term_start, term_norm, term_gain, n, B, M, S, Tmax, mix, src,
                       stream, form, "dynmix speed-reverb kernel", term_conv, term_rir, term_taps);
}

extern "C" int sepr_dynmix_turns_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16,
                                     int N, const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain,
                                     const int* term_conv, const int* term_rir, const int* term_taps, const int* term_on, const int* term_off,
                                     const int* n, int B, int M, int S, int Tmax, float* mix, float* const* src, const float* const* conv_taps,
                                     const int* conv_L, const int* conv_M, const int* conv_K, int NC, const float* rir, long long rir_total,
                                     const long long* rir_off, int R, const float* ramp, int RL, sepr_stream_t stream) {
  using namespace sepr;
  TurnsForm form = {};
  if (!term_conv || !pp_fill(conv_taps, conv_L, conv_M, conv_K, NC, DS_POLICY, form.cv)) return SEPR_EINVAL;
  if (!term_rir || !term_taps || R < 0 || (R > 0 && bank_bad(rir, rir_total, rir_off, R, form.bk))) return SEPR_EINVAL;      // R = 0: no bank
  if (!term_on || !term_off || RL < 0 || RL > DT_MAX_RAMP || (RL > 0 && !ramp) || reinterpret_cast<uintptr_t>(ramp) % 4 != 0) return SEPR_EINVAL;
  form.ramp = ramp;
  form.RL = RL;
  return dynmix_launch(buf16, total16, buf32, total32, offsets, N16, N, term_utt, term_start, term_norm, term_gain, n, B, M, S, Tmax, mix, src,
                       stream, form, "dynmix turns kernel", term_conv, term_rir, term_taps, term_on, term_off);
}
