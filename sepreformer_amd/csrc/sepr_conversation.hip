// Conversations rendered and scored on the device (contracts in include/sepr.h).
//
//   render_kernel        (sepr_conversation_render) mixture and per-talker tracks of R conversations of any length from the resident corpus of
//                        the mixing launch.  A conversation is a schedule of segments - utterance, first sample used, output sample where it
//                        lands, length, the two factors - sorted by (track, place).  One thread per four flat output samples (one float4 store per
//                        row); a workgroup makes 1024.  The conversation of the tile's first sample and, per track, its first live segment are found
//                        by binary search on addresses that depend on the workgroup alone (scalar loads); a thread walks forward from there, and
//                        only a thread that lies in a later conversation than its tile's first sample searches for itself.  A segment that covers
//                        the thread's four samples is read with two aligned 16-byte (float32) or 8-byte (int16) loads and realigned in registers;
//                        a segment's first and last samples, where it covers part of the four, one clamped element at a time.
//                        The arithmetic is sepr_dynmix_fwd's: (x * norm) * gain, two roundings, the tracks summed in track order from +0.
//   render_rooms_kernel  (sepr_conversation_render_rooms, section 5h-2) the same with an impulse response per segment: the float64 FIR of the mixing
//                        launch per contributing segment, 2048 outputs per workgroup, taps in chunks of 1024 through 38 912 bytes of LDS; tails run
//                        on under later segments; silent stretches stage nothing.  Its comment stands at the kernel.
//   segsnr_ref_kernel / segsnr_value_kernel   (sepr_segment_sisnr_fwd) the segment-wise SI-SNR of every output channel and of the mixture against
//                        every utterance, in float64.  One workgroup per segment takes the reference's mean and centred energy into the workspace;
//                        one workgroup per (signal, segment) then makes three passes over the segment - the signal's mean, the centred cross term,
//                        and, alpha known, the residual summed directly.  A thread adds the samples tid, tid + 256, ... in order, a wave adds its
//                        lanes by butterfly, and the four wave sums are added in wave order: a fixed order, no atomics.
// Nothing here depends on the launch order of workgroups: results are bit-identical from run to run.  Neither entry trusts its device tables: every
// index read from one is clamped, so a bad table gives wrong values but no access outside the buffers.
#include "sepr_common.h"

namespace sepr {
namespace {
constexpr int CV_TPB = 256;              // threads per workgroup of the render kernel
constexpr int CV_PER = 4;                // output samples per thread: one float4
constexpr int CV_TILE = CV_TPB * CV_PER;
constexpr int CV_MAX_TRACKS = 8;
constexpr int SN_TPB = 256;              // threads per workgroup of the metric kernels
constexpr int SN_MAX_CH = 8;

__device__ __forceinline__ long long cv_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct CvCorpus {
  const short* buf16;
  const float* buf32;
  const long long* off;
  long long total16, total32;
  int N16, N;
};

struct CvTable {
  const int* utt;
  const int* start;
  const int* place;
  const int* len;
  const float* norm;
  const float* gain;
  const int* track_off;                  // [R * S + 1] cumulative segment counts per (conversation, track)
  const long long* out_off;              // [R + 1]
  int R, S, G;
};

// one utterance's slice of the corpus buffers under a clamped index and start: element e0 of its buffer is the segment's first sample
struct CvUtt {
  long long e0, total;
  bool is16;
  __device__ __forceinline__ CvUtt(const CvCorpus& c, int utt, int start) {
    const int u = utt < 0 ? 0 : (utt >= c.N ? c.N - 1 : utt);
    const long long o0 = c.off[u], len = c.off[u + 1] - o0;
    is16 = u < c.N16;
    total = is16 ? c.total16 : c.total32;
    e0 = o0 - (is16 ? 0 : c.off[c.N16]) + cv_clamp(start, 0, len > 0 ? len : 0);
  }
  // the sample d of the segment, its element position clamped into the buffer
  __device__ __forceinline__ float one(const CvCorpus& c, long long d) const {
    const long long e = cv_clamp(e0 + d, 0, total - 1);
    return is16 ? (float)c.buf16[e] * 3.0517578125e-05f : c.buf32[e];
  }
  // the samples d .. d + 3 of the segment: aligned loads at the aligned-down element, realigned in registers.  The first element is clamped into
  // the buffer and the second load is made only below the buffer's allocated end (its element count rounded up to 16 bytes): no load leaves it.
  __device__ __forceinline__ void four(const CvCorpus& c, long long d, float x[4]) const {
    const long long e = cv_clamp(e0 + d, 0, total - 1), a0 = e & ~3LL;
    const int sh = (int)(e & 3);
    if (is16) {
      const long long pad = (total + 7) & ~7LL;
      const uint2 lo = *reinterpret_cast<const uint2*>(c.buf16 + a0);
      const uint2 hi = a0 + 4 < pad ? *reinterpret_cast<const uint2*>(c.buf16 + a0 + 4) : make_uint2(0u, 0u);
      const unsigned w[4] = {lo.x, lo.y, hi.x, hi.y};
      const int ds = sh >> 1;
      const unsigned u0 = ds ? w[1] : w[0], u1 = ds ? w[2] : w[1], u2 = ds ? w[3] : w[2];
      const bool odd = sh & 1;
      const unsigned d0 = odd ? __builtin_amdgcn_alignbyte(u1, u0, 2) : u0, d1 = odd ? __builtin_amdgcn_alignbyte(u2, u1, 2) : u1;
      x[0] = (float)(short)(d0 & 0xffffu) * 3.0517578125e-05f;
      x[1] = (float)((int)d0 >> 16) * 3.0517578125e-05f;
      x[2] = (float)(short)(d1 & 0xffffu) * 3.0517578125e-05f;
      x[3] = (float)((int)d1 >> 16) * 3.0517578125e-05f;
    } else {
      const long long pad = (total + 3) & ~3LL;
      const float4 q0 = ld4(c.buf32 + a0);
      const float4 q1 = a0 + 4 < pad ? ld4(c.buf32 + a0 + 4) : zero4();
      const float w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = sh == 0 ? w[k] : (sh == 1 ? w[k + 1] : (sh == 2 ? w[k + 2] : w[k + 3]));
    }
  }
};

// the conversation of flat output sample f: the last r in [0, R) with out_off[r] <= f (0 when there is none)
__device__ __forceinline__ int cv_conversation(const long long* __restrict__ out_off, int R, long long f) {
  int lo = 0, hi = R;                                              // the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (out_off[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// the first segment of (conversation, track) j - the segments [lo, hi) of the table, both clamped into [0, G] - that is live at or after sample t: the
// first with place + len > t, or hi.  The segments of a track are sorted by place and do not overlap, so their ends are sorted too: that is the
// last segment with place <= t if it reaches past t, else the one after it.
__device__ __forceinline__ int cv_first_live(const CvTable& tb, int j, long long t, int& hi) {
  const int* __restrict__ place = tb.place;
  const int* __restrict__ len = tb.len;
  int lo = tb.track_off[j];
  hi = tb.track_off[j + 1];
  lo = lo < 0 ? 0 : (lo > tb.G ? tb.G : lo);
  hi = hi < lo ? lo : (hi > tb.G ? tb.G : hi);
  int a = lo, b = hi;                                              // place[g] <= t for g in [lo, a), place[g] > t for g in [b, hi)
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (place[mid] <= t) a = mid + 1; else b = mid;
  }
  if (a > lo && (long long)place[a - 1] + len[a - 1] > t) return a - 1;
  return a;
}

__global__ __launch_bounds__(CV_TPB) void render_kernel(CvCorpus c, CvTable tb, long long total, float* __restrict__ mix, float* __restrict__ tracks) {
#pragma clang fp contract(off)
  const long long tile0 = (long long)blockIdx.x * CV_TILE;
  const long long f0 = tile0 + (long long)threadIdx.x * CV_PER;      // total is a multiple of 4: a thread's four samples are all below it or none is
  if (f0 >= total) return;
  const int rt = cv_conversation(tb.out_off, tb.R, tile0);          // of the tile's first sample: workgroup-uniform
  const bool mine = f0 >= tb.out_off[rt + 1] && rt + 1 < tb.R;      // this thread lies in a later conversation (offsets are multiples of 4)
  const int r = mine ? cv_conversation(tb.out_off, tb.R, f0) : rt;
  const long long t0 = f0 - tb.out_off[r], tt = tile0 - tb.out_off[rt];
  float acc[CV_PER] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < tb.S; ++s) {
    int g, hi;
    if (!mine) {
      g = cv_first_live(tb, rt * tb.S + s, tt, hi);                // workgroup-uniform; the thread walks on from it below
    } else {
      g = cv_first_live(tb, r * tb.S + s, t0, hi);
    }
    float v[CV_PER] = {0.f, 0.f, 0.f, 0.f};                        // +0.0 where no segment of the track covers the sample
    for (; g < hi; ++g) {
      const long long p = tb.place[g], q = p + tb.len[g];          // the segment covers [p, q)
      if (q <= t0) continue;
      if (p >= t0 + CV_PER) break;
      const CvUtt ut(c, tb.utt[g], tb.start[g]);
      const float norm = tb.norm[g], gain = tb.gain[g];
      if (p <= t0 && q >= t0 + CV_PER) {
        float x[CV_PER];
        ut.four(c, t0 - p, x);
#pragma unroll
        for (int i = 0; i < CV_PER; ++i) {
          const float a = x[i] * norm;
          v[i] = a * gain;
        }
      } else {
#pragma unroll
        for (int i = 0; i < CV_PER; ++i) {
          if (t0 + i >= p && t0 + i < q) {
            const float a = ut.one(c, t0 + i - p) * norm;
            v[i] = a * gain;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CV_PER; ++i) acc[i] = acc[i] + v[i];       // ((0 + track 0) + track 1) + ...
    if (tracks) st4(tracks + (long long)s * total + f0, make_float4(v[0], v[1], v[2], v[3]));
  }
  st4(mix + f0, make_float4(acc[0], acc[1], acc[2], acc[3]));
}

// ---- conversations in rooms (sepr_conversation_render_rooms) -------------------------------------------------------
// A segment with a response is the FIR of sepr_dynmix_reverb_fwd over the segment's samples, zero outside the SEGMENT; its tail runs on under the
// later segments of its track until the conversation ends.  A workgroup makes a tile of CR_TILE flat output samples; where conversations meet
// inside the tile it makes the piece of each in turn, so a piece never holds samples of two.  Per piece and track it finds the segments whose
// support can reach the piece (binary search for the first at or past the piece's end, then back while place + len + 16383 lies past its start) and
// adds them in table order; a (track, piece) that none reaches is zeros with nothing staged.  Every decision that a barrier depends on is taken on
// table values and kernel arguments alone: workgroup-uniform.
// The FIR is reverb_tile's of sepr_dynmix.hip WRITTEN AGAIN, with its plan - 2048 outputs per workgroup, taps in ascending
// chunks of 1024, the chunk's span staged in LDS as doubles, the float64 sums in registers across chunks - and its sums, tap by tap.  That one
// indexes an utterance from a term's start, is zero outside the utterance and carries a gate; this one indexes a segment from its place, is zero
// outside the segment, keeps the sum after `direct` taps and runs once per contributing segment: as one function both would carry the other's
// predicates.  It differs in who owns what.  There a thread owns outputs tid + 256 i and reads one double from LDS per FMA, which bounds the loop
// by the LDS at under a fifth of the FP64 rate; here a thread owns EIGHT CONSECUTIVE outputs and walks the taps in groups of eight over a
// window of 15 staged samples kept in registers: a group is 64 FMAs for eight new samples and eight taps read, so the LDS is out of the way,
// and the outputs need no transposition at the end.  Every output still adds its taps in ascending order: the same bits.
constexpr int CR_TPB = 256;
constexpr int CR_PER = 8;                // outputs per thread
constexpr int CR_TILE = CR_TPB * CR_PER;
constexpr int CR_CHUNK = 1024;           // taps per chunk
constexpr int CR_SPAN = CR_TILE + CR_CHUNK - 1;          // segment samples a chunk's outputs reach
constexpr int CR_MAX_TAPS = 16384;
constexpr int CR_BLOCKS = (CR_SPAN + 1) / 8;             // the span is stored in blocks of 8 doubles, 10 apart: a thread reads whole blocks with 16-byte
constexpr int CR_PITCH = 10;                             // loads, and the 80-byte pitch puts the blocks of any 16 consecutive lanes on 16 different bank quads
static_assert((CR_SPAN + 1) % 8 == 0 && CR_CHUNK % 8 == 0 && CR_PER == 8, "whole blocks of eight");

struct CrLds {
  __attribute__((aligned(16))) double xs[CR_BLOCKS * CR_PITCH];      // the staged span of the segment
  __attribute__((aligned(16))) double hs[CR_CHUNK];                  // a chunk's taps
};

__device__ __forceinline__ void cr_load8(const double* __restrict__ p, double out[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double2 v = *reinterpret_cast<const double2*>(p + 2 * k);
    out[2 * k] = v.x, out[2 * k + 1] = v.y;
  }
}

// taps jb .. je - 1 of the staged chunk (0 <= jb < je <= CR_CHUNK), ascending, into the eight consecutive outputs 8 tid .. 8 tid + 7 of the thread:
// acc[i] = fma(hs[j], xs[8 tid + i + 1023 - j], acc[i]).  Group m holds the taps 8 m .. 8 m + 7; its window is w[c] = xs[8 (tid + 127 - m) + c],
// c = 0 .. 14, so output i under tap 8 m + q reads w[7 + i - q]; the next group keeps w[0 .. 6] as w[8 .. 14] and loads one block.
__device__ __forceinline__ void cr_taps(const double* __restrict__ xs, const double* __restrict__ hs, int jb, int je, double acc[CR_PER]) {
  const int tid = threadIdx.x;
  int m = jb >> 3;
  double w[16];
  cr_load8(xs + (tid + (CR_CHUNK / 8 - 1) - m) * CR_PITCH, w);
  cr_load8(xs + (tid + CR_CHUNK / 8 - m) * CR_PITCH, w + 8);
  for (; 8 * m < je; ++m) {
    double h[8];
    cr_load8(hs + 8 * m, h);
    if (8 * m >= jb && 8 * m + 8 <= je) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int i = 0; i < CR_PER; ++i) acc[i] = fma(h[q], w[7 + i - q], acc[i]);
      }
    } else {                                                                 // the group holds jb or je: the taps outside [jb, je) are left out
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (8 * m + q >= jb && 8 * m + q < je) {
#pragma unroll
          for (int i = 0; i < CR_PER; ++i) acc[i] = fma(h[q], w[7 + i - q], acc[i]);
        }
      }
    }
#pragma unroll
    for (int k = 14; k >= 8; --k) w[k] = w[k - 8];
    if (8 * (m + 1) < je) cr_load8(xs + (tid + (CR_CHUNK / 8 - 1) - (m + 1)) * CR_PITCH, w);
  }
}

struct CrRooms {
  const int* rir;
  const int* taps;
  const int* direct;
  const float* h;                        // the NR responses back to back
  const long long* off;                  // [NR + 1]
  long long total;
  int NR;
};

// sum[i] = sum[i] + (z[i] * norm) * gain where local sample t0 + i lies in [p, e): the segment's support under the taps that made z
__device__ __forceinline__ void cr_add(const float z[CR_PER], float norm, float gain, long long t0, long long p, long long e, float sum[CR_PER]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < CR_PER; ++i) {
    if (t0 + i >= p && t0 + i < e) {
      const float a = z[i] * norm;
      sum[i] = sum[i] + a * gain;
    }
  }
}

// segment g added to the running sums of its track on the piece [ta, ta + L) of its conversation (local samples; thread tid owns ta + 8 tid .. + 7).
// Workgroup-uniform arguments; every thread of the workgroup passes every barrier.
__device__ __forceinline__ void cr_segment(const CvCorpus& c, const CvTable& tb, const CrRooms& rm, int g, long long ta, int L, bool want_direct,
                                           CrLds& lds, float wet[CR_PER], float dir[CR_PER]) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const long long p = tb.place[g];
  const int ln = tb.len[g] < 0 ? 0 : tb.len[g];
  const int ri = rm.rir[g];
  const bool room = ri >= 0 && rm.NR > 0;
  int K = 1, D = 1;
  const float* __restrict__ hp = nullptr;
  if (room) {                                                                // the table is not trusted: every tap read lies inside the bank
    const int rr = ri >= rm.NR ? rm.NR - 1 : ri;
    const long long h0 = cv_clamp(rm.off[rr], 0, rm.total - 1);
    const long long hl = cv_clamp(rm.off[rr + 1] - h0, 1, rm.total - h0 < CR_MAX_TAPS ? rm.total - h0 : CR_MAX_TAPS);
    const int tp = rm.taps[g], dd = rm.direct[g];
    K = tp < 1 ? 1 : (tp > (int)hl ? (int)hl : tp);
    D = dd < 1 ? 1 : (dd > K ? K : dd);
    hp = rm.h + h0;
  }
  const long long te = ta + L, eK = p + ln + (K - 1), eD = p + ln + (D - 1);
  if (p >= te || eK <= ta) return;                                           // the support misses the piece
  const CvUtt ut(c, tb.utt[g], tb.start[g]);
  const float norm = tb.norm[g], gain = tb.gain[g];
  const long long t0 = ta + (long long)tid * CR_PER;
  if (!room) {                                                               // h = [1.0]: float32(1.0 x) is x; the dry kernel's loads
    float x[CR_PER];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long th = t0 + 4 * h;
      if (p <= th && p + ln >= th + 4) {
        ut.four(c, th - p, x + 4 * h);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[4 * h + i] = (th + i >= p && th + i < p + ln) ? ut.one(c, th + i - p) : 0.f;
      }
    }
    cr_add(x, norm, gain, t0, p, eK, wet);
    if (want_direct) cr_add(x, norm, gain, t0, p, eD, dir);
    return;
  }
  const bool split = want_direct && D < K;                                   // else the two sums are one sequence of operations
  double acc[CR_PER], accd[CR_PER];
#pragma unroll
  for (int i = 0; i < CR_PER; ++i) acc[i] = 0.0, accd[i] = 0.0;
  bool snapped = !split;
  double* __restrict__ hs = lds.hs;
  for (int k0 = 0; k0 < K; k0 += CR_CHUNK) {
    if (!snapped && D <= k0) {                                               // the sum after D taps: a prefix of the same sequence
#pragma unroll
      for (int i = 0; i < CR_PER; ++i) accd[i] = acc[i];
      snapped = true;
    }
    const int kc = K - k0 < CR_CHUNK ? K - k0 : CR_CHUNK;
    const long long d0 = ta - p - k0 - (CR_CHUNK - 1);                       // the segment sample of xs[0]: output o reads xs[o + 1023 - j] under tap k0 + j
    // a chunk whose outputs below L reach only samples before the segment's first adds fma(h, +0, acc) = acc (acc is never -0), and so does every later
    // chunk; one that reaches only samples past its last does too, but a later chunk reaches further back
    if (d0 + (CR_CHUNK - 1) + (L - 1) < 0) break;
    if (d0 + (CR_CHUNK - 1) - (kc - 1) >= ln) continue;
    __syncthreads();                                                         // the last readers of xs / hs are done
    for (int i = tid; i < CR_SPAN + 1; i += CR_TPB) {                        // (the last one completes a block; no output reads it)
      const long long d = d0 + i;
      lds.xs[i + (i >> 3) * (CR_PITCH - 8)] = (d >= 0 && d < ln) ? (double)ut.one(c, d) : 0.0;       // zero outside the SEGMENT
    }
    for (int i = tid; i < kc; i += CR_TPB) hs[i] = (double)hp[k0 + i];
    __syncthreads();
    if (tid * CR_PER < L) {                                                  // (per wave: whole waves past the piece skip the loop)
      int j = 0;
      if (!snapped && D < k0 + kc) {                                         // k0 < D here
        j = D - k0;
        cr_taps(lds.xs, hs, 0, j, acc);
#pragma unroll
        for (int i = 0; i < CR_PER; ++i) accd[i] = acc[i];
      }
      if (j < kc) cr_taps(lds.xs, hs, j, kc, acc);
    }
    if (D < k0 + kc) snapped = true;
  }
  if (!snapped) {
#pragma unroll
    for (int i = 0; i < CR_PER; ++i) accd[i] = acc[i];
  }
  float z[CR_PER];
#pragma unroll
  for (int i = 0; i < CR_PER; ++i) z[i] = (float)acc[i];
  cr_add(z, norm, gain, t0, p, eK, wet);
  if (split) {
#pragma unroll
    for (int i = 0; i < CR_PER; ++i) z[i] = (float)accd[i];
    cr_add(z, norm, gain, t0, p, eD, dir);
  } else if (want_direct) {
    cr_add(z, norm, gain, t0, p, eK, dir);
  }
}

__global__ __launch_bounds__(CR_TPB) void render_rooms_kernel(CvCorpus c, CvTable tb, CrRooms rm, long long total, float* __restrict__ mix,
                                                              float* __restrict__ tracks) {
#pragma clang fp contract(off)
  __shared__ CrLds lds;
  const int tid = threadIdx.x;
  const long long tile0 = (long long)blockIdx.x * CR_TILE;
  const long long tend = tile0 + CR_TILE < total ? tile0 + CR_TILE : total;
  for (int r = cv_conversation(tb.out_off, tb.R, tile0); r < tb.R; ++r) {    // the conversations that meet in this tile, one piece each
    const long long a = tb.out_off[r], b = tb.out_off[r + 1];
    if (a >= tend) break;
    const long long fa = (a > tile0 ? a : tile0) & ~3LL, fe = (b < tend ? b : tend) & ~3LL;        // multiples of 4 whatever the table holds
    if (fe <= fa) continue;
    const long long ta = fa - a, te = ta + (fe - fa);
    const int L = (int)(fe - fa);                                            // 4 .. CR_TILE
    const long long f0 = fa + (long long)tid * CR_PER;
    const bool lo4 = tid * CR_PER < L, hi4 = tid * CR_PER + 4 < L;           // the thread's two float4 stores lie inside the piece
    float acc[CR_PER];
#pragma unroll
    for (int i = 0; i < CR_PER; ++i) acc[i] = 0.f;
    for (int s = 0; s < tb.S; ++s) {
      const int* __restrict__ place = tb.place;
      const int* __restrict__ len = tb.len;
      int lo = tb.track_off[r * tb.S + s], hi = tb.track_off[r * tb.S + s + 1];
      lo = lo < 0 ? 0 : (lo > tb.G ? tb.G : lo);
      hi = hi < lo ? lo : (hi > tb.G ? tb.G : hi);
      int ga = lo, gb = hi;                                                  // place[g] < te for g in [lo, ga), >= te for g in [gb, hi)
      while (ga < gb) {
        const int mid = ga + ((gb - ga) >> 1);
        if (place[mid] < te) ga = mid + 1; else gb = mid;
      }
      int gf = ga;                                                           // ends are sorted on a track: the first segment that cannot reach ends the walk
      while (gf > lo && (long long)place[gf - 1] + len[gf - 1] + (CR_MAX_TAPS - 1) > ta) --gf;
      float wet[CR_PER], dir[CR_PER];
#pragma unroll
      for (int i = 0; i < CR_PER; ++i) wet[i] = 0.f, dir[i] = 0.f;
      for (int g = gf; g < ga; ++g) cr_segment(c, tb, rm, g, ta, L, tracks != nullptr, lds, wet, dir);
#pragma unroll
      for (int i = 0; i < CR_PER; ++i) acc[i] = acc[i] + wet[i];             // ((0 + wet 0) + wet 1) + ...
      if (tracks) {
        float* __restrict__ row = tracks + (long long)s * total + f0;
        if (lo4) st4(row, make_float4(dir[0], dir[1], dir[2], dir[3]));
        if (hi4) st4(row + 4, make_float4(dir[4], dir[5], dir[6], dir[7]));
      }
    }
    if (lo4) st4(mix + f0, make_float4(acc[0], acc[1], acc[2], acc[3]));
    if (hi4) st4(mix + f0 + 4, make_float4(acc[4], acc[5], acc[6], acc[7]));
  }
}

// ---- segment-wise SI-SNR ------------------------------------------------------------------------------------------------------------------
struct SnSeg {
  const float* r;                        // the reference segment's first sample
  long long b;                           // its first sample's index in a row
  int n;
};

// segment g under clamps: the row into [0, S), begin into [0, T], the length into [0, T - begin]
__device__ __forceinline__ SnSeg sn_segment(const float* __restrict__ ref, const int* __restrict__ rows, const int* __restrict__ begin,
                                            const int* __restrict__ length, int g, int S, int T, long long ld) {
  const int row = rows[g] < 0 ? 0 : (rows[g] >= S ? S - 1 : rows[g]);
  const int b = begin[g] < 0 ? 0 : (begin[g] > T ? T : begin[g]);
  const int n = length[g] < 0 ? 0 : (length[g] > T - b ? T - b : length[g]);
  return {ref + (long long)row * ld + b, b, n};
}

__global__ __launch_bounds__(SN_TPB) void segsnr_ref_kernel(const float* __restrict__ ref, const int* __restrict__ rows, const int* __restrict__ begin,
                                                            const int* __restrict__ length, int S, int T, long long ld, double* __restrict__ stat) {
#pragma clang fp contract(off)
  __shared__ double red[SN_TPB / 64];
  const int g = blockIdx.x, tid = threadIdx.x;
  const SnSeg sg = sn_segment(ref, rows, begin, length, g, S, T, ld);
  double a = 0.0;
  for (int i = tid; i < sg.n; i += SN_TPB) a += (double)sg.r[i];
  const double mean = sg.n > 0 ? block_sum_d(a, red) / (double)sg.n : 0.0;
  double e = 0.0;
  for (int i = tid; i < sg.n; i += SN_TPB) {
    const double d = (double)sg.r[i] - mean;
    e += d * d;
  }
  e = block_sum_d(e, red);
  if (tid == 0) {
    stat[2 * (long long)g] = mean;
    stat[2 * (long long)g + 1] = e;
  }
}

// signal k = blockIdx.y < C is channel k of est, k = C the mixture; against segment g = blockIdx.x
__global__ __launch_bounds__(SN_TPB) void segsnr_value_kernel(const float* __restrict__ est, const float* __restrict__ ref, const float* __restrict__ mix,
                                                              const int* __restrict__ rows, const int* __restrict__ begin,
                                                              const int* __restrict__ length, int C, int S, int T, long long ld, double eps,
                                                              const double* __restrict__ stat, double* __restrict__ v, double* __restrict__ v_mix) {
#pragma clang fp contract(off)
  __shared__ double red[SN_TPB / 64];
  const int g = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const SnSeg sg = sn_segment(ref, rows, begin, length, g, S, T, ld);
  const float* __restrict__ x = (k < C ? est + (long long)k * ld : mix) + sg.b;
  const double mr = stat[2 * (long long)g], srr = stat[2 * (long long)g + 1];
  double a = 0.0;
  for (int i = tid; i < sg.n; i += SN_TPB) a += (double)x[i];
  const double ma = sg.n > 0 ? block_sum_d(a, red) / (double)sg.n : 0.0;
  double sar = 0.0;
  for (int i = tid; i < sg.n; i += SN_TPB) sar += ((double)x[i] - ma) * ((double)sg.r[i] - mr);
  sar = block_sum_d(sar, red);
  const double alpha = sar / (srr + eps);
  double res = 0.0;
  for (int i = tid; i < sg.n; i += SN_TPB) {                       // the residual itself, not a difference of moments
    const double d = ((double)x[i] - ma) - alpha * ((double)sg.r[i] - mr);
    res += d * d;
  }
  res = block_sum_d(res, red);
  if (tid == 0) {
    const double val = 20.0 * log10(eps + fabs(alpha) * sqrt(srr) / (sqrt(res) + eps));
    if (k < C) v[(long long)g * C + k] = val; else v_mix[g] = val;
  }
}

struct SnLayout {
  double* stat;                          // [G][2]: the reference segment's mean and centred energy
  SnLayout(Arena& a, int G) { stat = a.f64(2 * (size_t)G); }
};
}  // namespace
}  // namespace sepr

extern "C" int sepr_conversation_render(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16,
                                        int N, const int* seg_utt, const int* seg_start, const int* seg_place, const int* seg_len,
                                        const float* seg_norm, const float* seg_gain, const int* track_off, const long long* out_off, int R, int S_max,
                                        int G, long long total, float* mix, float* tracks, sepr_stream_t stream) {
  using namespace sepr;
  if (!offsets || N < 1 || N16 < 0 || N16 > N || total16 < 0 || total32 < 0) return SEPR_EINVAL;
  if ((N16 > 0 && (!buf16 || total16 < 1)) || (N > N16 && (!buf32 || total32 < 1))) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(buf16) | reinterpret_cast<uintptr_t>(buf32)) % 16 != 0) return SEPR_EINVAL;       // aligned vector loads
  if (!seg_utt || !seg_start || !seg_place || !seg_len || !seg_norm || !seg_gain || !track_off || !out_off || !mix) return SEPR_EINVAL;
  if (R < 1 || R > 65535 || S_max < 1 || S_max > CV_MAX_TRACKS || G < 1) return SEPR_EINVAL;
  if (total < 4 || total % 4 != 0 || total > (1LL << 40)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(mix) | reinterpret_cast<uintptr_t>(tracks)) % 16 != 0) return SEPR_EINVAL;       // float4 stores
  if (reinterpret_cast<uintptr_t>(out_off) % 8 != 0) return SEPR_EINVAL;
  const CvCorpus c = {buf16, buf32, offsets, total16, total32, N16, N};
  const CvTable tb = {seg_utt, seg_start, seg_place, seg_len, seg_norm, seg_gain, track_off, out_off, R, S_max, G};
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)cdiv(total, CV_TILE)), dim3(CV_TPB), 0, static_cast<hipStream_t>(stream), c, tb, total, mix,
                     tracks);
  SEPR_CHECK_LAUNCH("conversation render kernel");
  return SEPR_OK;
}

extern "C" int sepr_conversation_render_rooms(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets,
                                              int N16, int N, const int* seg_utt, const int* seg_start, const int* seg_place, const int* seg_len,
                                              const float* seg_norm, const float* seg_gain, const int* seg_rir, const int* seg_taps,
                                              const int* seg_direct, const int* track_off, const long long* out_off, int R, int S_max, int G,
                                              long long total, float* mix, float* tracks, const float* rir, long long rir_total,
                                              const long long* rir_off, int NR, sepr_stream_t stream) {
  using namespace sepr;
  // what sepr_conversation_render refuses
  if (!offsets || N < 1 || N16 < 0 || N16 > N || total16 < 0 || total32 < 0) return SEPR_EINVAL;
  if ((N16 > 0 && (!buf16 || total16 < 1)) || (N > N16 && (!buf32 || total32 < 1))) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(buf16) | reinterpret_cast<uintptr_t>(buf32)) % 16 != 0) return SEPR_EINVAL;
  if (!seg_utt || !seg_start || !seg_place || !seg_len || !seg_norm || !seg_gain || !track_off || !out_off || !mix) return SEPR_EINVAL;
  if (R < 1 || R > 65535 || S_max < 1 || S_max > CV_MAX_TRACKS || G < 1) return SEPR_EINVAL;
  if (total < 4 || total % 4 != 0 || total > (1LL << 40)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(mix) | reinterpret_cast<uintptr_t>(tracks)) % 16 != 0) return SEPR_EINVAL;
  if (reinterpret_cast<uintptr_t>(out_off) % 8 != 0) return SEPR_EINVAL;
  // the three columns, and what sepr_dynmix_reverb_fwd refuses of a bank (NR = 0: no bank, every segment response-free)
  if (!seg_rir || !seg_taps || !seg_direct || NR < 0) return SEPR_EINVAL;
  if (NR > 0 && (!rir || !rir_off || rir_total < 1 || reinterpret_cast<uintptr_t>(rir) % 4 != 0 || reinterpret_cast<uintptr_t>(rir_off) % 8 != 0))
    return SEPR_EINVAL;
  const CvCorpus c = {buf16, buf32, offsets, total16, total32, N16, N};
  const CvTable tb = {seg_utt, seg_start, seg_place, seg_len, seg_norm, seg_gain, track_off, out_off, R, S_max, G};
  const CrRooms rm = {seg_rir, seg_taps, seg_direct, NR > 0 ? rir : nullptr, NR > 0 ? rir_off : nullptr, NR > 0 ? rir_total : 0, NR};
  hipLaunchKernelGGL(render_rooms_kernel, dim3((unsigned)cdiv(total, CR_TILE)), dim3(CR_TPB), 0, static_cast<hipStream_t>(stream), c, tb, rm, total,
                     mix, tracks);
  SEPR_CHECK_LAUNCH("conversation rooms kernel");
  return SEPR_OK;
}

extern "C" long long sepr_segment_sisnr_bytes(int G, int C) {
  using namespace sepr;
  if (G < 1 || C < 1 || C > SN_MAX_CH) return 0;
  return (long long)layout_bytes<SnLayout>(G);
}

extern "C" int sepr_segment_sisnr_fwd(const float* est, const float* ref, const float* mix, const int* rows, const int* begin, const int* length, int G,
                                      int C, int S, int T, long long ld, double eps, double* v, double* v_mix, void* ws, size_t ws_bytes,
                                      sepr_stream_t stream) {
  using namespace sepr;
  if (!est || !ref || !mix || !rows || !begin || !length || !v || !v_mix) return SEPR_EINVAL;
  if (G < 1 || C < 1 || C > SN_MAX_CH || S < 1 || S > CV_MAX_TRACKS || T < 1 || ld < T) return SEPR_EINVAL;
  if (!(eps >= 0.0 && eps <= 1.0)) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(est) | reinterpret_cast<uintptr_t>(ref) | reinterpret_cast<uintptr_t>(mix)) % 4 != 0) return SEPR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(v_mix)) % 8 != 0) return SEPR_EINVAL;
  Arena arena(ws, ws_bytes);
  const SnLayout lay(arena, G);
  if (!arena.ok_need()) return SEPR_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(segsnr_ref_kernel, dim3((unsigned)G), dim3(SN_TPB), 0, st, ref, rows, begin, length, S, T, ld, lay.stat);
  hipLaunchKernelGGL(segsnr_value_kernel, dim3((unsigned)G, (unsigned)(C + 1)), dim3(SN_TPB), 0, st, est, ref, mix, rows, begin, length, C, S, T, ld,
                     eps, lay.stat, v, v_mix);
  SEPR_CHECK_LAUNCH("segment SI-SNR kernels");
  return SEPR_OK;
}
