/*
 * sepr.h - C ABI of libsepr_hip.so: the SepReformer separator forward path for MI355X (gfx950).
 *
 * The reference (dmlguq456/SepReformer) is pure PyTorch Python: it has no FFI layer, every op below is
 * reached there through torch.nn modules calling aten kernels.  This header is therefore the boundary
 * the reference *would* bind if its modules dispatched to a native library: one entry point per fused
 * block of the hot path, each citing the reference module it replaces (paths relative to
 * /root/reference/models/SepReformer_Base_WSJ0/).  See INTEGRATION.md for the ctypes stubs.
 *
 * Conventions
 *   - plain C: raw device pointers, ints, a stream handle; no torch / C++ types cross the boundary;
 *   - every function returns an int status: SEPR_OK (0) or a negative SEPR_E* code; nothing throws;
 *   - no allocation inside: scratch is a caller-provided workspace (sepr_workspace_bytes tells how much);
 *   - the library never frees or retains caller memory, holds no global mutable state besides the
 *     opt-in profiler, the latched A/B switches and the per-thread deferred-finisher window (both below), and launches on the stream it is given (NULL = default stream): re-entrant
 *     from several host threads, one per device, like torch.nn.parallel.data_parallel's replicas
 *     (reference engine.py:64,98,130,167);
 *   - all activations are fp32, *channel-last* rows: a tensor the reference holds as [b, C, T] is
 *     [b, T, C] here (row = one frame); "rows" of a batch are (b, t) flattened;
 *   - weights are fp32 in the layouts noted per struct ("packed" = re-laid-out once on the host by
 *     sepreformer_amd/pack.py from the reference's state_dict tensors).
 *
 * This header is also READ AS TEXT: sepreformer_amd/lib.py derives its whole ctypes binding from it (sepreformer_amd/abi.py).  Inside the
 * extern "C" block keep to: #define NAME integer; typedef struct { members } name; typedef type name; enum { A = n, B, ... }; prototypes
 * with every parameter NAMED; base types void, char, short, int, unsigned, unsigned char, long long, unsigned long long, size_t, float,
 * double and the typedefs and structs declared above the use; comments anywhere.  The reader raises, with the line, on anything else.
 */
#ifndef SEPR_H_
#define SEPR_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEPR_VERSION 413 /* minor*100 + patch ("ABI 4.13").  Any struct-layout or context-size change bumps the MINOR number
                            (3.01 -> 3.03 grew sepr_ega_w under a patch bump: a caller built against 3.01 would have passed a short
                            struct).  A binding must compare sepr_version() with the SEPR_VERSION it was written against before its
                            first call: sepreformer_amd/lib.py refuses to load a library whose version differs. */

#define SEPR_OK 0
#define SEPR_EINVAL (-1)     /* bad shape / unsupported size / null pointer */
#define SEPR_EWORKSPACE (-2) /* workspace too small */
#define SEPR_EHIP (-3)       /* a HIP launch failed (see sepr_last_hip_error) */

typedef void* sepr_stream_t; /* hipStream_t */

/* ---- weight bundles (device pointers) --------------------------------------------------------- */

/* Optional second-precision ("bf16x3") form of one projection: the weight matrix pre-split into bf16
 * hi/lo planes in MFMA fragment order [N/16][K/32][plane][lane][8] with any LayerNorm gamma folded in,
 * and the bias with LayerNorm beta folded in (sepreformer_amd/pack.py::pack_x3).  wp == NULL selects the
 * exact f32-MFMA core for that projection; both cores share prologues and epilogues. */
typedef struct {
  const void* wp;
  const float* bias;
} sepr_x3_w;

/* GCFN, modules/network.py:46-66.  F -> 6F -> (dwconv3, GLU) 3F -> F */
typedef struct {
  const float* ln_g; /* [F]     net1.0.weight */
  const float* ln_b; /* [F]     net1.0.bias */
  const float* w1;   /* [6F,F]  net1.1.weight */
  const float* b1;   /* [6F]    net1.1.bias */
  const float* dw_w; /* [3,6F]  depthwise.weight, packed tap-major */
  const float* dw_b; /* [6F]    depthwise.bias */
  const float* w2;   /* [F,3F]  net2.2.weight */
  const float* b2;   /* [F]     net2.2.bias */
  const float* ls;   /* [F]     Layer_scale.layer_scale */
  sepr_x3_w x3_up;   /* net1 (LayerNorm folded) */
  sepr_x3_w x3_down; /* net2.2 */
  /* optional fully fused form (bf16x3, F = 64 or 128; pack.py::pack_gcfn_fused); both or none */
  const void* fused_w1p;   /* per 32-channel hidden chunk: [v0 v1 g0 g1][F/32][plane][64][8] bf16 (gamma folded)
                              + 4 KB fp32 constants [2][b1v b1g wv0 wv1 wv2 wg0 wg1 wg2 cbv cbg][16] */
  const void* fused_w2p;   /* [3F/32][F/16][plane][64][8] bf16, permuted k-slot order */
} sepr_gcfn_w;

/* CLA, modules/network.py:159-187 (eval-mode BatchNorm folded into w2/b2 by the packer) */
typedef struct {
  const float* ln_g; /* [F] */
  const float* ln_b; /* [F] */
  const float* w1;   /* [2F,F]  linear1.weight */
  const float* b1;   /* [2F] */
  const float* dw_w; /* [K,F]   dw_conv_1d.weight, packed tap-major (K = 65) */
  const float* dw_b; /* [F] */
  const float* w2;   /* [2F,F]  linear2.weight * bn_scale[row] */
  const float* b2;   /* [2F]    (linear2.bias - running_mean) * bn_scale + BN.bias */
  const float* w3;   /* [F,2F]  linear3.1.weight */
  const float* b3;   /* [F] */
  const float* ls;   /* [F] */
  sepr_x3_w x3_1;    /* linear1 (LayerNorm folded) */
  sepr_x3_w x3_2;    /* linear2 (BatchNorm folded) */
  sepr_x3_w x3_3;    /* linear3.1 */
  /* optional fused head / tail forms (bf16x3, F = 128; pack.py::pack_cla_fused); all three or none */
  const void* fused_w1p;   /* per 32 output channels: [v0 v1 g0 g1][F/32][plane][64][8] bf16 (gamma folded)
                              + 4 KB fp32 constants [4 tiles][16] biases */
  const void* fused_w2p;   /* per 64 hidden channels: [4 tiles][F/32][plane][64][8] bf16 + 4 KB [4][16] biases */
  const void* fused_w3p;   /* [2F/32][F/16][plane][64][8] bf16, permuted k-slot order */
} sepr_cla_w;

/* MultiHeadAttention, modules/network.py:69-124 */
typedef struct {
  const float* ln_g; /* [F] */
  const float* ln_b; /* [F] */
  const float* wqkv; /* [3F,F]  linear_q / linear_k / linear_v weights stacked */
  const float* bqkv; /* [3F] */
  const float* wo;   /* [F,F]   linear_out.weight */
  const float* bo;   /* [F] */
  const float* ls;   /* [F] */
  sepr_x3_w x3_qkv;  /* stacked q/k/v (LayerNorm folded) */
  sepr_x3_w x3_out;  /* linear_out */
  /* optional fully fused speaker-attention form (bf16x3, F = 128, 16-channel heads, S = 2;
     pack.py::pack_spk_fused); both or none; only read by sepr_spkattn_fwd */
  const void* fused_qkv_p; /* per head pair: [q0 q1 k0 k1 v0 v1][F/32][plane][64][8] bf16 (gamma folded)
                              + 4 KB fp32 constants [6 tiles][16] biases */
  const void* fused_out_p; /* [F/32][F/16][plane][64][8] bf16, permuted k-slot order */
} sepr_mha_w;

/* EGA, modules/network.py:126-155 + the shared relative-position table, modules/module.py:42-57 */
typedef struct {
  sepr_mha_w attn;
  const float* gate_ln_g; /* [F]   block.linear.0 */
  const float* gate_ln_b; /* [F] */
  const float* gate_w;    /* [F,F] block.linear.1 */
  const float* gate_b;    /* [F] */
  const float* pe_k;      /* [2*maxlen, F/H]  separator.pos_emb.pe_k.weight */
  int maxlen;
  sepr_x3_w x3_gate;      /* block.linear.1 (LayerNorm folded) */
  const void* fused_gate_p; /* optional (bf16x3, F = 128; pack.py::pack_gate_fused): per 64 output channels
                               [4 tiles][F/32][plane][64][8] bf16 (gamma folded) + 4 KB fp32 constants [4][16] biases */
  const void* pe_k_planes;  /* optional (bf16x3; pack.py, ABI 3.02): pe_k split ONCE into bf16 planes [2: hi, lo][2*maxlen][F/H] -
                               the attention kernel then stages its relative-position band without a per-tile VALU split */
  const void* fused_qkv_p;  /* optional (bf16x3, F = 128; pack.py::pack_gate_fused on self_attn's in-projection, ABI 4.11): the [3F, F]
                               q / k / v projection behind its LayerNorm in the gate's chunk form (6 chunks of 64 output channels) -
                               pooling + LayerNorm + projection then run as ONE launch (sepr_cla_fused.hip launch_ega_qkv) */
  const void* fused_out_p;  /* optional (bf16x3, F = 128, with fused_gate_p; pack.py::pack_outproj_fused, ABI 4.11): self_attn.linear_out as
                               fragments [F/16][F/32][plane][64][8] bf16 - the gate launch then computes its tile's rows of
                               LayerScale(linear_out(.)) itself and the separate output projection is gone */
} sepr_ega_w;

/* DownConvLayer, modules/module.py:63-78 (eval BN folded: y = gelu(conv_nobias * scale + shift)) */
typedef struct {
  const float* w;     /* [K,F] down_conv.weight packed tap-major (K = 5) */
  const float* scale; /* [F] */
  const float* shift; /* [F] */
} sepr_down_w;

/* SpkSplitStage, modules/module.py:110-125 */
typedef struct {
  const float* w1;   /* [4FS,F]   linear.0.weight */
  const float* b1;   /* [4FS] */
  const float* w2;   /* [FS,2FS]  linear.2.weight */
  const float* b2;   /* [FS] */
  const float* gn_g; /* [F]       norm.weight */
  const float* gn_b; /* [F] */
  sepr_x3_w x3_1;
  sepr_x3_w x3_2;
  /* optional one-kernel form of linear.0 + GLU + linear.2 (bf16x3, F = 128): the [rows, 2FS] gated tensor never reaches
   * HBM.  fused_w1p: per 32-channel hidden chunk the up-projection fragments + biases (gate rows pre-scaled by -log2 e),
   * fused_w2p: [FS/128][2FS/32][8][2][64][8] bf16 down-projection slices, one block of 128 output channels after the
   * other (pack.pack_glumlp_fused).  NULL = the two generic projections. */
  const void* fused_w1p;
  const void* fused_w2p;
} sepr_split_w;

/* Decoder-side fusion conv, modules/module.py:187,214 */
typedef struct {
  const float* w;    /* [F,2F]  simple_fusion.i.weight */
  const float* b;    /* [F] */
  sepr_x3_w x3;
} sepr_fuse_w;

/* OutputLayer + AudioDecoder, modules/module.py:237-283 */
typedef struct {
  const float* w1;   /* [4F,F]  end_conv1x1.0.weight */
  const float* b1;   /* [4F] */
  const float* w2;   /* [N,2F]  end_conv1x1.2.weight */
  const float* b2;   /* [N] */
  const float* wdec; /* [K,N]   ConvTranspose1d weight [N,1,K] packed tap-major */
  sepr_x3_w x3_1;
  sepr_x3_w x3_2;
  /* optional one-kernel form of end_conv1x1.0 + GLU + end_conv1x1.2 (bf16x3, F = 128, N % 128 == 0), as in sepr_split_w */
  const void* fused_w1p;
  const void* fused_w2p;
  /* optional (ABI 4.10), heads WITHOUT a mask only (masking = False, model.py:28): end_conv1x1.2 (2F -> N, bias) and the
   * ConvTranspose1d(N -> 1, K = 16, stride 4, no bias) have no nonlinearity between them, so they are ONE linear map:
   * fold_w2p = bf16 hi/lo k-slot fragments [2F/32][1][2][64][8] of W_fold[K, 2F] = wdec^T . W2, fold_b [K] = wdec^T . b2 (both formed in
   * fp64, pack.pack_glumlp_fold).  With fused_w1p set, sepr_outlayer_decoder_fwd(idx = NULL, enc = NULL) is then one launch: up-projection,
   * GLU, 16-row down-projection, overlap-add into wav; no [rows, N] tensor, no workspace.  NULL = the two-step form. */
  const void* fold_w2p;
  const float* fold_b;
} sepr_out_w;

/* ---- library ---------------------------------------------------------------------------------- */

int sepr_version(void);
const char* sepr_build_info(void);
/* A/B switches of the launch path (environment variables of the same names with the SEPR_ prefix).  They are read ONCE per process,
 * on first use - no entry point calls getenv on its launch path - and the host-side mirrors (sepreformer_amd/train_engine.py) ask the
 * library instead of parsing the environment themselves, so both sides always agree on a context layout.  sepr_knobs_reload() re-reads
 * the environment (tests that flip a switch inside one process call it between whole forward + backward runs, never inside one). */
enum { SEPR_KNOB_X3_WIDE = 0 /* 0 / 1 (default) / 2: sepr_gemm_x3.hip */, SEPR_KNOB_TRAIN_GCFN_PLANES /* default 1 */,
       SEPR_KNOB_TRAIN_ATTN_ONE /* default 1 */, SEPR_KNOB_TRAIN_CLA16 /* default 1 */,
       SEPR_KNOB_FOLD_HEAD /* default 1: main OutputLayer + AudioDecoder as one launch when sepr_out_w.fold_* are set */,
       SEPR_KNOB_TN16 /* default 1: weight-gradient contractions of two bf16 operands on the LDS-DMA + transposing-read kernel */,
       SEPR_KNOB_GB_FUSE /* default 1 (SEPR_GB_FUSE): sepr_global_block_fwd runs the EGA gate inside the GCFN kernel where that form exists;
                            0 = always the two calls (A/B, bit-identity tests) */,
       SEPR_KNOB_ATTN_PACK /* default 1 (SEPR_ATTN_PACK): the dk = 16 bf16x3 inference attention runs relattn_x3p_kernel (hi and lo plane of a K /
                              band row in one K = 32 MFMA fragment, read once); 0 = relattn_x3_kernel (A/B) */,
       SEPR_KNOB_COUNT };
int sepr_knob(int id);
void sepr_knobs_reload(void);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char* sepr_last_hip_error(void);

/* ops for sepr_workspace_bytes */
enum {
  SEPR_OP_ENCODER = 0, SEPR_OP_GCFN, SEPR_OP_CLA, SEPR_OP_EGA, SEPR_OP_SPKATTN,
  SEPR_OP_SPKSPLIT, SEPR_OP_OUTLAYER, SEPR_OP_PIT /* n = utterances, T = samples, S = speakers */, SEPR_OP_COUNT
};
/* Scratch bytes op needs for n sequences of T frames (Tp = pooled frames for EGA, source frames for
 * OUTLAYER; otherwise ignored), width F, encoder channels N, S speakers.  0 on bad arguments. */
size_t sepr_workspace_bytes(int op, int n, int T, int Tp, int F, int N, int S);

/* ---- hot path, in forward order ----------------------------------------------------------------- */

/* AudioEncoder.forward, modules/module.py:19-23: Conv1d(1->N, K=16, stride, no bias) + exact GELU.
 * wav [B,T] -> enc [B,L,N] (L = (T-K)/stride + 1); also the GroupNorm(1,N,eps) statistics of each
 * sample of enc (mean, rstd) -> gn_stats [B,2] for sepr_projector_fwd.  w_enc is [K,N] (packed). */
int sepr_encoder_fwd(const float* wav, int B, int T, const float* w_enc, int N, int K, int stride,
                     float gn_eps, float* enc, float* gn_stats, void* ws, size_t ws_bytes,
                     sepr_stream_t stream);

/* FeatureProjector.forward + Separator.pad_signal, modules/module.py:32-35,220-234:
 * GroupNorm(1,N) apply + 1x1 conv N->F (no bias); rows l >= L of out [B,Lp,F] are written as zeros. */
int sepr_projector_fwd(const float* enc, int B, int L, int Lp, int N, int F, const float* gn_stats,
                       const float* gn_g, const float* gn_b, const float* w, float* out,
                       sepr_stream_t stream);

/* GCFN.forward, modules/network.py:60-66.  x,y [n,T,F]; y may alias x (the fully fused form needs x != y and
 * is skipped when they alias). */
int sepr_gcfn_fwd(const float* x, float* y, int n, int T, int F, const sepr_gcfn_w* w, void* ws,
                  size_t ws_bytes, sepr_stream_t stream);

/* CLA.forward (eval), modules/network.py:174-187.  x,y [n,T,F]; y may alias x. */
int sepr_cla_fwd(const float* x, float* y, int n, int T, int F, int K, const sepr_cla_w* w, void* ws,
                 size_t ws_bytes, sepr_stream_t stream);

/* EGA.forward, modules/network.py:138-155 (with MultiHeadAttention.forward :90-124 and the relative
 * position bias of modules/module.py:52-57,196-198 computed from pe_k without materialising pos_k).
 * x,y [n,T,F], T = Tp * 2^k; y must NOT alias x. */
int sepr_ega_fwd(const float* x, float* y, int n, int T, int Tp, int F, int H, const sepr_ega_w* w,
                 void* ws, size_t ws_bytes, sepr_stream_t stream);

/* One global block, modules/network.py:198-209: y_mid = EGA(x), y = GCFN(y_mid) - what sepr_ega_fwd followed by sepr_gcfn_fwd write, bit
 * for bit.  gate_perm_p (optional; pack.py::pack_gate_fused_perm, built beside sepr_ega_w.fused_gate_p) is the gate projection with its
 * output rows in the order of the GCFN kernel's frame fragments: with it, for F = 128, 1 < T / Tp dividing 64 and launches large enough for
 * the 126-frame-tile GCFN kernel, the gate runs in that kernel's tile prologue (no stand-alone pass over the residual stream).  Every other
 * case, and SEPR_GB_FUSE=0, is the two calls.  x, y_mid, y [n,T,F], pairwise distinct; workspace as for sepr_ega_fwd. */
int sepr_global_block_fwd(const float* x, float* y_mid, float* y, int n, int T, int Tp, int F, int H, const sepr_ega_w* ega,
                          const sepr_gcfn_w* gcfn, const void* gate_perm_p, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* SpkAttention.forward up to (excluding) its feed_forward GCFN, modules/network.py:233-247:
 * attention across the S speakers of each frame + residual.  x,y [B*S,T,F] (row index b*S+s);
 * y may alias x.  Follow with sepr_gcfn_fwd for :249. */
int sepr_spkattn_fwd(const float* x, float* y, int nS, int S, int T, int F, int H,
                     const sepr_mha_w* w, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* DownConvLayer.forward (eval), modules/module.py:72-78.  x [n,T,F] -> y [n,(T-1)/2+1,F]. */
int sepr_downconv_fwd(const float* x, float* y, int n, int T, int F, int K, const sepr_down_w* w,
                      sepr_stream_t stream);

/* SpkSplitStage.forward, modules/module.py:120-125.  x [B,T,F] -> y [B*S,T,F] incl. GroupNorm(1,F). */
int sepr_spksplit_fwd(const float* x, float* y, int B, int S, int T, int F, float gn_eps,
                      const sepr_split_w* w, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* Decoder-side fusion, modules/module.py:212-214: nearest x2 upsample of lo [n,T/2,F], concat with
 * skip [n,T,F] along channels, Conv1d(2F->F,k=1) -> y [n,T,F]. */
int sepr_fuse_fwd(const float* lo, const float* skip, float* y, int n, int T, int F, const sepr_fuse_w* w,
                  sepr_stream_t stream);

/* OutputLayer.forward (+Masking when enc != NULL) and AudioDecoder.forward, modules/module.py:249-283,
 * modules/network.py:34-43, model.py:42-52.  x [nS,Tsrc,F]; frame l < L of the head reads source
 * frame idx[l] (idx == NULL: l itself, i.e. the crop of :250; otherwise the nearest-upsample table of
 * model.py:49).  enc [B,L,N] or NULL.  wav [S,B,Tout], Tout = (L-1)*stride + K. */
int sepr_outlayer_decoder_fwd(const float* x, int nS, int S, int Tsrc, int L, const int* idx,
                              const float* enc, int F, int N, int K, int stride, const sepr_out_w* w,
                              float* wav, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* The auxiliary heads (model.py:47-52) as NH basis calls + ONE decoder launch that reads each encoder frame once for all heads and
 * speakers, instead of NH sepr_outlayer_decoder_fwd(idx, enc) calls that each read enc once per speaker.  The waveforms are bit-identical.
 * sepr_outlayer_basis_fwd: the two OutputLayer projections of a head on its nS*Tsrc SOURCE rows (Tsrc <= L; the launches
 * sepr_outlayer_decoder_fwd issues for an upsampled head): x [nS,Tsrc,F] -> o2 [nS*Tsrc,N], caller-owned.  Workspace as for
 * SEPR_OP_OUTLAYER.
 * sepr_aux_decoder_fwd: for h < NH, 1 <= NH <= 4: wav[h] [S,B,Tout] = decoder(ReLU(o2[h][b*S+s, idx[h][l]]) * enc[b,l]) with wdec[h] [K,N] (sepr_out_w.wdec), idx[h] [L] the
 * nearest-upsample table with values < Tsrc[h] <= L.  o2, idx, wdec, wav, Tsrc are HOST arrays of NH entries (device pointers / ints), copied into
 * the launch.  S in {2,3}, K = 16, 4 <= stride <= 16, N % 64 == 0; SEPR_EINVAL for anything else or a NULL entry (use the per-head call then). */
int sepr_outlayer_basis_fwd(const float* x, int nS, int Tsrc, int L, int F, int N, const sepr_out_w* w, float* o2, void* ws,
                            size_t ws_bytes, sepr_stream_t stream);
int sepr_aux_decoder_fwd(int NH, const float* const* o2, const int* const* idx, const float* const* wdec, float* const* wav,
                         const int* Tsrc, const float* enc, int B, int S, int L, int N, int K, int stride, sepr_stream_t stream);

/* GroupNorm(1 group) statistics of x [n, count] -> stats [n,2] = (mean, rstd).  modules/module.py:28,117 */
int sepr_groupnorm_stats(const float* x, int n, long long count, float eps, float* stats, void* ws,
                         size_t ws_bytes, sepr_stream_t stream);

/* y[M,N] = x[M,K] . w[N,K]^T + bias : the f32-MFMA projection core on its own (tests, roofline bench) */
int sepr_linear_fwd(const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                    sepr_stream_t stream);
/* the same product on the bf16x3 core; wp = pack_x3(w) */
int sepr_linear_x3_fwd(const float* x, const void* wp, const float* bias, float* y, int M, int N, int K,
                       sepr_stream_t stream);

/* ---- criteria --------------------------------------------------------- */
/* Permutation-invariant SI-SNR of S <= 3 separated waveforms, utils/implements/criterions.py:
 *   PIT_SISNR_time.__call__ :191-217   loss[b]   = min over permutations of sum_s clamp(-SISNR(est_s, tgt_p(s)), clamp_min)
 *   PIT_SISNRi.__call__     :232-260   sisnri[b] = per-estimate SISNR(est_s, tgt_p(s)) - SISNR(mix, tgt_p(s)) of the
 *                                                  permutation maximising their sum
 * est, tgt [S,B,T] (the reference's lists of [B,T] stacked), mix [B,T] or NULL (then sisnri / sisnri_perm must be
 * NULL).  eps_loss = 1e-8 (:199), eps_i = the caller's eps (1e-15 in engine.py:131), clamp_min = -30 (:212).
 * loss [B]; loss_perm / sisnri_perm [B,S] = target index per estimate (NULL to skip); sisnri [B,S].  The batch
 * mean the reference returns (sum / num_utts) is a host-side mean of `loss`.  Scale-invariant form only
 * (scale_inv: true in every shipped config).  Workspace: sepr_workspace_bytes(SEPR_OP_PIT, B, T, 0, 0, 0, S). */
int sepr_pit_sisnr_fwd(const float* est, const float* tgt, const float* mix, int S, int B, int T,
                       double eps_loss, double eps_i, double clamp_min, float* loss, int* loss_perm,
                       float* sisnri, int* sisnri_perm, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* PIT_SISNR_mag.__call__, utils/implements/criterions.py:148-176 with the conv-STFT of :43-113: per utterance
 *   loss[b] = min over permutations of sum_s -20 log10(eps + |M(c t_p(s))| / (|M(est_s) - M(c t_p(s))| + eps)),
 * M = sqrt(re^2 + im^2 + 1e-10) of the STFT of the zero-mean signal (frame_len-point DFT kernel `dft`, hop
 * frame_shift, zero padding to a multiple of the hop, no centre padding), c = max(<e~,t~> / (|t~|^2 + eps), 1e-2),
 * norms over bins and frames.  est, tgt [S,B,T]; dft [(frame_len + 2 rounded up to 4), frame_len] row-major = the
 * reference's STFTBase.K (real rows, then imaginary rows, then zero rows); loss [B]; perm [B,S] or NULL.
 * mel_opt = false only.  Workspace: sepr_pit_sisnr_mag_workspace(S, B, T, frame_len, frame_shift). */
size_t sepr_pit_sisnr_mag_workspace(int S, int B, int T, int frame_len, int frame_shift);
int sepr_pit_sisnr_mag_fwd(const float* est, const float* tgt, int S, int B, int T, const float* dft,
                           int frame_len, int frame_shift, double eps, float* loss, int* perm, void* ws,
                           size_t ws_bytes, sepr_stream_t stream);

/* Source-aggregated, soft-thresholded SDR (SA-SDR with a threshold) - beyond the reference.  One ratio per
 * utterance over all S sources, not scale-invariant, defined when a target is silent (~ = zero-mean):
 *   D = sum_k |t~_k|^2,  E_p = sum_s |e~_s - t~_p(s)|^2,  loss[b] = min over permutations of 10 log10((E_p + tau D + eps) / (D + eps)),
 *   tau = 10^(-snr_max / 10) (snr_max = 30: the -30 dB floor clamp_min gives the SI-SNR form), eps = 1e-8.
 * perm [B,S] (NULL to skip) = the first minimiser of E_p in itertools.permutations order.  The magnitude form is the same expression on
 * M = sqrt(re^2 + im^2 + 1e-10) of the conv-STFT of the zero-mean signals (geometry, padding and `dft` of sepr_pit_sisnr_mag_fwd, target
 * scale 1, no projection), norms over bins and frames.  Same arguments as the SI-SNR siblings, snr_max in the place of clamp_min.
 * Workspaces are the siblings' layouts and are sized by the siblings' entries: sepr_workspace_bytes(SEPR_OP_PIT, B, T, 0, 0, 0, S) and
 * sepr_pit_sisnr_mag_workspace(S, B, T, frame_len, frame_shift). */
int sepr_pit_sasdr_fwd(const float* est, const float* tgt, int S, int B, int T, double eps, double snr_max, float* loss, int* perm,
                       void* ws, size_t ws_bytes, sepr_stream_t stream);
int sepr_pit_sasdr_mag_fwd(const float* est, const float* tgt, int S, int B, int T, const float* dft, int frame_len, int frame_shift,
                           double eps, double snr_max, float* loss, int* perm, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* BSS-eval source criteria of mir_eval 0.7 bss_eval_sources (compute_permutation=True, distortion filters of 512 taps), the
 * metric behind PIT_SDRi (utils/implements/criterions.py:264-289, engine.py:133) - evaluation only, no backward.
 * est, ref [S,B,T] float32 on the device, 2 <= S <= 3; mix [B,T] or NULL (then sdr_mix must be NULL); lengths [B] is a HOST
 * array of valid lengths, S*512 <= lengths[b] <= T (samples beyond lengths[b] are ignored).  float64 arithmetic throughout:
 * lagged correlations, the joint Gram of the delayed references and each reference's own Gram, Cholesky factors with the
 * right-hand sides carried as bordering rows, and the closed-form projection energies E, P_j, P_all:
 *   SDR = 10 log10(P_j / (E - P_j)), SIR = 10 log10(P_j / (P_all - P_j)), SAR = 10 log10(P_all / (E - P_all)),
 * a zero denominator giving +inf as mir_eval's _safe_db does.  Outputs [B,S], indexed by REFERENCE k as mir_eval returns them:
 * sdr/sir/sar[b,k] of estimate perm[b,k], perm = the first maximiser of the mean SIR in itertools.permutations order (the
 * reverse of sepr_pit_sisnr_fwd's estimate-indexed permutations).  sdr_mix[b,k]: the SDR of the mixture against reference k
 * (the mixture repeated S times, as PIT_SDRi passes it: every SIR ties, so the permutation is the identity).
 * status[b]: 0 ok, 1 a silent (all-zero) reference, estimate or mixture (mir_eval raises ValueError), 2 a non-positive
 * Cholesky pivot; the values of a failed utterance are NaN.  Bit-identical from run to run.
 * Workspace: sepr_bss_eval_workspace(S, B, T) bytes, about (S*512)^2 * 8 per utterance (0 for unsupported S / T). */
size_t sepr_bss_eval_workspace(int S, int B, int T);
int sepr_bss_eval_fwd(const float* est, const float* ref, const float* mix, const int* lengths, int S, int B, int T,
                      double* sdr, double* sir, double* sar, int* perm, double* sdr_mix, int* status, void* ws,
                      size_t ws_bytes, sepr_stream_t stream);

/* STOI and ESTOI, the intelligibility measures of Taal et al. 2011 and Jensen & Taal 2016 (the definition restates
 * pystoi 0.3.3 and is given in full in section 5f and tests/stoi_ref.py) - evaluation only, no backward.
 * Inputs are float32 on the device and ALREADY AT 10 kHz: ref [B][S][T], est [B][S][T], mix [B][T] or NULL (then stoi_mix and estoi_mix
 * must be NULL too, and both must be given with a mixture), lengths [B] DEVICE int32 valid samples (clamped to [0, T]; samples beyond
 * are never read).  2 <= S <= 3, T >= 256, B S (S + 2) <= 65535.  tables: DEVICE float64 [256 + 2 * 256 * 212], built by the host once
 * (sepreformer_amd/criterion.py::stoi_tables): w[t] = hanning(258)[1 + t], then for t < 256 and k < 212 the pair
 * (cos, sin)(2 pi ((7 + k) t mod 512) / 512) at tables[256 + 2 (212 t + k)]; 16-byte aligned.
 * Per (b, reference i): frames x[128 k .. 128 k + 256) w while 128 k <= len - 256; e_k = 20 log10(||frame_k|| + 2^-52); frame k is kept iff
 * max(e) - 40 - e_k < 0; the kept frames of the reference - and the frames of every processed signal at the same indices - are
 * overlap-added at hop 128, framed again (kept - 1 frames, windowed a second time) and transformed at 512 points; band value b =
 * sqrt(sum |X|^2 over bins [lo_b, hi_b)), the bins of linspace(0, 10000, 513) nearest to 150 * 2^((2 b -+ 1) / 6), b < 15.  Over all
 * segments of 30 consecutive frames: STOI = mean of the row-normalised correlations of X and min(Y ||X_row|| / (||Y_row|| + eps),
 * X (1 + 10^(15 / 20))); ESTOI = mean of the correlations after row- then column-normalisation.  All arithmetic is float64.
 * Outputs: stoi, estoi [B][S][S] float64, entry (i, j) = reference i against estimate j; stoi_mix, estoi_mix [B][S] = reference i
 * against the mixture; kept [B][S] int32 = kept frames of reference i; status [B][S] int32, bit 0 = "too short" (fewer than 30 spectral
 * frames: the values of that reference are 1e-5, as the package returns them with a warning).  Bit-identical from run to run, and an
 * utterance's values do not depend on what else is in the call.  No atomics, no host synchronisation or allocation (capturable: the
 * grids are sized by T, never by a count read back from the device).  Every argument check returns SEPR_EINVAL (SEPR_EWORKSPACE for a
 * short workspace) before any HIP call.  Workspace: sepr_stoi_workspace(S, B, T) bytes (0 for unsupported arguments), about
 * 15 (S + 2) S doubles per frame of T. */
size_t sepr_stoi_workspace(int S, int B, int T);
int sepr_stoi_fwd(const float* ref, const float* est, const float* mix, const int* lengths, int S, int B, int T, const double* tables,
                  double* stoi, double* estoi, double* stoi_mix, double* estoi_mix, int* kept, int* status, void* ws, size_t ws_bytes,
                  sepr_stream_t stream);

/* Long-form separation (the reference has no long-form mode): boundary alignment and overlap-add of the
 * separator's outputs on overlapping windows.  R recordings; recording r has lengths[r] = T_r >= 1 samples and
 * Nc_r = 1 (T_r <= W) or 1 + ceil((T_r - W) / H) windows of W samples at hop H = W - O, window k covering [kH, kH + W); its
 * windows are chunks[chunk_offset[r] .. chunk_offset[r + 1]), chunk_offset[0] = 0.  chunk_offset [R+1] and lengths [R] are
 * HOST arrays (copied into the workspace on `stream`: under graph capture they are read when the copy node runs).
 * chunks [total_chunks][S][W] float32 (total_chunks = chunk_offset[R]); W and O multiples of 4, 0 < O <= W / 2; chunks and y
 * 16-byte aligned; S in {2, 3}.  Per boundary k | k+1, over a_i = source i of window k on its last O samples and b_j = source j
 * of window k+1 on its first O samples, in float64 and a fixed order: C[i][j] = <a_i, b_j>, Ea[i] = <a_i, a_i>, Eb[j] = <b_j, b_j>;
 *   pi_k = the lexicographically first maximiser of sum_i |C[i][pi(i)]| / sqrt(Ea[i] Eb[pi(i)] + 1e-20);
 *   P_0 = identity, P_{k+1}(s) = pi_k(P_k(s));  g_0 = 1, g_{k+1}(s) = g_k(s) * (C[i][j] / Eb[j]) with i = P_k(s), j = pi_k(i)
 *   when match_gain, else g = 1; the ratio is replaced by 1 (gain carried) when Ea[i] / O or Eb[j] / O is below 1e-10, the
 *   normalised correlation |C[i][j]| / sqrt(Ea[i] Eb[j] + 1e-20) is below 0.5, or the ratio is not finite.
 * perm [total_chunks][S] int32 = P_k(s), gain [total_chunks][S] float32 = g_k(s) (rounded from float64).
 * y[r][s][t] = sum_k w_k(t) g_k(s) chunks[k][P_k(s)][t - kH] for t < T_r: in the overlap of boundary k - 1 | k at offset j
 * the incoming window weighs w = (float) sin^2(pi (j + 0.5) / (2 O)) (double sine), the outgoing 1.0f - w; elsewhere 1.
 * y is packed by the offsets: track s of recording r starts at y + S (chunk_offset[r] H + r O) + s (Nc_r H + O) and holds
 * Nc_r H + O >= T_r samples, zero from T_r on; S (total_chunks H + R O) floats in all.  Bit-identical from run to run; no host
 * synchronisation or allocation (capturable).  Every argument check returns SEPR_EINVAL (SEPR_EWORKSPACE for a short workspace)
 * before any HIP call.  Workspace: sepr_stitch_workspace(R, total_chunks, S) bytes (0 for unsupported arguments). */
size_t sepr_stitch_workspace(int R, int total_chunks, int S);
int sepr_stitch_fwd(const float* chunks, const int* chunk_offset, const int* lengths, int R, int S, int W, int O, int match_gain,
                    float* y, int* perm, float* gain, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* The stream bank: the stitch above, one boundary per call, for recordings whose length is known only at their end.
 * A stream's window k covers [kH, kH + W).  Its state lives in a slot of `state`: the raw last O samples of its latest window (all S
 * sources, un-permuted), P and g - g in float64, so that the gains equal sepr_stitch_fwd's bit for bit at every boundary.
 * sepr_streambank_step advances the A >= 1 streams of one hop in ONE launch (one workgroup per stream, which does everything for it in
 * order).  win: HOST array of S device pointers; win[s] holds source s of the hop's windows as [A][ld] rows (ld >= W, a multiple of 4;
 * 16-byte aligned), row a belonging to table row a - the separator's outputs are read where the forward left them.
 * table: DEVICE int64 [A][6] = slot, k, n_emit, has_window, out offset, track stride (the last two in elements).  For a row with a window:
 *   k = 0: P = identity, g = 1.  k > 0: C, Ea, Eb over the saved tail and the window's first O samples with sepr_stitch_fwd's arithmetic and
 *   order (shared code), its pi and ratio rules, then g(s) = g(s) * ratio[P(s)], P(s) = pi(P(s)).
 *   Emit n_emit samples of every track s at out + offset + s * stride: sample j < O of a window k > 0 is
 *   fmaf(w * g_k, c_k[P_k(s)][j], ((1.0f - w) * g_{k-1}) * tail[P_{k-1}(s)][j]) with sepr_stitch_fwd's w, any other j is g_k * c_k[P_k(s)][j]
 *   (gains rounded to float32).  n_emit = H for a window that is not its stream's last, T - kH in (O, W] for the last.
 *   Save the window's last O samples, P and g.
 * A row without a window is the flush form, used when a stream ends on a full window: it emits g(s) * tail[P(s)][j] for j < n_emit <= O and
 * leaves the state as it is.  Zeros are written for n_emit <= j < roundup4(n_emit) and nothing beyond; offset and stride are multiples of 4.
 * perm [A][S] int32 and gain [A][S] float32 receive P and g of every row as the step leaves them.  The kernel clamps slot into [0, slots),
 * n_emit into [0, W] ([0, O] for a flush) and a stored P into [0, S), and emits nothing for a row whose offset / stride are negative,
 * misaligned or reach past out_elems: a bad table gives wrong samples, never an access outside the state, the windows or `out`.  Two rows of
 * one launch must not name the same slot.  No workspace, no atomics, no host synchronisation (capturable); bit-identical from run to run.
 * SEPR_EINVAL before any HIP call for null pointers (win[s] included), S outside 2..3, A < 1, slots < 1, W or O not multiples of 4, O <= 0,
 * 2 O > W, ld < W or not a multiple of 4, out_elems < 4, misaligned buffers; SEPR_EWORKSPACE for a state shorter than
 * sepr_streambank_state_bytes(slots, S, O) (0 for unsupported arguments).
 * sepr_streambank_gather forms the [A][W] input of a hop in one launch: x[a][j] = sample start + j of the stream whose ring of `cap` samples
 * begins at store + base (sample t lies at index t mod cap), zero for start + j >= received.  table: DEVICE int64 [A][3] = base, start,
 * received; cap a multiple of 4 with cap >= W; base and start multiples of 4.  A row whose ring does not lie inside store_elems gives zeros.
 * New entries, no struct change: ABI 4.13. */
long long sepr_streambank_state_bytes(int slots, int S, int O);   /* (long long: the size_t entries are the workspace sizes) */
int sepr_streambank_step(const float* const* win, long long ld, const long long* table, int A, int slots, int S, int W, int O, int match_gain,
                         float* out, long long out_elems, int* perm, float* gain, void* state, size_t state_bytes, sepr_stream_t stream);
int sepr_streambank_gather(const float* store, long long store_elems, long long cap, const long long* table, int A, int W, float* x,
                           sepr_stream_t stream);

/* Sample-rate conversion inside the stream bank: the converter of sepr_resample_fwd below - the same constants, tables and
 * [K][L] device layout, the same float64 fma chain from 0.0 in the order j = 0 .. K - 1, n M in 64 bits, one rounding - computed a span of
 * outputs at a time, so that a stream is converted while it arrives.  sepr_streambank_convert serves A >= 1 rows in ONE launch; a row is
 * one stream on the input side, one (stream, track) on the output side.  table: DEVICE int64 [A][10] =
 *   conv, n0, n1, T_known, src base, src origin, src cap, dst base, dst origin, dst cap.
 * The row computes outputs [n0, n1) of converter conv < NC:  y[n] = float32(sum_{j < K} double(tap[(n M) mod L][j]) * double(x[floor(n M / L)
 * - Hh + j])) with x zero outside [0, T_known).  Source sample t is read from the ring src[base + (t - origin) mod cap], output n is written to
 * the ring dst[base + (n - origin) mod cap] (bases, origins and caps in elements; a linear buffer is a ring that never wraps).  The caller
 * names only outputs whose inputs exist - floor(n M / L) + Hh + 2 <= T_known while the stream is open, every n < ceil(T L / M) once T is known
 * - and then the result equals sepr_resample_fwd of the whole recording bit for bit.  conv_taps / conv_L / conv_M / conv_K / NC: a converter
 * set (described once, at sepr_resample_fwd below) with 1 <= NC <= 16 and 4-byte aligned tables; rows of different converters share the
 * launch, L = 1 included.  nmax: HOST, at least the largest n1 - n0 of the table; it sizes the grid, and a row
 * computes at most nmax outputs.  The kernel clamps conv into [0, NC), n0 and n1 into [0, 2^62 / M] and computes nothing for a row whose
 * src or dst ring does not lie inside src_elems / dst_elems: a bad table gives wrong samples, never an access outside the buffers.  Two rows
 * must not write the same destination element, and dst must not overlap what the launch reads.  No workspace, no atomics, no host
 * synchronisation or allocation (capturable); bit-identical from run to run.  SEPR_EINVAL before any HIP call for null pointers
 * (conv_taps[k] included), A < 1 or > 65535, NC outside 1..16, L, M or K < 1, K odd, nmax < 1, src_elems or dst_elems < 1, buffers not
 * 4-byte aligned (the table 8), and for a converter whose tile span (255 M / L + K + 1 samples) exceeds 64 KiB of doubles.
 * sepr_streambank_carry keeps the history the output side needs.  buf holds rows [slots][S][row_len] (row_len >= 2 hist, both multiples of 4,
 * 16-byte aligned): [0, hist) of a row are the last hist samples emitted before the hop, the step emits from hist on.  For the slot of every row
 * of step_table (sepr_streambank_step's [A][6] table; column 0, clamped into [0, slots)) and every track, [0, hist) <- [hist, 2 hist): after a
 * window that emitted hist = H samples, the row again starts with the last H emitted.  A launch of its own after the conversion that reads the
 * old history - the order of two launches on one stream is the synchronisation.  New entries, no struct change: ABI 4.13. */
int sepr_streambank_convert(const float* src, long long src_elems, float* dst, long long dst_elems, const long long* table, int A,
                            long long nmax, const float* const* conv_taps, const int* conv_L, const int* conv_M, const int* conv_K, int NC,
                            sepr_stream_t stream);
int sepr_streambank_carry(float* buf, long long buf_elems, const long long* step_table, int A, int slots, int S, int hist, long long row_len,
                          sepr_stream_t stream);

/* Sample-rate conversion of whole recordings (the reference resamples on the host inside librosa.load(path, sr=fs),
 * engine.py:155).  Rational ratio fs_out / fs_in = L / M (coprime), K taps per output phase (K even), Hh = (K - 2) / 2:
 *   y[n] = sum_{j < K} tap[(n M) mod L][j] * x[floor(n M / L) - Hh + j],  x zero outside [0, T),  0 <= n < N = ceil(T L / M).
 * The products of float32 taps and float32 samples are exact in float64; they are summed in float64 in the order j = 0 .. K - 1 and the sum
 * is rounded once to float32.  Bit-identical from run to run; a recording's result does not depend on what else is in the call.
 * R recordings in one launch, packed as CSR: recording r is x[in_offset[r] .. in_offset[r + 1]) (T_r >= 1 samples) and receives
 * y[out_offset[r] .. out_offset[r + 1]), out_offset[r + 1] - out_offset[r] = sepr_resample_out_len(T_r, L, M); both offset arrays start
 * at 0 and are HOST arrays (copied into the workspace on `stream`: under graph capture they are read when the copy node runs).
 * taps: DEVICE layout, float32 [K][L] with taps[j][q] = tap[(q M) mod L][j] - transposed and in output order, so that output n reads column
 * n mod L (for L = 1 this is the tap row itself); sepreformer_amd/resample.py::plan builds the table for the Kaiser-windowed sinc of section 5d.
 * R <= 65535; ratios whose tile span (255 M / L + K + 1 samples, + K for L = 1) exceeds 64 KiB of doubles are SEPR_EINVAL.  Every argument
 * check returns SEPR_EINVAL (SEPR_EWORKSPACE for a short workspace) before any HIP call; no host synchronisation or allocation (capturable).
 * sepr_resample_out_len: 0 for T, L or M < 1.  Workspace: sepr_resample_workspace(R) bytes (0 for unsupported R).
 * A CONVERTER SET (conv_taps / conv_L / conv_M / conv_K / NC of sepr_streambank_convert, sepr_dynmix_speed_fwd, sepr_dynmix_speed_reverb_fwd) is
 * NC <= 16 converters as HOST arrays read before the call returns: conv_taps[k] the DEVICE pointer to converter k's float32 [K][L] table in the
 * layout above, conv_L[k], conv_M[k] >= 1, conv_K[k] even and >= 2; anything else, or a null array or table pointer while NC > 0, is
 * SEPR_EINVAL.  The least NC, the span limit and the alignment are each entry's own. */
long long sepr_resample_out_len(long long T, int L, int M);
size_t sepr_resample_workspace(int R);
int sepr_resample_fwd(const float* x, const long long* in_offset, float* y, const long long* out_offset, int R, const float* taps, int L,
                      int M, int K, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* Training batches from a device-resident corpus (the reference mixes on the host, in numpy, inside its DataLoader
 * workers: models/SepReformer_Large_DM_{WSJ0,WHAM,WHAMR}/dataset.py::_dynamic_mixing / _direct_load / _collate).
 * Corpus: N >= 1 utterances of at least one sample.  The first N16 are int16 (PCM16 as on disk; the sample value is s / 32768, exact in
 * float32) and lie back to back in buf16, the other N - N16 are float32 and lie back to back in buf32.  offsets [N + 1] int64 (DEVICE) holds
 * the cumulative element counts over all N: utterance u < N16 is buf16[offsets[u] .. offsets[u + 1]), utterance u >= N16 is
 * buf32[offsets[u] - offsets[N16] .. offsets[u + 1] - offsets[N16]).  total16 = offsets[N16] and total32 = offsets[N] - offsets[N16] are passed
 * by value (the table is device memory); both buffers are 16-byte aligned and ALLOCATED up to a multiple of 16 bytes (the kernels read
 * aligned 16-byte words).  A buffer with no utterance may be NULL.
 *
 * sepr_corpus_energy: sum of squares per utterance.  ss16 [N16] int64 = sum s^2 of the raw int16 values - exact (a square is below 2^30), so
 * independent of the summation order: rms = sqrt(ss / (32768^2 n)) is the same number everywhere.  ss32 [N - N16] float64 = sum of the
 * (exact) float64 squares in a fixed order: per-workgroup partials, then one finishing pass; no atomics, bit-identical from run to run.
 * Workspace: sepr_corpus_energy_workspace(N) bytes (0 for N < 1).
 *
 * sepr_dynmix_fwd: one launch builds a batch.  Example b of B has M mixture terms and S target terms, flattened as term j = b (M + S) + m
 * (m < M: mixture terms, then the S target terms); S in {2, 3}, M in {S, S + 1}.  A term is (term_utt[j], term_start[j], term_norm[j],
 * term_gain[j]): its value at output sample t is (x[term_start + t] * term_norm) * term_gain with x the utterance's sample value - two
 * separately rounded float32 multiplies, never contracted.  n [B] int32 = the example's length, Tmax a multiple of 4.
 *   mix[b][t]    = ((0 + term_0) + term_1) + ... in term order for t < n[b], 0 for n[b] <= t < Tmax          mix [B][Tmax] float32
 *   src[s][b][t] = target term s for t < n[b], 0 beyond                                                       src[s] [B][Tmax] float32
 * src is a HOST array of S device pointers (read before the call returns), so the rows of one [S][B][Tmax] tensor and S separate tensors
 * are both served; mix and every src[s] 16-byte aligned.  A target term that equals mixture term s bit for bit (the WSJ0 / WHAM forms) is
 * computed once.  All five table arrays are DEVICE memory, so the call cannot validate them: the caller guarantees
 * term_start + n[b] <= the utterance's length; the kernel clamps the utterance index, the start and every read position, so that a bad table
 * yields wrong samples but never a read outside the corpus buffers.  SEPR_EINVAL before any HIP call for a null pointer, B < 1 (or > 65535),
 * S outside 2..3, M outside S..S+1, Tmax < 4 or not a multiple of 4, a misaligned pointer or an inconsistent corpus description.  No
 * workspace, no host synchronisation or allocation (capturable: the pointers are frozen, the table contents are read at replay).
 *
 * sepr_dynmix_speed_fwd: sepr_dynmix_fwd with speed perturbation.  term_conv [B (M + S)] int32 (DEVICE): -1 = the term is
 * the stored utterance, as in sepr_dynmix_fwd and with its bits; k in 0 .. NC - 1 = the term is the utterance passed through converter k.  The
 * converters are a converter set (sepr_resample_fwd above) with 0 <= NC <= 16 (the four arrays may be NULL for NC = 0).  The perturbed utterance has
 * sepr_resample_out_len(T, L, M) samples and its sample y[n] is exactly sepr_resample_fwd's: exact float64 products summed in the order
 * j = 0 .. K - 1, rounded once to float32, x zero outside [0, T) of THAT utterance.  A perturbed term's value at output sample t is
 * (y[term_start + t] * term_norm) * term_gain: term_start indexes the perturbed utterance, the phase is ((term_start + t) M) mod L in 64-bit
 * arithmetic, and the caller guarantees term_start + n[b] <= the perturbed length.  The conversion runs inside the one launch, on the cropped span
 * only: per workgroup of 2048 outputs the input span 2047 M / L + K + 1 samples is staged in LDS, and a converter whose span exceeds 3072 samples
 * is SEPR_EINVAL, as are NC outside 0..16, a null term_conv, a null converter array or table pointer while NC > 0, L, M or K < 1, K odd, and
 * everything sepr_dynmix_fwd refuses - all before any HIP call.  A target term that equals mixture term s bit for bit, converter index included,
 * is computed once.  The kernel clamps the converter index (negative = none, above NC - 1 = NC - 1), the utterance index and every read
 * position: a bad table yields wrong samples but never a read outside the corpus.  No workspace, no host synchronisation or allocation
 * (capturable: the pointers and the converter descriptions are frozen, the table contents are read at replay).
 *
 * sepr_dynmix_reverb_fwd: sepr_dynmix_fwd with reverberation by convolution.  The RIR bank is R >= 1 float32 impulse
 * responses h_r of len_r samples, 1 <= len_r <= 16384, back to back in rir [rir_total] (DEVICE, 4-byte aligned) with rir_off [R + 1] int64 (DEVICE)
 * their cumulative sample counts.  term_rir [B (M + S)] int32 (DEVICE): -1 = the term is the stored utterance, with sepr_dynmix_fwd's loads and
 * bits; r in 0 .. R - 1 = the term is the utterance convolved with the first term_taps [B (M + S)] (int32, DEVICE, 1 <= taps <= len_r) samples of
 * h_r:
 *   y[t] = float32(sum_{j = 0 .. taps - 1} double(h_r[j]) * double(x[term_start + t - j])),   x = 0 outside [0, T) of THAT utterance,
 * the products exact in float64, added in the order j = 0 .. taps - 1 as fma(h, x, acc) from acc = 0.0, one rounding to float32; the term's
 * value is (y[t] * term_norm) * term_gain, the two separately rounded float32 multiplies.  So a term is "convolve the whole utterance, truncate
 * to its stored length, crop" bit for bit - the tail of the samples before the crop is in the crop, the reverberant utterance keeps the stored
 * length (the caller guarantees term_start + n[b] <= T as for a plain term) - and h = [1.0] gives the plain term's bits.  The convolution runs
 * inside the one launch: per workgroup of 2048 outputs the taps are walked in ascending chunks of 1024, each staging 3071 input samples in LDS,
 * the float64 sums staying in registers, so no RIR length changes the LDS plan.  A target term that equals mixture term s in all six fields is
 * computed once.  The kernel clamps the RIR index (negative = none, above R - 1 = R - 1), taps to 1 .. min(len_r, 16384), every RIR read into
 * [0, rir_total), and the utterance index, the start and every corpus read as sepr_dynmix_fwd does: a bad table yields wrong samples but never a
 * read outside the buffers.  SEPR_EINVAL before any HIP call for everything sepr_dynmix_fwd refuses, a null term_rir, term_taps, rir or
 * rir_off, R < 1, rir_total < 1 or a misaligned rir.  No workspace, no host synchronisation or allocation (capturable: the pointers are
 * frozen, the table contents - RIR indices and tap counts included - are read at replay).
 *
 * sepr_dynmix_speed_reverb_fwd: both inside one launch, the talker first and the room second.  The arguments are the common
 * ones, the three columns term_conv, term_rir, term_taps [B (M + S)] int32 (DEVICE), the converter set of sepr_dynmix_speed_fwd (0 <= NC <= 16)
 * and the bank arguments of sepr_dynmix_reverb_fwd.  A term is (utt, start, norm, gain, conv, rir, taps).  With conv >= 0 and rir >= 0, x the stored
 * utterance of T samples and (L, M, K) the converter:
 *   y    the perturbed utterance of P = sepr_resample_out_len(T, L, M) samples; y[n] is exactly sepr_dynmix_speed_fwd's / sepr_resample_fwd's float32
 *        sample (exact float64 products, j = 0 .. K - 1 in order, one rounding, x zero outside [0, T) of THAT utterance);
 *   z[t] = float32(sum_{j = 0 .. taps - 1} double(h_rir[j]) * double(y[term_start + t - j])),   y ZERO outside [0, P) - not the converter evaluated
 *        at negative positions, where it would ring - the products exact in float64, added as fma(h, y, acc) in the order j = 0 .. taps - 1 from
 *        acc = 0.0, one rounding;
 * the term's value is (z[t] * term_norm) * term_gain, the two separately rounded float32 multiplies.  term_start indexes the perturbed utterance; the
 * caller guarantees term_start + n[b] <= P.  So the term is "convert the whole utterance, convolve, truncate to P, crop" bit for bit; conv = -1 gives
 * sepr_dynmix_reverb_fwd's bits, rir = -1 sepr_dynmix_speed_fwd's, both -1 sepr_dynmix_fwd's, and h = [1.0] sepr_dynmix_speed_fwd's (a perturbed
 * sample that is -0.0 comes out +0.0).  Per workgroup of 2048 outputs and chunk of kc <= 1024 taps, the 2048 + kc - 1 perturbed samples the chunk
 * reaches (fewer at the utterance's beginning and in the last tile of an example) are converted into LDS as doubles, in passes whose input span fits
 * 3072 samples, and the FIR sums stay in registers across chunks; 57344 bytes of LDS whatever the response's length.  A target term that equals
 * mixture term s in all seven fields is computed once.  The kernel clamps conv, rir, taps, the utterance index, the start and every read position as
 * the two entries do: a bad table yields wrong samples but never a read outside the corpus, the bank or a tap table.  SEPR_EINVAL before any HIP
 * call for everything sepr_dynmix_speed_fwd or sepr_dynmix_reverb_fwd refuses (a converter whose 2048-output span exceeds 3072 samples included).
 * No workspace, no host synchronisation or allocation (capturable: the pointers and the converter descriptions are frozen, the table contents are
 * read at replay).  A new entry, no struct change: ABI 4.13.
 *
 * sepr_dynmix_turns_fwd: turn-taking - partially overlapped talkers - inside the one launch.  The arguments of
 * sepr_dynmix_speed_reverb_fwd, two more columns term_on, term_off [B (M + S)] int32 (DEVICE) and the table ramp [RL] float32 (DEVICE, 4-byte aligned),
 * 0 <= RL <= 4096, which the host makes as ramp[i] = float32(0.5 - 0.5 cos(pi (i + 0.5) / RL)) in float64; RL = 0 is a hard gate.  A term is
 * (utt, start, norm, gain, conv, rir, taps, on, off): [on, off) is its TURN in output samples of the example; either end may lie outside [0, n).  For
 * any integer t, negative ones included, with d = t - on and e = off - 1 - t,
 *   w(t) = 0                    if d < 0 or e < 0
 *        = ramp[min(d, e)]      if min(d, e) < RL
 *        = 1                    otherwise.
 * The gate acts on the talker's float32 signal y - the stored utterance, or the perturbed one when conv >= 0 - at index p = start + t, BEFORE any response:
 *   g[p] = +0.0f                            where w(p - start) == 0   (a selection, not a product: never -0.0)
 *        = float32(y[p] * w(p - start))     elsewhere (one float32 multiply),
 * and the term is exactly what the forms above make of g in place of y: (g[start + t] * norm) * gain without a response,
 * float32(sum_{j < taps} double(h[j]) * double(g[start + t - j])) and then the two multiplies with one.  The history before the crop (t - j < 0) is gated
 * by the same w: a talker whose turn began before the window keeps their tail, one who starts inside it has silence behind them, and the room rings on
 * after `off`, in the mixture and in the target alike - the talker stops, the room does not.  on and off are only compared and subtracted; the kernel
 * clamps both to [-2^30, 2^30], so a term with (on, off) = (-2^30, 2^30) has w = 1 wherever it can be evaluated and - x * 1.0f being x - carries the bits
 * of sepr_dynmix_speed_reverb_fwd, hence of every entry above.  One entry covers every kind of term: conv < 0 = no converter (NC = 0 allowed), rir < 0 = no
 * response, and R = 0 (rir, rir_off may then be NULL) makes every rir none.  A target term that equals mixture term s in all nine fields is computed
 * once.  A tile of 2048 outputs that lies past off + K - 1 (K = the clamped taps, 1 without a response) or ends at or before on is exactly +0 raw samples
 * and skips its loads, its conversion and its tap chunks, as does a single tap chunk that reaches only closed samples; the two multiplies still act on
 * the zeros.  Every clamp of sepr_dynmix_speed_reverb_fwd holds; the ramp index is below RL by construction.  SEPR_EINVAL before any HIP call for RL < 0,
 * RL > 4096, a null ramp with RL > 0, a misaligned ramp, a null term_on or term_off, R < 0, and everything sepr_dynmix_speed_reverb_fwd refuses (its
 * bank checks for R >= 1).  57344 bytes of LDS, no workspace, no host synchronisation or allocation (capturable).  A new entry, no struct change: ABI 4.13. */
size_t sepr_corpus_energy_workspace(int N);
int sepr_corpus_energy(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N,
                       long long* ss16, double* ss32, void* ws, size_t ws_bytes, sepr_stream_t stream);
int sepr_dynmix_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N,
                    const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain, const int* n, int B, int M,
                    int S, int Tmax, float* mix, float* const* src, sepr_stream_t stream);
int sepr_dynmix_speed_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N,
                          const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain, const int* term_conv,
                          const int* n, int B, int M, int S, int Tmax, float* mix, float* const* src, const float* const* conv_taps,
                          const int* conv_L, const int* conv_M, const int* conv_K, int NC, sepr_stream_t stream);
int sepr_dynmix_reverb_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N,
                           const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain, const int* term_rir,
                           const int* term_taps, const int* n, int B, int M, int S, int Tmax, float* mix, float* const* src, const float* rir,
                           long long rir_total, const long long* rir_off, int R, sepr_stream_t stream);
int sepr_dynmix_speed_reverb_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16,
                                 int N, const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain,
                                 const int* term_conv, const int* term_rir, const int* term_taps, const int* n, int B, int M, int S, int Tmax,
                                 float* mix, float* const* src, const float* const* conv_taps, const int* conv_L, const int* conv_M,
                                 const int* conv_K, int NC, const float* rir, long long rir_total, const long long* rir_off, int R,
                                 sepr_stream_t stream);
int sepr_dynmix_turns_fwd(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16, int N,
                          const int* term_utt, const int* term_start, const float* term_norm, const float* term_gain, const int* term_conv,
                          const int* term_rir, const int* term_taps, const int* term_on, const int* term_off, const int* n, int B, int M, int S,
                          int Tmax, float* mix, float* const* src, const float* const* conv_taps, const int* conv_L, const int* conv_M,
                          const int* conv_K, int NC, const float* rir, long long rir_total, const long long* rir_off, int R, const float* ramp,
                          int RL, sepr_stream_t stream);

/* ---- room impulse responses by the image-source method (a new entry, no struct change: ABI 4.13) -------
 * sepr_rir_ism_fwd simulates R impulse responses of N samples, one per shoebox room, in one call.  The definition is independent of the
 * order of summation and bit-reproducible in numpy (tests/rirsim_ref.py):
 *   constants   HW = 40 (a pulse has TW = 2 HW + 1 = 81 taps), Q = 32 fractional steps, FB = 48 fixed-point fraction bits,
 *               FOURPI = float64(4 pi).
 *   lut         [Q + 1][TW] float64 (DEVICE), built by the host: lut[k][j] = sinc(x) 0.5 (1 + cos(pi x / (HW + 1))), x = (j - HW) - k / Q,
 *               zero for |x| > HW + 1.  The entry reads the table it is given; it does not compute one.
 *   rooms       [R][10] float64 (DEVICE): Lx Ly Lz sx sy sz mx my mz beta - the room, an omnidirectional source s and microphone m, one
 *               reflection coefficient beta in [0, 1) for all six walls.  fsc = fs / c (samples per metre), computed by the caller.
 *   images      per axis, for an integer k and a parity p in {0, 1}: offset = fl(fl(k (2 L)) + c_p) with c_0 = fl(s - m), c_1 = -fl(s + m)
 *               (the image 2 k L + (1 - 2 p) s seen from m, written so that exchanging s and m negates or keeps every offset exactly), and
 *               n = |2 k - p| reflections.
 *   per image   float64, every operation rounded separately (no contraction): d = sqrt((dx dx + dy dy) + dz dz), tau = d fsc,
 *               i0 = floor(tau), a = bpow[nx + ny + nz] / (FOURPI d) with bpow[0] = 1, bpow[n] = bpow[n - 1] beta (a sequential product).
 *               The image belongs to the response iff i0 - HW <= N - 1.
 *   taps        for j = 0 .. TW - 1 and t = i0 - HW + j in [0, N): f = tau - i0, k = floor(f Q), w = f Q - k,
 *               v = lut[k][j] + w (lut[k + 1][j] - lut[k][j]); the tap adds the INTEGER rint((a v) 2^48) (half to even) to acc[r][t].
 *   output      acc [R][N] int64 (DEVICE, the caller's workspace, zeroed by the entry and left holding the sums); h = acc / 2^48 (exact);
 *               rir [R][N] float32 (DEVICE) = float32(h / max|h_r|) with normalise = 1 (an all-zero response stays zero), float32(h) with
 *               normalise = 0; peak_idx [R] int32 (DEVICE) = the first index of the maximum of |h_r|.
 * Integer addition commutes, so the kernel's decomposition (tiles of 256 samples, 8 column splits per tile, 64-bit LDS and global atomic adds)
 * does not show in the result: two calls give equal bits.  SEPR_EINVAL before any HIP call: a null pointer, R outside 1 .. 65535, N outside
 * 1 .. 16384, normalise other than 0 or 1, fsc not positive and finite, sqrt(3) (N + HW + 1) / fsc / 1.5 + 3 >= 1024 (the table of powers of
 * beta, bounded for the smallest room dimension the contract allows, 1.5 m), rooms, lut or acc not 8-byte aligned, rir or peak_idx not 4-byte
 * aligned.  What the entry cannot see - the rooms are device memory - is the caller's to check (reverb.validate_rooms: every dimension
 * >= 1.5 m, source and microphone >= 0.1 m from every wall and from each other, 0 <= beta < 1); the kernel clamps the room sizes to
 * [1.5, 1e6], the positions into the room, beta to [0, 1] and every derived index, so a bad table gives wrong samples and bounded work but
 * never an access outside acc, rir, lut or its LDS arrays.  No host synchronisation or allocation (capturable). */
int sepr_rir_ism_fwd(const double* rooms, int R, int N, double fsc, const double* lut, long long* acc, float* rir, int* peak_idx, int normalise,
                     sepr_stream_t stream);

/* ---- conversations rendered and scored on the device (new entries, no struct change: ABI 4.13) ------------
 * A conversation is a schedule of G_r >= 1 segments on S_r <= S_max talker tracks, laid along n_r output samples (a multiple of 4).  Segment g
 * is (seg_utt, seg_start, seg_place, seg_len, seg_norm, seg_gain): sample seg_start + d of the utterance lands on output sample seg_place + d
 * for 0 <= d < seg_len.  The segments of all R conversations lie in one table of G rows sorted by (conversation, track, place);
 * track_off [R S_max + 1] int32 holds the cumulative segment counts per (conversation, track) - a track without a segment has an empty range -
 * and out_off [R + 1] int64 the first flat output sample of each conversation (multiples of 4, out_off[R] = total).  The segments of one track do
 * not overlap.  All eight tables are DEVICE memory; the corpus is described exactly as for sepr_dynmix_fwd.  A segment may begin before output
 * sample 0 or end after n_r (seg_place >= -2^30; section 5e-8: a window cut out of a longer schedule): both render entries then make the part
 * of it - and, in rooms, of its tail - that falls inside [0, n_r); every search and walk compares values only and stores are bounded by total.
 *
 * sepr_conversation_render: one launch renders every conversation.  With x the utterance's sample value (an int16 sample is s / 32768),
 *   track_s[t] = (x[seg_start + t - seg_place] * seg_norm) * seg_gain  for the one segment of track s that covers t, else +0.0   (two separately
 *                rounded float32 multiplies, never contracted: the arithmetic of sepr_dynmix_fwd)
 *   mix[t]     = ((0 + track_0[t]) + track_1[t]) + ... over the S_max tracks in track order
 * mix [total] float32, conversation r at out_off[r]; tracks [S_max][total] float32 or NULL, which skips the track rows; both 16-byte aligned.
 * The kernel is tiled over the flat output samples: a tile finds its conversation and each track's first live segment by binary search over
 * seg_place; a segment that covers the four samples of a thread is read with aligned vector loads and realigned in registers, its first and last
 * samples one at a time.  The call cannot validate the tables: the kernel clamps every track range into [0, G], the utterance index, the start
 * and every read position as sepr_dynmix_fwd does, and stores at flat samples below total only, so a bad table gives wrong samples but never an
 * access outside the corpus buffers, the tables or the outputs.  SEPR_EINVAL before any HIP call for a null pointer (tracks excepted),
 * R < 1 or R > 65535, S_max outside 1..8, G < 1, total < 4, not a multiple of 4 or above 2^40, a misaligned buffer or an inconsistent corpus
 * description.  No workspace, no host synchronisation or allocation (capturable: the pointers are frozen, the tables are read at replay).
 *
 * sepr_segment_sisnr_fwd: the SI-SNR of every output channel, and of the mixture, against every segment.  est [C][ld], ref [S][ld], mix [ld]
 * float32 with T <= ld valid samples per row; rows, begin, length [G] int32 (DEVICE): segment g is r = ref[rows[g]][begin[g] .. begin[g] +
 * length[g]) and a signal a is the same span of an est row or of mix.  In float64 (a float32 value is exact in it), with n = length[g]:
 *   a~ = a - (sum a) / n,   r~ = r - (sum r) / n,   s_rr = sum r~^2,   s_ar = sum a~ r~,   alpha = s_ar / (s_rr + eps)
 *   value = 20 log10(eps + |alpha| sqrt(s_rr) / (sqrt(sum (a~ - alpha r~)^2) + eps))
 * - the per-pair term of PIT_SISNRi over the segment.  The residual is summed DIRECTLY, in a pass after alpha is known, not formed from raw or
 * centred moments, so the relative error of both norms does not depend on the SNR or on a DC offset.  v [G][C] float64 = the value of est
 * row c, v_mix [G] float64 = the value of mix.  Every sum runs in a fixed order - thread i of 256 adds the samples i, i + 256, ..., a wave adds
 * its lanes by butterfly, the four wave sums are added in wave order - with no atomics: bit-identical from run to run.  The grids are G and
 * (G, C + 1) workgroups.  The kernels clamp rows[g] into [0, S), begin[g] into [0, T] and length[g] into [0, T - begin[g]] (an empty segment gives
 * 20 log10(eps)).  Workspace: sepr_segment_sisnr_bytes(G, C) bytes (0 for G < 1 or C outside 1..8).  SEPR_EINVAL before any HIP call for a null
 * pointer, G < 1, C or S outside 1..8, T < 1, ld < T, eps outside [0, 1], est, ref or mix not 4-byte aligned, v or v_mix not 8-byte aligned;
 * SEPR_EWORKSPACE for a short workspace.  No host synchronisation or allocation (capturable).
 *
 * sepr_conversation_render_rooms: conversations in rooms (a new entry, no struct change: ABI 4.13).  A segment gains three
 * int32 fields, seg_rir, seg_taps, seg_direct [G] (DEVICE).  rir = -1 means no response and stands for h = [1.0], taps = direct = 1; rir = r >= 0
 * names response h_r of the bank of sepr_dynmix_reverb_fwd (rir [rir_total] float32, rir_off [NR + 1] int64, DEVICE), with
 * 1 <= direct <= taps <= len_r <= 16384.  With x the utterance's float32 sample value (an int16 sample is s / 32768), for a segment g:
 *   x_g[d]   = x[seg_start + d] for 0 <= d < seg_len, +0 for every other integer d: zero outside the SEGMENT, not outside the utterance - a cut
 *              utterance does not ring with samples that were never played;
 *   z_g^K[t] = float32(sum_{j = 0 .. K - 1} double(h[j]) * double(x_g[t - seg_place - j])), the products exact in float64, added as fma(h, x, acc) in
 *              the order j = 0 .. K - 1 from acc = 0.0, one rounding: the arithmetic of sepr_dynmix_reverb_fwd;
 *   v_g^K[t] = (z_g^K[t] * seg_norm) * seg_gain, the two separately rounded float32 multiplies, never contracted, on the support
 *              seg_place <= t < min(n, seg_place + seg_len + K - 1): the tail runs past the segment's end and is cut only by the conversation's;
 *   wet_s[t] = ((+0.0 + v_a^taps[t]) + v_b^taps[t]) + ... over the segments of track s whose support holds t, in table order (by place), in float32.
 *              Several segments can contribute to one sample - a tail under the next turns of the same track.  A running sum that starts at +0.0 is
 *              never -0.0, so leaving out a segment that contributes a zero is exact, and the kernel skips whatever reaches only silence;
 *   tracks_s[t] the same sum with K = direct_g: the scoring reference, aligned in time with the mixture (the mixing launch's target = "direct");
 *   mix[t]   = ((+0.0 + wet_0[t]) + wet_1[t]) + ... over the S_max tracks in order.
 * So with every rir = -1, mix and tracks are sepr_conversation_render's on the same table, except that a track sample that is -0.0 there comes
 * out +0.0 here (as a perturbed -0.0 does in section 5e-5); a unit impulse h = [1.0] gives the bits of rir = -1; and a response [0, .., 0, 1.0] of
 * k + 1 taps gives the dry track delayed by k samples and cut at n.  A noise bed needs nothing of the kernel: it is one more track after the talkers,
 * its segments rir = -1, summed into mix last because it is the last track.
 * Arguments: sepr_conversation_render's up to seg_gain, the three columns, sepr_conversation_render's from track_off to tracks, the bank (NR >= 0
 * responses; NR = 0 with NULL bank pointers makes every segment response-free), the stream.  The kernel makes tiles of 2048 flat output samples; a
 * tile in which conversations meet makes the piece of each in turn, so no piece mixes two.  Per piece and track it finds the segments whose support
 * can reach the piece - binary search over seg_place, then back while place + len + 16383 lies past the piece's start - and adds them in table
 * order, each by the FIR plan of the mixing launch (taps in ascending chunks of 1024, the chunk's span staged in LDS as doubles, the float64 sums in
 * registers across chunks; a thread owns eight consecutive outputs and slides a window of staged samples through its registers; the sum after
 * `direct` taps is a prefix of the same sequence and is kept on the way).  A (track, piece) that no support
 * reaches is zeros with nothing staged, and a tap chunk that reaches no sample of the segment is skipped.  The decomposition does not show in the
 * result, there are no atomics, and two calls give equal bits.  The tables are device memory, so the kernel clamps: the response index (negative =
 * none, above NR - 1 = NR - 1), taps to 1 .. min(len_r, 16384), direct to 1 .. taps, every bank read into [0, rir_total), and everything
 * sepr_conversation_render clamps; stores go below total only.  A bad table gives wrong samples and bounded work, never an access outside a buffer.
 * SEPR_EINVAL before any HIP call for everything sepr_conversation_render refuses, a null column, NR < 0, and with NR > 0 what
 * sepr_dynmix_reverb_fwd refuses of a bank (a null rir or rir_off, rir_total < 1, a misaligned rir) or a rir_off that is not 8-byte aligned.
 * 38912 bytes of LDS, no workspace, no host synchronisation or allocation (capturable: the pointers are frozen, the tables are read at replay). */
int sepr_conversation_render_rooms(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16,
                                   int N, const int* seg_utt, const int* seg_start, const int* seg_place, const int* seg_len,
                                   const float* seg_norm, const float* seg_gain, const int* seg_rir, const int* seg_taps, const int* seg_direct,
                                   const int* track_off, const long long* out_off, int R, int S_max, int G, long long total, float* mix,
                                   float* tracks, const float* rir, long long rir_total, const long long* rir_off, int NR, sepr_stream_t stream);
int sepr_conversation_render(const short* buf16, long long total16, const float* buf32, long long total32, const long long* offsets, int N16,
                             int N, const int* seg_utt, const int* seg_start, const int* seg_place, const int* seg_len, const float* seg_norm,
                             const float* seg_gain, const int* track_off, const long long* out_off, int R, int S_max, int G, long long total,
                             float* mix, float* tracks, sepr_stream_t stream);
long long sepr_segment_sisnr_bytes(int G, int C);   /* (long long: the size_t entries are the workspace sizes of the older entries) */
int sepr_segment_sisnr_fwd(const float* est, const float* ref, const float* mix, const int* rows, const int* begin, const int* length, int G,
                           int C, int S, int T, long long ld, double eps, double* v, double* v_mix, void* ws, size_t ws_bytes,
                           sepr_stream_t stream);

/* ---- frame activity: what a channel emits when none of its talkers speaks (new entries, no struct change: ABI 4.13) ----
 * sepr_frame_energy_fwd: x [rows][ld] float32 with T <= ld valid samples per row (rows may be views with the common row stride ld); frame a multiple
 * of 4 in 32..4096; nF = ceil(T / frame), the last frame holding the 1..frame samples that are left.  e [rows][nF] float64 = the sum of x^2 over the
 * frame; the square of a float32 value is exact in float64, so only the additions round.  One wave per (row, frame), in this order: lane l of 64
 * starts from +0.0 and adds the squares of the samples 4 q, 4 q + 1, 4 q + 2, 4 q + 3 of the frame for q = l, l + 64, l + 128, ..., in ascending
 * order, leaving out those at or past the frame's end; then the lanes are added by butterfly - for o = 32, 16, 8, 4, 2, 1 every lane adds the value of
 * lane l ^ o to its own - and lane 0 stores.  One launch for all rows (frames by fours on grid.x, rows on grid.y).  Where x is 16-byte aligned and ld
 * a multiple of 4 four samples are one load; the additions are the same either way.  Zero samples behind a recording add +0.0 and change no bit, so
 * recordings laid out on frame boundaries in one buffer give the frames each gives alone.  SEPR_EINVAL before any HIP call for a null pointer, rows
 * outside 1..65535, T < 1 or above 2^36, ld < T, a frame that is no multiple of 4 in 32..4096, x not 4-byte or e not 8-byte aligned.
 *
 * sepr_frame_activity_fwd: e [rows][nF] float64 (contiguous).  Per row: level[row] = the maximum of e[f] + 0.0 over the frames, a NaN never taken
 * (-infinity when every frame is NaN) - a maximum does not depend on the order, and + 0.0 gives a zero one sign; t = level * ratio, one float64
 * multiply, and thr = t > floor ? t : floor; raw[f] = e[f] > thr, strictly, so an all-zero row is inactive everywhere and a NaN frame is inactive;
 * active [rows][nF] uint8 = 1 where raw[f'] holds for some f' in the row with |f' - f| <= hang, else 0.  The caller passes ratio = 10^(ratio_db / 10)
 * as a double: the device calls no pow, and a host restatement has the same threshold.  hang = 0 (no widening) and hang >= nF (a row with one raw
 * frame is active everywhere) are both legal.  Two launches: a workgroup per row finds level and counts raw into the workspace, cnt[row][f + 1] =
 * #{f' <= f : raw[f']} in int32; a thread per frame then tests cnt[min(nF, f + hang + 1)] - cnt[max(0, f - hang)] > 0.  Integers only after the
 * compare.  Workspace: sepr_frame_activity_bytes(rows, nF) bytes (0 for rows outside 1..65535 or nF outside 1..2^30).  SEPR_EINVAL before any HIP
 * call for a null e, active or level, rows or nF outside those ranges, hang < 0, a ratio or floor that is negative, infinite or NaN, e or level not
 * 8-byte aligned; SEPR_EWORKSPACE for a short or null workspace.
 *
 * sepr_frame_class_sums_fwd: e_est [C][nF] and e_mix [nF] float64, active [C][nF] and cls [C][nF] uint8 (DEVICE, read at replay); a class byte is
 * used as cls & 3.  out [C][4][4] float64: for channel c and class k, over the frames f with (cls[c][f] & 3) == k: out[c][k][0] = their number,
 * [1] = the number of them with active[c][f] != 0, [2] = the sum of e_est[c][f], [3] = the sum of e_mix[f].  The grid is (C, 4) workgroups of 256
 * threads, in the form of segsnr_value_kernel: thread i starts from +0.0 and takes the frames i, i + 256, ... in order, adding only those of its class;
 * a wave adds its lanes by the butterfly above; the four wave sums are added ((w0 + w1) + w2) + w3.  The counts are sums of ones in the same order:
 * exact below 2^53.  The workspace, sepr_frame_class_sums_bytes(C, nF) bytes (0 for C outside 1..8 or nF outside 1..2^30), keeps the wave sums,
 * part [C][4][4][4] float64 with the wave last, so that a restatement can be compared stage by stage.  SEPR_EINVAL before any HIP call for a null
 * pointer, C or nF outside those ranges, e_est, e_mix or out not 8-byte aligned; SEPR_EWORKSPACE for a short or null workspace.
 * All three: no atomics, two calls give equal bits, no host synchronisation or allocation (capturable: the pointers are frozen, the tables are read
 * at replay). */
int sepr_frame_energy_fwd(const float* x, int rows, long long T, long long ld, int frame, double* e, sepr_stream_t stream);
long long sepr_frame_activity_bytes(int rows, int nF);
int sepr_frame_activity_fwd(const double* e, int rows, int nF, double ratio, double floor, int hang, unsigned char* active, double* level, void* ws,
                            size_t ws_bytes, sepr_stream_t stream);
long long sepr_frame_class_sums_bytes(int C, int nF);
int sepr_frame_class_sums_fwd(const double* e_est, const double* e_mix, const unsigned char* active, const unsigned char* cls, int C, int nF,
                              double* out, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* ---- Graph-PIT: assignment of the target rows of a conversation window to output channels (new entries, no struct
 * change: ABI 4.13) -----------------------------------------------------------------------------------------------------------------------------
 * A window holds U <= 8 target rows - one per utterance heard in it - for a separator of C <= 3 output channels; plain PIT has no answer to
 * "which row goes on which channel" when U != C.  Graph-PIT (von Neumann et al., 2021): every row is a node, rows that may not share a channel are
 * joined by an edge, a valid assignment is a colouring col: u -> c of that graph with C colours, and the loss is the minimum over the valid
 * colourings.  est and rows are HOST arrays of C and U device pointers, each to a [B][T] float32 tensor, read at the call and frozen in a captured
 * launch; spans [B][U][2] int32 and adj [B][U] uint32 are DEVICE tables, read at replay.  Row u of example b is t_u, ZERO outside its span
 * [on, off) = (spans[b][u][0], spans[b][u][1]) whatever the buffer holds there: the kernels never read a row outside its span, clamped as on into
 * [0, T] and off into [on, T].  An empty span makes a silent row: it is no node - always coloured 0, not enumerated, its adjacency bits ignored.
 * Bit v of adj[b][u] says rows u and v may not share a channel; an edge named by either side counts, bits at or above U and a row's own bit do not.
 *
 * All arithmetic is float64 on exact float32 inputs; ~ is zero-mean over all T samples, as in sepr_pit_sasdr_fwd.  The moments of example b:
 *   se_c = sum e_c, ee_c = sum e_c^2 over T;   st_u = sum t_u, tt_u = sum t_u^2, et_cu = sum e_c t_u over the span of u;
 *   tv_uv = sum t_u t_v over the intersection of the spans of u and v (0 when empty) - rows of one colour may overlap, so the Gram term is exact.
 * For a colouring, with the rows of a colour taken in ascending order and the pairs in lexicographic order:
 *   Sy_c = sum_{u in c} st_u,   yy_c = sum_{u in c} tt_u + 2 sum_{u < v in c} tv_uv - Sy_c^2 / T,   ee~_c = ee_c - se_c^2 / T,
 *   ey_c = sum_{u in c} et_cu - se_c Sy_c / T,   E = max(0, sum_c ((ee~_c - 2 ey_c) + yy_c)),   D = sum_c yy_c.
 * sepr_graph_pit_assign: col [B][U] int32 = the first minimiser of E over the valid colourings in lexicographic order of (col(0), .., col(U - 1));
 * value [B] float64 = 10 log10((E + tau D + eps) / (D + eps)), tau = 10^(-snr_max / 10): for U = C rows over all T, every pair adjacent, it is
 * sepr_pit_sasdr_fwd's loss; status [B] int32 = 0.  Where no valid colouring exists status = 1, col = 0 and value = NaN.  Two launches: one
 * workgroup per (example, moment) - thread i of 256 adds the samples i, i + 256, ... of the interval, a wave adds its lanes by butterfly, the four
 * wave sums are added in wave order, an empty interval stores 0 at once - into the workspace; then one workgroup per example evaluates the at most
 * 3^8 colourings, whole, from the moment tables in LDS, thread i the colourings i, i + 256, ..., and reduces the minimum and its first index in a
 * fixed order.  Workspace: sepr_graph_pit_bytes(C, U, B) bytes (0 for unsupported C, U, B).
 * sepr_graph_pit_assemble: out_c[b][t] = ((+0.0 + t_u1[t]) + t_u2[t]) + ... over the rows of colour c in ascending u - float32 adds, never
 * contracted; a row is skipped outside its span, which changes no bit of a sum that began at +0.0.  out is a HOST array of C device pointers to
 * [B][T] tensors; col is read at replay and clamped into [0, C).  One thread per four samples: a row that covers them is read with one aligned
 * 16-byte load, one that covers some of them element by element under the span's mask - a span that starts at an odd sample causes no misaligned
 * load -; one float4 store per thread and channel.
 * Both: no atomics, results bit-identical from run to run; no host synchronisation or allocation (capturable); every table value is clamped, so a
 * bad table gives wrong values but never an access outside a buffer.  SEPR_EINVAL before any HIP call for a null pointer (in the arrays too),
 * C outside 1..3, U outside 1..8, B outside 1..65535, T < 4 or not a multiple of 4, eps outside [0, 1], snr_max outside [0, 300], an est pointer
 * or table that is not 4-byte aligned, value not 8-byte aligned, and in assemble a row or out pointer that is not 16-byte aligned;
 * SEPR_EWORKSPACE for a short workspace. */
long long sepr_graph_pit_bytes(int C, int U, int B);
int sepr_graph_pit_assign(const float* const* est, const float* const* rows, const int* spans, const unsigned* adj, int C, int U, int B, int T,
                          double eps, double snr_max, int* col, double* value, int* status, void* ws, size_t ws_bytes, sepr_stream_t stream);
int sepr_graph_pit_assemble(const float* const* rows, const int* spans, const int* col, int C, int U, int B, int T, float* const* out,
                            sepr_stream_t stream);

/* ================================================================================================================= */
/* Training path: train-mode forward twins that keep what the backward needs, and the       */
/* backward of every block.  The reference trains through torch.autograd over the same modules (engine.py:50-83:     */
/* data_parallel forward, PIT losses, backward, clip_grad_norm_, AdamW); here each block has an explicit backward.   */
/*                                                                                                                   */
/* Conventions (in addition to the ones at the top of this header)                                                   */
/*   - a block's train_fwd writes its saved-for-backward tensors into a caller-provided context buffer `ctx` of       */
/*     sepr_train_ctx_bytes(op, ...) bytes; the matching _bwd reads the same buffer (the caller keeps it and the      */
/*     block's input x alive in between); `ws` is scratch of sepr_train_ws_bytes(op, ...) bytes;                      */
/*   - parameter gradients are ACCUMULATED (+=) into fp32 buffers laid out exactly like the reference parameters      */
/*     (e.g. depthwise.weight [C,1,K]); the caller zeroes them once per step; activation gradients are overwritten;   */
/*   - a projection travels as sepr_lin: exact-f32 form (w: fp32 [N][K] row-major) or packed-bf16 form (wp: pack_x3    */
/*     fragments, hi and lo planes), never both; b may be NULL.  `planes` selects the arithmetic of the packed form:   */
/*     0 or 3 = bf16x3 (hi.hi + hi.lo + lo.hi, ~2^-16), 1 = plain bf16 operands (one MFMA per product, fp32           */
/*     accumulate: the "bf16" training precision of BASELINE configs[4]; activations are rounded to bf16 on the fly,   */
/*     the lo plane is ignored).  The host packs, per weight version, the forward form and the                         */
/*     transposed form the input gradient needs, with LayerNorm / GroupNorm affines and LayerScale folded in           */
/*     (sepreformer_amd/train_pack.py); the raw parameters ride along for the gradient finishers;                      */
/*   - train-mode BatchNorm uses batch statistics over (sequences x frames) and updates running_mean / running_var     */
/*     in place (momentum 0.1, unbiased variance), like torch.nn.BatchNorm1d (network.py:167, module.py:69);          */
/*   - dropout (network.py:55,57,87,121,124,171): inverted dropout from a counter-based generator keyed by             */
/*     (seed, element index); p_drop = 0 disables it exactly; the backward regenerates the masks from the same seed.  */
/*     (The fused GCFN pair - sepr_gcfn_train_fwd / sepr_gcfn_bwd with fused_w1p set - draws its two sites from a      */
/*     cheaper 16-bit-per-element generator, csrc/sepr_train.h sepr_drop_word: p is quantised to p_eff = round(p *     */
/*     65536) / 65536 and the kept values are scaled by 1 / (1 - p_eff).)                                             */
/* ================================================================================================================= */
typedef struct { const float* w; const void* wp; const float* b; int planes; } sepr_lin;
typedef unsigned long long sepr_u64;

/* GCFN, modules/network.py:46-66 */
typedef struct {
  sepr_lin up;      /* [6F,F]  net1.1.weight * ln_gamma, net1.1.bias + W . ln_beta */
  sepr_lin up_t;    /* [F,6F]  (net1.1.weight * ln_gamma)^T */
  sepr_lin down;    /* [F,3F]  net2.2 */
  sepr_lin down_t;  /* [3F,F]  (layer_scale * net2.2.weight)^T */
  const float* dw_w; /* [3,6F] tap-major */
  const float* dw_b; /* [6F] */
  const float* ls;   /* [F] */
  const float* w1; const float* ln_g; const float* ln_b; const float* w2; const float* b2;   /* raw parameters */
  /* Optional fused form (F in {64, 128}; train_pack.py): the forward is then ONE launch of the fused inference kernel
   * (sepr_gcfn_fwd's, with both dropout sites and a LayerNorm-statistics side output) that keeps only the per-row
   * statistics, and the backward recomputes the hidden tensor inside its middle kernel (csrc/sepr_gcfn_bwd_fused.hip).
   * fused_w1p / fused_w2p exactly as in sepr_gcfn_w.  NULL fused_w1p = the unfused path. */
  const void* fused_w1p; const void* fused_w2p;
  const sepr_u64* seed_salt;   /* optional device word XOR-ed into `seed` by every dropout kernel of the call (hipGraph replay) */
} sepr_gcfn_tw;
typedef struct { float* ln_g; float* ln_b; float* w1; float* b1; float* dw_w; float* dw_b; float* w2; float* b2; float* ls; } sepr_gcfn_grad;

/* CLA, modules/network.py:159-187 (BatchNorm NOT folded: batch statistics) */
typedef struct {
  sepr_lin l1, l1_t;   /* [2F,F] linear1 * ln_gamma (+ beta in the bias); [F,2F] transpose */
  const float* dw_w;   /* [K,F] tap-major */
  const float* dw_wf;  /* [K,F] tap-major, taps reversed (input gradient of the 'same' conv) */
  const float* dw_b;   /* [F] */
  const float* zeros;  /* [>= 2F] zeros */
  sepr_lin l2, l2_t;   /* [2F,F] linear2; [F,2F] linear2^T */
  const float* bn_g; const float* bn_b; float* bn_rm; float* bn_rv;   /* BN affine; running stats (updated in place) */
  sepr_lin l3, l3_t;   /* [F,2F] linear3.1; [2F,F] (layer_scale * linear3.1.weight)^T */
  const float* ls;
  const float* w1; const float* ln_g; const float* ln_b; const float* w3; const float* b3;   /* raw parameters */
  const sepr_u64* seed_salt;   /* as in sepr_gcfn_tw */
} sepr_cla_tw;
typedef struct { float* ln_g; float* ln_b; float* w1; float* b1; float* dw_w; float* dw_b; float* w2; float* b2; float* bn_g; float* bn_b;
                 float* w3; float* b3; float* ls; } sepr_cla_grad;

/* MultiHeadAttention, modules/network.py:69-124 */
typedef struct {
  sepr_lin qkv, qkv_t;  /* [3F,F] stacked q/k/v * ln_gamma; [F,3F] transpose */
  sepr_lin out, out_t;  /* [F,F] linear_out; (layer_scale * linear_out.weight)^T */
  const float* ls;
  const float* wqkv; const float* ln_g; const float* ln_b; const float* wo; const float* bo;   /* raw (wqkv stacked [3F,F]) */
  const sepr_u64* seed_salt;   /* as in the GCFN struct; for EGA the attention struct carries it for the whole block */
} sepr_mha_tw;
typedef struct { float* ln_g; float* ln_b; float* wq; float* bq; float* wk; float* bk; float* wv; float* bv; float* wo; float* bo; float* ls; } sepr_mha_grad;

/* EGA, modules/network.py:126-155 */
typedef struct {
  sepr_mha_tw attn;
  sepr_lin gate, gate_t;  /* [F,F] block.linear.1 * gamma; transpose */
  const float* gate_w; const float* gate_ln_g; const float* gate_ln_b;   /* raw */
  const float* pe_k; int maxlen;
} sepr_ega_tw;
typedef struct { sepr_mha_grad attn; float* gate_ln_g; float* gate_ln_b; float* gate_w; float* gate_b; float* pe_k; } sepr_ega_grad;

/* DownConvLayer, modules/module.py:63-78 */
typedef struct { const float* w /* [K,F] tap-major */; const float* b; const float* bn_g; const float* bn_b; float* bn_rm; float* bn_rv; } sepr_down_tw;
typedef struct { float* w /* [F,1,K] */; float* b; float* bn_g; float* bn_b; } sepr_down_grad;

/* SpkSplitStage, modules/module.py:110-125 */
typedef struct { sepr_lin l1, l1_t, l2, l2_t; const float* gn_g; const float* gn_b; } sepr_split_tw;
typedef struct { float* w1; float* b1; float* w2; float* b2; float* gn_g; float* gn_b; } sepr_split_grad;

/* fusion conv, modules/module.py:187,212-214 */
typedef struct { sepr_lin l, l_t; } sepr_fuse_tw;
typedef struct { float* w; float* b; } sepr_fuse_grad;

/* OutputLayer + AudioDecoder, modules/module.py:237-283 */
typedef struct { sepr_lin l1, l1_t, l2, l2_t; const float* wdec /* [K,N] tap-major */; } sepr_out_tw;
typedef struct { float* w1; float* b1; float* w2; float* b2; float* wdec /* [N,1,K] */; } sepr_out_grad;

/* AudioEncoder + FeatureProjector, modules/module.py:12-35.  The projector runs on the exact-f32 core with the GroupNorm
 * affine in its prologue (as in inference: padded frames must come out exactly zero), only its input gradient uses a
 * folded, transposed form. */
typedef struct {
  const float* w_enc;      /* [K,N] tap-major */
  const float* proj_w;     /* [F,N] feature_projector.conv1d.weight */
  const float* gn_g; const float* gn_b;   /* [N] feature_projector.norm */
  sepr_lin proj_t;         /* [N,F] (conv1d.weight * gn_gamma)^T */
  const float* ones;       /* [>= N] ones */
} sepr_front_tw;
typedef struct { float* w_enc /* [N,1,K] */; float* gn_g; float* gn_b; float* proj_w; } sepr_front_grad;

enum { SEPR_TOP_GCFN = 0, SEPR_TOP_CLA, SEPR_TOP_EGA, SEPR_TOP_SPKATTN, SEPR_TOP_DOWN, SEPR_TOP_SPLIT, SEPR_TOP_FUSE, SEPR_TOP_OUT,
       SEPR_TOP_FRONT, SEPR_TOP_GCFN_FUSED /* sizes of the fused GCFN pair (sepr_gcfn_tw.fused_w1p != NULL) */,
       SEPR_TOP_EGA_X3 /* sizes of EGA when its attention runs on the bf16 MFMA (packed-bf16 precisions, dk 16 / 32) */,
       SEPR_TOP_GCFN_FUSED16 /* the fused GCFN pair in the plain-bf16 precision (sepr_lin.planes == 1): its context also keeps the
                                normalised rows as bf16 [n*T][F] for the plane-staged backward (ABI 3.02) */, SEPR_TOP_COUNT };
/* n sequences of T frames (Tp: pooled frames for EGA, source frames for OUT, padded frames Lp for FRONT), width F, encoder
 * channels N, S speakers, K = depthwise taps where the op has them (CLA 65, DOWN 5; else ignored). */
size_t sepr_train_ctx_bytes(int op, int n, int T, int Tp, int F, int N, int S, int H);
size_t sepr_train_ws_bytes(int op, int n, int T, int Tp, int F, int N, int S, int H, int K);

int sepr_gcfn_train_fwd(const float* x, float* y, int n, int T, int F, const sepr_gcfn_tw* w, void* ctx, size_t ctx_bytes, void* ws,
                        size_t ws_bytes, float p_drop, sepr_u64 seed, sepr_stream_t stream);
int sepr_gcfn_bwd(const float* x, const float* dy, float* dx, int n, int T, int F, const sepr_gcfn_tw* w, const sepr_gcfn_grad* g,
                  const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, float p_drop, sepr_u64 seed, sepr_stream_t stream);

int sepr_cla_train_fwd(const float* x, float* y, int n, int T, int F, int K, const sepr_cla_tw* w, void* ctx, size_t ctx_bytes, void* ws,
                       size_t ws_bytes, float p_drop, sepr_u64 seed, sepr_stream_t stream);
int sepr_cla_bwd(const float* x, const float* dy, float* dx, int n, int T, int F, int K, const sepr_cla_tw* w, const sepr_cla_grad* g,
                 const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, float p_drop, sepr_u64 seed, sepr_stream_t stream);

int sepr_ega_train_fwd(const float* x, float* y, int n, int T, int Tp, int F, int H, const sepr_ega_tw* w, void* ctx, size_t ctx_bytes,
                       void* ws, size_t ws_bytes, float p_drop, sepr_u64 seed, sepr_stream_t stream);
int sepr_ega_bwd(const float* x, const float* dy, float* dx, int n, int T, int Tp, int F, int H, const sepr_ega_tw* w,
                 const sepr_ega_grad* g, const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, float p_drop, sepr_u64 seed,
                 sepr_stream_t stream);

int sepr_spkattn_train_fwd(const float* x, float* y, int nS, int S, int T, int F, int H, const sepr_mha_tw* w, void* ctx,
                           size_t ctx_bytes, void* ws, size_t ws_bytes, float p_drop, sepr_u64 seed, sepr_stream_t stream);
int sepr_spkattn_bwd(const float* x, const float* dy, float* dx, int nS, int S, int T, int F, int H, const sepr_mha_tw* w,
                     const sepr_mha_grad* g, const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, float p_drop, sepr_u64 seed,
                     sepr_stream_t stream);

int sepr_downconv_train_fwd(const float* x, float* y, int n, int T, int F, int K, const sepr_down_tw* w, void* ctx, size_t ctx_bytes,
                            void* ws, size_t ws_bytes, sepr_stream_t stream);
int sepr_downconv_bwd(const float* x, const float* dy, float* dx, int n, int T, int F, int K, const sepr_down_tw* w,
                      const sepr_down_grad* g, const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, sepr_stream_t stream);

int sepr_spksplit_train_fwd(const float* x, float* y, int B, int S, int T, int F, float gn_eps, const sepr_split_tw* w, void* ctx,
                            size_t ctx_bytes, void* ws, size_t ws_bytes, sepr_stream_t stream);
/* dx_accumulate != 0: dx += (the skip tensors are also read by the DownConv of their stage) */
int sepr_spksplit_bwd(const float* x, const float* dy, float* dx, int dx_accumulate, int B, int S, int T, int F, const sepr_split_tw* w,
                      const sepr_split_grad* g, const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* forward is sepr_fuse_fwd with w->l; backward: dlo [n,T/2,F], dskip [n,T,F] */
int sepr_fuse_bwd(const float* lo, const float* skip, const float* dy, float* dlo, float* dskip, int n, int T, int F,
                  const sepr_fuse_tw* w, const sepr_fuse_grad* g, void* ws, size_t ws_bytes, sepr_stream_t stream);

int sepr_outlayer_decoder_train_fwd(const float* x, int nS, int S, int Tsrc, int L, const int* idx, const float* enc, int F, int N,
                                    int K, int stride, const sepr_out_tw* w, float* wav, void* ctx, size_t ctx_bytes, void* ws,
                                    size_t ws_bytes, sepr_stream_t stream);
/* dwav [S,B,Tout] -> dx [nS,Tsrc,F] (dx_accumulate: +=; rows of the main head beyond L get zero), denc [B,L,N] += for the
 * masked (auxiliary) heads; idx_start [Tsrc+1]: first output frame mapped to each source frame (inverse of idx) */
int sepr_outlayer_decoder_bwd(const float* x, const float* dwav, float* dx, int dx_accumulate, float* denc, int nS, int S, int Tsrc,
                              int L, const int* idx, const int* idx_start, const float* enc, int F, int N, int K, int stride,
                              const sepr_out_tw* w, const sepr_out_grad* g, const void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes,
                              sepr_stream_t stream);

/* encoder + projector: wav [B,T] -> enc [B,L,N] (kept by the caller: the auxiliary heads read it), out [B,Lp,F] */
int sepr_front_train_fwd(const float* wav, int B, int T, int N, int K, int stride, int F, int Lp, float gn_eps, const sepr_front_tw* w,
                         float* enc, float* out, void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, sepr_stream_t stream);
/* dout [B,Lp,F]; denc_aux [B,L,N] or NULL = gradient the auxiliary heads sent into enc (overwritten: used as scratch) */
int sepr_front_bwd(const float* wav, const float* enc, const float* dout, float* denc_aux, int B, int T, int N, int K, int stride, int F,
                   int Lp, const sepr_front_tw* w, const sepr_front_grad* g, const void* ctx, size_t ctx_bytes, void* ws,
                   size_t ws_bytes, sepr_stream_t stream);

/* G[N][K] (+)= sum_m A[m][n] B[m][k]: the weight-gradient contraction on its own (tests, roofline bench).
 * x3: 0 = exact f32 MFMA, 1 = bf16x3, 2 = plain bf16 operands. */
size_t sepr_linear_wgrad_workspace(int M, int N, int K);
int sepr_linear_wgrad(const float* A, const float* B, float* G, float* colsum, int M, int N, int K, int accumulate, int x3, void* ws,
                      size_t ws_bytes, sepr_stream_t stream);
/* the same for two bf16 operands A16 [M][lda], B16 [M][ldb] (leading dimensions in elements), as the plain-bf16 training precision stores the
 * large intermediates of the GCFN / CLA backward (ABI 4.12); one bf16 MFMA per product, fp32 accumulate */
int sepr_linear_wgrad_bf16(const void* A16, int lda, const void* B16, int ldb, float* G, float* colsum, int M, int N, int K, int accumulate,
                           void* ws, size_t ws_bytes, sepr_stream_t stream);
/* the same with the normalisation prologue of a projection behind a LayerNorm: B'[m][k] = (B[m][k] - stats[2m]) * stats[2m+1] */
int sepr_linear_wgrad_norm(const float* A, const float* B, const float* stats, float* G, float* colsum, int M, int N, int K,
                           int accumulate, int x3, void* ws, size_t ws_bytes, sepr_stream_t stream);

/* ---- per-step weight re-pack on the device (ABI 4.00) -----------------------------------------------------------------
 * What the reference's modules do implicitly - read the CURRENT value of every nn.Parameter on each forward (network.py:60-66 etc.) - costs
 * this path a re-layout of every projection after each optimizer step (sepreformer_amd/train_pack.py).  One call handles a STACK of G
 * same-shaped projections and reads the parameters where they live:
 *   src    device table of G * panels pointers; block g's [SN][SK] fp32 source matrix is the row-wise concatenation of its `panels`
 *          tensors (panels = 3: linear_q / linear_k / linear_v stacked, network.py:76-78), each [SN / panels][SK] row-major
 *   scale  device table of G pointers (or NULL with scale_kind 0): scale_kind 1 = per source COLUMN [SK] (LayerNorm / GroupNorm gamma
 *          folded into the weight), 2 = per source ROW [SN] (LayerScale folded in)
 *   transpose 0: out[n][k] = src[n][k] * s;  1: out[n][k] = src[k][n] * s  (the input-gradient form), N x K = SK x SN
 *   planes 1: out = G x pack_x3 fragments (bf16 hi / lo planes, [N/16][K/32][2][64][8], as sepr_x3_w.wp); 0: G x fp32 [N][K]
 * N % 16 == 0 and K % 32 == 0.  Bit-identical to the torch formulation fl32((double)w * (double)s) -> bf16 split. */
int sepr_train_pack_lin(const void* const* src, const void* const* scale, int G, int SN, int SK, int panels, int scale_kind, int transpose,
                        int planes, void* out, sepr_stream_t stream);
/* out[g][n] = (float)((double)bias[g][n] + sum_k (double)W[g][n][k] (double)beta[g][k]): the bias with the LayerNorm beta folded in.
 * w / bias: tables of G * panels pointers ([N / panels][K] and [N / panels] each), beta: G pointers [K].  bias NULL: 0; w and beta NULL: a
 * plain gather of the biases into one [G][N] buffer. */
int sepr_train_fold_bias(const void* const* w, const void* const* bias, const void* const* beta, int G, int N, int K, int panels, float* out,
                         sepr_stream_t stream);

/* The fused GCFN kernel's weight forms (sepr_gcfn_tw.fused_w1p / fused_w2p, i.e. sepr_gcfn_w's) for a stack of G blocks in one launch:
 * seven device tables of G pointers to the blocks' parameters (net1.1.weight [6F,F], net1.1.bias, net1.0.weight / bias [F], net2.2.weight
 * [F,3F], depthwise.weight [6F,1,3], depthwise.bias [6F]).  w1p: G x (3F/32) x (4 * (F/32) * 2 KiB + 4 KiB) bytes, w2p: G x (3F/32) x
 * (F/16) x 2 KiB bytes; layouts as documented on sepr_gcfn_w.  F in {64, 128}. */
int sepr_train_pack_gcfn_fused(const void* const* w1, const void* const* b1, const void* const* ln_g, const void* const* ln_b,
                               const void* const* w2, const void* const* dw_w, const void* const* dw_b, int G, int F, void* w1p, void* w2p,
                               sepr_stream_t stream);

/* ---- deferred gradient finishers (ABI 4.00) ---------------------------------------------------------------------------
 * Every sepr_<block>_bwd ends the gradient of a projection behind a LayerNorm / in front of a LayerScale with a weight-sized "finisher"
 * launch (csrc/sepr_train.h); a step has ~320 of them at 5-7 us each - launch latency, not work - and nothing in the backward reads
 * their outputs.  Between sepr_train_defer_begin and sepr_train_defer_flush ON THE SAME HOST THREAD the finishers are queued and the
 * flush runs them as a few batched launches on `stream` (bit-identical arithmetic).  `arena`: device scratch that receives the reduced
 * contractions until the flush - the sum over the deferred projections of (N K + N) floats, i.e. about one model's worth of parameters
 * (Base: 64 MB is plenty); a full arena simply falls back to immediate launches.  flush(close = 0) keeps the window open (a caller that
 * needs the gradients of the blocks processed so far - an early all-reduce bucket - flushes there); flush(close = 1) ends it.  The window
 * is per host thread (thread-local state); without one the entry points behave exactly as before. */
int sepr_train_defer_begin(void* arena, size_t arena_bytes);
int sepr_train_defer_flush(int close, sepr_stream_t stream);

/* PIT_SISNR_time backward (criterions.py:191-217): d(sum_b loss[b] * gl[b]) / d est.  est, tgt, dest [S,B,T]; perm from the forward. */
int sepr_pit_sisnr_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, double eps,
                       double clamp_min, float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream);
/* PIT_SISNR_mag backward (criterions.py:148-176).  dft_t [frame_len][ldd]: the transpose of the first frame_len + 2 rows of
 * `dft`, zero padded to ldd = frame_len + 2 rounded up to a multiple of 32 columns. */
int sepr_pit_sisnr_mag_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, const float* dft,
                           const float* dft_t, int frame_len, int frame_shift, double eps, float* dest, void* ws, size_t ws_bytes,
                           sepr_stream_t stream);
size_t sepr_pit_sisnr_mag_bwd_workspace(int S, int B, int T, int frame_len, int frame_shift);
/* Backward of sepr_pit_sasdr_fwd / sepr_pit_sasdr_mag_fwd: d(sum_b loss[b] * gl[b]) / d est with the forward's perm held fixed,
 *   d loss[b] / d e_s = (20 / ln 10) / (E + tau D + eps) (e~_s - t~_p(s))     (on M, then re / M, STFT adjoint, overlap-add, de-mean)
 * - no clamp branch, nothing flows through a target scale.  A pair that is bit-equal gets a gradient that is exactly 0.  Workspaces: the
 * siblings' (sepr_pit_sisnr_bwd's, sepr_pit_sisnr_mag_bwd_workspace). */
int sepr_pit_sasdr_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, double eps,
                       double snr_max, float* dest, void* ws, size_t ws_bytes, sepr_stream_t stream);
int sepr_pit_sasdr_mag_bwd(const float* est, const float* tgt, const int* perm, const float* gl, int S, int B, int T, const float* dft,
                           const float* dft_t, int frame_len, int frame_shift, double eps, double snr_max, float* dest, void* ws,
                           size_t ws_bytes, sepr_stream_t stream);

/* ---- optimizer step of the reference loop (ABI 3.03) ------------------------------------------------
 * engine.py:76-77: torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.AdamW.step() as three launches over the whole
 * model.  The gradients live in ONE flat fp32 buffer (the training path's gradient buffer: 64-element aligned slices, zero padding);
 * the moments in two flat fp32 buffers of the caller.  All table pointers are DEVICE pointers.
 *   params[i]     parameter tensor i (fp32, contiguous, 16-byte aligned)
 *   grad_off[i]   element offset of its gradient in `grads`;  state_off[i]: of its moments in exp_avg / exp_avg_sq (multiples of 4)
 *   numel[i]      elements of tensor i
 *   blocks[2 b], blocks[2 b + 1] = (tensor, first element) of update block b; a block covers sepr_adamw_block_elems() elements
 * step: device double, incremented by the call; lr: device float (a scheduler refreshes it without re-capturing a graph);
 * max_norm <= 0: no clipping (no norm pass).  scal (device, 8 floats) receives [0] the total gradient norm BEFORE clipping,
 * [1] the clip coefficient min(1, max_norm / (norm + 1e-6)), [2..4] the step's derived scalars.  The gradients are NOT scaled in
 * place: the coefficient is applied inside the update.  Arithmetic: torch's AdamW (decoupled weight decay), fp32 per element.
 * A non-finite total norm yields a NaN coefficient that reaches every element (clip_grad_norm_'s torch.clamp semantics).  The norm
 * pass reads grads[0 .. grads_numel): the 64-element alignment padding between slices must be zero (the training path's buffer is
 * allocated zeroed and only slices are ever written). */
typedef struct {
  float* const* params;
  const long long* grad_off;
  const long long* state_off;
  const int* numel;
  const int* blocks;
  int ntensors, nblocks;
} sepr_adamw_tables;
int sepr_adamw_block_elems(void);
size_t sepr_adamw_workspace(void);
int sepr_adamw_step(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                    double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                    float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream);
/* The same step behind a guard, for a loop that looks at the host once per log interval: the norm pass always runs (ws is always
 * needed; max_norm <= 0 still means no clipping).  A total norm that is not finite sets scal[5] = 1 and skips the step: `step` does
 * not advance, no parameter or moment is written, and of scal only [0] (the norm) and [5] are written: [1..4] keep the step before's.  Otherwise scal[5] = 0 and the arithmetic is sepr_adamw_step's, bit for bit.
 * (sepr_adamw_step itself never writes scal[5].) */
int sepr_adamw_step_guarded(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                            double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                            float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream);
/* The guarded step that also keeps an exponential moving average (EMA) of the parameters: the same three launches and the same skip
 * rule.  ema: a flat fp32 buffer of the caller, laid out by state_off like the two moments, 16-byte aligned.  With t the step counter
 * after its increment, the prepare kernel forms in double d_t = ema_decay when ema_warmup <= 0, else
 * d_t = min(ema_decay, (1 + t) / (ema_warmup + t)), and writes scal[6] = (float)(1 - d_t).  The update kernel stores the new parameter p
 * and then, from the same register, e = e + scal[6] * (p - e): fp32, three rounded operations, no FMA.  Parameters, moments, the
 * counter and scal[0..5] are sepr_adamw_step_guarded's, bit for bit.  A skipped step writes neither ema nor scal[6].
 * SEPR_EINVAL for a null or misaligned ema, or an ema_decay outside [0, 1). */
int sepr_adamw_step_ema(const sepr_adamw_tables* t, const float* grads, long long grads_numel, float* exp_avg, float* exp_avg_sq,
                        double* step, const float* lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                        float* ema, double ema_decay, double ema_warmup, float* scal, void* ws, size_t ws_bytes, sepr_stream_t stream);
/* One launch over the same block table: every parameter tensor trades places, bitwise, with its state_off slot of `shadow` (flat
 * fp32, 16-byte aligned; an EMA buffer, for instance): float4 where four elements remain, scalars in the tail.  Twice is the
 * identity.  grad_off is not read.  The caller re-packs whatever it derived from the parameters (Model.invalidate_packed). */
int sepr_adamw_swap(const sepr_adamw_tables* t, float* shadow, sepr_stream_t stream);

/* ---- run ledger: what a training loop needs to know about its steps, kept on the device ---------------------------------------
 * One launch, one thread, plain stores, fixed order: fold one step into `ledger` (float64, zeroed by the caller at the start of
 * an epoch).  parts: the step's loss scalars as one fp32 device vector (time loss, then one per stage).  opt_scal: the `scal` of the
 * optimizer step that followed (NULL for validation: the gradient-norm slots then stay as they are).  A skipped step
 * (opt_scal[5] != 0) adds to SEPR_LEDGER_SKIPPED and to nothing else.  Slots: */
enum {
  SEPR_LEDGER_STEPS = 0,      /* steps counted (not skipped) */
  SEPR_LEDGER_SKIPPED = 1,    /* steps the guarded optimizer skipped */
  SEPR_LEDGER_NONFINITE = 2,  /* counted steps with a non-finite loss part */
  SEPR_LEDGER_GNORM_SUM = 3,  /* sum of the total gradient norm before clipping (scal[0]) */
  SEPR_LEDGER_GNORM_MAX = 4,  /* its maximum */
  SEPR_LEDGER_CLIPPED = 5,    /* steps with scal[1] < 1 */
  SEPR_LEDGER_PART_SUM = 6,   /* [nparts] sum of each part; then [nparts] the last counted step's parts */
  SEPR_LEDGER_MAX_PARTS = 64
};
int sepr_run_ledger_doubles(int nparts);      /* SEPR_LEDGER_PART_SUM + 2 nparts; 0 for nparts outside 1..SEPR_LEDGER_MAX_PARTS */
int sepr_run_ledger_update(const float* parts, int nparts, const float* opt_scal, double* ledger, int ledger_doubles,
                           sepr_stream_t stream);

/* ---- opt-in kernel timer (bench.py roofline) ------------------------------------------------- */
/* Sites a projection launch can be attributed to. */
enum {
  SEPR_SITE_NONE = 0, SEPR_SITE_GCFN_UP, SEPR_SITE_GCFN_DOWN, SEPR_SITE_CLA, SEPR_SITE_ATTN_PROJ,
  SEPR_SITE_EGA_GATE, SEPR_SITE_SPLIT, SEPR_SITE_FUSE, SEPR_SITE_OUT, SEPR_SITE_PROJECTOR,
  SEPR_SITE_LINEAR, SEPR_SITE_WGRAD /* gemm_tn (training) */, SEPR_SITE_GCFN_BWD /* fused GCFN backward middle */,
  SEPR_SITE_COUNT
};
/* Start bracketing every launch of `site` with hipEvents on its own stream (up to max_launches). */
int sepr_prof_start(int site, int max_launches);
/* Synchronise the recorded events; returns launches, summed kernel ms and summed algorithmic FLOPs. */
int sepr_prof_stop(long long* launches, double* total_ms, double* flops);
/* Algorithmic HBM bytes of the launches of the session sepr_prof_stop last closed (sites that report them: the weight-gradient
 * contraction and the fused GCFN backward; 0 otherwise). */
double sepr_prof_last_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* SEPR_H_ */
