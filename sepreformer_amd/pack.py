"""Host-side weight packing: reference ``state_dict`` tensors -> the layouts ``include/sepr.h`` documents.

Done once per weight version on the device that owns the parameters (plain torch ops; weights are
"PyTorch-owned storage", the kernels only read them).  What happens here:

* depthwise-conv weights ``[C,1,K]`` become tap-major ``[K,C]`` so a wave reads contiguous channels;
* q/k/v projections are stacked into one ``[3F,F]`` matrix (one launch instead of three);
* eval-mode BatchNorm is folded: CLA's into ``linear2`` (reference ``modules/network.py:181-183``),
  DownConv's into a per-channel scale/shift behind the depthwise conv (``modules/module.py:74-75``);
  folding is done in fp64 and rounded once;
* 1x1 ``Conv1d`` weights ``[O,I,1]`` are viewed ``[O,I]``; ``LayerScale`` ``[1,1,F]`` is viewed ``[F]``;
* encoder / decoder kernels ``[N,1,K]`` become tap-major ``[K,N]``.
"""
from __future__ import annotations

import os
from typing import Dict, List

import torch

from . import lib as L
from .config import SepConfig

BN_EPS = 1e-5      # torch.nn.BatchNorm1d default
GN_EPS = 1e-8      # reference modules/module.py:28,117


PRECISIONS = ("fp32", "bf16x3")          # inference arithmetic (the training path adds "bf16": train_pack.PRECISIONS)


def _switch(name: str, default: str) -> bool:
    """An A/B switch of the environment: on by default ("1") it is off only at "0", off by default ("0") it is on only at "1"."""
    v = os.environ.get(name, default)
    return v == "1" if default == "0" else v != "0"


# ---- the primitives every packed form is made of: fold, split, fragment order, k-slot order, tile-pair interleave, chunk ------
def fold_norm(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """A norm's affine folded into the projection behind it: ``(x*gamma + beta) . w^T + b = x . (w*gamma)^T + (b + w . beta)``, in fp64,
    rounded to fp32 once.  ``w [..., N, K]``, ``b [..., N]``, ``gamma`` / ``beta`` ``[..., K]`` -> ``(w', b')``."""
    w64, beta64 = w.detach().double(), beta.detach().double()
    # one matrix reduces with @ and a stack with einsum, as their packers always have: a device may order the two fp64 sums differently
    wb = w64 @ beta64 if w64.dim() == 2 else torch.einsum("...nk,...k->...n", w64, beta64)
    return (w64 * gamma.detach().double()[..., None, :]).float(), (b.detach().double() + wb).float()


def split_bf16(w: torch.Tensor):
    """fp32 -> ``(hi, lo)`` bf16: ``hi = bf16(w)`` (round to nearest even), ``lo = bf16(w - hi)``."""
    hi = w.to(torch.bfloat16)
    return hi, (w - hi.to(torch.float32)).to(torch.bfloat16)


def _split_frag(w: torch.Tensor) -> torch.Tensor:
    """fp32 ``[..., R*16, K]`` (K % 32 == 0) -> ``[..., R][K/32][plane][64][8]`` bf16, THE fragment order: a wave of the bf16x3 core reads
    the 64 x 16-byte fragment of one (16-row tile, 32-deep K step, plane) as one contiguous 1 KiB block, lane ``g*16 + i`` holding
    ``w[16*tile + i][32*step + 8*g : 32*step + 8*g + 8]`` (sepreformer_amd/csrc/sepr_gemm_x3.h)."""
    R16, K = w.shape[-2:]
    planes = [p.unflatten(-2, (R16 // 16, 16)).unflatten(-1, (K // 32, 4, 8)).movedim(-4, -2) for p in split_bf16(w)]   # [..., tile, step, g, i, 8]
    return torch.stack(planes, dim=-4).flatten(-3, -2)


def pack_x3(w: torch.Tensor) -> torch.Tensor:
    """fp32 ``[N,K]`` -> bf16 hi/lo planes in MFMA fragment order ``[N/16][K/32][plane][lane][8]`` (``split_bf16``, ``_split_frag``), the lanes
    as ``[4 k groups][16 rows]``."""
    N, K = w.shape
    if N % 16 or K % 32:
        raise ValueError(f"bf16x3 packing needs N % 16 == 0 and K % 32 == 0, got {N}x{K}")
    return _split_frag(w.detach().to(torch.float32)).unflatten(-2, (4, 16))        # [tile, step, plane, g, i, 8]


# k slot (lane group g, element e) of the fused kernels' register fragments -> channel of a 32-wide K chunk: e < 4 ? 4g + e : 16 + 4g + e - 4
KSLOT = tuple(4 * g + e if e < 4 else 16 + 4 * g + e - 4 for g in range(4) for e in range(8))


def _kslot_frags(w2: torch.Tensor, nch: int) -> torch.Tensor:
    """``w2`` ``[..., R*16, 32*nch]`` -> ``[..., nch][R][2][64][8]`` bf16: per 32-wide K chunk, the fragments in ``KSLOT`` order."""
    cols = (32 * torch.arange(nch, device=w2.device)[:, None] + torch.tensor(KSLOT, device=w2.device)).reshape(-1)
    return _split_frag(w2.detach().float()[..., cols].unflatten(-1, (nch, 32)).movedim(-2, -3)).squeeze(-4)


def gate_perm_rows(F: int, device=None) -> torch.Tensor:
    """THE tile-pair row interleave: row ``4q + r`` of 16-row tile ``pt`` is output channel ``32*(pt // 2) + 8q + 4*(pt % 2) + r`` - the 8
    channels lane group ``q`` of a frame fragment holds at K step ``pt // 2`` (``gcfn_fused3_kernel``'s loader) split over a tile pair, so
    that a lane's accumulators of a tile pair are 8 consecutive channels of its frame (the kernels' epilogues rely on it)."""
    pt = torch.arange(F // 16, device=device)[:, None, None]
    q = torch.arange(4, device=device)[None, :, None]
    r = torch.arange(4, device=device)[None, None, :]
    return (32 * (pt // 2) + 8 * q + 4 * (pt % 2) + r).reshape(-1)


def _tile_rows(bases, device) -> torch.Tensor:
    """First rows ``[nch][tiles]`` of 16-row tiles -> their rows ``[nch, tiles*16]``."""
    return (torch.tensor(bases, device=device)[:, :, None] + torch.arange(16, device=device)).flatten(1)


def _glu_bases(H: int, nch: int):
    """Tiles of a value-then-gate projection ``[2H, K]`` per 32-channel chunk: ``v0 v1 g0 g1``."""
    return [[32 * c, 32 * c + 16, H + 32 * c, H + 32 * c + 16] for c in range(nch)]


def _chunks(wm: torch.Tensor, rows: torch.Tensor, cst: torch.Tensor) -> torch.Tensor:
    """THE LDS-DMA chunk of the row-stationary kernels: the fragments of the 16-row tiles ``rows`` (``_tile_rows``) of ``wm [..., N, K]``,
    ``[tiles][K/32][2][64][8]`` bf16, followed by a 4 KB fp32 constants block: ``cst [..., nch, <= 1024]``, zero padded.  -> bytes ``[..., nch, :]``."""
    frag = _split_frag(wm[..., rows.reshape(-1), :]).contiguous().view(torch.uint8).reshape(*wm.shape[:-2], rows.shape[0], -1)
    block = torch.zeros(*cst.shape[:-1], 1024, dtype=torch.float32, device=wm.device)
    block[..., :cst.shape[-1]] = cst
    return torch.cat([frag, block.view(torch.uint8)], dim=-1)


def _pair_block(vals) -> torch.Tensor:
    """The constants block of ``gcfn_fused3_kernel``: up to 10 vectors ``[..., nch, 2 tile pairs * 16]`` -> ``[..., nch, [2][10][16]]``,
    tile-pair stride 160 floats."""
    vals = list(vals) + [torch.zeros_like(vals[0])] * (10 - len(vals))
    return torch.stack(vals, dim=-2).unflatten(-1, (2, 16)).transpose(-3, -2).flatten(-3)


NEG_LOG2E = -1.4426950408889634     # sigmoid(g) = 1 / (1 + exp2(-log2(e) g)): the kernels evaluate the GLU as value * rcp(1 + exp2(gate'))
                                    # (csrc/sepr_common.h glu_prescaled), the packers put the factor into the gate half


class Packed:
    """Packed device tensors + the ctypes structs pointing at them (tensors are kept alive here)."""

    # fused form -> (widths its kernels take, the switch of width 256 and its default); the A/B switch is ``self.fuse_<form>``
    FUSED = {"mlp": ((128, 256), "SEPR_FUSE_MLP256", "0"),        # (F = 256: built, measured no gain - 426 vs 426 utt/s; off)
             "gcfn": ((64, 128, 256), "SEPR_FUSE_GCFN256", "1"),
             "cla": ((128, 256), "SEPR_FUSE_CLA256", "1"),
             "gate": ((128, 256), "SEPR_FUSE_GATE256", "1"),
             "spk": ((128, 256), "SEPR_FUSE_SPK256", "1")}

    def __init__(self, precision: str = "fp32"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}")
        self.precision = precision
        self.fuse_gcfn = _switch("SEPR_FUSE_GCFN", "1")     # A/B switch for the fused GCFN kernel
        self.fuse_spk = _switch("SEPR_FUSE_SPK", "1")       # A/B switch for the fused speaker attention
        self.fuse_cla = _switch("SEPR_FUSE_CLA", "1")       # A/B switch for the fused CLA head / tail
        self.fuse_gate = _switch("SEPR_FUSE_GATE", "1")     # A/B switch for the fused EGA gate
        self.fuse_mlp = _switch("SEPR_FUSE_MLP", "1")       # A/B switch for the fused SpkSplit / OutputLayer GLU-MLP
        self.keep: List[torch.Tensor] = []

    def fusable(self, form: str, F: int, widths=None) -> bool:
        """Whether the fused ``form`` applies at width ``F``: bf16x3 arithmetic, a width its kernels take, its A/B switch (read at
        construction) and, at F = 256, the width's own switch (read here)."""
        takes, sw256, default = self.FUSED[form]
        return (self.precision == "bf16x3" and F in (widths or takes) and getattr(self, "fuse_" + form)
                and (F != 256 or _switch(sw256, default)))

    def t(self, x: torch.Tensor) -> int:
        x = x.detach().to(torch.float32).contiguous()
        self.keep.append(x)
        return x.data_ptr()

    def kept(self, **forms) -> dict:
        """Keep the packed tensors alive; the struct fields that point at them."""
        self.keep += forms.values()
        return {k: v.data_ptr() for k, v in forms.items()}

    def x3(self, w: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor = None, beta: torch.Tensor = None) -> L.X3W:
        """bf16x3 form of ``y = LN_affine(x) . w^T + bias`` (NULL struct in fp32 mode), LayerNorm's affine folded (``fold_norm``)."""
        if self.precision != "bf16x3":
            return L.X3W()
        if gamma is not None:
            w, bias = fold_norm(w, bias, gamma, beta)
        return L.X3W(**self.kept(wp=pack_x3(w)), bias=self.t(bias))

    def glumlp_fused(self, w1, b1, w2) -> dict:
        """Fused Linear -> GLU -> Linear (SpkSplit, OutputLayer) for F = 128 and, opt-in, 256 in bf16x3 mode; ``{}`` otherwise."""
        F, H, N = w1.shape[1], w1.shape[0] // 2, w2.shape[0]
        if not self.fusable("mlp", F) or H % 32 or N % F:
            return {}
        w1p, w2p = pack_glumlp_fused(w1, b1, w2)
        return self.kept(fused_w1p=w1p, fused_w2p=w2p)

    def glumlp_fold(self, w1, w2, b2, dec_weight) -> dict:
        """OutputLayer's second projection with the AudioDecoder folded in (heads without a mask; bf16x3, F = 128 or 256, k = 16)."""
        F, H = w1.shape[1], w1.shape[0] // 2
        if not self.fusable("mlp", F) or H % 32 or w2.shape[0] % F or dec_weight.shape[2] != 16 or not _switch("SEPR_FOLD_HEAD", "1"):
            return {}
        w2p, bf = pack_glumlp_fold(w2, b2, dec_weight)
        return self.kept(fold_w2p=w2p, fold_b=bf)

    def gcfn_fused(self, sd, p: str) -> dict:
        """Fused-GCFN weight forms (bf16x3 mode, F in {64, 128, 256}); empty dict otherwise."""
        if not self.fusable("gcfn", sd[p + ".net1.0.weight"].shape[0]):
            return {}
        w1p, w2p = pack_gcfn_fused(sd[p + ".net1.1.weight"], sd[p + ".net1.1.bias"], sd[p + ".net1.0.weight"],
                                   sd[p + ".net1.0.bias"], sd[p + ".net2.2.weight"], sd[p + ".depthwise.weight"],
                                   sd[p + ".depthwise.bias"])
        return self.kept(fused_w1p=w1p, fused_w2p=w2p)

    def cla_fused(self, sd, p: str, w2: torch.Tensor, b2: torch.Tensor) -> dict:
        """Fused CLA head / tail weight forms (bf16x3, F = 128 or 256); ``w2`` / ``b2`` = linear2 with BatchNorm folded."""
        if not self.fusable("cla", sd[p + ".layer_norm.weight"].shape[0]):
            return {}
        w1p, w2p, w3p = pack_cla_fused(sd[p + ".linear1.weight"], sd[p + ".linear1.bias"], sd[p + ".layer_norm.weight"],
                                       sd[p + ".layer_norm.bias"], w2, b2, sd[p + ".linear3.1.weight"])
        return self.kept(fused_w1p=w1p, fused_w2p=w2p, fused_w3p=w3p)

    def gate_fused(self, sd, p: str) -> dict:
        """Fused EGA-gate weight form (bf16x3, F = 128 or 256)."""
        if not self.fusable("gate", sd[p + ".block.linear.0.weight"].shape[0]):
            return {}
        return self.kept(fused_gate_p=pack_gate_fused(sd[p + ".block.linear.1.weight"], sd[p + ".block.linear.1.bias"],
                                                      sd[p + ".block.linear.0.weight"], sd[p + ".block.linear.0.bias"]))

    def gate_perm(self, sd, p: str) -> int:
        """The gate projection in the fused GCFN kernel's row order (``sepr_global_block_fwd``; bf16x3, F = 128), 0 where it does not apply."""
        if not self.fusable("gate", sd[p + ".block.linear.0.weight"].shape[0], (128,)) or not self.fuse_gcfn:
            return 0
        return self.kept(p=pack_gate_fused_perm(sd[p + ".block.linear.1.weight"], sd[p + ".block.linear.1.bias"],
                                                sd[p + ".block.linear.0.weight"], sd[p + ".block.linear.0.bias"]))["p"]

    def qkv_fused(self, sd, p: str) -> dict:
        """EGA attention in-projection ``[3F, F]`` behind its LayerNorm in the gate's chunk form (bf16x3, F = 128): pooling + LayerNorm +
        q / k / v in one launch (``launch_ega_qkv``).  ``SEPR_FUSE_QKV=0`` keeps pool_stats + the generic projection."""
        if not self.fusable("gate", sd[p + ".layer_norm.weight"].shape[0], (128,)) or not _switch("SEPR_FUSE_QKV", "1"):
            return {}
        wqkv = torch.cat([sd[f"{p}.linear_{n}.weight"] for n in "qkv"], dim=0)
        bqkv = torch.cat([sd[f"{p}.linear_{n}.bias"] for n in "qkv"], dim=0)
        # fused_out_p [F/16][F/32][2][64][8] bf16: the gate launch's folded output projection (SEPR_FUSE_OUT=0: separate launch; kept either way)
        out = self.kept(fused_qkv_p=pack_gate_fused(wqkv, bqkv, sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"]),
                        fused_out_p=_split_frag(sd[p + ".linear_out.weight"].detach().float()).contiguous())
        if not _switch("SEPR_FUSE_OUT", "1"):
            del out["fused_out_p"]
        return out

    def spk_fused(self, sd, p: str, heads: int, num_spks: int) -> dict:
        """Fused speaker-attention weight forms (bf16x3, F = 128 with 16-channel or 256 with 32-channel heads, two speakers); else empty."""
        F = sd[p + ".layer_norm.weight"].shape[0]
        if not self.fusable("spk", F) or (F, F // heads) not in ((128, 16), (256, 32)) or num_spks != 2:
            return {}
        wqkv = torch.cat([sd[f"{p}.linear_{n}.weight"] for n in "qkv"], dim=0)
        bqkv = torch.cat([sd[f"{p}.linear_{n}.bias"] for n in "qkv"], dim=0)
        w1p, w2p = pack_spk_fused(wqkv, bqkv, sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"],
                                  sd[p + ".linear_out.weight"])
        return self.kept(fused_qkv_p=w1p, fused_out_p=w2p)


def pack_gcfn_fused(w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w2: torch.Tensor,
                    dw_w: torch.Tensor, dw_b: torch.Tensor):
    """Weights of the fully fused GCFN kernel (sepreformer_amd/csrc/sepr_gcfn_fused.hip), F = 64, 128 or 256.

    ``w1`` ``[6F,F]`` (value rows then gate rows), ``w2`` ``[F,3F]``, ``dw_w`` ``[6F,1,3]``, ``dw_b`` ``[6F]``; every argument may carry
    the same leading batch dimensions, which the results then carry too.  Returns two tensors:

    * ``w1p`` bytes ``[3F/32, :]``: per 32-channel hidden chunk (``_chunks``), the up-projection fragments ``[4][F/32][2][64][8]`` bf16
      (value tiles 0,1 then their gate tiles; LayerNorm gamma folded) followed by the 4 KB fp32 constants block
      ``[2 tile pairs][b1v b1g wv0 wv1 wv2 wg0 wg1 wg2 cbv cbg][16 channels]`` (bias with beta folded, conv taps,
      conv bias; the gate's taps and conv bias multiplied by -log2(e)), zero padded;
    * ``w2p`` ``[3F/32][F/16][2][64][8]`` bf16: the chunk's K slice of the down-projection in k-slot order (``KSLOT``) with the output
      rows of each tile pair interleaved (``gate_perm_rows``).

    The device packer of the training path (``pack_gcfn_fused_kernel``, csrc/sepr_train_packw.hip) is the one other statement of this form."""
    F = w1.shape[-1]
    H3, dev = 3 * F, w1.device
    nch = H3 // 32
    w1f, b1f = fold_norm(w1, b1, gamma, beta)
    gscale = torch.ones(2 * H3, dtype=torch.float64, device=dev)
    gscale[H3:] = NEG_LOG2E
    taps = (dw_w.detach().double().reshape(*dw_b.shape, 3) * gscale[:, None]).float().unbind(-1)        # 3 x [..., 6F]
    cb = (dw_b.detach().double() * gscale).float()
    rows = _tile_rows(_glu_bases(H3, nch), dev)
    v, g = rows[:, :32], rows[:, 32:]
    w1p = _chunks(w1f, rows, _pair_block([b1f[..., v], b1f[..., g], *[t[..., v] for t in taps], *[t[..., g] for t in taps],
                                          cb[..., v], cb[..., g]]))
    return w1p, _kslot_frags(w2.detach()[..., gate_perm_rows(F, dev), :], nch)


def pack_gcfn_fused_batched(w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w2: torch.Tensor,
                            dw_w: torch.Tensor, dw_b: torch.Tensor):
    """``pack_gcfn_fused`` for a STACK of G blocks (the reference of the training path's device packer).  ``w1 [G,6F,F]``, ``b1 [G,6F]``,
    ``gamma/beta [G,F]``, ``w2 [G,F,3F]``, ``dw_w [G,6F,3]`` (or ``[G,6F,1,3]``), ``dw_b [G,6F]`` -> ``(w1p [G, bytes],
    w2p [G,3F/32,F/16,2,64,8] bf16)``, byte-identical per block to ``pack_gcfn_fused`` (CPU test: tests/test_pack_digests_cpu.py)."""
    w1p, w2p = pack_gcfn_fused(w1, b1, gamma, beta, w2, dw_w, dw_b)
    return w1p.flatten(1), w2p


def pack_glumlp_fused(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor):
    """Weights of the plain GLU-MLP mode of the fused GCFN kernel (``gcfn_fused3_kernel<..., MODE = 1>``):
    ``y = w2 . GLU(w1 x + b1)`` with ``w1`` ``[2H, F]`` (value rows, then gate rows), ``w2`` ``[N, H]``, N a multiple of F (one kernel launch
    writes F output columns: 128 for Base, 256 for the Large variants).

    * ``w1p``: per 32-channel hidden chunk the fragments ``[v0 v1 g0 g1][F/32][2][64][8]`` bf16 + the 4 KB constants block of
      ``pack_gcfn_fused`` with only the biases filled in; the gate rows and their bias carry the -log2(e) of ``glu_prescaled``;
    * ``w2p`` ``[N/F][H/32][F/16][2][64][8]`` bf16: for every block of F output channels the K slices in k-slot order with the
      tile-pair row interleave of ``pack_gcfn_fused`` (one kernel launch per block)."""
    F, H, N = w1.shape[1], w1.shape[0] // 2, w2.shape[0]
    nch, dev = H // 32, w1.device
    gscale = torch.ones(2 * H, dtype=torch.float64, device=dev)
    gscale[H:] = NEG_LOG2E
    w1f = (w1.detach().double() * gscale[:, None]).float()
    b1f = (b1.detach().double() * gscale).float()
    rows = _tile_rows(_glu_bases(H, nch), dev)
    w1p = _chunks(w1f, rows, _pair_block([b1f[rows[:, :32]], b1f[rows[:, 32:]]]))
    return w1p, _kslot_frags(w2.detach().unflatten(0, (N // F, F))[:, gate_perm_rows(F, dev)], nch)


def pack_glumlp_fold(w2: torch.Tensor, b2: torch.Tensor, dec_weight: torch.Tensor):
    """``end_conv1x1.2`` (``w2 [N,H]``, ``b2 [N]``) followed by ``ConvTranspose1d(N -> 1, K, stride)`` (``dec_weight [N,1,K]``, no bias) with
    nothing in between (reference ``modules/module.py:252-256,278-283`` with ``masking=False``, ``model.py:28``) is one linear map from the
    gated tensor to the K taps a frame adds to the waveform: ``W_fold [K,H] = wdec^T . w2``, ``b_fold [K] = wdec^T . b2``, formed in fp64
    and rounded once.  Returns (``[H/32][1][2][64][8]`` bf16 hi/lo k-slot fragments for ``gcfn_fused3_kernel<..., MODE = 2>``, ``b_fold`` fp32)."""
    wd = dec_weight.detach().double()[:, 0, :]                                # [N, K]
    wf = (wd.t() @ w2.detach().double()).float()                              # [K, H]
    bf = (wd.t() @ b2.detach().double()).float().contiguous()
    if wf.shape[0] != 16 or wf.shape[1] % 32:
        raise ValueError(f"folded head needs K = 16 taps and H % 32 == 0, got {tuple(wf.shape)}")
    return _kslot_frags(wf, wf.shape[1] // 32), bf


def _biased_chunks(wm: torch.Tensor, bm: torch.Tensor, bases) -> torch.Tensor:
    """``_chunks`` of the tiles starting at ``bases [nch][tiles]`` with their biases ``[tiles][16]`` as the constants."""
    rows = _tile_rows(bases, wm.device)
    return _chunks(wm, rows, bm[rows])


def _chunks64(wm: torch.Tensor, bm: torch.Tensor) -> torch.Tensor:
    """``_biased_chunks`` of 64 consecutive rows each: four 16-row tiles and their biases."""
    return _biased_chunks(wm, bm, [[64 * c + 16 * j for j in range(4)] for c in range(wm.shape[0] // 64)])


def pack_gate_fused(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """A projection ``[N,F]`` behind a LayerNorm (the EGA gate, N = F; EGA's q / k / v, N = 3F) for the fused gate kernels, F = 128 or 256:
    per 64 output channels four 16-row tiles (gamma folded into the weights, beta into the bias) and their biases."""
    return _chunks64(*fold_norm(w, b, gamma, beta))


def pack_gate_fused_perm(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """``pack_gate_fused`` with the output rows in ``gate_perm_rows`` order, for the gate prologue of the fused GCFN kernel: a lane's gate
    accumulators are then the channels it holds of the frame.  Same folded fp32 rows, same bf16 split - only their position changes."""
    wf, bf = fold_norm(w, b, gamma, beta)
    rows = gate_perm_rows(w.shape[0], w.device)
    return _chunks64(wf[rows], bf[rows])


def pack_cla_fused(w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w2: torch.Tensor,
                   b2: torch.Tensor, w3: torch.Tensor):
    """Weights of the fused CLA head / tail kernels (sepreformer_amd/csrc/sepr_cla_fused.hip), F = 128 or 256.

    ``w1`` ``[2F,F]`` (value rows then gate rows, LayerNorm in front), ``w2`` ``[2F,F]`` / ``b2`` with the eval
    BatchNorm already folded, ``w3`` ``[F,2F]``.  Returns three tensors:

    * ``w1p``: per 32 output channels the fragments ``[v0 v1 g0 g1][F/32][2][64][8]`` bf16 (gamma folded) + a 4 KB fp32
      constants block ``[v0 v1 g0 g1][16]`` of biases (beta folded), zero padded;
    * ``w2p``: per 64 hidden channels the fragments ``[4 tiles][F/32][2][64][8]`` + 4 KB constants ``[4][16]`` biases;
    * ``w3p`` ``[2F/32][F/16][2][64][8]``: linear3 in k-slot order (``_kslot_frags``)."""
    F = w1.shape[1]
    w1f, b1f = fold_norm(w1, b1, gamma, beta)
    w1p = _biased_chunks(w1f, b1f, _glu_bases(F, F // 32))
    return w1p, _chunks64(w2.detach().float(), b2.detach().float()), _kslot_frags(w3, 2 * F // 32)


def pack_spk_fused(wqkv: torch.Tensor, bqkv: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, wo: torch.Tensor):
    """Weights of the fused speaker-attention kernel (sepreformer_amd/csrc/sepr_spk_fused.hip): F = 128 with 16-channel heads, F = 256 with
    32-channel heads (``Packed.spk_fused``).

    ``wqkv`` ``[3F,F]`` (q rows, k rows, v rows), ``wo`` ``[F,F]``.  Returns two tensors:

    * ``w1p``: per head pair ``c`` the fragments ``[6][F/32][2][64][8]`` bf16 of the tiles
      ``q(2c) q(2c+1) k(2c) k(2c+1) v(2c) v(2c+1)`` (LayerNorm gamma folded) followed by a 4 KB fp32 constants block
      ``[6 tiles][16 channels]`` of biases (beta folded), zero padded;
    * ``w2p`` ``[F/32][F/16][2][64][8]`` bf16: the pair's K slice of the output projection in k-slot order."""
    F = wqkv.shape[1]
    wf, bf = fold_norm(wqkv, bqkv, gamma, beta)
    w1p = _biased_chunks(wf, bf, [[tt * F + 16 * (2 * c + hh) for tt in range(3) for hh in range(2)] for c in range(F // 32)])
    return w1p, _kslot_frags(wo, F // 32)


def _tapmajor(w: torch.Tensor) -> torch.Tensor:
    return w[:, 0, :].t().contiguous()          # [C,1,K] -> [K,C]


def pack_gcfn(pk: Packed, sd: Dict[str, torch.Tensor], p: str) -> L.GcfnW:
    return L.GcfnW(
        ln_g=pk.t(sd[p + ".net1.0.weight"]), ln_b=pk.t(sd[p + ".net1.0.bias"]),
        w1=pk.t(sd[p + ".net1.1.weight"]), b1=pk.t(sd[p + ".net1.1.bias"]),
        dw_w=pk.t(_tapmajor(sd[p + ".depthwise.weight"])), dw_b=pk.t(sd[p + ".depthwise.bias"]),
        w2=pk.t(sd[p + ".net2.2.weight"]), b2=pk.t(sd[p + ".net2.2.bias"]),
        ls=pk.t(sd[p + ".Layer_scale.layer_scale"].reshape(-1)),
        x3_up=pk.x3(sd[p + ".net1.1.weight"], sd[p + ".net1.1.bias"], sd[p + ".net1.0.weight"], sd[p + ".net1.0.bias"]),
        x3_down=pk.x3(sd[p + ".net2.2.weight"], sd[p + ".net2.2.bias"]),
        **pk.gcfn_fused(sd, p))


def pack_cla(pk: Packed, sd, p: str) -> L.ClaW:
    s = sd[p + ".BN.weight"].double() / torch.sqrt(sd[p + ".BN.running_var"].double() + BN_EPS)
    w2 = (sd[p + ".linear2.weight"].double() * s[:, None]).float()
    b2 = ((sd[p + ".linear2.bias"].double() - sd[p + ".BN.running_mean"].double()) * s + sd[p + ".BN.bias"].double()).float()
    return L.ClaW(
        ln_g=pk.t(sd[p + ".layer_norm.weight"]), ln_b=pk.t(sd[p + ".layer_norm.bias"]),
        w1=pk.t(sd[p + ".linear1.weight"]), b1=pk.t(sd[p + ".linear1.bias"]),
        dw_w=pk.t(_tapmajor(sd[p + ".dw_conv_1d.weight"])), dw_b=pk.t(sd[p + ".dw_conv_1d.bias"]),
        w2=pk.t(w2), b2=pk.t(b2),
        w3=pk.t(sd[p + ".linear3.1.weight"]), b3=pk.t(sd[p + ".linear3.1.bias"]),
        ls=pk.t(sd[p + ".Layer_scale.layer_scale"].reshape(-1)),
        x3_1=pk.x3(sd[p + ".linear1.weight"], sd[p + ".linear1.bias"], sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"]),
        x3_2=pk.x3(w2, b2),
        x3_3=pk.x3(sd[p + ".linear3.1.weight"], sd[p + ".linear3.1.bias"]),
        **pk.cla_fused(sd, p, w2, b2))


def pack_mha(pk: Packed, sd, p: str, spk_fused: dict = None) -> L.MhaW:
    wqkv = torch.cat([sd[f"{p}.linear_{n}.weight"] for n in "qkv"], dim=0)
    bqkv = torch.cat([sd[f"{p}.linear_{n}.bias"] for n in "qkv"], dim=0)
    return L.MhaW(
        ln_g=pk.t(sd[p + ".layer_norm.weight"]), ln_b=pk.t(sd[p + ".layer_norm.bias"]),
        wqkv=pk.t(wqkv), bqkv=pk.t(bqkv),
        wo=pk.t(sd[p + ".linear_out.weight"]), bo=pk.t(sd[p + ".linear_out.bias"]),
        ls=pk.t(sd[p + ".Layer_scale.layer_scale"].reshape(-1)),
        x3_qkv=pk.x3(wqkv, bqkv, sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"]),
        x3_out=pk.x3(sd[p + ".linear_out.weight"], sd[p + ".linear_out.bias"]),
        **(spk_fused or {}))


def pack_ega(pk: Packed, sd, p: str, pe_ptr: int, maxlen: int, pe_planes_ptr: int = 0) -> L.EgaW:
    return L.EgaW(
        attn=pack_mha(pk, sd, p + ".block.self_attn"),
        gate_ln_g=pk.t(sd[p + ".block.linear.0.weight"]), gate_ln_b=pk.t(sd[p + ".block.linear.0.bias"]),
        gate_w=pk.t(sd[p + ".block.linear.1.weight"]), gate_b=pk.t(sd[p + ".block.linear.1.bias"]),
        pe_k=pe_ptr, maxlen=maxlen, pe_k_planes=pe_planes_ptr,
        x3_gate=pk.x3(sd[p + ".block.linear.1.weight"], sd[p + ".block.linear.1.bias"],
                      sd[p + ".block.linear.0.weight"], sd[p + ".block.linear.0.bias"]),
        **pk.gate_fused(sd, p), **pk.qkv_fused(sd, p + ".block.self_attn"))


def pack_down(pk: Packed, sd, p: str) -> L.DownW:
    s = sd[p + ".BN.weight"].double() / torch.sqrt(sd[p + ".BN.running_var"].double() + BN_EPS)
    shift = (sd[p + ".down_conv.bias"].double() - sd[p + ".BN.running_mean"].double()) * s + sd[p + ".BN.bias"].double()
    return L.DownW(w=pk.t(_tapmajor(sd[p + ".down_conv.weight"])), scale=pk.t(s.float()), shift=pk.t(shift.float()))


def pack_split(pk: Packed, sd, p: str) -> L.SplitW:
    return L.SplitW(
        w1=pk.t(sd[p + ".linear.0.weight"][:, :, 0]), b1=pk.t(sd[p + ".linear.0.bias"]),
        w2=pk.t(sd[p + ".linear.2.weight"][:, :, 0]), b2=pk.t(sd[p + ".linear.2.bias"]),
        gn_g=pk.t(sd[p + ".norm.weight"]), gn_b=pk.t(sd[p + ".norm.bias"]),
        x3_1=pk.x3(sd[p + ".linear.0.weight"][:, :, 0], sd[p + ".linear.0.bias"]),
        x3_2=pk.x3(sd[p + ".linear.2.weight"][:, :, 0], sd[p + ".linear.2.bias"]),
        **pk.glumlp_fused(sd[p + ".linear.0.weight"][:, :, 0], sd[p + ".linear.0.bias"], sd[p + ".linear.2.weight"][:, :, 0]))


def pack_fuse(pk: Packed, sd, p: str) -> L.FuseW:
    w, b = sd[p + ".weight"][:, :, 0], sd[p + ".bias"]
    return L.FuseW(w=pk.t(w), b=pk.t(b), x3=pk.x3(w, b))


def pack_out(pk: Packed, sd, p: str, dec_weight: torch.Tensor, fold: bool = False) -> L.OutW:
    return L.OutW(
        w1=pk.t(sd[p + ".end_conv1x1.0.weight"]), b1=pk.t(sd[p + ".end_conv1x1.0.bias"]),
        w2=pk.t(sd[p + ".end_conv1x1.2.weight"]), b2=pk.t(sd[p + ".end_conv1x1.2.bias"]),
        wdec=pk.t(_tapmajor(dec_weight)),
        x3_1=pk.x3(sd[p + ".end_conv1x1.0.weight"], sd[p + ".end_conv1x1.0.bias"]),
        x3_2=pk.x3(sd[p + ".end_conv1x1.2.weight"], sd[p + ".end_conv1x1.2.bias"]),
        **pk.glumlp_fused(sd[p + ".end_conv1x1.0.weight"], sd[p + ".end_conv1x1.0.bias"], sd[p + ".end_conv1x1.2.weight"]),
        **(pk.glumlp_fold(sd[p + ".end_conv1x1.0.weight"], sd[p + ".end_conv1x1.2.weight"], sd[p + ".end_conv1x1.2.bias"], dec_weight)
           if fold else {}))


class PackedModel(Packed):
    """All blocks of one model, addressed the way the forward driver walks them."""

    def __init__(self, cfg: SepConfig, sd: Dict[str, torch.Tensor], precision: str = "fp32"):
        super().__init__(precision)
        R = cfg.num_stages
        self.cfg = cfg
        self.enc_w = self.t(_tapmajor(sd["audio_encoder.conv1d.weight"]))
        self.proj_g = self.t(sd["feature_projector.norm.weight"])
        self.proj_b = self.t(sd["feature_projector.norm.bias"])
        self.proj_w = self.t(sd["feature_projector.conv1d.weight"][:, :, 0])
        pe = self.t(sd["separator.pos_emb.pe_k.weight"])
        pe_planes = 0
        if precision == "bf16x3":       # the table as bf16 hi / lo planes, split once here instead of per key tile in the attention kernel
            planes = torch.stack(split_bf16(sd["separator.pos_emb.pe_k.weight"].to(torch.float32)), 0).contiguous()
            self.keep.append(planes)
            pe_planes = planes.data_ptr()

        def glob(p):
            return (pack_ega(self, sd, p + ".block.ega", pe, cfg.maxlen, pe_planes), pack_gcfn(self, sd, p + ".block.gcfn"),
                    self.gate_perm(sd, p + ".block.ega"))

        def loc(p):
            return pack_cla(self, sd, p + ".block.cla"), pack_gcfn(self, sd, p + ".block.gcfn")

        def enc_stage(p, down):
            st = {"g": [glob(f"{p}.g_block_{i}") for i in (1, 2)], "l": [loc(f"{p}.l_block_{i}") for i in (1, 2)]}
            st["down"] = pack_down(self, sd, p + ".downconv") if down else None
            return st

        self.enc_stages = [enc_stage(f"separator.enc_stages.{i}", True) for i in range(R)]
        self.bottleneck = enc_stage("separator.bottleneck_G", False)
        if cfg.per_level_split:
            self.splits = [pack_split(self, sd, f"separator.spk_split_blocks.{i}") for i in range(R + 1)]
        else:
            one = pack_split(self, sd, "separator.spk_split_block")
            self.splits = [one] * (R + 1)
        self.fuse = [pack_fuse(self, sd, f"separator.simple_fusion.{i}") for i in range(R)]
        self.dec_stages = []
        for i in range(R):
            p = f"separator.dec_stages.{i}"
            self.dec_stages.append({
                "g": [glob(f"{p}.g_block_{j}") for j in (1, 2, 3)],
                "l": [loc(f"{p}.l_block_{j}") for j in (1, 2, 3)],
                "spk": [(pack_mha(self, sd, f"{p}.spk_attn_{j}.self_attn",
                                  self.spk_fused(sd, f"{p}.spk_attn_{j}.self_attn", cfg.heads, cfg.num_spks)),
                         pack_gcfn(self, sd, f"{p}.spk_attn_{j}.feed_forward")) for j in (1, 2, 3)],
            })
        self.out_main = pack_out(self, sd, "out_layer", sd["audio_decoder.weight"], fold=True)   # no mask on the main head (model.py:28)
        self.out_aux = [pack_out(self, sd, f"out_layer_bn.{i}", sd[f"decoder_bn.{i}.weight"]) for i in range(R)]
