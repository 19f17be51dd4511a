"""Branch parity: what the block tests measure once the residual is taken out, against a float64 reference, on hard inputs.
Shared by tests/test_branch_parity_cpu.py (the proof that the bar has teeth, reference side only) and
tests/test_branch_parity_gpu.py (the device against the same cases); the second half of the file holds the same instrument for the training
backward (tests/test_branch_parity_bwd_cpu.py, tests/test_branch_parity_bwd_gpu.py).  Test infrastructure only.

Why.  GCFN, CLA, EGA and SpkAttention return ``x + branch(x)``; the kernels pass ``x`` through and compute the branch, which with the
synthetic weights is 5 - 15 % of ``x``.  ``agreement_db(y, want)`` therefore sees a defect of the computed part 17 - 27 dB smaller than it
is.  ``branch_db`` subtracts the residual on both sides first.  Blocks without a residual are measured as they are.

The reference is the oracle (oracle/sepreformer_oracle.py) run unchanged in float64: ``sd64`` state dict, float64 input.

The bar (never taken from a device measurement):
  * ``floor_db``  = float32 oracle against float64 oracle on the very case (same input, same measure): what float32 CPU arithmetic itself
    achieves.  For large-magnitude inputs it is set by the float32 STORAGE of ``x + branch`` (one ulp of x against a branch of ~0.1).
  * fp32 precision:  ``bar = min(80, floor_db - 6)``.  80 dB is the suite's MIN_DB, 6 dB (2x in amplitude) allows another summation order.
  * bf16x3 precision: every projection / attention product multiplies operands split as ``a = hi + lo``, ``hi = bf16(a)``,
    ``lo = bf16(a - hi)`` and sums ``hi*hi + hi*lo + lo*hi`` in fp32.  Per operand ``|a - hi - lo| <= 2^-17 |a|`` (two 8-bit significands, the
    second taken from the remainder), the dropped ``lo*lo`` is ``<= 2^-16 |a b|`` (``|lo| <= 2^-8 |a|`` each), so one product carries
    ``<= ~2^-15.4`` relative error before any cancellation in the sum - about 93 dB on a well-conditioned product, less where the terms of
    the dot product cancel (offsets in front of a LayerNorm do not reach it, the normalised row does).  The cancellation is the case's own,
    so it is not guessed: ``floor_x3_db`` is the float64 oracle with exactly that split applied to the operands of every ``Linear``,
    1x1 convolution and attention ``matmul`` (fp32-rounded operands, as the device holds them; float64 sums, so only the split is in the
    figure), its output rounded to float32 as the device stores it, measured against the clean float64 oracle.
    ``bar = min(80, floor_x3_db - 6, floor_db - 6)``: outside the products the bf16x3 path IS the fp32 path (LayerNorm, softmax, depthwise
    convolution, storage), so it is never asked for more than the fp32 path on the same case.
  * A mutant (the oracle with one planted defect) must miss the bar of at least one listed case by 6 dB: test_branch_parity_cpu.py.

Input families.  ``randn * 1`` is the one distribution a normalising kernel cannot get wrong; real recordings hold digital silence, DC,
clipping and 60 dB level swings.  ``input_families`` / ``wave_families`` below are deterministic and need no files.

What exact silence and exactly constant rows can NOT show, by arithmetic: a row whose elements are all equal (or all zero) has
``x - mean == 0`` exactly, so LayerNorm / GroupNorm return their bias whatever ``eps`` is - the eps mutants are invisible there in exact
arithmetic and are carried by ``quiet`` (row variance 1e-8 against eps 1e-5) and the 1e-5-level waveform (GroupNorm variance ~1e-12
against eps 1e-8).  ``constant_rows`` / ``zeros`` / silent utterances are in the lists for the device's sake: rstd = 1/sqrt(eps) there, and a
variance formed as E[x^2] - mean^2 or a mean that is one ulp off is multiplied by 316 (LayerNorm) or 1e4 (GroupNorm).
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as TF

from oracle import sepreformer_oracle as orc
from sepreformer_amd.config import VARIANTS
from sepreformer_amd.synth import synth_mixture, synth_state_dict

MIN_DB = 80.0
MARGIN_DB = 6.0
BASE = "SepReformer_Base_WSJ0"
GPU_VARIANTS = ["tiny", BASE, "SepReformer_Large_DM_WHAMR"]
E0 = "separator.enc_stages.0"
D0 = "separator.dec_stages.0"


# ----------------------------------------------------------------------------------------------------------------------
# float64 reference and the measure
# ----------------------------------------------------------------------------------------------------------------------
def sd64(sd):
    """The float64 state dict (integer entries, e.g. BatchNorm's batch counter, stay as they are)."""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def oracle64(fn, sd, *args, **kw):
    """``fn`` (a function of oracle.sepreformer_oracle taking the state dict first) on float64 weights and float64 tensor arguments."""
    up = lambda a: a.double() if isinstance(a, torch.Tensor) and a.is_floating_point() else a   # noqa: E731
    if next(v for v in sd.values() if v.is_floating_point()).dtype != torch.float64:
        sd = sd64(sd)
    return fn(sd, *[up(a) for a in args], **{k: up(v) for k, v in kw.items()})


def branch_db(y, x, y64, x64):
    """Agreement of the computed part only: ``agreement_db(y - x, y64 - x64)``; ``x is None`` = the block has no residual."""
    if x is None:
        return orc.agreement_db(y.double(), y64)
    return orc.agreement_db(y.double() - x.double(), y64.double() - x64.double())


def bar(floor_db: float, floor_x3_db: Optional[float] = None) -> float:
    b = min(MIN_DB, floor_db - MARGIN_DB)
    return b if floor_x3_db is None else min(b, floor_x3_db - MARGIN_DB)


# ----------------------------------------------------------------------------------------------------------------------
# input families
# ----------------------------------------------------------------------------------------------------------------------
ROW_FAMILIES = ["randn", "plus10", "plus100", "loud", "quiet", "zeros", "silent_rows", "outlier", "row_range", "constant_rows", "one_hot_rows"]
WORST_FLOORS = ["randn", "plus100", "row_range", "outlier"]          # what the large shapes run: randn and the three lowest floors
WAVE_FAMILIES = ["speech", "silent_utt", "silent_half", "dc", "clipped", "level_1e-5"]
# Families the float64 oracle could not evaluate finitely would be listed here with the reason and leave the lists above (none did);
# test_branch_parity_cpu.py::test_family_lists_are_whole holds this to at most one family in ten.
REMOVED_FAMILIES: Dict[str, str] = {}


def input_families(shape, seed: int) -> Dict[str, torch.Tensor]:
    """Row tensors ``[..., rows, channels]`` (channel-last activations).  Deterministic."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = torch.randn(*shape, generator=g)
    rows, ch = shape[-2], shape[-1]
    out = {"randn": r, "plus10": r + 10.0, "plus100": r + 100.0, "loud": r * 1e3, "quiet": r * 1e-4, "zeros": torch.zeros(*shape)}
    s = r.clone()
    s[..., 1::3, :] = 0.0                                             # a third of the rows digital silence
    out["silent_rows"] = s
    o = r.clone()
    o[..., ::17, min(5, ch - 1)] = 300.0                              # one channel hits 300 every 17th frame
    out["outlier"] = o
    out["row_range"] = r * torch.exp(3.0 * torch.randn(*shape[:-1], 1, generator=g))   # per-row level over ~ +-26 dB (1 sigma)
    c = r.clone()
    c[..., ::7, :] = torch.randn(*shape[:-2], (rows + 6) // 7, 1, generator=g) * 2.0   # every 7th row constant: variance exactly 0
    out["constant_rows"] = c
    idx = (torch.arange(rows) * 7) % ch
    h = torch.zeros(*shape)
    h[..., torch.arange(rows), idx] = r[..., torch.arange(rows), idx] * 4.0            # one non-zero channel per row
    out["one_hot_rows"] = h
    return out


def wave_families(batch: int, samples: int, seed: int) -> Dict[str, torch.Tensor]:
    """Waveforms ``[batch, samples]``; ``speech`` is the project's synthetic mixture at the level of smoke()."""
    base = synth_mixture(batch, samples, seed=seed) * 4.0
    out = {"speech": base}
    s = base.clone()
    s[min(1, batch - 1)] = 0.0                                        # digital silence for one whole utterance of the batch
    out["silent_utt"] = s
    h = base.clone()
    h[:, samples // 2:] = 0.0                                         # silence for the second half
    out["silent_half"] = h
    out["dc"] = base + 0.5
    out["clipped"] = (base * 8.0).clamp(-1.0, 1.0)                    # full-scale clipping
    out["level_1e-5"] = base * (1e-5 / float(base.pow(2).mean().sqrt()))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the shared case list
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    """kind + shape + the families it runs + the variants it runs at (None = every variant of the device test)."""

    def __init__(self, kind, families, variants=None, **shape):
        self.kind, self.families, self.variants, self.shape = kind, list(families), variants, shape
        self.tag = kind + "." + "_".join(f"{k}{v}" for k, v in shape.items())

    def __repr__(self):
        return self.tag


RESIDUAL = {"gcfn", "cla", "ega", "spkattn"}
WAVE_KINDS = {"encoder", "projector", "e2e"}

BLOCK_CASES: List[Case] = (
    [Case("gcfn", ROW_FAMILIES, n=n, T=T) for n, T in ((2, 37), (3, 300))]                       # T a multiple of nothing; several sequences
    + [Case("cla", ROW_FAMILIES, n=n, T=T) for n, T in ((2, 24), (2, 150), (1, 500))]             # below the 65-tap window, one tile, several
    + [Case("ega", ROW_FAMILIES, n=2, fac=f, Tp=Tp) for f, Tp in ((1, 25), (2, 25), (4, 130), (16, 50), (8, 300))]
    + [Case("spkattn", ROW_FAMILIES, B=2, T=33)]
    + [Case("down", ROW_FAMILIES, n=2, T=T) for T in (40, 41, 6)]
    + [Case("split", ROW_FAMILIES, B=3, T=129)]
    + [Case("fuse", ROW_FAMILIES, B=2, T=24)]
    + [Case("encoder", WAVE_FAMILIES, B=3, T=4 * 131 + 12), Case("projector", WAVE_FAMILIES, B=3, T=4 * 131 + 12)]
    + [Case("head_main", ROW_FAMILIES, B=3, T=4 * 131 + 12), Case("head_aux", ROW_FAMILIES, B=3, T=4 * 131 + 12, Ts=37)]
)
# Base width, pooled length above maxlen = 2000 (the [T', T', dk] table: 280 MB in float32)
MAXLEN_CASES: List[Case] = [Case("ega", WORST_FLOORS, variants=[BASE], n=1, fac=1, Tp=2100),
                            Case("ega", WORST_FLOORS, variants=[BASE], n=1, fac=2, Tp=2050)]
# the training forward of the four residual blocks (another kernel instantiation): one shape per block
TRAIN_CASES: List[Case] = [Case("gcfn_train", ROW_FAMILIES, n=3, T=300), Case("cla_train", ROW_FAMILIES, n=2, T=150),
                           Case("ega_train", ROW_FAMILIES, n=2, fac=2, Tp=130), Case("spkattn_train", ROW_FAMILIES, B=3, T=33)]
E2E_CASES: List[Case] = [Case("e2e", WAVE_FAMILIES, variants=["tiny"], B=2, T=1500),
                         Case("e2e", WAVE_FAMILIES, variants=[BASE], B=2, T=4000)]
ALL_CASES = BLOCK_CASES + MAXLEN_CASES + TRAIN_CASES + E2E_CASES


def cases_for(variant, cases=None):
    return [c for c in (ALL_CASES if cases is None else cases) if c.variants is None or variant in c.variants]


_sds: Dict[Tuple[str, str], dict] = {}


def state(variant: str, dtype=torch.float32):
    """Synthetic weights of ``variant`` (seed 0, as every parity test uses), cached per dtype."""
    key = (variant, str(dtype))
    if key not in _sds:
        sd = synth_state_dict(VARIANTS[variant], 0)
        _sds[key] = sd if dtype == torch.float32 else sd64(sd)
    return _sds[key]


def make_inputs(case: Case, cfg, family: str) -> Dict[str, torch.Tensor]:
    """float32 host inputs of ``case`` (row tensors channel-last, as the device takes them)."""
    k, s = case.kind.replace("_train", ""), case.shape
    F, S = cfg.feat, cfg.num_spks
    seed = sum(ord(ch) for ch in case.tag) % 997
    if k in ("gcfn", "cla", "down"):
        return {"x": input_families((s["n"], s["T"], F), seed)[family]}
    if k == "ega":
        return {"x": input_families((s["n"], s["Tp"] * s["fac"], F), seed)[family]}
    if k == "spkattn":
        return {"x": input_families((s["B"] * S, s["T"], F), seed)[family]}
    if k == "split":
        return {"x": input_families((s["B"], s["T"], F), seed)[family]}
    if k == "fuse":
        return {"lo": input_families((s["B"] * S, s["T"] // 2, F), seed)[family], "sk": input_families((s["B"] * S, s["T"], F), seed + 1)[family]}
    if k in WAVE_KINDS:
        return {"wav": wave_families(s["B"], s["T"], seed)[family]}
    if k in ("head_main", "head_aux"):
        L_ = cfg.frames(s["T"])
        rows = cfg.padded_frames(L_) if k == "head_main" else s["Ts"]
        return {"z": input_families((s["B"] * S, rows, F), seed)[family], "wav": wave_families(s["B"], s["T"], seed)["speech"] * 0.025}
    raise KeyError(case.kind)


_posk: Dict[tuple, torch.Tensor] = {}


def _pos_k(sd, Tp, maxlen, variant_key):
    """The [T', T', dk] table, built once per (weights, length, dtype, clamp in force): 280 MB (float32) / 560 MB (float64) at T' = 2100."""
    w = sd["separator.pos_emb.pe_k.weight"]
    if Tp < 1000:
        return orc.rel_pos_k(sd, Tp, maxlen)
    key = (variant_key, Tp, maxlen, str(w.dtype), orc.rel_pos_k)
    if key not in _posk:
        for old in [q for q in _posk if q[3] == key[3] and q != key]:
            del _posk[old]                                            # one large table per dtype at a time
        _posk[key] = orc.rel_pos_k(sd, Tp, maxlen)
    return _posk[key]


def _cl(t):
    return t.permute(0, 2, 1)


def reference(case: Case, variant: str, sd, inp) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(output, residual input or None) of ``case`` from the oracle in the dtype of ``sd``, in the device's channel-last layout
    (heads / e2e: ``[S, B, samples]``; e2e also stacks the auxiliary outputs behind the main ones)."""
    dt = sd["separator.pos_emb.pe_k.weight"].dtype
    with torch.no_grad():
        return _forward(case, variant, sd, {k: v.to(dt) for k, v in inp.items()})


@contextlib.contextmanager
def _bn_training(sd, p):
    """Train-mode BatchNorm ``p`` of the oracle: batch statistics, and the in-place update of the running ones goes to a copy."""
    sdc = dict(sd)
    for name in ("running_mean", "running_var", "num_batches_tracked"):
        if p + name in sdc:
            sdc[p + name] = sdc[p + name].clone()
    orc.BN_TRAINING = True
    try:
        yield sdc
    finally:
        orc.BN_TRAINING = False


def _forward(case: Case, variant: str, sd, t):
    """The oracle call of ``case`` on the tensors ``t`` (already in the dtype of ``sd``); grad mode is the caller's."""
    cfg = VARIANTS[variant]
    F, H, S = cfg.feat, cfg.heads, cfg.num_spks
    k, s = case.kind, case.shape
    if k in ("gcfn", "gcfn_train"):
        return orc.gcfn(sd, E0 + ".g_block_1.block.gcfn", t["x"]), t["x"]
    if k == "cla":
        return orc.cla(sd, E0 + ".l_block_1.block.cla", t["x"]), t["x"]
    if k == "cla_train":
        with _bn_training(sd, E0 + ".l_block_1.block.cla.BN.") as sdc:
            return orc.cla(sdc, E0 + ".l_block_1.block.cla", t["x"]), t["x"]
    if k in ("ega", "ega_train"):
        pos = _pos_k(sd, s["Tp"], cfg.maxlen, variant)
        return orc.ega(sd, E0 + ".g_block_1.block.ega", _cl(t["x"]), pos, H), t["x"]
    if k in ("spkattn", "spkattn_train"):                            # network.py:241-247 in channel-last terms
        B, T = s["B"], s["T"]
        xr = t["x"].view(B, S, T, F).permute(0, 2, 1, 3).reshape(B * T, S, F)
        yr = xr + orc.mha(sd, D0 + ".spk_attn_1.self_attn", xr, None, H)
        return yr.view(B, T, S, F).permute(0, 2, 1, 3).reshape(B * S, T, F), t["x"]
    if k == "down":
        return orc.down_conv(sd, E0 + ".downconv", t["x"]), None
    if k == "down_train":
        with _bn_training(sd, E0 + ".downconv.BN.") as sdc:
            return orc.down_conv(sdc, E0 + ".downconv", t["x"]), None
    if k == "split":
        p = "separator.spk_split_blocks.0" if cfg.per_level_split else "separator.spk_split_block"
        return _cl(orc.spk_split(sd, p, _cl(t["x"]), S)), None
    if k == "fuse":
        up = orc.TF.interpolate(_cl(t["lo"]), size=s["T"], mode="nearest")
        y = orc.TF.conv1d(torch.cat([up, _cl(t["sk"])], 1), sd["separator.simple_fusion.0.weight"], sd["separator.simple_fusion.0.bias"])
        return _cl(y), None
    if k == "encoder":
        return _cl(orc.audio_encoder(sd, t["wav"], cfg.enc_stride)), None
    if k == "projector":
        e = orc.audio_encoder(sd, t["wav"], cfg.enc_stride)
        return _cl(orc.pad_signal(orc.feature_projector(sd, e), cfg.num_stages)), None
    if k in ("head_main", "head_aux"):
        e = orc.audio_encoder(sd, t["wav"], cfg.enc_stride)
        B = s["B"]
        if k == "head_main":
            o = orc.output_layer(sd, "out_layer", _cl(t["z"]), e, S, False)
            w = sd["audio_decoder.weight"]
        else:
            up = orc.TF.interpolate(_cl(t["z"]), size=e.shape[-1], mode="nearest")
            o = orc.output_layer(sd, "out_layer_bn.1", up, e, S, True)
            w = sd["decoder_bn.1.weight"]
        return torch.stack([orc.audio_decoder(w, o[i], cfg.enc_stride).reshape(B, -1) for i in range(S)], 0), None
    if k == "e2e":
        audio, aux = orc.model_forward(sd, cfg, t["wav"])
        B = s["B"]
        n = min(a.reshape(B, -1).shape[-1] for a in list(audio) + [a for st in aux for a in st])
        rows = [torch.stack([a.reshape(B, -1)[:, :n] for a in audio], 0)]
        rows += [torch.stack([a.reshape(B, -1)[:, :n] for a in st], 0) for st in aux]
        return torch.stack(rows, 0), None                            # [1 + R, S, B, n]
    raise KeyError(k)


# ----------------------------------------------------------------------------------------------------------------------
# patching the oracle: a namespace that answers like torch / torch.nn.functional except for the names given
# ----------------------------------------------------------------------------------------------------------------------
class _Proxy:
    def __init__(self, real, **over):
        self.__dict__["_real"], self.__dict__["_over"] = real, over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._real, name)


@contextlib.contextmanager
def patched(**names):
    """Replace module globals of the oracle (``TF``, ``torch``, ``mha``, ``_ln``, ``_lin``, ``_bn_eval``, ``rel_pos_k``) for the duration."""
    old = {k: getattr(orc, k) for k in names}
    try:
        for k, v in names.items():
            setattr(orc, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(orc, k, v)


# ----------------------------------------------------------------------------------------------------------------------
# bf16x3: the split of the module docstring applied to the oracle's products
# ----------------------------------------------------------------------------------------------------------------------
def _split(a):
    a32 = a.float()
    hi = a32.bfloat16().float()
    lo = (a32 - hi).bfloat16().float()
    return hi.double(), lo.double()


def _mm_x3_raw(a, b):
    ah, al = _split(a)
    bh, bl = _split(b)
    return torch.matmul(ah, bh) + torch.matmul(ah, bl) + torch.matmul(al, bh)


class _MMx3(torch.autograd.Function):
    """The split product with the device's backward.  ``_split`` goes through ``.bfloat16()``, whose autograd backward rounds the GRADIENT
    to bf16, so differentiating ``_mm_x3_raw`` would corrupt the reference.  The device's dgrad and wgrad are split products themselves:
    ``dA = mm_x3(dC, B^T)``, ``dB = mm_x3(A^T, dC)`` (fp32-rounded operands, float64 sums), summed over the dimensions ``matmul`` broadcast."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _mm_x3_raw(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        da = _mm_x3_raw(dc, b.transpose(-1, -2)).sum_to_size(a.shape) if ctx.needs_input_grad[0] else None
        db = _mm_x3_raw(a.transpose(-1, -2), dc).sum_to_size(b.shape) if ctx.needs_input_grad[1] else None
        return da, db


def _mm_x3(a, b):
    return _MMx3.apply(a, b)


def _lin_x3(sd, p, x):
    return _mm_x3(x, sd[p + ".weight"].t()) + sd[p + ".bias"]


def _conv1d_x3(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    if groups != 1 or w.shape[-1] != 1 or stride != 1:
        return TF.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=groups)    # depthwise / encoder: plain fp32 on the device
    y = _mm_x3(x.transpose(1, 2), w[:, :, 0].t()).transpose(1, 2).contiguous()
    return y if b is None else y + b[None, :, None]


def x3_context():
    return patched(_lin=_lin_x3, TF=_Proxy(TF, conv1d=_conv1d_x3), torch=_Proxy(torch, matmul=_mm_x3))


def reference_x3(case, variant, inp):
    """The float64 oracle with bf16 hi+lo products, output rounded to float32 (device storage)."""
    with x3_context():
        y, x = reference(case, variant, state(variant, torch.float64), inp)
    return y.float().double(), x


_floor_cache: Dict[tuple, dict] = {}


def floors(case: Case, variant: str, family: str, want_x3: bool = True) -> dict:
    """Everything the reference side says about one (case, family): float64 output ``y64`` / ``x64``, ``floor_db``, ``floor_x3_db``."""
    key = (case.tag, variant, family)
    got = _floor_cache.get(key)
    if got is None:
        cfg = VARIANTS[variant]
        inp = make_inputs(case, cfg, family)
        y64, x64 = reference(case, variant, state(variant, torch.float64), inp)
        y32, x32 = reference(case, variant, state(variant), inp)
        got = {"inp": inp, "y64": y64, "x64": x64, "floor_db": branch_db(y32, x32, y64, x64),
               "finite": bool(torch.isfinite(y64).all()), "floor_x3_db": None}
        _floor_cache[key] = got
    if want_x3 and got["floor_x3_db"] is None:
        y3, _ = reference_x3(case, variant, got["inp"])
        got["floor_x3_db"] = branch_db(y3, got["x64"], got["y64"], got["x64"])
    return got


# ----------------------------------------------------------------------------------------------------------------------
# mutants: the oracle with ONE planted defect each (the kind of slip a kernel makes), written here about the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _mha_variant(mask_last_ragged=False, pos_unscaled=False):
    """MultiHeadAttention as oracle.mha states it, with two switchable defects (both off: identical, checked by the CPU test)."""
    def mha(sd, p, x, pos_k, heads):
        n, t, F = x.shape
        dk = F // heads
        x = orc._ln(sd, p + ".layer_norm", x)
        q, k, v = (orc._lin(sd, p + ".linear_" + c, x).view(n, -1, heads, dk).transpose(1, 2) for c in "qkv")
        A = torch.matmul(q, k.transpose(-2, -1))
        if pos_k is not None:
            rq = q.contiguous().view(n * heads, -1, dk).transpose(0, 1)
            Bm = torch.matmul(rq, pos_k.transpose(-2, -1)).transpose(0, 1).view(n, heads, pos_k.size(0), pos_k.size(1))
            scores = A / math.sqrt(dk) + Bm if pos_unscaled else (A + Bm) / math.sqrt(dk)
            if mask_last_ragged and t % 128:
                scores = scores.clone()
                scores[..., t - 1] = float("-inf")
        else:
            scores = A / math.sqrt(dk)
        o = torch.matmul(torch.softmax(scores, dim=-1), v).transpose(1, 2).contiguous().view(n, -1, heads * dk)
        return orc._lin(sd, p + ".linear_out", o) * sd[p + ".Layer_scale.layer_scale"]
    return mha


def _clamp(lo_off, hi_off):
    def rel_pos_k(sd, t, maxlen):
        pos = torch.arange(0, t).long()
        pos = (pos[:, None] - pos[None, :]).clamp(-maxlen + lo_off, maxlen - 1 - hi_off) + maxlen
        return TF.embedding(pos, sd["separator.pos_emb.pe_k.weight"])
    return rel_pos_k


def _halo_conv(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    y = TF.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=groups)
    if groups == x.shape[1] and w.shape[-1] == 3 and x.shape[-1] > 128:      # GCFN's 3-tap depthwise: frame 128 of sequence 0 loses its left tap
        y = y.clone()
        y[0, :, 128] -= w[:, 0, 0] * x[0, :, 127]
    return y


def _interp_last(x, size=None, mode="nearest"):
    y = TF.interpolate(x, size=size, mode=mode).clone()
    y[..., -1] = x[..., max(x.shape[-1] - 2, 0)]                              # the last output frame reads source frame src - 2
    return y


def _pool_count(x, out_len):
    y = TF.adaptive_avg_pool1d(x, out_len).clone()
    fac = x.shape[-1] // out_len
    # the last window sums one frame too few and still divides by fac.  (A wrong divisor alone is a scale on a row that goes straight
    # into the attention's LayerNorm, which removes it: no input can show it, so the mutant is the miscounted window.)
    y[..., -1] = x[..., x.shape[-1] - fac:x.shape[-1] - 1].sum(-1) / fac
    return y


def _ln_eps(sd, p, x):
    w = sd[p + ".weight"]
    return TF.layer_norm(x, (w.shape[0],), w, sd[p + ".bias"], 1e-6)


def _gn_eps(x, groups, w, b, eps):
    return TF.group_norm(x, groups, w, b, eps * 0.1)


EGA_KINDS = {"ega", "ega_train"}


def mutants() -> Dict[str, dict]:
    """name -> {"ctx": () -> context manager that plants the defect in the oracle, "kinds": the case kinds it can touch}."""
    return {
        "clamp_neg_off_by_one": {"ctx": lambda: patched(rel_pos_k=_clamp(1, 0)), "kinds": EGA_KINDS},
        "clamp_both_off_by_one": {"ctx": lambda: patched(rel_pos_k=_clamp(1, 1)), "kinds": EGA_KINDS},
        "ragged_last_key_masked": {"ctx": lambda: patched(mha=_mha_variant(mask_last_ragged=True)), "kinds": EGA_KINDS},
        "dwconv_halo_tap_lost": {"ctx": lambda: patched(TF=_Proxy(TF, conv1d=_halo_conv)), "kinds": {"gcfn", "gcfn_train"}},
        "upsample_last_index": {"ctx": lambda: patched(TF=_Proxy(TF, interpolate=_interp_last)), "kinds": EGA_KINDS | {"head_aux", "fuse"}},
        "avgpool_wrong_count": {"ctx": lambda: patched(TF=_Proxy(TF, adaptive_avg_pool1d=_pool_count)), "kinds": EGA_KINDS},
        "layernorm_eps_1e-6": {"ctx": lambda: patched(_ln=_ln_eps), "kinds": {"gcfn", "cla", "ega", "spkattn", "gcfn_train", "cla_train", "ega_train", "spkattn_train"}},
        "groupnorm_eps_1e-9": {"ctx": lambda: patched(TF=_Proxy(TF, group_norm=_gn_eps)), "kinds": {"projector", "split", "e2e"}},
        "pos_term_unscaled": {"ctx": lambda: patched(mha=_mha_variant(pos_unscaled=True)), "kinds": EGA_KINDS},
    }


# ======================================================================================================================
# the backward: the same instrument on the branch GRADIENT (tests/test_branch_parity_bwd_cpu.py, tests/test_branch_parity_bwd_gpu.py)
#
# ``dx = dy + J^T dy``: the backward kernels pass ``dy`` through and compute only the second term, 3 - 30 % of ``dy`` with the synthetic
# weights, so ``agreement_db`` on whole ``dx`` hides a defect of the computed part by 10 - 30 dB exactly as it does on ``y``.  The measure is
# ``branch_db(dx, dy, dx64, dy64)``; a parameter gradient is measured with ``agreement_db`` against its float64 gradient; the reference is
# float64 ``torch.autograd`` over the oracle; ``floor_db`` is float32 autograd against it on the very case, one figure per tensor, and
# ``floor_x3_db`` the float64 backward through the split products (``_MMx3``), rounded to float32.  ``bar()`` is unchanged.
#
# A tensor whose float64 gradient is (next to) nothing - max-abs <= ZERO_REL x the largest parameter-gradient max-abs of the block in that
# case - has no agreement to measure: the STRUCTURAL_ZERO biases of tests/test_train_gpu.py (float32 against float64 autograd reads
# -175 dB there) and the tensors a family makes exactly zero (``zeros``: the weight of a LayerNorm whose input rows are all zero).  It is
# judged on magnitude, ``max|g| <= MAG_TOL x scale``, the rule agree_grad of tests/test_train_gpu.py uses.  With ``dy = zeros`` every
# gradient and ``dx`` must be exactly 0.
# ======================================================================================================================
ZERO_REL = 1e-9
MAG_TOL = 1e-3
STRUCTURAL_ZERO = ("linear_k.bias", "dw_conv_1d.bias", "cla.linear2.bias", "down_conv.bias")    # tests/test_train_gpu.py's list (the CPU test compares)
BWD_X_FAMILIES = ["randn", "plus100"]                                # the x families every hard dy family runs against
BWD_DY_FAMILIES = ["row_range", "silent_rows", "loud", "zeros"]
BWD_PAIRS: List[Tuple[str, str]] = [(xf, "randn") for xf in ROW_FAMILIES] + [(xf, df) for df in BWD_DY_FAMILIES for xf in BWD_X_FAMILIES]
BWD_PAIRS_LARGE: List[Tuple[str, str]] = [(xf, "randn") for xf in WORST_FLOORS]
PE_K = "separator.pos_emb.pe_k.weight"
BWD_KIND = {"gcfn_train": "gcfn", "cla_train": "cla", "ega_train": "ega", "spkattn_train": "spkattn", "down_train": "down", "split": "split", "fuse": "fuse"}

# the shapes tests/test_train_gpu.py already names (milliseconds each on the device) ...
BWD_CASES: List[Case] = (
    [Case("gcfn_train", BWD_PAIRS, n=n, T=T) for n, T in ((2, 37), (3, 300), (1, 1))]
    + [Case("cla_train", BWD_PAIRS, n=n, T=T) for n, T in ((2, 24), (2, 150), (3, 700))]         # below the 65-tap window, one tile, several
    + [Case("ega_train", BWD_PAIRS, n=2, fac=f, Tp=Tp) for f, Tp in ((1, 25), (4, 30), (2, 130), (16, 9))]   # Tp 130 > tiny's maxlen 40
    + [Case("spkattn_train", BWD_PAIRS, B=3, T=33)]
    + [Case("down_train", BWD_PAIRS, n=2, T=T) for T in (40, 41, 6)]
    + [Case("split", BWD_PAIRS, B=3, T=129), Case("fuse", BWD_PAIRS, B=2, T=24)]
)
# ... and one several-tile shape per residual block on randn and the three lowest floors
BWD_LARGE_CASES: List[Case] = [Case("gcfn_train", BWD_PAIRS_LARGE, n=3, T=2731), Case("cla_train", BWD_PAIRS_LARGE, n=2, T=2100),
                               Case("ega_train", BWD_PAIRS_LARGE, n=2, fac=8, Tp=300)]


def param_prefixes(case: Case, cfg) -> Tuple[str, ...]:
    """The state-dict prefixes of the parameters ``case`` has gradients for (the prefix check_param_grads of tests/test_train_gpu.py is given)."""
    k = BWD_KIND[case.kind]
    if k == "split":
        return ("separator.spk_split_blocks.0." if cfg.per_level_split else "separator.spk_split_block.",)
    return {"gcfn": (E0 + ".g_block_1.block.gcfn.",), "cla": (E0 + ".l_block_1.block.cla.",), "ega": (E0 + ".g_block_1.block.ega.", PE_K),
            "spkattn": (D0 + ".spk_attn_1.self_attn.",), "down": (E0 + ".downconv.",), "fuse": ("separator.simple_fusion.0.",)}[k]


def dy_shape(case: Case, cfg):
    k, s = BWD_KIND[case.kind], case.shape
    F, S = cfg.feat, cfg.num_spks
    if k in ("gcfn", "cla"):
        return (s["n"], s["T"], F)
    if k == "ega":
        return (s["n"], s["Tp"] * s["fac"], F)
    if k == "down":
        K = cfg.down_kernel
        return (s["n"], (s["T"] + 2 * ((K - 1) // 2) - K) // 2 + 1, F)
    if k == "split":
        return (s["B"] * S, s["T"], F)
    return (s["B"] * S, s["T"], F)                                    # spkattn, fuse


def make_dy(case: Case, cfg, family: str) -> torch.Tensor:
    """The output gradient of ``case`` (channel-last, float32) from ``input_families`` under a seed of its own."""
    seed = 500 + sum(ord(ch) for ch in case.tag) % 991
    return input_families(dy_shape(case, cfg), seed)[family]


_DX_NAME = {"x": "dx", "lo": "dlo", "sk": "dskip"}


def reference_bwd(case: Case, variant: str, sd_dtype, inp, dy):
    """``torch.autograd`` over the oracle call ``reference()`` makes for the kind: ({"dx": ...} in the device's channel-last layout
    (fuse: "dlo" and "dskip"), the residual term of ``dx`` (``dy``, or None for a block without a residual), {state-dict key: gradient})."""
    from oracle import train_oracle as tor
    cfg = VARIANTS[variant]
    pre = param_prefixes(case, cfg)
    sdl = tor.leaf_state({k: v for k, v in state(variant).items() if k.startswith(pre)}, sd_dtype)   # the block's own entries: all its call reads
    t = {k: v.to(sd_dtype).clone().requires_grad_(True) for k, v in inp.items()}
    dyt = dy.to(sd_dtype)
    with torch.enable_grad():
        y, res = _forward(case, variant, sdl, t)
        y.backward(dyt)
    grads = {k: v.grad for k, v in sdl.items() if v.requires_grad and v.grad is not None}
    return {_DX_NAME[k]: v.grad for k, v in t.items()}, (None if res is None else dyt), grads


def reference_bwd_x3(case, variant, inp, dy):
    """The float64 backward through the bf16 hi+lo products (forward and backward), every result rounded to float32 (device storage)."""
    with x3_context():
        dx, res, grads = reference_bwd(case, variant, torch.float64, inp, dy)
    rnd = lambda v: v.float().double()                                # noqa: E731
    return {k: rnd(v) for k, v in dx.items()}, res, {k: rnd(v) for k, v in grads.items()}


def measure_bwd(r: dict, name: str, got) -> float:
    """The figure of tensor ``name`` of floors_bwd()'s ``r``: the branch for ``dx`` of a residual block, plain agreement otherwise."""
    if name in r["dx64"]:
        dy = r["dy"] if r["residual"] else None                      # float32, as the device received it
        return branch_db(got, dy, r["dx64"][name], None if dy is None else dy.double())
    return orc.agreement_db(got.double(), r["g64"][name])


_floor_bwd_cache: Dict[tuple, dict] = {}


def floors_bwd(case: Case, variant: str, xfam: str, dyfam: str, want_x3: bool = True) -> dict:
    """Everything the reference side says about one (case, x family, dy family): inputs, float64 ``dx64`` / ``g64``, per tensor its
    ``rule`` ("db" | "magnitude" | "zero"), ``floor_db`` and ``floor_x3_db`` (None where the rule is not "db"), and ``scale``.
    Cached; the cache holds one variant at a time (float64 gradients of the Large width are megabytes per case)."""
    key = (case.tag, variant, xfam, dyfam)
    got = _floor_bwd_cache.get(key)
    if got is None:
        for old in [q for q in _floor_bwd_cache if q[1] != variant]:
            del _floor_bwd_cache[old]
        cfg = VARIANTS[variant]
        inp, dy = make_inputs(case, cfg, xfam), make_dy(case, cfg, dyfam)
        dx64, res, g64 = reference_bwd(case, variant, torch.float64, inp, dy)
        got = {"inp": inp, "dy": dy, "residual": res is not None, "dx64": dx64, "g64": g64,
               "finite": all(bool(torch.isfinite(v).all()) for v in list(dx64.values()) + list(g64.values())),
               "scale": max(float(v.abs().max()) for v in g64.values()), "rule": {}, "floor_db": {}, "floor_x3_db": None}
        if float(dy.abs().max()) == 0.0:
            got["rule"] = {n: "zero" for n in list(dx64) + list(g64)}
            got["floor_db"] = {n: None for n in got["rule"]}
        else:
            dx32, _, g32 = reference_bwd(case, variant, torch.float32, inp, dy)
            got["g32_max"] = {n: float(v.abs().max()) for n, v in g32.items()}
            for n, v in list(dx32.items()) + list(g32.items()):
                small = n in g64 and (n.endswith(STRUCTURAL_ZERO) or float(g64[n].abs().max()) <= ZERO_REL * got["scale"])
                got["rule"][n] = "magnitude" if small else "db"
                got["floor_db"][n] = None if small else measure_bwd(got, n, v)
        _floor_bwd_cache[key] = got
    if want_x3 and got["floor_x3_db"] is None:
        if all(rule != "db" for rule in got["rule"].values()):
            got["floor_x3_db"] = {n: None for n in got["rule"]}
        else:
            dx3, _, g3 = reference_bwd_x3(case, variant, got["inp"], got["dy"])
            got["floor_x3_db"] = {n: (measure_bwd(got, n, v) if got["rule"][n] == "db" else None) for n, v in list(dx3.items()) + list(g3.items())}
    return got


# ----------------------------------------------------------------------------------------------------------------------
# backward mutants: the oracle's exact forward with ONE planted defect in the gradient.  Each is a torch.autograd.Function whose backward
# asks plain autograd for the gradient of the very op (so with the defect off it is bit-identical to the oracle's own backward, checked
# by the CPU test) and then spoils it the way a kernel would.
# ----------------------------------------------------------------------------------------------------------------------
def _grad_of(fn, inputs, dy):
    """Plain autograd of ``fn`` at ``inputs`` (detached) for the output gradient ``dy``."""
    with torch.enable_grad():
        leaves = [a.detach().requires_grad_(True) for a in inputs]
        return torch.autograd.grad(fn(*leaves), leaves, dy)


class _LNBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, drop_term, eps_bwd):
        ctx.save_for_backward(x, w, b)
        ctx.defect = (drop_term, eps_bwd)
        return TF.layer_norm(x, (w.shape[0],), w, b, 1e-5)

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        drop_term, eps = ctx.defect
        dx, dw, db = _grad_of(lambda x_, w_, b_: TF.layer_norm(x_, (w.shape[0],), w_, b_, eps), (x, w, b), dy)
        if drop_term:                                                 # dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w: the last term is lost
            xc = x - x.mean(-1, keepdim=True)
            rstd = torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + 1e-5)
            xhat = xc * rstd
            dx = dx + rstd * xhat * (dy * w * xhat).mean(-1, keepdim=True)
        return dx, dw, db, None, None


def _ln_bwd(drop_term=False, eps_bwd=1e-5):
    return lambda sd, p, x: _LNBwd.apply(x, sd[p + ".weight"], sd[p + ".bias"], drop_term, eps_bwd)


class _SoftmaxBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, dim, no_rowsum):
        ctx.save_for_backward(s)
        ctx.dim, ctx.no_rowsum = dim, no_rowsum
        return torch.softmax(s, dim=dim)

    @staticmethod
    def backward(ctx, dy):
        (s,) = ctx.saved_tensors
        (ds,) = _grad_of(lambda s_: torch.softmax(s_, dim=ctx.dim), (s,), dy)
        if ctx.no_rowsum:                                             # ds = p (dy - sum(dy p)): the row sum is not subtracted
            p = torch.softmax(s, dim=ctx.dim)
            ds = ds + p * (dy * p).sum(ctx.dim, keepdim=True)
        return ds, None, None


def _softmax_bwd(no_rowsum=False):
    return lambda s, dim=-1: _SoftmaxBwd.apply(s, dim, no_rowsum)


class _BNBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, rm, rv, training, const_stats):
        ctx.save_for_backward(x, w, b, rm.clone(), rv.clone())
        ctx.training, ctx.const_stats = training, const_stats
        return TF.batch_norm(x, rm, rv, w, b, training, 0.1, 1e-5)   # (train mode: updates rm / rv in place, as the oracle's call does)

    @staticmethod
    def backward(ctx, dy):
        x, w, b, rm, rv = ctx.saved_tensors
        dx, dw, db = _grad_of(lambda x_, w_, b_: TF.batch_norm(x_, rm.clone(), rv.clone(), w_, b_, ctx.training, 0.1, 1e-5), (x, w, b), dy)
        if ctx.const_stats and ctx.training:                          # batch mean and variance taken as constants: dx = dy w rstd
            dims = [d for d in range(x.dim()) if d != 1]
            rstd = torch.rsqrt(x.var(dims, unbiased=False, keepdim=True) + 1e-5)
            dx = dy * w.view(1, -1, *([1] * (x.dim() - 2))) * rstd
        return dx, dw, db, None, None, None, None


def _bn_bwd(const_stats=False):
    return lambda sd, p, x: _BNBwd.apply(x, sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"],
                                         orc.BN_TRAINING, const_stats)


class _DW3Bwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, halo_lost):
        ctx.save_for_backward(x, w, b)
        ctx.halo_lost = halo_lost
        return TF.conv1d(x, w, b, padding=1, groups=x.shape[1])

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dx, dw, db = _grad_of(lambda x_, w_, b_: TF.conv1d(x_, w_, b_, padding=1, groups=x.shape[1]), (x, w, b), dy)
        if ctx.halo_lost and x.shape[-1] > 128:                       # y[128] = w0 x[127] + ...: frame 127 of sequence 0 loses dy[128] w0
            dx = dx.clone()
            dx[0, :, 127] -= w[:, 0, 0] * dy[0, :, 128]
        return dx, dw, db, None


def _dw3_bwd(halo_lost=False):
    def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups == x.shape[1] and groups > 1 and w.shape[-1] == 3 and b is not None and stride == 1 and padding == 1:   # GCFN's 3-tap depthwise
            return _DW3Bwd.apply(x, w, b, halo_lost)
        return TF.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=groups)
    return conv1d


class _UpBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, last_lost):
        ctx.save_for_backward(x)
        ctx.size, ctx.last_lost = size, last_lost
        return TF.interpolate(x, size=size, mode="nearest")

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        (dx,) = _grad_of(lambda x_: TF.interpolate(x_, size=ctx.size, mode="nearest"), (x,), dy)
        fac = ctx.size // x.shape[-1]
        if ctx.last_lost and fac > 1 and fac * x.shape[-1] == ctx.size:   # dx[i] = sum of dy over i's fac frames: the last one is left out
            dx = dx - dy[..., fac - 1::fac]
        return dx, None, None


def _up_bwd(last_lost=False):
    return lambda x, size=None, mode="nearest": _UpBwd.apply(x, size, last_lost)


class _PoolBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_len, wrong_count):
        ctx.save_for_backward(x)
        ctx.out_len, ctx.wrong_count = out_len, wrong_count
        return TF.adaptive_avg_pool1d(x, out_len)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        (dx,) = _grad_of(lambda x_: TF.adaptive_avg_pool1d(x_, ctx.out_len), (x,), dy)
        if ctx.wrong_count:                                           # the last window hands dy / (fac + 1) to its frames
            fac = x.shape[-1] // ctx.out_len
            dx = dx.clone()
            dx[..., x.shape[-1] - fac:] *= fac / (fac + 1.0)
        return dx, None, None


def _pool_bwd(wrong_count=False):
    return lambda x, out_len: _PoolBwd.apply(x, out_len, wrong_count)


class _PosKBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, t, maxlen, drop_clamped):
        pos = torch.arange(0, t).long()
        raw = pos[:, None] - pos[None, :]
        ctx.save_for_backward(w)
        ctx.idx = raw.clamp(-maxlen, maxlen - 1) + maxlen
        ctx.inside = ((raw >= -maxlen) & (raw <= maxlen - 1)) if drop_clamped else None
        return TF.embedding(ctx.idx, w)

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        if ctx.inside is not None:                                    # pairs beyond the clamp are dropped instead of adding into the edge rows
            dy = dy * ctx.inside[..., None].to(dy.dtype)
        (dw,) = _grad_of(lambda w_: TF.embedding(ctx.idx, w_), (w,), dy)
        return dw, None, None, None


def _pos_k_bwd(drop_clamped=False):
    return lambda sd, t, maxlen: _PosKBwd.apply(sd[PE_K], t, maxlen, drop_clamped)


class _LinBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, last_row_lost):
        ctx.save_for_backward(x, w, b)
        ctx.last_row_lost = last_row_lost
        return TF.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dx, dw, db = _grad_of(TF.linear, (x, w, b), dy)
        if ctx.last_row_lost:                                         # the weight gradient leaves out the last row of the flattened batch
            dw = dw - torch.outer(dy.reshape(-1, dy.shape[-1])[-1], x.reshape(-1, x.shape[-1])[-1])
        return dx, dw, db, None


def _lin_bwd(last_row_lost=False):
    return lambda sd, p, x: _LinBwd.apply(x, sd[p + ".weight"], sd[p + ".bias"], last_row_lost)


_ATTN = {"ega_train", "spkattn_train"}
_LN_KINDS = {"gcfn_train", "cla_train", "ega_train", "spkattn_train"}


def bwd_mutants() -> Dict[str, dict]:
    """name -> {"ctx": () -> context that plants the defect, "off": the same Function with the defect off, "kinds": the kinds it can touch}."""
    tf = lambda **kw: patched(TF=_Proxy(TF, **kw))                     # noqa: E731
    return {
        "ln_bwd_xhat_term_lost": {"ctx": lambda: patched(_ln=_ln_bwd(drop_term=True)), "off": lambda: patched(_ln=_ln_bwd()), "kinds": _LN_KINDS},
        "ln_bwd_eps_1e-6": {"ctx": lambda: patched(_ln=_ln_bwd(eps_bwd=1e-6)), "off": lambda: patched(_ln=_ln_bwd()), "kinds": _LN_KINDS},
        "softmax_bwd_no_rowsum": {"ctx": lambda: patched(torch=_Proxy(torch, softmax=_softmax_bwd(True))),
                                  "off": lambda: patched(torch=_Proxy(torch, softmax=_softmax_bwd())), "kinds": _ATTN},
        "bn_bwd_stats_constant": {"ctx": lambda: patched(_bn_eval=_bn_bwd(True)), "off": lambda: patched(_bn_eval=_bn_bwd()),
                                  "kinds": {"cla_train", "down_train"}},
        "dwconv_bwd_halo_lost": {"ctx": lambda: tf(conv1d=_dw3_bwd(True)), "off": lambda: tf(conv1d=_dw3_bwd()), "kinds": {"gcfn_train"}},
        "upsample_bwd_last_lost": {"ctx": lambda: tf(interpolate=_up_bwd(True)), "off": lambda: tf(interpolate=_up_bwd()),
                                   "kinds": {"ega_train", "fuse"}},
        "avgpool_bwd_wrong_count": {"ctx": lambda: tf(adaptive_avg_pool1d=_pool_bwd(True)), "off": lambda: tf(adaptive_avg_pool1d=_pool_bwd()),
                                    "kinds": {"ega_train"}},
        "pe_k_grad_clamped_dropped": {"ctx": lambda: patched(rel_pos_k=_pos_k_bwd(True)), "off": lambda: patched(rel_pos_k=_pos_k_bwd()),
                                      "kinds": {"ega_train"}},
        "wgrad_last_row_lost": {"ctx": lambda: patched(_lin=_lin_bwd(True)), "off": lambda: patched(_lin=_lin_bwd()), "kinds": _LN_KINDS},
    }
