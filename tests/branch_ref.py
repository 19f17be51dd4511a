"""Branch parity: what the block tests measure once the residual is taken out, against a float64 reference, on hard inputs.
Shared by tests/test_branch_parity_cpu.py (the proof that the bar has teeth, reference side only) and
tests/test_branch_parity_gpu.py (the device against the same cases).  Test infrastructure only.

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
    cfg = VARIANTS[variant]
    F, H, S = cfg.feat, cfg.heads, cfg.num_spks
    dt = sd["separator.pos_emb.pe_k.weight"].dtype
    t = {k: v.to(dt) for k, v in inp.items()}
    k, s = case.kind, case.shape
    with torch.no_grad():
        if k in ("gcfn", "gcfn_train"):
            return orc.gcfn(sd, E0 + ".g_block_1.block.gcfn", t["x"]), t["x"]
        if k == "cla":
            return orc.cla(sd, E0 + ".l_block_1.block.cla", t["x"]), t["x"]
        if k == "cla_train":                                             # train-mode BatchNorm: batch statistics (and an in-place update
            p = E0 + ".l_block_1.block.cla.BN."                          # of the running ones: on a copy)
            sdc = dict(sd)
            for name in ("running_mean", "running_var", "num_batches_tracked"):
                if p + name in sdc:
                    sdc[p + name] = sdc[p + name].clone()
            orc.BN_TRAINING = True
            try:
                return orc.cla(sdc, E0 + ".l_block_1.block.cla", t["x"]), t["x"]
            finally:
                orc.BN_TRAINING = False
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
    """Replace module globals of the oracle (``TF``, ``torch``, ``mha``, ``_ln``, ``_lin``, ``rel_pos_k``) for the duration."""
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


def _mm_x3(a, b):
    ah, al = _split(a)
    bh, bl = _split(b)
    return torch.matmul(ah, bh) + torch.matmul(ah, bl) + torch.matmul(al, bh)


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
