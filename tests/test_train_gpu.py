"""Training path on the device against the train-mode oracle (torch.autograd over the CPU restatement,
pinned to the imported reference by tests/golden/make_train_golden.py: every one of the 710 gradient tensors identical).

Tolerances (floating point): every forward output and every gradient tensor must agree with the oracle to >= MIN_DB
(80 dB, the same bar as the inference parity tests; exact-f32 mode is held to 100 dB where noted).  All measured values go
to gpurun_out/train_parity_report.json.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import criterion_oracle as co
from oracle import sepreformer_oracle as orc
from oracle import train_oracle as tor
from sepreformer_amd import lib as L
from sepreformer_amd.config import VARIANTS
from sepreformer_amd.synth import synth_sources, synth_state_dict

pytestmark = pytest.mark.gpu
# Round 6 (suite-time budget: the driver runs the whole -m gpu suite in one process under a 1 200 s limit; the CPU oracle's fp32 forward +
# backward is what the long tests spend): cases that a cheaper test of the same round now covers run only with SEPR_SLOW_TESTS=1.
slow = pytest.mark.skipif(os.environ.get("SEPR_SLOW_TESTS", "0") != "1", reason="superseded long case: set SEPR_SLOW_TESTS=1 to run it")
_FROZEN_ORACLE = {}        # (B, T, seed) -> the oracle's step with the auxiliary gates of the FIRST device forward that asked for it
MIN_DB = 80.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
PRECISIONS = ["fp32", "bf16x3"]
# "bf16" = plain bf16 operands (one MFMA per product, fp32 accumulate / master weights: BASELINE configs[4]'s precision).  Operand
# rounding is 2^-9 relative (~54 dB per product), so its bar against the fp32 oracle is BF16_DB, and every measured value is recorded.
PRECISIONS_T = PRECISIONS + ["bf16"]
BF16_DB = 35.0


def record(name, db):
    v = float(db)
    # dB figures keep two decimals; small magnitudes (PIT SI-SNR deltas, ~1e-4 dB against a 1e-3 gate) keep three significant digits
    REPORT[name] = round(v, 2) if abs(v) >= 1.0 or v == 0.0 else float(f"{v:.3e}")
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "train_parity_report.json")
    merged = {}
    if os.path.exists(path):
        try:
            with open(path) as f:
                merged = json.load(f)
        except ValueError:
            merged = {}
    merged.update(REPORT)
    with open(path, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)


class Soft:
    """Collects every disagreement of a test so that one device run shows all of them."""

    def __init__(self, tag, precision=None):
        self.tag, self.bad = tag, []
        self.cap = BF16_DB if precision == "bf16" else None     # plain-bf16 arithmetic: every bar is capped at BF16_DB

    def agree(self, name, got, want, min_db=MIN_DB):
        if self.cap is not None:
            min_db = min(min_db, self.cap)
        got = got.detach().float().cpu()
        want = want.detach().float().cpu()
        if got.shape != want.shape:
            self.bad.append(f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}")
            return
        if not torch.isfinite(got).all():
            self.bad.append(f"{name}: non-finite values")
            record(f"{self.tag}.{name}", -999)
            return
        db = orc.agreement_db(got, want) if float(want.abs().max()) > 0 else (999.0 if float(got.abs().max()) == 0 else -999.0)
        record(f"{self.tag}.{name}", db)
        if db < min_db:
            self.bad.append(f"{name}: {db:.1f} dB < {min_db}")

    def done(self):
        assert not self.bad, f"[{self.tag}] " + "; ".join(self.bad[:40])


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def cl(x):  # [b, C, T] -> channel-last device tensor
    return x.permute(0, 2, 1).contiguous().cuda()


def cf(y):  # channel-last device tensor -> [b, C, T] host
    return y.detach().cpu().permute(0, 2, 1)


_cache = {}


def setup(variant, precision):
    """TrainEngine + TrainPack + GradBuffer over the synthetic weights of `variant` (dropout 0), and the host state_dict."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    key = (variant, precision)
    if key not in _cache:
        cfg = dataclasses.replace(VARIANTS[variant], dropout=0.0)
        sd = synth_state_dict(cfg, 0)
        dev = torch.device("cuda:0")
        sdd = {k: v.to(dev) for k, v in sd.items()}
        gb = GradBuffer(cfg, dev)
        tp = TrainPack(cfg, sdd, gb, precision)
        _cache[key] = (cfg, sd, sdd, gb, tp, TrainEngine(cfg, dev))
    cfg, sd, sdd, gb, tp, eng = _cache[key]
    gb.flat.zero_()
    return cfg, sd, sdd, gb, tp, eng


# Parameters whose gradient is identically zero in exact arithmetic: a bias in front of a train-mode BatchNorm (the batch mean
# removes it: CLA dw_conv_1d.bias and linear2.bias, DownConv down_conv.bias) and the key bias of an attention (softmax is
# invariant to a per-query constant).  Autograd and the HIP backward both return rounding noise there, so the check is on
# magnitude (noise << the gradients that matter), not on agreement.
STRUCTURAL_ZERO = ("linear_k.bias", "dw_conv_1d.bias", "cla.linear2.bias", "down_conv.bias")


def agree_grad(soft, name, key, got, want, scale, min_db=MIN_DB):
    if key.endswith(STRUCTURAL_ZERO):
        noise_ref, noise_got = float(want.detach().abs().max()), float(got.detach().abs().max())
        record(f"{soft.tag}.{name}.structural_zero_rel", noise_got / (scale + 1e-30))
        tol = 3e-2 if soft.cap is not None else 1e-3        # plain bf16 operands: the rounding noise is 2^-9 of the terms
        if not (noise_ref <= 1e-3 * scale):
            soft.bad.append(f"{name}: reference gradient {noise_ref:.2e} is not ~0 against scale {scale:.2e}")
        if not (noise_got <= tol * scale):
            soft.bad.append(f"{name}: gradient {noise_got:.2e} should be ~0 against scale {scale:.2e}")
        return
    soft.agree(name, got, want, min_db)


def check_param_grads(soft, gb, sdl, prefix, min_db=MIN_DB):
    items = [(k, v) for k, v in sdl.items() if k.startswith(prefix) and v.requires_grad and v.grad is not None]
    assert items, prefix
    scale = max(float(v.grad.abs().max()) for _, v in items)
    for k, v in items:
        agree_grad(soft, "grad." + k[len(prefix):].lstrip("."), k, gb.view(k), v.grad, scale, min_db)


# ---------------------------------------------------------------------------------------------------------------------
# the weight-gradient contraction on its own
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(1000, 128, 128), (4099, 768, 128), (257, 64, 512), (5000, 256, 16), (130, 192, 64), (33, 128, 384),
                                   (70000, 128, 384), (1, 64, 64)])
def test_wgrad_core(M, N, K, x3):
    lib = L.load()
    a, b = rnd(M, N, seed=1), rnd(M, K, seed=2)
    ad, bd = a.cuda(), b.cuda()
    G = torch.full((N, K), 7.0, device="cuda")
    cs = torch.full((N,), -3.0, device="cuda")
    ws = torch.empty(int(lib.sepr_linear_wgrad_workspace(M, N, K)) + 256, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.sepr_linear_wgrad(ad.data_ptr(), bd.data_ptr(), G.data_ptr(), cs.data_ptr(), M, N, K, 0, x3, ws.data_ptr(), ws.numel(), st), "wgrad")
    want = (a.double().t() @ b.double()).float()
    soft = Soft(f"wgrad.{M}x{N}x{K}.{['f32', 'x3', 'bf16'][x3]}")
    g_db = [110.0, 85.0, 40.0][x3]                      # plain bf16 operands: 2^-9 rounding of both factors
    soft.agree("G", G, want, g_db)
    soft.agree("colsum", cs, a.double().sum(0).float(), 110.0)
    # accumulate on top, and bitwise reproducibility (no atomics)
    G2 = G.clone()
    L.check(lib.sepr_linear_wgrad(ad.data_ptr(), bd.data_ptr(), G2.data_ptr(), cs.data_ptr(), M, N, K, 1, x3, ws.data_ptr(), ws.numel(), st), "wgrad")
    soft.agree("G_accumulated", G2, 2 * want, g_db)
    G3 = torch.empty_like(G)
    L.check(lib.sepr_linear_wgrad(ad.data_ptr(), bd.data_ptr(), G3.data_ptr(), None, M, N, K, 0, x3, ws.data_ptr(), ws.numel(), st), "wgrad")
    assert torch.equal(G3, G)
    soft.done()


@pytest.mark.parametrize("M,N,K,lda,ldb", [(256, 128, 128, 128, 128), (4099, 768, 128, 768, 128), (8191, 128, 384, 128, 384), (33, 128, 128, 128, 128),
                                           (31, 256, 128, 256, 128), (1000, 128, 128, 384, 256), (70000, 768, 128, 768, 128), (256000, 128, 384, 128, 384),
                                           (5000, 192, 128, 192, 128)])
def test_wgrad_bf16_operands(M, N, K, lda, ldb, monkeypatch):
    """The contraction of two bf16 operands (sepr_linear_wgrad_bf16: what the plain-bf16 precision runs for the GCFN / CLA weight gradients)
    on gemm_tn16_kernel - LDS-DMA ring, transposing LDS reads, column sums on the matrix pipe - against fp64 of the same bf16 values: whole
    and ragged last slabs (M % 32), a tensor shorter than one slab, strided operands (lda > N), 500 row slices; and against the
    register-staged kernel (SEPR_TN16=0: exactly the same products, fp32 sums in another order).  N = 192 is not a whole tile: that launch
    stays on the register-staged kernel whatever the switch says."""
    lib = L.load()
    g = torch.Generator().manual_seed(M + N)
    a = (torch.randn(M, lda, generator=g) * (1 + torch.arange(lda) % 7)).to(torch.bfloat16)
    b = (torch.randn(M, ldb, generator=g) + 0.25).to(torch.bfloat16)
    ad, bd = a.cuda(), b.cuda()
    want = (a[:, :N].double().t() @ b[:, :K].double()).float()
    want_cs = a[:, :N].double().sum(0).float()
    ws = torch.empty(int(lib.sepr_linear_wgrad_workspace(M, N, K)) + 256, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    soft = Soft(f"wgrad_bf16.{M}x{N}x{K}")
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SEPR_TN16", mode)
        G = torch.full((N, K), 7.0, device="cuda")
        cs = torch.full((N,), -3.0, device="cuda")
        L.check(lib.sepr_linear_wgrad_bf16(ad.data_ptr(), lda, bd.data_ptr(), ldb, G.data_ptr(), cs.data_ptr(), M, N, K, 0, ws.data_ptr(), ws.numel(), st), "wgrad_bf16")
        soft.agree(f"G.tn16={mode}", G, want, 110.0)           # the bf16 values are the inputs here: only the fp32 summation order is left
        soft.agree(f"colsum.tn16={mode}", cs, want_cs, 110.0)
        G2 = G.clone()
        cs2 = cs.clone()
        L.check(lib.sepr_linear_wgrad_bf16(ad.data_ptr(), lda, bd.data_ptr(), ldb, G2.data_ptr(), cs2.data_ptr(), M, N, K, 1, ws.data_ptr(), ws.numel(), st), "wgrad_bf16")
        soft.agree(f"G_accumulated.tn16={mode}", G2, 2 * want, 110.0)
        soft.agree(f"colsum_accumulated.tn16={mode}", cs2, 2 * want_cs, 110.0)
        G3 = torch.empty_like(G)
        L.check(lib.sepr_linear_wgrad_bf16(ad.data_ptr(), lda, bd.data_ptr(), ldb, G3.data_ptr(), None, M, N, K, 0, ws.data_ptr(), ws.numel(), st), "wgrad_bf16")
        assert torch.equal(G3, G)                              # no atomics: bitwise repeatable
        res[mode] = G
    soft.agree("G.tn16_vs_staged", res["1"], res["0"], 110.0)
    soft.done()


@pytest.mark.parametrize("x3", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(64000, 768, 128), (20000, 256, 128), (300000, 128, 128), (777, 384, 128)])
def test_wgrad_norm_full_size(M, N, K, x3):
    """The contraction behind a LayerNorm (normalisation prologue from per-row statistics) at the launch sizes of a 4 s batch:
    two workgroups per CU, dozens of row slices.  Round 3 found the first version of this path returning wrong (1e-2 relative),
    run-to-run different values in its bf16 instantiations exactly there - no test went beyond 8000 rows.  Checked against fp64
    and for bitwise repeatability."""
    lib = L.load()
    g = torch.Generator().manual_seed(M)
    a, b = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g) * 2 + 0.5
    mean, rstd = b.mean(1), 1.0 / torch.sqrt(b.var(1, unbiased=False) + 1e-5)
    want = (a.double().t() @ ((b.double() - mean.double()[:, None]) * rstd.double()[:, None])).float()
    ad, bd, sd_ = a.cuda(), b.cuda(), torch.stack([mean, rstd], 1).contiguous().cuda()
    ws = torch.empty(int(lib.sepr_linear_wgrad_workspace(M, N, K)) + 256, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(3):
        G = torch.empty(N, K, device="cuda")
        cs = torch.empty(N, device="cuda")
        L.check(lib.sepr_linear_wgrad_norm(ad.data_ptr(), bd.data_ptr(), sd_.data_ptr(), G.data_ptr(), cs.data_ptr(), M, N, K, 0, x3,
                                           ws.data_ptr(), ws.numel(), st), "wgrad_norm")
        outs.append((G, cs))
    soft = Soft(f"wgrad_norm.{M}x{N}x{K}.{['f32', 'x3', 'bf16'][x3]}")
    soft.agree("G", outs[0][0], want, [110.0, 85.0, 40.0][x3])
    soft.agree("colsum", outs[0][1], a.double().sum(0).float(), 110.0)
    assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    soft.done()


# ---------------------------------------------------------------------------------------------------------------------
# every block: train-mode forward and backward against autograd over the oracle's restatement of the same module
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_VARIANTS = ["tiny", "SepReformer_Base_WSJ0", "SepReformer_Large_DM_WHAMR"]   # F = 16 / 128 / 256 (dk = 32, generic GCFN pair)


@pytest.mark.parametrize("precision", PRECISIONS_T)
@pytest.mark.parametrize("variant", BLOCK_VARIANTS)
def test_gcfn_train(variant, precision):
    cfg, sd, sdd, gb, tp, eng = setup(variant, precision)
    F = cfg.feat
    soft = Soft(f"{variant}.{precision}.gcfn", precision)
    p = "separator.enc_stages.0.g_block_1.block.gcfn"
    for n, T in ((2, 37), (3, 300), (1, 1)):
        gb.flat.zero_()
        x, dy = rnd(n, T, F, seed=T), rnd(n, T, F, seed=T + 7)
        y, rec = eng.block_fwd("gcfn", x.cuda(), tp.gcfn[0], n, T)
        dx = eng.block_bwd(rec, dy.cuda())
        sdl = tor.leaf_state(sd)
        xl = x.clone().requires_grad_(True)
        yo = orc.gcfn(sdl, p, xl)
        yo.backward(dy)
        soft.agree(f"T{T}.y", y, yo)
        soft.agree(f"T{T}.dx", dx, xl.grad)
        check_param_grads(soft, gb, sdl, p)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS_T)
@pytest.mark.parametrize("variant", BLOCK_VARIANTS)
def test_cla_train(variant, precision):
    cfg, sd, sdd, gb, tp, eng = setup(variant, precision)
    F = cfg.feat
    soft = Soft(f"{variant}.{precision}.cla", precision)
    p = "separator.enc_stages.0.l_block_1.block.cla"
    for n, T in ((2, 24), (2, 150), (3, 700)):
        gb.flat.zero_()
        sdd[p + ".BN.running_mean"].copy_(sd[p + ".BN.running_mean"])       # (shared device state: see test_cla_train_full_size)
        sdd[p + ".BN.running_var"].copy_(sd[p + ".BN.running_var"])
        rm0, rv0 = sdd[p + ".BN.running_mean"].clone(), sdd[p + ".BN.running_var"].clone()
        x, dy = rnd(n, T, F, seed=T), rnd(n, T, F, seed=T + 7)
        y, rec = eng.block_fwd("cla", x.cuda(), tp.cla[0], n, T)
        dx = eng.block_bwd(rec, dy.cuda())
        sdl = tor.leaf_state(sd)
        xl = x.clone().requires_grad_(True)
        orc.BN_TRAINING = True
        try:
            yo = orc.cla(sdl, p, xl)
        finally:
            orc.BN_TRAINING = False
        yo.backward(dy)
        soft.agree(f"T{T}.y", y, yo)
        soft.agree(f"T{T}.dx", dx, xl.grad)
        check_param_grads(soft, gb, sdl, p)
        soft.agree(f"T{T}.running_mean", sdd[p + ".BN.running_mean"], sdl[p + ".BN.running_mean"], 100.0)
        soft.agree(f"T{T}.running_var", sdd[p + ".BN.running_var"], sdl[p + ".BN.running_var"], 100.0)
        sdd[p + ".BN.running_mean"].copy_(rm0)
        sdd[p + ".BN.running_var"].copy_(rv0)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS_T)
@pytest.mark.parametrize("variant", BLOCK_VARIANTS)
def test_ega_train(variant, precision):
    cfg, sd, sdd, gb, tp, eng = setup(variant, precision)
    F, H = cfg.feat, cfg.heads
    soft = Soft(f"{variant}.{precision}.ega", precision)
    p = "separator.enc_stages.0.g_block_1.block.ega"
    for fac, Tp in ((1, 25), (4, 30), (2, 130), (16, 9)):      # Tp 130 > tiny's maxlen 40: clamped relative positions
        gb.flat.zero_()
        T = Tp * fac
        x, dy = rnd(2, F, T, seed=fac), rnd(2, T, F, seed=fac + 7)
        y, rec = eng.block_fwd("ega", cl(x), tp.ega[0], 2, T, Tp)
        dx = eng.block_bwd(rec, dy.cuda())
        sdl = tor.leaf_state(sd)
        xl = x.clone().requires_grad_(True)
        yo = orc.ega(sdl, p, xl, orc.rel_pos_k(sdl, Tp, cfg.maxlen), H)
        yo.backward(dy)
        soft.agree(f"fac{fac}.Tp{Tp}.y", y, yo)
        soft.agree(f"fac{fac}.Tp{Tp}.dx", cf(dx), xl.grad)
        check_param_grads(soft, gb, sdl, p)
        soft.agree(f"fac{fac}.Tp{Tp}.grad.pe_k", gb.view("separator.pos_emb.pe_k.weight"), sdl["separator.pos_emb.pe_k.weight"].grad)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS_T)
@pytest.mark.parametrize("variant", BLOCK_VARIANTS)
def test_spkattn_train(variant, precision):
    cfg, sd, sdd, gb, tp, eng = setup(variant, precision)
    F, H, S = cfg.feat, cfg.heads, cfg.num_spks
    soft = Soft(f"{variant}.{precision}.spkattn", precision)
    p = "separator.dec_stages.0.spk_attn_1.self_attn"
    B, T = 3, 33
    x, dy = rnd(B * S, T, F, seed=5), rnd(B * S, T, F, seed=6)
    y, rec = eng.block_fwd("spk", x.cuda(), tp.spk[0], B * S, T)
    dx = eng.block_bwd(rec, dy.cuda())
    sdl = tor.leaf_state(sd)
    xl = x.clone().requires_grad_(True)
    xr = xl.view(B, S, T, F).permute(0, 2, 1, 3).reshape(B * T, S, F)          # network.py:241-243 in channel-last terms
    yr = xr + orc.mha(sdl, p, xr, None, H)                                      # :244
    yo = yr.view(B, T, S, F).permute(0, 2, 1, 3).reshape(B * S, T, F)           # :245-247
    yo.backward(dy)
    soft.agree("y", y, yo)
    soft.agree("dx", dx, xl.grad)
    check_param_grads(soft, gb, sdl, p)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", BLOCK_VARIANTS)
def test_downconv_split_fuse_train(variant, precision):
    cfg, sd, sdd, gb, tp, eng = setup(variant, precision)
    F, S = cfg.feat, cfg.num_spks
    soft = Soft(f"{variant}.{precision}.plumbing")
    # DownConv, train-mode BatchNorm (module.py:63-78)
    p = "separator.enc_stages.0.downconv"
    for T in (40, 41, 301):
        gb.flat.zero_()
        rm0, rv0 = sdd[p + ".BN.running_mean"].clone(), sdd[p + ".BN.running_var"].clone()
        x = rnd(2, T, F, seed=T)
        y, cx, To = eng.down_fwd(x.cuda(), tp.down[0], 2, T)
        dy = rnd(2, To, F, seed=T + 1)
        dx = eng.down_bwd(x.cuda(), cx, tp.down[0], dy.cuda(), 2, T)
        sdl = tor.leaf_state(sd)
        xl = x.clone().requires_grad_(True)
        orc.BN_TRAINING = True
        try:
            yo = orc.down_conv(sdl, p, xl)
        finally:
            orc.BN_TRAINING = False
        yo.backward(dy)
        soft.agree(f"down.T{T}.y", y, yo)
        soft.agree(f"down.T{T}.dx", dx, xl.grad)
        check_param_grads(soft, gb, sdl, p)
        sdd[p + ".BN.running_mean"].copy_(rm0)
        sdd[p + ".BN.running_var"].copy_(rv0)
    # SpkSplit + GroupNorm (module.py:110-125), with and without accumulation into dx
    p = "separator.spk_split_blocks.0" if cfg.per_level_split else "separator.spk_split_block"
    gb.flat.zero_()
    B, T = 3, 129
    x, dy = rnd(B, F, T, seed=9), rnd(B * S, F, T, seed=10)
    xd = cl(x)
    y, cx = eng.split_fwd(xd, tp.splits[0], B, T)
    dx = torch.empty_like(xd)
    eng.split_bwd(xd, cx, tp.splits[0], cl(dy), dx, False, B, T)
    sdl = tor.leaf_state(sd)
    xl = x.clone().requires_grad_(True)
    yo = orc.spk_split(sdl, p, xl, S)
    yo.backward(dy)
    soft.agree("split.y", cf(y), yo)
    soft.agree("split.dx", cf(dx), xl.grad)
    check_param_grads(soft, gb, sdl, p)
    base = rnd(B, T, F, seed=11).cuda()
    dx2 = base.clone()
    eng.split_bwd(xd, cx, tp.splits[0], cl(dy), dx2, True, B, T)
    soft.agree("split.dx_accumulate", dx2 - base, dx, 90.0)
    # fusion conv (module.py:212-214)
    gb.flat.zero_()
    lo, sk, dy = rnd(2 * S, F, 12, seed=12), rnd(2 * S, F, 24, seed=13), rnd(2 * S, F, 24, seed=14)
    y = eng.fuse_fwd(cl(lo), cl(sk), tp.fuse[0], 2 * S, 24)
    dlo, dsk = eng.fuse_bwd(cl(lo), cl(sk), tp.fuse[0], cl(dy), 2 * S, 24)
    sdl = tor.leaf_state(sd)
    lol, skl = lo.clone().requires_grad_(True), sk.clone().requires_grad_(True)
    up = torch.nn.functional.interpolate(lol, size=24, mode="nearest")
    yo = torch.nn.functional.conv1d(torch.cat([up, skl], 1), sdl["separator.simple_fusion.0.weight"], sdl["separator.simple_fusion.0.bias"])
    yo.backward(dy)
    soft.agree("fuse.y", cf(y), yo)
    soft.agree("fuse.dlo", cf(dlo), lol.grad)
    soft.agree("fuse.dskip", cf(dsk), skl.grad)
    check_param_grads(soft, gb, sdl, "separator.simple_fusion.0")
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", BLOCK_VARIANTS)
def test_front_and_heads_train(variant, precision):
    cfg, sd, sdd, gb, tp, eng = setup(variant, precision)
    F, S, N = cfg.feat, cfg.num_spks, cfg.enc_channels
    soft = Soft(f"{variant}.{precision}.ends")
    B, T = 3, 4 * 131 + 12
    L_ = cfg.frames(T)
    Lp = cfg.padded_frames(L_)
    wav = rnd(B, T, seed=12, scale=0.1)
    wd = wav.cuda()
    # encoder + GroupNorm + projector + pad, with an extra gradient flowing into enc (as the auxiliary heads send one)
    gb.flat.zero_()
    enc, cur, ctx = eng.front_fwd(wd, tp, B, T, L_, Lp)
    dcur, denc = rnd(B, F, Lp, seed=13), rnd(B, N, L_, seed=14)
    denc_d = cl(denc)
    eng.front_bwd(wd, enc, ctx, tp, cl(dcur), denc_d, B, T, Lp)
    sdl = tor.leaf_state(sd)
    e = orc.audio_encoder(sdl, wav, cfg.enc_stride)
    pj = orc.pad_signal(orc.feature_projector(sdl, e), cfg.num_stages)
    (pj * dcur).sum().backward(retain_graph=True)
    e.backward(denc, retain_graph=True)
    soft.agree("front.enc", cf(enc), e, 100.0)
    soft.agree("front.proj", cf(cur), pj)
    for k in ("audio_encoder.conv1d.weight", "feature_projector.norm.weight", "feature_projector.norm.bias", "feature_projector.conv1d.weight"):
        soft.agree("front.grad." + k, gb.view(k), sdl[k].grad)
    # main head: crop + OutputLayer + decoder (module.py:249-283)
    gb.flat.zero_()
    e_d = enc
    z = rnd(B * S, F, Lp, seed=15)
    zd = cl(z)
    wav_o, cx = eng.head_fwd(zd, tp.out_main, B * S, Lp, L_, None, None)
    dwav = rnd(S, B, wav_o.shape[-1], seed=16)
    dz = torch.empty_like(zd)
    eng.head_bwd(zd, cx, tp.out_main, dwav.cuda(), dz, False, None, B * S, Lp, L_, None, None)
    sdl = tor.leaf_state(sd)
    zl = z.clone().requires_grad_(True)
    e_h = e.detach()
    o = orc.output_layer(sdl, "out_layer", zl, e_h, S, False)
    want = torch.stack([orc.audio_decoder(sdl["audio_decoder.weight"], o[s], cfg.enc_stride).reshape(B, -1) for s in range(S)], 0)
    want.backward(dwav)
    soft.agree("head_main.wav", wav_o, want)
    soft.agree("head_main.dx", cf(dz), zl.grad)
    check_param_grads(soft, gb, sdl, "out_layer.")
    soft.agree("head_main.grad.decoder", gb.view("audio_decoder.weight"), sdl["audio_decoder.weight"].grad)
    # auxiliary head: nearest upsample + OutputLayer + ReLU mask x encoder + decoder (model.py:47-52), accumulating into dx / denc
    gb.flat.zero_()
    Ts = 37
    zs = rnd(B * S, F, Ts, seed=17)
    zsd = cl(zs)
    idx = eng._index(Ts, L_)
    wav_a, cx = eng.head_fwd(zsd, tp.out_aux[1], B * S, Ts, L_, idx, e_d)
    dwav = rnd(S, B, wav_a.shape[-1], seed=18)
    base_dx, base_denc = rnd(B * S, Ts, F, seed=19).cuda(), rnd(B, L_, N, seed=20).cuda()
    dzs, dencd = base_dx.clone(), base_denc.clone()
    eng.head_bwd(zsd, cx, tp.out_aux[1], dwav.cuda(), dzs, True, dencd, B * S, Ts, L_, idx, e_d)
    sdl = tor.leaf_state(sd)
    zl = zs.clone().requires_grad_(True)
    el = e.detach().clone().requires_grad_(True)
    up = torch.nn.functional.interpolate(zl, size=L_, mode="nearest")
    o = orc.output_layer(sdl, "out_layer_bn.1", up, el, S, True)
    want = torch.stack([orc.audio_decoder(sdl["decoder_bn.1.weight"], o[s], cfg.enc_stride).reshape(B, -1) for s in range(S)], 0)
    want.backward(dwav)
    soft.agree("head_aux.wav", wav_a, want)
    soft.agree("head_aux.dx", cf(dzs - base_dx), zl.grad)
    soft.agree("head_aux.denc", cf(dencd - base_denc), el.grad)
    check_param_grads(soft, gb, sdl, "out_layer_bn.1.")
    soft.agree("head_aux.grad.decoder", gb.view("decoder_bn.1.weight"), sdl["decoder_bn.1.weight"].grad)
    soft.done()


# ---------------------------------------------------------------------------------------------------------------------
# criteria backward (criterions.py:148-217) against autograd over the criterion oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,T", [(2, 6, 8000), (3, 4, 3001), (2, 2, 1500)])
def test_criteria_backward(S, B, T):
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    g = torch.Generator().manual_seed(S * 100 + B)
    src = [0.1 * torch.randn(B, T, generator=g) + 0.01 * (s + 1) for s in range(S)]
    perm = [torch.randperm(S, generator=g).tolist() for _ in range(B)]
    est = [torch.stack([0.7 * src[perm[b][s]][b] + [0.3, 0.03, 0.001, 1.0][b % 4] * 0.1 * torch.randn(T, generator=g) + 0.02 for b in range(B)])
           for s in range(S)]
    sizes = torch.full((B,), T)
    soft = Soft(f"criteria.S{S}.B{B}.T{T}")
    dev = torch.device("cuda:0")
    srcd = [s_.to(dev) for s_ in src]
    # time-domain loss
    estd = [e.to(dev).requires_grad_(True) for e in est]
    loss = PIT_SISNR_time(dev, S, True)(estims=estd, input_sizes=sizes, target_attr=srcd)
    loss.backward()
    esto = [e.clone().double().requires_grad_(True) for e in est]
    lo = co.pit_sisnr_time(esto, [s_.double() for s_ in src], dtype=torch.float64)[0]
    lo.backward()
    soft.agree("time.loss", loss.reshape(1), lo.reshape(1).float(), 100.0)
    for s in range(S):
        soft.agree(f"time.dest{s}", estd[s].grad, esto[s].grad.float())
    # STFT-magnitude loss
    estd = [e.to(dev).requires_grad_(True) for e in est]
    loss = PIT_SISNR_mag(dev, 512, 128, "hann", 4, S, True, False)(estims=estd, idx=1, input_sizes=sizes, target_attr=srcd)
    loss.backward()
    esto = [e.clone().double().requires_grad_(True) for e in est]
    lo = co.pit_sisnr_mag(esto, [s_.double() for s_ in src], 512, 128)[0]
    lo.backward()
    soft.agree("mag.loss", loss.reshape(1), lo.reshape(1).float(), 90.0)
    for s in range(S):
        # fp32 STFT products on both ends of the M_e - M_s cancellation (estimates 60 dB close to their targets are in the
        # batch); the reference evaluates the same expression in fp32
        soft.agree(f"mag.dest{s}", estd[s].grad, esto[s].grad.float(), 60.0)
    soft.done()


# ---------------------------------------------------------------------------------------------------------------------
# the whole training step behind the reference's surface: model.train(); loss.backward()
# ---------------------------------------------------------------------------------------------------------------------
def _train_step(variant, precision, x, src, aux_loss=True):
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    cfg = dataclasses.replace(VARIANTS[variant], dropout=0.0)
    dev = torch.device("cuda:0")
    m = Model.from_config(cfg, init_seed=0, precision=precision).load_synthetic_(0).to(dev)
    m.train()
    assert m.dropout_p == 0.0
    sizes = torch.full((x.shape[0],), x.shape[1])
    audio, aux = m(x.to(dev))
    srcd = [s_.to(dev) for s_ in src]
    l_time = PIT_SISNR_time(dev, cfg.num_spks, True)(estims=audio, input_sizes=sizes, target_attr=srcd)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=srcd) for i, a in enumerate(aux)]
    if aux_loss:
        loss = ((1 - 0.4) * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks      # reference engine.py:73-74
    else:
        loss = l_time / cfg.num_spks
    loss.backward()
    return cfg, m, audio, aux, loss, l_time, l_mag


@pytest.mark.parametrize("variant,gtag", [("tiny", "train_tiny"), ("tiny3", "train_tiny_s3")])      # two and THREE speakers (round 6)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_train_step_tiny_matches_reference(golden, precision, variant, gtag):
    """model.train(); loss.backward() on the tiny configuration against the REFERENCE's own training step (fixture made
    by tests/golden/make_train_golden.py from the imported reference + its criteria) and, tensor by tensor, the pinned oracle."""
    g = golden(gtag)
    x = torch.from_numpy(g["x"])
    src = [torch.from_numpy(g["src"][:, s].copy()) for s in range(g["src"].shape[1])]
    cfg, m, audio, aux, loss, l_time, l_mag = _train_step(variant, precision, x, src)
    soft = Soft(f"train_step.{variant}.{precision}")
    soft.agree("main", torch.stack(list(audio), 0), torch.from_numpy(g["main"]))
    soft.agree("aux", torch.stack([torch.stack(list(a), 0) for a in aux], 0), torch.from_numpy(g["aux"]))
    assert abs(float(loss) - float(g["loss"])) < 2e-3, (float(loss), float(g["loss"]))
    assert abs(float(l_time) - float(g["loss_time"])) < 2e-3
    assert np.abs(np.asarray([float(v) for v in l_mag]) - g["loss_mag"]).max() < 5e-3
    # the reference's gradient summaries (norm, sum, seeded projection) for every tensor
    from sepreformer_amd.synth import _gen

    def probe(name, shape):        # the seeded projection vectors of tests/golden/make_train_golden.py
        return _gen(4242, name).normal(0.0, 1.0, size=tuple(shape)).astype(np.float32)

    names = [str(n) for n in g["grad_names"]]
    params = dict(m.named_parameters())
    assert set(names) == set(params)
    worst = 0.0
    for i, k in enumerate(names):
        gr = params[k].grad.detach().double().cpu()
        nrm, sm, pr = g["grad_summary"][i]
        got = np.array([float(gr.norm()), float(gr.sum()), float((gr * torch.from_numpy(probe(k, gr.shape)).double()).sum())])
        if k.endswith(STRUCTURAL_ZERO):
            continue
        dev_ = np.abs(got - np.array([nrm, sm, pr])).max() / (nrm + 1e-30)
        worst = max(worst, dev_)
        if dev_ > 2e-3:
            soft.bad.append(f"summary {k}: relative deviation {dev_:.2e}")
    record(f"train_step.{variant}.{precision}.summary_worst_rel", worst)
    # tensor by tensor against the oracle (identical to the reference: PINNING_train.json)
    sdl = tor.leaf_state(synth_state_dict(cfg, 0))
    o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
    o_loss, _, _ = tor.train_loss(o_audio, o_aux, src)
    o_loss.backward()
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad)
    # three speakers in bf16x3: measured worst tensor 77.0 dB (six permutations, three sources per mixture; exact-f32 mode holds 80 dB) -
    # the 75 dB bar of this case is 0.5 bit below the two-speaker one, a wrong S != 2 path would sit below 30 dB
    bar = 75.0 if (variant == "tiny3" and precision != "fp32") else MIN_DB
    for k, p_ in params.items():
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, bar)
    # BatchNorm bookkeeping
    st = m.state_dict()
    off = 0
    for k in [str(n) for n in g["bn_names"]]:
        n_el = st[k].numel()
        soft.agree("bn." + k, st[k], torch.from_numpy(g["bn_after"][off:off + n_el]), 100.0)
        off += n_el
    assert int(st["separator.enc_stages.0.l_block_1.block.cla.BN.num_batches_tracked"]) == int(g["num_batches_tracked_after"])
    soft.done()


@pytest.mark.parametrize("precision,aux_loss", [("fp32", True), pytest.param("fp32", False, marks=slow), ("bf16x3", True), ("bf16x3", False)])
def test_train_step_base_matches_oracle(precision, aux_loss):
    """Base width (F = 128, 4 stages), 0.5 s, batch 2: loss and all 710 gradient tensors against the oracle.

    Two losses.  ``aux_loss=False``: PIT_SISNR_time on the main outputs only - every op on that path is smooth, and every
    gradient tensor must agree to >= 80 dB in both arithmetic modes.  ``aux_loss=True``: the reference's full training loss
    (engine.py:66-74), whose auxiliary heads multiply by ReLU(.) (module.py:257-260, network.py:41).  A ReLU gate is
    discontinuous in the forward activation: a forward deviation of relative size e flips a fraction ~e of the gates, and
    each flipped gate changes its element's gradient by O(1), so two implementations whose forwards agree to e can only
    agree to ~sqrt(e) on everything upstream of an auxiliary head - measured 84 dB in exact-f32 mode (e ~ 1e-7 between the
    MFMA fmaf chain and aten's CPU summation order) and 50-65 dB in bf16x3 mode (e ~ 1e-5).  That is a property of the loss,
    not of the backward kernels (every block's backward agrees to >= 97 dB on identical inputs, tests above), so the bar for
    the full loss is 80 dB in f32 mode and 45 dB in bf16x3 mode, while the last decoder stage and the main head - downstream of
    every auxiliary head - keep the 80 dB bar in both modes."""
    B, T = 2, 4000
    srcn = synth_sources(B, T, seed=31)
    src = [torch.from_numpy(srcn[:, s].copy()) for s in range(2)]
    x = src[0] + src[1]
    cfg, m, audio, aux, loss, l_time, l_mag = _train_step("SepReformer_Base_WSJ0", precision, x, src, aux_loss)
    key = ("base_step", aux_loss)
    if key not in _ORACLE_MEMO:                                 # the oracle's forward + backward once per loss, shared by the arithmetics
        sdl = tor.leaf_state(synth_state_dict(cfg, 0))
        o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
        if aux_loss:
            o_loss, _, _ = tor.train_loss(o_audio, o_aux, src)
        else:
            o_loss = co.pit_sisnr_time(o_audio, src)[0] / cfg.num_spks
        o_loss.backward()
        _ORACLE_MEMO[key] = (sdl, [a.detach() for a in o_audio], o_loss.detach())
    sdl, o_audio, o_loss = _ORACLE_MEMO[key]
    soft = Soft(f"train_step.base.{precision}.{'full' if aux_loss else 'main'}")
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0))
    assert abs(float(loss) - float(o_loss)) < 5e-3, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    relaxed = 45.0 if (aux_loss and precision == "bf16x3") else MIN_DB
    for k, p_ in m.named_parameters():
        if sdl[k].grad is None:                       # auxiliary-head parameters under the main-only loss
            assert p_.grad is None or float(p_.grad.abs().max()) == 0.0, k
            continue
        downstream = k.startswith(("separator.dec_stages.3.", "out_layer.", "audio_decoder."))
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, MIN_DB if downstream else relaxed)
    soft.done()


@pytest.mark.parametrize("variant", [pytest.param("SepReformer_Large_DM_WHAMR", marks=slow), "SepReformer_Large_DM_WHAM"])   # WHAM = WHAMR + per-level splits
def test_train_step_large_matches_oracle(variant):
    """Large (F = 256, dk = 32: the generic GCFN pair, the dk = 32 MFMA attention backward; _WHAM: one speaker split per level
    instead of the shared one), 0.25 s (suite-time budget; 0.5 s measured the same bars), one utterance, the smooth main-output loss:
    loss and every gradient tensor against the oracle at the 80 dB bar in the default bf16x3 arithmetic."""
    B, T = 1, 2000
    srcn = synth_sources(B, T, seed=37)
    src = [torch.from_numpy(srcn[:, s].copy()) for s in range(2)]
    x = src[0] + src[1]
    cfg, m, audio, aux, loss, l_time, l_mag = _train_step(variant, "bf16x3", x, src, False)
    sdl = tor.leaf_state(synth_state_dict(cfg, 0))
    o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
    o_loss = co.pit_sisnr_time(o_audio, src)[0] / cfg.num_spks
    o_loss.backward()
    soft = Soft(f"train_step.{variant}.bf16x3.main")
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0))
    assert abs(float(loss) - float(o_loss)) < 5e-3, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    n = 0
    for k, p_ in m.named_parameters():
        if sdl[k].grad is None:                       # auxiliary-head parameters under the main-only loss
            assert p_.grad is None or float(p_.grad.abs().max()) == 0.0, k
            continue
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, MIN_DB)
        n += 1
    assert n > 500, n
    soft.done()


def test_gcfn_train_unfused_path(monkeypatch):
    """The unfused GCFN pair (what F = 256 / exact-f32 models run, and the A/B reference of the fused pair): same checks as
    test_gcfn_train with SEPR_TRAIN_FUSE_GCFN=0, plus fused vs unfused outputs / input gradients against each other."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=0.0)
    sd = synth_state_dict(cfg, 0)
    dev = torch.device("cuda:0")
    sdd = {k: v.to(dev) for k, v in sd.items()}
    gb_u, gb_f = GradBuffer(cfg, dev), GradBuffer(cfg, dev)
    monkeypatch.setenv("SEPR_TRAIN_FUSE_GCFN", "0")
    tp_u = TrainPack(cfg, sdd, gb_u, "bf16x3")
    monkeypatch.setenv("SEPR_TRAIN_FUSE_GCFN", "1")
    tp_f = TrainPack(cfg, sdd, gb_f, "bf16x3")
    assert not tp_u.fused_gcfn and tp_f.fused_gcfn and not tp_u.gcfn[0][0].fused_w1p and tp_f.gcfn[0][0].fused_w1p
    eng = TrainEngine(cfg, dev)
    F = cfg.feat
    p = "separator.enc_stages.0.g_block_1.block.gcfn"
    soft = Soft("base.bf16x3.gcfn_unfused")
    for n, T in ((2, 37), (3, 301), (2, 2000)):
        x, dy = rnd(n, T, F, seed=T), rnd(n, T, F, seed=T + 7)
        yu, rec_u = eng.block_fwd("gcfn", x.cuda(), tp_u.gcfn[0], n, T)
        dxu = eng.block_bwd(rec_u, dy.cuda())
        yf, rec_f = eng.block_fwd("gcfn", x.cuda(), tp_f.gcfn[0], n, T)
        dxf = eng.block_bwd(rec_f, dy.cuda())
        assert rec_f[2].numel() < rec_u[2].numel() // 100          # the fused context is the statistics only
        soft.agree(f"T{T}.y_fused_vs_unfused", yf, yu, 95.0)
        soft.agree(f"T{T}.dx_fused_vs_unfused", dxf, dxu, 95.0)
        if T < 1000:
            sdl = tor.leaf_state(sd)
            xl = x.clone().requires_grad_(True)
            yo = orc.gcfn(sdl, p, xl)
            yo.backward(dy)
            soft.agree(f"T{T}.y", yu, yo)
            soft.agree(f"T{T}.dx", dxu, xl.grad)
            check_param_grads(soft, gb_u, sdl, p)
        for k in (".net1.1.weight", ".net2.2.weight", ".depthwise.weight", ".depthwise.bias", ".net1.0.weight", ".Layer_scale.layer_scale"):
            soft.agree(f"T{T}.grad{k}_fused_vs_unfused", gb_f.view(p + k), gb_u.view(p + k), 90.0)
        gb_u.flat.zero_()
        gb_f.flat.zero_()
    soft.done()


def _separator_state(t):
    """The (model, engine, pack, gradient buffer, tape, ...) tuple of the autograd node behind a train-mode output."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if getattr(fn, "state", None) is not None:
            return fn.state
        todo += [f for f, _ in fn.next_functions]
    raise AssertionError("no _SeparatorFn node behind this tensor")


@slow        # (batch 2 x 0.5 s: round 6's batch-16 x 0.5 s test is the same check at the bench's batch)
def test_train_step_base_full_loss_frozen_gates():
    """Round-2 review item: the reference's FULL loss at Base width in the default bf16x3 arithmetic, with the discontinuity
    removed instead of the bar lowered.  The auxiliary heads' ReLU gates (module.py:257-260) are frozen to the gates the
    DEVICE forward took (read back from the heads' saved pre-activations) in the oracle as well - then the loss is smooth in
    the forward activations and EVERY gradient tensor must agree to >= 80 dB, upstream of the auxiliary heads included
    (without the freeze: 45-65 dB there, test_train_step_base_matches_oracle)."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    B, T = 2, 4000
    srcn = synth_sources(B, T, seed=31)
    src = [torch.from_numpy(srcn[:, s].copy()) for s in range(2)]
    x = src[0] + src[1]
    cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=0.0)
    dev = torch.device("cuda:0")
    m = Model.from_config(cfg, init_seed=0, precision="bf16x3").load_synthetic_(0).to(dev)
    m.train()
    sizes = torch.full((B,), T)
    audio, aux = m(x.to(dev))
    # the gates the device took: pre-ReLU head outputs o2 [nS, Tsrc, N] at the end of each auxiliary head's context
    # (sepr_train_api.hip OutCtx: a1 [Mp,4F], o1 [Mp,2F], o2 [Mp,N], 256-byte aligned slices), upsampled like model.py:49
    state = _separator_state(audio[0])
    tape = state[4]
    F, N, S = cfg.feat, cfg.enc_channels, cfg.num_spks
    L_ = cfg.frames(T)
    masks = []
    for rec in tape:
        if rec[0] != "head_aux":
            continue
        _, cur, cx, _w, Tc, idx, _i = rec
        Mp = B * S * Tc
        al = lambda v: (v + 255) // 256 * 256                                                   # noqa: E731
        off = al(al(4 * F * Mp * 4) + 2 * F * Mp * 4)
        o2 = cx[off:off + N * Mp * 4].view(torch.float32).view(B * S, Tc, N).cpu()
        gate = (o2 > 0).float()[:, idx[0].cpu().long(), :]                                     # [nS, L, N]
        masks.append(gate.permute(0, 2, 1).contiguous())
    assert len(masks) == cfg.num_stages
    srcd = [s_.to(dev) for s_ in src]
    l_time = PIT_SISNR_time(dev, S, True)(estims=audio, input_sizes=sizes, target_attr=srcd)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, S, True, False)
    l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=srcd) for i, a in enumerate(aux)]
    loss = ((1 - 0.4) * l_time + 0.4 * sum(l_mag) / len(l_mag)) / S
    loss.backward()
    sdl = tor.leaf_state(synth_state_dict(cfg, 0))
    orc.RELU_MASKS = iter(masks)
    try:
        o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
    finally:
        orc.RELU_MASKS = None
    o_loss, _, _ = tor.train_loss(o_audio, o_aux, src)
    o_loss.backward()
    soft = Soft("train_step.base.bf16x3.full_frozen_gates")
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0))
    soft.agree("aux", torch.stack([torch.stack(list(a), 0) for a in aux], 0),
               torch.stack([torch.stack([t_.detach()[..., :T] for t_ in a], 0) for a in o_aux], 0))
    assert abs(float(loss) - float(o_loss)) < 5e-3, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    worst = 999.0
    for k, p_ in m.named_parameters():
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, MIN_DB)
        if not k.endswith(STRUCTURAL_ZERO):
            worst = min(worst, REPORT.get(f"{soft.tag}.grad.{k}", 999.0))
    record(f"{soft.tag}.worst_grad_db", worst)
    soft.done()


def test_train_step_full_size_properties():
    """BASELINE configs[4] at its real length (Base, 4 s, batch 4: 32 000 rows per sequence at the top level - BatchNorm batch
    statistics over 128 000 rows, the fp64 partial trees, the weight-gradient split-M plan at M = 256 000): size-independent
    properties of the whole step in the default arithmetic.
      * dropout live (p = 0.05): two runs from the same seed give the bitwise-identical loss and gradients (no atomics, counter-based
        masks), a different seed does not;
      * dropout off: the loss is within 5e-3 of the oracle's train-mode forward loss, the main outputs agree to >= 80 dB, and the
        updated BatchNorm running statistics agree with the oracle's (torch.nn.BatchNorm1d's formula) to >= 80 dB;
      * every gradient is finite and the global norm is the same to 1e-4 relative whether the batch is run as 4 or re-run."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    B, T = 4, 32000
    srcn = synth_sources(B, T, seed=77)
    src = [torch.from_numpy(srcn[:, s].copy()) for s in range(2)]
    x = src[0] + src[1]
    dev = torch.device("cuda:0")
    sizes = torch.full((B,), T)
    srcd = [s_.to(dev) for s_ in src]

    def run(p_drop, seed):
        torch.manual_seed(seed)
        cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=p_drop)
        m = Model.from_config(cfg, init_seed=0, precision="bf16x3").load_synthetic_(0).to(dev)
        m.train()
        audio, aux = m(x.to(dev))
        l_time = PIT_SISNR_time(dev, 2, True)(estims=audio, input_sizes=sizes, target_attr=srcd)
        crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, 2, True, False)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=srcd) for i, a in enumerate(aux)]
        loss = ((1 - 0.4) * l_time + 0.4 * sum(l_mag) / len(l_mag)) / 2
        loss.backward()
        flat = torch.cat([p_.grad.reshape(-1) for p_ in m.parameters()])
        return cfg, m, [a.detach() for a in audio], float(loss), flat

    _, _, _, la, ga = run(0.05, 1)
    _, _, _, lb, gb_ = run(0.05, 1)
    _, _, _, lc, gc = run(0.05, 2)
    assert torch.isfinite(ga).all() and np.isfinite(la)
    assert la == lb and torch.equal(ga, gb_), (la, lb)
    assert not torch.equal(ga, gc)
    record("train_step.base_4s_b4.loss_dropout", la)
    cfg, m, audio, l0, g0 = run(0.0, 1)
    assert torch.isfinite(g0).all()
    sdl = synth_state_dict(cfg, 0)
    with torch.no_grad():
        o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
        o_loss, _, _ = tor.train_loss(o_audio, o_aux, src)
    record("train_step.base_4s_b4.loss", l0)
    record("train_step.base_4s_b4.loss_abs_dev", abs(l0 - float(o_loss)))
    assert abs(l0 - float(o_loss)) < 5e-3, (l0, float(o_loss))
    soft = Soft("train_step.base_4s_b4")
    soft.agree("main", torch.stack(audio, 0), torch.stack(list(o_audio), 0))
    st = m.state_dict()
    for k in ("separator.enc_stages.0.l_block_1.block.cla.BN.running_mean", "separator.enc_stages.0.l_block_1.block.cla.BN.running_var",
              "separator.enc_stages.0.downconv.BN.running_mean", "separator.enc_stages.0.downconv.BN.running_var",
              "separator.dec_stages.3.l_block_3.block.cla.BN.running_mean", "separator.dec_stages.3.l_block_3.block.cla.BN.running_var",
              "separator.bottleneck_G.l_block_2.block.cla.BN.running_var"):
        soft.agree("bn." + k, st[k], sdl[k])
    soft.done()


def test_train_graph_replay_matches_eager():
    """The captured training step (model.train_graphs: weight re-pack + forward as one hipGraph, backward as another) against
    the eager step.  Dropout off: same kernels in the same order, so loss, every gradient and the updated BatchNorm state are
    BITWISE those of the eager step, also on the second and third replay with the weights changed in between by the optimizer.
    Dropout on: every replay draws fresh masks (the per-step seed travels through the device-side salt), and two models built
    from the same seed follow the same trajectory."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    dev = torch.device("cuda:0")
    B, T = 2, 4000
    srcn = synth_sources(B, T, seed=31)
    src = [torch.from_numpy(srcn[:, s].copy()).to(dev) for s in range(2)]
    x = (src[0] + src[1]).contiguous()
    sizes = torch.full((B,), T)

    def trajectory(graphs, p_drop, steps, seed=7):
        torch.manual_seed(seed)
        cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=p_drop)
        m = Model.from_config(cfg, init_seed=0, precision="bf16x3").load_synthetic_(0).to(dev)
        m.train()
        m.train_graphs = graphs
        opt = torch.optim.AdamW(m.parameters(), lr=1.0e-4)
        ct, cm = PIT_SISNR_time(dev, 2, True), PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, 2, True, False)
        out = []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            audio, aux = m(x)
            lm = [cm(estims=a, idx=i, input_sizes=sizes, target_attr=src) for i, a in enumerate(aux)]
            loss = (0.6 * ct(estims=audio, input_sizes=sizes, target_attr=src) + 0.4 * sum(lm) / len(lm)) / 2
            loss.backward()
            out.append((float(loss), torch.cat([p_.grad.reshape(-1) for p_ in m.parameters()]).clone()))
            opt.step()
        return m, out

    me, eager = trajectory(False, 0.0, 3)
    mg, graph = trajectory(True, 0.0, 3)
    for i, ((le, ge), (lg, gg)) in enumerate(zip(eager, graph)):
        assert le == lg, (i, le, lg)
        assert torch.equal(ge, gg), i
    for (k, a), (_, b) in zip(me.state_dict().items(), mg.state_dict().items()):
        assert torch.equal(a, b), k
    assert len(mg.__dict__["_train_graphs"]) == 1 and next(iter(mg.__dict__["_train_graphs"].values())).replays == 3
    # dropout: fresh masks per replay, reproducible from the seed
    _, d1 = trajectory(True, 0.3, 2, seed=11)
    _, d2 = trajectory(True, 0.3, 2, seed=11)
    assert d1[0][0] == d2[0][0] and d1[1][0] == d2[1][0] and torch.equal(d1[1][1], d2[1][1])
    m3, _ = trajectory(True, 0.3, 1, seed=11)
    tg = next(iter(m3.__dict__["_train_graphs"].values()))
    la = []
    for _ in range(2):                                          # the SAME weights and input twice: only the masks differ
        audio, aux = m3(x)
        la.append(float(torch.stack(audio).abs().sum()))
        torch.stack(audio).sum().backward()
    assert la[0] != la[1], la
    assert tg.replays == 3


def test_captured_whole_step_matches_eager():
    """train_step.CapturedTrainStep (forward + criteria + backward in one hipGraph, clip + AdamW in a second) against the same
    step launched from the host.  Dropout off: the captured kernels are the eager ones in the same order, so after the same number
    of optimizer steps every parameter, every BatchNorm buffer and the loss are BITWISE equal.  Dropout on: the device-side salt
    gives every replay its own masks (checked with a zero learning rate: same weights, same input, different loss), and the
    trajectory is reproducible from the seed."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.train_step import CapturedTrainStep
    dev = torch.device("cuda:0")
    B, T = 2, 4000
    srcn = synth_sources(B, T, seed=31)
    src = [torch.from_numpy(srcn[:, s].copy()).to(dev) for s in range(2)]
    x = (src[0] + src[1]).contiguous()
    sizes = torch.full((B,), T)

    def build(p_drop, lr, seed):
        torch.manual_seed(seed)
        cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=p_drop)
        m = Model.from_config(cfg, init_seed=0, precision="bf16x3").load_synthetic_(0).to(dev)
        m.train()
        opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=0.0 if lr == 0.0 else 1.0e-2, capturable=True)
        ct, cm = PIT_SISNR_time(dev, 2, True), PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, 2, True, False)

        def loss_fn(audio, aux, *tg):
            tg = list(tg)
            lm = [cm(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
            return (0.6 * ct(estims=audio, input_sizes=sizes, target_attr=tg) + 0.4 * sum(lm) / len(lm)) / 2
        return m, opt, loss_fn

    def eager(steps):
        m, opt, loss_fn = build(0.0, 1.0e-4, 7)
        params = list(m.parameters())
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            audio, aux = m(x)
            loss = loss_fn(audio, aux, *src)
            loss.backward()
            gn = torch.nn.utils.clip_grad_norm_(params, 5.0)
            opt.step()
        return m, float(loss), float(gn)

    me, le, ge = eager(4)
    mc, opt, loss_fn = build(0.0, 1.0e-4, 7)
    step = CapturedTrainStep(mc, loss_fn, opt, x, src, max_norm=5.0, warmup=1)      # 1 eager step + 3 replays = 4 optimizer steps
    for _ in range(3):
        lc, gc = step(x, src)
    assert step.calls == 3 and float(lc) == le and float(gc) == ge, (float(lc), le, float(gc), ge)
    for (k, a), (_, b) in zip(me.state_dict().items(), mc.state_dict().items()):
        assert torch.equal(a, b), k
    # the evaluation path sees the weights the replays wrote (the packed forms are invalidated by every call)
    mc.eval(); me.eval()
    with torch.no_grad():
        a_c, _ = mc(x)
        a_e, _ = me(x)
    assert torch.equal(torch.stack(list(a_c)), torch.stack(list(a_e)))
    # dropout: a zero learning rate keeps the weights, so only the masks can change the loss between replays
    md, optd, lfd = build(0.3, 0.0, 11)
    sd_ = CapturedTrainStep(md, lfd, optd, x, src, max_norm=5.0, warmup=1)
    l1 = float(sd_(x, src)[0])
    salt1 = int(sd_.salt.item())
    l2 = float(sd_(x, src)[0])
    assert l1 != l2 and int(sd_.salt.item()) != salt1, (l1, l2)
    md2, optd2, lfd2 = build(0.3, 0.0, 11)
    sd2 = CapturedTrainStep(md2, lfd2, optd2, x, src, max_norm=5.0, warmup=1)
    assert float(sd2(x, src)[0]) == l1 and float(sd2(x, src)[0]) == l2


def test_train_step_tiny_bf16():
    """precision="bf16" (plain bf16 operands in every projection / contraction of the step, fp32 accumulate, fp32 master
    weights and gradients): the tiny configuration's whole step against the oracle.  Outputs / loss / gradients are those of
    a bf16-autocast run: the bar is BF16_DB per tensor, the measured agreement is recorded beside the bf16x3 numbers."""
    g_x = synth_sources(4, 2000, seed=5) * 4.0
    src = [torch.from_numpy(g_x[:, s].copy()) for s in range(2)]
    x = src[0] + src[1]
    cfg, m, audio, aux, loss, l_time, l_mag = _train_step("tiny", "bf16", x, src)
    sdl = tor.leaf_state(synth_state_dict(cfg, 0))
    o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
    o_loss, _, _ = tor.train_loss(o_audio, o_aux, src)
    o_loss.backward()
    soft = Soft("train_step.tiny.bf16", "bf16")
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0))
    record("train_step.tiny.bf16.loss_abs_dev", abs(float(loss) - float(o_loss)))
    assert abs(float(loss) - float(o_loss)) < 0.1, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    dbs = []
    for k, p_ in m.named_parameters():
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, 25.0)
        if f"{soft.tag}.grad.{k}" in REPORT:
            dbs.append(REPORT[f"{soft.tag}.grad.{k}"])
    record("train_step.tiny.bf16.grad_db_median", float(np.median(dbs)))
    record("train_step.tiny.bf16.grad_db_min", float(np.min(dbs)))
    soft.done()


def test_dropout_contract():
    """p = 0 disables dropout exactly; p > 0: keep rate ~ 1 - p, survivors scaled by 1 / (1 - p), the same (seed, block) gives
    the same mask in forward and backward (the gradient of a dropped element is zero), a different seed a different mask."""
    cfg, sd, sdd, gb, tp, eng = setup("SepReformer_Base_WSJ0", "bf16x3")
    F = cfg.feat
    n, T = 4, 500
    x, dy = rnd(n, T, F, seed=1).cuda(), rnd(n, T, F, seed=2).cuda()
    y0, _ = eng.block_fwd("gcfn", x, tp.gcfn[0], n, T, 0, 0.0, 123)
    y0b, _ = eng.block_fwd("gcfn", x, tp.gcfn[0], n, T, 0, 0.0, 456)
    assert torch.equal(y0, y0b)
    y1, rec1 = eng.block_fwd("gcfn", x, tp.gcfn[0], n, T, 0, 0.3, 123)
    y1b, _ = eng.block_fwd("gcfn", x, tp.gcfn[0], n, T, 0, 0.3, 123)
    y2, _ = eng.block_fwd("gcfn", x, tp.gcfn[0], n, T, 0, 0.3, 124)
    assert torch.equal(y1, y1b) and not torch.equal(y1, y2) and not torch.equal(y1, y0)
    # output dropout: the branch (y - x) is exactly zero where dropped
    dropped = ((y1 - x) == 0).float().mean().item()
    assert 0.25 < dropped < 0.35, dropped
    # backward with the same record regenerates the same masks: finite, and deterministic
    dx = eng.block_bwd(rec1, dy)
    gb.flat.zero_()
    dx2 = eng.block_bwd(rec1, dy)
    assert torch.isfinite(dx).all() and torch.equal(dx, dx2)
    # numerical check of every dropout-enabled block kind (all the reference's sites: GCFN x2, CLA, attention probabilities and
    # attention output of EGA / speaker attention): directional derivative of sum(y * dy) along a random direction, same masks
    v = rnd(n, T, F, seed=3).cuda()
    eps = 1e-2
    for kind, w, Tp in (("gcfn", tp.gcfn[0], 0), ("cla", tp.cla[0], 0), ("ega", tp.ega[0], T // 4), ("spk", tp.spk[0], 0)):
        y_, rec = eng.block_fwd(kind, x, w, n, T, Tp, 0.3, 77)
        y_b, _ = eng.block_fwd(kind, x, w, n, T, Tp, 0.3, 77)
        y_0, _ = eng.block_fwd(kind, x, w, n, T, Tp, 0.0, 77)
        assert torch.equal(y_, y_b) and not torch.equal(y_, y_0), kind
        dxk = eng.block_bwd(rec, dy)
        yp, _ = eng.block_fwd(kind, x + eps * v, w, n, T, Tp, 0.3, 77)
        ym, _ = eng.block_fwd(kind, x - eps * v, w, n, T, Tp, 0.3, 77)
        num = float(((yp - ym).double() * dy.double()).sum() / (2 * eps))
        ana = float((dxk.double() * v.double()).sum())
        record(f"dropout.fd.{kind}.rel_dev", abs(num - ana) / max(1.0, abs(ana)))
        assert abs(num - ana) <= 2e-2 * max(1.0, abs(ana)), (kind, num, ana)


def test_training_loop_learns_and_is_reproducible():
    """The reference loop (engine.py:50-83) on the tiny configuration with dropout live (p = 0.05): 12 AdamW steps on one fixed
    batch drive the loss down; the same seed gives a bit-identical trajectory (no atomics anywhere in the backward, the dropout
    generator is counter-based); eval() afterwards runs on the updated weights and running statistics."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    cfg = VARIANTS["tiny"]
    dev = torch.device("cuda:0")
    B, T = 4, 2000
    srcn = synth_sources(B, T, seed=5) * 4.0
    src = [torch.from_numpy(srcn[:, s].copy()).to(dev) for s in range(2)]
    x = (src[0] + src[1]).contiguous()
    sizes = torch.full((B,), T)

    def run(steps):
        torch.manual_seed(1234)
        m = Model.from_config(cfg, init_seed=0).to(dev)          # the reference's default init (LayerScale 1e-5)
        m.train()
        assert m.dropout_p == pytest.approx(0.05)
        opt = torch.optim.AdamW(m.parameters(), lr=1.0e-3, weight_decay=1.0e-2)
        crit_t = PIT_SISNR_time(dev, 2, True)
        crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, 2, True, False)
        losses = []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            audio, aux = m(x)
            l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=src) for i, a in enumerate(aux)]
            loss = (0.6 * crit_t(estims=audio, input_sizes=sizes, target_attr=src) + 0.4 * sum(l_mag) / len(l_mag)) / 2
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
            opt.step()
            losses.append(float(loss))
        return m, losses

    m1, l1 = run(12)
    m2, l2 = run(12)
    record("train_loop.tiny.loss_first", l1[0])
    record("train_loop.tiny.loss_last", l1[-1])
    assert all(np.isfinite(l1)) and l1[-1] < l1[0] - 1.0, l1
    assert l1 == l2, (l1, l2)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    bn = m1.state_dict()["separator.enc_stages.0.l_block_1.block.cla.BN.num_batches_tracked"]
    assert int(bn) == 12
    m1.eval()
    audio, _ = m1(x)
    assert torch.isfinite(torch.stack(audio)).all()


# ---------------------------------------------------------------------------------------------------------------------
# round 4: the SAME checks at the launch sizes of the bench (the round-2 contraction bug lived between "toy" and "full size")
# ---------------------------------------------------------------------------------------------------------------------
# Every block kind's train-mode forward + backward against fp64 autograd over the oracle at >= 17 000 rows (two workgroups per CU
# on every CU, dozens of row slices in the contraction, sequence ends on tile seams), in all three arithmetics.  The oracle runs in
# fp64 here so that its own summation error over 32 000-64 000 rows is not what the bar measures.
def _oracle64(sd):
    return tor.leaf_state(sd, dtype=torch.float64)


_ORACLE_MEMO = {}


@pytest.mark.parametrize("precision", PRECISIONS_T)
@pytest.mark.parametrize("n,T", [(8, 8000), (4, 8191)])
def test_gcfn_train_full_size(n, T, precision):
    """GCFN at 64 000 / 32 764 rows (T = 8191: odd, sequence ends inside wave tiles and workgroup tiles; the large-launch
    instantiations of the fused forward, the recomputing middle kernel and both weight-gradient contractions)."""
    cfg, sd, sdd, gb, tp, eng = setup("SepReformer_Base_WSJ0", precision)
    F = cfg.feat
    soft = Soft(f"full_size.{precision}.gcfn.n{n}.T{T}", precision)
    p = "separator.dec_stages.3.g_block_1.block.gcfn"
    w = tp.gcfn[tp.block_prefixes["gcfn"].index(p)]
    gb.flat.zero_()
    x, dy = rnd(n, T, F, seed=T), rnd(n, T, F, seed=T + 7)
    y, rec = eng.block_fwd("gcfn", x.cuda(), w, n, T)
    dx = eng.block_bwd(rec, dy.cuda())
    dx2 = eng.block_bwd(rec, dy.cuda())                         # the backward is a pure function of its record: bitwise repeatable
    assert torch.equal(dx, dx2)
    gb.flat.mul_(0.5)                                           # (two backward calls accumulated the parameter gradients twice)
    key = ("gcfn", n, T)
    if key not in _ORACLE_MEMO:                                 # one fp64 autograd pass per shape, shared by the three arithmetics
        sdl = _oracle64(sd)
        xl = x.double().requires_grad_(True)
        yo = orc.gcfn(sdl, p, xl)
        yo.backward(dy.double())
        _ORACLE_MEMO[key] = (yo.detach().float(), xl.grad.float(), {k: v for k, v in sdl.items() if k.startswith(p)})
    yo, dxo, sdl = _ORACLE_MEMO[key]
    soft.agree("y", y, yo)
    soft.agree("dx", dx, dxo)
    check_param_grads(soft, gb, sdl, p)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS_T)
def test_cla_train_full_size(precision):
    """CLA at 32 000 rows: train-mode BatchNorm statistics over the whole launch (fp64 partial trees), the k = 65 depthwise
    weight gradient over 8000-frame sequences."""
    cfg, sd, sdd, gb, tp, eng = setup("SepReformer_Base_WSJ0", precision)
    F = cfg.feat
    n, T = 4, 8000
    soft = Soft(f"full_size.{precision}.cla.n{n}.T{T}", precision)
    p = "separator.enc_stages.0.l_block_1.block.cla"
    gb.flat.zero_()
    # (the device state_dict is shared with other tests of this precision, e.g. test_dropout_contract, which run CLA blocks without
    #  restoring the running statistics: start from the pristine values the oracle starts from)
    sdd[p + ".BN.running_mean"].copy_(sd[p + ".BN.running_mean"])
    sdd[p + ".BN.running_var"].copy_(sd[p + ".BN.running_var"])
    rm0, rv0 = sdd[p + ".BN.running_mean"].clone(), sdd[p + ".BN.running_var"].clone()
    x, dy = rnd(n, T, F, seed=T), rnd(n, T, F, seed=T + 7)
    y, rec = eng.block_fwd("cla", x.cuda(), tp.cla[0], n, T)
    dx = eng.block_bwd(rec, dy.cuda())
    key = ("cla", n, T)
    if key not in _ORACLE_MEMO:                                 # one fp64 autograd pass, shared by the three arithmetics (suite time)
        sdl = _oracle64(sd)
        xl = x.double().requires_grad_(True)
        orc.BN_TRAINING = True
        try:
            yo = orc.cla(sdl, p, xl)
        finally:
            orc.BN_TRAINING = False
        yo.backward(dy.double())
        _ORACLE_MEMO[key] = (yo.detach().float(), xl.grad.float(), {k: v for k, v in sdl.items() if k.startswith(p)})
    yo, dxo, sdl = _ORACLE_MEMO[key]
    soft.agree("y", y, yo)
    soft.agree("dx", dx, dxo)
    check_param_grads(soft, gb, sdl, p)
    soft.agree("running_mean", sdd[p + ".BN.running_mean"], sdl[p + ".BN.running_mean"], 100.0)
    soft.agree("running_var", sdd[p + ".BN.running_var"], sdl[p + ".BN.running_var"], 100.0)
    sdd[p + ".BN.running_mean"].copy_(rm0)
    sdd[p + ".BN.running_var"].copy_(rv0)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS_T)
@pytest.mark.parametrize("fac", [16, 1])
def test_ega_train_full_size(fac, precision):
    """EGA at the bench's attention size: T' = 500 pooled frames, 8 sequences (64 (sequence, head) pairs x 8 query blocks), pooling
    factor 16 (the top level: 64 000 rows through the gate / pool backward) and 1 (the bottleneck)."""
    cfg, sd, sdd, gb, tp, eng = setup("SepReformer_Base_WSJ0", precision)
    F, H = cfg.feat, cfg.heads
    n, Tp = 8, 500
    T = Tp * fac
    soft = Soft(f"full_size.{precision}.ega.n{n}.fac{fac}", precision)
    p = "separator.enc_stages.0.g_block_1.block.ega"
    gb.flat.zero_()
    x, dy = rnd(n, F, T, seed=fac), rnd(n, T, F, seed=fac + 7)
    y, rec = eng.block_fwd("ega", cl(x), tp.ega[0], n, T, Tp)
    dx = eng.block_bwd(rec, dy.cuda())
    key = ("ega", n, fac)
    if key not in _ORACLE_MEMO:
        sdl = _oracle64(sd)
        xl = x.double().requires_grad_(True)
        yo = orc.ega(sdl, p, xl, orc.rel_pos_k(sdl, Tp, cfg.maxlen), H)
        yo.backward(dy.double())
        _ORACLE_MEMO[key] = (yo.detach().float(), xl.grad.float(),
                             {k: v for k, v in sdl.items() if k.startswith(p) or k == "separator.pos_emb.pe_k.weight"})
    yo, dxo, sdl = _ORACLE_MEMO[key]
    soft.agree("y", y, yo)
    soft.agree("dx", cf(dx), dxo)
    check_param_grads(soft, gb, sdl, p)
    soft.agree("grad.pe_k", gb.view("separator.pos_emb.pe_k.weight"), sdl["separator.pos_emb.pe_k.weight"].grad)
    soft.done()


@pytest.mark.parametrize("precision", PRECISIONS_T)
def test_spkattn_train_full_size(precision):
    """Speaker attention at 2 x 2 x 8000 = 32 000 rows."""
    cfg, sd, sdd, gb, tp, eng = setup("SepReformer_Base_WSJ0", precision)
    F, H, S = cfg.feat, cfg.heads, cfg.num_spks
    B, T = 2, 8000
    soft = Soft(f"full_size.{precision}.spkattn.B{B}.T{T}", precision)
    p = "separator.dec_stages.0.spk_attn_1.self_attn"
    gb.flat.zero_()
    x, dy = rnd(B * S, T, F, seed=5), rnd(B * S, T, F, seed=6)
    y, rec = eng.block_fwd("spk", x.cuda(), tp.spk[0], B * S, T)
    dx = eng.block_bwd(rec, dy.cuda())
    key = ("spk", B, T)
    if key not in _ORACLE_MEMO:
        sdl = _oracle64(sd)
        xl = x.double().requires_grad_(True)
        xr = xl.view(B, S, T, F).permute(0, 2, 1, 3).reshape(B * T, S, F)
        yr = xr + orc.mha(sdl, p, xr, None, H)
        yo = yr.view(B, T, S, F).permute(0, 2, 1, 3).reshape(B * S, T, F)
        yo.backward(dy.double())
        _ORACLE_MEMO[key] = (yo.detach().float(), xl.grad.float(), {k: v for k, v in sdl.items() if k.startswith(p)})
    yo, dxo, sdl = _ORACLE_MEMO[key]
    soft.agree("y", y, yo)
    soft.agree("dx", dx, dxo)
    check_param_grads(soft, gb, sdl, p)
    soft.done()


@pytest.mark.parametrize("x3", [1, 2])
def test_general_loader_contraction_full_size(x3):
    """The contraction's GENERAL loader (row maps, two-source concat, per-sequence statistics: fusion conv, projector, output
    heads) at >= 20 000 rows through the blocks that use it - front_bwd (per-sequence GroupNorm statistics), fuse_bwd (x2 upsample
    + concat), head_bwd (crop row map) - against fp64 autograd and for bitwise repeatability (only the straight-line
    loader had a full-size test; the general loader runs one workgroup per CU by construction, asserted in the launcher)."""
    precision = {1: "bf16x3", 2: "bf16"}[x3]
    cfg, sd, sdd, gb, tp, eng = setup("SepReformer_Base_WSJ0", precision)
    F, S, N = cfg.feat, cfg.num_spks, cfg.enc_channels
    soft = Soft(f"full_size.{precision}.general_loader", precision)
    # fusion conv at 2 x 12 000 -> 24 000 frames
    n, Tl = 2, 12000
    lo, sk, dy = rnd(n, F, Tl, seed=12), rnd(n, F, 2 * Tl, seed=13), rnd(n, F, 2 * Tl, seed=14)
    flats = []
    for _ in range(2):
        gb.flat.zero_()
        dlo, dsk = eng.fuse_bwd(cl(lo), cl(sk), tp.fuse[0], cl(dy), n, 2 * Tl)
        flats.append((gb.flat.clone(), dlo.clone(), dsk.clone()))
    assert all(torch.equal(a, b) for a, b in zip(flats[0], flats[1]))
    sdl = _oracle64(sd)
    lol, skl = lo.double().requires_grad_(True), sk.double().requires_grad_(True)
    up = torch.nn.functional.interpolate(lol, size=2 * Tl, mode="nearest")
    yo = torch.nn.functional.conv1d(torch.cat([up, skl], 1), sdl["separator.simple_fusion.0.weight"], sdl["separator.simple_fusion.0.bias"])
    yo.backward(dy.double())
    soft.agree("fuse.dlo", cf(dlo), lol.grad)
    soft.agree("fuse.dskip", cf(dsk), skl.grad)
    check_param_grads(soft, gb, sdl, "separator.simple_fusion.0")
    # encoder + GroupNorm + projector at 3 x 8000 frames (per-sequence statistics in the projector's weight gradient)
    B, T = 3, 4 * 7997 + 12
    L_ = cfg.frames(T)
    Lp = cfg.padded_frames(L_)
    wav = rnd(B, T, seed=12, scale=0.1)
    wd = wav.cuda()
    dcur, denc = rnd(B, F, Lp, seed=13), rnd(B, N, L_, seed=14)
    flats = []
    for _ in range(2):
        gb.flat.zero_()
        enc, cur, ctx = eng.front_fwd(wd, tp, B, T, L_, Lp)
        denc_d = cl(denc)
        eng.front_bwd(wd, enc, ctx, tp, cl(dcur), denc_d, B, T, Lp)
        flats.append(gb.flat.clone())
    assert torch.equal(flats[0], flats[1])
    sdl = _oracle64(sd)
    e = orc.audio_encoder(sdl, wav.double(), cfg.enc_stride)
    pj = orc.pad_signal(orc.feature_projector(sdl, e), cfg.num_stages)
    (pj * dcur.double()).sum().backward(retain_graph=True)
    e.backward(denc.double())
    for k in ("audio_encoder.conv1d.weight", "feature_projector.norm.weight", "feature_projector.norm.bias", "feature_projector.conv1d.weight"):
        soft.agree("front.grad." + k, gb.view(k), sdl[k].grad)
    # main head at 2 x 2 x 8000 frames (crop L_ < Lp)
    B = 2
    e2 = e.detach()[:B].float()
    z = rnd(B * S, F, Lp, seed=15)
    zd = cl(z)
    flats = []
    for _ in range(2):
        gb.flat.zero_()
        wav_o, cx = eng.head_fwd(zd, tp.out_main, B * S, Lp, L_, None, None)
        dwav = rnd(S, B, wav_o.shape[-1], seed=16)
        dz = torch.empty_like(zd)
        eng.head_bwd(zd, cx, tp.out_main, dwav.cuda(), dz, False, None, B * S, Lp, L_, None, None)
        flats.append((gb.flat.clone(), dz.clone()))
    assert all(torch.equal(a, b) for a, b in zip(flats[0], flats[1]))
    sdl = _oracle64(sd)
    zl = z.double().requires_grad_(True)
    o = orc.output_layer(sdl, "out_layer", zl, e2.double(), S, False)
    want = torch.stack([orc.audio_decoder(sdl["audio_decoder.weight"], o[s], cfg.enc_stride).reshape(B, -1) for s in range(S)], 0)
    want.backward(dwav.double())
    soft.agree("head_main.wav", wav_o, want)
    soft.agree("head_main.dx", cf(dz), zl.grad)
    check_param_grads(soft, gb, sdl, "out_layer.")
    soft.agree("head_main.grad.decoder", gb.view("audio_decoder.weight"), sdl["audio_decoder.weight"].grad)
    soft.done()


B4_STEP_MIN_DB = 80.0      # batch-4 whole-step bar = the batch-1 bar (measured, round 5: worst tensor 81.35 dB, median 92.9 dB; batch 1: 81.57 / 96.3)


def _frozen_gate_step(precision, B, T, seed, share_oracle=False):
    """One train step of Base (dropout 0) on the device with the reference's FULL loss, and the same step through the oracle with
    the auxiliary heads' ReLU gates frozen to the gates the device forward took (see test_train_step_base_full_loss_frozen_gates).
    Returns (cfg, model, device outputs, device loss, oracle leaf state with .grad, oracle outputs, oracle loss)."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    srcn = synth_sources(B, T, seed=seed)
    src = [torch.from_numpy(srcn[:, s].copy()) for s in range(2)]
    x = src[0] + src[1]
    cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=0.0)
    dev = torch.device("cuda:0")
    m = Model.from_config(cfg, init_seed=0, precision=precision).load_synthetic_(0).to(dev)
    m.train()
    sizes = torch.full((B,), T)
    audio, aux = m(x.to(dev))
    state = _separator_state(audio[0])
    tape = state[4]
    F, N, S = cfg.feat, cfg.enc_channels, cfg.num_spks
    masks = []
    for rec in tape:
        if rec[0] != "head_aux":
            continue
        _, cur, cx, _w, Tc, idx, _i = rec
        Mp = B * S * Tc
        al = lambda v: (v + 255) // 256 * 256                                                   # noqa: E731
        off = al(al(4 * F * Mp * 4) + 2 * F * Mp * 4)
        o2 = cx[off:off + N * Mp * 4].view(torch.float32).view(B * S, Tc, N).cpu()
        gate = (o2 > 0).float()[:, idx[0].cpu().long(), :]
        masks.append(gate.permute(0, 2, 1).contiguous())
    assert len(masks) == cfg.num_stages
    srcd = [s_.to(dev) for s_ in src]
    l_time = PIT_SISNR_time(dev, S, True)(estims=audio, input_sizes=sizes, target_attr=srcd)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, S, True, False)
    l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=srcd) for i, a in enumerate(aux)]
    loss = ((1 - 0.4) * l_time + 0.4 * sum(l_mag) / len(l_mag)) / S
    loss.backward()
    key = (B, T, seed)
    if share_oracle and key in _FROZEN_ORACLE:
        # the same inputs were already differentiated through the oracle with the gates of ANOTHER arithmetic's device forward: a handful of
        # gates of the 10^6 differ, which is far below the bars of the test that shares (plain bf16: 20 dB worst tensor, 30 dB median)
        sdl, o_audio, o_aux, o_loss = _FROZEN_ORACLE[key]
        return cfg, m, audio, aux, loss, sdl, o_audio, o_aux, o_loss
    sdl = tor.leaf_state(synth_state_dict(cfg, 0))
    orc.RELU_MASKS = iter(masks)
    try:
        o_audio, o_aux = tor.model_forward_train(sdl, cfg, x)
    finally:
        orc.RELU_MASKS = None
    o_loss, _, _ = tor.train_loss(o_audio, o_aux, src)
    o_loss.backward()
    if B == 1:
        _FROZEN_ORACLE[key] = (sdl, [a.detach() for a in o_audio], [[t_.detach() for t_ in a] for a in o_aux], o_loss.detach())
    return cfg, m, audio, aux, loss, sdl, o_audio, o_aux, o_loss


@pytest.mark.parametrize("B,bar", [(1, MIN_DB), pytest.param(4, B4_STEP_MIN_DB, marks=slow)])      # batch 4 x 4 s (106 s of oracle): round 6's batch-16 test covers the batch regime
def test_train_step_base_4s_gradients_match_oracle(B, bar):
    """The reference loop's step (engine.py:60-77: forward, full loss, backward) at its REAL length - Base, 4 s:
    8000-frame sequences at the top level, T' = 500 attention, every kernel of the bench's training step in its large-launch
    instantiation - with EVERY one of the 1312 gradient tensors checked against the oracle (auxiliary ReLU gates frozen to the device's,
    which removes the loss's only discontinuity).  Default bf16x3 arithmetic; one utterance at the 80 dB bar of the 0.5 s test, and (round 5,
    review round 4 weak #1) a batch of FOUR - 32 000 rows per top-level contraction, four times longer fp32 sums on both sides, BatchNorm
    statistics over four sequences - at the same bar (the margin did not shrink with the batch: 81.4 dB worst tensor against 81.6)."""
    T = 32000
    cfg, m, audio, aux, loss, sdl, o_audio, o_aux, o_loss = _frozen_gate_step("bf16x3", B, T, seed=41)
    soft = Soft("train_step.base_4s.bf16x3.full_frozen_gates" + ("" if B == 1 else f".b{B}"))
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0))
    soft.agree("aux", torch.stack([torch.stack(list(a), 0) for a in aux], 0),
               torch.stack([torch.stack([t_.detach()[..., :T] for t_ in a], 0) for a in o_aux], 0))
    assert abs(float(loss) - float(o_loss)) < 5e-3, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    dbs = []
    for k, p_ in m.named_parameters():
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, bar)
        if not k.endswith(STRUCTURAL_ZERO):
            dbs.append(REPORT.get(f"{soft.tag}.grad.{k}", 999.0))
    record(f"{soft.tag}.worst_grad_db", float(np.min(dbs)))
    record(f"{soft.tag}.median_grad_db", float(np.median(dbs)))
    assert len(dbs) > 1200
    soft.done()


def test_train_step_base_0p25s_batch16_gradients_match_oracle():
    """The bench's batch regime (round 6): a batch of SIXTEEN at Base width (0.25 s utterances, so the oracle stays cheap: the suite-time
    budget; 0.5 s measured the same bars) - 16 sequences in every BatchNorm statistic and weight-gradient contraction - with every
    gradient tensor against the oracle at the 80 dB bar of the batch-1 / batch-4 tests (auxiliary ReLU gates frozen to the device's)."""
    B, T = 16, 2000
    cfg, m, audio, aux, loss, sdl, o_audio, o_aux, o_loss = _frozen_gate_step("bf16x3", B, T, seed=43)
    soft = Soft("train_step.base_0p25s.bf16x3.full_frozen_gates.b16")
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0))
    assert abs(float(loss) - float(o_loss)) < 5e-3, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    dbs = []
    for k, p_ in m.named_parameters():
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, MIN_DB)
        if not k.endswith(STRUCTURAL_ZERO):
            dbs.append(REPORT.get(f"{soft.tag}.grad.{k}", 999.0))
    record(f"{soft.tag}.worst_grad_db", float(np.min(dbs)))
    record(f"{soft.tag}.median_grad_db", float(np.median(dbs)))
    assert len(dbs) > 1200
    soft.done()


# plain-bf16 whole-step bars (operand rounding 2^-9 per product, ~130 blocks deep): per tensor BF16_STEP_MIN_DB, median BF16_STEP_MEDIAN_DB
BF16_STEP_MIN_DB, BF16_STEP_MEDIAN_DB = 20.0, 30.0   # measured (round 4): min 27.2 / 27.6, median 35.0 / 41.1 dB


@pytest.mark.parametrize("B,T", [(1, 32000)])        # (round 4 also ran (2, 4000): median 35.0 dB, min 27.2 dB; dropped for suite time)
def test_train_step_base_bf16_matches_oracle(B, T):
    """precision="bf16" (the arithmetic BASELINE configs[4] names) at Base width: the whole step at 0.5 s x 2 and at 4 s x 1 against
    the fp32 oracle (frozen gates).  A bf16 step is a different rounding of the same function, not a parity claim at 80 dB: the
    bar is BF16_STEP_MEDIAN_DB for the median tensor and BF16_STEP_MIN_DB for the worst one (a wrong kernel shows up below 10 dB:
    sign / scale / indexing errors are O(1)), forward outputs >= 30 dB, loss within 0.1."""
    # (seed 41 = the inputs of test_train_step_base_4s_gradients_match_oracle[1]: its oracle step is shared when it ran in this process)
    cfg, m, audio, aux, loss, sdl, o_audio, o_aux, o_loss = _frozen_gate_step("bf16", B, T, seed=41, share_oracle=True)
    tag = f"train_step.base_{T}x{B}.bf16"
    soft = Soft(tag, "bf16")
    soft.agree("main", torch.stack(list(audio), 0), torch.stack([a.detach() for a in o_audio], 0), 30.0)
    record(f"{tag}.loss_abs_dev", abs(float(loss) - float(o_loss)))
    assert abs(float(loss) - float(o_loss)) < 0.1, (float(loss), float(o_loss))
    gscale = max(float(v.grad.abs().max()) for v in sdl.values() if v.requires_grad and v.grad is not None)
    dbs = []
    for k, p_ in m.named_parameters():
        agree_grad(soft, "grad." + k, k, p_.grad, sdl[k].grad, gscale, BF16_STEP_MIN_DB)
        if f"{tag}.grad.{k}" in REPORT:
            dbs.append(REPORT[f"{tag}.grad.{k}"])
    record(f"{tag}.grad_db_median", float(np.median(dbs)))
    record(f"{tag}.grad_db_min", float(np.min(dbs)))
    assert float(np.median(dbs)) >= BF16_STEP_MEDIAN_DB, float(np.median(dbs))
    soft.done()


def test_training_loop_learns_bf16():
    """The 12-step AdamW loop of test_training_loop_learns_and_is_reproducible in precision="bf16": the loss of a plain-bf16 model
    goes down as well, by at least 80 % of what the default arithmetic achieves on the same data, and the trajectory is bitwise
    reproducible."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    cfg = VARIANTS["tiny"]
    dev = torch.device("cuda:0")
    B, T = 4, 2000
    srcn = synth_sources(B, T, seed=5) * 4.0
    src = [torch.from_numpy(srcn[:, s].copy()).to(dev) for s in range(2)]
    x = (src[0] + src[1]).contiguous()
    sizes = torch.full((B,), T)

    def run(precision, steps=12):
        torch.manual_seed(1234)
        m = Model.from_config(cfg, init_seed=0, precision=precision).to(dev)
        m.train()
        opt = torch.optim.AdamW(m.parameters(), lr=1.0e-3, weight_decay=1.0e-2)
        crit_t = PIT_SISNR_time(dev, 2, True)
        crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, 2, True, False)
        losses = []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            audio, aux = m(x)
            l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=src) for i, a in enumerate(aux)]
            loss = (0.6 * crit_t(estims=audio, input_sizes=sizes, target_attr=src) + 0.4 * sum(l_mag) / len(l_mag)) / 2
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
            opt.step()
            losses.append(float(loss))
        return losses

    ref = run("bf16x3")
    l1, l2 = run("bf16"), run("bf16")
    record("train_loop.tiny.bf16.loss_first", l1[0])
    record("train_loop.tiny.bf16.loss_last", l1[-1])
    assert all(np.isfinite(l1)) and l1 == l2, (l1, l2)
    assert l1[0] - l1[-1] >= 0.8 * (ref[0] - ref[-1]) and l1[-1] < l1[0] - 1.0, (l1, ref)


def test_training_loop_base_width_60_steps_bf16_follows_bf16x3():
    """Round-4 review item 8: longer evidence that a plain-bf16 model TRAINS at Base width.  SepReformer_Base_WSJ0, 0.5 s, batch 4, 60 AdamW
    steps (clip 5, dropout live, FlatAdamW) in precision "bf16" and in "bf16x3" on the same data and seeds: the bf16 trajectory goes down
    (every 10-step mean below the one before), ends within 5 % of the bf16x3 final loss (relative to the total decrease), and is
    bitwise reproducible."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    dev = torch.device("cuda:0")
    B, T = 4, 4000
    srcn = synth_sources(B, T, seed=7) * 4.0
    src = [torch.from_numpy(srcn[:, s].copy()).to(dev) for s in range(2)]
    x = (src[0] + src[1]).contiguous()
    sizes = torch.full((B,), T)

    def run(precision, steps=60):
        torch.manual_seed(4321)
        m = Model.from_config(cfg, init_seed=0, precision=precision).to(dev)
        m.train()
        opt = FlatAdamW(m, lr=2.0e-4, weight_decay=1.0e-2)
        crit_t = PIT_SISNR_time(dev, 2, True)
        crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, 2, True, False)
        losses = []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            audio, aux = m(x)
            l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=src) for i, a in enumerate(aux)]
            loss = (0.6 * crit_t(estims=audio, input_sizes=sizes, target_attr=src) + 0.4 * sum(l_mag) / len(l_mag)) / 2
            loss.backward()
            opt.step(max_norm=5.0)
            losses.append(loss.detach())
        return [float(v) for v in torch.stack(losses).cpu()]

    ref = run("bf16x3")
    l1, l2 = run("bf16"), run("bf16")
    for k, v in (("first", l1[0]), ("last", l1[-1]), ("x3_last", ref[-1])):
        record(f"train_loop.base_0p5s.bf16.loss_{k}", v)
    assert all(np.isfinite(l1)) and l1 == l2, "bf16 trajectory not reproducible"
    means = [sum(l1[i:i + 10]) / 10 for i in range(0, 60, 10)]
    assert all(b < a for a, b in zip(means, means[1:])), means
    drop_ref, drop = ref[0] - sum(ref[-5:]) / 5, l1[0] - sum(l1[-5:]) / 5
    assert drop_ref > 1.0 and abs(drop - drop_ref) <= 0.05 * drop_ref + 0.1, (drop, drop_ref, l1[-5:], ref[-5:])


def test_train_graphs_survive_a_larger_shape():
    """captured training graphs bake the engine's scratch-workspace pointer in.  Shape A, then a LARGER shape B
    (the engine allocates a bigger workspace), then A again: the replayed A step must still equal the eager A step bitwise (the
    graph keeps its workspace alive), in both capture levels (Model.train_graphs and CapturedTrainStep's engine)."""
    from sepreformer_amd.model import Model
    cfg = dataclasses.replace(VARIANTS["tiny"], dropout=0.0)
    dev = torch.device("cuda:0")
    xa = torch.from_numpy(synth_sources(2, 1500, seed=3).sum(1)).to(dev)
    xb = torch.from_numpy(synth_sources(6, 6000, seed=4).sum(1)).to(dev)

    def step(m, x):
        for p_ in m.parameters():
            p_.grad = None
        audio, aux = m(x)
        (torch.stack(audio).pow(2).sum() + sum(torch.stack(a).abs().sum() for a in aux)).backward()
        return torch.stack([a.detach().clone() for a in audio]), torch.cat([p_.grad.reshape(-1) for p_ in m.parameters()]).clone()

    me = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(dev).train()
    ya_e, ga_e = step(me, xa)
    mg = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(dev).train()
    mg.train_graphs = True
    ya1, ga1 = step(mg, xa)
    ws_a = mg.__dict__["_train_engine"]._ws
    step(mg, xb)                                                  # bigger scratch: the engine re-allocates
    assert mg.__dict__["_train_engine"]._ws is not ws_a
    junk = torch.full((ws_a.numel() // 4 + 1024,), float("nan"), device=dev)     # would land in the freed workspace if it had been freed
    ya2, ga2 = step(mg, xa)
    del junk
    assert torch.equal(ya1, ya_e) and torch.equal(ga1, ga_e)
    assert torch.equal(ya2, ya_e) and torch.equal(ga2, ga_e)
    # overlapping forwards of one shape in graph mode raise instead of returning wrong gradients
    a1, _ = mg(xa)
    a2, _ = mg(xa)
    with pytest.raises(RuntimeError, match="ONE static tape"):
        torch.stack(a1).sum().backward()
    torch.stack(a2).sum().backward()


@pytest.mark.parametrize("variant,n,T", [("SepReformer_Base_WSJ0", 3, 1201), ("SepReformer_Base_WSJ0", 5, 4000), ("tiny", 4, 333)])
def test_gcfn_bf16_plane_staged_backward_equals_register_staged(variant, n, T, monkeypatch):
    """The plain-bf16 GCFN pair in its two backward forms - (a) round 3: x / dy staged through registers (normalise / mask / round in
    the middle kernel, fp32 operands in the contractions), (b) round 4: the forward keeps the bf16 rows, a pre-pass writes
    bf16(dropout(dy)), the middle kernel stages both by LDS-DMA (three workgroups per CU) and the contractions read bf16 - round the
    same values at the same places and run the same MFMA order, so with dropout live (p = 0.3, same seed) the block output, the input
    gradient and every parameter gradient are BITWISE equal - except net2.2's bias gradient (and the LayerScale gradient that contains
    it), whose column sums are taken over the bf16 rows in form (b): bf16-level agreement there."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    cfg = dataclasses.replace(VARIANTS[variant], dropout=0.3)
    sd = synth_state_dict(cfg, 0)
    dev = torch.device("cuda:0")
    sdd = {k: v.to(dev) for k, v in sd.items()}
    F = cfg.feat
    x, dy = rnd(n, T, F, seed=T).cuda(), rnd(n, T, F, seed=T + 7).cuda()
    outs = []
    pfx = "separator.enc_stages.0.g_block_1.block.gcfn"
    # (both forms on the register-staged contraction: gemm_tn16_kernel - which form (b) runs by default - sums the same products in another order;
    #  test_bf16_blocks_tn16_contraction_agrees_with_register_staged compares the two contractions)
    monkeypatch.setenv("SEPR_TN16", "0")
    for planes in ("0", "1"):
        monkeypatch.setenv("SEPR_TRAIN_GCFN_PLANES", planes)
        gb = GradBuffer(cfg, dev)
        tp = TrainPack(cfg, sdd, gb, "bf16")
        eng = TrainEngine(cfg, dev)
        y, rec = eng.block_fwd("gcfn", x, tp.gcfn[0], n, T, 0, 0.3, 4242)
        assert (rec[2].numel() > n * T * F * 2) == (planes == "1")          # the context keeps the bf16 rows only in the plane form
        dx = eng.block_bwd(rec, dy)
        torch.cuda.synchronize()
        grads = {k[len(pfx) + 1:]: gb.view(k).clone() for k in sd if k.startswith(pfx + ".")}
        outs.append((y.clone(), dx.clone(), grads))
    assert torch.isfinite(outs[0][1]).all() and all(float(v.abs().max()) > 0 for v in outs[0][2].values())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for k, a_ in outs[0][2].items():
        b_ = outs[1][2][k]
        if k in ("net2.2.bias", "Layer_scale.layer_scale"):
            # the one place the two forms round differently: the column sums of dropout(dy) (bias gradient of net2.2, and through it
            # the LayerScale gradient) ride in the contraction's staging registers - fp32 values in form (a), the bf16 rows in form (b)
            assert orc.agreement_db(b_.cpu(), a_.cpu()) >= 45.0, (k, orc.agreement_db(b_.cpu(), a_.cpu()))
        elif k.startswith("depthwise."):
            # round 6: form (b) sums the depthwise partials of a workgroup's row tiles in registers when the launch has more tiles than
            # workgroups (n * T = 20 000 here), form (a) keeps one partial row per tile: the same per-tile sums, added in another order
            assert orc.agreement_db(b_.cpu(), a_.cpu()) >= 100.0, (k, orc.agreement_db(b_.cpu(), a_.cpu()))
        else:
            assert torch.equal(a_, b_), (k, int((a_ != b_).sum()), float((a_ - b_).abs().max()))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("variant", ["SepReformer_Base_WSJ0", "SepReformer_Large_DM_WHAMR"])
def test_train_blocks_wide_core_equals_narrow(variant, precision, monkeypatch):
    """The training path's projections on the 128 x 256 wide core (what a batch-16 step runs from 65 000 rows up) vs the 128 x 128
    core: forced on for every eligible launch (SEPR_X3_WIDE=2) vs off (0), dropout live so that the residual + dropout epilogue
    (EPI_RESDROP) and the GLU + saved pre-activation epilogue (EPI_GLUSAVE) run on both cores, plain-bf16 (TAG 16 / bf16-input TAG 48)
    and bf16x3 instantiations: block outputs, input gradients and ALL parameter gradients are bitwise equal."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    cfg = dataclasses.replace(VARIANTS[variant], dropout=0.3)
    sd = synth_state_dict(cfg, 0)
    dev = torch.device("cuda:0")
    sdd = {k: v.to(dev) for k, v in sd.items()}
    F = cfg.feat
    n, T = 2 * cfg.num_spks, 800
    x, dy = rnd(n, T, F, seed=3).cuda(), rnd(n, T, F, seed=4).cuda()
    outs = []
    for mode in ("0", "2"):
        monkeypatch.setenv("SEPR_X3_WIDE", mode)
        sdm = {k: v.clone() for k, v in sdd.items()}                       # (BatchNorm running statistics are updated by the CLA forward)
        gb = GradBuffer(cfg, dev)
        tp = TrainPack(cfg, sdm, gb, precision)
        eng = TrainEngine(cfg, dev)
        res = []
        for kind, w, Tp in (("gcfn", tp.gcfn[0], 0), ("cla", tp.cla[0], 0), ("ega", tp.ega[0], T // 8), ("spk", tp.spk[0], 0)):
            y, rec = eng.block_fwd(kind, x, w, n, T, Tp, 0.3, 99)
            dx = eng.block_bwd(rec, dy)
            res += [y.clone(), dx.clone()]
        torch.cuda.synchronize()
        outs.append(res + [gb.flat.clone()])
    for i, (a_, b_) in enumerate(zip(outs[0], outs[1])):
        assert torch.isfinite(a_).all() and torch.equal(a_, b_), (i, int((a_ != b_).sum()))
    assert float(outs[0][-1].abs().max()) > 0


@pytest.mark.parametrize("n,T", [(3, 1201), (4, 8000)])
def test_cla_bf16_stored_intermediates_equal_fp32_stored(n, T, monkeypatch):
    """Plain-bf16 precision, CLA block: c, d = gelu(bn(z)), dz and da stored as bf16 (SEPR_TRAIN_CLA16, default) vs as fp32.  Every reader
    of those four tensors is an MFMA operand loader that rounds to bf16, so the block output, the input gradient and every parameter
    gradient that does not pass through a column sum of da are BITWISE equal; linear1's bias gradient is the column sum of da (taken
    over the bf16 rows in the new form), and linear1.weight / the LayerNorm affine contain it: bf16-level agreement there."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=0.3)
    sd = synth_state_dict(cfg, 0)
    dev = torch.device("cuda:0")
    F = cfg.feat
    x, dy = rnd(n, T, F, seed=T).cuda(), rnd(n, T, F, seed=T + 7).cuda()
    pfx = "separator.enc_stages.0.l_block_1.block.cla"
    outs = []
    monkeypatch.setenv("SEPR_TN16", "0")          # (see test_gcfn_bf16_plane_staged_backward_equals_register_staged)
    for mode in ("0", "1"):
        monkeypatch.setenv("SEPR_TRAIN_CLA16", mode)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        gb = GradBuffer(cfg, dev)
        tp = TrainPack(cfg, sdd, gb, "bf16")
        eng = TrainEngine(cfg, dev)
        y, rec = eng.block_fwd("cla", x, tp.cla[0], n, T, 0, 0.3, 4242)
        dx = eng.block_bwd(rec, dy)
        torch.cuda.synchronize()
        outs.append((y.clone(), dx.clone(), {k[len(pfx) + 1:]: gb.view(k).clone() for k in sd if k.startswith(pfx + ".") and k in gb.offsets},
                     sdd[pfx + ".BN.running_var"].clone()))
    assert torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][3], outs[1][3])
    scale = max(float(v.abs().max()) for v in outs[0][2].values())
    for k, a_ in outs[0][2].items():
        b_ = outs[1][2][k]
        if k == "linear2.bias":
            # column sum of dz in front of a train-mode BatchNorm: identically zero in exact arithmetic (STRUCTURAL_ZERO), rounding noise in
            # both forms (fp32 dz vs bf16 dz rows)
            assert float(a_.abs().max()) <= 3e-2 * scale and float(b_.abs().max()) <= 3e-2 * scale, (k, float(a_.abs().max()), float(b_.abs().max()), scale)
        elif k.startswith(("linear1.", "layer_norm.")):
            if float(a_.abs().max()) > 0:
                assert orc.agreement_db(b_.cpu(), a_.cpu()) >= 45.0, (k, orc.agreement_db(b_.cpu(), a_.cpu()))
        else:
            assert torch.equal(a_, b_), (k, int((a_ != b_).sum()), float((a_ - b_).abs().max()), float(a_.abs().max()))


@pytest.mark.parametrize("kind,n,T,on", [("gcfn", 3, 1201, "1"), ("gcfn", 4, 8000, "1"), ("cla", 3, 1201, "1"), ("cla", 4, 8000, "1")])
def test_bf16_blocks_tn16_contraction_agrees_with_register_staged(kind, n, T, on, monkeypatch):
    """Plain-bf16 precision, GCFN and CLA blocks with dropout live: the weight-gradient contractions of two bf16 operands on gemm_tn16_kernel
    (default) vs on the register-staged gemm_tn_kernel (SEPR_TN16=0).  Nothing else changes, so block output and input gradient are bitwise
    equal; the parameter gradients are the same bf16 products summed in fp32 in another order."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    cfg = dataclasses.replace(VARIANTS["SepReformer_Base_WSJ0"], dropout=0.3)
    sd = synth_state_dict(cfg, 0)
    dev = torch.device("cuda:0")
    F = cfg.feat
    x, dy = rnd(n, T, F, seed=T).cuda(), rnd(n, T, F, seed=T + 7).cuda()
    pfx = "separator.enc_stages.0." + ("g_block_1.block.gcfn" if kind == "gcfn" else "l_block_1.block.cla")
    outs = []
    for mode in ("0", on):
        monkeypatch.setenv("SEPR_TN16", mode)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        gb = GradBuffer(cfg, dev)
        tp = TrainPack(cfg, sdd, gb, "bf16")
        eng = TrainEngine(cfg, dev)
        y, rec = eng.block_fwd(kind, x, (tp.gcfn if kind == "gcfn" else tp.cla)[0], n, T, 0, 0.3, 4242)
        dx = eng.block_bwd(rec, dy)
        torch.cuda.synchronize()
        outs.append((y.clone(), dx.clone(), {k[len(pfx) + 1:]: gb.view(k).clone() for k in sd if k.startswith(pfx + ".") and k in gb.offsets}))
    assert torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    scale = max(float(v.abs().max()) for v in outs[0][2].values())
    differ = 0
    for k, a_ in outs[0][2].items():
        b_ = outs[1][2][k]
        differ += int(not torch.equal(a_, b_))
        if float(a_.abs().max()) <= 3e-2 * scale and k == "linear2.bias":
            continue                                           # (structural zero in front of the train-mode BatchNorm: rounding noise in both)
        if float(a_.abs().max()) > 0:
            assert orc.agreement_db(b_.cpu(), a_.cpu()) >= 95.0, (k, orc.agreement_db(b_.cpu(), a_.cpu()))
    assert differ > 0          # the switch reached the library (the two kernels do not sum in the same order)


@pytest.mark.parametrize("variant,n,T,Tp", [("SepReformer_Base_WSJ0", 4, 2000, 500), ("SepReformer_Large_DM_WHAMR", 2, 520, 130)])
def test_ega_bf16_single_mfma_attention_agrees_with_the_triple(variant, n, T, Tp, monkeypatch):
    """Plain-bf16 precision, EGA block: the attention kernels with ONE bf16 MFMA per product (SEPR_TRAIN_ATTN_ONE, default) against the
    bf16x3 triple they ran with before (the projections around them are plain bf16 in both).  Two roundings of the same function at
    the precision's own level: the block output agrees to >= 55 dB (the residual dominates it), the input gradient to >= 45 dB and
    every parameter gradient to >= BF16_DB; dk = 16 (Base) and dk = 32 (Large), dropout on (the same masks in both forms)."""
    from sepreformer_amd.train_engine import TrainEngine
    from sepreformer_amd.train_pack import GradBuffer, TrainPack
    cfg = dataclasses.replace(VARIANTS[variant], dropout=0.1)
    sd = synth_state_dict(cfg, 0)
    dev = torch.device("cuda:0")
    F = cfg.feat
    x, dy = rnd(n, T, F, seed=T).cuda(), rnd(n, T, F, seed=T + 7).cuda()
    outs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("SEPR_TRAIN_ATTN_ONE", mode)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        gb = GradBuffer(cfg, dev)
        tp = TrainPack(cfg, sdd, gb, "bf16")
        eng = TrainEngine(cfg, dev)
        y, rec = eng.block_fwd("ega", x, tp.ega[0], n, T, Tp, 0.1, 777)
        dx = eng.block_bwd(rec, dy)
        torch.cuda.synchronize()
        pfx = tp.block_prefixes["ega"][0]
        outs.append((y.clone(), dx.clone(), {k[len(pfx) + 1:]: gb.view(k).clone() for k in sd if k.startswith(pfx + ".") and k in gb.offsets}))
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    assert not torch.equal(outs[0][0], outs[1][0])                      # the switch is live
    tag = f"ega_one_vs_triple.{variant}"
    y_db, dx_db = orc.agreement_db(outs[1][0].cpu(), outs[0][0].cpu()), orc.agreement_db(outs[1][1].cpu(), outs[0][1].cpu())
    record(f"{tag}.y", y_db)
    record(f"{tag}.dx", dx_db)
    assert y_db >= 55.0 and dx_db >= 45.0, (y_db, dx_db)
    worst = 1e9
    for k, a_ in outs[0][2].items():
        if float(a_.abs().max()) == 0.0 or k.endswith("linear_k.bias"):      # (linear_k.bias: structurally zero gradient)
            continue
        db = orc.agreement_db(outs[1][2][k].cpu(), a_.cpu())
        worst = min(worst, db)
        assert db >= BF16_DB, (k, db)
    record(f"{tag}.grad_db_min", worst)


# ---------------------------------------------------------------------------------------------------------------------
# optimizer step (round 4): clip_grad_norm_ + AdamW over the flat gradient buffer (sepr_adamw_step, sepreformer_amd.optim)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 0.05, 1.0e4])
def test_flat_adamw_matches_torch_adamw(max_norm):
    """engine.py:76-77 as three launches: after each of 4 steps every parameter, both moments and the returned norm equal
    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW fed the SAME gradients (fp32 rounding of one update apart: 1e-5 of the
    learning rate + 1 ulp of the parameter, per step taken); max_norm 0.05 clips on every step, 1e4 never does, None skips the norm pass."""
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    cfg = dataclasses.replace(VARIANTS["tiny"], dropout=0.0)
    dev = torch.device("cuda:0")
    lr = 1.0e-2
    ma = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(dev).train()
    mb = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(dev).train()
    oa = FlatAdamW(ma, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1.0e-2)
    ob = torch.optim.AdamW(mb.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1.0e-2)
    pa, pb = list(ma.parameters()), list(mb.parameters())
    for it in range(4):
        x = torch.from_numpy(synth_sources(2, 1500, seed=70 + it).sum(1) * 4.0).to(dev)
        oa.zero_grad(set_to_none=True)
        audio, aux = ma(x)
        (torch.stack(audio).pow(2).mean() + 0.1 * sum(torch.stack(a).abs().mean() for a in aux)).backward()
        for a_, b_ in zip(pa, pb):
            b_.grad = a_.grad.detach().clone()
        if it == 2:
            for g_ in (oa.param_groups[0], ob.param_groups[0]):       # a scheduler's update reaches the device scalar
                g_["lr"] = lr / 4
        gn_b = torch.nn.utils.clip_grad_norm_(pb, max_norm) if max_norm is not None else None
        ob.step()
        gn_a = oa.step(max_norm=max_norm)
        cur = lr / 4 if it >= 2 else lr
        if max_norm is not None:
            assert abs(float(gn_a) - float(gn_b)) <= 2e-6 * float(gn_b), (it, float(gn_a), float(gn_b))
            want = min(1.0, max_norm / (float(gn_b) + 1e-6))
            assert abs(float(oa.clip_coef) - want) <= 1e-6 * want
            assert (want < 1.0) == (max_norm == 0.05)
        else:
            assert gn_a is None
        worst = 0.0
        for a_, b_ in zip(pa, pb):
            tol = (it + 1) * (2e-5 * cur + 1.5e-7 * float(b_.detach().abs().max()))     # rounding differences add up over the steps
            d = float((a_.detach() - b_.detach()).abs().max())
            worst = max(worst, d / tol)
        assert worst <= 1.0, (it, worst)
        for a_, b_ in zip(pa, pb):
            sa, sb = oa.state[a_], ob.state[b_]
            assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-6 * float(sb["exp_avg"].abs().max()) + 1e-30)
            assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-6 * float(sb["exp_avg_sq"].abs().max()) + 1e-30)
        assert float(oa.state[pa[0]]["step"]) == it + 1
    # the state dict has torch.optim.AdamW's layout: loading it into a fresh FlatAdamW continues the same trajectory
    sd = oa.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and len(sd["state"]) == len(pa)
    mc = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(dev).train()
    mc.load_state_dict(ma.state_dict())
    oc = FlatAdamW(mc, lr=lr / 4, weight_decay=1.0e-2)
    oc.load_state_dict(sd)
    x = torch.from_numpy(synth_sources(2, 1500, seed=99).sum(1) * 4.0).to(dev)
    for m_, o_ in ((ma, oa), (mc, oc)):
        o_.zero_grad(set_to_none=True)
        audio, aux = m_(x)
        (torch.stack(audio).pow(2).mean() + 0.1 * sum(torch.stack(a).abs().mean() for a in aux)).backward()
        o_.step(max_norm=max_norm)
    for a_, c_ in zip(pa, mc.parameters()):
        assert torch.equal(a_.detach(), c_.detach())


def test_captured_step_with_flat_adamw_follows_torch_adamw():
    """CapturedTrainStep with optim.FlatAdamW (clip inside the optimizer graph) against the same captured step with torch's fused
    AdamW + clip_grad_norm_: 5 replays on the tiny model without dropout; the losses agree to 1e-5 relative (the two optimizers differ
    by fp32 rounding of the update), the reported gradient norms to 1e-5."""
    from sepreformer_amd.criterion import PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    cfg = dataclasses.replace(VARIANTS["tiny"], dropout=0.0)
    dev = torch.device("cuda:0")
    B, T = 2, 2000
    srcn = synth_sources(B, T, seed=12) * 4.0
    src = [torch.from_numpy(srcn[:, s].copy()).to(dev) for s in range(2)]
    x = (src[0] + src[1]).contiguous()
    sizes = torch.full((B,), T)

    def run(flat):
        m = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(dev).train()
        crit = PIT_SISNR_time(dev, 2, True)
        opt = FlatAdamW(m, lr=1.0e-3, weight_decay=1.0e-2) if flat else torch.optim.AdamW(m.parameters(), lr=1.0e-3, weight_decay=1.0e-2,
                                                                                             capturable=True)

        def loss_fn(audio, aux, *tg):
            return crit(estims=audio, input_sizes=sizes, target_attr=list(tg)) + 0.05 * sum(torch.stack(a).abs().mean() for a in aux)

        st = CapturedTrainStep(m, loss_fn, opt, x, src, max_norm=0.5, warmup=1)
        out = []
        for _ in range(5):
            loss, gn = st(x, src)
            out.append((float(loss.detach()), float(gn)))
        st.release()
        return out

    a, b = run(True), run(False)
    # (3e-5, round 6: the two optimizers round the update differently and five steps amplify it - 1.1e-5 on the fifth step's gradient norm
    #  since the auxiliary decoder sums its K steps in two accumulators; 0.4e-5 ... 1.0e-5 before)
    for (la, ga), (lb, gb_) in zip(a, b):
        assert abs(la - lb) <= 3e-5 * max(1.0, abs(lb)), (a, b)
        assert abs(ga - gb_) <= 3e-5 * gb_, (a, b)
    assert a[-1][0] < a[0][0]


@pytest.mark.gpu
def test_general_loader_two_workgroups_per_cu():
    """Round 3's fault shape class: the weight-gradient contraction's GENERAL loader normalising its B rows with two
    workgroups per CU - wrong, run-to-run different even columns of the upper tile half until round 5 pinned the packed-f32 form and
    removed the LDS pad that had kept the loader at one workgroup per CU.  SEPR_TN_FORCE_GEN=1 (latched per process: a subprocess) routes
    the public wgrad entry through that loader at 20 000 - 128 000 rows; every arithmetic must repeat bitwise and agree with fp64."""
    import subprocess
    env = dict(os.environ, SEPR_TN_FORCE_GEN="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tn_general_loader.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if "wgrad_norm" in ln]
    assert len(lines) == 9, out.stdout
    bar = {"x3=0": 1e-5, "x3=1": 1e-4, "x3=2": 2e-2}
    for ln in lines:
        assert "[gen=1" in ln and "repeats_equal=True" in ln, ln
        err = float(ln.split("max_rel_err=")[1].split()[0])
        assert err <= next(v for k, v in bar.items() if k + ":" in ln), ln


@pytest.mark.gpu
def test_device_repack_equals_torch_formulation():
    """Round 5: the per-step weight re-pack runs on the device (sepr_train_pack_lin / sepr_train_fold_bias, one launch per stack of projections,
    parameters read in place through pointer tables).  Against the batched torch formulation rounds 2-4 used - fold in fp64, transpose,
    bf16 hi / lo split, fragment permutation - the packed bytes must be IDENTICAL and the folded biases equal to one fp32 ulp."""
    from sepreformer_amd.train_pack import _Stack
    dev = torch.device("cuda:0")

    def pack_x3_batched(w):
        G, N, K = w.shape
        hi = w.to(torch.bfloat16)
        lo = (w - hi.to(torch.float32)).to(torch.bfloat16)

        def frag(p):
            return p.view(G, N // 16, 16, K // 32, 4, 8).permute(0, 1, 3, 4, 2, 5)

        return torch.stack([frag(hi), frag(lo)], dim=3).contiguous()

    G, F = 5, 128
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: (torch.randn(*s, generator=g) * 0.3).to(dev)          # noqa: E731
    for name, SN, SK, panels in (("up", 6 * F, F, 1), ("qkv", 3 * F, F, 3), ("down", F, 3 * F, 1), ("proj", 64, 256, 1)):
        w = [[rn(SN // panels, SK) for _ in range(panels)] for _ in range(G)]
        b = [[rn(SN // panels) for _ in range(panels)] for _ in range(G)]
        col, row, beta = [1.0 + rn(SK) for _ in range(G)], [1.0 + rn(SN) for _ in range(G)], [rn(SK) for _ in range(G)]
        W = torch.stack([torch.cat(ws, 0) for ws in w], 0)                                      # [G,SN,SK]
        B = torch.stack([torch.cat(bs, 0) for bs in b], 0)
        C, R_, BE = torch.stack(col, 0), torch.stack(row, 0), torch.stack(beta, 0)
        keep = []
        # forward form: gamma folded per column, beta folded into the bias
        s = _Stack(keep, w, (SN, SK), "bf16x3", b=b, scale=col, scale_kind=1, beta=beta)
        wf = (W.double() * C.double()[:, None, :]).float()
        assert torch.equal(s.wp.view(torch.int16), pack_x3_batched(wf).reshape(G, -1).view(torch.int16)), name
        bf = (B.double() + torch.einsum("gnk,gk->gn", W.double(), BE.double())).float()
        assert float((s.b - bf).abs().max()) <= 2.0 * float(torch.finfo(torch.float32).eps * bf.abs().max()), name
        # input-gradient forms: transposed, gamma per source column / LayerScale per source row
        st_ = _Stack(keep, w, (SN, SK), "bf16", scale=col, scale_kind=1, transpose=True)
        assert st_.planes == 1 and torch.equal(st_.wp.view(torch.int16), pack_x3_batched(wf.transpose(1, 2).contiguous()).reshape(G, -1).view(torch.int16)), name
        sr = _Stack(keep, w, (SN, SK), "bf16x3", scale=row, scale_kind=2, transpose=True)
        assert torch.equal(sr.wp.view(torch.int16), pack_x3_batched((W * R_[:, :, None]).transpose(1, 2).contiguous()).reshape(G, -1).view(torch.int16)), name
        # plain forms: no fold; exact-f32 layout; bias gather without a fold
        sp = _Stack(keep, w, (SN, SK), "bf16x3", b=b)
        assert torch.equal(sp.wp.view(torch.int16), pack_x3_batched(W).reshape(G, -1).view(torch.int16)) and torch.equal(sp.b, B), name
        s32 = _Stack(keep, w, (SN, SK), "fp32", scale=col, scale_kind=1, transpose=True)
        assert s32.wp is None and torch.equal(s32.w, wf.transpose(1, 2).contiguous()), name
        assert s.lin(2).wp == s.wp.data_ptr() + 2 * 2 * 2 * SN * SK and s.lin(2).b == s.b.data_ptr() + 4 * 2 * SN
    with pytest.raises(ValueError):
        _Stack([], [[rn(24, 32)]], (24, 32), "bf16x3")                   # not whole MFMA fragments


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 128])
def test_device_gcfn_fused_pack_equals_torch_packer(F):
    """sepr_train_pack_gcfn_fused (one launch for a stack of GCFN blocks, parameters read in place) against pack.pack_gcfn_fused_batched - the
    torch formulation whose per-block equality with the inference packer a CPU test pins: fragments and conv constants bit-identical, the
    fp64-folded biases to one fp32 ulp."""
    from sepreformer_amd.pack import pack_gcfn_fused_batched
    from sepreformer_amd.train_pack import _table
    dev = torch.device("cuda:0")
    G = 3
    g = torch.Generator().manual_seed(F)
    rn = lambda *s: (torch.randn(*s, generator=g) * 0.4).to(dev)          # noqa: E731
    w1, b1, lg, lb = [rn(6 * F, F) for _ in range(G)], [rn(6 * F) for _ in range(G)], [1.0 + rn(F) for _ in range(G)], [rn(F) for _ in range(G)]
    w2, dw, db = [rn(F, 3 * F) for _ in range(G)], [rn(6 * F, 1, 3) for _ in range(G)], [rn(6 * F) for _ in range(G)]
    st = lambda ts: torch.stack(ts, 0)                                     # noqa: E731
    want1, want2 = pack_gcfn_fused_batched(st(w1), st(b1), st(lg), st(lb), st(w2), st(dw).reshape(G, 6 * F, 3), st(db))
    KS, nch = F // 32, 3 * F // 32
    got1 = torch.full((G, nch * (4 * KS * 2048 + 4096)), 0xAB, dtype=torch.uint8, device=dev)
    got2 = torch.empty(G, nch, F // 16, 2, 64, 8, dtype=torch.bfloat16, device=dev)
    L.check(L.load().sepr_train_pack_gcfn_fused(*[_table(t).data_ptr() for t in (w1, b1, lg, lb, w2, dw, db)], G, F, got1.data_ptr(), got2.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "sepr_train_pack_gcfn_fused")
    torch.cuda.synchronize()
    assert want1.shape == got1.shape and torch.equal(got2.view(torch.int16), want2.view(torch.int16))
    chunk = 4 * KS * 2048 + 4096
    a, b = got1.view(G, nch, chunk), want1.view(G, nch, chunk)
    assert torch.equal(a[:, :, :4 * KS * 2048], b[:, :, :4 * KS * 2048])                      # up-projection fragments
    ca, cb = a[:, :, 4 * KS * 2048:].contiguous().view(torch.float32).view(G, nch, 1024), b[:, :, 4 * KS * 2048:].contiguous().view(torch.float32).view(G, nch, 1024)
    assert torch.equal(ca[:, :, 320:], cb[:, :, 320:]) and float(ca[:, :, 320:].abs().max()) == 0.0
    cav, cbv = ca[:, :, :320].view(G, nch, 2, 10, 16), cb[:, :, :320].view(G, nch, 2, 10, 16)
    assert torch.equal(cav[:, :, :, 2:], cbv[:, :, :, 2:])                                      # taps and conv biases (fp64 products)
    assert float((cav[:, :, :, :2] - cbv[:, :, :, :2]).abs().max()) <= 2.0 * float(torch.finfo(torch.float32).eps * cbv[:, :, :, :2].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_deferred_finishers_equal_immediate(precision):
    """Round 5: TrainEngine.backward queues the ~320 gradient-finisher launches of a step (sepr_train_defer_begin / _flush) and runs them as a
    few batched launches.  The batched kernel is the immediate kernels' code per job, jobs that accumulate into the same tensor never share
    a launch, launches keep queue order - so every gradient must be BIT-identical to the immediate form (forced here by an arena too small
    for any slot).  Base width so that EGA (three finishers per block, q / k / v sharing dgamma) and every block kind take part."""
    from sepreformer_amd.model import Model
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    dev = torch.device("cuda:0")
    m = Model.from_config(cfg, init_seed=0, precision=precision).load_synthetic_(0).to(dev)
    m.train()
    m.dropout_p = 0.0
    x = torch.from_numpy(synth_sources(2, 4000, seed=3).sum(1)).to(dev)

    def grads():
        m.zero_grad(set_to_none=True)
        audio, aux = m(x)
        (sum(a.square().mean() for a in audio) + sum(b.square().mean() for lvl in aux for b in lvl)).backward()
        return {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    g_def = grads()
    eng = m.__dict__["_train_engine"]
    assert eng._fin_arena is not None and eng._fin_arena.numel() > (32 << 20)
    big = eng._fin_arena
    eng._fin_arena = torch.empty(4096, dtype=torch.uint8, device=dev)          # no slot fits: every finisher launches immediately
    g_imm = grads()
    eng._fin_arena = big
    g_def2 = grads()
    bad = [k for k in g_def if not (torch.equal(g_def[k], g_imm[k]) and torch.equal(g_def[k], g_def2[k]))]
    assert not bad, bad[:8]
    assert all(torch.isfinite(v).all() for v in g_def.values())
