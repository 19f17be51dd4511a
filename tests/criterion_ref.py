"""The training criteria judged forward and backward against float64 autograd on hard inputs and shape edges.  Shared by
tests/test_criterion_hard_cpu.py (the proof that the bars have teeth, reference side only) and tests/test_criterion_hard_gpu.py (the device
against the same cases).  Test infrastructure only; the pattern is tests/branch_ref.py's.

What is judged: ``sepr_pit_sisnr_fwd/_bwd`` and ``sepr_pit_sisnr_mag_fwd/_bwd`` (csrc/sepr_criterion.hip) through ``pit_sisnr`` / ``pit_sisnr_mag`` and
the autograd Functions ``_PitTimeFn`` / ``_PitMagFn`` of sepreformer_amd/criterion.py.  The judged scalar is ``(per_utt * w).sum()`` with
``w = linspace(0.5, 2, B)``, so the upstream gradient differs per utterance.

Three evaluations of one case (S, B, T, family):
  * ``reference``  float64 ``torch.autograd`` over oracle/criterion_oracle.py: per-utterance loss, permutation, ``d est``.
  * ``floor32``    the same in float32; ``floor_db`` is its agreement with float64, per gradient row.
  * ``restated``   the device's algorithm step by step in the precision the kernel states (fp64 moments and pair sums, float32 means,
    scales, coefficients, STFT products, apply / overlap-add passes); ``floor_dev_db`` is its agreement with float64.  With ``mutant=`` one
    planted defect.  It reads neither ``floor32`` nor a device.

A figure is one gradient row ``d est[s, b, :]`` (a whole-tensor figure is carried by the loudest row: with ``target_near_eps`` one estimate's
gradient is 1e4 x the others').  Rules:
  * ``"db"``    ``agreement_db(got_row, want_row) >= bar``, ``bar = min(80, floor_db - 6, floor_dev_db - 6)`` (MIN_DB / MARGIN_DB of branch_ref);
  * ``"zero"``  the float64 row is exactly 0 (a clamped term, a silent row): the row must be exactly 0 and finite;
  * permutations equal the float64 permutation on every case (``tie``: two equal estimates make the tied sums bit-equal in any order, so the
    first permutation wins on both sides);
  * losses within 2e-4 dB (time) / 2e-3 dB (mag) of float64 (the tolerances of tests/test_criterion.py), widened only to float32 autograd's own
    loss error where that is larger; an utterance whose exact loss is eps-dominated (>= 60 dB: a silent row) is held to finiteness and the
    10 dB of test_device_constant_signals_stay_finite.
No bar is taken from a device measurement.
"""
from __future__ import annotations

import math
import zlib
from itertools import permutations
from typing import Dict, List, Optional

import torch

from oracle import criterion_oracle as co
from oracle.sepreformer_oracle import agreement_db

from branch_ref import MARGIN_DB, MIN_DB

KINDS = ["time", "mag"]
FRAME_LEN, FRAME_HOP = 512, 128
EPS = {"time": 1.0e-8, "mag": 1.0e-12}
CLAMP_MIN = -30.0
SCALE_MIN = 1.0e-2
LOSS_TOL = {"time": 2.0e-4, "mag": 2.0e-3}
EPS_DOMINATED_DB, EPS_DOMINATED_TOL = 60.0, 10.0
FLOOR_OF_BARS_DB = 55.0                       # every bar but dc100's is at least this (the CPU proof asserts it)
PIT_CHUNK = 4096

FAMILIES = ["plain", "silent_est", "silent_tgt", "anti", "dc3", "dc100", "close60", "half_clamped", "tie", "quiet_est", "scale_edge",
            "target_near_eps"]
EVERY_PAIR = ["plain", "anti", "half_clamped"]
T_EDGES = [400, 512, 513, 4096, 4097]         # one frame after padding; exactly one frame; one past a hop (two frames); one chunk; a chunk + 1 sample
TIME_MUTANTS = ["time_no_clamp", "time_gl0", "time_no_sign", "time_no_et_term", "time_no_mean"]
MAG_MUTANTS = ["mag_scale_gate_open", "mag_no_scale_path", "mag_no_demean", "mag_pad_minus_mean", "mag_ola_drops_last_frame", "mag_no_sqrt_floor",
               "mag_identity_perm", "mag_gl0"]
MUTANTS = {"time": TIME_MUTANTS, "mag": MAG_MUTANTS}


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, S, B, T, family, salt=0):
        self.S, self.B, self.T, self.family = S, B, T, family
        self.tag = f"S{S}_B{B}_T{T}.{family}"
        self.seed = (zlib.crc32(self.tag.encode()) + salt) % (2 ** 31)
        self._built = None

    def __repr__(self):
        return self.tag

    def tensors(self):
        """(est, src) float32 ``[S, B, T]``; built once."""
        if self._built is None:
            self._built = build(self.S, self.B, self.T, self.family, self.seed)
        return self._built

    def weights(self):
        return torch.linspace(0.5, 2.0, self.B)


def build(S, B, T, family, seed):
    g = torch.Generator().manual_seed(seed)
    src = 0.1 * torch.randn(S, B, T, generator=g)
    nz = torch.randn(S, B, T, generator=g)
    nxt = [(s + 1) % S for s in range(S)]                              # speaker-swapped: the permutation is not the identity
    if family == "target_near_eps":
        src[0] *= 5.0e-5                                               # |t~|^2 ~ 2.5e-11 T: about the time loss's eps
    est = 0.7 * src[nxt] + 0.03 * nz
    if family == "plain":
        pass
    elif family == "silent_est":
        est[0, 0] = 0.0
    elif family == "silent_tgt":
        src[0, 0] = 0.0
    elif family == "anti":
        est[0] = -est[0]
    elif family == "dc3":
        est, src = est + 3.0, src - 2.0
    elif family == "dc100":
        est, src = est + 100.0, src - 50.0
    elif family == "close60":
        est = src[nxt] + 1.0e-4 * nz
    elif family == "half_clamped":
        est[0] = src[1 % S] + 1.0e-3 * nz[0]
    elif family == "tie":
        assert S >= 2
        est[1] = est[0]
    elif family == "quiet_est":
        est = 1.0e-4 * est
    elif family == "scale_edge":
        est[0] = 0.005 * src[1 % S] + 0.1 * nz[0]
    elif family == "target_near_eps":
        est[S - 1] = 0.7 * src[0] + 2.0e-6 * nz[S - 1]                 # the estimate that belongs to target 0
    else:
        raise KeyError(family)
    return est.contiguous(), src.contiguous()


# seeds at which the raw scale of (est_0, its target) has rows on both sides of 1e-2 (asserted by the CPU proof, never by the device)
_SALT = {"S2_B3_T400.scale_edge": 0, "S2_B3_T4097.scale_edge": 1}
SCALE_EDGE_MARGIN = 1.0e-3                                            # no row's raw scale within this of 1e-2: no arithmetic can flip the gate


def _cases() -> List[Case]:
    out = []
    for T in (400, 4097):
        out += [Case(2, 3, T, f, _SALT.get(f"S2_B3_T{T}.{f}", 0)) for f in FAMILIES]
    for S in (1, 2, 3):
        for T in T_EDGES:
            if S == 2 and T in (400, 4097):
                continue
            out += [Case(S, 3, T, f) for f in EVERY_PAIR]
    out.append(Case(2, 65, 512, "plain"))                              # mag_finalize_kernel: b = blockIdx.x * 64 + threadIdx.x
    return out


CASES: List[Case] = _cases()


def cases_for(S: int) -> List[Case]:
    return [c for c in CASES if c.S == S]


# ----------------------------------------------------------------------------------------------------------------------
# float64 / float32 autograd over the oracle
# ----------------------------------------------------------------------------------------------------------------------
def autograd(est, src, w, kind, dtype):
    """(per-utterance loss [B], permutation [B, S], d (loss . w) / d est [S, B, T]) of the oracle in ``dtype``."""
    e = est.to(dtype).clone().requires_grad_(True)
    t = src.to(dtype)
    with torch.enable_grad():
        if kind == "time":
            _, per, perm = co.pit_sisnr_time(list(e), list(t), eps=EPS["time"], dtype=dtype)
        else:
            _, per, perm = co.pit_sisnr_mag(list(e), list(t), FRAME_LEN, FRAME_HOP, eps=EPS["mag"], dtype=dtype)
        (per * w.to(dtype)).sum().backward()
    return per.detach(), perm.to(torch.int64), e.grad


def reference(case: Case, kind: str):
    est, src = case.tensors()
    return autograd(est, src, case.weights(), kind, torch.float64)


def floor32(case: Case, kind: str):
    est, src = case.tensors()
    return autograd(est, src, case.weights(), kind, torch.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the device's algorithm restated (csrc/sepr_criterion.hip), each step in the precision the kernel uses
# ----------------------------------------------------------------------------------------------------------------------
def _moments(est, src):
    """pit_partial_kernel + the finalisers' zero-mean forms, fp64: means [S,B] x 2, |a~|^2, |t~|^2 [S,B] (clamped at 0), <a~,t~> [S,S,B]."""
    e, t = est.double(), src.double()
    n = float(est.shape[-1])
    se, st = e.sum(-1), t.sum(-1)
    aa = ((e * e).sum(-1) - se * se / n).clamp_min(0.0)
    tt = ((t * t).sum(-1) - st * st / n).clamp_min(0.0)
    at = torch.einsum("sbt,kbt->skb", e, t) - se[:, None] * st[None] / n
    return se / n, st / n, aa, tt, at


def _walk(l):
    """The permutation walk of pit_finalize_kernel / mag_finalize_kernel over ``l[s, k, b]``: itertools order, the first optimum wins."""
    S, _, B = l.shape
    perms = list(permutations(range(S)))
    best = torch.zeros(B, dtype=torch.float64)
    arg = torch.zeros(B, dtype=torch.int64)
    for p, pm in enumerate(perms):
        sl = torch.zeros(B, dtype=torch.float64)
        for s in range(S):
            sl = sl + l[s, pm[s]]
        better = torch.ones(B, dtype=torch.bool) if p == 0 else sl < best
        best = torch.where(better, sl, best)
        arg = torch.where(better, torch.full_like(arg, p), arg)
    return best, torch.tensor(perms, dtype=torch.int64)[arg]          # [B], [B, S]


def _f32(x):
    return x.to(torch.float32)


def restate_time(est, src, gl, mutant: Optional[str] = None):
    """sepr_pit_sisnr_fwd + sepr_pit_sisnr_bwd: (loss float32 [B], perm [B,S], d est float32 [S,B,T])."""
    assert mutant is None or mutant in TIME_MUTANTS, mutant
    S, B, T = est.shape
    eps = EPS["time"]
    mean_a, mean_t, aa, tt, at = _moments(est, src)
    # forward: sisnr_db for every (s, k), clamp, walk
    alpha = at / (tt[None] + eps)
    num = alpha.abs() * tt[None].sqrt()
    res2 = (aa[:, None] - 2.0 * alpha * at + alpha * alpha * tt[None]).clamp_min(0.0)
    l = (-20.0 * torch.log10(eps + num / (res2.sqrt() + eps))).clamp_min(CLAMP_MIN)
    best, perm = _walk(l)
    # pit_bwd_coef_kernel, per (s, b) with k = perm[b, s]
    bi = torch.arange(B)
    g = _f32(gl).double()
    if mutant == "time_gl0":
        g = g[0].expand(B)
    ca, ct, mt = torch.zeros(S, B, dtype=torch.float64), torch.zeros(S, B, dtype=torch.float64), torch.zeros(S, B, dtype=torch.float64)
    for s in range(S):
        k = perm[:, s]
        tt_k, at_k, aa_s = tt[k, bi], at[s, k, bi], aa[s]
        c = tt_k + eps
        al = at_k / c
        P = al.abs() * tt_k.sqrt()
        R = (aa_s - 2.0 * al * at_k + al * al * tt_k).clamp_min(0.0).sqrt()
        u = P / (R + eps)
        loss = -20.0 * torch.log10(eps + u)
        live = R > 0.0
        if mutant != "time_no_clamp":
            live = live & (loss > CLAMP_MIN)
        Rs = torch.where(R > 0.0, R, torch.ones_like(R))
        gu = -(20.0 / math.log(10.0)) / (eps + u) * g
        et = at_k - al * tt_k
        sign = torch.where(al >= 0.0, 1.0, -1.0).double()
        if mutant == "time_no_sign":
            sign = torch.ones_like(sign)
        kt = gu * sign * tt_k.sqrt() / (c * (R + eps))
        ke = -gu * P / ((R + eps) * (R + eps) * Rs)
        ct_s = kt - ke * al - (0.0 if mutant == "time_no_et_term" else ke * et / c)
        ca[s] = torch.where(live, ke, torch.zeros_like(ke))
        ct[s] = torch.where(live, ct_s, torch.zeros_like(ct_s))
        mt[s] = mean_t[k, bi]
    ca32, ct32, ma32, mt32 = _f32(ca), _f32(ct), _f32(mean_a), _f32(mt)
    if mutant == "time_no_mean":
        ma32, mt32 = torch.zeros_like(ma32), torch.zeros_like(mt32)
    # pit_bwd_apply_kernel: o = fmaf(ca, a - ma, ct * (t - mt)) in float32 (the fma's product is exact in float64)
    tg = torch.stack([src[perm[:, s], bi] for s in range(S)], 0)                           # [S, B, T]: the permuted target of each estimate
    x = est - ma32[..., None]
    y = ct32[..., None] * (tg - mt32[..., None])
    dest = _f32(ca32[..., None].double() * x.double() + y.double())
    return _f32(best), perm, dest


_dft = {}


def _kernel():
    """The DFT kernel rows the device multiplies by (real rows, imaginary rows): float32 [N + 2, N]."""
    if "k" not in _dft:
        _dft["k"] = co.stft_kernel(FRAME_LEN, FRAME_HOP)[:, 0, :].to(torch.float32).contiguous()
    return _dft["k"]


def restate_mag(est, src, gl, mutant: Optional[str] = None):
    """sepr_pit_sisnr_mag_fwd + sepr_pit_sisnr_mag_bwd: (loss float32 [B], perm [B,S], d est float32 [S,B,T])."""
    assert mutant is None or mutant in MAG_MUTANTS, mutant
    S, B, T = est.shape
    N, hop, eps = FRAME_LEN, FRAME_HOP, EPS["mag"]
    nbin = N // 2 + 1
    Tpad = (T + hop - 1) // hop * hop
    nfr = (Tpad - N) // hop + 1
    assert nfr >= 1
    floor = torch.tensor(0.0 if mutant == "mag_no_sqrt_floor" else 1.0e-10, dtype=torch.float32)
    K = _kernel()
    mean_a, mean_t, aa, tt, at = _moments(est, src)
    # mag_scales_kernel: float32 means and clamped scales
    mu_e, mu_t = _f32(mean_a), _f32(mean_t)
    raw = at / (tt[None] + eps)                                                            # [S, S, B]
    sc = _f32(raw.clamp_min(SCALE_MIN))

    # stft_prep_kernel: zero-mean, zero-padded
    def prep(x, mu):
        z = torch.zeros(S, B, Tpad, dtype=torch.float32)
        z[..., :T] = x - mu[..., None]
        if mutant == "mag_pad_minus_mean":
            z[..., T:] = (-mu)[..., None]
        return z
    xe, xt = prep(est, mu_e), prep(src, mu_t)
    # the STFT projection: frames x kernel in float32
    Ce = xe.unfold(-1, N, hop) @ K.t()                                                     # [S, B, nfr, N + 2]
    Ct = xt.unfold(-1, N, hop) @ K.t()
    er, ei, tr, ti = Ce[..., :nbin], Ce[..., nbin:], Ct[..., :nbin], Ct[..., nbin:]
    me = torch.sqrt(er * er + ei * ei + floor)                                             # [S, B, nfr, nbin]
    # stft_pair_kernel: fp64 sums of M_s^2 and (M_e - M_s)^2 for every (s, k)
    P2 = torch.zeros(S, S, B, dtype=torch.float64)
    R2 = torch.zeros(S, S, B, dtype=torch.float64)
    for s in range(S):
        for k in range(S):
            c = sc[s, k][:, None, None]
            a, b_ = c * tr[k], c * ti[k]
            ms = torch.sqrt(a * a + b_ * b_ + floor)
            d = me[s].double() - ms.double()
            P2[s, k] = (ms.double() ** 2).sum((-1, -2))
            R2[s, k] = (d * d).sum((-1, -2))
    l = -20.0 * torch.log10(eps + P2.sqrt() / (R2.sqrt() + eps))
    best, perm = _walk(l)
    if mutant == "mag_identity_perm":
        perm = torch.arange(S).expand(B, S).clone()
        best = sum(l[s, s] for s in range(S))
    # backward
    bi = torch.arange(B)
    g = _f32(gl).double()
    if mutant == "mag_gl0":
        g = g[0].expand(B)
    dest = torch.zeros(S, B, T, dtype=torch.float32)
    for s in range(S):
        k = perm[:, s]
        scs = sc[s, k, bi][:, None, None]                                                  # [B, 1, 1]
        P, R = P2[s, k, bi].sqrt(), R2[s, k, bi].sqrt()
        u = P / (R + eps)
        gu = -(20.0 / math.log(10.0)) / (eps + u) * g
        kR = torch.where(R > 0.0, P / ((R + eps) * (R + eps) * torch.where(R > 0.0, R, torch.ones_like(R))), torch.zeros_like(R))
        ge = _f32(-gu * kR)[:, None, None]
        gs1 = _f32(torch.where(P > 0.0, gu / (torch.where(P > 0.0, P, torch.ones_like(P)) * (R + eps)), torch.zeros_like(P)))[:, None, None]
        gs2 = _f32(gu * kR)[:, None, None]
        # stft_pair_bwd_kernel (float32 per element, fp64 reduction of dL/dc)
        trk, tik = tr[k, bi], ti[k, bi]                                                    # [B, nfr, nbin]
        t2 = trk * trk + tik * tik
        ms = torch.sqrt(scs * scs * t2 + floor)
        d = me[s] - ms
        gme = ge * d
        De = torch.cat([gme * er[s] / me[s], gme * ei[s] / me[s]], -1)                     # [B, nfr, N + 2]
        gms = gs1 * ms + gs2 * d
        dLdc = (gms * scs * t2 / ms).double().sum((-1, -2))                                # [B]
        # adjoint projection, then stft_ola_kernel: the scale path, frames added from the last one that covers t down to the first
        fr = De @ K                                                                        # [B, nfr, N]
        tt_k = tt[k, bi]
        cs = _f32(dLdc / (tt_k + eps))
        if mutant == "mag_no_scale_path":
            cs = torch.zeros_like(cs)
        elif mutant != "mag_scale_gate_open":
            cs = torch.where(raw[s, k, bi] >= SCALE_MIN, cs, torch.zeros_like(cs))
        da = cs[:, None] * xt[k, bi]                                                       # [B, Tpad]
        last = nfr - 2 if mutant == "mag_ola_drops_last_frame" else nfr - 1
        for f in range(last, -1, -1):
            da[:, f * hop:f * hop + N] += fr[:, f]
        # demean_kernel
        if mutant == "mag_no_demean":
            dest[s] = da[:, :T]
        else:
            dest[s] = da[:, :T] - _f32(da[:, :T].double().sum(-1) / float(T))[:, None]
    return _f32(best), perm, dest


def restate(est, src, gl, kind, mutant=None):
    return (restate_time if kind == "time" else restate_mag)(est, src, gl, mutant)


def restated(case: Case, kind: str, mutant: Optional[str] = None):
    est, src = case.tensors()
    return restate(est, src, case.weights(), kind, mutant)


def raw_scale(case: Case):
    """The unclamped scale <a~, t~> / (|t~|^2 + eps) of every (estimate, target, utterance) in float64: [S, S, B]."""
    est, src = case.tensors()
    _, _, _, tt, at = _moments(est, src)
    return at / (tt[None] + EPS["mag"])


# ----------------------------------------------------------------------------------------------------------------------
# the inputs and the measure of tests/test_train_gpu.py::test_criteria_backward (what a mutant is held against "the old way")
# ----------------------------------------------------------------------------------------------------------------------
OLD_SHAPES = [(2, 6, 8000), (3, 4, 3001), (2, 2, 1500)]
OLD_BARS = {"time": (100.0, 80.0), "mag": (90.0, 60.0)}              # (mean loss, every d est_s as a whole [B, T] tensor), dB


def old_inputs(S, B, T):
    """(est, src) exactly as test_criteria_backward draws them."""
    g = torch.Generator().manual_seed(S * 100 + B)
    src = [0.1 * torch.randn(B, T, generator=g) + 0.01 * (s + 1) for s in range(S)]
    perm = [torch.randperm(S, generator=g).tolist() for _ in range(B)]
    est = [torch.stack([0.7 * src[perm[b][s]][b] + [0.3, 0.03, 0.001, 1.0][b % 4] * 0.1 * torch.randn(T, generator=g) + 0.02 for b in range(B)])
           for s in range(S)]
    return torch.stack(est, 0), torch.stack(src, 0)


_old_cache: Dict[tuple, tuple] = {}


def old_way(kind: str, mutant: Optional[str]) -> dict:
    """The restatement (with ``mutant``) measured as test_criteria_backward measures the device: uniform upstream gradient 1/B, the mean
    loss and every ``d est_s`` as one tensor against float64 autograd, 100 / 80 dB (time) and 90 / 60 dB (mag)."""
    fig = {}
    for S, B, T in OLD_SHAPES:
        est, src = old_inputs(S, B, T)
        w = torch.full((B,), 1.0 / B)
        key = (kind, S, B, T)
        if key not in _old_cache:
            _old_cache[key] = autograd(est, src, w, kind, torch.float64)
        l64, _, g64 = _old_cache[key]
        lm, _, gm = restate(est, src, w, kind, mutant)
        tag = f"S{S}_B{B}_T{T}"
        want = (l64.sum() / B).reshape(1).float()
        fig[f"{tag}.loss"] = agreement_db((lm.double().sum() / B).reshape(1).float(), want) - OLD_BARS[kind][0]
        for s in range(S):
            ok = bool(torch.isfinite(gm[s]).all())
            fig[f"{tag}.dest{s}"] = (agreement_db(gm[s], g64[s].float()) if ok else -999.0) - OLD_BARS[kind][1]
    low = min(fig, key=fig.get)
    bar = OLD_BARS[kind][0 if low.endswith(".loss") else 1]
    return {"lowest_figure": low, "lowest_agreement_db": fig[low] + bar, "its_bar_db": bar, "passes_old_bars": bool(fig[low] >= 0.0)}


# ----------------------------------------------------------------------------------------------------------------------
# floors, bars and the judgement shared by the CPU proof and the device test
# ----------------------------------------------------------------------------------------------------------------------
def row_db(got, want):
    """agreement_db of every gradient row: [S, B] floats (rows of ``want`` that are exactly 0 read nan)."""
    S, B, _ = want.shape
    out = torch.full((S, B), float("nan"), dtype=torch.float64)
    for s in range(S):
        for b in range(B):
            if float(want[s, b].abs().max()) > 0.0:
                out[s, b] = agreement_db(got[s, b], want[s, b])
    return out


_floor_cache: Dict[tuple, dict] = {}


def floors(case: Case, kind: str) -> dict:
    """Everything the reference side says about (case, kind): float64 loss / perm / gradient, per row the rule, ``floor_db``, ``floor_dev_db``
    and the bar, per utterance the loss tolerance.  Cached."""
    key = (case.tag, kind)
    r = _floor_cache.get(key)
    if r is None:
        l64, p64, g64 = reference(case, kind)
        l32, p32, g32 = floor32(case, kind)
        lr, pr, gr = restated(case, kind)
        zero = g64.abs().amax(-1) == 0.0                                                   # [S, B]
        f32db, fdev = row_db(g32, g64), row_db(gr, g64)
        bar = torch.minimum(torch.full_like(f32db, MIN_DB), torch.minimum(f32db, fdev) - MARGIN_DB)
        tol = torch.maximum(torch.full_like(l64, LOSS_TOL[kind]), (l32.double() - l64).abs())
        tol = torch.where(l64 >= EPS_DOMINATED_DB, torch.full_like(tol, EPS_DOMINATED_TOL), tol)
        r = {"loss64": l64, "perm64": p64, "g64": g64, "zero": zero, "floor_db": f32db, "floor_dev_db": fdev, "bar": bar, "loss_tol": tol,
             "finite": bool(torch.isfinite(l64).all() and torch.isfinite(g64).all()),
             "loss32": l32, "perm32": p32, "g32": g32, "restated": (lr, pr, gr)}
        _floor_cache[key] = r
    return r


def judge(case: Case, kind: str, loss, perm, grad, report: Optional[dict] = None, prefix: str = ""):
    """Every rule of the module docstring on one evaluation of (case, kind).  -> (list of failures, least ``figure - bar`` over the "db" rows or
    None).  ``report`` receives every figure under ``prefix``."""
    r = floors(case, kind)
    bad = []
    name = f"{prefix}{kind}.{case.tag}"
    loss, grad = loss.detach().double().cpu(), grad.detach().float().cpu()
    perm = perm.detach().to(torch.int64).cpu()
    if tuple(grad.shape) != tuple(r["g64"].shape) or tuple(loss.shape) != tuple(r["loss64"].shape):
        return [f"{name}: shapes {tuple(loss.shape)} / {tuple(grad.shape)}"], None
    if not torch.equal(perm, r["perm64"]):
        bad.append(f"{name}: permutation {perm.tolist()} != float64's {r['perm64'].tolist()}")
    if not torch.isfinite(loss).all():
        bad.append(f"{name}: non-finite loss {loss.tolist()}")
    else:
        err = (loss - r["loss64"]).abs()
        if report is not None:
            report[name + ".loss_err_db"] = float(f"{float(err.max()):.3e}")
        for b in range(case.B):
            if not err[b] <= r["loss_tol"][b]:
                bad.append(f"{name}: loss[{b}] {float(loss[b]):.6f} vs {float(r['loss64'][b]):.6f} (tolerance {float(r['loss_tol'][b]):.1e} dB)")
    least = None
    for s in range(case.S):
        for b in range(case.B):
            row = grad[s, b]
            rname = f"{name}.dest{s}.b{b}"
            if not torch.isfinite(row).all():
                bad.append(f"{rname}: non-finite gradient")
                if report is not None:
                    report[rname] = -999.0
                continue
            if bool(r["zero"][s, b]):
                top = float(row.abs().max())
                if report is not None and case.B <= 8:
                    report[rname + ".max_abs"] = top
                if top != 0.0:
                    bad.append(f"{rname}: max|.| {top:.3e} where the float64 gradient is exactly 0")
                continue
            db, need = agreement_db(row, r["g64"][s, b]), float(r["bar"][s, b])
            if report is not None and case.B <= 8:
                report[rname] = round(db, 2)
                report[rname + ".bar_db"] = round(need, 2)
            if least is None or db - need < least[0]:
                least = (db - need, rname, db, need)
            if not db >= need:
                bad.append(f"{rname}: {db:.1f} dB < bar {need:.1f} (float32 floor {float(r['floor_db'][s, b]):.1f}, restated floor "
                           f"{float(r['floor_dev_db'][s, b]):.1f})")
    return bad, least
