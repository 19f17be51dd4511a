"""The source-aggregated, soft-thresholded SDR criteria on the device: ``sepr_pit_sasdr_fwd/_bwd`` and
``sepr_pit_sasdr_mag_fwd/_bwd`` against the float64 restatement tests/sasdr_ref.py of the float32 inputs, on silent targets and the other
hard inputs, at the lengths where the kernels take another path; run to run, under graph capture, with a guard behind the workspace; the
feed with ``absent=1.0``; three steps of ``Trainer(criterion="sasdr")``, twice, and cut and resumed.

Bounds (none is taken from what the code under test returns):
  * time forward: one float32 ulp of the value plus 1e-9 dB - the moments are fp64 and ``tau D`` takes the cancellation out of ``E``;
  * magnitude forward: ``2 * MAG_FWD_SIBLING_DB``, twice the largest error of ``sepr_pit_sisnr_mag_fwd`` against ITS float64 restatement
    (oracle/criterion_oracle.py) over the same inputs - the same f32 projection feeds both;
  * backward, ``|dest - ref|_2 / |ref|_2`` per (s, b): ``2 * TIME_BWD_SIBLING`` / ``2 * MAG_BWD_SIBLING``, twice what ``sepr_pit_sisnr_bwd`` /
    ``sepr_pit_sisnr_mag_bwd`` reach on their active rows (a finite, non-zero float64 gradient) over the same inputs; where the float64
    gradient is exactly 0 the device's is exactly 0.
The three sibling figures were measured on an MI355X with ``sibling_figures`` below (the manner of tests/test_criterion_hard_gpu.py) and
are recorded in DESIGN.md section 5e-7.  The family ``equal`` is left out of them: ``est == tgt`` is the singular point of the SI-SNR
forms (R = 0, the value is set by eps and by the rounding of the residual: the magnitude sibling is 1.3 to 4.3 dB from float64 there and
its gradient rows are off by 100 %), which is no active pair and would make the bounds say nothing.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_ref as cr                                                   # noqa: E402
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_turns_ref as turns_ref                                         # noqa: E402
import sasdr_ref as sr                                                       # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
N, HOP = 512, 128
T_OF = {"time": [4, 4095, 4096, 4097, 8193],          # PIT_CHUNK = 4096: a few samples, one short of a chunk, a chunk, one past, two and one
        "mag": [512, 640, 8193]}                        # one frame, a frame that straddles the pad, many frames
FAMILIES = ["plain", "one_silent", "all_silent", "silent_est", "equal", "dc", "amp_1e-4", "amp_1e4", "tie"]

MAG_FWD_SIBLING_DB = 6.822e-6    # sepr_pit_sisnr_mag_fwd, S = 3, T = 512, all_silent
TIME_BWD_SIBLING = 1.831e-6      # sepr_pit_sisnr_bwd, S = 3, T = 4, silent_est
MAG_BWD_SIBLING = 1.173e-5       # sepr_pit_sisnr_mag_bwd, S = 2, T = 8193, plain


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(S, T, family):
    """(est, tgt) float32 ``[S, B, T]``.  The estimates follow the targets speaker-swapped (est_s ~ tgt_(s+1) % S), so the permutation is not
    the identity; every row carries a DC offset unless the family says otherwise."""
    g = torch.Generator().manual_seed(1000 * S + T + 7 * FAMILIES.index(family))
    nxt = [(s + 1) % S for s in range(S)]
    tgt = 0.1 * torch.randn(S, B, T, generator=g) + 0.05
    nz = torch.randn(S, B, T, generator=g)
    if family == "one_silent":                            # one talker says nothing in the window; the estimate that belongs to it is quiet noise
        tgt[0] = 0.0
    elif family == "all_silent":
        tgt[:, :2] = 0.0
    est = tgt[nxt] + 0.03 * nz
    if family == "one_silent":
        est[nxt.index(0)] = torch.tensor([1.0e-1, 1.0e-3, 1.0e-5])[:, None] * nz[nxt.index(0)]
    elif family == "all_silent":
        est[:, 0] = 0.1 * nz[:, 0]
        est[:, 1] = 1.0e-4 * nz[:, 1]
    elif family == "silent_est":
        est[0, 0] = 0.0
        est[S - 1, 1] = 0.0
    elif family == "equal":
        est = tgt[nxt].clone()                            # bit for bit: loss = 10 log10(tau) up to eps, gradient exactly 0
    elif family == "dc":
        # DC-only rows at values whose T-fold sums are exact in float32 products and float64 sums: the mean is the value itself on both
        # sides, the zero-mean row is exactly 0, and the case has one answer.  b = 0: a DC-only estimate; 1: a DC-only target; 2: both
        est[0, 0] = 0.5
        tgt[0, 1] = -0.25
        est[0, 2] = 2.0
        tgt[nxt[0], 2] = 0.375
    elif family == "amp_1e-4":
        est, tgt = 1.0e-4 * est, 1.0e-4 * tgt
    elif family == "amp_1e4":
        est, tgt = 1.0e4 * est, 1.0e4 * tgt
    elif family == "tie":
        est[1 % S] = est[0]                               # two equal estimates: the tied permutations are bit-equal sums, the first wins
    return est.contiguous(), tgt.contiguous()


def cases(kind, S):
    return [(T, f) for T in T_OF[kind] for f in FAMILIES if not (f == "tie" and S == 1)]


def weights():
    return torch.linspace(0.5, 2.0, B)


@functools.lru_cache(maxsize=None)
def kernel():
    from sepreformer_amd.criterion import stft_kernel
    return stft_kernel(N, HOP)


@functools.lru_cache(maxsize=None)
def reference(kind, S, T, family):
    """float64: (loss [B], perm [B, S], E of every permutation [P, B], d (loss . w) / d est [S, B, T]) - computed once, never written to."""
    est, tgt = build(S, T, family)
    if kind == "time":
        return sr.autograd(sr.sasdr_time, est, tgt, weights())
    return sr.autograd(sr.sasdr_mag, est, tgt, weights(), frame_len=N, frame_hop=HOP, K=kernel()[:N + 2])


@functools.lru_cache(maxsize=None)
def crit_mag(S):
    from sepreformer_amd.criterion import PIT_SASDR_mag
    return PIT_SASDR_mag(torch.device(DEV), N, HOP, "hann", 1, S)


def device(kind, S, est, tgt):
    """(forward loss [B], perm [B, S], the Function's loss [B], d (loss . w) / d est) from the device, on the host."""
    from sepreformer_amd.criterion import _SaSdrMagFn, _SaSdrTimeFn, pit_sasdr, pit_sasdr_mag
    e, t, w = est.to(DEV).requires_grad_(True), tgt.to(DEV), weights().to(DEV)
    if kind == "time":
        out = pit_sasdr(e.detach(), t)
        per = _SaSdrTimeFn.apply(e, t, sr.EPS_TIME, sr.SNR_MAX)
    else:
        c = crit_mag(S)
        out = pit_sasdr_mag(e.detach(), t, c._dft, N, HOP)
        per = _SaSdrMagFn.apply(e, t, c._dft, c._dft_t, N, HOP, sr.EPS_MAG, sr.SNR_MAX)
    (per * w).sum().backward()
    torch.cuda.synchronize()
    return out["loss"].cpu(), out["perm"].cpu().long(), per.detach().cpu(), e.grad.cpu()


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def perm_decided(allE):
    """Per utterance: the two smallest E_p differ by more than 1e-9 relative (or there is one permutation)."""
    if allE.shape[0] == 1:
        return torch.ones(allE.shape[1], dtype=torch.bool)
    two = torch.sort(allE, dim=0).values[:2]
    return (two[1] - two[0]) > 1.0e-9 * two[1]


def row_errors(grad, g64):
    """-> (relative L2 error of every row whose float64 gradient is not 0 [(s, b, value)], rows that must be exactly 0 and are not)."""
    rel, nonzero = [], []
    for s in range(g64.shape[0]):
        for b in range(g64.shape[1]):
            want = g64[s, b]
            if float(want.abs().max()) == 0.0:
                if float(grad[s, b].abs().max()) != 0.0:
                    nonzero.append((s, b, float(grad[s, b].abs().max())))
            else:
                rel.append((s, b, float((grad[s, b].double() - want).norm() / want.norm())))
    return rel, nonzero


def sibling_figures(kind, S):
    """What the SI-SNR sibling reaches against its own float64 restatement over the same inputs: (largest forward error in dB over the finite
    utterances, largest relative L2 error over its active gradient rows).  The measurement behind the three constants above."""
    from sepreformer_amd.criterion import PIT_SISNR_mag, _PitMagFn, _PitTimeFn
    fwd = bwd = 0.0
    for T, family in cases(kind, S):
        if family == "equal":                             # the SI-SNR forms' singular point: see the module docstring
            continue
        est, tgt = build(S, T, family)
        l64, _, g64 = cr.autograd(est, tgt, weights(), kind, torch.float64)
        e, t, w = est.to(DEV).requires_grad_(True), tgt.to(DEV), weights().to(DEV)
        if kind == "time":
            per = _PitTimeFn.apply(e, t, cr.EPS["time"], cr.CLAMP_MIN)
        else:
            c = PIT_SISNR_mag(torch.device(DEV), N, HOP, "hann", 1, S, True, False)
            per = _PitMagFn.apply(e, t, c._dft, c._dft_t, N, HOP, cr.EPS["mag"])
        (per * w).sum().backward()
        torch.cuda.synchronize()
        ok = torch.isfinite(l64) & torch.isfinite(per.detach().cpu().double())
        err = float((per.detach().cpu().double() - l64)[ok].abs().max()) if bool(ok.any()) else 0.0
        rows = [r for r in row_errors(e.grad.cpu(), g64)[0] if np.isfinite(r[2]) and bool(torch.isfinite(g64[r[0], r[1]]).all())]
        worst = max([r[2] for r in rows], default=0.0)
        print(f"sibling {kind} S{S} T{T} {family}: forward error {err:.3e} dB, backward {worst:.3e} over {len(rows)} active rows")
        fwd, bwd = max(fwd, err), max(bwd, worst)
    return fwd, bwd


# ---- forward and backward against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("kind", ["time", "mag"])
def test_against_float64(kind, S):
    bad = []
    worst_f = worst_b = 0.0
    bwd_bound = 2.0 * (TIME_BWD_SIBLING if kind == "time" else MAG_BWD_SIBLING)
    for T, family in cases(kind, S):
        est, tgt = build(S, T, family)
        l64, p64, allE, g64 = reference(kind, S, T, family)
        loss, perm, per, grad = device(kind, S, est, tgt)
        name = f"{kind}.S{S}.T{T}.{family}"
        assert torch.isfinite(l64).all() and torch.isfinite(g64).all(), name       # the criterion is defined on every one of these inputs
        if not torch.equal(loss, per):
            bad.append(f"{name}: the autograd Function's loss differs from the forward entry's")
        decided = perm_decided(allE)
        tied = allE.shape[0] > 1 and (torch.sort(allE, dim=0).values[0] == torch.sort(allE, dim=0).values[1])
        for b in range(B):
            # decided: float64's permutation; an exact tie (two equal estimates, every target silent): the first minimiser on both sides
            if (bool(decided[b]) or (allE.shape[0] > 1 and bool(tied[b]))) and perm[b].tolist() != p64[b].tolist():
                bad.append(f"{name}: perm[{b}] {perm[b].tolist()} != {p64[b].tolist()}")
            err = abs(float(loss[b]) - float(l64[b]))
            tol = ulp32(l64[b]) + 1.0e-9 if kind == "time" else 2.0 * MAG_FWD_SIBLING_DB
            worst_f = max(worst_f, err / tol)
            print(f"{name}.b{b}: loss {float(loss[b]):.7f} float64 {float(l64[b]):.9f} error {err:.3e} dB (tolerance {tol:.3e})")
            if not err <= tol:
                bad.append(f"{name}: loss[{b}] {float(loss[b]):.7f} vs {float(l64[b]):.9f}: {err:.3e} dB > {tol:.3e}")
        if family == "equal":
            want = 10.0 * np.log10(sr.tau_of())
            if T >= 512 and not float((loss.double() - want).abs().max()) < 1.0e-2:
                bad.append(f"{name}: est == tgt gives {loss.tolist()}, not 10 log10(tau) = {want:.3f} dB")
            if float(grad.abs().max()) != 0.0:
                bad.append(f"{name}: est == tgt, gradient max|.| {float(grad.abs().max()):.3e}, not 0")
        if not torch.isfinite(grad).all():
            bad.append(f"{name}: non-finite gradient")
            continue
        rel, nonzero = row_errors(grad, g64)
        for s, b, top in nonzero:
            bad.append(f"{name}: dest[{s}, {b}] max|.| {top:.3e} where the float64 gradient is exactly 0")
        for s, b, r in rel:
            worst_b = max(worst_b, r)
            print(f"{name}.dest{s}.b{b}: relative error {r:.3e} (bound {bwd_bound:.3e})")
            if not r <= bwd_bound:
                bad.append(f"{name}: dest[{s}, {b}] relative error {r:.3e} > {bwd_bound:.3e}")
    print(f"{kind} S{S}: worst forward error / tolerance {worst_f:.3f}, worst backward relative error {worst_b:.3e} (bound {bwd_bound:.3e})")
    assert not bad, f"{len(bad)} failed: " + "; ".join(bad[:40])


def test_silent_target_families_hold_what_they_say():
    """The inputs are what the cases claim: silent rows are all zeros, the deliberate ties are the only undecided permutations."""
    for kind in ("time", "mag"):
        for S in (2, 3):
            for T, family in cases(kind, S):
                est, tgt = build(S, T, family)
                _, _, allE, _ = reference(kind, S, T, family)
                undecided = ~perm_decided(allE)
                if family == "tie":
                    assert bool(undecided.all()) and torch.equal(est[0], est[1])
                elif family == "all_silent":
                    assert undecided.tolist() == [True, True, False] and float(tgt[:, :2].abs().max()) == 0.0
                else:
                    assert not bool(undecided.any()), (kind, S, T, family)
                if family == "one_silent":
                    assert float(tgt[0].abs().max()) == 0.0


def test_call_surface_returns_num_spks_times_the_mean():
    from sepreformer_amd.criterion import PIT_SASDR_time
    S, T = 2, 4097
    est, tgt = build(S, T, "one_silent")
    l64, _, _, _ = reference("time", S, T, "one_silent")
    sizes = torch.full((B,), T)
    crit_t = PIT_SASDR_time(torch.device(DEV), S)
    for kind, crit, kw in (("time", crit_t, {}), ("mag", crit_mag(S), {"idx": 0})):
        want = device(kind, S, est, tgt)[0]
        for grad in (False, True):
            out = crit(estims=[e.to(DEV).requires_grad_(grad) for e in est], target_attr=[t.to(DEV) for t in tgt], input_sizes=sizes, **kw)
            assert out.requires_grad == grad and out.dim() == 0
            assert float(out.detach()) == float(S * torch.sum(want.to(DEV)) / B)
        with pytest.raises(RuntimeError, match="expected 2 estimates"):
            crit(estims=[est[0].to(DEV)], target_attr=[tgt[0].to(DEV)], input_sizes=sizes, **kw)
    assert abs(float(crit_t(estims=list(est.to(DEV)), target_attr=list(tgt.to(DEV)), input_sizes=sizes)) - S * float(l64.mean())) < 1e-4
    with pytest.raises(IndexError):
        crit_mag(S)(estims=list(est.to(DEV)), target_attr=list(tgt.to(DEV)), input_sizes=sizes, idx=1)


# ---- run to run, capture, guard ---------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", ["time", "mag"])
def test_run_to_run_bit_equal(kind):
    S, T = 3, 8193
    est, tgt = build(S, T, "one_silent")
    a, b = device(kind, S, est, tgt), device(kind, S, est, tgt)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(bits(a[3]), bits(b[3]))


@pytest.mark.parametrize("kind", ["time", "mag"])
def test_under_graph_capture(kind):
    """Forward and backward captured on one input, replayed on another written into the static tensors: the bits of the eager run."""
    from sepreformer_amd.criterion import _SaSdrMagFn, _SaSdrTimeFn
    S, T = 2, 4097
    first, second = build(S, T, "plain"), build(S, T, "one_silent")
    e = first[0].to(DEV).requires_grad_(True)
    t = first[1].to(DEV)
    w = weights().to(DEV)
    c = crit_mag(S)

    def run():
        if kind == "time":
            per = _SaSdrTimeFn.apply(e, t, sr.EPS_TIME, sr.SNR_MAX)
        else:
            per = _SaSdrMagFn.apply(e, t, c._dft, c._dft_t, N, HOP, sr.EPS_MAG, sr.SNR_MAX)
        (g,) = torch.autograd.grad((per * w).sum(), e)
        return per.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        per, g = run()
    for est, tgt in (second, first):
        with torch.no_grad():
            e.copy_(est)
            t.copy_(tgt)
        graph.replay()
        torch.cuda.synchronize()
        want = device(kind, S, est, tgt)
        assert torch.equal(bits(per.cpu()), bits(want[0])) and torch.equal(bits(g.cpu()), bits(want[3]))


@pytest.mark.parametrize("S,T", [(1, 4097), (3, 640)])
def test_guard_behind_the_workspace_is_untouched(S, T):
    """The four entries on workspaces of exactly the siblings' sizes with a filled region behind each; one byte less is refused."""
    lib = L.load()
    est, tgt = build(S, T, "one_silent")
    e, t, gl = est.to(DEV), tgt.to(DEV), weights().to(DEV)
    c = crit_mag(S)
    G = 4096
    stream = torch.cuda.current_stream().cuda_stream
    loss, perm, dest = torch.empty(B, device=DEV), torch.empty(B, S, dtype=torch.int32, device=DEV), torch.empty_like(e)
    sizes = {"time_fwd": lib.sepr_workspace_bytes(L.OP_PIT, B, T, 0, 0, 0, S),
             "time_bwd": lib.sepr_workspace_bytes(L.OP_PIT, B, T, 0, 0, 0, S) + 16 * B * S + 512,
             "mag_fwd": lib.sepr_pit_sisnr_mag_workspace(S, B, T, N, HOP), "mag_bwd": lib.sepr_pit_sisnr_mag_bwd_workspace(S, B, T, N, HOP)}

    def call(which, ws, nbytes):
        if which == "time_fwd":
            return lib.sepr_pit_sasdr_fwd(e.data_ptr(), t.data_ptr(), S, B, T, 1e-8, 30.0, loss.data_ptr(), perm.data_ptr(), ws.data_ptr(), nbytes, stream)
        if which == "time_bwd":
            return lib.sepr_pit_sasdr_bwd(e.data_ptr(), t.data_ptr(), perm.data_ptr(), gl.data_ptr(), S, B, T, 1e-8, 30.0, dest.data_ptr(),
                                          ws.data_ptr(), nbytes, stream)
        if which == "mag_fwd":
            return lib.sepr_pit_sasdr_mag_fwd(e.data_ptr(), t.data_ptr(), S, B, T, c._dft.data_ptr(), N, HOP, 1e-12, 30.0, loss.data_ptr(),
                                              perm.data_ptr(), ws.data_ptr(), nbytes, stream)
        return lib.sepr_pit_sasdr_mag_bwd(e.data_ptr(), t.data_ptr(), perm.data_ptr(), gl.data_ptr(), S, B, T, c._dft.data_ptr(), c._dft_t.data_ptr(),
                                          N, HOP, 1e-12, 30.0, dest.data_ptr(), ws.data_ptr(), nbytes, stream)

    for which in ("time_fwd", "time_bwd", "mag_fwd", "mag_bwd"):
        nbytes = int(sizes[which])
        assert nbytes > 0
        block = torch.full((nbytes + G,), 0x5A, dtype=torch.uint8, device=DEV)
        assert call(which, block, 8) == L.SEPR_EWORKSPACE                     # refused before any launch
        assert call(which, block, nbytes) == L.SEPR_OK, which
        torch.cuda.synchronize()
        assert bool((block[nbytes:] == 0x5A).all()), which
        assert bool(torch.isfinite(loss).all()) and (which.endswith("fwd") or bool(torch.isfinite(dest).all()))


# ---- the feed ---------------------------------------------------------------------------------------------------------------------------
def fixture(golden):
    g = golden("dynmix")
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    c.roles = dict(roles)
    return c, [str(k) for k in g["keys"]], arrays


def test_feed_with_an_absent_talker(golden):
    """``DynamicMixFeed`` over ``partial(plan_wham, turns=..., absent=1.0)``, B = 4, T = 4096: every example has one target row that is +0.0
    in every bit, and the batch equals tests/dynmix_turns_ref.py on the same plan."""
    corpus, keys, arrays = fixture(golden)
    Bf, T = 4, 4096
    turns = df.Turns((0.0, 0.5), 40)
    feed = df.DynamicMixFeed(corpus, functools.partial(df.plan_wham, turns=turns, absent=1.0), batch=Bf, max_len=T, seed=3, fixed_length=True)
    assert feed.absent == 1.0 and feed.turns == turns
    assert df.DynamicMixFeed(corpus, functools.partial(df.plan_wham, turns=turns), batch=Bf, max_len=T, seed=3, fixed_length=True).absent == 0.0
    with pytest.raises(ValueError, match="turns"):
        df.DynamicMixFeed(corpus, functools.partial(df.plan_wham, absent=0.5), batch=Bf, max_len=T, seed=3, fixed_length=True)
    sizes, mix, src, _ = next(iter(feed))
    plan = feed.last_plan
    FAR = df.TURN_FAR
    assert plan.on is not None and mix.shape == (Bf, T)
    gone = (plan.on[:, plan.M:] == FAR) & (plan.off[:, plan.M:] == FAR)
    assert gone.sum(1).tolist() == [1] * Bf
    assert np.array_equal(plan.on[:, :2], plan.on[:, plan.M:]) and (plan.on[:, 2] == -FAR).all() and (plan.off[:, 2] == FAR).all()
    for b in range(Bf):
        s = int(np.argmax(gone[b]))
        assert bool((bits(src[s][b]) == 0).all())                                # +0.0, not -0.0, padding included
        assert float(src[1 - s][b].abs().max()) > 0
    full = plan._replace(speed=np.full_like(plan.utt, 100), rir=np.full_like(plan.utt, -1), taps=np.ones_like(plan.utt))
    wm, ws = turns_ref.batch([arrays[nm] for nm in corpus.names], [], full.n, full.utt, full.start, full.norm, full.gain, full.speed, full.rir,
                             full.taps, full.on, full.off, turns_ref.ramp_table(turns.ramp), full.M, full.S, T)
    assert torch.equal(bits(mix.cpu()), bits(torch.from_numpy(wm))) and torch.equal(bits(torch.stack(src).cpu()), bits(torch.from_numpy(ws)))


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def make_trainer(corpus, keys, directory, criterion="sasdr", absent=0.5, **kw):
    import test_trainer_gpu as tt
    from sepreformer_amd import trainer as T
    planner = functools.partial(df.plan_wsj0, turns=df.Turns((0.0, 0.5), 40), **({"absent": absent} if absent else {}))
    train = df.DynamicMixFeed(corpus, planner, batch=tt.B, max_len=tt.MAXLEN, seed=3, fixed_length=True, keys=keys)
    valid = df.DynamicMixFeed(corpus, df.plan_direct, batch=tt.B, max_len=tt.MAXLEN, seed=4, drop_last=False)
    kw.setdefault("max_epoch", 3)
    kw.setdefault("log", lambda s: None)
    return T.Trainer(tt.tiny(0.0), train, valid, str(directory), lr=tt.LR, seed=11, warmup_steps=tt.WARMUP, criterion=criterion, **kw)


def state_bits(t):
    return [bits(v.detach().float().cpu()) for v in t.model.state_dict().values() if v.is_floating_point()]


def test_trainer_three_steps_twice(golden, tmp_path):
    """The tiny configuration with ``criterion="sasdr"`` on a feed with ``absent=0.5``: three steps, a finite ledger of ``1 + R`` parts, no
    step skipped, windows with a silent talker among the batches; a second run is bit-equal.  The SI-SNR pair is refused on this feed."""
    corpus, keys, _ = fixture(golden)
    six = (keys * 2)[:6]                                                         # three batches of two

    def run(directory):
        t = make_trainer(corpus, six, directory)
        assert t.criterion == "sasdr" and type(t.crit_t).__name__ == "PIT_SASDR_time" and type(t.crit_m).__name__ == "PIT_SASDR_mag"
        means = t.train_epoch(1)
        led = t.read_ledger()
        assert t.global_step == 3 and led.steps == 3 and led.skipped == 0 and led.nonfinite == 0 and t.nparts == 1 + t.cfg.num_stages
        assert all(np.isfinite(v) for v in led.values) and all(np.isfinite(m) for m in means[:2])
        out = (led.values, state_bits(t))
        t.release()
        return out

    a, b = run(tmp_path / "a"), run(tmp_path / "b")
    print("ledger", a[0])
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    plans = list(make_trainer(corpus, six, tmp_path / "p").train_feed.plans())
    gone = sum(int((p.on[:, p.M:] == df.TURN_FAR).sum()) for p in plans)
    assert 0 < gone < 6, gone                                                    # the epoch held windows with a silent talker and windows without
    with pytest.raises(ValueError, match="zero gradient"):
        make_trainer(corpus, six, tmp_path / "none", criterion="sisnr")


def test_trainer_resume_continues_bit_for_bit(golden, tmp_path):
    """Two epochs straight against one epoch, a checkpoint, fresh objects and one more epoch: the same bits.  The checkpoint records the
    criterion, and resuming it with the other one is refused."""
    import trainer_ref as tr
    from sepreformer_amd import trainer as T
    corpus, keys, _ = fixture(golden)
    whole = make_trainer(corpus, keys, tmp_path / "whole")
    whole.run()
    cut = make_trainer(corpus, keys, tmp_path / "cut", max_epoch=2)
    cut.run()
    del cut
    ck = T.read_checkpoint(T.latest_checkpoint(str(tmp_path / "cut")))
    assert ck[T.RUN_STATE_KEY]["criterion"] == "sasdr"
    with pytest.raises(ValueError, match="criterion"):
        make_trainer(corpus, keys, tmp_path / "cut", criterion="sisnr", absent=0.0).load_latest()
    again = make_trainer(corpus, keys, tmp_path / "cut")
    again.run()
    assert again.start_epoch == 2 and again.global_step == whole.global_step == 4
    assert again.last_train == whole.last_train and again.last_valid == whole.last_valid
    assert all(torch.equal(x, y) for x, y in zip(state_bits(again), state_bits(whole)))
    assert tr.same_bits(again.ledger, whole.ledger)
