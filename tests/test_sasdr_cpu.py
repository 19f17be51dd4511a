"""The host side of training on windows with a silent talker: the planner's ``absent`` draw, the refusals, the four
``sepr_pit_sasdr_*`` entries across header, binding and library, and the float64 restatement tests/sasdr_ref.py against its own autograd."""
import math
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import sasdr_ref as sr                                                       # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import trainer as T                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = df.TURN_FAR
ENTRIES = ("sepr_pit_sasdr_fwd", "sepr_pit_sasdr_bwd", "sepr_pit_sasdr_mag_fwd", "sepr_pit_sasdr_mag_bwd")


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def host_corpus(golden):
    arrays, roles = dr.fixture_corpus(golden("dynmix"))
    c = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    c.set_energies(np.array([dr.energy(arrays[nm]) for nm in c.names], dtype=np.int64), np.zeros(0))
    c.roles = roles
    return c, [str(k) for k in golden("dynmix")["keys"]]


@pytest.mark.parametrize("planner", [df.plan_wsj0, df.plan_wham, df.plan_whamr])
def test_absent_zero_is_the_planner_of_before(golden, planner):
    """``absent=0`` (and the default): the plans equal those of the planner without the argument, and the generator ends in the same state."""
    corpus, keys = host_corpus(golden)
    turns = df.Turns((0.0, 0.6), 40)
    for kw in ({"turns": turns}, {}):
        r0, r1, r2 = random.Random(5), random.Random(5), random.Random(5)
        for key in keys * 3:
            a = planner(corpus, r0, key, 2000, **kw)
            b = planner(corpus, r1, key, 2000, absent=0.0, **kw)
            c = planner(corpus, r2, key, 2000, absent=0, **kw)
            assert a == b == c
        assert r0.getstate() == r1.getstate() == r2.getstate()


def covers(turns_of, n):
    """The union of the turns, clipped to [0, n), is [0, n)."""
    seen = [False] * n
    for on, off in turns_of:
        for t in range(max(on, 0), min(off, n)):
            seen[t] = True
    return all(seen)


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("rho", [0.0, 0.3, 1.0])
def test_absent_one_silences_exactly_one_talker(S, rho):
    """``absent=1.0``: one source has the empty turn ``(TURN_FAR, TURN_FAR)``, the others cover ``[0, n)`` laid out by the rule of ``S - 1``
    talkers with the same rho and their drawn order; the draws are rho, the order, the coin, the talker - in that order."""
    turns = df.Turns((rho, rho), 0)
    who_seen = set()
    for seed in range(40):
        for n in (4, 1000, 2001):
            rng, twin = random.Random(seed), random.Random(seed)
            out = df._draw_turns(rng, turns, S, n, 1.0)
            empty = [s for s, t in enumerate(out) if t == (FAR, FAR)]
            assert len(empty) == 1
            who_seen.add(empty[0])
            rest = [t for s, t in enumerate(out) if s != empty[0]]
            assert all(on < off for on, off in rest) and covers(rest, n)
            # the same draws by hand
            r = twin.uniform(rho, rho)
            order = twin.sample(range(S), S)
            coin, who = twin.random(), twin.randrange(S)
            assert coin < 1.0 and who == empty[0] and twin.getstate() == rng.getstate()
            order = [w for w in order if w != who]
            if S == 2:
                assert rest == [(-FAR, FAR)]                                     # one talker left: the open turn
            else:
                d = min(n, math.ceil(n / (2 - r)))
                h = n - d
                want = {order[0]: (-FAR, FAR if d >= n else d), order[1]: (-FAR if h <= 0 else h, FAR)}
                assert {s: t for s, t in enumerate(out) if s != who} == want
    assert who_seen == set(range(S))


def test_absent_between_zero_and_one_draws_alike_either_way():
    """0 < absent < 1: the coin and the talker are both drawn whatever the coin says; with the coin against, the turns are those of ``absent=0``."""
    turns = df.Turns((0.0, 1.0), 80)
    kept = gone = 0
    for seed in range(60):
        a, b, c = random.Random(seed), random.Random(seed), random.Random(seed)
        out = df._draw_turns(a, turns, 2, 4000, 0.5)
        plain = df._draw_turns(b, turns, 2, 4000)
        b.random(), b.randrange(2)
        assert a.getstate() == b.getstate()
        if (FAR, FAR) in out:
            gone += 1
        else:
            kept += 1
            assert out == plain
        df._draw_turns(c, turns, 2, 4000, 1.0)
        assert c.getstate() == a.getstate()
    assert kept > 10 and gone > 10


@pytest.mark.parametrize("planner", [df.plan_wsj0, df.plan_wham, df.plan_whamr])
def test_target_and_mixture_term_carry_the_empty_turn(golden, planner):
    corpus, keys = host_corpus(golden)
    rng = random.Random(2)
    for key in keys * 2:
        e = planner(corpus, rng, key, 2000, turns=df.Turns((0.0, 0.5), 40), absent=1.0)
        tt = [(t[7], t[8]) for t in e.tgt]
        assert tt.count((FAR, FAR)) == 1 and tt.count((-FAR, FAR)) == 1
        assert [(t[7], t[8]) for t in e.mix[:2]] == tt
        if len(e.mix) == 3:
            assert (e.mix[2][7], e.mix[2][8]) == (-FAR, FAR)                    # the noise keeps the open turn
    plan = df.collate_plan(corpus, [planner(corpus, rng, k, 2000, turns=df.Turns((0.0, 0.5), 40), absent=1.0) for k in keys])
    assert plan.on is not None and int((plan.on[:, plan.M:] == FAR).sum()) == len(keys)


def test_refusals():
    rng = random.Random(0)
    with pytest.raises(ValueError, match="turns"):
        df._draw_turns(rng, None, 2, 100, 0.5)
    for bad in (-0.1, 1.5, True, "0.5", None):
        with pytest.raises(ValueError, match="absent"):
            df._draw_turns(rng, df.Turns(), 2, 100, bad)
    assert rng.getstate() == random.Random(0).getstate()                     # refused before any draw
    with pytest.raises(ValueError, match="zero gradient"):
        T.check_criterion("sisnr", 0.5)
    with pytest.raises(ValueError, match="criterion"):
        T.check_criterion("snr", 0.0)
    T.check_criterion("sisnr", 0.0), T.check_criterion("sasdr", 0.0), T.check_criterion("sasdr", 1.0)
    # a checkpoint without the key was trained with the SI-SNR pair
    T.check_resume_criterion("sisnr", None), T.check_resume_criterion("sisnr", {}), T.check_resume_criterion("sasdr", {"criterion": "sasdr"})
    for now, rs in (("sasdr", None), ("sasdr", {}), ("sisnr", {"criterion": "sasdr"}), ("sasdr", {"criterion": "sisnr"})):
        with pytest.raises(ValueError, match="criterion"):
            T.check_resume_criterion(now, rs)


def test_planner_refuses_absent_without_turns(golden):
    corpus, keys = host_corpus(golden)
    for planner in (df.plan_wsj0, df.plan_wham, df.plan_whamr):
        with pytest.raises(ValueError, match="turns"):
            planner(corpus, random.Random(0), keys[0], 2000, absent=0.5)
    assert df.Turns._fields == ("overlap", "ramp")                           # the probability is the planner's argument, not a field of Turns


def test_tool_takes_the_two_options():
    src = open(os.path.join(ROOT, "tools", "train_from_scp.py")).read()
    assert '"--criterion"' in src and '"--turn-absent"' in src and "criterion=args.criterion" in src


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_four_entries():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    assert int(re.search(r"#define SEPR_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == 413
    assert "SEPR_OP_SASDR" not in hdr and len(re.findall(r"\bSEPR_OP_[A-Z]+\b", hdr.split("SEPR_OP_COUNT")[0].split("SEPR_OP_ENCODER")[-1])) == 7
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is L._i and len(sig) == len(args), (name, len(sig), len(args))
        for a, t in zip(args, sig):
            want = L._d if a.startswith("double ") else L._i if a.startswith("int ") and "*" not in a else L._sz if a.startswith("size_t ") else L._fp
            assert t is want, (name, a)
        assert "double snr_max" in args and "double eps" in args and not any("clamp_min" in a for a in args)
    # the sibling's arguments, snr_max in the place of clamp_min
    assert L.SIGNATURES["sepr_pit_sasdr_bwd"] == L.SIGNATURES["sepr_pit_sisnr_bwd"]
    i = L.SIGNATURES["sepr_pit_sisnr_mag_fwd"][1].index(L._d)
    assert L.SIGNATURES["sepr_pit_sasdr_mag_fwd"][1] == L.SIGNATURES["sepr_pit_sisnr_mag_fwd"][1][:i + 1] + [L._d] + L.SIGNATURES["sepr_pit_sisnr_mag_fwd"][1][i + 1:]
    i = L.SIGNATURES["sepr_pit_sisnr_mag_bwd"][1].index(L._d)
    assert L.SIGNATURES["sepr_pit_sasdr_mag_bwd"][1] == L.SIGNATURES["sepr_pit_sisnr_mag_bwd"][1][:i + 1] + [L._d] + L.SIGNATURES["sepr_pit_sisnr_mag_bwd"][1][i + 1:]
    lib = L.load()
    assert lib.sepr_version() == 413
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # every refusal comes before any HIP call: null pointers, S out of range
    assert lib.sepr_pit_sasdr_fwd(None, None, 2, 1, 16, 1e-8, 30.0, None, None, None, 0, None) == L.SEPR_EINVAL
    assert lib.sepr_pit_sasdr_bwd(None, None, None, None, 2, 1, 16, 1e-8, 30.0, None, None, 0, None) == L.SEPR_EINVAL
    assert lib.sepr_pit_sasdr_mag_fwd(None, None, 2, 1, 1024, None, 512, 128, 1e-12, 30.0, None, None, None, 0, None) == L.SEPR_EINVAL
    assert lib.sepr_pit_sasdr_mag_bwd(None, None, None, None, 2, 1, 1024, None, None, 512, 128, 1e-12, 30.0, None, None, 0, None) == L.SEPR_EINVAL


def test_public_surface():
    from sepreformer_amd import criterion as C
    for name in ("pit_sasdr", "pit_sasdr_mag", "PIT_SASDR_time", "PIT_SASDR_mag", "_SaSdrTimeFn", "_SaSdrMagFn"):
        assert hasattr(C, name), name
    t = C.PIT_SASDR_time("cpu", 2)
    m = C.PIT_SASDR_mag("cpu", 512, 128, "hann", 4, 2)
    assert t.snr_max == m.snr_max == 30.0 and m.num_stages == 4 and "snr_max=30.0" in repr(t) and "snr_max=30.0" in repr(m)
    with pytest.raises(RuntimeError, match="HIP device"):
        t(estims=[torch.zeros(1, 8)] * 2, target_attr=[torch.zeros(1, 8)] * 2, input_sizes=torch.tensor([8]))


# ---- the restatement against its own autograd --------------------------------------------------------------------------------------------
def draw(S, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    tgt = 0.1 * torch.randn(S, B, T, generator=g, dtype=torch.float64) + 0.05
    est = tgt[[(s + 1) % S for s in range(S)]] + 0.03 * torch.randn(S, B, T, generator=g, dtype=torch.float64) - 0.02
    tgt[0, 0] = 0.0                                                            # one silent target
    if B > 1:
        tgt[:, 1] = 0.0                                                        # every target silent
    return est, tgt


def rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("S", [1, 2, 3])
def test_time_gradient_formula_is_autograd(S):
    est, tgt = draw(S, 3, 700, 10 + S)
    gl = torch.linspace(0.5, 2.0, 3, dtype=torch.float64)
    loss, perm, allE, grad = sr.autograd(sr.sasdr_time, est, tgt, gl)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    assert rel(sr.grad_time(est, tgt, gl), grad) < 1e-12
    if S > 1:
        assert perm[2].tolist() == [(s + 1) % S for s in range(S)]
    # every target silent: 10 log10((E + eps) / eps), finite
    e = sr.zero_mean(est)[:, 1]
    E = min(float(sum((e[s] ** 2).sum() for s in range(S))), float(allE[:, 1].min()))
    assert abs(float(loss[1]) - 10 * math.log10((E + 1e-8) / 1e-8)) < 1e-9


@pytest.mark.parametrize("S", [1, 2, 3])
def test_mag_gradient_formula_is_autograd(S):
    """d loss / d M by the closed form equals autograd with respect to the magnitudes; the chain behind it (re / M, the STFT adjoint, overlap-add,
    de-mean) is autograd's own."""
    est, tgt = draw(S, 3, 1100, 20 + S)
    gl = torch.linspace(0.5, 2.0, 3, dtype=torch.float64)
    K = sr.stft_kernel64(512, 128)
    Me = sr.stft_mag(sr.zero_mean(est), K, 128).requires_grad_(True)
    Mt = sr.stft_mag(sr.zero_mean(tgt), K, 128)
    D = (Mt * Mt).sum((0, 2, 3))
    E, perm, _ = sr.walk(sr.pair_energy(Me, Mt))
    loss = sr.value(E, D, sr.EPS_MAG)
    (loss * gl).sum().backward()
    assert torch.isfinite(loss).all() and rel(sr.grad_mag_wrt_M(Me.detach(), Mt, gl), Me.grad) < 1e-12
    l2, p2, _, g2 = sr.autograd(sr.sasdr_mag, est, tgt, gl)
    assert torch.equal(p2, perm) and torch.allclose(l2, loss.detach(), rtol=0, atol=1e-12) and torch.isfinite(g2).all()
    assert float(g2.sum(-1).abs().max()) < 1e-9 * float(g2.abs().max()) * est.shape[-1]       # behind the de-mean: every row sums to 0


def test_kernel_is_the_criterions_kernel():
    from sepreformer_amd.criterion import stft_kernel
    for N, hop in ((512, 128), (512, 256), (256, 64)):
        assert torch.allclose(sr.stft_kernel64(N, hop).float(), stft_kernel(N, hop)[:N + 2], rtol=0, atol=1e-7)


def test_silent_channel_behaves():
    """What the criterion is for (the setup of DESIGN.md section 5e-7): target 1 silent, estimate 1 noise at a falling scale - the loss stays
    finite and falls, and the gradient on the silent channel goes to zero with the estimate, in both forms; exactly 0 for a silent estimate."""
    g = torch.Generator().manual_seed(0)
    S, B, Tn = 2, 2, 8000
    tgt = torch.zeros(S, B, Tn, dtype=torch.float64)
    tgt[0] = 0.1 * torch.randn(B, Tn, generator=g, dtype=torch.float64)
    nz = torch.randn(B, Tn, generator=g, dtype=torch.float64)
    e0 = tgt[0] + 0.01 * torch.randn(B, Tn, generator=g, dtype=torch.float64)
    gl = torch.full((B,), 1.0 / B, dtype=torch.float64)
    for fn in (sr.sasdr_time, sr.sasdr_mag):
        norms, losses = [], []
        for scale in (1e-1, 1e-3, 1e-5, 0.0):
            est = torch.stack([e0, scale * nz])
            loss, perm, _, grad = sr.autograd(fn, est, tgt, gl)
            assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and perm.tolist() == [[0, 1]] * B
            norms.append(float(grad[1].norm()))
            losses.append(float(loss.mean()))
        print(fn.__name__, "loss", losses, "silent-channel gradient norm", norms)
        assert norms[3] == 0.0 and norms[2] < 0.05 and norms[2] < norms[1] and max(norms) < 10.0
        assert losses[0] > losses[1] >= losses[2] >= losses[3] and losses[3] < -15.0
