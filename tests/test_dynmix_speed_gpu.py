"""Speed perturbation inside the mixing launch: ``sepr_dynmix_speed_fwd`` against the numpy restatement
(tests/dynmix_speed_ref.py, bit for bit), against the composition of the two existing entry points (``resample.resample`` of whole
utterances, then the plain ``sepr_dynmix_fwd``), against the plain launch for unperturbed plans, under graph capture, through
``DynamicMixFeed`` and feeding a ``CapturedTrainStep``."""
import dataclasses
import functools
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_one_field as one                                               # noqa: E402
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_speed_ref as ref                                               # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEEDS = list(range(95, 106))
CONVERTERS = [p for p in SPEEDS if p != 100]                                 # a fixed converter set: index k = CONVERTERS[k]


def synthetic_corpus(fmt):
    """Twelve utterances of 700 + 131 i samples, alternately QUIET and LOUD in storage order (a read across an utterance boundary
    shows), one of 40 samples - shorter than Hh, the whole filter overhangs both ends - and two long ones (more than two output tiles
    of 2048).  ``fmt``: int16, float32, or both."""
    rng = np.random.default_rng(7)
    arrays = {}

    def add(name, n, use16, loud):
        if use16:
            a = 30000 if loud else 300
            arrays[name] = rng.integers(-a, a, size=n, dtype=np.int16)
        else:
            arrays[name] = rng.normal(0, 0.3 if loud else 0.003, size=n).astype(np.float32)

    for i in range(12):
        add(f"u{i}", 700 + 131 * i, fmt == "int16" or (fmt == "both" and i % 4 < 2), i % 2 == 1)
        if i == 5:
            add("short", 40, fmt != "float32", False)                        # between the loud u5 and the next utterance of its group
    add("long0", 4500, fmt != "float32", True)
    add("long1", 4700, fmt == "int16", False)
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    return corpus, [arrays[nm] for nm in corpus.names]


def speed_plan(rng, corpus, B, M, S, Tmax, cycle, short_first=False):
    """A random table with a speed per term (``cycle`` runs through 95..105, 100 = unperturbed, included): n from 4 to Tmax (one example
    with n == Tmax), starts of every alignment, terms starting at 0 and terms ending exactly at the perturbed length, some target terms
    equal to their mixture terms (speed included) and some not."""
    NT = M + S
    n = np.sort(rng.integers(1, Tmax // 4 + 1, size=B) * 4)[::-1].astype(np.int32)
    n[0] = Tmax
    if B > 1:
        n[-1] = 4
    utt, start = np.zeros((B, NT), np.int32), np.zeros((B, NT), np.int32)
    speed = np.zeros((B, NT), np.int32)
    norm = rng.uniform(0.3, 3.0, size=(B, NT)).astype(np.float32)
    gain = rng.uniform(0.5, 1.8, size=(B, NT)).astype(np.float32)
    plen = lambda u, p: ref.perturbed_len(int(corpus.lengths[u]), p)         # noqa: E731
    for b in range(B):
        for j in range(NT):
            p = next(cycle)
            if short_first and b == 0:
                u = corpus.index["short"]
            else:
                u = int(rng.choice([u for u in range(len(corpus)) if plen(u, p) >= n[b]]))
            s = int(rng.integers(0, plen(u, p) - n[b] + 1))
            if j == 0 and b < 8:                                             # every alignment modulo 8
                s = min((s & ~7) + b, plen(u, p) - int(n[b]))
            if j == 1 and b % 3 == 0:
                s = 0
            if j == 1 and b % 3 == 1:
                s = plen(u, p) - int(n[b])                                   # ends exactly at the perturbed length N
            utt[b, j], start[b, j], speed[b, j] = u, s, p
        if b % 2 == 0:                                                       # targets ARE the first S mixture terms (WSJ0 / WHAM form)
            for s in range(S):
                for arr in (utt, start, norm, gain, speed):
                    arr[b, M + s] = arr[b, s]
    return df.BatchPlan([str(b) for b in range(B)], n, utt, start, norm, gain, M, S, speed)


def ref_batch(utts, plan, T):
    speed = plan.speed if plan.speed is not None else np.full_like(plan.utt, 100)
    mix, src = ref.mix_batch(utts, plan.n, plan.utt, plan.start, plan.norm, plan.gain, speed, plan.M, plan.S, T)
    return torch.from_numpy(mix), torch.from_numpy(src)


def fixture_corpus(g):
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    c.roles = roles
    return c, [arrays[nm] for nm in c.names]


@pytest.mark.parametrize("fmt", ["int16", "float32", "both"])
def test_speed_plans_bit_equal(fmt):
    """S = 2 and 3, M = S and S + 1, B = 1 and 32, Tmax of two output tiles plus a remainder, of one plus a remainder and below one, the
    40-sample utterance (n = 36), every speed of 95..105, perturbed and unperturbed terms inside one example, starts of every alignment
    modulo 8, a start of 0 and an end exactly at the perturbed length: mix and src equal the restatement bit for bit, the zero padding
    included; a guard region around the outputs is untouched."""
    corpus, utts = synthetic_corpus(fmt)
    assert corpus.n16 == {"int16": 15, "float32": 0, "both": 8}[fmt]
    rng = np.random.default_rng(11)
    cycle = itertools.cycle([95, 100, 105, 96, 104, 97, 103, 98, 102, 99, 101, 100, 95, 105])
    seen_align, seen_speed, mixed, at_zero, at_end = set(), set(), 0, 0, 0
    for S in (2, 3):
        for M in (S, S + 1):
            for B, Tmax in ((1, 4284), (2, 2252), (32, 664), (3, 36), (2, 4)):
                plan = speed_plan(rng, corpus, B, M, S, Tmax, cycle, short_first=Tmax == 36)
                seen_align |= {int(s) % 8 for s in plan.start.ravel()}
                seen_speed |= {int(p) for p in plan.speed.ravel()}
                mixed += sum(1 for row in plan.speed if 100 in row and (row != 100).any())
                for b in range(B):
                    for j in range(M + S):
                        p, u = int(plan.speed[b, j]), int(plan.utt[b, j])
                        if p != 100:
                            at_zero += plan.start[b, j] == 0
                            at_end += plan.start[b, j] + plan.n[b] == ref.perturbed_len(int(corpus.lengths[u]), p)
                G = 64
                block = torch.full(((S + 1) * B * Tmax + 2 * G,), 123.0, device=DEV)
                body = block[G:G + (S + 1) * B * Tmax].view(S + 1, B, Tmax)
                mix, src = df.mix_batch(corpus, plan, Tmax, mix=body[0], src=[body[1 + s] for s in range(S)])
                torch.cuda.synchronize()
                wm, ws = ref_batch(utts, plan, Tmax)
                assert torch.equal(mix.cpu(), wm), (fmt, S, M, B, Tmax)
                assert torch.equal(torch.stack(src).cpu(), ws), (fmt, S, M, B, Tmax)
                assert bool((block[:G] == 123.0).all()) and bool((block[-G:] == 123.0).all())
    assert seen_align == set(range(8)) and seen_speed == set(SPEEDS)
    assert mixed > 0 and at_zero > 0 and at_end > 0


def test_equals_whole_utterance_conversion_then_plain_mix():
    """The composition of the two existing entry points: every utterance converted whole by ``resample.resample`` at every speed a term
    uses, a float32 corpus of the results, the plain ``sepr_dynmix_fwd`` with the same starts, norms and gains - the same bits."""
    corpus, utts = synthetic_corpus("both")
    rng = np.random.default_rng(3)
    plan = speed_plan(rng, corpus, 8, 3, 2, 664, itertools.cycle(SPEEDS))
    mix, src = df.mix_batch(corpus, plan, 664)
    pairs = sorted({(int(u), int(p)) for u, p in zip(plan.utt.ravel(), plan.speed.ravel())})
    converted = {}
    for p in sorted({p for _, p in pairs}):
        us = [u for u, q in pairs if q == p]
        xs = [torch.from_numpy(dr.values(utts[u])) for u in us]
        ys = xs if p == 100 else rs.resample(xs, p, 100, device=DEV)
        for u, y in zip(us, ys):
            converted[(u, p)] = y.cpu().numpy()
            assert y.shape[0] == ref.perturbed_len(utts[u].shape[0], p)
    whole = df.Corpus.from_arrays({f"{u}@{p}": converted[(u, p)] for u, p in pairs}, device=DEV)
    where = np.array([[whole.index[f"{u}@{p}"] for u, p in zip(ru, rp)] for ru, rp in zip(plan.utt, plan.speed)], np.int32)
    wm, ws = df.mix_batch(whole, plan._replace(utt=where, speed=None), 664)
    assert torch.equal(mix, wm) and all(torch.equal(a, b) for a, b in zip(src, ws))


def test_unperturbed_plan_gives_the_plain_launch():
    """Converter indices all -1 (with no converter at all, and with ten converters passed along): the bits of ``sepr_dynmix_fwd``."""
    corpus, _ = synthetic_corpus("both")
    rng = np.random.default_rng(5)
    for S, M, B, Tmax in ((2, 2, 5, 2252), (3, 4, 32, 664), (2, 3, 1, 4284)):
        plan = speed_plan(rng, corpus, B, M, S, Tmax, itertools.cycle([100]))
        assert (df.pack_table(plan)[-B * (M + S):] == -1).all()
        pm, ps = df.mix_batch(corpus, plan._replace(speed=None), Tmax)
        for conv in (None, CONVERTERS):
            mix, src = df.mix_batch(corpus, plan, Tmax, speeds=conv)
            assert torch.equal(mix, pm) and all(torch.equal(a, b) for a, b in zip(src, ps)), (S, M, B, conv)


def test_determinism_and_independence():
    corpus, _ = synthetic_corpus("both")
    plan = speed_plan(np.random.default_rng(9), corpus, 6, 3, 2, 2252, itertools.cycle(SPEEDS))
    a = df.mix_batch(corpus, plan, 2252, speeds=CONVERTERS)
    b = df.mix_batch(corpus, plan, 2252, speeds=CONVERTERS)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    # an example's rows do not depend on its neighbours, nor on the converter set's order
    for order, conv in (([5, 0, 3], CONVERTERS[::-1]), ([2], None), ([1, 1, 4, 0, 1, 2, 3, 5, 5], CONVERTERS)):
        sub = df.BatchPlan([plan.keys[i] for i in order], plan.n[order], plan.utt[order], plan.start[order], plan.norm[order],
                           plan.gain[order], plan.M, plan.S, plan.speed[order])
        mix, src = df.mix_batch(corpus, sub, 2252, speeds=conv)
        for pos, i in enumerate(order):
            assert torch.equal(mix[pos], a[0][i]) and all(torch.equal(src[s][pos], a[1][s][i]) for s in range(plan.S))


def test_capture_replays_with_an_updated_table(golden):
    """The launch inside a torch.cuda.graph with a fixed converter set, the plan table - index block included - rewritten between
    replays: every replay equals the eager batch."""
    g = golden("dynmix")
    corpus, _ = fixture_corpus(g)
    rng = random.Random(21)
    keys = [str(k) for k in g["keys"]]
    plans = [df.collate_plan(corpus, [df.plan_whamr(corpus, rng, k, 2400, speeds=SPEEDS) for k in keys]) for _ in range(3)]
    assert len({tuple(df.pack_table(p, CONVERTERS)[-len(keys) * 5:]) for p in plans}) == 3          # the index block really changes
    B, T, S = 4, 2400, 2
    table = torch.from_numpy(df.pack_table(plans[0], CONVERTERS)).to(DEV)
    mix = torch.zeros(B, T, device=DEV)
    src = [torch.zeros(B, T, device=DEV) for _ in range(S)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.mix_batch(corpus, plans[0], T, mix, src, table=table, speeds=CONVERTERS)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        df.mix_batch(corpus, plans[0], T, mix, src, table=table, speeds=CONVERTERS)
    for plan in plans[1:] + plans[:1]:
        table.copy_(torch.from_numpy(df.pack_table(plan, CONVERTERS)))
        graph.replay()
        torch.cuda.synchronize()
        em, es = df.mix_batch(corpus, plan, T)
        assert torch.equal(mix, em) and all(torch.equal(a, b) for a, b in zip(src, es))


@pytest.mark.parametrize("tag", ["wsj0", "whamr"])
def test_through_the_feed(golden, tag):
    """``DynamicMixFeed`` with ``functools.partial(plan_*, speeds=range(95, 106))`` on the fixture's corpus: every batch equals the
    restatement bit for bit; seed 1 and four epochs of one batch make all eleven speeds occur (found on the host, asserted here)."""
    g = golden("dynmix")
    corpus, utts = fixture_corpus(g)
    planner = functools.partial({"wsj0": df.plan_wsj0, "whamr": df.plan_whamr}[tag], speeds=range(95, 106))
    feed = df.DynamicMixFeed(corpus, planner, batch=4, max_len=2000, seed=1)
    seen = set()
    for _ in range(4):
        batches = list(feed)
        assert len(batches) == 1
        sizes, mix, src, key = batches[0]
        plan = feed.last_plan
        assert plan.speed is not None and torch.equal(sizes, torch.from_numpy(plan.n.astype(np.float32)))
        seen |= {int(p) for p in plan.speed[:, plan.M:].ravel()}
        if tag == "whamr":
            assert np.array_equal(plan.speed[:, :2], plan.speed[:, 3:]) and (plan.speed[:, 2] == 100).all()
        wm, ws = ref_batch(utts, plan, mix.shape[1])
        assert torch.equal(mix.cpu(), wm) and torch.equal(torch.stack(src).cpu(), ws)
    assert seen == set(SPEEDS)


def test_captured_train_step_fed_with_speeds(golden):
    """A tiny-width CapturedTrainStep fed by DynamicMixFeed(fixed_length=True) with speeds through next_into: the loss is finite and
    moves, and every batch the step consumed equals the restatement's."""
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    g = golden("dynmix")
    corpus, utts = fixture_corpus(g)
    B, T = 2, 2000
    feed = df.DynamicMixFeed(corpus, functools.partial(df.plan_wsj0, speeds=range(95, 106)), batch=B, max_len=T, seed=3, fixed_length=True)
    cfg = dataclasses.replace(VARIANTS["tiny"], dropout=0.0)
    m = Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(DEV).train()
    crit = PIT_SISNR_time(torch.device(DEV), 2, True)
    opt = FlatAdamW(m, lr=1.0e-3, weight_decay=1.0e-2)
    sizes = torch.full((B,), T)

    def loss_fn(audio, aux, *tg):
        return crit(estims=audio, input_sizes=sizes, target_attr=list(tg))

    x = torch.zeros(B, T, device=DEV)
    tg = [torch.zeros(B, T, device=DEV) for _ in range(2)]
    first = feed.next_into(x, tg)
    step = CapturedTrainStep(m, loss_fn, opt, x, tg, max_norm=5.0, warmup=1)
    wm, ws = ref_batch(utts, first, T)
    assert torch.equal(step.x.cpu(), wm) and torch.equal(torch.stack(step.targets).cpu(), ws)
    losses, perturbed = [], 0
    for _ in range(5):
        plan = feed.next_into(step.x, step.targets)
        loss, _ = step(step.x, step.targets)
        losses.append(float(loss.detach()))
        perturbed += int((plan.speed != 100).sum())
        wm, ws = ref_batch(utts, plan, T)
        assert torch.equal(step.x.cpu(), wm) and torch.equal(torch.stack(step.targets).cpu(), ws)
    step.release()
    print("losses", losses)
    assert perturbed > 0 and all(np.isfinite(v) for v in losses) and len(set(losses)) > 1


def test_a_target_that_differs_in_one_field_is_recomputed():
    """B = 5: utt, start, norm bits, gain bits, conv.  Every term goes through a converter, and the example that changes the speed alone
    pairs a converter with another converter; the two utterances of a pair differ in content and both hold start + n at every speed."""
    rng = np.random.default_rng(23)
    arrays = {"a16": rng.integers(-20000, 20000, size=2600, dtype=np.int16), "b16": rng.integers(-20000, 20000, size=2600, dtype=np.int16),
              "a32": rng.normal(0, 0.1, size=2700).astype(np.float32), "b32": rng.normal(0, 0.1, size=2700).astype(np.float32)}
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    utts, i = [arrays[nm] for nm in corpus.names], corpus.index
    assert ref.perturbed_len(2600, 105) >= 47 + one.TMAX
    same, changed = one.plans(df, {"utt": (i["a16"], i["a32"]), "start": (3, 40), "norm": (0.75, 1.5), "gain": (1.25, 0.5), "speed": (95, 104)},
                              {"utt": (i["b16"], i["b32"]), "start": (4, 47), "norm": (0.8, 1.4), "gain": (1.3, 0.6), "speed": (105, 96)})
    assert len(changed.n) == 5 and 100 not in changed.speed
    one.check(lambda p: df.mix_batch(corpus, p, one.TMAX), lambda p: ref_batch(utts, p, one.TMAX), same, changed)
