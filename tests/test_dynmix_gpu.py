"""Dynamic mixing on the device: ``sepr_corpus_energy`` and ``sepr_dynmix_fwd`` against the numpy restatement
(tests/dynmix_ref.py, bit for bit) and against the reference's recorded outputs (tests/golden/dynmix.npz), through ``DynamicMixFeed``,
under graph capture, and feeding a ``CapturedTrainStep``."""
import dataclasses
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_one_field as one                                               # noqa: E402
import dynmix_ref as ref                                                     # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANNERS = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr, "direct": df.plan_direct}


def fixture_corpus(g, as_float=False):
    arrays, roles = ref.fixture_corpus(g)
    if as_float:
        arrays = {k: ref.values(v) for k, v in arrays.items()}
    c = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    c.roles = roles
    return c, [arrays[nm] for nm in c.names]


def ref_batch(utts, plan, T):
    mix, src = ref.mix_batch(utts, plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.M, plan.S, T)
    return torch.from_numpy(mix), torch.from_numpy(src)


def test_corpus_energy_int16_and_float32():
    """int16: equal to the integer sums, utterances of 1 sample, of odd length and one longer than a workgroup's span (8 x 256 samples
    per pass) included.  float32: within 1e-12 relative of a float64 numpy sum."""
    rng = np.random.default_rng(3)
    lens = [1, 2, 7, 255, 256, 257, 2049, 4097, 40001, 1]
    a16 = {f"i{i}": rng.integers(-32768, 32768, size=n, dtype=np.int16) for i, n in enumerate(lens)}
    a16["i0"][:] = -32768
    a32 = {f"f{i}": rng.uniform(-1, 1, size=n).astype(np.float32) for i, n in enumerate(lens)}
    c = df.Corpus.from_arrays({**a16, **a32}, device=DEV)
    assert c.n16 == len(lens) and c.names[:len(lens)] == list(a16)
    want = torch.tensor([ref.energy(x) for x in a16.values()], dtype=torch.int64)
    assert torch.equal(torch.from_numpy(c.ss16), want)
    w32 = np.array([ref.energy(x) for x in a32.values()])
    assert np.all(np.abs(c.ss32 - w32) <= 1e-12 * w32), (c.ss32, w32)
    assert c.rms.dtype == np.float32 and all(c.rms[i] == ref.rms(x) for i, x in enumerate(a16.values()))
    only32 = df.Corpus.from_arrays(a32, device=DEV)                          # no int16 buffer at all
    assert np.array_equal(only32.ss32, c.ss32)


def random_plan(rng, corpus, B, M, S, Tmax, force_full=True):
    """A random table: starts of every alignment, n from 4 to Tmax (one example with n == Tmax), some target terms equal to their
    mixture terms and some not."""
    NT = M + S
    n = np.sort(rng.integers(1, Tmax // 4 + 1, size=B) * 4)[::-1].astype(np.int32)
    if force_full:
        n[0] = Tmax
    n[-1] = 4 if B > 1 else n[-1]
    utt, start = np.zeros((B, NT), np.int32), np.zeros((B, NT), np.int32)
    norm = rng.uniform(0.3, 3.0, size=(B, NT)).astype(np.float32)
    gain = rng.uniform(0.5, 1.8, size=(B, NT)).astype(np.float32)
    ok = [u for u in range(len(corpus)) if corpus.lengths[u] >= Tmax]
    for b in range(B):
        for j in range(NT):
            u = int(rng.choice(ok))
            utt[b, j], start[b, j] = u, int(rng.integers(0, corpus.lengths[u] - n[b] + 1))
        if b % 2 == 0:                                                       # targets ARE the first S mixture terms (WSJ0 / WHAM form)
            for s in range(S):
                for arr in (utt, start, norm, gain):
                    arr[b, M + s] = arr[b, s]
    return df.BatchPlan([str(b) for b in range(B)], n, utt, start, norm, gain, M, S)


@pytest.mark.parametrize("fmt", ["int16", "float32", "both"])
def test_dynmix_random_plans_bit_equal(fmt):
    """S = 2 and 3, M = S and S + 1, B = 1 and 32, starts of every alignment modulo 8, n from 4 to Tmax: mix and src equal the
    restatement bit for bit, the zero padding included; a guard region around the outputs is untouched."""
    rng = np.random.default_rng(7)
    arrays = {}
    for i in range(12):
        n = 700 + 131 * i
        x = rng.integers(-20000, 20000, size=n, dtype=np.int16)
        use16 = fmt == "int16" or (fmt == "both" and i % 2 == 0)
        arrays[f"u{i}"] = x if use16 else (rng.normal(0, 0.1, size=n)).astype(np.float32)
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    utts = [arrays[nm] for nm in corpus.names]
    seen = set()
    for S in (2, 3):
        for M in (S, S + 1):
            for B, Tmax in ((1, 604), (32, 512), (3, 8), (2, 4)):
                plan = random_plan(rng, corpus, B, M, S, Tmax)
                if B == 32:                                                  # every alignment modulo 8 of the first term's start
                    for b in range(8):
                        u = plan.utt[b, 0]
                        plan.start[b, 0] = min((int(plan.start[b, 0]) & ~7) + b, int(corpus.lengths[u]) - int(plan.n[b]))
                        if b % 2 == 0:
                            plan.start[b, M] = plan.start[b, 0]
                seen |= {int(s) % 8 for s in plan.start.ravel()}
                G = 64
                block = torch.full(((S + 1) * B * Tmax + 2 * G,), 123.0, device=DEV)
                body = block[G:G + (S + 1) * B * Tmax].view(S + 1, B, Tmax)
                mix, src = df.mix_batch(corpus, plan, Tmax, mix=body[0], src=[body[1 + s] for s in range(S)])
                torch.cuda.synchronize()
                wm, ws = ref_batch(utts, plan, Tmax)
                assert torch.equal(mix.cpu(), wm), (fmt, S, M, B)
                assert torch.equal(torch.stack(src).cpu(), ws), (fmt, S, M, B)
                assert bool((block[:G] == 123.0).all()) and bool((block[-G:] == 123.0).all())
    assert seen == set(range(8))


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr", "direct"])
def test_feed_against_reference_and_restatement(golden, tag):
    """End to end through DynamicMixFeed on the fixture's corpus, seeds and key order: bit-equal to the restatement; against the
    reference's recorded batch the CPU test's split - >= 120 dB everywhere (the RMS is the one permitted difference: exact integer sum
    against numpy's pairwise float32 sum, a few ulp, about -128 dB), bit-equal for ``_direct_load`` and for terms of norm factor 1."""
    g = golden("dynmix")
    corpus, utts = fixture_corpus(g)
    keys = [str(k) for k in g["keys"]]
    feed = df.DynamicMixFeed(corpus, PLANNERS[tag], batch=len(keys), max_len=int(g["max_len"]), seed=int(g[f"{tag}.seed"]), keys=keys)
    batches = list(feed)
    assert len(batches) == 1
    sizes, mix, src, key = batches[0]
    plan = feed.last_plan
    want_mix, want_src = torch.from_numpy(g[f"{tag}.mixture"]), torch.from_numpy(g[f"{tag}.src"])
    assert key == [str(k) for k in g[f"{tag}.keys_out"]]
    assert sizes.dtype == torch.float32 and torch.equal(sizes, torch.from_numpy(g[f"{tag}.input_sizes"]))
    assert mix.shape == want_mix.shape and len(src) == want_src.shape[0]
    wm, ws = ref_batch(utts, plan, mix.shape[1])
    got_src = torch.stack(src).cpu()
    assert torch.equal(mix.cpu(), wm) and torch.equal(got_src, ws)
    for b in range(len(keys)):
        db = [ref.agreement_db(mix[b].cpu(), want_mix[b])] + [ref.agreement_db(got_src[s, b], want_src[s, b]) for s in range(plan.S)]
        print(f"{tag} example {b}: agreement {['%.1f' % d for d in db]} dB")
        assert min(db) >= 120.0, (tag, b, db)
        for s in range(plan.S):
            if tag == "direct" or plan.norm[b, plan.M + s] == np.float32(1.0):
                assert torch.equal(got_src[s, b], want_src[s, b]), (tag, b, s)
        if tag == "direct":
            assert torch.equal(mix[b].cpu(), want_mix[b])


def test_float32_corpus_follows_int16(golden):
    """The same audio stored as float32, the same seeds: the same draws, and >= 120 dB against the int16 run (the float64 energy sum
    against the integer one moves the RMS by an ulp at most)."""
    g = golden("dynmix")
    keys = [str(k) for k in g["keys"]]
    out = []
    for as_float in (False, True):
        corpus, _ = fixture_corpus(g, as_float)
        assert corpus.n16 == (0 if as_float else len(corpus))
        feed = df.DynamicMixFeed(corpus, df.plan_whamr, batch=4, max_len=int(g["max_len"]), seed=5, keys=keys)
        (_, mix, src, key), = list(feed)
        out.append((mix.cpu(), torch.stack(src).cpu(), key, feed.last_plan))
    assert out[0][2] == out[1][2] and np.array_equal(out[0][3].start, out[1][3].start)
    assert ref.agreement_db(out[1][0], out[0][0]) >= 120.0 and ref.agreement_db(out[1][1], out[0][1]) >= 120.0


def test_determinism_and_independence(golden):
    g = golden("dynmix")
    corpus, utts = fixture_corpus(g)

    def run(batch):
        feed = df.DynamicMixFeed(corpus, df.plan_wham, batch=batch, max_len=2000, seed=9, fixed_length=True)
        return [(m.cpu(), torch.stack(s).cpu(), k, feed.last_plan) for _, m, s, k in feed]

    a, b = run(2), run(2)
    assert len(a) == 2 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b))
    assert all(x[0].shape == (2, 2000) for x in a)
    # an example's rows do not depend on its neighbours: the same table rows in batches of other sizes and positions
    plan = a[0][3]
    for order in ([1, 0], [0], [1, 1, 0, 1]):
        sub = df.BatchPlan([plan.keys[i] for i in order], plan.n[order], plan.utt[order], plan.start[order], plan.norm[order],
                           plan.gain[order], plan.M, plan.S)
        mix, src = df.mix_batch(corpus, sub, 2000)
        for pos, i in enumerate(order):
            assert torch.equal(mix[pos].cpu(), a[0][0][i]) and torch.equal(torch.stack(src)[:, pos].cpu(), a[0][1][:, i])


def test_capture_replays_with_an_updated_table(golden):
    """The launch inside a torch.cuda.graph, the plan table rewritten between replays: every replay equals the eager batch."""
    g = golden("dynmix")
    corpus, _ = fixture_corpus(g)
    rng = random.Random(21)
    keys = [str(k) for k in g["keys"]]
    plans = [df.collate_plan(corpus, [df.plan_whamr(corpus, rng, k, 2400) for k in keys]) for _ in range(3)]
    B, T, S = 4, 2400, 2
    table = torch.from_numpy(df.pack_table(plans[0])).to(DEV)
    mix = torch.zeros(B, T, device=DEV)
    src = [torch.zeros(B, T, device=DEV) for _ in range(S)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.mix_batch(corpus, plans[0], T, mix, src, table=table)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        df.mix_batch(corpus, plans[0], T, mix, src, table=table)
    for plan in plans[1:] + plans[:1]:
        table.copy_(torch.from_numpy(df.pack_table(plan)))
        graph.replay()
        torch.cuda.synchronize()
        em, es = df.mix_batch(corpus, plan, T)
        assert torch.equal(mix, em) and all(torch.equal(a, b) for a, b in zip(src, es))


def test_captured_train_step_fed_by_the_feed(golden):
    """A tiny-width CapturedTrainStep fed by DynamicMixFeed(fixed_length=True) through next_into: the loss is finite and moves, and
    every batch the step consumed equals the restatement's."""
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    g = golden("dynmix")
    corpus, utts = fixture_corpus(g)
    B, T = 2, 2000
    feed = df.DynamicMixFeed(corpus, df.plan_wsj0, batch=B, max_len=T, seed=3, fixed_length=True)
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
    losses = []
    for _ in range(5):
        plan = feed.next_into(step.x, step.targets)
        loss, _ = step(step.x, step.targets)
        losses.append(float(loss.detach()))
        wm, ws = ref_batch(utts, plan, T)
        assert torch.equal(step.x.cpu(), wm) and torch.equal(torch.stack(step.targets).cpu(), ws)
    step.release()
    print("losses", losses)
    assert all(np.isfinite(v) for v in losses) and len(set(losses)) > 1


def test_a_target_that_differs_in_one_field_is_recomputed():
    """B = 4: utt, start, norm bits, gain bits.  The two utterances of a pair differ in content and both hold start + n."""
    rng = np.random.default_rng(23)
    arrays = {"a16": rng.integers(-20000, 20000, size=2600, dtype=np.int16), "b16": rng.integers(-20000, 20000, size=2600, dtype=np.int16),
              "a32": rng.normal(0, 0.1, size=2700).astype(np.float32), "b32": rng.normal(0, 0.1, size=2700).astype(np.float32)}
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    utts, i = [arrays[nm] for nm in corpus.names], corpus.index
    same, changed = one.plans(df, {"utt": (i["a16"], i["a32"]), "start": (3, 40), "norm": (0.75, 1.5), "gain": (1.25, 0.5)},
                              {"utt": (i["b16"], i["b32"]), "start": (4, 47), "norm": (0.8, 1.4), "gain": (1.3, 0.6)})
    assert len(changed.n) == 4
    one.check(lambda p: df.mix_batch(corpus, p, one.TMAX), lambda p: ref_batch(utts, p, one.TMAX), same, changed)
