"""Speed perturbation and then reverberation of a source inside one mixing launch:
``sepr_dynmix_speed_reverb_fwd`` against the numpy restatement (tests/dynmix_speed_reverb_ref.py, bit for bit), against the composition of
the existing entries (``resample.resample`` of whole utterances, then ``sepr_dynmix_reverb_fwd``), against the reverberant and the speed
launch for plans that use one of the two only, run to run and row by row, under graph capture and through ``DynamicMixFeed``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_one_field as one                                               # noqa: E402
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_speed_ref as sr                                                # noqa: E402
import dynmix_speed_reverb_ref as ref                                        # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TMAX = 4100                                                                  # a multiple of 4, not of 8: tiles of 2048, 2048 and 4
NS = [4100, 4096, 2052, 2048, 2044, 4]
RIR_LENGTHS = [1, 2, 1023, 1024, 1025, 2500, 3073]                           # both sides of the 1024-tap chunk boundary, 1 to 4 chunks
R2500 = RIR_LENGTHS.index(2500)
SPEEDS = [90, 95, 100, 105, 110]
CONVERTERS = [p for p in SPEEDS if p != 100]                                 # a fixed converter set: index k = CONVERTERS[k]


def synthetic_corpus(fmt):
    """Six utterances of 5000, 4101, 2600 (int16) and 4999, 3000, 37 (float32) samples - ``fmt`` "int16" / "float32" stores all six in
    that format - with large values, so a read into a neighbour is not a read of zeros."""
    rng = np.random.default_rng(7)
    arrays = {}
    for i, (n, is16) in enumerate(((5000, True), (4101, True), (2600, True), (4999, False), (3000, False), (37, False))):
        if fmt == "int16" or (fmt == "both" and is16):
            arrays[f"u{i}"] = rng.integers(-20000, 20000, size=n, dtype=np.int16)
        else:
            arrays[f"u{i}"] = rng.normal(0, 0.1, size=n).astype(np.float32)
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    return corpus, [arrays[nm] for nm in corpus.names]


@functools.lru_cache(maxsize=None)
def bank_arrays():
    rng = np.random.default_rng(17)
    return tuple(np.ones(1, np.float32) if n == 1 else rng.normal(0, 0.2, size=n).astype(np.float32) for n in RIR_LENGTHS)


def make_bank(device=DEV):
    return rv.RirBank.from_arrays(list(bank_arrays()), 8000, device=device, normalise=None), list(bank_arrays())


def plen(corpus, u, p):
    return sr.perturbed_len(int(corpus.lengths[u]), int(p))


def both_plan(corpus, bank, M, S, seed=0, ns=NS):
    """A table of len(ns) examples.  Source terms run through the kinds both / both / both / speed only / RIR only, with a speed from
    90, 95, 105, 110 and any response (all of its taps); a mixture term beyond the S sources (``M == S + 1``) has neither.  Each term's
    utterance is one whose PERTURBED length holds n; starts run through 0, 1, an odd mid start and P - n.  Targets run through the four
    kinds at the mixture term's speed: the direct path, dry, the mixture term itself (the computed-once path), an explicit tap count.  The
    last example (n = 4) is the 37-sample utterance, perturbed, under the 2500-tap response."""
    rng = np.random.default_rng(seed)
    B, NT = len(ns), M + S
    short = int(np.argmin(corpus.lengths))
    assert corpus.lengths[short] == 37
    utt, start = np.zeros((B, NT), np.int32), np.zeros((B, NT), np.int32)
    speed = np.full((B, NT), 100, np.int32)
    rir, taps = np.full((B, NT), -1, np.int32), np.ones((B, NT), np.int32)
    norm = rng.uniform(0.3, 3.0, size=(B, NT)).astype(np.float32)
    gain = rng.uniform(0.5, 1.8, size=(B, NT)).astype(np.float32)
    direct = bank.direct_taps()
    k = seed
    for b, n in enumerate(ns):
        for j in range(M):
            kind = ("both", "both", "both", "speed", "rir")[k % 5] if j < S else "neither"
            is_short = n == 4 and j < 2
            if is_short:
                kind = "both"
            p = int(rng.choice(CONVERTERS)) if kind in ("both", "speed") else 100
            r = int(rng.integers(len(bank))) if kind in ("both", "rir") else -1
            fit = [u for u in range(len(corpus)) if plen(corpus, u, p) >= n and u != short]
            u = short if is_short else fit[k % len(fit)]
            P = plen(corpus, u, p)
            s = [0, min(1, P - n), min(((P - n) // 2) | 1, P - n), P - n][k % 4]
            utt[b, j], start[b, j], speed[b, j] = u, s, p
            if r >= 0:
                r = R2500 if is_short else r
                rir[b, j], taps[b, j] = r, bank.lengths[r]
            k += 1
        for s in range(S):
            j = M + s
            for arr in (utt, start, norm, gain, speed, rir, taps):
                arr[b, j] = arr[b, s]
            if rir[b, s] < 0:
                continue
            kind = (b + s) % 4
            if kind == 0:
                taps[b, j] = direct[rir[b, s]]
            elif kind == 1:
                rir[b, j], taps[b, j] = -1, 1
            elif kind == 3:
                taps[b, j] = min(700, int(bank.lengths[rir[b, s]]))
    return df.BatchPlan([str(b) for b in range(B)], np.array(ns, np.int32), utt, start, norm, gain, M, S, speed, rir, taps)


def ref_batch(utts, hs, plan, T):
    mix, src = ref.batch(utts, hs, plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.speed, plan.rir, plan.taps, plan.M, plan.S, T)
    return torch.from_numpy(mix), torch.from_numpy(src)


def same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("fmt", ["int16", "float32", "both"])
def test_plans_bit_equal(fmt):
    """(M, S) = (2, 2), (3, 2) with a plain third term, (3, 3) and (4, 3); B = 6, Tmax = 4100, n = 4100 .. 4: mix and src equal the
    restatement bit for bit, the zero padding included; a guard region around the outputs is untouched.  Asserted here: the plans hold
    all four kinds of term, every response and every speed in a term that has both, all four kinds of target and the computed-once
    path, starts 0, 1, odd and P - n, and the 37-sample utterance under the 2500-tap response with n = 4."""
    corpus, utts = synthetic_corpus(fmt)
    assert corpus.n16 == {"int16": 6, "float32": 0, "both": 3}[fmt]
    bank, hs = make_bank()
    terms, used, sped, kinds, starts = set(), set(), set(), set(), set()
    for i, (M, S) in enumerate(((2, 2), (3, 2), (3, 3), (4, 3))):
        plan = both_plan(corpus, bank, M, S, seed=3 * i)
        B = len(plan.n)
        for b in range(B):
            for j in range(M + S):
                p, r = int(plan.speed[b, j]), int(plan.rir[b, j])
                terms.add(("both" if r >= 0 else "speed") if p != 100 else ("rir" if r >= 0 else "neither"))
                if p != 100 and r >= 0 and j < M:
                    used.add(r)
                    sped.add(p)
            for s in range(S):
                assert plan.speed[b, M + s] == plan.speed[b, s]
                m, t = (plan.rir[b, s], plan.taps[b, s]), (plan.rir[b, M + s], plan.taps[b, M + s])
                if plan.speed[b, s] != 100 and m[0] >= 0:
                    kinds.add("same" if t == m else "dry" if t[0] < 0 else "direct" if t[1] == bank.direct_taps()[t[0]] else "count")
            for j in range(M):
                P, s, n = plen(corpus, plan.utt[b, j], plan.speed[b, j]), int(plan.start[b, j]), int(plan.n[b])
                assert s + n <= P
                if plan.speed[b, j] != 100 and plan.rir[b, j] >= 0:
                    starts.add("0" if s == 0 else "1" if s == 1 else "end" if s == P - n else "odd" if s % 2 else "even")
        if M > S:
            assert (plan.rir[:, S:M] == -1).all() and (plan.speed[:, S:M] == 100).all()
        assert plan.n[-1] == 4 and corpus.lengths[plan.utt[-1, 0]] == 37 and plan.taps[-1, 0] == 2500 and plan.speed[-1, 0] != 100
        G = 64
        block = torch.full(((S + 1) * B * TMAX + 2 * G,), 123.0, device=DEV)
        body = block[G:G + (S + 1) * B * TMAX].view(S + 1, B, TMAX)
        mix, src = df.mix_batch(corpus, plan, TMAX, mix=body[0], src=[body[1 + s] for s in range(S)], rirs=bank)
        torch.cuda.synchronize()
        wm, ws = ref_batch(utts, hs, plan, TMAX)
        assert torch.equal(mix.cpu(), wm), (fmt, M, S)
        assert torch.equal(torch.stack(src).cpu(), ws), (fmt, M, S)
        assert bool((block[:G] == 123.0).all()) and bool((block[-G:] == 123.0).all())
        assert bool((mix[-1, 4:] == 0).all()) and float(mix[-1, :4].abs().max()) > 0
    assert terms == {"both", "speed", "rir", "neither"}
    assert used == set(range(len(bank))) and sped == set(CONVERTERS)
    assert kinds == {"same", "dry", "direct", "count"} and {"0", "1", "odd", "end"} <= starts


def test_equals_whole_utterance_conversion_then_the_reverb_launch():
    """The composition of the existing entries: every (utterance, speed) a term uses converted whole by ``resample.resample`` on the
    device, a float32 corpus of the results, ``sepr_dynmix_reverb_fwd`` with the same starts, responses, taps, norms and gains - the same
    bits."""
    corpus, utts = synthetic_corpus("both")
    bank, _ = make_bank()
    for M, S in ((3, 2), (3, 3)):
        plan = both_plan(corpus, bank, M, S, seed=5)
        got = df.mix_batch(corpus, plan, TMAX, rirs=bank, speeds=CONVERTERS)
        pairs = sorted({(int(u), int(p)) for u, p in zip(plan.utt.ravel(), plan.speed.ravel())})
        converted = {}
        for p in sorted({p for _, p in pairs}):
            us = [u for u, q in pairs if q == p]
            xs = [torch.from_numpy(dr.values(utts[u])) for u in us]
            ys = xs if p == 100 else rs.resample(xs, p, 100, device=DEV)
            for u, y in zip(us, ys):
                converted[f"{u}@{p}"] = y.cpu().numpy()
                assert y.shape[0] == plen(corpus, u, p)
        whole = df.Corpus.from_arrays(converted, device=DEV)
        where = np.array([[whole.index[f"{u}@{p}"] for u, p in zip(ru, rp)] for ru, rp in zip(plan.utt, plan.speed)], np.int32)
        want = df.mix_batch(whole, plan._replace(utt=where, speed=None), TMAX, rirs=bank)
        assert same(got, want), (M, S)


def test_degenerate_plans_give_the_existing_launches():
    """All speeds 100: the bits of ``sepr_dynmix_reverb_fwd``.  All ``rir`` -1, and the unit impulse (RIR 0 = [1.0]) in every term at
    every speed: the bits of ``sepr_dynmix_speed_fwd``.  Both off: those of ``sepr_dynmix_fwd``."""
    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    for M, S in ((2, 2), (4, 3)):
        plan = both_plan(corpus, bank, M, S, seed=2)
        assert set(CONVERTERS) <= {int(p) for p in plan.speed.ravel()}
        dry = plan._replace(rir=np.full_like(plan.rir, -1), taps=np.ones_like(plan.taps))
        speed_launch = df.mix_batch(corpus, dry._replace(rir=None, taps=None), TMAX)
        assert same(df.mix_batch(corpus, dry, TMAX, rirs=bank), speed_launch)
        unit = plan._replace(rir=np.zeros_like(plan.rir), taps=np.ones_like(plan.taps))
        assert same(df.mix_batch(corpus, unit, TMAX, rirs=bank), speed_launch)
        # at 100 % the starts must fit the stored lengths: the starts of a plan made for them
        slow = plan._replace(speed=np.full_like(plan.speed, 100), start=np.minimum(plan.start, corpus.lengths[plan.utt] - plan.n[:, None]).astype(np.int32))
        assert (slow.start >= 0).all() and (slow.rir >= 0).any()
        assert same(df.mix_batch(corpus, slow, TMAX, rirs=bank), df.mix_batch(corpus, slow._replace(speed=None), TMAX, rirs=bank))
        assert same(df.mix_batch(corpus, slow, TMAX, rirs=bank, speeds=CONVERTERS), df.mix_batch(corpus, slow._replace(speed=None), TMAX, rirs=bank))
        off = slow._replace(rir=np.full_like(plan.rir, -1), taps=np.ones_like(plan.taps))
        assert same(df.mix_batch(corpus, off, TMAX, rirs=bank), df.mix_batch(corpus, off._replace(speed=None, rir=None, taps=None), TMAX))


def test_determinism_and_independence():
    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    plan = both_plan(corpus, bank, 3, 2, seed=9)
    a = df.mix_batch(corpus, plan, TMAX, rirs=bank, speeds=CONVERTERS)
    b = df.mix_batch(corpus, plan, TMAX, rirs=bank, speeds=CONVERTERS)
    assert same(a, b)
    for i in range(len(plan.n)):                                             # row b of the batch is a B = 1 launch of example b
        one_ = df.BatchPlan([plan.keys[i]], plan.n[i:i + 1], plan.utt[i:i + 1], plan.start[i:i + 1], plan.norm[i:i + 1], plan.gain[i:i + 1],
                            plan.M, plan.S, plan.speed[i:i + 1], plan.rir[i:i + 1], plan.taps[i:i + 1])
        mix, src = df.mix_batch(corpus, one_, TMAX, rirs=bank)               # its own converter set: another order of the converters
        assert torch.equal(mix[0], a[0][i]) and all(torch.equal(src[s][0], a[1][s][i]) for s in range(plan.S)), i


def test_capture_replays_with_an_updated_table():
    """The launch inside a torch.cuda.graph with a fixed converter set; the device table rewritten with a second plan - other speeds,
    responses, taps and starts - and replayed: the bits are the second plan's."""
    corpus, utts = synthetic_corpus("both")
    bank, hs = make_bank()
    p0, p1 = both_plan(corpus, bank, 3, 2, seed=1), both_plan(corpus, bank, 3, 2, seed=6)
    for f in ("speed", "rir", "taps", "start"):
        assert not np.array_equal(getattr(p0, f), getattr(p1, f)), f
    B, S = len(NS), 2
    table = torch.from_numpy(df.pack_table(p0, CONVERTERS)).to(DEV)
    mix = torch.zeros(B, TMAX, device=DEV)
    src = [torch.zeros(B, TMAX, device=DEV) for _ in range(S)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.mix_batch(corpus, p0, TMAX, mix, src, table=table, rirs=bank, speeds=CONVERTERS)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        df.mix_batch(corpus, p0, TMAX, mix, src, table=table, rirs=bank, speeds=CONVERTERS)
    for plan in (p1, p0):
        table.copy_(torch.from_numpy(df.pack_table(plan, CONVERTERS)))
        graph.replay()
        torch.cuda.synchronize()
        wm, ws = ref_batch(utts, hs, plan, TMAX)
        assert torch.equal(mix.cpu(), wm) and torch.equal(torch.stack(src).cpu(), ws)


def test_through_the_feed(golden):
    """``DynamicMixFeed(planner=partial(plan_whamr, speeds=..., rirs=bank, speed_reverb=True), rirs=bank, fixed_length=True)`` on the
    fixture's corpus WITHOUT its reverberant roles: two batches equal the restatement of the plans the feed returns, and ``next_into``
    writes the same bits into the caller's tensors."""
    g = golden("dynmix")
    arrays, roles = dr.fixture_corpus(g)
    arrays = {nm: a for nm, a in arrays.items() if "_reverb/" not in nm}
    corpus = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    corpus.roles = {r: k for r, k in roles.items() if not r.endswith("_reverb")}
    utts = [arrays[nm] for nm in corpus.names]
    hs = rv.synthetic_rirs(5, 8000, rt60=(0.1, 0.3), seed=2)
    bank = rv.RirBank.from_arrays(hs, 8000, device=DEV)
    hs = [bank.rir(r) for r in range(len(bank))]
    B, T = 4, 2000
    planner = functools.partial(df.plan_whamr, speeds=range(95, 106), rirs=bank, speed_reverb=True)

    def feed():
        return df.DynamicMixFeed(corpus, planner, batch=B, max_len=T, seed=1, rirs=bank, fixed_length=True)

    f1, f2 = feed(), feed()
    assert f1.speed_reverb
    x = torch.full((B, T), 7.0, device=DEV)
    tg = [torch.full((B, T), 7.0, device=DEV) for _ in range(2)]
    it = iter(f1)
    perturbed = 0
    for _ in range(2):
        sizes, mix, src, keys = next(it)
        plan = f1.last_plan
        assert plan.speed is not None and plan.rir is not None and mix.shape == (B, T)
        assert (plan.rir[:, 2] == -1).all() and (plan.speed[:, 2] == 100).all() and (plan.rir[:, :2] >= 0).all()
        assert np.array_equal(plan.rir[:, :2], plan.rir[:, 3:]) and np.array_equal(plan.speed[:, :2], plan.speed[:, 3:])
        assert (plan.taps[:, 3:] <= plan.taps[:, :2]).all()                   # the direct path of the same RIR at the same speed
        perturbed += int((plan.speed != 100).sum())
        wm, ws = ref_batch(utts, hs, plan, T)
        assert torch.equal(mix.cpu(), wm) and torch.equal(torch.stack(src).cpu(), ws)
        p2 = f2.next_into(x, tg)
        assert p2.keys == plan.keys and np.array_equal(p2.rir, plan.rir) and np.array_equal(p2.start, plan.start) and np.array_equal(p2.speed, plan.speed)
        assert torch.equal(x, mix) and all(torch.equal(a, b) for a, b in zip(tg, src))
        it = iter(f1)                                                        # one batch per epoch of four keys
    assert perturbed > 0
    with pytest.raises(ValueError, match="rirs"):
        df.mix_batch(corpus, f1.last_plan, T)


def test_a_target_that_differs_in_one_field_is_recomputed():
    """B = 7: utt, start, norm bits, gain bits, speed, rir, taps.  Every term has a converter and a response; the example that changes the
    speed alone pairs a converter with another converter, the one that changes the response alone two responses of equal length, the one
    that changes the tap count alone cuts a response that has non-zero samples beyond the shorter count."""
    rng = np.random.default_rng(23)
    arrays = {"a16": rng.integers(-20000, 20000, size=2600, dtype=np.int16), "b16": rng.integers(-20000, 20000, size=2600, dtype=np.int16),
              "a32": rng.normal(0, 0.1, size=2700).astype(np.float32), "b32": rng.normal(0, 0.1, size=2700).astype(np.float32)}
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    utts, i = [arrays[nm] for nm in corpus.names], corpus.index
    assert sr.perturbed_len(2600, 105) >= 47 + one.TMAX
    hs = [rng.normal(0, 0.2, size=300).astype(np.float32) for _ in range(2)]
    assert all(np.all(h[77:] != 0) for h in hs)
    bank = rv.RirBank.from_arrays(hs, 8000, device=DEV, normalise=None)
    same_, changed = one.plans(df, {"utt": (i["a16"], i["a32"]), "start": (3, 40), "norm": (0.75, 1.5), "gain": (1.25, 0.5), "speed": (95, 104),
                                    "rir": (0, 1), "taps": (300, 300)},
                               {"utt": (i["b16"], i["b32"]), "start": (4, 47), "norm": (0.8, 1.4), "gain": (1.3, 0.6), "speed": (105, 96),
                                "rir": (1, 0), "taps": (120, 77)})
    assert len(changed.n) == 7 and 100 not in changed.speed and (changed.rir >= 0).all()
    one.check(lambda p: df.mix_batch(corpus, p, one.TMAX, rirs=bank), lambda p: ref_batch(utts, hs, p, one.TMAX), same_, changed)
