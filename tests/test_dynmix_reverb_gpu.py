"""Reverberation inside the mixing launch: ``sepr_dynmix_reverb_fwd`` against the numpy restatement
(tests/dynmix_reverb_ref.py, bit for bit), against the plain ``sepr_dynmix_fwd`` over whole utterances convolved on the host, against
the plain launch for plans without a response and with the unit impulse, run to run and row by row, under graph capture and through
``DynamicMixFeed``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_one_field as one                                               # noqa: E402
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_reverb_ref as ref                                              # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TMAX = 4100                                                                  # a multiple of 4, not of 8: tiles of 2048, 2048 and 4
NS = [4100, 4096, 2052, 2048, 2044, 4]
RIR_LENGTHS = [1, 2, 1023, 1024, 1025, 2500, 3073]                           # both sides of the 1024-tap chunk boundary, 1 to 4 chunks
R2500 = RIR_LENGTHS.index(2500)


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


def reverb_plan(corpus, bank, M, S, seed=0, ns=NS, wet=None):
    """A table of len(ns) examples.  Mixture source terms run through every RIR (all of its taps); a mixture term beyond the S sources
    (``M == S + 1``) is not reverberated.  Targets run through the four kinds: the direct path, dry, the mixture term itself (the
    computed-once path), an explicit tap count.  Starts run through 0, 1, an odd mid start and T - n.  The last example (n = 4) is the
    37-sample utterance under the 2500-tap response."""
    rng = np.random.default_rng(seed)
    B, NT = len(ns), M + S
    lens = corpus.lengths
    short = int(np.argmin(lens))
    assert lens[short] == 37
    utt, start = np.zeros((B, NT), np.int32), np.zeros((B, NT), np.int32)
    rir, taps = np.full((B, NT), -1, np.int32), np.ones((B, NT), np.int32)
    norm = rng.uniform(0.3, 3.0, size=(B, NT)).astype(np.float32)
    gain = rng.uniform(0.5, 1.8, size=(B, NT)).astype(np.float32)
    direct = bank.direct_taps()
    k = seed
    for b, n in enumerate(ns):
        for j in range(M):
            fit = [u for u in range(len(corpus)) if lens[u] >= n and u != short]
            u = short if (n == 4 and j < 2) else fit[k % len(fit)]
            T = int(lens[u])
            s = [0, min(1, T - n), min(((T - n) // 2) | 1, T - n), T - n][k % 4]
            utt[b, j], start[b, j] = u, s
            if j < S and wet is not False:
                r = R2500 if u == short else k % len(bank)
                rir[b, j], taps[b, j] = r, bank.lengths[r]
            k += 1
        for s in range(S):
            j = M + s
            for arr in (utt, start, norm, gain, rir, taps):
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
    return df.BatchPlan([str(b) for b in range(B)], np.array(ns, np.int32), utt, start, norm, gain, M, S, None, rir, taps)


def ref_batch(utts, hs, plan, T):
    mix, src = ref.batch(utts, hs, plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.rir, plan.taps, plan.M, plan.S, T)
    return torch.from_numpy(mix), torch.from_numpy(src)


def same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("fmt", ["int16", "float32", "both"])
def test_reverb_plans_bit_equal(fmt):
    """(M, S) = (2, 2), (3, 2) with an unreverberated third term, (3, 3) and (4, 3); B = 6, Tmax = 4100, n = 4100 .. 4; every RIR length
    in a mixture term, all four kinds of target, the computed-once path, starts 0, 1, odd and T - n: mix and src equal the restatement
    bit for bit, the zero padding included; a guard region around the outputs is untouched."""
    corpus, utts = synthetic_corpus(fmt)
    assert corpus.n16 == {"int16": 6, "float32": 0, "both": 3}[fmt]
    bank, hs = make_bank()
    used, kinds, starts = set(), set(), set()
    for i, (M, S) in enumerate(((2, 2), (3, 2), (3, 3), (4, 3))):
        plan = reverb_plan(corpus, bank, M, S, seed=3 * i)
        B = len(plan.n)
        used |= {int(r) for r in plan.rir[:, :M].ravel()}
        for b in range(B):
            for s in range(S):
                m, t = (plan.rir[b, s], plan.taps[b, s]), (plan.rir[b, M + s], plan.taps[b, M + s])
                kinds.add("same" if t == m else "dry" if t[0] < 0 else "direct" if t[1] == bank.direct_taps()[t[0]] else "count")
            for j in range(M):
                T, s, n = int(corpus.lengths[plan.utt[b, j]]), int(plan.start[b, j]), int(plan.n[b])
                starts.add("0" if s == 0 else "1" if s == 1 else "end" if s == T - n else "odd" if s % 2 else "even")
        if M > S:
            assert (plan.rir[:, S:M] == -1).all()
        assert plan.n[-1] == 4 and corpus.lengths[plan.utt[-1, 0]] == 37 and plan.taps[-1, 0] == 2500
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
    assert used == set(range(len(bank))) | {-1}
    assert kinds == {"same", "dry", "direct", "count"} and {"0", "1", "odd", "end"} <= starts


def test_equals_whole_utterance_convolution_then_plain_mix():
    """Every (utterance, response, taps) a term uses convolved whole on the host (the restatement's float64 sums, truncated to the
    stored length, rounded to float32), a float32 corpus of the results, the existing ``sepr_dynmix_fwd`` with the same starts, norms
    and gains: the same bits as the reverberant launch on the dry corpus."""
    corpus, utts = synthetic_corpus("both")
    bank, hs = make_bank()
    for M, S in ((3, 2), (3, 3)):
        plan = reverb_plan(corpus, bank, M, S, seed=5)
        got = df.mix_batch(corpus, plan, TMAX, rirs=bank)
        trip = sorted({(int(u), int(r), int(k) if r >= 0 else 1) for u, r, k in zip(plan.utt.ravel(), plan.rir.ravel(), plan.taps.ravel())})
        whole = {}
        for u, r, k in trip:
            x = dr.values(utts[u])
            whole[f"{u}@{r}@{k}"] = x if r < 0 else ref.conv64(x, hs[r], 0, x.shape[0], k).astype(np.float32)
        wet = df.Corpus.from_arrays(whole, device=DEV)
        where = np.array([[wet.index[f"{u}@{r}@{k if r >= 0 else 1}"] for u, r, k in zip(ru, rr, rk)]
                          for ru, rr, rk in zip(plan.utt, plan.rir, plan.taps)], np.int32)
        want = df.mix_batch(wet, plan._replace(utt=where, rir=None, taps=None), TMAX)
        assert same(got, want), (M, S)


def test_no_response_and_unit_impulse_give_the_plain_launch():
    """A plan whose every ``rir`` is -1, and one whose every term takes the unit impulse (RIR 0 = [1.0]): the bits of
    ``sepr_dynmix_fwd``."""
    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    for M, S in ((2, 2), (4, 3)):
        plan = reverb_plan(corpus, bank, M, S, seed=2, wet=False)
        assert (plan.rir == -1).all()
        plain = df.mix_batch(corpus, plan._replace(rir=None, taps=None), TMAX)
        assert same(df.mix_batch(corpus, plan, TMAX, rirs=bank), plain)
        unit = plan._replace(rir=np.zeros_like(plan.rir), taps=np.ones_like(plan.taps))
        assert same(df.mix_batch(corpus, unit, TMAX, rirs=bank), plain)
        half = unit._replace(rir=np.where(np.arange(M + S)[None, :] % 2 == 0, 0, -1).astype(np.int32).repeat(len(plan.n), 0))
        assert same(df.mix_batch(corpus, half, TMAX, rirs=bank), plain)


def test_determinism_and_independence():
    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    plan = reverb_plan(corpus, bank, 3, 2, seed=9)
    a = df.mix_batch(corpus, plan, TMAX, rirs=bank)
    b = df.mix_batch(corpus, plan, TMAX, rirs=bank)
    assert same(a, b)
    for i in range(len(plan.n)):                                             # row b of the batch is a B = 1 launch of example b
        one = df.BatchPlan([plan.keys[i]], plan.n[i:i + 1], plan.utt[i:i + 1], plan.start[i:i + 1], plan.norm[i:i + 1], plan.gain[i:i + 1],
                           plan.M, plan.S, None, plan.rir[i:i + 1], plan.taps[i:i + 1])
        mix, src = df.mix_batch(corpus, one, TMAX, rirs=bank)
        assert torch.equal(mix[0], a[0][i]) and all(torch.equal(src[s][0], a[1][s][i]) for s in range(plan.S)), i


def test_capture_replays_with_an_updated_table():
    """The launch inside a torch.cuda.graph; the device table rewritten with a second plan - other RIRs, taps and starts - and
    replayed: the bits are the second plan's."""
    corpus, utts = synthetic_corpus("both")
    bank, hs = make_bank()
    p0, p1 = reverb_plan(corpus, bank, 3, 2, seed=1), reverb_plan(corpus, bank, 3, 2, seed=6)
    assert not np.array_equal(p0.rir, p1.rir) and not np.array_equal(p0.taps, p1.taps) and not np.array_equal(p0.start, p1.start)
    B, S = len(NS), 2
    table = torch.from_numpy(df.pack_table(p0)).to(DEV)
    mix = torch.zeros(B, TMAX, device=DEV)
    src = [torch.zeros(B, TMAX, device=DEV) for _ in range(S)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.mix_batch(corpus, p0, TMAX, mix, src, table=table, rirs=bank)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        df.mix_batch(corpus, p0, TMAX, mix, src, table=table, rirs=bank)
    for plan in (p1, p0):
        table.copy_(torch.from_numpy(df.pack_table(plan)))
        graph.replay()
        torch.cuda.synchronize()
        wm, ws = ref_batch(utts, hs, plan, TMAX)
        assert torch.equal(mix.cpu(), wm) and torch.equal(torch.stack(src).cpu(), ws)


def test_through_the_feed(golden):
    """``DynamicMixFeed(planner=partial(plan_whamr, rirs=bank), rirs=bank, fixed_length=True)`` on the fixture's corpus WITHOUT its
    reverberant roles: two batches equal the restatement of the plans the feed returns, and ``next_into`` writes the same bits into
    the caller's tensors."""
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
    planner = functools.partial(df.plan_whamr, rirs=bank)

    def feed():
        return df.DynamicMixFeed(corpus, planner, batch=B, max_len=T, seed=1, rirs=bank, fixed_length=True)

    f1, f2 = feed(), feed()
    x = torch.full((B, T), 7.0, device=DEV)
    tg = [torch.full((B, T), 7.0, device=DEV) for _ in range(2)]
    it = iter(f1)
    for _ in range(2):
        sizes, mix, src, keys = next(it)
        plan = f1.last_plan
        assert plan.rir is not None and (plan.rir[:, 2] == -1).all() and (plan.rir[:, :2] >= 0).all() and mix.shape == (B, T)
        assert np.array_equal(plan.rir[:, :2], plan.rir[:, 3:]) and (plan.taps[:, 3:] <= plan.taps[:, :2]).all()       # the direct path of the same RIR
        wm, ws = ref_batch(utts, hs, plan, T)
        assert torch.equal(mix.cpu(), wm) and torch.equal(torch.stack(src).cpu(), ws)
        p2 = f2.next_into(x, tg)
        assert p2.keys == plan.keys and np.array_equal(p2.rir, plan.rir) and np.array_equal(p2.start, plan.start)
        assert torch.equal(x, mix) and all(torch.equal(a, b) for a, b in zip(tg, src))
        it = iter(f1)                                                        # one batch per epoch of four keys
    with pytest.raises(ValueError, match="rirs"):
        df.mix_batch(corpus, f1.last_plan, T)
    with pytest.raises(ValueError, match="bank is on"):
        df.mix_batch(corpus, f1.last_plan, T, rirs=rv.RirBank.from_arrays(hs, 8000))


def test_a_target_that_differs_in_one_field_is_recomputed():
    """B = 6: utt, start, norm bits, gain bits, rir, taps.  The example that changes the response alone pairs two responses of equal
    length, the one that changes the tap count alone cuts a response that has non-zero samples beyond the shorter count."""
    rng = np.random.default_rng(23)
    arrays = {"a16": rng.integers(-20000, 20000, size=2600, dtype=np.int16), "b16": rng.integers(-20000, 20000, size=2600, dtype=np.int16),
              "a32": rng.normal(0, 0.1, size=2700).astype(np.float32), "b32": rng.normal(0, 0.1, size=2700).astype(np.float32)}
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    utts, i = [arrays[nm] for nm in corpus.names], corpus.index
    hs = [rng.normal(0, 0.2, size=300).astype(np.float32) for _ in range(2)]
    assert all(np.all(h[77:] != 0) for h in hs)
    bank = rv.RirBank.from_arrays(hs, 8000, device=DEV, normalise=None)
    same, changed = one.plans(df, {"utt": (i["a16"], i["a32"]), "start": (3, 40), "norm": (0.75, 1.5), "gain": (1.25, 0.5), "rir": (0, 1),
                                   "taps": (300, 300)},
                              {"utt": (i["b16"], i["b32"]), "start": (4, 47), "norm": (0.8, 1.4), "gain": (1.3, 0.6), "rir": (1, 0),
                               "taps": (120, 77)})
    assert len(changed.n) == 6
    one.check(lambda p: df.mix_batch(corpus, p, one.TMAX, rirs=bank), lambda p: ref_batch(utts, hs, p, one.TMAX), same, changed)
