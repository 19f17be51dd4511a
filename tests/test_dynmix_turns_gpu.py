"""Turn-taking inside the mixing launch: ``sepr_dynmix_turns_fwd`` against the numpy restatement
(tests/dynmix_turns_ref.py, bit for bit), against each of the four existing entries for plans whose every turn is open, run to run and row by
row, under graph capture, through ``DynamicMixFeed``, and its refusals and clamps."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_speed_ref as sr                                                # noqa: E402
import dynmix_turns_ref as ref                                               # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TMAX = 4100                                                                  # a multiple of 4, not of 8: tiles of 2048, 2048 and 4
NS = [4100, 4096, 2052, 2048, 2044, 4]
RIR_LENGTHS = [1, 2, 1023, 1024, 1025, 2500, 3073]                           # both sides of the 1024-tap chunk boundary, 1 to 4 chunks
R2, R2500 = RIR_LENGTHS.index(2), RIR_LENGTHS.index(2500)
SPEEDS = [90, 95, 100, 105, 110]
CONVERTERS = [p for p in SPEEDS if p != 100]                                 # a fixed converter set: index k = CONVERTERS[k]
FAR = ref.FAR
RL = 80
LENGTHS = ((5000, True), (4101, True), (2600, True), (4999, False), (3000, False), (37, False))


def synthetic_corpus(fmt, device=DEV):
    """Six utterances of 5000, 4101, 2600 (int16) and 4999, 3000, 37 (float32) samples - ``fmt`` "int16" / "float32" stores all six in
    that format - with large values, so a read into a neighbour is not a read of zeros."""
    rng = np.random.default_rng(7)
    arrays = {}
    for i, (n, is16) in enumerate(LENGTHS):
        if fmt == "int16" or (fmt == "both" and is16):
            arrays[f"u{i}"] = rng.integers(-20000, 20000, size=n, dtype=np.int16)
        else:
            arrays[f"u{i}"] = rng.normal(0, 0.1, size=n).astype(np.float32)
    corpus = df.Corpus.from_arrays(arrays, device=device)
    return corpus, [arrays[nm] for nm in corpus.names]


@functools.lru_cache(maxsize=None)
def bank_arrays():
    rng = np.random.default_rng(17)
    return tuple(np.ones(1, np.float32) if n == 1 else rng.normal(0, 0.2, size=n).astype(np.float32) for n in RIR_LENGTHS)


def make_bank(device=DEV):
    return rv.RirBank.from_arrays(list(bank_arrays()), 8000, device=device, normalise=None), list(bank_arrays())


def plen(corpus, u, p):
    return sr.perturbed_len(int(corpus.lengths[u]), int(p))


def turn_pool(n):
    """The turns the source terms of an example of n samples run through."""
    if n > 2048:                                                             # two tiles and more: the tile edge, both ends of the example, tile 1 silent
        return [(2047, n), (2048, n - 1), (2049, FAR), (-FAR, 1500), (1000, 1100), (300, 2100), (-FAR, FAR), (-500, 1500)]
    if n > 4:
        return [(-500, n), (10, n - 1), (1000, 1100), (-FAR, FAR), (n - 300, FAR), (-FAR, 700), (-500, 900)]
    return [(1, 3), (-FAR, FAR), (0, n), (-500, 2)]


def turn_plan(corpus, bank, M, S, seed=0, ns=NS):
    """A table of len(ns) examples.  Source terms run through the kinds both / both / speed / RIR / neither (a converter from 90, 95, 105, 110, any
    response with all of its taps) and through ``turn_pool``; a mixture term beyond the S sources has neither and a turn of the pool too.  Three
    terms are set by hand: example 0 (n = 4100) holds a stored term under the 2-tap response whose turn ends at 1500 - tile 1 is silent, gap
    548 - and one under the 2500-tap response with the turn (-500, 1500) from start 700 - the tail crosses the gap, the history before the crop
    is cut at -500; example 3 (n = 2048) holds a perturbed term under the 2500-tap response from start 2600 with the turn (-500, 2^30).
    Targets run through the four kinds of ``_target_rv`` at the mixture term's speed and turn; the second target of example 0 differs from its
    mixture term in the turn alone, which lies wholly past n; the last example (n = 4) is the 37-sample utterance."""
    rng = np.random.default_rng(seed)
    B, NT = len(ns), M + S
    short = int(np.argmin(corpus.lengths))
    long16, long32 = int(np.argmax(corpus.lengths)), int(np.flatnonzero(corpus.lengths == 4999)[0])
    utt, start = np.zeros((B, NT), np.int32), np.zeros((B, NT), np.int32)
    speed = np.full((B, NT), 100, np.int32)
    rir, taps = np.full((B, NT), -1, np.int32), np.ones((B, NT), np.int32)
    on, off = np.full((B, NT), -FAR, np.int32), np.full((B, NT), FAR, np.int32)
    norm = rng.uniform(0.3, 3.0, size=(B, NT)).astype(np.float32)
    gain = rng.uniform(0.5, 1.8, size=(B, NT)).astype(np.float32)
    direct = bank.direct_taps()
    k = seed
    for b, n in enumerate(ns):
        pool = turn_pool(n)
        for j in range(M):
            kind = ("both", "both", "speed", "rir", "neither")[k % 5] if j < S else "neither"
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
            on[b, j], off[b, j] = pool[(k + b) % len(pool)]
            k += 1
    for (b, j), (u, s, p, r, tn) in {(0, 0): (long16, 600, 100, R2, (-FAR, 1500)), (0, 1): (long32, 700, 100, R2500, (-500, 1500)),
                                     (3, 0): (long16, 2600, 90, R2500, (-500, FAR))}.items():
        utt[b, j], start[b, j], speed[b, j], rir[b, j], taps[b, j], (on[b, j], off[b, j]) = u, s, p, r, bank.lengths[r], tn
        assert s + ns[b] <= plen(corpus, u, p)
    for b in range(B):
        for s in range(S):
            j = M + s
            for arr in (utt, start, norm, gain, speed, rir, taps, on, off):
                arr[b, j] = arr[b, s]
            if (b, s) == (0, 1):
                on[b, j], off[b, j] = ns[b] + 5, ns[b] + 900                 # the turn alone differs, and it lies wholly outside [0, n)
                continue
            if rir[b, s] < 0:
                continue
            kind = (b + s) % 4
            if kind == 0:
                taps[b, j] = direct[rir[b, s]]
            elif kind == 1:
                rir[b, j], taps[b, j] = -1, 1
            elif kind == 3:
                taps[b, j] = min(700, int(bank.lengths[rir[b, s]]))
    return df.BatchPlan([str(b) for b in range(B)], np.array(ns, np.int32), utt, start, norm, gain, M, S, speed, rir, taps, on=on, off=off)


def coverage(plan, seen):
    """What the issue asks the turns to include, read off the table."""
    M, S = plan.M, plan.S
    for b, n in enumerate(int(v) for v in plan.n):
        for j in range(M + S):
            p, r, k, a, z, s = (int(arr[b, j]) for arr in (plan.speed, plan.rir, plan.taps, plan.on, plan.off, plan.start))
            seen.add(("kind", ("both" if r >= 0 else "speed") if p != 100 else ("rir" if r >= 0 else "neither")))
            if a in (2047, 2048, 2049):
                seen.add(("on", a))
            if z in (n, n - 1):
                seen.add(("off", "n" if z == n else "n-1"))
            if a == -500 and r >= 0 and k == 2500 and s >= 500:
                seen.add(("history", "perturbed" if p != 100 else "stored"))
            if 0 < z - a < 2 * RL:
                seen.add("short")
            if n > 2048 and r >= 0 and 0 < z <= 2048:                       # the turn ends inside tile 0
                seen.add(("tile 1", "silent" if 2048 >= z + k - 1 else "tail"))
            if a >= n or z <= 0:
                seen.add("outside")
        for s in range(S):
            fields = [arr[b, s] == arr[b, M + s] for arr in (plan.utt, plan.start, plan.norm, plan.gain, plan.speed, plan.rir, plan.taps)]
            turn = plan.on[b, s] == plan.on[b, M + s] and plan.off[b, s] == plan.off[b, M + s]
            if all(fields):
                seen.add("same" if turn else "turn alone")
    return seen


WANT = {("kind", "both"), ("kind", "speed"), ("kind", "rir"), ("kind", "neither"), ("on", 2047), ("on", 2048), ("on", 2049), ("off", "n"),
        ("off", "n-1"), ("history", "perturbed"), ("history", "stored"), "short", ("tile 1", "silent"), ("tile 1", "tail"), "outside", "same",
        "turn alone"}


def ref_batch(utts, hs, plan, T, ramp=RL):
    mix, src = ref.batch(utts, hs, plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.speed, plan.rir, plan.taps, plan.on, plan.off,
                         ref.ramp_table(ramp), plan.M, plan.S, T)
    return torch.from_numpy(mix), torch.from_numpy(src)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and len(a[1]) == len(b[1]) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("fmt,ramp", [("both", 0), ("both", 1), ("both", 80), ("int16", 80), ("float32", 80)])
def test_plans_bit_equal(fmt, ramp):
    """(M, S) = (2, 2), (3, 2), (3, 3) and (4, 3); B = 6, Tmax = 4100, n = 4100 .. 4: mix and src equal the restatement in every bit - signs of
    zeros included - with the zero padding; a guard region around the outputs is untouched.  Asserted here: the plans hold all four kinds of
    term, ``on`` at 2047, 2048 and 2049, ``off`` at n and n - 1, on = -500 inside the history of a 2500-tap response over a stored and over a
    perturbed utterance, a turn shorter than 2 RL, a turn that ends inside tile 0 under a response shorter and one longer than the gap to tile 1,
    a turn wholly outside [0, n) - that target row is +0.0 in every bit - a target that is its mixture term and one that differs from it in the
    turn alone."""
    corpus, utts = synthetic_corpus(fmt)
    assert corpus.n16 == {"int16": 6, "float32": 0, "both": 3}[fmt]
    bank, hs = make_bank()
    seen = set()
    for i, (M, S) in enumerate(((2, 2), (3, 2), (3, 3), (4, 3))):
        plan = turn_plan(corpus, bank, M, S, seed=3 * i)
        coverage(plan, seen)
        B = len(plan.n)
        G = 64
        block = torch.full(((S + 1) * B * TMAX + 2 * G,), 123.0, device=DEV)
        body = block[G:G + (S + 1) * B * TMAX].view(S + 1, B, TMAX)
        mix, src = df.mix_batch(corpus, plan, TMAX, mix=body[0], src=[body[1 + s] for s in range(S)], rirs=bank, speeds=CONVERTERS, ramp=ramp)
        torch.cuda.synchronize()
        wm, ws = ref_batch(utts, hs, plan, TMAX, ramp)
        assert torch.equal(bits(mix.cpu()), bits(wm)), (fmt, M, S)
        assert torch.equal(bits(torch.stack(src).cpu()), bits(ws)), (fmt, M, S)
        assert bool((block[:G] == 123.0).all()) and bool((block[-G:] == 123.0).all())
        assert bool((mix[-1, 4:] == 0).all()) and float(mix[-1, :4].abs().max()) > 0
        assert plan.on[0, M + 1] >= plan.n[0] and bool((bits(src[1][0]) == 0).all())           # the turn wholly outside: +0.0, not -0.0
        assert float(src[0][0].abs().max()) > 0 and float(src[0][0, 2048:].abs().max()) == 0     # the silent tile 1 under the 2-tap response
        assert float(mix[0, 2048:3900].abs().min()) > 0                                          # the 2500-tap tail rings on in tile 1
    assert seen == WANT


def test_open_turns_are_the_old_launches():
    """A plan whose every turn is open equals, bit for bit, the launch of the same plan without the columns through each of the four existing
    entries: speed-reverb, reverb, speed and plain."""
    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    for M, S in ((2, 2), (4, 3)):
        plan = turn_plan(corpus, bank, M, S, seed=2)._replace(on=None, off=None)
        kinds = {(p != 100, r >= 0) for p, r in zip(plan.speed.ravel(), plan.rir.ravel())}
        assert kinds == {(True, True), (True, False), (False, True), (False, False)}
        slow = plan._replace(speed=None, start=np.minimum(plan.start, corpus.lengths[plan.utt] - plan.n[:, None]).astype(np.int32))
        assert (slow.start >= 0).all()
        olds = {"sepr_dynmix_speed_reverb_fwd": plan, "sepr_dynmix_reverb_fwd": slow, "sepr_dynmix_speed_fwd": plan._replace(rir=None, taps=None),
                "sepr_dynmix_fwd": slow._replace(rir=None, taps=None)}
        for entry, old in olds.items():
            opened = old._replace(on=np.full_like(old.utt, -FAR), off=np.full_like(old.utt, FAR))
            for ramp in (0, 80):
                assert same(df.mix_batch(corpus, opened, TMAX, rirs=bank, ramp=ramp), df.mix_batch(corpus, old, TMAX, rirs=bank)), (entry, M, S, ramp)


def test_determinism_and_independence():
    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    plan = turn_plan(corpus, bank, 3, 2, seed=9)
    a = df.mix_batch(corpus, plan, TMAX, rirs=bank, speeds=CONVERTERS, ramp=RL)
    b = df.mix_batch(corpus, plan, TMAX, rirs=bank, speeds=CONVERTERS, ramp=RL)
    assert same(a, b)
    for i in range(len(plan.n)):                                             # row b of the batch is a B = 1 launch of example b
        one = df.BatchPlan([plan.keys[i]], plan.n[i:i + 1], plan.utt[i:i + 1], plan.start[i:i + 1], plan.norm[i:i + 1], plan.gain[i:i + 1],
                           plan.M, plan.S, plan.speed[i:i + 1], plan.rir[i:i + 1], plan.taps[i:i + 1], on=plan.on[i:i + 1], off=plan.off[i:i + 1])
        mix, src = df.mix_batch(corpus, one, TMAX, rirs=bank, ramp=RL)       # its own converter set: another order of the converters
        assert torch.equal(bits(mix[0]), bits(a[0][i])) and all(torch.equal(bits(src[s][0]), bits(a[1][s][i])) for s in range(plan.S)), i


def test_capture_replays_with_an_updated_table():
    """The launch inside a torch.cuda.graph with a fixed converter set; the device table rewritten with a second plan - other turns among the
    rest - and replayed: the bits are the second plan's."""
    corpus, utts = synthetic_corpus("both")
    bank, hs = make_bank()
    p0, p1 = turn_plan(corpus, bank, 3, 2, seed=1), turn_plan(corpus, bank, 3, 2, seed=6)
    for f in ("speed", "rir", "start", "on", "off"):
        assert not np.array_equal(getattr(p0, f), getattr(p1, f)), f
    B, S = len(NS), 2
    table = torch.from_numpy(df.pack_table(p0, CONVERTERS)).to(DEV)
    mix = torch.zeros(B, TMAX, device=DEV)
    src = [torch.zeros(B, TMAX, device=DEV) for _ in range(S)]
    ramp = df.ramp_table(DEV, RL)                                            # uploaded before the capture, as a feed does when it is built
    assert ramp.shape == (RL,) and np.array_equal(ramp.cpu().numpy(), ref.ramp_table(RL))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.mix_batch(corpus, p0, TMAX, mix, src, table=table, rirs=bank, speeds=CONVERTERS, ramp=ramp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        df.mix_batch(corpus, p0, TMAX, mix, src, table=table, rirs=bank, speeds=CONVERTERS, ramp=ramp)
    for plan in (p1, p0):
        table.copy_(torch.from_numpy(df.pack_table(plan, CONVERTERS)))
        graph.replay()
        torch.cuda.synchronize()
        wm, ws = ref_batch(utts, hs, plan, TMAX)
        assert torch.equal(bits(mix.cpu()), bits(wm)) and torch.equal(bits(torch.stack(src).cpu()), bits(ws))


def test_through_the_feed(golden):
    """``DynamicMixFeed(planner=partial(plan_whamr, turns=Turns(...), speeds=..., rirs=bank, speed_reverb=True), rirs=bank, fixed_length=True)``
    on the fixture's corpus without its reverberant roles: two batches equal the restatement of the plans the feed returns, and ``next_into``
    writes the same bits into the caller's static tensors.  Without a bank and without speeds the same feed runs on R = 0 and NC = 0."""
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
    turns = df.Turns((0.0, 0.6), 40)
    planner = functools.partial(df.plan_whamr, turns=turns, speeds=range(95, 106), rirs=bank, speed_reverb=True)

    def feed():
        return df.DynamicMixFeed(corpus, planner, batch=B, max_len=T, seed=1, rirs=bank, fixed_length=True)

    f1, f2 = feed(), feed()
    assert f1.speed_reverb and f1.turns == turns and f1._ramp.shape == (turns.ramp,) and f1._ramp.device.type == "cuda"
    x = torch.full((B, T), 7.0, device=DEV)
    tg = [torch.full((B, T), 7.0, device=DEV) for _ in range(2)]
    it = iter(f1)
    gated = 0
    for _ in range(2):
        sizes, mix, src, keys = next(it)
        plan = f1.last_plan
        assert plan.on is not None and plan.speed is not None and plan.rir is not None and mix.shape == (B, T)
        assert np.array_equal(plan.on[:, :2], plan.on[:, 3:]) and np.array_equal(plan.off[:, :2], plan.off[:, 3:])
        assert (plan.on[:, 2] == -FAR).all() and (plan.off[:, 2] == FAR).all()
        gated += int((plan.on[:, :2] > -FAR).sum() + (plan.off[:, :2] < FAR).sum())
        wm, ws = ref_batch(utts, hs, plan, T, turns.ramp)
        assert torch.equal(bits(mix.cpu()), bits(wm)) and torch.equal(bits(torch.stack(src).cpu()), bits(ws))
        p2 = f2.next_into(x, tg)
        assert p2.keys == plan.keys and np.array_equal(p2.on, plan.on) and np.array_equal(p2.off, plan.off) and np.array_equal(p2.start, plan.start)
        assert torch.equal(bits(x), bits(mix)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(tg, src))
        it = iter(f1)                                                        # one batch per epoch of four keys
    assert gated > 0
    for bad in (None, True, -1, 4097, torch.zeros(8), torch.zeros(8, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError, match="ramp"):
            df.mix_batch(corpus, f1.last_plan, T, rirs=bank, ramp=bad)
    # turns alone: the dry sources, no converter and no bank
    arrays, roles = dr.fixture_corpus(g)
    whole = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    whole.roles = dict(roles)
    alone = df.DynamicMixFeed(whole, functools.partial(df.plan_wham, turns=df.Turns((0.0, 0.0), 0)), batch=B, max_len=T, seed=3, fixed_length=True)
    sizes, mix, src, keys = next(iter(alone))
    plan = alone.last_plan
    assert plan.on is not None and plan.speed is None and plan.rir is None and (plan.off[:, :2] < FAR).any()
    full = plan._replace(speed=np.full_like(plan.utt, 100), rir=np.full_like(plan.utt, -1), taps=np.ones_like(plan.utt))
    wm, ws = ref_batch([arrays[nm] for nm in whole.names], [], full, T, 0)
    assert torch.equal(bits(mix.cpu()), bits(wm)) and torch.equal(bits(torch.stack(src).cpu()), bits(ws))


def test_refusals_and_clamps():
    """Every refusal of ``sepr_dynmix_turns_fwd`` comes before any HIP call.  Then a launch the entry accepts, with a table of wild fields -
    ``on`` and ``off`` at INT_MIN and INT_MAX among them: whatever it computes, the guard region around the outputs is untouched."""
    lib = L_.load()
    p = 0x1000                                                               # never dereferenced: the checks reject the call first
    rows2 = (C.c_void_p * 2)(p, p)
    E = L_.SEPR_EINVAL

    def conv(L=(20, 20), M=(19, 21), K=(138, 132), taps=(p, p)):
        return dict(taps=(C.c_void_p * len(taps))(*taps), cl=(C.c_int * len(L))(*L), cm=(C.c_int * len(M))(*M), ck=(C.c_int * len(K))(*K), NC=len(L))

    def mix(buf16=p, t16=100, buf32=None, t32=0, off=p, n16=3, N=3, tu=p, ts=p, tn=p, tg=p, tc=p, tr=p, tt=p, ton=p, toff=p, n=p, B=2, M=2, S=2, T=64,
            out=p, rows=rows2, taps=None, cl=None, cm=None, ck=None, NC=0, rir=p, rtot=10, roff=p, R=2, ramp=p, RL=80):
        return lib.sepr_dynmix_turns_fwd(buf16, t16, buf32, t32, off, n16, N, tu, ts, tn, tg, tc, tr, tt, ton, toff, n, B, M, S, T, out, rows, taps, cl,
                                         cm, ck, NC, rir, rtot, roff, R, ramp, RL, None)

    for kw in (dict(RL=-1), dict(RL=4097), dict(ramp=None), dict(ramp=None, RL=1), dict(ramp=p + 2), dict(ton=None), dict(toff=None),
               # what the speed-reverb entry refuses: the common arguments, the converters, the bank
               dict(off=None), dict(tu=None), dict(ts=None), dict(tn=None), dict(tg=None), dict(n=None), dict(out=None), dict(rows=None),
               dict(rows=(C.c_void_p * 2)(p, None)), dict(buf16=None), dict(B=0), dict(B=65536), dict(S=1), dict(M=1), dict(M=4), dict(T=0),
               dict(T=62), dict(out=p + 4), dict(buf16=p + 2), dict(N=0, n16=0), dict(n16=4), dict(t16=0), dict(t32=-1),
               dict(tc=None), dict(NC=-1), dict(NC=17), dict(tr=None), dict(tt=None), dict(rir=None), dict(roff=None), dict(R=-1), dict(rtot=0),
               dict(rir=p + 2), dict(R=0, tr=None), dict(R=0, tt=None)):
        assert mix(**kw) == E, kw
        if "NC" not in kw:
            assert mix(**kw, **conv()) == E, kw
    for kw in (dict(taps=(p, None)), dict(L=(20, 0)), dict(M=(0, 21)), dict(K=(137, 132)), dict(L=(20, 2), M=(19, 3), K=(138, 194))):
        assert mix(**conv(**kw)) == E, kw
    good = conv()
    for name in ("taps", "cl", "cm", "ck"):
        assert mix(**{**good, name: None}) == E, name

    corpus, _ = synthetic_corpus("both")
    bank, _ = make_bank()
    plan = turn_plan(corpus, bank, 3, 2, seed=4)
    B, NT = plan.utt.shape
    rng = np.random.default_rng(1)
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    wild = lambda: rng.choice(np.array([lo, lo + 1, -FAR - 1, -1, 0, 1, 2047, 4100, 70000, FAR + 1, hi - 1, hi], np.int64), size=(B, NT)).astype(np.int32)      # noqa: E731
    bad = plan._replace(on=wild(), off=wild())
    assert (bad.on == lo).any() and (bad.off == hi).any() and (bad.on == hi).any() and (bad.off == lo).any()
    table = df.pack_table(bad, CONVERTERS)
    lay = df.table_layout(B, NT, turns=True)
    for name in ("utt", "start", "conv", "rir", "taps"):                     # wild indices as well; n stays (it is clamped to Tmax anyway)
        first, words = lay[name]
        table[first:first + words] = wild().ravel()
    S, G = plan.S, 4096
    for ramp in (0, RL):
        block = torch.full(((S + 1) * B * TMAX + 2 * G,), 123.0, device=DEV)
        body = block[G:G + (S + 1) * B * TMAX].view(S + 1, B, TMAX)
        df.mix_batch(corpus, bad, TMAX, mix=body[0], src=[body[1 + s] for s in range(S)], table=torch.from_numpy(table).to(DEV), rirs=bank,
                     speeds=CONVERTERS, ramp=ramp)
        torch.cuda.synchronize()
        assert bool((block[:G] == 123.0).all()) and bool((block[-G:] == 123.0).all())
        assert bool((body[:, -1, 4:] == 0).all())                            # the zero padding of the n = 4 example, whatever the table says
