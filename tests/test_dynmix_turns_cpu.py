"""Turn-taking in the dynamic-mixing feed, without a device: the gate's weight in the numpy restatement
(tests/dynmix_turns_ref.py), the planners without and with ``turns=`` replayed draw by draw, the drawn turns, the table layout with and without
the two columns, the ramp table and the parsers."""
import functools
import math
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_turns_ref as ref                                               # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

PLANNERS = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr}
FAR = 1 << 30


def host_corpus(g):
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    c.roles = dict(roles)
    c.set_energies(np.array([dr.energy(arrays[nm]) for nm in c.names], dtype=np.int64), np.zeros(0))
    return c


def host_bank():
    rng = np.random.default_rng(3)
    hs = [np.ones(1, np.float32) if n == 1 else rng.normal(0, 0.3, size=n).astype(np.float32) for n in (1, 2, 300, 1025)]
    return rv.RirBank.from_arrays(hs, 8000, device=None, normalise=None)


def test_weight_of_the_restatement():
    """0 outside the turn, symmetric inside, min(d, e) for a turn shorter than 2 RL, identically 1 for the open turn on -20000 .. 140000."""
    t = np.arange(-20000, 140000, dtype=np.int64)
    for RL in (0, 1, 80):
        ramp = ref.ramp_table(RL)
        assert np.array_equal(ref.weight(t, -FAR, FAR, ramp), np.ones(t.shape, np.float32))
        for on, off in ((100, 1000), (-500, 70), (2047, 2048), (5, 5), (7, 3), (1000, 1100), (0, 139999)):
            w = ref.weight(t, on, off, ramp)
            inside = (t >= on) & (t < off)
            assert w.dtype == np.float32 and (w[~inside] == 0).all() and (w[inside] > 0).all() and (w <= 1).all()
            if off > on:
                wi = w[inside]
                assert np.array_equal(wi, wi[::-1])                          # w(on + i) == w(off - 1 - i)
                k = min(RL, (off - on + 1) // 2)
                assert np.array_equal(wi[:k], ramp[:k]) and (wi[RL:len(wi) - RL] == 1).all()
    ramp = ref.ramp_table(80)
    w = ref.weight(np.arange(1000, 1100), 1000, 1100, ramp)                  # 100 < 2 RL: never reaches 1, the two fades meet in the middle
    assert np.array_equal(w[:50], ramp[:50]) and np.array_equal(w[50:], ramp[:50][::-1]) and w.max() < 1
    # the gate selects +0.0 and multiplies once
    y = np.array([-1.0, -0.0, 3.0, -2.0, 5.0], np.float32)
    g = ref.gated(y, 1, 1, 3, ref.ramp_table(1))                             # t = -1 .. 3, turn [1, 3): samples 2 and 3, each on the one-sample ramp
    assert np.array_equal(g.view(np.int32), (np.array([0, 0, 3.0, -2.0, 0], np.float32) * ref.ramp_table(1)[0]).astype(np.float32).view(np.int32))
    assert np.array_equal(ref.gated(y, 0, -FAR, FAR, ramp).view(np.int32), y.view(np.int32))      # the open turn keeps every bit, -0.0 included


def test_ramp_table():
    for RL in (0, 1, 2, 80, 4096):
        r = df.turn_ramp(RL)
        want = np.array([np.float32(0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / RL)) for i in range(RL)], np.float32)
        assert r.dtype == np.float32 and r.shape == (RL,) and np.array_equal(r, ref.ramp_table(RL))
        assert np.max(np.abs(r.astype(np.float64) - want.astype(np.float64)), initial=0.0) <= 2.0 ** -24      # numpy's cos against libm's: one ulp of a value below 1
        assert (np.diff(r) > 0).all() and (r > 0).all() and (r < 1).all()
        assert np.allclose(r + r[::-1], 1.0, atol=2.0 ** -23)
    assert df.turn_ramp(1)[0] == np.float32(0.5)
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            df.turn_ramp(bad)


def test_turns_and_parse_turns():
    assert df.Turns() == ((0.0, 1.0), 80) and df.parse_turns("0:1") == df.Turns() and df.parse_turns("0.25:0.5", 0) == df.Turns((0.25, 0.5), 0)
    assert df.parse_turns("1") == df.Turns((1.0, 1.0), 80)
    for bad in ("0.5:0.2", "-0.1:1", "0:1.5"):
        with pytest.raises(ValueError):
            df.parse_turns(bad)
    for ramp in (-1, 4097, 2.5, True):
        with pytest.raises(ValueError):
            df._draw_turns(random.Random(0), df.Turns((0.0, 1.0), ramp), 2, 100)


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("rho", [0.0, 0.3, 1.0])
def test_drawn_turns(S, rho):
    """d = min(n, ceil(n / (S - (S - 1) rho))), h = (n - d) // (S - 1), the s-th talker of the drawn order gets [s h, s h + d); an on <= 0 is
    -2^30, an off >= n and the last talker's is 2^30; the draws are uniform(lo, hi), then sample(range(S), S)."""
    for n in (4, 100, 2048, 31996, 32000):
        r1, r2 = random.Random(n), random.Random(n)
        got = df._draw_turns(r1, df.Turns((rho, rho)), S, n)
        assert r2.uniform(rho, rho) == rho
        order = r2.sample(range(S), S)
        assert r1.getstate() == r2.getstate() and len(got) == S
        d = min(n, math.ceil(n / (S - (S - 1) * rho)))
        h = (n - d) // (S - 1)
        assert d * S >= n
        covered = np.zeros(n, bool)
        for s, who in enumerate(order):
            on, off = got[who]
            assert on == (-FAR if s * h <= 0 else s * h) and off == (FAR if s * h + d >= n or s == S - 1 else s * h + d)
            lo, hi = max(on, 0), min(off, n)
            assert hi - lo >= n / S - 1 and hi - lo >= min(d, n - s * h)     # active for a turn's length, at least n / S
            covered[lo:hi] = True
        assert covered.all()
        if rho == 1.0:
            assert got == [(-FAR, FAR)] * S
        if rho == 0.0 and S == 2:                                            # back to back: the second begins where the first ends, or a sample before
            (a_on, a_off), (b_on, _) = got[order[0]], got[order[1]]
            assert a_on == -FAR and (n == 4 or 0 <= a_off - b_on <= 1)


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr"])
def test_planners_without_and_with_turns(golden, tag):
    """With ``turns`` the example is the example the planner makes without them from the same generator state - the two draws come after all of
    its own, replayed here - with a turn per term: each target carries its mixture term's, the noise the open one.  (That a planner without
    ``turns`` still makes the draws it made before this keyword existed is pinned by the recorded draws of tests/golden/dynmix.npz in
    tests/test_dynmix_cpu.py; ``turns=None`` against no keyword, below, only says the default is None.)"""
    g = golden("dynmix")
    corpus = host_corpus(g)
    keys = [str(k) for k in g["keys"]]
    bank = host_bank()
    planner = PLANNERS[tag]
    for extra in ({}, dict(speeds=list(range(95, 106))), dict(rirs=bank), dict(speeds=list(range(95, 106)), rirs=bank, speed_reverb=True)):
        for lo, hi in ((0.0, 1.0), (0.0, 0.0), (0.3, 0.3), (1.0, 1.0)):
            r0, r1, r2 = random.Random(8), random.Random(8), random.Random(8)
            for key in keys:
                e0 = planner(corpus, r0, key, 3000, **extra)
                e1 = planner(corpus, r1, key, 3000, turns=None, **extra)
                assert e0 == e1 and r0.getstate() == r1.getstate()
                e2 = planner(corpus, r2, key, 3000, turns=df.Turns((lo, hi), 40), **extra)
                rho = r1.uniform(lo, hi)
                order = r1.sample(range(2), 2)
                assert r1.getstate() == r2.getstate()                        # exactly the two draws, after everything else
                r0.setstate(r1.getstate())
                assert (e2.key, e2.n) == (e0.key, e0.n) and len(e2.mix) == len(e0.mix) and len(e2.tgt) == len(e0.tgt) == 2
                for t0, t2 in zip(e0.mix + e0.tgt, e2.mix + e2.tgt):
                    assert len(t2) == 9 and t2[:len(t0)] == t0 and t2[len(t0):7] == (100, -1, 1)[len(t0) - 4:]
                n = e0.n
                d = min(n, math.ceil(n / (2 - rho)))
                h = n - d
                want = [None, None]
                want[order[0]] = (-FAR, FAR if d >= n else d)
                want[order[1]] = (-FAR if h <= 0 else h, FAR)
                assert [t[7:] for t in e2.mix[:2]] == want and [t[7:] for t in e2.tgt] == want
                assert all(t[7:] == (-FAR, FAR) for t in e2.mix[2:])         # the noise
                if lo == 1.0:
                    assert want == [(-FAR, FAR)] * 2
                covered = np.zeros(n, bool)
                for on, off in want:
                    covered[max(on, 0):min(off, n)] = True
                assert covered.all()


def test_collate_and_table_layout(golden):
    g = golden("dynmix")
    corpus = host_corpus(g)
    keys = [str(k) for k in g["keys"]]
    bank = host_bank()
    assert df.BatchPlan._field_defaults["taps"] is None and df.BatchPlan(keys, None, None, None, None, None, 2, 2).on is None
    # without the columns: every layout as it was
    assert df.table_layout(3, 5) == df.table_layout(3, 5, turns=False) == {"utt": (0, 15), "start": (15, 15), "norm": (30, 15), "gain": (45, 15), "n": (60, 3)}
    assert list(df.table_layout(3, 5, True, True)) == ["utt", "start", "norm", "gain", "n", "conv", "rir", "taps"]
    # with them: one layout whatever else the plan carries
    full = df.table_layout(3, 5, turns=True)
    assert list(full) == ["utt", "start", "norm", "gain", "n", "conv", "rir", "taps", "on", "off"]
    assert full == df.table_layout(3, 5, True, False, True) == df.table_layout(3, 5, True, True, True) == df.table_layout(3, 5, False, True, True)
    assert full["on"] == (4 * 15 + 3 + 3 * 15, 15) and full["off"] == (4 * 15 + 3 + 4 * 15, 15) and df._table_words(3, 5, turns=True) == 9 * 15 + 3
    rng = random.Random(5)
    plain = df.collate_plan(corpus, [df.plan_whamr(corpus, rng, k, 3000) for k in keys])
    assert plain.on is None and plain.off is None and df.pack_table(plain).shape == (df._table_words(*plain.utt.shape),)
    forced = df.collate_plan(corpus, [df.plan_whamr(corpus, random.Random(5), k, 3000) for k in keys[:1]], turns=True)
    assert (forced.on == -FAR).all() and (forced.off == FAR).all() and forced.speed is None and forced.rir is None
    for extra in ({}, dict(speeds=[95, 105]), dict(rirs=bank), dict(speeds=[95, 105], rirs=bank, speed_reverb=True)):
        rng = random.Random(6)
        planner = functools.partial(df.plan_whamr, turns=df.Turns((0.0, 0.5), 16), **extra)
        egs = [planner(corpus, rng, k, 3000) for k in keys]
        plan = df.collate_plan(corpus, egs, rirs=extra.get("rirs"), speed_reverb=extra.get("speed_reverb", False))
        B, NT = plan.utt.shape
        assert plan.on.dtype == plan.off.dtype == np.int32 and plan.on.shape == plan.off.shape == (B, NT) == (len(keys), 5)
        assert np.array_equal(plan.on[:, :2], plan.on[:, 3:]) and np.array_equal(plan.off[:, :2], plan.off[:, 3:])
        assert (plan.on[:, 2] == -FAR).all() and (plan.off[:, 2] == FAR).all() and (plan.on > -FAR).any() and (plan.off < FAR).any()
        assert (plan.speed is not None) == ("speeds" in extra) and (plan.rir is not None) == ("rirs" in extra)
        order = plan_speeds = df.plan_speeds(plan)
        t = df.pack_table(plan)
        lay = df.table_layout(B, NT, turns=True)
        assert t.dtype == np.int32 and t.shape == (9 * B * NT + B,)
        cut = lambda name: t[lay[name][0]:lay[name][0] + lay[name][1]]       # noqa: E731
        assert np.array_equal(cut("on"), plan.on.ravel()) and np.array_equal(cut("off"), plan.off.ravel()) and np.array_equal(cut("n"), plan.n)
        assert np.array_equal(cut("utt"), plan.utt.ravel()) and np.array_equal(cut("gain"), plan.gain.ravel().view(np.int32))
        if plan.speed is None:
            assert (cut("conv") == -1).all()
        else:
            assert np.array_equal(cut("conv"), np.array([-1 if p == 100 else order.index(p) for p in plan.speed.ravel()], np.int32)) and plan_speeds
        if plan.rir is None:
            assert (cut("rir") == -1).all() and (cut("taps") == 1).all()
        else:
            assert np.array_equal(cut("rir"), plan.rir.ravel()) and np.array_equal(cut("taps"), plan.taps.ravel())
        # _replace keeps and takes the columns; the tuple is the eleven fields it was
        again = plan._replace(utt=plan.utt.copy())
        assert again.on is plan.on and again.off is plan.off and len(again) == len(plan) == 11 and isinstance(again, df.BatchPlan)
        assert list(plan._asdict())[-4:] == ["rir", "taps", "on", "off"] and plan._asdict()["on"] is plan.on
        assert df.BatchPlan(*plan).on is None                                # by position the columns are dropped: the docstring's warning
        opened = plan._replace(on=None, off=None)
        assert opened.on is None and opened.off is None and opened.speed is plan.speed
        if plan.speed is not None and plan.rir is not None:                  # the plan without its turns is the head of the table
            assert np.array_equal(df.pack_table(opened), t[:df._table_words(B, NT, True, True)])
    with pytest.raises(ValueError, match="both columns"):
        plain._replace(on=np.zeros_like(plain.utt))


def test_feed_reads_turns_from_the_planner(golden):
    """The host half only: ``DynamicMixFeed`` needs a device corpus, so the flag is read the way the feed reads it."""
    planner = functools.partial(df.plan_whamr, turns=df.Turns((0.2, 0.4), 8), speed_reverb=True)
    assert (getattr(planner, "keywords", None) or {}).get("turns") == df.Turns((0.2, 0.4), 8)
    import inspect
    assert inspect.signature(df.DynamicMixFeed.__init__).parameters["turns"].default is None
    for fn in (df.plan_wsj0, df.plan_wham, df.plan_whamr):
        assert inspect.signature(fn).parameters["turns"].default is None
    assert "turns" not in inspect.signature(df.plan_direct).parameters
    for fn in (df.table_layout, df.collate_plan):
        assert inspect.signature(fn).parameters["turns"].default is False
