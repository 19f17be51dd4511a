"""Speed perturbation and reverberation of one source in the dynamic-mixing feed, without a device: the planners
with ``speed_reverb=True`` replayed draw by draw, ``collate_plan``'s checks with and without the flag, the table layout, the numpy
restatement (tests/dynmix_speed_reverb_ref.py) against ``np.convolve`` of the whole converted utterance, and the argument checks of
``sepr_dynmix_speed_reverb_fwd``."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_reverb_ref as rr                                               # noqa: E402
import dynmix_speed_ref as sr                                                # noqa: E402
import dynmix_speed_reverb_ref as ref                                        # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

PLANNERS = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr}
SPEEDS = list(range(95, 106))


def host_corpus(g, without=()):
    arrays, roles = dr.fixture_corpus(g)
    arrays = {nm: a for nm, a in arrays.items() if nm.split("/")[0] not in without}
    c = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    c.roles = {r: k for r, k in roles.items() if r not in without}
    c.set_energies(np.array([dr.energy(arrays[nm]) for nm in c.names], dtype=np.int64), np.zeros(0))
    return c, [arrays[nm] for nm in c.names]


def host_bank(seed=3, lengths=(1, 2, 300, 1025, 2500)):
    rng = np.random.default_rng(seed)
    hs = [np.ones(1, np.float32) if n == 1 else rng.normal(0, 0.3, size=n).astype(np.float32) for n in lengths]
    return rv.RirBank.from_arrays(hs, 8000, device=None, normalise=None), hs


def replay(tag, corpus, rng, key, max_len, R):
    """The planners' draw sequence by hand: after the draw that orders the sources one choice(SPEEDS) per source, then one randrange(R) per
    source; every later draw on the PERTURBED lengths (the noise at 100 %).
    -> (utterances of the mixture terms, speeds, RIR indices of the two sources, gains, starts, n)."""
    keys = corpus.roles["s1"]
    if tag == "wsj0":
        while True:
            kr = rng.choice(keys)
            if df.wsj0_distinct_speakers(key, kr):
                break
    else:
        kr = rng.choice(keys)
    i1, i2 = (0, 1) if rng.random() > 0.5 else (1, 0)
    sp = [rng.choice(SPEEDS), rng.choice(SPEEDS)]
    rs = [rng.randrange(R), rng.randrange(R)]
    srcs = ("s1", "s2")
    utts = [corpus.lookup(srcs[i1], key), corpus.lookup(srcs[i2], kr)]
    lens = [sr.perturbed_len(int(corpus.lengths[u]), p) for u, p in zip(utts, sp)]
    if tag == "wsj0":
        gains = [np.float32(pow(10, -rng.uniform(-5, 5) / 20)) for _ in range(2)]
        mn = min(lens)
        starts = [rng.randint(0, ln - mn) for ln in lens]
        n = mn - mn % 4
        if n > max_len:
            st = rng.randint(0, n - max_len)
            starts, n = [s + st for s in starts], max_len
    else:
        if tag == "wham":
            gains = [np.float32(pow(10, -rng.uniform(-5, 5) / 20)) for _ in range(3)]
        else:
            gains = [np.float32(pow(10, -rng.uniform(-3, 3) / 20)) for _ in range(2)] + [np.float32(pow(10, -rng.uniform(-6, 3) / 20))]
        utts.append(corpus.lookup("noise", key))
        lens.append(int(corpus.lengths[utts[2]]))
        mn = min([max_len] + lens)
        starts = [rng.randint(0, ln - mn) for ln in lens]
        n = mn - mn % 4
    return utts, sp, rs, gains, starts, n


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr"])
def test_planners_with_speeds_and_rirs(golden, tag):
    g = golden("dynmix")
    corpus, _ = host_corpus(g, without=("s1_reverb", "s2_reverb"))            # plan_whamr never looks the twins up
    assert "s1_reverb" not in corpus.roles
    bank, hs = host_bank()
    keys = [str(k) for k in g["keys"]]
    max_len = int(g["max_len"])
    planner = PLANNERS[tag]
    direct = bank.direct_taps()
    r1, r2 = random.Random(13), random.Random(13)
    seen_r, seen_p = set(), set()
    for rounds in range(8):
        for k in keys:
            e = planner(corpus, r1, k, max_len, speeds=SPEEDS, rirs=bank, speed_reverb=True)
            utts, sp, rs, gains, starts, n = replay(tag, corpus, r2, k, max_len, len(bank))
            assert r1.getstate() == r2.getstate(), (tag, k)                  # after EVERY example
            assert e.n == n and len(e.mix) == len(utts) and len(e.tgt) == 2
            assert all(len(t) == 7 for t in e.mix + e.tgt)
            rms = corpus.rms
            for j, t in enumerate(e.mix):
                assert t[:2] == (utts[j], starts[j]) and t[3] == gains[j] and t[2] == np.float32(rms[utts[0]]) / np.float32(rms[utts[j]])
                assert t[4:] == ((sp[j], rs[j], len(hs[rs[j]])) if j < 2 else (100, -1, 1))      # the noise: neither perturbed nor reverberated
                assert t[1] + n <= sr.perturbed_len(int(corpus.lengths[t[0]]), t[4])
            for j, t in enumerate(e.tgt):
                assert t[:5] == e.mix[j][:5] and t[5:] == (rs[j], int(direct[rs[j]]))          # "direct" is the default, at the same speed
            seen_r |= set(rs)
            seen_p |= set(sp)
    assert seen_r == set(range(len(bank))) and seen_p == set(SPEEDS)
    # the four kinds of target, each at the mixture term's speed
    for target, want in (("direct", lambda r: (r, int(direct[r]))), ("dry", lambda r: (-1, 1)), ("full", lambda r: (r, len(hs[r]))),
                         (700, lambda r: (r, min(700, len(hs[r]))))):
        e = planner(corpus, random.Random(2), keys[1], max_len, speeds=SPEEDS, rirs=bank, speed_reverb=True, target=target)
        base = planner(corpus, random.Random(2), keys[1], max_len, speeds=SPEEDS, rirs=bank, speed_reverb=True)
        assert e.mix == base.mix
        for m, t in zip(e.mix, e.tgt):
            assert t[:5] == m[:5] and t[5:] == want(m[5]), target
        if target == "full":
            assert e.tgt == e.mix[:2]
    # without the keyword the refusal stays; the keyword with one of the two alone changes nothing
    with pytest.raises(ValueError, match="speeds and rirs"):
        planner(corpus, random.Random(2), keys[1], max_len, rirs=bank, speeds=SPEEDS)
    full, _ = host_corpus(g)                                                  # plan_whamr without rirs reads the twins
    for kw in (dict(speeds=SPEEDS), dict(rirs=bank), dict()):
        assert planner(full, random.Random(4), keys[0], max_len, speed_reverb=True, **kw) == planner(full, random.Random(4), keys[0], max_len, **kw)
    for kw in (dict(speeds=SPEEDS), dict(rirs=bank)):
        with pytest.raises(ValueError):
            df.plan_direct(corpus, random.Random(0), keys[0], max_len, **kw)
    assert "speed_reverb" not in df.plan_direct.__code__.co_varnames
    # every batch passes collate_plan with the flag and carries all three columns
    egs = [planner(corpus, r1, k, max_len, speeds=SPEEDS, rirs=bank, speed_reverb=True) for k in keys]
    plan = df.collate_plan(corpus, egs, rirs=bank, speed_reverb=True)
    assert plan.speed is not None and plan.rir is not None and plan.taps is not None
    assert plan.speed.dtype == plan.rir.dtype == plan.taps.dtype == np.int32 and plan.speed.shape == plan.rir.shape == plan.taps.shape == plan.utt.shape
    if any(t[4] != 100 for e in egs for t in e.mix):
        with pytest.raises(ValueError, match="speeds and RIRs"):
            df.collate_plan(corpus, egs, rirs=bank)


def test_collate_and_table_layout(golden):
    g = golden("dynmix")
    corpus, _ = host_corpus(g, without=("s1_reverb", "s2_reverb"))
    bank, hs = host_bank()
    keys = [str(k) for k in g["keys"]]
    rng = random.Random(11)
    egs = [df.plan_whamr(corpus, rng, k, 3000, speeds=[95, 105, 97], rirs=bank, speed_reverb=True, target=("direct", "dry", "full", 5)[i])
           for i, k in enumerate(keys)]
    plan = df.collate_plan(corpus, egs, rirs=bank, speed_reverb=True)
    B, NT = plan.utt.shape
    assert (B, NT, plan.M, plan.S) == (4, 5, 3, 2)
    order = [95, 97, 105]
    assert df.plan_speeds(plan) == sorted({int(p) for p in plan.speed.ravel()} - {100}) and set(df.plan_speeds(plan)) <= set(order)
    plain = df.pack_table(plan._replace(speed=None, rir=None, taps=None))
    t = df.pack_table(plan, order)
    layout = df.table_layout(B, NT, speeds=True, rirs=True)
    assert list(layout) == ["utt", "start", "norm", "gain", "n", "conv", "rir", "taps"]
    assert t.dtype == np.int32 and t.shape == (df._table_words(B, NT, True, True),) == (7 * B * NT + B,)
    assert plain.size == 4 * B * NT + B and np.array_equal(t[:plain.size], plain)                       # the plain table, then conv | rir | taps
    at = lambda name: t[layout[name][0]:layout[name][0] + layout[name][1]].reshape(B, NT)          # noqa: E731
    assert np.array_equal(at("conv"), np.vectorize(lambda p: -1 if p == 100 else order.index(p))(plan.speed))
    assert np.array_equal(at("rir"), plan.rir) and np.array_equal(at("taps"), plan.taps)
    assert (plan.speed[:, 2] == 100).all() and (plan.rir[:, 2] == -1).all() and (plan.speed[:, :2] != 100).all() and (plan.rir[:, :2] >= 0).all()
    assert np.array_equal(plan.speed[:, 3:], plan.speed[:, :2])
    by_key = {e.key: e for e in egs}
    for b, k in enumerate(plan.keys):
        for j, term in enumerate(by_key[k].mix + by_key[k].tgt):
            assert (plan.speed[b, j], plan.rir[b, j], plan.taps[b, j]) == term[4:]
    # all speeds 100 under the flag: still the three columns (one layout per feed)
    same = df.collate_plan(corpus, [df.plan_whamr(corpus, random.Random(1), k, 3000, speeds=[100], rirs=bank, speed_reverb=True) for k in keys],
                           rirs=bank, speed_reverb=True)
    assert same.speed is not None and (same.speed == 100).all() and same.rir is not None
    # without responses the flag changes nothing
    sp_only = [df.plan_whamr(*a, speeds=[95, 105]) for a in [(host_corpus(g)[0], random.Random(3), k, 3000) for k in keys]]
    full = host_corpus(g)[0]
    assert df.collate_plan(full, sp_only, speed_reverb=True).rir is None
    # validation
    e = egs[0]
    u, s, nf, gn, p, r, k = e.mix[0]
    assert p != 100
    T, Lr = int(corpus.lengths[u]), len(hs[r])
    P = sr.perturbed_len(T, p)

    def with_term(term, n=None):
        return e._replace(mix=(term,) + e.mix[1:], n=e.n if n is None else n)

    df.collate_plan(corpus, [with_term((u, s, nf, gn, p, r, Lr))], rirs=bank, speed_reverb=True)
    df.collate_plan(corpus, [with_term((u, P - e.n, nf, gn, p, r, 1))], rirs=bank, speed_reverb=True)       # ends exactly at the perturbed length
    with pytest.raises(ValueError, match="speed"):
        df.collate_plan(corpus, [with_term((u, P - e.n + 1, nf, gn, p, r, 1))], rirs=bank, speed_reverb=True)
    with pytest.raises(ValueError):
        df.collate_plan(corpus, [with_term((u, s, nf, gn, 0, r, 1))], rirs=bank, speed_reverb=True)
    for bad in ((len(bank), 1), (-2, 1), (r, 0), (r, Lr + 1), (r, -1)):
        with pytest.raises(ValueError, match="RIR"):
            df.collate_plan(corpus, [with_term((u, s, nf, gn, p) + bad)], rirs=bank, speed_reverb=True)
    with pytest.raises(ValueError, match="no bank"):
        df.collate_plan(corpus, egs, speed_reverb=True)
    with pytest.raises(ValueError, match="speeds and RIRs"):
        df.collate_plan(corpus, egs, rirs=bank)
    with pytest.raises(ValueError, match="converter set"):
        df.pack_table(plan, [95, 105] if 97 in plan.speed else [95])


def small_utts():
    rng = np.random.default_rng(5)
    return [rng.integers(-20000, 20000, size=3100, dtype=np.int16), rng.normal(0, 0.1, size=2999).astype(np.float32),
            rng.integers(-20000, 20000, size=37, dtype=np.int16), rng.normal(0, 0.1, size=37).astype(np.float32)]


def test_restatement_against_np_convolve_of_the_converted_utterance():
    """The float64 sums of the restatement's second stage, before the rounding, against ``np.convolve`` in float64 of the WHOLE converted
    utterance truncated to P.  Bound per sample, as in section 5e-3: each of the two is a sum of ``taps`` exact products with at most
    ``taps - 1`` rounded additions, so their difference is within ``taps 2^-52 sum_j |h_j| |y_{t-j}|`` - derived, not measured."""
    utts = small_utts()
    _, hs = host_bank()
    for u, x in enumerate(utts):
        for p in (90, 95, 105, 110):
            y = ref.perturbed(utts, u, p)
            P = sr.perturbed_len(x.shape[0], p)
            assert y.dtype == np.float32 and y.shape == (P,) and np.array_equal(y, sr.convert(dr.values(x), p))
            for h in hs:
                taps = h.shape[0]
                got = rr.conv64(y, h, 0, P, taps)
                want = np.convolve(y.astype(np.float64), h.astype(np.float64))[:P]
                bound = taps * 2.0 ** -52 * np.convolve(np.abs(y).astype(np.float64), np.abs(h).astype(np.float64))[:P]
                assert (np.abs(got - want) <= bound).all(), (u, p, taps, float(np.max(np.abs(got - want) - bound)))
                assert np.max(np.abs(got)) > 0


def test_restatement_consequences():
    """The term is "convert whole, convolve, truncate to P, crop"; p = 100 is the reverberant term, rir = -1 the speed term, both the plain
    term, the unit impulse the speed term; y is ZERO before sample 0 (the first output under a long response is h[0] y[0] alone)."""
    utts = small_utts()
    _, hs = host_bank()
    nf, gn = np.float32(1.7), np.float32(0.6)
    for u, x in enumerate(utts):
        for p in (95, 104):
            y = ref.perturbed(utts, u, p)
            P = y.shape[0]
            n = min(P - P % 4, 1500) if P > 100 else 4
            for r in (2, 4):
                h = hs[r]
                whole = rr.conv64(y, h, 0, P, h.shape[0]).astype(np.float32)
                wet = list(utts)
                wet[u] = whole
                for start in sorted({0, 1, P - n}):
                    got = ref.term(utts, hs, u, start, nf, gn, n, p, r, h.shape[0])
                    assert got.dtype == np.float32 and np.array_equal(got, dr.term(wet, u, start, nf, gn, n)), (u, p, r, start)
                first = ref.term(utts, hs, u, 0, np.float32(1), np.float32(1), 4, p, r, h.shape[0])[0]
                assert first == np.float32(np.float64(h[0]) * np.float64(y[0]))
            for start in (0, 1, P - n):
                sp = sr.term(utts, u, start, nf, gn, n, p)
                assert np.array_equal(ref.term(utts, hs, u, start, nf, gn, n, p, -1, 1), sp)
                assert np.array_equal(ref.term(utts, hs, u, start, nf, gn, n, p, 0, 1), sp)            # h = [1.0]
        T = x.shape[0]
        n = min(T - T % 4, 1500) if T > 100 else 4
        assert np.array_equal(ref.term(utts, hs, u, 1, nf, gn, n, 100, 3, 1025), rr.term(utts, hs, u, 1, nf, gn, n, 3, 1025))
        assert np.array_equal(ref.term(utts, hs, u, 1, nf, gn, n, 100, -1, 1), dr.term(utts, u, 1, nf, gn, n))


def test_c_abi_argument_checks():
    """Every check of ``sepr_dynmix_speed_reverb_fwd`` comes before any HIP call: testable without a device.  One bad argument at a time;
    the good call is never made (it would launch)."""
    lib = L_.load()
    p = 0x1000                                                               # never dereferenced: the checks reject the call first
    rows2, rows3 = (C.c_void_p * 2)(p, p), (C.c_void_p * 3)(p, p, p)
    E = L_.SEPR_EINVAL

    def conv(L=(20, 20), M=(19, 21), K=(138, 132), taps=(p, p)):
        return dict(taps=(C.c_void_p * len(taps))(*taps), cl=(C.c_int * len(L))(*L), cm=(C.c_int * len(M))(*M), ck=(C.c_int * len(K))(*K), NC=len(L))

    def mix(buf16=p, t16=100, buf32=None, t32=0, off=p, n16=3, N=3, tu=p, ts=p, tn=p, tg=p, tc=p, tr=p, tt=p, n=p, B=2, M=2, S=2, T=64, out=p,
            rows=rows2, taps=None, cl=None, cm=None, ck=None, NC=0, rir=p, rtot=10, roff=p, R=2):
        return lib.sepr_dynmix_speed_reverb_fwd(buf16, t16, buf32, t32, off, n16, N, tu, ts, tn, tg, tc, tr, tt, n, B, M, S, T, out, rows, taps, cl, cm,
                                                ck, NC, rir, rtot, roff, R, None)

    # the checks of sepr_dynmix_fwd, without and with converters
    for kw in (dict(off=None), dict(tu=None), dict(ts=None), dict(tn=None), dict(tg=None), dict(n=None), dict(out=None), dict(rows=None),
               dict(rows=(C.c_void_p * 2)(p, None)), dict(buf16=None), dict(B=0), dict(B=-1), dict(B=65536), dict(S=1), dict(S=4, rows=rows3),
               dict(M=1), dict(M=4), dict(S=3, M=2, rows=rows3), dict(S=3, M=5, rows=rows3), dict(T=0), dict(T=62), dict(T=66),
               dict(out=p + 4), dict(buf16=p + 2), dict(N=0, n16=0), dict(n16=4), dict(N=4), dict(t16=0), dict(t16=-1), dict(t32=-1),
               dict(n16=2, buf32=None, t32=5), dict(n16=2, buf32=p, t32=0), dict(n16=2, buf32=p + 4, t32=5),
               dict(rows=(C.c_void_p * 2)(p, p + 8))):
        assert mix(**kw) == E, kw
        assert mix(**kw, **conv()) == E, kw
    # those of sepr_dynmix_speed_fwd
    assert mix(tc=None) == E and mix(tc=None, **conv()) == E
    assert mix(NC=-1) == E and mix(NC=17) == E
    assert mix(**conv(L=(20,) * 17, M=(19,) * 17, K=(138,) * 17, taps=(p,) * 17)) == E
    good = conv()
    for name in ("taps", "cl", "cm", "ck"):
        assert mix(**{**good, name: None}) == E, name
    for kw in (dict(taps=(p, None)), dict(taps=(None, p)), dict(L=(20, 0)), dict(L=(-1, 20)), dict(M=(0, 21)), dict(M=(19, -3)), dict(K=(138, 0)),
               dict(K=(-2, 132)), dict(K=(137, 132)), dict(K=(138, 133))):
        assert mix(**conv(**kw)) == E, kw
    # a converter the kernel cannot stage: its 2048-output span (2047 M / L + K + 1 samples) exceeds 3072
    assert mix(**conv(L=(20, 2), M=(19, 3), K=(138, 194))) == E
    assert mix(**conv(L=(20, 1), M=(19, 2), K=(138, 258))) == E
    assert mix(**conv(L=(20, 20), M=(19, 21), K=(138, 924))) == E
    # those of sepr_dynmix_reverb_fwd, without and with converters
    for kw in (dict(tr=None), dict(tt=None), dict(rir=None), dict(roff=None), dict(R=0), dict(R=-1), dict(rtot=0), dict(rtot=-5),
               dict(rir=p + 2), dict(rir=p + 1), dict(rir=p + 3)):
        assert mix(**kw) == E, kw
        assert mix(**kw, **conv()) == E, kw
