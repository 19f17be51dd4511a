"""Speed perturbation in the dynamic-mixing feed, without a device: the converters' geometry, the planners
with ``speeds=``, the table layout, the numpy restatement (tests/dynmix_speed_ref.py) against the composition "convert the whole
utterance, then mix plainly", and the argument checks of ``sepr_dynmix_speed_fwd``."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_speed_ref as ref                                               # noqa: E402
import resample_ref as rr                                                    # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402

SPEEDS = range(95, 106)
PLANNERS = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr}


def host_corpus(g):
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    c.roles = roles
    c.set_energies(np.array([dr.energy(arrays[nm]) for nm in c.names], dtype=np.int64), np.zeros(0))
    return c, [arrays[nm] for nm in c.names]


def test_converter_geometry():
    """``resample.plan(p, 100)`` is the restatement's converter for p in 90..110; K runs from 130 to 144; the issue's example lengths;
    the eleven device tables of 95..105 total about 330 KB."""
    ks = []
    for p in range(90, 111):
        pl = rs.plan(p, 100)
        L, M, K, Hh, _ = rr.geometry(p, 100)
        assert (pl.L, pl.M, pl.K, pl.Hh) == (L, M, K, Hh) and K == 2 * Hh + 2
        assert (L, M) == df.speed_ratio(p) and L * p == M * 100
        assert np.array_equal(pl.taps, rr.taps(p, 100))
        assert rs.device_table(pl).shape == (K, L)
        ks.append(K)
    assert min(ks) == 130 and max(ks) == 144
    assert df.perturbed_len(32000, 95) == 33685 and df.perturbed_len(32000, 105) == 30477 and df.perturbed_len(32000, 100) == 32000
    total = sum(rs.device_table(rs.plan(p, 100)).nbytes for p in SPEEDS)
    assert total == sum(4 * rr.geometry(p, 100)[0] * rr.geometry(p, 100)[2] for p in SPEEDS) == 311760      # "about 330 KB": 6 % under
    assert abs(total - 330e3) < 0.1 * 330e3


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr"])
def test_planners_with_speeds(golden, tag):
    g = golden("dynmix")
    corpus, _ = host_corpus(g)
    keys = [str(k) for k in g["keys"]]
    max_len = int(g["max_len"])

    def run(seed, speeds, rounds=6):
        rng = random.Random(seed)
        return [PLANNERS[tag](corpus, rng, k, max_len, speeds=speeds) for _ in range(rounds) for k in keys], rng.getstate()

    a, sa = run(4, SPEEDS)
    b, sb = run(4, SPEEDS)
    assert a == b and sa == sb                                               # the same seed, the same examples and the same draws
    assert run(4, list(SPEEDS))[0] == a                                      # a range and a list draw alike
    noise = {corpus.lookup("noise", k) for k in keys}
    seen = set()
    for e in a:
        assert all(len(t) == 5 for t in e.mix + e.tgt) and e.n % 4 == 0 and 0 < e.n <= max_len
        for u, s, nf, gn, p in e.mix + e.tgt:
            N = ref.perturbed_len(int(corpus.lengths[u]), p)
            assert 0 <= s and s + e.n <= N, (e.key, u, s, e.n, p, N)
            assert p == 100 if u in noise else p in SPEEDS
            seen.add(p)
        r = corpus.rms                                                       # the norm factors keep the STORED utterances' RMS
        assert e.tgt[0][2] == np.float32(1.0) and e.tgt[1][2] == np.float32(r[e.tgt[0][0]]) / np.float32(r[e.tgt[1][0]])
        if tag == "whamr":                                                   # a dry source and its reverberant twin share speed, start, norm, gain
            for wet, dry in zip(e.mix[:2], e.tgt):
                assert wet[1:] == dry[1:] and corpus.lengths[wet[0]] == corpus.lengths[dry[0]] and wet[0] != dry[0]
            assert e.mix[2][0] in noise and e.mix[2][4] == 100
        else:
            assert e.tgt == e.mix[:2]
            if tag == "wham":
                assert e.mix[2][0] in noise and e.mix[2][4] == 100
    assert len(seen - {100}) > 1
    # an uncropped example takes the whole of its shortest perturbed source: the perturbed lengths are out_len
    whole = PLANNERS[tag](corpus, random.Random(1), keys[0], 10 ** 6, speeds=[95])
    lens = [ref.perturbed_len(int(corpus.lengths[t[0]]), t[4]) for t in whole.mix]
    assert lens[0] == rr.out_len(int(corpus.lengths[whole.mix[0][0]]), 20, 19) and whole.n == min(lens) - min(lens) % 4
    for i in range(0, len(a), len(keys)):                                    # every batch passes collate_plan and carries the speeds
        plan = df.collate_plan(corpus, a[i:i + len(keys)])
        assert plan.speed is not None and plan.speed.dtype == np.int32 and plan.speed.shape == plan.utt.shape
        assert set(plan.speed.ravel().tolist()) <= set(SPEEDS) | {100}
    # speeds=[100]: the draws are made, nothing is perturbed - the examples of the plain planner after two more draws per example
    e100 = PLANNERS[tag](corpus, random.Random(2), keys[1], max_len, speeds=[100])
    assert all(t[4] == 100 for t in e100.mix + e100.tgt)


def test_without_speeds_nothing_changes(golden):
    """``speeds=None``: four-field terms, no ``speed`` in the plan, today's table layout - and ``plan_direct`` refuses speeds."""
    g = golden("dynmix")
    corpus, _ = host_corpus(g)
    keys = [str(k) for k in g["keys"]]
    for tag, planner in PLANNERS.items():
        r1, r2 = random.Random(8), random.Random(8)
        e1 = [planner(corpus, r1, k, 3000) for k in keys]
        e2 = [planner(corpus, r2, k, 3000, speeds=None) for k in keys]
        assert e1 == e2 and r1.getstate() == r2.getstate() and all(len(t) == 4 for e in e1 for t in e.mix + e.tgt)
        plan = df.collate_plan(corpus, e1)
        assert plan.speed is None
        B, NT = plan.utt.shape
        t = df.pack_table(plan)
        assert t.dtype == np.int32 and t.shape == (4 * B * NT + B,) == (df._table_words(B, NT),)
        want = np.concatenate([plan.utt.ravel(), plan.start.ravel(), plan.norm.ravel().view(np.int32), plan.gain.ravel().view(np.int32), plan.n])
        assert np.array_equal(t, want)
    with pytest.raises(ValueError, match="speeds"):
        df.plan_direct(corpus, random.Random(0), keys[0], 3000, speeds=SPEEDS)
    assert len(df.plan_direct(corpus, random.Random(0), keys[0], 3000).mix[0]) == 4


def test_parse_speeds():
    assert df.parse_speeds("95:105") == list(SPEEDS) and df.parse_speeds("95,100, 105") == [95, 100, 105] and df.parse_speeds("97") == [97]
    for bad in ("", "105:95", "0:3", "-5,100"):
        with pytest.raises(ValueError):
            df.parse_speeds(bad)


def test_table_layout_with_speeds(golden):
    g = golden("dynmix")
    corpus, _ = host_corpus(g)
    keys = [str(k) for k in g["keys"]]
    rng = random.Random(11)
    plan = df.collate_plan(corpus, [df.plan_whamr(corpus, rng, k, 3000, speeds=SPEEDS) for k in keys])
    B, NT = plan.utt.shape
    plain = df.pack_table(plan._replace(speed=None))
    own = df.plan_speeds(plan)
    assert own == sorted(set(plan.speed.ravel().tolist()) - {100}) and len(own) >= 2
    for order in (None, list(SPEEDS), [105, 100] + own[::-1]):
        t = df.pack_table(plan, order)
        assert t.dtype == np.int32 and t.shape == (df._table_words(B, NT, True),) == (5 * B * NT + B,)
        assert np.array_equal(t[:plain.size], plain)
        conv = t[plain.size:].reshape(B, NT)
        used = own if order is None else order
        for p, k in zip(plan.speed.ravel(), conv.ravel()):
            assert (k == -1) if p == 100 else (0 <= k < len(used) and used[k] == p)
    assert (conv[:, 2] == -1).all()                                          # the noise term
    with pytest.raises(ValueError, match="converter set"):
        df.pack_table(plan, [own[0]])
    # collate_plan validates against the PERTURBED length
    e = df.plan_wsj0(corpus, random.Random(0), keys[0], 10 ** 6, speeds=[105])
    u, s, nf, gn, p = e.mix[0]
    N = ref.perturbed_len(int(corpus.lengths[u]), 105)
    ok = e._replace(n=4, mix=((u, N - 4, nf, gn, p),) + e.mix[1:])
    df.collate_plan(corpus, [ok])
    with pytest.raises(ValueError, match="reads"):
        df.collate_plan(corpus, [ok._replace(mix=((u, N - 3, nf, gn, p),) + e.mix[1:])])
    assert N < int(corpus.lengths[u])                                        # ... which the stored length would have let through


def test_restatement_is_the_composition():
    """A perturbed term of the restatement equals ``dynmix_ref.term`` over the whole utterance converted to float32 first, bit for bit
    (int16 and float32 storage; the 40-sample utterance, whose whole filter overhangs both ends), and the sequential float64 sum rounds
    like ``resample_ref.resample``'s on these inputs."""
    rng = np.random.default_rng(5)
    utts = [rng.integers(-20000, 20000, size=900, dtype=np.int16), rng.normal(0, 0.1, size=1031).astype(np.float32),
            rng.integers(-20000, 20000, size=40, dtype=np.int16)]
    for p in (95, 97, 100, 103, 105):
        whole = [ref.convert(dr.values(x), p) for x in utts]
        for u, x in enumerate(utts):
            N = ref.perturbed_len(x.shape[0], p)
            assert whole[u].shape == (N,) and whole[u].dtype == np.float32
            if p != 100:
                assert np.array_equal(whole[u], rr.resample(dr.values(x), p, 100).astype(np.float32))
            else:
                assert np.array_equal(whole[u], dr.values(x))
            for start, n in ((0, N), (N - 8, 8), (3, min(N - 3, 36))):
                nf, gn = np.float32(1.7), np.float32(0.6)
                assert np.array_equal(ref.term(utts, u, start, nf, gn, n, p), dr.term(whole, u, start, nf, gn, n))


def test_c_abi_argument_checks():
    """Every check of ``sepr_dynmix_speed_fwd`` comes before any HIP call: testable without a device."""
    lib = L_.load()
    p = 0x1000                                                               # never dereferenced: the checks reject the call first
    rows2, rows3 = (C.c_void_p * 2)(p, p), (C.c_void_p * 3)(p, p, p)
    E = L_.SEPR_EINVAL

    def conv(L=(20, 20), M=(19, 21), K=(138, 132), taps=(p, p)):
        return dict(taps=(C.c_void_p * len(taps))(*taps), cl=(C.c_int * len(L))(*L), cm=(C.c_int * len(M))(*M), ck=(C.c_int * len(K))(*K), NC=len(L))

    def mix(buf16=p, t16=100, buf32=None, t32=0, off=p, n16=3, N=3, tu=p, ts=p, tn=p, tg=p, tc=p, n=p, B=2, M=2, S=2, T=64, out=p, rows=rows2,
            taps=None, cl=None, cm=None, ck=None, NC=0):
        return lib.sepr_dynmix_speed_fwd(buf16, t16, buf32, t32, off, n16, N, tu, ts, tn, tg, tc, n, B, M, S, T, out, rows, taps, cl, cm, ck, NC, None)

    # the checks of sepr_dynmix_fwd
    for kw in (dict(off=None), dict(tu=None), dict(ts=None), dict(tn=None), dict(tg=None), dict(n=None), dict(out=None), dict(rows=None),
               dict(rows=(C.c_void_p * 2)(p, None)), dict(buf16=None), dict(B=0), dict(B=-1), dict(S=1), dict(S=4, rows=rows3),
               dict(M=1), dict(M=4), dict(S=3, M=2, rows=rows3), dict(S=3, M=5, rows=rows3), dict(T=0), dict(T=62), dict(T=66),
               dict(out=p + 4), dict(buf16=p + 2), dict(N=0, n16=0), dict(n16=4), dict(N=4), dict(t16=0)):
        assert mix(**kw) == E, kw
        assert mix(**kw, **conv()) == E, kw
    # its own
    assert mix(tc=None) == E and mix(tc=None, **conv()) == E
    assert mix(NC=-1) == E and mix(NC=17) == E
    many = conv(L=(20,) * 17, M=(19,) * 17, K=(138,) * 17, taps=(p,) * 17)
    assert mix(**many) == E
    good = conv()
    for name in ("taps", "cl", "cm", "ck"):
        assert mix(**{**good, name: None}) == E, name
    for kw in (dict(taps=(p, None)), dict(taps=(None, p)), dict(L=(20, 0)), dict(L=(-1, 20)), dict(M=(0, 21)), dict(M=(19, -3)), dict(K=(138, 0)),
               dict(K=(-2, 132)), dict(K=(137, 132)), dict(K=(138, 133))):
        assert mix(**conv(**kw)) == E, kw
    # a converter whose tile span (2047 M / L + K + 1 samples) does not fit the kernel's 3072 staged samples
    assert mix(**conv(L=(20, 2), M=(19, 3), K=(138, 194))) == E              # 150 %: 3070 + 195
    assert mix(**conv(L=(20, 1), M=(19, 2), K=(138, 258))) == E              # 200 %
    assert mix(**conv(L=(20, 20), M=(19, 21), K=(138, 924))) == E            # 2149 + 925 > 3072
