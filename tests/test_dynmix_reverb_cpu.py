"""Reverberation in the dynamic-mixing feed, without a device: the numpy restatement
(tests/dynmix_reverb_ref.py) against the composition "convolve the whole utterance, truncate, then mix plainly" and against
``np.convolve``, the planners with ``rirs=``, the table layout, ``RirBank``, ``synthetic_rirs`` and the argument checks of
``sepr_dynmix_reverb_fwd``."""
import ctypes as C
import math
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_reverb_ref as ref                                              # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

PLANNERS = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr}


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


def small_utts():
    rng = np.random.default_rng(5)
    return [rng.integers(-20000, 20000, size=3100, dtype=np.int16), rng.normal(0, 0.1, size=2999).astype(np.float32),
            rng.integers(-20000, 20000, size=37, dtype=np.int16), rng.normal(0, 0.1, size=37).astype(np.float32)]


def test_restatement_is_the_composition():
    """A reverberant term of the restatement equals ``dynmix_ref.term`` over the whole utterance convolved, truncated to its stored
    length and rounded to float32 first - bit for bit: int16 and float32 storage, starts 0, 1, mid and T - n, and the 37-sample
    utterances under a 2500-tap response."""
    utts = small_utts()
    _, hs = host_bank()
    nf, gn = np.float32(1.7), np.float32(0.6)
    for u, x in enumerate(utts):
        T = x.shape[0]
        for r, h in enumerate(hs):
            for taps in sorted({1, h.shape[0], (h.shape[0] + 1) // 2}):
                whole = ref.conv64(dr.values(x), h, 0, T, taps).astype(np.float32)
                assert whole.shape == (T,)
                wet = list(utts)
                wet[u] = whole
                n = min(T - T % 4, 1500) if T > 100 else 4
                for start in sorted({0, 1, (T - n) // 2 | 1 if T - n > 2 else 0, T - n}):
                    got = ref.term(utts, hs, u, start, nf, gn, n, r, taps)
                    assert got.dtype == np.float32 and np.array_equal(got, dr.term(wet, u, start, nf, gn, n)), (u, r, taps, start)
    # the tail of the samples before the crop is in the crop: the first output of a crop at `start` depends on x[start - 1]
    x = dr.values(utts[1])
    a = ref.conv64(x, hs[2], 500, 8, 300)
    x2 = x.copy()
    x2[499] += np.float32(0.5)
    assert ref.conv64(x2, hs[2], 500, 8, 300)[0] != a[0]


def test_restatement_against_np_convolve():
    """The float64 sums, before the rounding, against ``np.convolve`` in float64 (another summation order).  Bound, per sample: each of
    the two is a sum of ``taps`` exact products with at most ``taps - 1`` rounded additions, so each is within
    ``(taps - 1) 2^-53 sum_j |h_j| |x_{t-j}|`` of the true value to first order; their difference is within
    ``taps 2^-52 sum_j |h_j| |x_{t-j}|`` - derived, not measured."""
    utts = small_utts()
    _, hs = host_bank()
    for x in utts:
        xv = dr.values(x)
        T = xv.shape[0]
        for h in hs:
            taps = h.shape[0]
            got = ref.conv64(xv, h, 0, T, taps)
            want = np.convolve(xv.astype(np.float64), h.astype(np.float64))[:T]
            bound = taps * 2.0 ** -52 * np.convolve(np.abs(xv).astype(np.float64), np.abs(h).astype(np.float64))[:T]
            assert got.dtype == np.float64 and (np.abs(got - want) <= bound).all(), (T, taps, float(np.max(np.abs(got - want) - bound)))
            assert np.max(np.abs(got)) > 0


def test_unit_impulse_is_the_plain_term():
    utts = small_utts()
    one = [np.ones(1, np.float32), np.array([1.0, 0.5], np.float32)]
    for u, x in enumerate(utts):
        T = x.shape[0]
        n = T - T % 4 - 4
        for start in (0, 1, T - n):
            want = dr.term(utts, u, start, np.float32(1.3), np.float32(0.8), n)
            assert np.array_equal(ref.term(utts, one, u, start, np.float32(1.3), np.float32(0.8), n, 0, 1), want)
            assert np.array_equal(ref.term(utts, one, u, start, np.float32(1.3), np.float32(0.8), n, 1, 1), want)      # taps = 1 of [1, 0.5]
            assert np.array_equal(ref.term(utts, one, u, start, np.float32(1.3), np.float32(0.8), n, -1, 1), want)


def test_without_rirs_nothing_changes(golden):
    """``rirs=None``: today's Examples, today's generator state, today's table bytes; ``BatchPlan`` ends in two ``None`` fields."""
    g = golden("dynmix")
    corpus, _ = host_corpus(g)
    keys = [str(k) for k in g["keys"]]
    assert df.BatchPlan._fields[-2:] == ("rir", "taps") and df.BatchPlan._field_defaults["rir"] is None and df.BatchPlan._field_defaults["taps"] is None
    for tag, planner in PLANNERS.items():
        r1, r2 = random.Random(8), random.Random(8)
        e1 = [planner(corpus, r1, k, 3000) for k in keys]
        e2 = [planner(corpus, r2, k, 3000, rirs=None, target="full") for k in keys]
        assert e1 == e2 and r1.getstate() == r2.getstate() and all(len(t) == 4 for e in e1 for t in e.mix + e.tgt)
        p1, p2 = df.collate_plan(corpus, e1), df.collate_plan(corpus, e2, rirs=None)
        assert p1.rir is None and p1.taps is None and p1.speed is None
        B, NT = p1.utt.shape
        t = df.pack_table(p1)
        assert t.dtype == np.int32 and t.shape == (4 * B * NT + B,) == (df._table_words(B, NT),) and np.array_equal(t, df.pack_table(p2))
        want = np.concatenate([p1.utt.ravel(), p1.start.ravel(), p1.norm.ravel().view(np.int32), p1.gain.ravel().view(np.int32), p1.n])
        assert t.tobytes() == want.astype(np.int32).tobytes()
    bank, _ = host_bank()
    with pytest.raises(ValueError, match="rirs"):
        df.plan_direct(corpus, random.Random(0), keys[0], 3000, rirs=bank)
    assert len(df.plan_direct(corpus, random.Random(0), keys[0], 3000).mix[0]) == 4


def replay(tag, corpus, rng, key, max_len, R):
    """The planners' draw sequence by hand, with one randrange(R) per source directly after the draw that orders the sources.
    -> (utterances of the mixture terms, RIR indices of the two sources, gains, starts, n)."""
    keys = corpus.roles["s1"]
    if tag == "wsj0":
        while True:
            kr = rng.choice(keys)
            if df.wsj0_distinct_speakers(key, kr):
                break
    else:
        kr = rng.choice(keys)
    i1, i2 = (0, 1) if rng.random() > 0.5 else (1, 0)
    rs = [rng.randrange(R), rng.randrange(R)]
    srcs = ("s1", "s2")
    utts = [corpus.lookup(srcs[i1], key), corpus.lookup(srcs[i2], kr)]
    lens = [int(corpus.lengths[u]) for u in utts]
    if tag == "wsj0":
        gains = [np.float32(pow(10, -rng.uniform(-5, 5) / 20)) for _ in range(2)]
        mn = min(lens)
        starts = [rng.randint(0, ln - mn) for ln in lens]
        n = mn - mn % 4
        if n > max_len:
            st = rng.randint(0, n - max_len)
            starts, n = [s + st for s in starts], max_len
    elif tag == "wham":
        gains = [np.float32(pow(10, -rng.uniform(-5, 5) / 20)) for _ in range(3)]
        utts.append(corpus.lookup("noise", key))
        lens.append(int(corpus.lengths[utts[2]]))
        mn = min([max_len] + lens)
        starts = [rng.randint(0, ln - mn) for ln in lens]
        n = mn - mn % 4
    else:
        gains = [np.float32(pow(10, -rng.uniform(-3, 3) / 20)) for _ in range(2)] + [np.float32(pow(10, -rng.uniform(-6, 3) / 20))]
        utts.append(corpus.lookup("noise", key))
        lens.append(int(corpus.lengths[utts[2]]))
        mn = min([max_len] + lens)
        starts = [rng.randint(0, ln - mn) for ln in lens]
        n = mn - mn % 4
    return utts, rs, gains, starts, n


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr"])
def test_planners_with_rirs(golden, tag):
    g = golden("dynmix")
    corpus, _ = host_corpus(g, without=("s1_reverb", "s2_reverb"))            # plan_whamr(rirs=) never looks the twins up
    assert "s1_reverb" not in corpus.roles
    bank, hs = host_bank()
    keys = [str(k) for k in g["keys"]]
    max_len = int(g["max_len"])
    planner = PLANNERS[tag]
    direct = bank.direct_taps()
    r1, r2 = random.Random(13), random.Random(13)
    seen = set()
    for rounds in range(5):
        for k in keys:
            e = planner(corpus, r1, k, max_len, rirs=bank)
            utts, rs, gains, starts, n = replay(tag, corpus, r2, k, max_len, len(bank))
            assert r1.getstate() == r2.getstate(), (tag, k)                  # today's draws plus one randrange(R) per source, there
            assert e.n == n and len(e.mix) == len(utts) and len(e.tgt) == 2
            assert all(len(t) == 7 and t[4] == 100 for t in e.mix + e.tgt)
            rms = corpus.rms
            for j, t in enumerate(e.mix):
                assert t[:2] == (utts[j], starts[j]) and t[3] == gains[j] and t[2] == np.float32(rms[utts[0]]) / np.float32(rms[utts[j]])
                assert t[5:] == ((rs[j], len(hs[rs[j]])) if j < 2 else (-1, 1))                  # the noise is not reverberated
            for j, t in enumerate(e.tgt):
                assert t[:5] == e.mix[j][:5] and t[5:] == (rs[j], int(direct[rs[j]]))          # "direct" is the default
            seen |= set(rs)
    assert seen == set(range(len(bank)))
    # the four kinds of target
    for target, want in (("direct", lambda r: (r, int(direct[r]))), ("dry", lambda r: (-1, 1)), ("full", lambda r: (r, len(hs[r]))),
                         (700, lambda r: (r, min(700, len(hs[r])))), (1, lambda r: (r, 1))):
        e = planner(corpus, random.Random(2), keys[1], max_len, rirs=bank, target=target)
        base = planner(corpus, random.Random(2), keys[1], max_len, rirs=bank)
        assert e.mix == base.mix
        for m, t in zip(e.mix, e.tgt):
            assert t[:5] == m[:5] and t[5:] == want(m[5]), target
        if target == "full":
            assert e.tgt == e.mix[:2]
    for bad in ("wet", 0, -3, 1.5, True):
        with pytest.raises(ValueError, match="target"):
            planner(corpus, random.Random(2), keys[1], max_len, rirs=bank, target=bad)
    with pytest.raises(ValueError, match="speeds and rirs"):
        planner(corpus, random.Random(2), keys[1], max_len, rirs=bank, speeds=range(95, 106))
    # every batch passes collate_plan and carries the RIRs
    egs = [planner(corpus, r1, k, max_len, rirs=bank) for k in keys]
    plan = df.collate_plan(corpus, egs, rirs=bank)
    assert plan.speed is None and plan.rir.dtype == np.int32 and plan.taps.dtype == np.int32 and plan.rir.shape == plan.taps.shape == plan.utt.shape


def test_collate_and_table_layout(golden):
    g = golden("dynmix")
    corpus, _ = host_corpus(g, without=("s1_reverb", "s2_reverb"))
    bank, hs = host_bank()
    keys = [str(k) for k in g["keys"]]
    rng = random.Random(11)
    egs = [df.plan_whamr(corpus, rng, k, 3000, rirs=bank, target=("direct", "dry", "full", 5)[i]) for i, k in enumerate(keys)]
    plan = df.collate_plan(corpus, egs, rirs=bank)
    B, NT = plan.utt.shape
    assert (B, NT, plan.M, plan.S) == (4, 5, 3, 2)
    plain = df.pack_table(plan._replace(rir=None, taps=None))
    t = df.pack_table(plan)
    assert t.dtype == np.int32 and t.shape == (df._table_words(B, NT, False, True),) == (6 * B * NT + B,)
    assert np.array_equal(t[:plain.size], plain) and np.array_equal(t[plain.size - B:plain.size], plan.n)      # [.. | n | rir | taps]
    assert np.array_equal(t[plain.size:plain.size + B * NT].reshape(B, NT), plan.rir)
    assert np.array_equal(t[plain.size + B * NT:].reshape(B, NT), plan.taps)
    assert (plan.rir[:, 2] == -1).all() and (plan.rir[:, :2] >= 0).all()     # the noise term; the sources
    by_key = {e.key: e for e in egs}
    for b, k in enumerate(plan.keys):
        for j, term in enumerate(by_key[k].mix + by_key[k].tgt):
            assert (plan.rir[b, j], plan.taps[b, j]) == term[5:]
    assert (plan.rir[:, 3:] == -1).any() and np.array_equal(plan.taps[:, :2], np.array([[len(hs[r]) for r in row] for row in plan.rir[:, :2]]))
    # validation
    e = egs[0]
    u, s, nf, gn, p, r, k = e.mix[0]
    L = len(hs[r])

    def with_term(term):
        return e._replace(mix=(term,) + e.mix[1:])

    df.collate_plan(corpus, [with_term((u, s, nf, gn, p, r, L))], rirs=bank)
    df.collate_plan(corpus, [with_term((u, s, nf, gn, p, r, 1))], rirs=bank)
    for bad in ((len(bank), 1), (-2, 1), (r, 0), (r, L + 1), (r, -1)):
        with pytest.raises(ValueError, match="RIR"):
            df.collate_plan(corpus, [with_term((u, s, nf, gn, p) + bad)], rirs=bank)
    with pytest.raises(ValueError, match="no bank"):
        df.collate_plan(corpus, egs)
    with pytest.raises(ValueError, match="speeds and RIRs"):
        df.collate_plan(corpus, [with_term((u, 0, nf, gn, 95, r, L))], rirs=bank)


def test_rir_bank():
    h = [np.array([0.0, 0.5, -2.0, 2.0, 0.25], np.float64), np.array([-0.3], np.float32), np.array([0.1, 0.1, 0.05], np.float32)]
    bank = rv.RirBank.from_arrays(h, 8000)                                    # device=None, peak normalisation
    assert len(bank) == 3 and bank.device is None and bank.buf is None and bank.fs == 8000 and bank.names == ["0", "1", "2"]
    assert bank.lengths.dtype == np.int64 and bank.lengths.tolist() == [5, 1, 3] and bank.offsets_host.tolist() == [0, 5, 6, 9] and bank.total == 9
    assert bank.host.dtype == np.float32
    for r, a in enumerate(h):
        a64 = a.astype(np.float64)
        assert np.array_equal(bank.rir(r), (a64 / np.max(np.abs(a64))).astype(np.float32))
    assert np.array_equal(bank.rir(1), np.array([-1.0], np.float32))
    raw = rv.RirBank.from_arrays({"a": h[2], "b": h[1]}, 16000, normalise=None)
    assert np.array_equal(raw.rir(0), h[2]) and np.array_equal(raw.rir(1), h[1]) and raw.index == {"a": 0, "b": 1}
    # direct_taps: the FIRST maximum of |h| (index 2 of h[0], index 0 of h[2]), early_ms in samples, clipped to the length
    d = bank.direct_taps()
    assert d.dtype == np.int32 and d.tolist() == [3, 1, 1]
    assert bank.direct_taps(0.125).tolist() == [4, 1, 2]                      # 0.125 ms at 8 kHz = 1 sample
    assert bank.direct_taps(0.25).tolist() == [5, 1, 3] and bank.direct_taps(50.0).tolist() == [5, 1, 3]
    assert raw.direct_taps(0.125).tolist() == [3, 1]                          # 2 samples at 16 kHz
    # refusals
    long = np.zeros(16385, np.float32)
    long[0] = 1.0
    for bad in ([], [np.zeros(0, np.float32)], [np.zeros(7, np.float32)], [np.array([1.0, np.nan], np.float32)], [np.array([np.inf], np.float32)],
                [long], [np.ones((2, 2), np.float32)], [np.array([1, 2], np.int16)]):
        for norm in ("peak", None):
            with pytest.raises(ValueError):
                rv.RirBank.from_arrays(bad, 8000, normalise=norm)
    assert len(rv.RirBank.from_arrays([long[:16384]], 8000)) == 1
    with pytest.raises(ValueError):
        rv.RirBank.from_arrays(h, 8000, normalise="energy")
    with pytest.raises(ValueError, match="duplicate"):
        rv.RirBank(["a", "a"], [h[1], h[1]], 8000)


def test_rir_bank_from_scp(tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(0)
    a = (rng.normal(0, 3000, size=400)).astype(np.int16)
    a[7] = 20000
    wavfile.write(str(tmp_path / "a.wav"), 8000, a)
    wavfile.write(str(tmp_path / "b.wav"), 16000, a)
    scp = tmp_path / "rirs.scp"
    scp.write_text(f"ra {tmp_path / 'a.wav'}\n")
    bank = rv.RirBank.from_scp(str(scp), 8000)
    assert bank.names == ["ra"] and bank.lengths.tolist() == [400] and bank.direct_taps().tolist() == [8]
    assert np.array_equal(bank.rir(0), (a.astype(np.float64) / 20000.0).astype(np.float32))
    scp.write_text(f"ra {tmp_path / 'a.wav'}\nrb {tmp_path / 'b.wav'}\n")
    with pytest.raises(RuntimeError, match="resample=True"):
        rv.RirBank.from_scp(str(scp), 8000)


def test_synthetic_rirs():
    fs = 8000
    a = rv.synthetic_rirs(6, fs, seed=4)
    b = rv.synthetic_rirs(6, fs, seed=4)
    c = rv.synthetic_rirs(6, fs, seed=5)
    assert len(a) == 6 and all(x.dtype == np.float32 and x.ndim == 1 for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x[:100], y[:100]) for x, y in zip(a, c))
    for h in a:                                                              # rt60 in [0.2, 0.8] s, d in [0, 40]
        d = int(np.argmax(np.abs(h)))
        assert 0 <= d <= 40 and 1600 <= h.shape[0] - d <= 6400
    for rt, drr in ((0.3, 5.0), (0.25, 0.0), (3.0, 10.0)):
        hs = rv.synthetic_rirs(4, fs, rt60=rt, drr_db=drr, seed=1)
        for h in hs:
            d = int(np.argmax(np.abs(h)))
            assert 0 <= d <= int(0.005 * fs) and h.shape[0] == min(16384, d + math.ceil(rt * fs))                # the length formula
            assert h[d] == 1.0 and not h[:d].any() and (np.abs(np.delete(h, d)) < 1.0).all()                     # the strict maximum
            j = np.arange(1, h.shape[0] - d, dtype=np.float64)
            env = 10.0 ** (-3.0 * j / (rt * fs))
            sigma = math.sqrt(10.0 ** (-drr / 10.0) / float(np.sum(env * env)))
            assert (np.abs(h[d + 1:].astype(np.float64)) <= 6.0 * sigma * env * (1 + 2.0 ** -23)).all()           # within 6x the envelope
            assert np.abs(h[d + 1:]).max() > 0
    assert rv.RirBank.from_arrays(a, fs).direct_taps().tolist() == [int(np.argmax(np.abs(h))) + 1 for h in a]
    assert rv.parse_synthetic("8:0.2:0.6") == (8, 0.2, 0.6) and rv.parse_synthetic("3:0.5") == (3, 0.5, 0.5)
    for bad in ("8", "0:0.2:0.3", "4:0.5:0.2", "4:0:1", "1:2:3:4"):
        with pytest.raises(ValueError):
            rv.parse_synthetic(bad)


def test_c_abi_argument_checks():
    """Every check of ``sepr_dynmix_reverb_fwd`` comes before any HIP call: testable without a device."""
    lib = L_.load()
    p = 0x1000                                                               # never dereferenced: the checks reject the call first
    rows2, rows3 = (C.c_void_p * 2)(p, p), (C.c_void_p * 3)(p, p, p)
    E = L_.SEPR_EINVAL

    def mix(buf16=p, t16=100, buf32=None, t32=0, off=p, n16=3, N=3, tu=p, ts=p, tn=p, tg=p, tr=p, tt=p, n=p, B=2, M=2, S=2, T=64, out=p, rows=rows2,
            rir=p, rtot=10, roff=p, R=2):
        return lib.sepr_dynmix_reverb_fwd(buf16, t16, buf32, t32, off, n16, N, tu, ts, tn, tg, tr, tt, n, B, M, S, T, out, rows, rir, rtot, roff, R, None)

    # the checks of sepr_dynmix_fwd
    for kw in (dict(off=None), dict(tu=None), dict(ts=None), dict(tn=None), dict(tg=None), dict(n=None), dict(out=None), dict(rows=None),
               dict(rows=(C.c_void_p * 2)(p, None)), dict(buf16=None), dict(B=0), dict(B=-1), dict(B=65536), dict(S=1), dict(S=4, rows=rows3),
               dict(M=1), dict(M=4), dict(S=3, M=2, rows=rows3), dict(S=3, M=5, rows=rows3), dict(T=0), dict(T=62), dict(T=66),
               dict(out=p + 4), dict(buf16=p + 2), dict(N=0, n16=0), dict(n16=4), dict(N=4), dict(t16=0), dict(t16=-1), dict(t32=-1),
               dict(n16=2, buf32=None, t32=5), dict(n16=2, buf32=p, t32=0), dict(n16=2, buf32=p + 4, t32=5),
               dict(rows=(C.c_void_p * 2)(p, p + 8))):
        assert mix(**kw) == E, kw
    # its own
    for kw in (dict(tr=None), dict(tt=None), dict(rir=None), dict(roff=None), dict(R=0), dict(R=-1), dict(rtot=0), dict(rtot=-5),
               dict(rir=p + 2), dict(rir=p + 1), dict(rir=p + 3)):
        assert mix(**kw) == E, kw
