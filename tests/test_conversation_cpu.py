"""Conversations, the part that needs no device: the planner's invariants, overlap fractions and scores on hand-made
tables, the C ABI's declarations and refusals, and the condition that makes the GPU test's derived tolerance honest."""
import os
import random
import re

import numpy as np
import pytest

import conversation_ref as ref
from sepreformer_amd import conversation as cv
from sepreformer_amd import datafeed as df
from sepreformer_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEAKERS = ("011", "01z", "22g", "40a", "c02")


def host_corpus(parseable=True, n_utts=30, seed=3):
    """A corpus layout on the host (no device): WSJ0-style names in two roles, lengths of 0.6 .. 2.5 s at 8 kHz, energies set by hand."""
    rng = np.random.default_rng(seed)
    arrays, roles = {}, {"s1": [], "s2": []}
    for i in range(n_utts):
        a, b = SPEAKERS[i % len(SPEAKERS)], SPEAKERS[(i + 2) % len(SPEAKERS)]
        key = f"x{i:02d}_{a}c02{i:02d}_0.5_{b}o03{i:02d}_-0.5" if parseable else f"utt{i:02d}"
        for role in roles:
            roles[role].append(key)
            n = int(rng.integers(4800, 20000))
            arrays[f"{role}/{key}"] = rng.normal(0, 0.05 + 0.01 * (i % 5), size=n).astype(np.float32)
    corpus = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    corpus.roles = roles
    corpus.set_energies(np.zeros(0, np.int64), np.array([float((a.astype(np.float64) ** 2).sum()) for a in arrays.values()]))
    corpus._host = None                                           # the planner reads names, lengths and energies: there is no sample to touch
    return corpus


@pytest.fixture(scope="module")
def corpus():
    return host_corpus()


def same(a, b):
    return a.key == b.key and a.n == b.n and a.S == b.S and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[3:], b[3:]))


@pytest.mark.parametrize("S, max_active", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_planner_is_deterministic_and_keeps_its_invariants(corpus, S, max_active):
    overlapped = 0
    for seed in range(50):
        c = cv.plan_conversation(corpus, random.Random(seed), seconds=12.0, speakers=S, max_active=max_active)
        assert same(c, cv.plan_conversation(corpus, random.Random(seed), seconds=12.0, speakers=S, max_active=max_active))
        assert c.n == 96000 and c.S == S
        ref.check_schedule(c, max_active=max_active, lengths=corpus.lengths)
        assert np.all(c.start == 0)
        last = int(np.argmax(c.place.astype(np.int64) + c.len))
        assert np.all((c.len == corpus.lengths[c.utt]) | (np.arange(len(c.utt)) == last))       # only the last utterance is cut
        assert int(c.place.min()) == 0
        # one speaker per track, distinct across tracks
        spk = [{cv.wsj0_speaker(corpus.names[u]) for u in c.utt[c.track == s]} for s in range(S) if np.any(c.track == s)]
        assert all(len(x) == 1 for x in spk) and len(set.union(*spk)) == len(spk)
        # RMS-normalised to the conversation's first utterance, by a float32 divide
        first = int(c.utt[np.argmin(c.place)])
        assert np.array_equal(c.norm, (corpus.rms[first] / corpus.rms[c.utt]).astype(np.float32))
        assert np.all((c.gain >= np.float32(10 ** (-2.5 / 20)) * 0.999) & (c.gain <= np.float32(10 ** (2.5 / 20)) * 1.001))
        ov = cv.overlap_fraction(c)
        assert ov.dtype == np.float64 and np.all((ov >= 0) & (ov <= 1))
        overlapped += int(np.any(ov > 0))
    assert (overlapped == 0) if max_active == 1 else (overlapped >= 40)
    assert not same(cv.plan_conversation(corpus, random.Random(0), 12.0, speakers=S), cv.plan_conversation(corpus, random.Random(1), 12.0, speakers=S))


def test_planner_turns_and_pool():
    c = cv.plan_conversation(host_corpus(), random.Random(5), seconds=20.0, speakers=3)
    order = np.argsort(c.place, kind="stable")
    assert np.all(np.diff(c.track[order]) != 0)                   # the next utterance belongs to another track than the one before
    plain = host_corpus(parseable=False)
    c = cv.plan_conversation(plain, random.Random(5), seconds=20.0, speakers=2)
    for s in range(2):                                            # unparseable keys: every utterance is a speaker of its own
        assert len(set(c.utt[c.track == s].tolist())) == 1
    with pytest.raises(ValueError):
        cv.plan_conversation(host_corpus(), random.Random(0), seconds=5.0, speakers=9)
    with pytest.raises(ValueError):
        cv.plan_conversation(host_corpus(), random.Random(0), seconds=5.0, speakers=6)      # five speakers in the pool
    one = cv.plan_conversation(host_corpus(), random.Random(2), seconds=9.0, speakers=1)
    ref.check_schedule(one, max_active=1)
    assert one.n % 4 == 0 and cv.plan_conversation(host_corpus(), random.Random(2), seconds=1.00013, speakers=1).n == 8000


def conv(n, S, segs):
    return cv.make_conversation("hand", n, S, [(0, 0, p, ln, 1.0, 1.0, t) for t, p, ln in segs])


def test_overlap_fraction_on_hand_made_schedules():
    c = conv(100, 2, [(0, 0, 40), (1, 30, 20), (0, 60, 40)])
    assert np.array_equal(cv.overlap_fraction(c), np.array([10 / 40, 0.0, 10 / 20]))
    c = conv(100, 3, [(0, 0, 100), (1, 10, 30), (2, 20, 40)])     # the union of the other tracks, not their sum
    assert np.array_equal(cv.overlap_fraction(c), np.array([0.5, 1.0, 1.0]))
    c = conv(8, 2, [(0, 0, 4), (1, 4, 4)])                        # abutting turns do not overlap
    assert np.array_equal(cv.overlap_fraction(c), np.zeros(2))
    assert [cv.overlap_bin(f) for f in (0.0, 1e-9, 0.2, 0.2000001, 0.5, 0.51, 1.0)] == [0, 1, 1, 2, 2, 3, 3]
    with pytest.raises(ValueError):
        conv(100, 2, [(0, 0, 40), (0, 39, 10)])
    with pytest.raises(ValueError):
        conv(100, 2, [(0, 90, 11)])
    with pytest.raises(ValueError):
        conv(102, 2, [(0, 0, 4)])


def test_score_on_hand_made_matrices():
    # one conversation, two tracks, two channels: track 0 sits in channel 1, track 1 in channel 0, and segment 2 (track 0) jumps to channel 0
    v = np.array([[1.0, 9.0], [8.0, 2.0], [7.0, 3.0], [6.0, 6.0], [0.0, 12.0]])
    v_mix = np.array([1.0, 1.0, 2.0, 2.0, 0.0])
    track = np.array([0, 1, 0, 1, 0])
    s = cv.score(v, v_mix, np.zeros(5, int), track, [2], 2, overlap=[0.0, 0.1, 0.3, 0.9, 0.0])
    assert s["assignment"] == {0: (1, 0)}                         # 9 + 3 + 12 + 8 + 6 = 38 against 1 + 7 + 0 + 2 + 6 = 16
    assert s["best"].tolist() == [1, 0, 0, 0, 1]                  # segment 3 is a tie: the lowest channel
    assert s["assigned"].tolist() == [1, 0, 1, 0, 1]
    assert s["switch"].tolist() == [0, 0, 1, 0, 0] and s["switch_rate"] == 0.2
    assert s["utt"].tolist() == [8.0, 7.0, 5.0, 4.0, 12.0] and s["cons"].tolist() == [8.0, 7.0, 1.0, 4.0, 12.0]
    assert s["sisnri_utt"] == 36.0 / 5 and s["sisnri_cons"] == 32.0 / 5
    assert [s["bins"][k]["n"] for k in cv.OVERLAP_BINS] == [2, 1, 1, 1]
    assert s["bins"]["0"]["sisnri_utt"] == 10.0 and s["bins"]["(0.2,0.5]"]["sisnri_cons"] == 1.0
    # the assignment's tie rule: every assignment scores the same, the lexicographically first wins - also with a spare channel
    s = cv.score(np.ones((4, 2)), np.zeros(4), np.zeros(4, int), [0, 1, 0, 1], [2], 2)
    assert s["assignment"] == {0: (0, 1)} and s["switch"].tolist() == [0, 1, 0, 1]
    s = cv.score(np.ones((2, 3)), np.zeros(2), np.zeros(2, int), [0, 1], [2], 3)
    assert s["assignment"] == {0: (0, 1)}
    s = cv.score(np.array([[0.0, 0.0, 5.0], [0.0, 4.0, 4.0]]), np.zeros(2), np.zeros(2, int), [0, 1], [2], 3)
    assert s["assignment"] == {0: (2, 1)} and s["best"].tolist() == [2, 1] and s["switch_rate"] == 0.0
    # more talkers than channels: no assignment, NaN, left out of the means; a second conversation beside it still counts
    v = np.array([[5.0, 1.0], [1.0, 5.0], [3.0, 2.0], [4.0, 0.0], [0.0, 4.0]])
    s = cv.score(v, np.ones(5), [0, 0, 0, 1, 1], [0, 1, 2, 0, 1], [3, 2], 2)
    assert s["assignment"] == {0: None, 1: (0, 1)}
    assert np.isnan(s["cons"][:3]).all() and np.isnan(s["switch"][:3]).all() and s["assigned"].tolist() == [-1, -1, -1, 0, 1]
    assert s["utt"].tolist() == [4.0, 4.0, 2.0, 3.0, 3.0] and s["sisnri_cons"] == 3.0 and s["switch_rate"] == 0.0
    alone = cv.score(v[:3], np.ones(3), [0, 0, 0], [0, 1, 2], [3], 2)
    assert np.isnan(alone["sisnri_cons"]) and np.isnan(alone["switch_rate"]) and alone["sisnri_utt"] == 10.0 / 3


def test_entries_are_declared_bound_and_refuse_before_any_device_call():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    for name in ("sepr_conversation_render", "sepr_segment_sisnr_bytes", "sepr_segment_sisnr_fwd"):
        assert re.search(r"^(int|long long) " + name + r"\(", hdr, re.M) and name in L.SIGNATURES
    assert re.search(r"^long long sepr_segment_sisnr_bytes\(int G, int C\);", hdr, re.M) and L.SIGNATURES["sepr_segment_sisnr_bytes"][0] is L._ll
    assert int(re.search(r"#define SEPR_VERSION (\d+)", hdr).group(1)) == 413 == L.ABI_VERSION
    mk = open(os.path.join(ROOT, "sepreformer_amd", "csrc", "Makefile")).read()
    assert "sepr_conversation.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    lib = L.load()
    p = 0x10000                                                   # a well-aligned address that is never dereferenced: every call below is refused
    good = dict(buf16=p, total16=64, buf32=p, total32=64, off=p, N16=2, N=4, cols=[p] * 7, out_off=p, R=2, S=2, G=3, total=4104, mix=p, tracks=p)

    def render(**kw):
        a = {**good, **kw}
        return lib.sepr_conversation_render(a["buf16"], a["total16"], a["buf32"], a["total32"], a["off"], a["N16"], a["N"], *a["cols"],
                                            a["out_off"], a["R"], a["S"], a["G"], a["total"], a["mix"], a["tracks"], None)

    bad = [dict(off=None), dict(mix=None), dict(out_off=None), dict(R=0), dict(R=65536), dict(S=0), dict(S=9), dict(G=0), dict(total=0),
           dict(total=4102), dict(mix=p + 4), dict(tracks=p + 8), dict(buf16=p + 2), dict(buf16=None), dict(buf32=None), dict(N16=5), dict(N=0),
           dict(total16=-1), dict(total32=0), dict(out_off=p + 4)]
    bad += [dict(cols=[p] * k + [None] + [p] * (6 - k)) for k in range(7)]
    for kw in bad:
        assert render(**kw) == L.SEPR_EINVAL, kw

    sgood = dict(est=p, ref=p, mix=p, rows=p, begin=p, length=p, G=5, C=2, S=2, T=100, ld=100, eps=1e-15, v=p, v_mix=p, ws=p, ws_bytes=1 << 20)

    def sisnr(**kw):
        a = {**sgood, **kw}
        return lib.sepr_segment_sisnr_fwd(a["est"], a["ref"], a["mix"], a["rows"], a["begin"], a["length"], a["G"], a["C"], a["S"], a["T"], a["ld"],
                                          a["eps"], a["v"], a["v_mix"], a["ws"], a["ws_bytes"], None)

    sbad = [dict(est=None), dict(ref=None), dict(mix=None), dict(rows=None), dict(begin=None), dict(length=None), dict(v=None), dict(v_mix=None),
            dict(G=0), dict(C=0), dict(C=9), dict(S=0), dict(S=9), dict(T=0), dict(ld=99), dict(eps=-1.0), dict(eps=float("nan")), dict(est=p + 2),
            dict(v=p + 4)]
    for kw in sbad:
        assert sisnr(**kw) == L.SEPR_EINVAL, kw
    need = lib.sepr_segment_sisnr_bytes(5, 2)
    assert need >= 5 * 2 * 8 and need % 256 == 0 and lib.sepr_segment_sisnr_bytes(1 << 20, 8) >= (1 << 20) * 16
    assert [lib.sepr_segment_sisnr_bytes(*a) for a in ((0, 2), (5, 0), (5, 9))] == [0, 0, 0]
    assert sisnr(ws_bytes=need - 1) == L.SEPR_EWORKSPACE and sisnr(ws=None) == L.SEPR_EWORKSPACE
    with pytest.raises(RuntimeError, match="HIP device"):         # no CPU path
        cv.render(host_corpus(), [conv(8, 1, [(0, 0, 4)])])


@pytest.mark.parametrize("C", [2, 3])
def test_the_tolerance_is_honest_on_every_case(C):
    """``tol_db`` assumes that the float64 restatement itself is good to a fraction of it and that the cross term cancels by at most 1 / |rho| <= 34:
    on every case of the GPU test the float64 restatement and a numpy longdouble one agree within half the tolerance, every non-silent case
    has |rho| >= 0.03 and an SI-SNR of at least -30 dB, and the silent ones give -300."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps          # the comparison needs a wider format than float64
    pr = ref.sisnr_problem(C)
    assert pr["ld"] > pr["T"] and np.all(pr["begin"] % 4 != 0) and int((pr["begin"] + pr["length"]).max()) <= pr["T"]
    assert sorted(set(pr["length"].tolist())) == sorted(ref.LENGTHS) and set(pr["family"]) == set(ref.FAMILIES)
    v, vm = ref.sisnr_ref(pr["est"], pr["ref"], pr["mix"], pr["rows"], pr["begin"], pr["length"])
    assert abs(ref.tol_db(5000) - 4.8e-10) < 0.1e-10
    best = v.argmax(1)
    for g, fam in enumerate(pr["family"]):
        n, sl = int(pr["length"][g]), slice(int(pr["begin"][g]), int(pr["begin"][g]) + int(pr["length"][g]))
        r = pr["ref"][pr["rows"][g], sl]
        for k in range(C + 1):
            a, got = (pr["est"][k, sl], v[g, k]) if k < C else (pr["mix"][sl], vm[g])
            assert abs(got - ref.sisnr_longdouble(a, r)) <= 0.5 * ref.tol_db(n), (g, fam, n, k)
            silent = n == 1 or fam == "silent_ref" or (fam == "silent_est" and (k == 0 or n == 2))
            if silent:
                assert abs(got + 300.0) < 1e-9, (g, fam, n, k)
            else:
                assert ref.correlation(a, r) >= 0.03 and -30.0 <= got <= 60.0, (g, fam, n, k, got)
        if n >= 3 and fam in ("noise", "dc"):
            assert best[g] == 0
        if n >= 3 and fam == "swapped":
            assert best[g] == 1
