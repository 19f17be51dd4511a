"""Conversations in rooms without a device: the restatement (tests/conversation_rooms_ref.py) against ``np.convolve``
and against the dry restatement, the planner's rooms and noise bed, the refusals of ``make_conversation``, ``render`` and the C entry, and that the
hand schedule of the device test holds what it names."""
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conversation_ref as cref                                              # noqa: E402
import conversation_rooms_ref as rref                                        # noqa: E402
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_reverb_ref as drr                                              # noqa: E402

from sepreformer_amd import conversation as cv                               # noqa: E402
from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def host_corpus(fmt="both", noise=True):
    arrays = rref.corpus_arrays(fmt, noise=noise)
    corpus = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    corpus.roles = rref.roles_of(arrays)
    utts = [arrays[nm] for nm in corpus.names]
    corpus.set_energies(np.array([dr.energy(a) for a in utts[:corpus.n16]], dtype=np.int64),
                        np.array([dr.energy(a) for a in utts[corpus.n16:]], dtype=np.float64))
    return corpus, utts


@pytest.fixture(scope="module")
def hand():
    """The hand conversations on 8 tracks and their restated render, computed once."""
    arrays = rref.corpus_arrays("both")
    corpus = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    utts = [arrays[nm] for nm in corpus.names]
    convs = rref.hand_conversations(8, seed=8)
    bank = rref.hand_bank()
    return utts, bank, convs, rref.render_ref(utts, bank, convs)


def test_restatement_against_np_convolve(hand):
    """Every segment of the hand schedule, under ``taps`` and under ``direct``: the float64 sums before the rounding against ``np.convolve`` in
    float64, within the bound tests/test_dynmix_reverb_cpu.py derives - ``taps 2^-52 sum_j |h_j| |x_{t-j}|`` per sample."""
    utts, bank, convs, _ = hand
    seen = 0
    for c in convs:
        for g in range(len(c.utt)):
            if c.rir[g] < 0:
                continue
            x = cref.sample_values(utts[int(c.utt[g])])[int(c.start[g]):int(c.start[g]) + int(c.len[g])]
            for K in {int(c.taps[g]), int(c.direct[g])}:
                h = bank[int(c.rir[g])][:K]
                m = x.shape[0] + K - 1
                got = drr.conv64(np.concatenate([x, np.zeros(K - 1, np.float32)]), bank[int(c.rir[g])], 0, m, K)
                want = np.convolve(x.astype(np.float64), h.astype(np.float64))
                bound = K * 2.0 ** -52 * np.convolve(np.abs(x).astype(np.float64), np.abs(h).astype(np.float64))
                assert got.shape == want.shape == (m,) and (np.abs(got - want) <= bound).all(), (g, K)
                v = rref.segment_value(x, bank[int(c.rir[g])], K, c.norm[g], c.gain[g], int(c.place[g]), c.n)
                a = (got.astype(np.float32) * np.float32(c.norm[g])).astype(np.float32)
                assert np.array_equal(bits(v), bits((a * np.float32(c.gain[g])).astype(np.float32)[:v.shape[0]]))
                seen += 1
    assert seen >= 12


def test_the_three_equalities_of_the_definition(hand):
    """Every ``rir = -1``: the dry restatement's bits (an int16 corpus holds no ``-0.0``).  The unit impulse everywhere: the same.  A pure delay of
    700 on every segment: the dry tracks 700 samples later, cut at ``n``."""
    arrays = rref.corpus_arrays("int16")
    utts = list(arrays.values())
    bank = rref.hand_bank()
    convs = rref.hand_conversations(8, seed=3)
    want_mix, want_tracks, _ = cref.render_ref(utts, [rref.dry(c) for c in convs], S_max=8)

    def with_rooms(c, r, taps):
        d = rref.dry(c)
        G = len(c.utt)
        d.rir, d.taps, d.direct = np.full(G, r, np.int32), np.full(G, taps, np.int32), np.full(G, taps, np.int32)
        return d

    for r, taps in ((-1, 1), (rref.R_UNIT, 1)):
        mix, tracks, wet, _ = rref.render_ref(utts, bank, [with_rooms(c, r, taps) for c in convs], S_max=8)
        assert np.array_equal(bits(mix), bits(want_mix)) and np.array_equal(bits(tracks), bits(want_tracks)), r
        assert np.array_equal(bits(wet), bits(tracks))
    # a delayed track overlaps its own next segment only where the two do not abut; the hand schedule abuts, so compare segment by segment
    k = rref.DELAY
    for c in convs:
        for g in range(len(c.utt)):
            one = rref.dry(c)
            for f in ("utt", "start", "place", "len", "norm", "gain", "track"):
                setattr(one, f, getattr(c, f)[g:g + 1])
            dry_mix, dry_tracks, _ = cref.render_ref(utts, [one], S_max=8)
            mix, tracks, wet, _ = rref.render_ref(utts, bank, [with_rooms(one, rref.R_DELAY, k + 1)], S_max=8)
            shifted = np.zeros_like(dry_tracks)
            if c.n > k:
                shifted[:, k:] = dry_tracks[:, :c.n - k]
            assert np.array_equal(bits(tracks), bits(shifted)) and np.array_equal(bits(wet), bits(shifted)), (c.key, g)


def test_the_hand_schedule_holds_what_it_names(hand):
    """Asserted from the restatement, so the device test cannot pass by leaving the hard part out."""
    utts, bank, convs, (mix, tracks, wet, out_off) = hand
    a = convs[0]
    lengths = [u.shape[0] for u in utts]
    for c in convs:
        rref.check_schedule(c, bank_lengths=[h.shape[0] for h in bank], lengths=lengths)
    assert a.n == rref.HAND_N == 4100 and out_off.tolist() == [0, 4100, 4104]
    cnt = rref.contributors(convs)
    assert cnt[0, :4100].max() >= 3 and int((cnt[0, :4100] >= 3).sum()) >= 1000       # three and more contributors of ONE track under one sample
    end = a.place.astype(np.int64) + a.len
    reach = end + a.taps - 1
    assert np.any((end < a.n) & (reach > a.n))                                  # a tail cut by n
    assert np.any(end == a.n) and np.any(reach[a.track == 0] > 4096)            # a segment ending at n; a tail across 4096
    assert np.any((a.place < 2048) & (reach > 2048) & (end <= 2048))            # a tail across 2048
    same = a.track[1:] == a.track[:-1]
    assert np.any(same & (a.place[1:] == end[:-1]))                             # pause 0
    t0 = a.track == 0
    assert (a.rir[t0] < 0).any() and (a.rir[t0] >= 0).any() and not (a.track == 2).any()
    wet_seg = a.rir >= 0
    assert {1, 2049} <= set(a.direct[wet_seg].tolist()) and np.any((a.direct > 1) & (a.direct < a.taps)) and np.any((a.direct == a.taps) & (a.taps > 1))
    assert (1, 2049) in {(int(l), int(t)) for l, t in zip(a.len, a.taps)}      # a 1-sample segment with a 2049-tap response
    assert set(rref.BANK_TAPS) <= set(a.taps.tolist())
    for s in sorted(set(a.track[(a.rir >= 0) & (a.taps > 1) & (a.direct < a.taps)].tolist())):
        assert not np.array_equal(wet[s, :4100], tracks[s, :4100]), s            # wet differs from the reference on every reverberant track
    assert convs[1].n == 4 and int(convs[1].taps.max()) == 1025                # the second conversation's tail is cut at once
    assert float(np.abs(mix).max()) > 0.1 and not tracks[2].any() and not wet[2].any()


def test_planner_with_the_options_off_draws_nothing_more():
    corpus, _ = host_corpus()
    for seed in range(5):
        kw = dict(seconds=1.5, roles=("s1",), speakers=2 + seed % 2, overlap=(0.1, 0.6))
        r0, r1 = random.Random(seed), random.Random(seed)
        old = cv.plan_conversation(corpus, r0, **kw)
        new = cv.plan_conversation(corpus, r1, rirs=None, target="direct", early_ms=0.0, noise=None, noise_db=(-6.0, 3.0), **kw)
        assert r0.getstate() == r1.getstate()
        assert len(old) == len(new) == 10 and cv.Conversation.ROOM_FIELDS == ("rir", "taps", "direct", "bed")
        for f in cv.Conversation._fields + cv.Conversation.ROOM_FIELDS:
            x, y = getattr(old, f), getattr(new, f)
            assert (x is None and y is None) or np.array_equal(x, y), f
        assert old.rir is None and old.taps is None and old.direct is None and old.bed == 0
        cref.check_schedule(old, max_active=2, lengths=corpus.lengths)


@pytest.mark.parametrize("target, early_ms", [("direct", 0.0), ("direct", 2.5), ("full", 0.0)])
def test_planner_with_rooms_and_a_bed(target, early_ms):
    corpus, _ = host_corpus()
    hs = rv.synthetic_rirs(4, 8000, rt60=0.15)
    bank = rv.RirBank.from_arrays(hs, 8000, device=None)
    for seed in range(5):
        S = 2 + seed % 2
        kw = dict(seconds=1.5, roles=("s1",), speakers=S, overlap=(0.1, 0.6))
        dry = cv.plan_conversation(corpus, random.Random(seed), **kw)
        c = cv.plan_conversation(corpus, random.Random(seed), rirs=bank, target=target, early_ms=early_ms, noise="noise", **kw)
        rref.check_schedule(c, bank_lengths=bank.lengths, max_active=2, lengths=corpus.lengths)
        assert c.S == S and c.bed == 1 and c.n == dry.n
        talk = c.track < S
        for s in range(S):                                                      # one response per track, whole, its direct path as specified
            r = set(c.rir[c.track == s].tolist())
            assert len(r) == 1 and 0 <= min(r) < 4
            r = r.pop()
            k = c.track == s
            assert np.all(c.taps[k] == bank.lengths[r])
            want = bank.lengths[r] if target == "full" else min(bank.lengths[r], int(bank._direct[r]) + int(round(early_ms * 8)))
            assert np.all(c.direct[k] == want)
        # the draws: the speakers, then one response per track; the talkers' places differ from the dry plan's only through those draws
        rng = random.Random(seed)
        names = sorted({f"utt:s1/{k}" for k in corpus.roles["s1"]})
        rng.sample(names, S)
        assert [rng.randrange(4) for _ in range(S)] == [int(c.rir[c.track == s][0]) for s in range(S)]
        b = ~talk
        assert np.all(c.track[b] == S) and c.place[b][0] == 0 and int(c.place[b][-1]) + int(c.len[b][-1]) == c.n
        assert np.array_equal(c.place[b][1:], (c.place[b] + c.len[b])[:-1]) and np.all(c.start[b] == 0)
        assert len(set(c.gain[b].tolist())) == 1 and set(c.utt[b].tolist()) <= {corpus.index["noise/n0"], corpus.index["noise/n1"]}
        first = int(c.utt[np.nonzero((c.track == 0) & (c.place == 0))[0][0]])
        assert np.array_equal(c.norm[b], np.array([np.float32(corpus.rms[first]) / np.float32(corpus.rms[u]) for u in c.utt[b]], np.float32))
        ov = cv.overlap_fraction(c)
        assert np.array_equal(ov[talk], cv.overlap_fraction(c._replace(**{f: getattr(c, f)[talk] for f in
                                                                          ("utt", "start", "place", "len", "norm", "gain", "track", "rir", "taps",
                                                                           "direct")}, bed=0)))
        assert not ov[b].any() and ov[talk].max() < 1.0                         # the bed covers everything and is ignored
    only_bed = cv.plan_conversation(corpus, random.Random(1), seconds=1.5, roles=("s1",), noise="noise")
    assert only_bed.rir is None and only_bed.bed == 1
    rref.check_schedule(only_bed, lengths=corpus.lengths)
    with pytest.raises(ValueError):
        cv.plan_conversation(corpus, random.Random(1), seconds=1.5, roles=("s1",), noise="nobody")
    with pytest.raises(ValueError):
        cv.plan_conversation(corpus, random.Random(1), seconds=1.5, roles=("s1",), rirs=bank, target="dry")


def test_refusals():
    corpus, _ = host_corpus()
    bank = rv.RirBank.from_arrays(rref.hand_bank(), 8000, device=None, normalise=None)
    f = np.float32(1.0)
    seg = [(0, 0, 0, 8, f, f, 0)]
    ok = cv.make_conversation("ok", 16, 1, seg, rooms=[(5, 2049, 7)])
    assert ok.rir.tolist() == [5] and ok.taps.tolist() == [2049] and ok.direct.tolist() == [7] and ok.bed == 0 and ok.rir.dtype == np.int32
    swapped = cv.make_conversation("s", 16, 2, [(0, 0, 8, 8, f, f, 1), (1, 0, 0, 8, f, f, 0)], rooms=[(3, 9, 2), (-1, 1, 1)])
    assert swapped.track.tolist() == [0, 1] and swapped.rir.tolist() == [-1, 3]      # the rooms are sorted along with the segments
    for rooms in ([(0, 1, 2)], [(2, 0, 0)], [(-2, 1, 1)], [(-1, 2, 1)], [(1, 16385, 1)], [(0, 1, 1), (0, 1, 1)]):
        with pytest.raises(ValueError):
            cv.make_conversation("bad", 16, 1, seg, rooms=rooms)
    with pytest.raises(ValueError):                                             # no room for a bed beside eight talkers
        cv.make_conversation("bad", 16, 8, seg, bed=True)
    with pytest.raises(ValueError):                                             # track S without a bed
        cv.make_conversation("bad", 16, 1, seg + [(1, 0, 0, 16, f, f, 1)])
    with pytest.raises(ValueError):                                             # a bed in a room
        cv.make_conversation("bad", 16, 1, seg + [(1, 0, 0, 16, f, f, 1)], rooms=[(-1, 1, 1), (0, 1, 1)], bed=True)
    bed = cv.make_conversation("bed", 16, 1, seg + [(1, 0, 0, 16, f, f, 1)], bed=True)
    assert bed.bed == 1 and bed.S == 1 and bed.track.tolist() == [0, 1]
    # render: the host checks come before anything else
    with pytest.raises(ValueError, match="rirs"):
        cv.render(corpus, [ok])
    with pytest.raises(ValueError):
        cv.render(corpus, [cv.make_conversation("r", 16, 1, seg, rooms=[(8, 1, 1)])], rirs=bank)      # rir >= len(bank)
    with pytest.raises(ValueError):
        cv.render(corpus, [cv.make_conversation("r", 16, 1, seg, rooms=[(4, 1026, 1)])], rirs=bank)   # taps > len_r
    with pytest.raises(RuntimeError, match="HIP device"):                       # checked, and then there is no CPU path
        cv.render(corpus, [ok], rirs=bank)


def test_entry_is_declared_bound_and_refuses_before_any_device_call():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    name = "sepr_conversation_render_rooms"
    assert re.search(r"^int " + name + r"\(", hdr, re.M) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 29
    lib = L.load()
    p = 0x10000                                                   # a well-aligned address that is never dereferenced: every call below is refused
    good = dict(buf16=p, total16=64, buf32=p, total32=64, off=p, N16=2, N=4, cols=[p] * 10, out_off=p, R=2, S=2, G=3, total=4104, mix=p, tracks=p,
                rir=p, rir_total=100, rir_off=p, NR=3)

    def render(**kw):
        a = {**good, **kw}
        return lib.sepr_conversation_render_rooms(a["buf16"], a["total16"], a["buf32"], a["total32"], a["off"], a["N16"], a["N"], *a["cols"],
                                                  a["out_off"], a["R"], a["S"], a["G"], a["total"], a["mix"], a["tracks"], a["rir"],
                                                  a["rir_total"], a["rir_off"], a["NR"], None)

    bad = [dict(off=None), dict(mix=None), dict(out_off=None), dict(R=0), dict(R=65536), dict(S=0), dict(S=9), dict(G=0), dict(total=0),
           dict(total=4102), dict(mix=p + 4), dict(tracks=p + 8), dict(buf16=p + 2), dict(buf16=None), dict(buf32=None), dict(N16=5), dict(N=0),
           dict(total16=-1), dict(total32=0), dict(out_off=p + 4)]                # what sepr_conversation_render refuses
    bad += [dict(cols=[p] * k + [None] + [p] * (9 - k)) for k in range(10)]
    bad += [dict(NR=-1), dict(rir=None), dict(rir_off=None), dict(rir_total=0), dict(rir=p + 2), dict(rir_off=p + 4)]      # and of a bank
    for kw in bad:
        assert render(**kw) == L.SEPR_EINVAL, kw
