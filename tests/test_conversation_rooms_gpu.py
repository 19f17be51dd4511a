"""Conversations in rooms on the device: ``sepr_conversation_render_rooms`` bit for bit against the numpy restatement
(tests/conversation_rooms_ref.py) on a hand schedule and on planned conversations with a noise bed, against the dry entry where the two must agree,
under capture with both device tables rewritten, and ``infer.evaluate_conversations(..., rirs=bank)`` end to end."""
import csv
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conversation_rooms_ref as rref                                        # noqa: E402

from sepreformer_amd import conversation as cv                               # noqa: E402
from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def synthetic_corpus(fmt, noise=False):
    """The six-utterance corpus of tests/test_conversation_gpu.py (role ``s1``), with ``noise`` two short utterances of role ``noise`` more."""
    if (fmt, noise) not in _cache:
        arrays = rref.corpus_arrays(fmt, noise=noise)
        corpus = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
        corpus.roles = rref.roles_of(arrays)
        _cache[fmt, noise] = (corpus, [arrays[nm] for nm in corpus.names])
    return _cache[fmt, noise]


def hand_bank():
    if "bank" not in _cache:
        hs = rref.hand_bank()
        _cache["bank"] = (rv.RirBank.from_arrays(hs, 8000, device=DEV, normalise=None), hs)
    return _cache["bank"]


def restated(fmt, S, seed):
    """The hand conversations and their restated render, computed once per case and left unchanged."""
    key = ("hand", fmt, S, seed)
    if key not in _cache:
        convs = rref.hand_conversations(S, seed)
        _cache[key] = (convs, rref.render_ref(synthetic_corpus(fmt)[1], hand_bank()[1], convs))
    return _cache[key]


def device_form(c):
    """The restatement's conversation as a ``cv.Conversation``, through ``make_conversation``'s checks."""
    segs = [(int(c.utt[g]), int(c.start[g]), int(c.place[g]), int(c.len[g]), c.norm[g], c.gain[g], int(c.track[g])) for g in range(len(c.utt))]
    rooms = None if c.rir is None else [(int(c.rir[g]), int(c.taps[g]), int(c.direct[g])) for g in range(len(c.utt))]
    out = cv.make_conversation(c.key, c.n, c.S, segs, rooms=rooms)
    for f in ("utt", "start", "place", "len", "track", "norm", "gain"):
        assert np.array_equal(getattr(out, f), getattr(c, f)), f
    return out


def bits(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("fmt", ["int16", "float32", "both"])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_render_is_the_restatement_bit_for_bit(fmt, S):
    corpus, utts = synthetic_corpus(fmt)
    bank, hs = hand_bank()
    ref_convs, (want_mix, want_tracks, want_wet, out_off) = restated(fmt, S, seed=S)
    convs = [device_form(c) for c in ref_convs]
    for c in convs:
        rref.check_schedule(c, bank_lengths=bank.lengths, lengths=corpus.lengths)
    rd = cv.render(corpus, convs, rirs=bank)
    assert rd.table.has_rooms and rd.mix.shape == (4104,) and rd.tracks.shape == (S, 4104) and out_off.tolist() == [0, 4100, 4104] == rd.out_off.tolist()
    assert torch.equal(bits(rd.mix), bits(want_mix))
    assert torch.equal(bits(rd.tracks), bits(want_tracks))
    assert float(np.abs(want_mix).max()) > 0.1 and not np.array_equal(want_wet[0], want_tracks[0]) and (S < 3 or not want_tracks[2].any())
    again = cv.render(corpus, convs, rirs=bank)                   # two calls are bit-identical
    assert torch.equal(bits(again.mix), bits(rd.mix)) and torch.equal(bits(again.tracks), bits(rd.tracks))
    bare = cv.render(corpus, convs, tracks=False, rirs=bank)      # the same mixture without the track rows
    assert bare.tracks is None and torch.equal(bits(bare.mix), bits(rd.mix))
    assert torch.equal(bits(rd.mixture(1)), bits(want_mix[4100:])) and rd.tracks_of(1).shape == (min(S, 2), 4) and rd.bed_of(0) is None
    assert torch.equal(bits(rd.tracks_of(0)), bits(want_tracks[:, :4100]))


def test_equalities_with_the_dry_entry():
    """On an int16 corpus (no ``-0.0``): every ``rir = -1`` through the new entry, and the unit impulse on every segment, give the bits of
    ``sepr_conversation_render``; the delay-700 response gives the dry tracks shifted by 700 and cut at ``n``."""
    corpus, utts = synthetic_corpus("int16")
    bank, _ = hand_bank()
    dry = [device_form(rref.dry(c)) for c in rref.hand_conversations(8, seed=5)]
    want = cv.render(corpus, dry)
    assert not want.table.has_rooms and want.table.rooms is None

    def everywhere(r, taps):
        return [c._replace(rir=np.full(len(c.utt), r, np.int32), taps=np.full(len(c.utt), taps, np.int32),
                           direct=np.full(len(c.utt), taps, np.int32)) for c in dry]

    none = cv.render(corpus, everywhere(-1, 1))                   # no bank at all: NR = 0
    unit = cv.render(corpus, everywhere(rref.R_UNIT, 1), rirs=bank)
    for got in (none, unit):
        assert got.table.has_rooms
        assert torch.equal(bits(got.mix), bits(want.mix)) and torch.equal(bits(got.tracks), bits(want.tracks))
    k = rref.DELAY
    late = cv.render(corpus, everywhere(rref.R_DELAY, k + 1), rirs=bank)
    shifted = torch.zeros_like(want.tracks)
    shifted[:, k:4100] = want.tracks[:, :4100 - k]                # the second conversation, 4 samples, is cut to nothing
    assert torch.equal(bits(late.tracks), bits(shifted)) and float(shifted.abs().max()) > 0.1
    mix = torch.zeros_like(want.mix)
    for s in range(8):
        mix = mix + shifted[s]
    assert torch.equal(bits(late.mix), bits(mix))


def planned(noise_corpus, bank, seeds=(0, 1, 2), seconds=1.5):
    corpus, _ = noise_corpus
    return [cv.plan_conversation(corpus, random.Random(s), seconds=seconds, roles=("s1",), speakers=2 + s % 2, overlap=(0.1, 0.6), rirs=bank,
                                 early_ms=2.0 * (s % 2), noise="noise") for s in seeds]


def synthetic_bank():
    if "synthetic" not in _cache:
        hs = rv.synthetic_rirs(4, 8000, rt60=0.15)
        bank = rv.RirBank.from_arrays(hs, 8000, device=DEV)
        _cache["synthetic"] = (bank, [bank.rir(r) for r in range(4)])          # the responses as the bank stores them
    return _cache["synthetic"]


def test_render_of_planned_conversations_with_a_bed():
    """The planner's own schedules, three of 1.5 s in one launch, two and three talkers in synthetic rooms over a noise bed."""
    corpus, utts = synthetic_corpus("both", noise=True)
    bank, hs = synthetic_bank()
    convs = planned((corpus, utts), bank)
    for c in convs:
        rref.check_schedule(c, bank_lengths=bank.lengths, max_active=2, lengths=corpus.lengths)
    want_mix, want_tracks, want_wet, out_off = rref.render_ref(utts, hs, convs)
    rd = cv.render(corpus, convs, rirs=bank)
    assert torch.equal(bits(rd.mix), bits(want_mix)) and torch.equal(bits(rd.tracks), bits(want_tracks))
    for r, c in enumerate(convs):
        a, b = int(out_off[r]), int(out_off[r + 1])
        assert rd.tracks_of(r).shape == (c.S, c.n) and torch.equal(bits(rd.bed_of(r)), bits(want_wet[c.S, a:b]))
        assert np.count_nonzero(want_wet[c.S, a:b]) > 0.9 * c.n      # the bed has no gap
        assert not np.array_equal(want_wet[:c.S, a:b], want_tracks[:c.S, a:b])


def test_capture_replays_with_both_tables_rewritten():
    """The rooms launch inside a torch.cuda.graph; both device tables rewritten with other conversations of the same counts - other responses,
    taps and places - and replayed: the bits are the new tables'."""
    corpus, utts = synthetic_corpus("both")
    bank, hs = hand_bank()
    r0 = rref.hand_conversations(3, seed=1)
    r1 = rref.hand_conversations(3, seed=2)
    m = r1[0]
    on1 = m.track == 1
    m.place = np.where(on1, m.place - 1, m.place).astype(np.int32)
    m.start = (m.start + 1).astype(np.int32)
    m.rir = np.where(m.rir == 4, 2, np.where(m.rir == -1, rref.R_UNIT, m.rir)).astype(np.int32)       # 1025 taps -> 1023; none -> the unit impulse
    m.taps = np.where(m.rir == 2, 1023, np.where(m.rir == 5, 1500, m.taps)).astype(np.int32)          # 2049 -> the first 1500
    m.direct = np.minimum(m.direct, m.taps).astype(np.int32)
    rref.check_schedule(m, bank_lengths=bank.lengths, lengths=corpus.lengths)
    c0, c1 = [device_form(c) for c in r0], [device_form(c) for c in r1]
    table = cv.ConvTable(c0, DEV)
    mix = torch.zeros(table.total, device=DEV)
    tracks = torch.zeros(table.S_max, table.total, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cv.render_into(corpus, table, mix, tracks, rirs=bank)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cv.render_into(corpus, table, mix, tracks, rirs=bank)
    wants = {}
    for name, convs, rconvs in (("c1", c1, r1), ("c0", c0, r0)):
        words, out_off = table.pack(convs)
        table.words.copy_(torch.from_numpy(words))
        table.out_off.copy_(torch.from_numpy(out_off))
        table.rooms.copy_(torch.from_numpy(table.pack_rooms(convs, rirs=bank)))
        graph.replay()
        torch.cuda.synchronize()
        want_mix, want_tracks, _, _ = wants[name] = rref.render_ref(utts, hs, rconvs)
        assert torch.equal(bits(mix), bits(want_mix)) and torch.equal(bits(tracks), bits(want_tracks)), name
    assert not np.array_equal(wants["c0"][0], wants["c1"][0])


def test_evaluate_conversations_end_to_end(tmp_path):
    """``infer.evaluate_conversations(..., rirs=bank)`` on the smallest synthetic-weight model, two conversations of 1.25 s, one over a bed: its
    numbers and its csv equal ``score(segment_sisnr(...))`` computed here from ``separate_long``'s own output on the restatement's render, over
    the spans moved with the direct path; ``method="bank"`` scores the same segments with finite values and the same ``v_mix``."""
    corpus, utts = synthetic_corpus("both", noise=True)
    bank, hs = synthetic_bank()
    model = Model.from_config(VARIANTS["tiny"], init_seed=0).load_synthetic_(0).eval().to(DEV)
    kwp = dict(seconds=1.25, roles=("s1",), speakers=2, rirs=bank)
    convs = [cv.plan_conversation(corpus, random.Random(11), noise="noise", **kwp), cv.plan_conversation(corpus, random.Random(12), **kwp)]
    assert [c.n for c in convs] == [10000, 10000] and [c.bed for c in convs] == [1, 0]
    kw = dict(chunk_seconds=0.5, overlap_seconds=0.125)
    path = str(tmp_path / "segments.csv")
    got = infer.evaluate_conversations(model, corpus, convs, rirs=bank, method="long", csv_path=path, **kw)

    want_mix, want_tracks, _, out_off = rref.render_ref(utts, hs, convs)
    mixes = [torch.from_numpy(want_mix[out_off[r]:out_off[r + 1]]).to(DEV) for r in range(2)]
    ests = longform.separate_long(model, mixes, **kw)
    peak = [int(np.argmax(np.abs(h))) for h in hs]                # the index of the first maximum of |h_r|
    vs, vms, spans = [], [], []
    for r, c in enumerate(convs):
        k = np.nonzero(c.track < c.S)[0]
        begin = np.array([min(int(c.place[g]) + peak[int(c.rir[g])], c.n - 1) for g in k])
        length = np.array([max(1, min(int(c.len[g]), c.n - b)) for g, b in zip(k, begin)])
        spans.append((k, begin, length))
        tr = torch.from_numpy(np.ascontiguousarray(want_tracks[:c.S, out_off[r]:out_off[r + 1]])).to(DEV)
        v, vm = cv.segment_sisnr(torch.stack(list(ests[r])), tr, mixes[r], c.track[k], begin, length)
        vs.append(v.cpu().numpy())
        vms.append(vm.cpu().numpy())
    assert any((b != c.place[k]).any() for c, (k, b, _) in zip(convs, spans))            # a span did move
    v, vm = np.concatenate(vs), np.concatenate(vms)
    G = sum(len(k) for k, _, _ in spans)
    assert G < sum(len(c.utt) for c in convs)                    # the bed's segments are not scored
    conv_of = np.concatenate([np.full(len(k), r) for r, (k, _, _) in enumerate(spans)])
    want = cv.score(v, vm, conv_of, np.concatenate([c.track[k] for c, (k, _, _) in zip(convs, spans)]), [2, 2], 2,
                    overlap=np.concatenate([cv.overlap_fraction(c)[k] for c, (k, _, _) in zip(convs, spans)]))
    assert got["n"] == G == v.shape[0] and got["conversations"] == 2
    assert np.array_equal(got["v"], v) and np.array_equal(got["v_mix"], vm) and np.all(np.isfinite(v))
    for key in ("best", "assigned", "utt", "cons", "switch"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for key in ("sisnri_utt", "sisnri_cons", "switch_rate"):
        assert got[key] == want[key] and np.isfinite(got[key]), key
    np.testing.assert_equal(got["bins"], want["bins"])
    assert got["assignment"] == want["assignment"]
    rows = list(csv.reader(open(path, newline=""), quotechar="|"))
    assert len(rows) == G and all(len(r) == 10 + 2 for r in rows)
    g = 0
    for c, (ks, begin, length) in zip(convs, spans):
        for i, k in enumerate(ks):
            row = rows[g]
            assert row[:6] == [c.key, str(k), str(int(c.track[k])), corpus.names[int(c.utt[k])], str(int(begin[i])), str(int(length[i]))]
            assert float(row[6]) == want["overlap"][g] and int(row[7]) == want["best"][g] and int(row[8]) == want["assigned"][g]
            assert float(row[9]) == vm[g] and [float(x) for x in row[10:]] == v[g].tolist()
            g += 1

    out = infer.evaluate_conversations(model, corpus, convs, rirs=bank, method="bank", slots=4, **kw)
    assert out["n"] == G and out["v"].shape == (G, 2) and np.all(np.isfinite(out["v"])) and np.array_equal(out["v_mix"], vm)
    with pytest.raises(ValueError):
        infer.evaluate_conversations(model, corpus, convs, method="long", **kw)          # rooms without rirs=
