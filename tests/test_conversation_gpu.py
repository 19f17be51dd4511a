"""Conversations on the device: sepr_conversation_render bit for bit against the numpy restatement, sepr_segment_sisnr_fwd
against the oracle's per-pair SI-SNR in float64 within the derived tolerance (tests/conversation_ref.py), and the test loop around
separate_long / separate_many end to end."""
import csv
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conversation_ref as ref                                               # noqa: E402

from sepreformer_amd import conversation as cv                               # noqa: E402
from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = ((5000, True), (4101, True), (2600, True), (4999, False), (3000, False), (37, False))
_cache = {}


def synthetic_corpus(fmt):
    """Six utterances of 5000, 4101, 2600 (int16) and 4999, 3000, 37 (float32) samples - ``fmt`` "int16" / "float32" stores all six in that
    format - with large values, so a read into a neighbour is not a read of zeros (the corpus of tests/test_dynmix_turns_gpu.py)."""
    if fmt not in _cache:
        rng = np.random.default_rng(7)
        arrays = {}
        for i, (n, is16) in enumerate(LENGTHS):
            if fmt == "int16" or (fmt == "both" and is16):
                arrays[f"u{i}"] = rng.integers(-20000, 20000, size=n, dtype=np.int16)
            else:
                arrays[f"u{i}"] = rng.normal(0, 0.1, size=n).astype(np.float32)
        corpus = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
        _cache[fmt] = (corpus, [arrays[nm] for nm in corpus.names])
    return _cache[fmt]


def bits(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().contiguous().view(torch.int32)


# (track, utt, start, place, len): 4100 samples; the render kernel's tiles are 1024 samples, a thread makes 4
SEGMENTS = [
    (0, 5, 3, 0, 1), (0, 0, 7, 1, 2047), (0, 1, 0, 2048, 2049), (0, 5, 0, 4097, 3),        # placed at 0; three that abut; the last ends at n
    (1, 3, 5, 1025, 2048), (1, 4, 1, 3073, 1), (1, 2, 100, 3500, 600),                     # 2048 long across samples 2048 and 3072; ends at n
    # track 2 holds no segment
    (3, 4, 2, 2047, 1), (3, 2, 0, 2048, 1), (3, 3, 11, 2049, 2047),                        # single samples either side of sample 2048
    (4, 0, 1, 1, 2049), (5, 1, 2, 1023, 2), (5, 0, 9, 1030, 2047),                         # 2049 and 2047 long across sample 2048; two samples across a tile
    (6, 2, 50, 3, 2500), (7, 3, 0, 0, 4100),                                               # the whole line
]


def hand_conversations(S, seed):
    """R = 2: 4100 samples on ``S`` tracks, and 4 samples - the last four of the corpus's last utterance - on min(S, 2) tracks."""
    rng = np.random.default_rng(seed)
    f = lambda: float(np.float32(rng.uniform(0.3, 1.7)))
    a = cv.make_conversation("a", 4100, S, [(u, st, p, ln, f(), f(), t) for t, u, st, p, ln in SEGMENTS if t < S])
    segs = [(5, 33, 0, 4, f(), f(), 0)] + ([(0, 4996, 1, 2, f(), f(), 1)] if S > 1 else [])
    return [a, cv.make_conversation("b", 4, min(S, 2), segs)]


@pytest.mark.parametrize("fmt", ["int16", "float32", "both"])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_render_is_the_restatement_bit_for_bit(fmt, S):
    corpus, utts = synthetic_corpus(fmt)
    convs = hand_conversations(S, seed=S)
    for c in convs:
        ref.check_schedule(c, lengths=corpus.lengths)
    want_mix, want_tracks, out_off = ref.render_ref(utts, convs)
    rd = cv.render(corpus, convs)
    assert rd.mix.shape == (4104,) and rd.tracks.shape == (S, 4104) and out_off.tolist() == [0, 4100, 4104] == rd.out_off.tolist()
    assert torch.equal(bits(rd.mix), bits(want_mix))
    assert torch.equal(bits(rd.tracks), bits(want_tracks))
    assert float(np.abs(want_mix).max()) > 0.1 and (S < 3 or not want_tracks[2].any())
    again = cv.render(corpus, convs)                              # two calls are bit-identical
    assert torch.equal(bits(again.mix), bits(rd.mix)) and torch.equal(bits(again.tracks), bits(rd.tracks))
    bare = cv.render(corpus, convs, tracks=False)                 # the same mixture without the track rows
    assert bare.tracks is None and torch.equal(bits(bare.mix), bits(rd.mix))
    assert torch.equal(bits(rd.mixture(1)), bits(want_mix[4100:])) and rd.tracks_of(1).shape == (min(S, 2), 4)
    assert torch.equal(bits(rd.tracks_of(0)), bits(want_tracks[:, :4100]))


def test_render_of_planned_conversations():
    """The planner's own schedules, three of them in one launch, on two and three tracks."""
    corpus, utts = synthetic_corpus("both")
    convs = [cv.plan_conversation(corpus, random.Random(s), seconds=1.5, speakers=2 + s % 2, overlap=(0.1, 0.6)) for s in range(3)]
    for c in convs:
        ref.check_schedule(c, max_active=2, lengths=corpus.lengths)
    want_mix, want_tracks, _ = ref.render_ref(utts, convs)
    rd = cv.render(corpus, convs)
    assert torch.equal(bits(rd.mix), bits(want_mix)) and torch.equal(bits(rd.tracks), bits(want_tracks))


def test_capture_replays_with_a_rewritten_table():
    """The launch inside a torch.cuda.graph; the device tables rewritten with other conversations of the same counts and replayed: the bits are
    the new tables'."""
    corpus, utts = synthetic_corpus("both")
    c0, c1 = hand_conversations(3, seed=1), hand_conversations(3, seed=2)
    moved = c1[0]._replace(place=np.where(c1[0].track == 1, c1[0].place - 1, c1[0].place).astype(np.int32),
                           start=(c1[0].start + 1).astype(np.int32), utt=np.where(c1[0].utt == 0, 3, c1[0].utt).astype(np.int32))
    c1 = [moved, c1[1]]
    ref.check_schedule(moved, lengths=corpus.lengths)
    table = cv.ConvTable(c0, DEV)
    mix = torch.zeros(table.total, device=DEV)
    tracks = torch.zeros(table.S_max, table.total, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cv.render_into(corpus, table, mix, tracks)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cv.render_into(corpus, table, mix, tracks)
    for convs in (c1, c0):
        words, out_off = table.pack(convs)
        table.words.copy_(torch.from_numpy(words))
        table.out_off.copy_(torch.from_numpy(out_off))
        graph.replay()
        torch.cuda.synchronize()
        want_mix, want_tracks, _ = ref.render_ref(utts, convs)
        assert torch.equal(bits(mix), bits(want_mix)) and torch.equal(bits(tracks), bits(want_tracks))
    assert not np.array_equal(ref.render_ref(utts, c0)[0], ref.render_ref(utts, c1)[0])


@pytest.mark.parametrize("C", [2, 3])
def test_segment_sisnr_against_the_oracle_in_float64(C):
    """Every case of ``conversation_ref.sisnr_problem`` within ``tol_db(n)`` of the oracle's ``_sisnr`` in float64 (the worst ratio is printed),
    on rows of ``ld > T`` floats; two calls are bit-identical, and so is a call on repacked rows."""
    pr = ref.sisnr_problem(C)
    T = pr["T"]
    want_v, want_vm = ref.sisnr_ref(pr["est"], pr["ref"], pr["mix"], pr["rows"], pr["begin"], pr["length"])
    est, rf, mix = (torch.from_numpy(pr[k]).to(DEV) for k in ("est", "ref", "mix"))
    v, vm = cv.segment_sisnr(est[:, :T], rf[:, :T], mix[:T], pr["rows"], pr["begin"], pr["length"])
    assert v.dtype == torch.float64 and v.shape == (len(pr["rows"]), C) and vm.shape == (len(pr["rows"]),)
    tol = np.array([ref.tol_db(int(n)) for n in pr["length"]])
    err = np.maximum(np.abs(v.cpu().numpy() - want_v).max(1), np.abs(vm.cpu().numpy() - want_vm))
    worst = int(np.argmax(err / tol))
    print(f"segment SI-SNR, C = {C}: worst error / tolerance {err[worst] / tol[worst]:.3g} ({err[worst]:.3g} dB at n = {pr['length'][worst]}, "
          f"{pr['family'][worst]})")
    assert np.all(np.isfinite(v.cpu().numpy())) and np.all(err <= tol), (worst, err[worst], tol[worst])
    v2, vm2 = cv.segment_sisnr(est[:, :T], rf[:, :T], mix[:T], pr["rows"], pr["begin"], pr["length"])
    assert torch.equal(v2.view(torch.int64), v.view(torch.int64)) and torch.equal(vm2.view(torch.int64), vm.view(torch.int64))
    v3, vm3 = cv.segment_sisnr(est[:, :T].contiguous(), rf[:, :T], mix[:T].clone(), pr["rows"], pr["begin"], pr["length"])
    assert torch.equal(v3.view(torch.int64), v.view(torch.int64)) and torch.equal(vm3.view(torch.int64), vm.view(torch.int64))


def test_a_planted_channel_swap_is_counted():
    """Tracks plus noise as the estimate, the two channels exchanged from sample 6000 on: the segments after the swap - the minority - are the
    switches, the assignment is the majority's."""
    corpus, utts = synthetic_corpus("both")
    f = np.float32(1.0)
    segs = [(0, 0, 0, 2500, f, f, 0), (3, 0, 2000, 2500, f, f, 1), (1, 100, 4600, 1300, f, f, 0), (4, 0, 6100, 2000, f, f, 1),
            (2, 0, 8000, 1996, f, f, 0)]
    conv = cv.make_conversation("swap", 10000, 2, segs)
    rd = cv.render(corpus, [conv])
    tr = rd.tracks_of(0)
    g = torch.Generator(device="cpu").manual_seed(3)
    est = tr + 0.01 * torch.randn(2, 10000, generator=g).to(DEV)
    est = torch.cat([est[:, :6000], est[[1, 0], 6000:]], dim=1)
    v, vm = cv.segment_sisnr(est, tr, rd.mixture(0), conv.track, conv.place, conv.len)
    s = cv.score(v, vm, np.zeros(5, int), conv.track, [2], 2, overlap=cv.overlap_fraction(conv))
    # sorted by (track, place): track 0 at 0, 4600, 8000, then track 1 at 2000, 6100
    assert conv.place.tolist() == [0, 4600, 8000, 2000, 6100]
    assert s["assignment"] == {0: (0, 1)} and s["assigned"].tolist() == [0, 0, 0, 1, 1]
    assert s["best"].tolist() == [0, 0, 1, 1, 0] and s["switch"].tolist() == [0, 0, 1, 0, 1] and s["switch_rate"] == 0.4
    assert s["sisnri_utt"] > s["sisnri_cons"] and np.all(v.cpu().numpy()[np.arange(5), s["best"]] > 15.0)
    assert [s["bins"][k]["n"] for k in cv.OVERLAP_BINS] == [1, 4, 0, 0]      # 4600 .. 5900 is the one stretch nobody else talks over


def test_evaluate_conversations_end_to_end(tmp_path):
    """``infer.evaluate_conversations`` on the smallest synthetic-weight model: its numbers and its csv equal ``score(segment_sisnr(...))`` computed
    here from ``separate_long``'s own output on the restatement's render; ``method="bank"`` scores the same segments with finite values.  The
    second conversation has three talkers for the model's two channels: no assignment there."""
    corpus, utts = synthetic_corpus("both")
    model = Model.from_config(VARIANTS["tiny"], init_seed=0).load_synthetic_(0).eval().to(DEV)
    convs = [cv.plan_conversation(corpus, random.Random(11), seconds=1.25, speakers=2),
             cv.plan_conversation(corpus, random.Random(12), seconds=1.3, speakers=3, max_active=3)]
    assert [c.n for c in convs] == [10000, 10400] and [c.S for c in convs] == [2, 3]
    kw = dict(chunk_seconds=0.5, overlap_seconds=0.125)
    path = str(tmp_path / "segments.csv")
    got = infer.evaluate_conversations(model, corpus, convs, method="long", csv_path=path, **kw)

    want_mix, want_tracks, out_off = ref.render_ref(utts, convs)
    mixes = [torch.from_numpy(want_mix[out_off[r]:out_off[r + 1]]).to(DEV) for r in range(2)]
    ests = longform.separate_long(model, mixes, **kw)
    vs, vms = [], []
    for r, c in enumerate(convs):
        tr = torch.from_numpy(np.ascontiguousarray(want_tracks[:c.S, out_off[r]:out_off[r + 1]])).to(DEV)
        v, vm = cv.segment_sisnr(torch.stack(list(ests[r])), tr, mixes[r], c.track, c.place, c.len)
        vs.append(v.cpu().numpy())
        vms.append(vm.cpu().numpy())
    v, vm = np.concatenate(vs), np.concatenate(vms)
    G = sum(len(c.utt) for c in convs)
    conv_of = np.concatenate([np.full(len(c.utt), r) for r, c in enumerate(convs)])
    want = cv.score(v, vm, conv_of, np.concatenate([c.track for c in convs]), [2, 3], 2,
                    overlap=np.concatenate([cv.overlap_fraction(c) for c in convs]))
    assert got["n"] == G == v.shape[0] and got["conversations"] == 2
    assert np.array_equal(got["v"], v) and np.array_equal(got["v_mix"], vm) and np.all(np.isfinite(v))
    for k in ("best", "assigned", "utt", "cons", "switch"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    for k in ("sisnri_utt", "sisnri_cons", "switch_rate"):
        assert got[k] == want[k] and np.isfinite(got[k]), k
    np.testing.assert_equal(got["bins"], want["bins"])           # (NaN where a bin holds no segment with an assignment)
    assert got["assignment"] == want["assignment"] and got["assignment"][1] is None
    assert np.isnan(got["cons"][conv_of == 1]).all() and not np.isnan(got["cons"][conv_of == 0]).any()
    rows = list(csv.reader(open(path, newline=""), quotechar="|"))
    assert len(rows) == G and all(len(r) == 10 + 2 for r in rows)
    g = 0
    for r, c in enumerate(convs):
        for k in range(len(c.utt)):
            row = rows[g]
            assert row[:6] == [c.key, str(k), str(int(c.track[k])), corpus.names[int(c.utt[k])], str(int(c.place[k])), str(int(c.len[k]))]
            assert float(row[6]) == want["overlap"][g] and int(row[7]) == want["best"][g] and int(row[8]) == want["assigned"][g]
            assert float(row[9]) == vm[g] and [float(x) for x in row[10:]] == v[g].tolist()
            g += 1

    bank = infer.evaluate_conversations(model, corpus, convs, method="bank", slots=4, **kw)
    assert bank["n"] == G and bank["v"].shape == (G, 2) and np.all(np.isfinite(bank["v"])) and np.all(np.isfinite(bank["v_mix"]))
    assert np.isfinite(bank["sisnri_utt"]) and np.array_equal(bank["v_mix"], vm)       # the mixture's scores do not depend on the separator
    with pytest.raises(ValueError):
        infer.evaluate_conversations(model, corpus, convs, method="whole")
