"""Graph-PIT and the conversation-window feed without a device: window schedules against the restatement of
tests/graphpit_ref.py, the epoch's reproducibility, the colourability condition, and the argument checks and workspace size of the three C
entries (the library loads without a GPU; every check returns before any HIP call)."""
import ctypes
import functools
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conversation_rooms_ref as rref                                        # noqa: E402
import dynmix_ref as dr                                                      # noqa: E402
import graphpit_ref as gref                                                  # noqa: E402

from sepreformer_amd import conversation as cv                               # noqa: E402
from sepreformer_amd import convfeed as cf                                   # noqa: E402
from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402
from sepreformer_amd import trainer as T_                                    # noqa: E402

T, U = 8000, 8


def host_corpus():
    arrays = rref.corpus_arrays("both", noise=True)
    corpus = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    corpus.roles = rref.roles_of(arrays)
    utts = [arrays[nm] for nm in corpus.names]
    corpus.set_energies(np.array([dr.energy(a) for a in utts[:corpus.n16]], dtype=np.int64),
                        np.array([dr.energy(a) for a in utts[corpus.n16:]], dtype=np.float64))
    return corpus


def hand_bank():
    return rv.RirBank.from_arrays(rref.hand_bank(), 8000, device=None, normalise=None)


def planned(corpus, count, bank=None, noise=None, seconds=60.0, max_active=2):
    return [cv.plan_conversation(corpus, random.Random(100 + i), seconds=seconds, roles=("s1",), speakers=3, max_active=max_active, rirs=bank,
                                 noise=noise) for i in range(count)]


def check_window(conv, w0, rows):
    """``window_schedule`` against ``window_ref``: rows, spans, mask and the schedule's columns; returns the window (or None)."""
    w, ref = cf.window_schedule(conv, w0, T, rows), gref.window_ref(conv, w0, T, rows)
    assert (w is None) == (ref is None)
    if w is None:
        return None
    assert w.used == ref.used and w.spans.tolist() == [list(s) for s in ref.spans] and w.adj.tolist() == ref.adj
    c = w.conv
    assert c.n == T and c.S == rows and c.bed == conv.bed
    want = sorted(ref.segs, key=lambda s: (rows if s[0] == "bed" else s[0], s[2]))
    if want:
        assert c.track.tolist() == [rows if s[0] == "bed" else s[0] for s in want] and c.place.tolist() == [s[2] for s in want]
        g = [s[1] for s in want]
        for f in ("utt", "start", "len"):
            assert getattr(c, f).tolist() == getattr(conv, f)[g].tolist()
        assert np.array_equal(c.norm, conv.norm[g]) and np.array_equal(c.gain, conv.gain[g])
        if conv.rir is not None:
            assert all(np.array_equal(getattr(c, f), getattr(conv, f)[g]) for f in ("rir", "taps", "direct"))
    else:                                                                     # silence: one segment that ends, tail and all, before the window
        assert len(c.utt) == 1 and int(c.place[0]) + int(c.len[0]) + (1 if c.taps is None else int(c.taps[0])) - 1 <= 0
    return w


@pytest.mark.parametrize("rooms", [False, True])
def test_window_schedules_of_planned_conversations(rooms):
    corpus = host_corpus()
    bank = hand_bank() if rooms else None
    seen = {"tail_rides": 0, "tail_alone": 0, "two_rows_one_talker": 0, "dropped": 0, "begins_inside": 0}
    for conv in planned(corpus, 4, bank, noise="noise" if rooms else None):
        rows = cf.window_rows(U, bool(conv.bed))
        assert rows == (7 if rooms else 8)
        for w0 in cf.window_starts(conv.n, 1236, T):
            w = check_window(conv, w0, rows)
            if w is None:
                seen["dropped"] += 1
                continue
            c = w.conv
            talk = c.track < rows
            if conv.bed:                                                      # the bed covers the window without a gap, on the track after the rows
                b = ~talk
                assert int(c.place[b][0]) <= 0 and int((c.place[b] + c.len[b])[-1]) >= T
                assert np.array_equal(c.place[b][1:], (c.place[b] + c.len[b])[:-1])
            direct = np.ones(len(c.utt), dtype=np.int64) if c.direct is None else c.direct
            tail_only = talk & (c.place.astype(np.int64) + c.len + direct - 1 <= 0)
            for g in np.nonzero(tail_only)[0]:
                u = int(c.track[g])
                mates = np.nonzero(talk & (c.track == u) & ~tail_only)[0]
                seen["tail_rides" if len(mates) else "tail_alone"] += 1
                assert (w.spans[u].tolist() == [0, 0]) == (len(mates) == 0)
                assert all(conv.track[np.nonzero(conv.utt == c.utt[m])[0][0]] == w.talker[u] for m in mates)
            tk = w.talker[:w.used].tolist()
            assert tk == sorted(tk) and all(t == -1 for t in w.talker[w.used:])
            seen["two_rows_one_talker"] += len(tk) != len(set(tk))
            seen["begins_inside"] += bool((c.place[talk] < 0).any())
            for u in range(w.used):                                          # no row talks over another row of its own talker
                for v in range(w.used):
                    assert not ((w.adj[u] >> v) & 1 and tk[u] == tk[v])
    print(seen)
    assert seen["two_rows_one_talker"] and seen["begins_inside"] and (not rooms or (seen["tail_rides"] and seen["tail_alone"])), seen


def test_tail_only_rule_and_limit_by_hand():
    """Talker 0: a segment that ended 100 samples before the window under 1025 taps, direct 1, then nothing; talker 1: one that ended before
    the window (tail only) and a later one inside it.  The first gets a row of silence, the second rides on its talker's row."""
    f = np.float32(1.0)
    segs = [(0, 0, 0, 400, f, f, 0), (1, 0, 100, 300, f, f, 1), (2, 0, 1200, 800, f, f, 1), (3, 0, 900, 500, f, f, 2)]
    conv = cv.make_conversation("hand", 4000, 3, segs, rooms=[(4, 1025, 1), (4, 1025, 1), (4, 1025, 10), (-1, 1, 1)])
    w = check_window(conv, 500, 8)
    assert w.used == 3 and w.talker[:3].tolist() == [0, 1, 2]
    assert w.spans[:3].tolist() == [[0, 0], [700, 1509], [400, 900]] and w.conv.track.tolist() == [0, 1, 1, 2]
    assert w.adj[:3].tolist() == [0, 0b100, 0b010]                             # dry [700, 1500) meets dry [400, 900)
    assert cf.window_schedule(conv, 500, T, 2) is None and gref.window_ref(conv, 500, T, 2) is None
    far = check_window(conv, 3600, 8)                                          # nothing reaches it: silence
    assert far.used == 0 and not far.adj.any()


def make_feed(corpus, **kw):
    kw.setdefault("planner", functools.partial(cv.plan_conversation, roles=("s1",), speakers=3, max_active=2))
    return cf.ConversationWindowFeed(corpus, batch=3, max_len=T, channels=2, conversations=3, seconds=20.0, seed=5, **kw)


def test_epoch_is_reproducible_from_the_state():
    corpus = host_corpus()
    feed = make_feed(corpus)
    assert feed.fixed_length and feed.batch == 3 and feed.max_len == T and feed.rows == 8
    first = list(feed.plans())
    state = feed.state_dict()
    second = list(feed.plans())
    assert first and second and [p.keys for p in first] != [p.keys for p in second]
    for p in first:
        assert p.spans.shape == (3, 8, 2) and p.spans.dtype == np.int32 and p.adj.shape == (3, 8) and len(p.keys) == 3 and p.n.tolist() == [T] * 3
    again = make_feed(corpus)
    again.load_state_dict(state)
    third = list(again.plans())
    assert again.epoch == feed.epoch == 2
    assert [p.keys for p in third] == [p.keys for p in second]
    assert all(np.array_equal(a.spans, b.spans) and np.array_equal(a.adj, b.adj) for a, b in zip(third, second))
    assert all(all(np.array_equal(x, y) for x, y in zip(wa.conv, wb.conv)) for a, b in zip(third, second) for wa, wb in zip(a.windows, b.windows))
    # the windows of the epoch: every conversation's windows at one offset, a multiple of 4, the partial batch dropped
    starts = {}
    for p in first:
        for k in p.keys:
            name, _, w0 = k.partition("@")
            starts.setdefault(name, []).append(int(w0))
    for name, ws in starts.items():
        assert len({w % T for w in ws}) == 1 and ws[0] % 4 == 0
    small = make_feed(corpus, rows=2)
    n = sum(len(p.keys) for p in small.plans())
    assert small.dropped > 0 and small.rows == 2 and n < sum(len(p.keys) for p in first)
    with pytest.raises(ValueError, match="max_active"):
        make_feed(corpus, planner=functools.partial(cv.plan_conversation, roles=("s1",), speakers=3, max_active=3))
    assert make_feed(corpus, planner=functools.partial(cv.plan_conversation, roles=("s1",), speakers=3, noise="noise")).rows == 7


@pytest.mark.parametrize("rooms", [False, True])
def test_every_window_has_a_colouring(rooms):
    """With ``max_active <= channels`` the restatement finds a valid colouring for EVERY window of 20 planned conversations (``speakers=3``, 60
    seconds): a condition, not a tolerance.  The estimates are zeros - validity does not depend on them."""
    corpus = host_corpus()
    bank = hand_bank() if rooms else None
    count = 0
    for conv in planned(corpus, 20, bank):
        for w0 in cf.window_starts(conv.n, 2000, T):
            w = cf.window_schedule(conv, w0, T, 32)                            # no window dropped: the condition holds for every one
            live = [bool(s[1] > s[0]) for s in w.spans]
            ed = gref.edges(w.adj, live, 32)
            used = [u for u in range(32) if live[u]]
            ok = False
            for cols in __import__("itertools").product(range(2), repeat=len(used)):
                col = dict(zip(used, cols))
                if all(col[u] != col[v] for u, v in ed):
                    ok = True
                    break
            assert ok, (conv.key, w0)
            count += 1
    assert count >= 20 * 58


def test_a_triangle_has_no_colouring_with_two_channels():
    est, rows = np.zeros((2, 8), dtype=np.float32), np.ones((3, 8), dtype=np.float32)
    out = gref.assign(est, rows, [(0, 8)] * 3, [0b110, 0b101, 0b011])
    assert out["status"] == 1 and out["col"] == [0, 0, 0] and np.isnan(out["value"])
    assert gref.assign(np.zeros((3, 8), dtype=np.float32), rows, [(0, 8)] * 3, [0b110, 0b101, 0b011])["status"] == 0


# ---- the C entries --------------------------------------------------------------------------------------------------------------------------
def test_bytes_against_the_dry_layout():
    lib = L.load()
    for C_ in range(0, 5):
        for U_ in range(0, 10):
            for B in (0, 1, 3, 16, 65535, 65536):
                assert int(lib.sepr_graph_pit_bytes(C_, U_, B)) == gref.dry_layout_bytes(C_, U_, B), (C_, U_, B)
    assert int(lib.sepr_graph_pit_bytes(2, 8, 16)) == 8192 and int(lib.sepr_graph_pit_bytes(-1, 8, 16)) == 0


def _ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def test_argument_checks_return_before_any_hip_call():
    """Fake, well-aligned addresses: every refusal is made on the arguments alone, so nothing is dereferenced and no device is needed."""
    lib = L.load()
    A = 0x10000
    good = dict(est=_ptrs([A, A]), rows=_ptrs([A] * 8), spans=A, adj=A, C=2, U=8, B=3, T=2052, eps=1e-8, snr=30.0, col=A, value=A, status=A, ws=A,
                nbytes=1 << 20)

    def assign(**kw):
        a = dict(good, **kw)
        return lib.sepr_graph_pit_assign(a["est"], a["rows"], a["spans"], a["adj"], a["C"], a["U"], a["B"], a["T"], a["eps"], a["snr"], a["col"],
                                         a["value"], a["status"], a["ws"], a["nbytes"], None)

    bad = [dict(est=None), dict(rows=None), dict(spans=None), dict(adj=None), dict(col=None), dict(value=None), dict(status=None),
           dict(C=0), dict(C=4), dict(U=0), dict(U=9), dict(B=0), dict(B=65536), dict(T=0), dict(T=2), dict(T=2050), dict(T=-4),
           dict(eps=-1.0), dict(eps=float("nan")), dict(snr=-1.0), dict(snr=float("inf")), dict(snr=float("nan")),
           dict(est=_ptrs([A, 0])), dict(est=_ptrs([A, A + 2])), dict(rows=_ptrs([A] * 7 + [0])), dict(rows=_ptrs([A + 1] + [A] * 7)),
           dict(spans=A + 2), dict(adj=A + 1), dict(col=A + 2), dict(status=A + 3), dict(value=A + 4)]
    for kw in bad:
        assert assign(**kw) == L.SEPR_EINVAL, kw
    need = int(lib.sepr_graph_pit_bytes(2, 8, 3))
    assert assign(nbytes=need - 1) == L.SEPR_EWORKSPACE and assign(ws=None) == L.SEPR_EWORKSPACE and assign(nbytes=0) == L.SEPR_EWORKSPACE

    good2 = dict(rows=_ptrs([A] * 8), spans=A, col=A, C=2, U=8, B=3, T=2052, out=_ptrs([A, A]))

    def assemble(**kw):
        a = dict(good2, **kw)
        return lib.sepr_graph_pit_assemble(a["rows"], a["spans"], a["col"], a["C"], a["U"], a["B"], a["T"], a["out"], None)

    bad2 = [dict(rows=None), dict(spans=None), dict(col=None), dict(out=None), dict(C=0), dict(C=4), dict(U=0), dict(U=9), dict(B=0), dict(T=0),
            dict(T=2050), dict(rows=_ptrs([A] * 7 + [0])), dict(rows=_ptrs([A + 4] + [A] * 7)), dict(out=_ptrs([A, 0])), dict(out=_ptrs([A, A + 8])),
            dict(spans=A + 2), dict(col=A + 1)]
    for kw in bad2:
        assert assemble(**kw) == L.SEPR_EINVAL, kw


def test_trainer_knows_the_criterion():
    assert "graph_sasdr" in T_.CRITERIA
    T_.check_criterion("graph_sasdr", 0.0, rows=8)
    T_.check_criterion("sasdr", 0.5)
    with pytest.raises(ValueError, match="rows"):
        T_.check_criterion("graph_sasdr", 0.0)
    with pytest.raises(ValueError, match="graph_sasdr"):
        T_.check_criterion("sasdr", 0.0, rows=8)
    with pytest.raises(ValueError, match="SI-SNR"):
        T_.check_criterion("graph_sisnr", 0.0, rows=8)
    T_.check_resume_criterion("graph_sasdr", {"criterion": "graph_sasdr"})
    with pytest.raises(ValueError, match="criterion"):
        T_.check_resume_criterion("graph_sasdr", {"criterion": "sasdr"})


def test_the_restatement_ties_to_the_trusted_criterion():
    """U = C rows over all T, every pair adjacent: the restatement's value is tests/sasdr_ref.py's loss and its colouring the inverse of the
    permutation (row u on channel col[u]; perm[s] = the target of estimate s)."""
    import torch
    import sasdr_ref as sr
    rng = np.random.default_rng(3)
    for C_ in (2, 3):
        tgt = rng.normal(0, 0.1, size=(C_, 1, 516)).astype(np.float32)
        est = (tgt[::-1] + rng.normal(0, 0.03, size=tgt.shape)).astype(np.float32)
        loss, perm, _ = sr.sasdr_time(torch.from_numpy(est.copy()), torch.from_numpy(tgt))
        full = (1 << C_) - 1
        out = gref.assign(est[:, 0], tgt[:, 0], [(0, 516)] * C_, [full & ~(1 << u) for u in range(C_)])
        assert abs(out["value"] - float(loss[0])) < 1e-9
        assert [out["col"][int(perm[0, s])] for s in range(C_)] == list(range(C_))
