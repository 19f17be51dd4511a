"""Graph-PIT on the device: ``sepr_graph_pit_assign`` / ``sepr_graph_pit_assemble`` against the float64 restatement of
tests/graphpit_ref.py on constructed inputs and edges, the tie to the trusted SA-SDR criterion, the window render of
``ConversationWindowFeed`` against the whole conversation's render and the numpy restatement, both entries under graph capture, and
``Trainer(criterion="graph_sasdr")`` end to end.

Shapes: T = 2052 (a multiple of 4, not of 256: the strided sums have ragged tails), B = 3, U = 8 with 5 live rows, C in {2, 3}.  Target rows
hold NaN outside their spans: a kernel that read a row outside its span would show it in every figure.

Tolerance of ``value``: 1e-6 dB.  The float64 moment form loses about ``T 2^-52 ee / E``, roughly 7e-9 relative at 30 dB; the bound leaves a
factor of about 30 over that.  ``col`` must be equal wherever the restatement's gap between the best and the second-best E is at least 1e-3 dB,
which the inputs are built to satisfy and which is asserted on the restatement first."""
import functools
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conversation_rooms_ref as rref                                        # noqa: E402
import graphpit_ref as gref                                                  # noqa: E402
import sasdr_ref as sr                                                       # noqa: E402

from sepreformer_amd import conversation as cv                               # noqa: E402
from sepreformer_amd import convfeed as cf                                   # noqa: E402
from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402
from sepreformer_amd.criterion import PIT_SASDR_time, PIT_SISNR_mag, PIT_SISNR_time, GraphPIT      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, B, U = 2052, 3, 8
TOL_DB, GAP_DB = 1e-6, 1e-3
_cache = {}


def bits(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().contiguous().view(torch.int32)


def overlap_adj(spans):
    """adj [B][U] from span overlap: rows whose spans intersect may not share a channel."""
    Bn, Un = len(spans), len(spans[0])
    adj = np.zeros((Bn, Un), dtype=np.int64)
    for b in range(Bn):
        for u in range(Un):
            for v in range(Un):
                if u != v and max(spans[b][u][0], spans[b][v][0]) < min(spans[b][u][1], spans[b][v][1]):
                    adj[b, u] |= 1 << v
    return adj


def make_rows(spans, seed, Tn=T, poison=True):
    """rows [U, B, T] float32: noise inside each span, NaN outside it."""
    rng = np.random.default_rng(seed)
    Bn, Un = len(spans), len(spans[0])
    rows = np.full((Un, Bn, Tn), np.nan if poison else 0.0, dtype=np.float32)
    for b in range(Bn):
        for u in range(Un):
            on, off = gref.clamp_span(spans[b][u][0], spans[b][u][1], Tn)
            rows[u, b, on:off] = rng.normal(0.01, 0.1, size=off - on).astype(np.float32)
    return rows


def estimates(rows, spans, hidden, C, snr_db, seed):
    """est [C, B, T]: the assembled targets of the hidden colouring plus noise at ``snr_db[b]`` dB (float32)."""
    rng = np.random.default_rng(seed)
    Un, Bn, Tn = rows.shape
    est = np.zeros((C, Bn, Tn), dtype=np.float32)
    for b in range(Bn):
        tg = gref.assemble(rows[:, b], spans[b], hidden[b], C)
        p = float((tg.astype(np.float64) ** 2).mean()) or 1e-4
        noise = rng.normal(0, 1, size=tg.shape) * math.sqrt(p * 10.0 ** (-snr_db[b] / 10.0))
        est[:, b] = (tg + noise).astype(np.float32)
    return est


def run_device(est, rows, spans, adj, C):
    """-> (graph, col [B, U], value [B], status [B], targets [C, B, T]) from one ``GraphPIT`` call."""
    Un, Bn, Tn = rows.shape
    g = GraphPIT(DEV, C, Un, Bn, Tn)
    g.load(spans, adj)
    e = [torch.from_numpy(np.ascontiguousarray(est[c])).to(DEV) for c in range(C)]
    r = [torch.from_numpy(np.ascontiguousarray(rows[u])).to(DEV) for u in range(Un)]
    out = g(e, r)
    torch.cuda.synchronize()
    g._keep = (e, r)
    return g, g.col.cpu().numpy(), g.value.cpu().numpy(), g.status.cpu().numpy(), torch.stack(out).cpu().numpy()


def check(est, rows, spans, adj, C, expect_col=None, need_gap=True):
    """One device call against the restatement, example by example; returns the restatement's results."""
    Un, Bn, Tn = rows.shape
    g, col, value, status, tg = run_device(est, rows, spans, adj, C)
    refs = []
    for b in range(Bn):
        ref = gref.assign(est[:, b], rows[:, b], spans[b], adj[b])
        refs.append(ref)
        print(f"b={b} ref col {ref['col']} dev col {col[b].tolist()} ref value {ref['value']!r} dev value {float(value[b])!r} gap {ref['gap_db']:.3e} dB")
        if need_gap:
            assert ref["gap_db"] >= GAP_DB, (b, ref["gap_db"])                 # the inputs are what the test says they are
        if expect_col is not None:
            assert ref["col"] == list(expect_col[b]), (b, ref["col"])
        assert int(status[b]) == ref["status"]
        if ref["gap_db"] >= GAP_DB:
            assert col[b].tolist() == ref["col"], b
        if ref["status"]:
            assert math.isnan(float(value[b])) and not col[b].any()
        else:
            assert abs(float(value[b]) - ref["value"]) <= TOL_DB, (b, float(value[b]), ref["value"])
        want = gref.assemble(rows[:, b], spans[b], col[b], C)
        assert np.array_equal(bits(tg[:, b]).numpy(), bits(want).numpy()), b
    again = torch.stack(g(*g._keep)).cpu().numpy()                             # two calls give equal bits
    torch.cuda.synchronize()
    assert np.array_equal(bits(again).numpy(), bits(tg).numpy())
    assert np.array_equal(g.col.cpu().numpy(), col) and np.array_equal(g.value.cpu().numpy().view(np.int64), value.view(np.int64))
    return g, refs


# five live rows (0, 2, 3, 5, 6) of eight; the spans move by b so that they start at 1, 2 and 3 modulo 4 as well
def main_spans(C):
    out = []
    for b in range(B):
        if C == 2:                                    # a path: 0 - 2 - 3 - 5 - 6
            live = {0: (0, 900 + b), 2: (500 + b, 1400), 3: (1001 + b, 1800), 5: (1500 + b, T), 6: (1802 + b, 2051)}
        else:                                         # a triangle 0 - 2 - 3, then 3 - 5 - 6
            live = {0: (0, 1200), 2: (401 + b, 1500), 3: (802 + b, 1900), 5: (1500 + b, T), 6: (1803 + b, T)}
        out.append([live.get(u, (77 * u, 77 * u)) for u in range(U)])
    return out


HIDDEN = {2: [0, 0, 1, 0, 0, 1, 0, 0], 3: [1, 0, 2, 0, 0, 1, 2, 0]}


@pytest.mark.parametrize("C", [2, 3])
def test_assign_and_assemble_against_the_restatement(C):
    """The estimates are a hidden valid colouring's assembled targets plus noise at 0, 10 and 25 dB."""
    spans = main_spans(C)
    adj = overlap_adj(spans)
    rows = make_rows(spans, seed=C)
    hidden = [HIDDEN[C]] * B
    est = estimates(rows, spans, hidden, C, (0.0, 10.0, 25.0), seed=10 + C)
    g, refs = check(est, rows, spans, adj, C, expect_col=hidden)
    assert [r["status"] for r in refs] == [0] * B and all(len(r["all"]) >= 2 for r in refs)
    # assemble under other colourings written into col, valid or not, garbage values included: bit for bit, clamped into [0, C)
    rng = np.random.default_rng(5)
    for trial in range(4):
        col = rng.integers(0, C, size=(B, U)).astype(np.int32) if trial < 3 else np.array([[-1, 9, 0, 1, 2, 3, -7, 1]] * B, dtype=np.int32)
        g.col.copy_(torch.from_numpy(col))
        tg = torch.stack(g.assemble(g._keep[1])).cpu().numpy()
        for b in range(B):
            assert np.array_equal(bits(tg[:, b]).numpy(), bits(gref.assemble(rows[:, b], spans[b], col[b], C)).numpy()), (trial, b)


def test_edges_of_the_spans():
    """A row over all of T, a span of one sample, spans that start at 1, 2 and 3 modulo 4, empty rows (on = off inside, at 0 and at T)."""
    spans = [[(0, T), (777 + b, 778 + b), (1, 500), (1002, 1500), (1503, 2051), (0, 0), (100, 100), (T, T)] for b in range(B)]
    adj = overlap_adj(spans)
    rows = make_rows(spans, seed=21)
    hidden = [[0, 1, 1, 1, 1, 0, 0, 0]] * B
    est = estimates(rows, spans, hidden, 2, (5.0, 15.0, 25.0), seed=22)
    check(est, rows, spans, adj, 2, expect_col=hidden)


def test_all_rows_empty():
    spans = [[(5 * u, 5 * u) for u in range(U)]] * B
    rows = make_rows(spans, seed=1)
    est = np.random.default_rng(2).normal(0, 0.1, size=(2, B, T)).astype(np.float32)
    adj = np.full((B, U), 0xFF, dtype=np.int64)                                # bits between silent rows count for nothing
    g, refs = check(est, rows, spans, adj, 2, expect_col=[[0] * U] * B, need_gap=False)
    for b in range(B):
        e = est[:, b].astype(np.float64)
        E = sum(math.fsum((e[c] * e[c]).tolist()) - math.fsum(e[c].tolist()) ** 2 / T for c in range(2))
        assert abs(refs[b]["value"] - 10.0 * math.log10((E + gref.EPS) / gref.EPS)) < 1e-9
        assert abs(float(g.value[b]) - 10.0 * math.log10((E + gref.EPS) / gref.EPS)) <= TOL_DB
    assert not torch.stack(g.targets).cpu().view(torch.int32).any()            # +0.0 in every bit


@pytest.mark.parametrize("C", [1, 2, 3])
def test_one_row(C):
    spans = [[(3 + b, 1999)] for b in range(B)]
    rows = make_rows(spans, seed=31)
    hidden = [[C - 1]] * B
    est = estimates(rows, spans, hidden, C, (0.0, 10.0, 25.0), seed=32)
    check(est, rows, spans, np.zeros((B, 1), dtype=np.int64), C, expect_col=hidden, need_gap=C > 1)


def test_tie_goes_to_the_first_colouring():
    """Rows 0 and 1 are the same samples on the same span and not adjacent; the estimates carry one of them on each channel.  Swapping the two
    gives the same E in every bit - the same moments, added in the same order - and the lexicographically first colouring wins, whichever
    way round the estimates were built."""
    spans = [[(101, 1300), (101, 1300), (1000, 2000)] + [(0, 0)] * 5] * B          # row 2 overlaps both: the Gram terms take part in the tie
    rows = make_rows(spans, seed=41)
    rows[1] = rows[0]
    adj = np.zeros((B, U), dtype=np.int64)
    for hidden in ([0, 1, 1] + [0] * 5, [1, 0, 0] + [0] * 5):
        est = estimates(rows, spans, [hidden] * B, 2, (10.0, 20.0, 25.0), seed=42)
        g, refs = check(est, rows, spans, adj, 2, need_gap=False)
        want = [0, 1, 1] + [0] * 5 if hidden[0] == 0 else [0, 1, 0] + [0] * 5
        for b in range(B):
            es = [e for e, c in refs[b]["all"]]
            assert es.count(min(es)) == 2                                      # an exact tie in the restatement
            assert refs[b]["col"] == want and g.col[b].tolist() == want


def test_triangle_with_two_channels_has_no_colouring():
    spans = [[(0, 1000), (500, 1500), (900, 2000)] + [(0, 0)] * 5, [(0, 1000), (500, 1500), (1000, 2000)] + [(0, 0)] * 5,
             [(0, 1000), (500, 1500), (900, 2000)] + [(0, 0)] * 5]
    adj = overlap_adj(spans)
    for u in range(U):
        adj[:, u] &= ~((1 << (u + 1)) - 1)                                     # every edge named by its lower row only: still an edge
    rows = make_rows(spans, seed=51)
    est = estimates(rows, spans, [[0, 1, 0] + [0] * 5] * B, 2, (10.0, 10.0, 10.0), seed=52)
    g, refs = check(est, rows, spans, adj, 2, need_gap=False)
    assert [r["status"] for r in refs] == [1, 0, 1] and g.status.tolist() == [1, 0, 1]
    assert math.isnan(float(g.value[0])) and not g.col[0].any() and g.col[1].tolist() == [0, 1, 0] + [0] * 5


def test_all_colourings_of_eight_rows():
    """U = 8 live rows, C = 3, no edge: 3^8 = 6561 colourings, more than one per thread."""
    spans = [[(100 * u + 1, 100 * u + 1000) for u in range(U)]]
    rows = make_rows(spans, seed=61)
    hidden = [[2, 0, 1, 1, 0, 2, 2, 1]]
    est = estimates(rows, spans, hidden, 3, (15.0,), seed=62)
    g, refs = check(est, rows, spans, np.zeros((1, U), dtype=np.int64), 3, expect_col=hidden)
    assert len(refs[0]["all"]) == 3 ** 8


def test_bad_tables_stay_inside_the_buffers():
    """``on > off``, ``off > T``, negative and huge values, adjacency words with every bit set: the results are the restatement's under the
    header's clamps, and the bytes around every output are untouched."""
    big = 2 ** 31 - 1
    spans = [[(900, 100), (-50, 300), (1000, T + 999), (-big, -1), (big, big), (2000, -big), (T - 1, big), (T, 0)],
             [(0, big), (-big, big), (5, 4), (T + 1, T + 2), (1, 2), (-1, 0), (big, -big), (700, 701)],
             [(T // 2, T // 2 + 1), (0, 0), (-big - 1, big), (3, 3), (big, 0), (1, T), (2, T), (3, T)]]
    clamped = [[gref.clamp_span(on, off, T) for on, off in row] for row in spans]
    rows = make_rows(clamped, seed=71, poison=False)
    est = np.random.default_rng(72).normal(0, 0.1, size=(3, B, T)).astype(np.float32)
    adj = np.array([[0xFFFFFFFF] * U, [0] * U, [0xFFFFFF00] * U], dtype=np.int64)
    C = 3
    pad = 1024
    g = GraphPIT(DEV, C, U, B, T)
    # the outputs re-seated inside guarded blocks
    blocks = {}
    for name, t in (("col", g.col), ("value", g.value), ("status", g.status)):
        blk = torch.full((pad + t.numel() * t.element_size() + pad,), 0x5A, dtype=torch.uint8, device=DEV)
        blocks[name] = blk
        setattr(g, name, blk[pad:pad + t.numel() * t.element_size()].view(t.dtype).view(t.shape))
    tblk = torch.full((C, pad + B * T + pad), float("nan"), dtype=torch.float32, device=DEV)
    tblk.view(torch.int32).fill_(0x5A5A5A5A)
    g.targets = [tblk[c, pad:pad + B * T].view(B, T) for c in range(C)]
    g.load(np.array(spans, dtype=np.int64), adj)
    e = [torch.from_numpy(est[c].copy()).to(DEV) for c in range(C)]
    r = [torch.from_numpy(rows[u].copy()).to(DEV) for u in range(U)]
    out = g(e, r)
    torch.cuda.synchronize()
    for b in range(B):
        ref = gref.assign(est[:, b], rows[:, b], spans[b], adj[b])
        print(b, ref["col"], g.col[b].tolist(), ref["value"], float(g.value[b]), ref["gap_db"])
        assert int(g.status[b]) == ref["status"]
        if ref["status"] == 0:
            assert abs(float(g.value[b]) - ref["value"]) <= TOL_DB
            if ref["gap_db"] >= GAP_DB:
                assert g.col[b].tolist() == ref["col"]
        want = gref.assemble(rows[:, b], spans[b], g.col[b].cpu().numpy(), C)
        assert np.array_equal(bits(torch.stack([o[b] for o in out])).numpy(), bits(want).numpy())
    for name, blk in blocks.items():
        assert bool((blk[:pad] == 0x5A).all()) and bool((blk[-pad:] == 0x5A).all()), name
    guard = tblk.view(torch.int32)
    assert bool((guard[:, :pad] == 0x5A5A5A5A).all()) and bool((guard[:, -pad:] == 0x5A5A5A5A).all())


@pytest.mark.parametrize("C", [2, 3])
def test_tie_to_the_trusted_criterion(C):
    """U = C rows over all of T, every pair adjacent: ``value`` is tests/sasdr_ref.py's loss within the same 1e-6 dB, and with the identity as
    the hidden colouring the SA-SDR loss on the assembled targets is the loss on the rows bit for bit."""
    rng = np.random.default_rng(80 + C)
    tgt = rng.normal(0, 0.1, size=(C, B, T)).astype(np.float32)
    spans = [[(0, T)] * C] * B
    full = (1 << C) - 1
    adj = np.array([[full & ~(1 << u) for u in range(C)]] * B, dtype=np.int64)
    for hidden in (list(range(C)), list(range(C))[::-1]):
        est = estimates(tgt, spans, [hidden] * B, C, (0.0, 10.0, 25.0), seed=90)
        g, refs = check(est, tgt, spans, adj, C, expect_col=[hidden] * B)
        loss, perm, _ = sr.sasdr_time(torch.from_numpy(est), torch.from_numpy(tgt))
        for b in range(B):
            assert abs(float(g.value[b]) - float(loss[b])) <= TOL_DB
            assert [int(g.col[b, int(perm[b, s])]) for s in range(C)] == list(range(C))
    crit = PIT_SASDR_time(DEV, C)
    e = [torch.from_numpy(est[c].copy()).to(DEV) for c in range(C)]
    est_id = estimates(tgt, spans, [list(range(C))] * B, C, (0.0, 10.0, 25.0), seed=91)
    e = [torch.from_numpy(est_id[c].copy()).to(DEV) for c in range(C)]
    r = [torch.from_numpy(tgt[u].copy()).to(DEV) for u in range(C)]
    g = GraphPIT(DEV, C, C, B, T)
    g.load(spans, adj)
    sizes = torch.full((B,), float(T))
    a = crit(estims=e, input_sizes=sizes, target_attr=g(e, r))
    b_ = crit(estims=e, input_sizes=sizes, target_attr=r)
    assert g.col.tolist() == [list(range(C))] * B and torch.equal(bits(a.reshape(1)), bits(b_.reshape(1)))
    for c in (PIT_SISNR_time(DEV, C, True), PIT_SISNR_mag(DEV, 512, 128, "hann", 2, C, True, False)):
        with pytest.raises(ValueError, match="SA-SDR|SASDR"):
            GraphPIT.check_pair(c)
    GraphPIT.check_pair(crit)


def test_replay_from_a_captured_graph():
    """Both entries captured once; ``load`` then rewrites ``spans`` and ``adj`` and the replay gives the bits of an eager call on those tables."""
    C = 2
    first, second = main_spans(2), [[(0, T), (777, 778), (1, 500), (1002, 1500), (1503, 2051), (0, 0), (100, 100), (T, T)]] * B
    rows = make_rows([[(0, T)] * U] * B, seed=95, poison=False)                # the same samples under both tables
    est = np.random.default_rng(96).normal(0, 0.1, size=(C, B, T)).astype(np.float32)
    e = [torch.from_numpy(est[c].copy()).to(DEV) for c in range(C)]
    r = [torch.from_numpy(rows[u].copy()).to(DEV) for u in range(U)]

    def eager(spans):
        g = GraphPIT(DEV, C, U, B, T)
        g.load(spans, overlap_adj(spans))
        out = torch.stack(g(e, r)).clone()
        torch.cuda.synchronize()
        return g.col.clone(), g.value.clone(), g.status.clone(), out

    g = GraphPIT(DEV, C, U, B, T)
    g.load(first, overlap_adj(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g(e, r)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = g(e, r)
    results = []
    for spans in (second, first):
        g.load(spans, overlap_adj(spans))
        graph.replay()
        torch.cuda.synchronize()
        col, value, status, tg = eager(spans)
        assert torch.equal(g.col, col) and torch.equal(g.value.view(torch.int64), value.view(torch.int64)) and torch.equal(g.status, status)
        assert torch.equal(bits(torch.stack(out)), bits(tg))
        results.append(g.col.clone())
    assert not torch.equal(results[0], results[1])                            # the two tables do ask for different answers


# ---- the window render ----------------------------------------------------------------------------------------------------------------------
def synthetic_corpus():
    if "corpus" not in _cache:
        arrays = rref.corpus_arrays("both", noise=True)
        corpus = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
        corpus.roles = rref.roles_of(arrays)
        _cache["corpus"] = (corpus, [arrays[nm] for nm in corpus.names])
    return _cache["corpus"]


def hand_bank():
    if "bank" not in _cache:
        hs = rref.hand_bank()
        _cache["bank"] = (rv.RirBank.from_arrays(hs, 8000, device=DEV, normalise=None), hs)
    return _cache["bank"]


DENSE = dict(roles=("s1",), speakers=3, max_active=2, pause=(0.0, 0.15), overlap=(0.1, 0.6), p_overlap=0.7)     # turns that overlap and abut


def write_windows(feed, conv, starts):
    ws = tuple(cf.window_schedule(conv, w0, T, feed.rows) for w0 in starts)
    assert all(w is not None for w in ws)
    plan = cf.WindowPlan(ws, np.stack([w.spans for w in ws]), np.stack([w.adj for w in ws]), [w.conv.key for w in ws], np.full(len(ws), T))
    x = torch.full((B, T), float("nan"), device=DEV)
    rows = [torch.full((B, T), float("nan"), device=DEV) for _ in range(feed.rows)]
    feed.write(plan, x, rows)
    torch.cuda.synchronize()
    assert feed.last_plan is plan
    return ws, x.cpu().numpy(), torch.stack(rows).cpu().numpy()


def test_dry_windows_are_slices_of_the_conversation():
    """Windows at the start, in the middle - beginning inside an utterance - and at the end of a planned conversation: the mixture and the
    per-talker sum of the rows are the slice ``[w0, w0 + T)`` of the whole conversation's render, bit for bit."""
    corpus, _ = synthetic_corpus()
    planner = functools.partial(cv.plan_conversation, **DENSE)
    conv = planner(corpus, random.Random(7), seconds=3.0)
    feed = cf.ConversationWindowFeed(corpus, batch=B, max_len=T, channels=2, planner=planner, conversations=1, seconds=3.0)
    inside = [int(p) + 8 for p, n in zip(conv.place, conv.len) if n > 100 and 0 < p + 8 < conv.n - T][0] // 4 * 4
    starts = [0, inside, conv.n - T]
    ws, mix, rows = write_windows(feed, conv, starts)
    assert any((ws[1].conv.place < 0) & (ws[1].conv.place + ws[1].conv.len > 0))      # it begins inside an utterance
    rd = cv.render(corpus, [conv])
    whole, tracks = rd.mixture(0).cpu().numpy(), rd.tracks_of(0).cpu().numpy()
    assert not feed._table.has_rooms
    for b, w0 in enumerate(starts):
        assert np.array_equal(bits(mix[b]).numpy(), bits(whole[w0:w0 + T]).numpy()), w0
        for s in range(conv.S):
            acc = np.zeros(T, dtype=np.float32)
            for u in range(ws[b].used):
                if ws[b].talker[u] == s:
                    acc = acc + rows[u, b]
            assert np.array_equal(bits(acc).numpy(), bits(tracks[s, w0:w0 + T]).numpy()), (w0, s)
        assert not rows[ws[b].used:, b].any()
        for u in range(ws[b].used):                                            # a row is zero outside its span
            on, off = ws[b].spans[u]
            assert not rows[u, b, :on].any() and not rows[u, b, off:].any() and rows[u, b, on:off].any()


def test_windows_in_rooms_with_a_bed_are_the_restatement():
    """Rooms from the hand bank and a noise bed: mixture, rows and bed bit-equal to the numpy restatement of the window schedule, for a
    window at the start, one whose first samples carry only the reverberation of a segment that ended before it, and the last one."""
    corpus, utts = synthetic_corpus()
    bank, hs = hand_bank()
    planner = functools.partial(cv.plan_conversation, noise="noise", **DENSE)
    conv = planner(corpus, random.Random(9), seconds=3.0, rirs=bank)
    feed = cf.ConversationWindowFeed(corpus, batch=B, max_len=T, channels=2, planner=planner, conversations=1, seconds=3.0, rirs=bank)
    assert feed.rows == 7 and feed.bed
    tail = None
    for w0 in range(4, conv.n - T, 52):
        w = cf.window_schedule(conv, w0, T, feed.rows)
        if w is not None:
            c = w.conv
            talk = c.track < feed.rows
            if (talk & (c.place.astype(np.int64) + c.len + c.direct - 1 <= 0)).any():
                tail = w0
                break
    assert tail is not None
    starts = [0, tail, conv.n - T]
    ws, mix, rows = write_windows(feed, conv, starts)
    assert feed._table.has_rooms
    bed = feed.bed_track().cpu().numpy()
    for b, w0 in enumerate(starts):
        want_mix, want_rows, want_bed = gref.render_window_ref(utts, hs, conv, w0, T, feed.rows)
        assert np.array_equal(bits(mix[b]).numpy(), bits(want_mix).numpy()), w0
        assert np.array_equal(bits(rows[:, b]).numpy(), bits(want_rows).numpy()), w0
        assert np.array_equal(bits(bed[b]).numpy(), bits(want_bed).numpy()), w0
        for u in range(feed.rows):
            on, off = ws[b].spans[u]
            assert not rows[u, b, :on].any() and not rows[u, b, off:].any()
    assert ws[1].used >= 3 and ws[1].spans[0].tolist() == [0, 0]               # a row of tails beside live rows
    # a hand schedule: talker 0 ended before the window and rings into it (a row of silence), talker 1's first segment did too and rides on the
    # row of the talker's next segment
    f = np.float32(1.0)
    segs = [(0, 0, 0, 400, f, f, 0), (1, 0, 100, 300, f, f, 1), (2, 0, 1200, 800, f, f, 1), (3, 0, 900, 500, f, f, 2)]
    hand = cv.make_conversation("hand", 4000, 3, segs, rooms=[(4, 1025, 1), (4, 1025, 1), (4, 1025, 10), (-1, 1, 1)])
    starts = [500, 1001 // 4 * 4, 4000 - T]
    ws, mix, rows = write_windows(feed, hand, starts)
    assert ws[0].conv.track.tolist() == [0, 1, 1, 2] and ws[0].spans[:3].tolist() == [[0, 0], [700, 1509], [400, 900]]
    for b, w0 in enumerate(starts):
        want_mix, want_rows, _ = gref.render_window_ref(utts, hs, hand, w0, T, feed.rows)
        assert np.array_equal(bits(mix[b]).numpy(), bits(want_mix).numpy()), w0
        assert np.array_equal(bits(rows[:, b]).numpy(), bits(want_rows).numpy()), w0
    assert np.abs(mix[0][:300]).max() > 0 and not rows[0, 0].any()             # the tails are heard, and are nobody's target


def test_feed_iteration_and_colourings_on_the_device():
    """One epoch through the iteration protocol: every window's graph has a colouring on the device (status 0) against its own mixture."""
    corpus, _ = synthetic_corpus()
    planner = functools.partial(cv.plan_conversation, **DENSE)
    feed = cf.ConversationWindowFeed(corpus, batch=B, max_len=T, channels=2, planner=planner, conversations=2, seconds=3.0, seed=3)
    g = GraphPIT(DEV, 2, feed.rows, B, T)
    n = 0
    for sizes, mix, rows, keys in feed:
        plan = feed.last_plan
        assert sizes.tolist() == [float(T)] * B and mix.shape == (B, T) and len(rows) == feed.rows and keys == plan.keys
        g.load(plan.spans, plan.adj)
        out = g([mix, torch.zeros_like(mix)], rows)
        torch.cuda.synchronize()
        assert g.status.tolist() == [0] * B and bool(torch.isfinite(g.value).all())
        total = out[0] + out[1]
        for b in range(B):                                                     # dry, no bed: the channels' targets add up to the mixture
            assert torch.allclose(total[b], mix[b], atol=1e-5)
        n += 1
    assert n >= 2 and feed.epoch == 1


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------------
def make_trainer(directory, **kw):
    import test_trainer_gpu as tt
    from sepreformer_amd import trainer as T_
    corpus, _ = synthetic_corpus()
    bank, _ = hand_bank()
    planner = functools.partial(cv.plan_conversation, roles=("s1",), speakers=3, max_active=2, noise="noise")
    mk = lambda seed: cf.ConversationWindowFeed(corpus, batch=tt.B, max_len=tt.MAXLEN, channels=2, planner=planner, conversations=1,
                                                seconds=1.25, seed=seed, rirs=bank)
    kw.setdefault("max_epoch", 3)
    kw.setdefault("log", lambda s: None)
    return T_.Trainer(tt.tiny(0.0), mk(3), mk(4), str(directory), lr=tt.LR, seed=11, warmup_steps=tt.WARMUP, criterion="graph_sasdr", **kw)


def state_bits(t):
    return [bits(v.detach().float().cpu()) for v in t.model.state_dict().values() if v.is_floating_point()]


def test_trainer_two_epochs_and_resume(tmp_path):
    """The tiny model on windows of 3-speaker conversations in rooms over a noise bed, two channels: two epochs of two batches with finite
    losses; one epoch, a checkpoint, fresh objects and one more epoch continue bit for bit; the checkpoint records the criterion."""
    import trainer_ref as tr
    from sepreformer_amd import trainer as T_
    probe = make_trainer(tmp_path / "probe")
    assert [len(list(probe.train_feed.plans())) for _ in range(2)] == [2, 2]   # two epochs of two batches
    assert probe.graph is not None and len(probe._targets) == probe.train_feed.rows == 7
    whole = make_trainer(tmp_path / "whole")
    whole.run()
    assert whole.global_step == 4 and all(np.isfinite(v) for v in whole.last_train[:2] + whole.last_valid[:2])
    led = whole.read_ledger()
    assert led.steps == 2 and led.skipped == 0 and led.nonfinite == 0 and all(np.isfinite(v) for v in led.values)
    assert whole.graph.status.tolist() == [0, 0]
    cut = make_trainer(tmp_path / "cut", max_epoch=2)
    cut.run()
    del cut
    ck = T_.read_checkpoint(T_.latest_checkpoint(str(tmp_path / "cut")))
    assert ck[T_.RUN_STATE_KEY]["criterion"] == "graph_sasdr"
    again = make_trainer(tmp_path / "cut")
    again.run()
    assert again.start_epoch == 2 and again.global_step == 4
    assert again.last_train == whole.last_train and again.last_valid == whole.last_valid
    assert all(torch.equal(x, y) for x, y in zip(state_bits(again), state_bits(whole)))
    assert tr.same_bits(again.ledger, whole.ledger)


def test_tool_trains_on_conversation_windows(tmp_path):
    """tools/train_from_scp.py --conversation-windows --criterion graph_sasdr on scp lists written from the synthetic corpus: three captured steps
    in synthetic rooms over the noise role, finite losses; the options are refused apart."""
    import subprocess
    import trainer_ref as tr
    arrays = rref.corpus_arrays("int16", noise=True)
    scp = {}
    for role, names in (("s1", ["s1/u0", "s1/u1", "s1/u2"]), ("s2", ["s1/u3", "s1/u4", "s1/u5"]), ("noise", ["noise/n0", "noise/n1"])):
        lines = []
        for nm in names:
            a = arrays[nm]
            wav = str(tmp_path / f"{role}_{nm.partition('/')[2]}.wav")
            tr.write_wav16(wav, a if a.dtype == np.int16 else np.round(a * 32768.0).astype(np.int16))
            lines.append(f"{nm.partition('/')[2]} {wav}")
        scp[role] = str(tmp_path / f"{role}.scp")
        with open(scp[role], "w") as f:
            f.write("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "train_from_scp.py"), "--form", "wham", "--scp", f"s1={scp['s1']}", f"s2={scp['s2']}",
           f"noise={scp['noise']}", "--model", "tiny", "--precision", "bf16x3", "--batch", "2", "--max-len", "2000", "--steps", "3", "--log", "1",
           "--synthetic-rirs", "4:0.1:0.2"]
    run = subprocess.run(cmd + ["--conversation-windows", "2:1.5", "--criterion", "graph_sasdr"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    losses = [float(ln.split("loss")[1].split()[0]) for ln in run.stdout.splitlines() if ln.startswith("step ")]
    assert len(losses) == 3 and all(np.isfinite(v) for v in losses), run.stdout
    for extra in (["--conversation-windows", "2:1.5"], ["--criterion", "graph_sasdr"]):
        bad = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "go together" in bad.stderr, bad.stderr
