"""Float64 restatement of Graph-PIT, written from the definition of ``sepr_graph_pit_assign`` /
``sepr_graph_pit_assemble`` in include/sepr.h, and the restatement of a conversation window's schedule and render.  Test infrastructure only.

* ``moments``: the sums by ``math.fsum`` over the stated intervals - a row is ZERO outside its span whatever the array holds there;
* ``assign``: brute force over every colouring in lexicographic order, the first minimiser of E among the valid ones;
* ``assemble``: float32 adds in ascending row order from +0.0;
* ``window_ref`` / ``render_window_ref``: the window ``[w0, w0 + T)`` of a conversation as rows, spans and adjacency, written again from the
  rules, and its render through tests/conversation_rooms_ref.py on a time line that starts early enough to hold every kept segment.
"""
from __future__ import annotations

import itertools
import math
from types import SimpleNamespace

import numpy as np

import conversation_rooms_ref as crr

EPS, SNR_MAX = 1.0e-8, 30.0


def clamp_span(on, off, T):
    on = min(max(int(on), 0), T)
    return on, min(max(int(off), on), T)


def moments(est, rows, spans):
    """est ``[C, T]``, rows ``[U, T]`` float32, spans ``[U, 2]`` -> dict of the moments of one example (Python floats from ``math.fsum``)."""
    C, T = est.shape
    U = rows.shape[0]
    e, t = est.astype(np.float64), rows.astype(np.float64)
    sp = [clamp_span(spans[u][0], spans[u][1], T) for u in range(U)]
    fs = lambda a: math.fsum(a.tolist())
    m = {"T": T, "span": sp,
         "se": [fs(e[c]) for c in range(C)], "ee": [fs(e[c] * e[c]) for c in range(C)],
         "st": [fs(t[u, sp[u][0]:sp[u][1]]) for u in range(U)], "tt": [fs(t[u, sp[u][0]:sp[u][1]] ** 2) for u in range(U)],
         "et": [[fs(e[c, sp[u][0]:sp[u][1]] * t[u, sp[u][0]:sp[u][1]]) for u in range(U)] for c in range(C)],
         "tv": {}}
    for u in range(U):
        for v in range(u + 1, U):
            lo, hi = max(sp[u][0], sp[v][0]), min(sp[u][1], sp[v][1])
            m["tv"][(u, v)] = fs(t[u, lo:hi] * t[v, lo:hi]) if hi > lo else 0.0
    return m


def energy(m, col, C):
    """(E, D) of the colouring ``col`` (a sequence of U colours) from the moments, in the header's order of operations."""
    T = float(m["T"])
    U = len(col)
    E = D = 0.0
    for c in range(C):
        Sy = tts = cross = ets = 0.0
        for u in range(U):
            if col[u] != c or m["span"][u][1] <= m["span"][u][0]:
                continue
            Sy += m["st"][u]
            tts += m["tt"][u]
            ets += m["et"][c][u]
            for v in range(u + 1, U):
                if col[v] == c and m["span"][v][1] > m["span"][v][0]:
                    cross += m["tv"][(u, v)]
        yy = (tts + 2.0 * cross) - Sy * Sy / T
        eet = m["ee"][c] - m["se"][c] * m["se"][c] / T
        ey = ets - m["se"][c] * Sy / T
        E += (eet - 2.0 * ey) + yy
        D += yy
    return max(E, 0.0), D


def edges(adj, live, U):
    """The graph on the live rows: an edge if either side names it; a row's own bit and bits at or above U do not count."""
    out = set()
    for u in range(U):
        for v in range(U):
            if u != v and live[u] and live[v] and (int(adj[u]) >> v) & 1:
                out.add((min(u, v), max(u, v)))
    return out


def value_of(E, D, eps=EPS, snr_max=SNR_MAX):
    return 10.0 * math.log10((E + 10.0 ** (-snr_max / 10.0) * D + eps) / (D + eps))


def assign(est, rows, spans, adj, eps=EPS, snr_max=SNR_MAX):
    """One example -> dict: ``col`` (list of U ints), ``value``, ``status``, ``E`` (of the winner), ``all`` (the (E, colouring) of every valid
    colouring in lexicographic order) and ``gap_db``: the distance in dB of ``value`` between the best and the second-best DISTINCT E (inf when
    there is one colouring or none)."""
    C, T = est.shape
    U = rows.shape[0]
    m = moments(est, rows, spans)
    live = [m["span"][u][1] > m["span"][u][0] for u in range(U)]
    ed = edges(adj, live, U)
    cand = []
    for col in itertools.product(*[range(C) if live[u] else (0,) for u in range(U)]):      # lexicographic; a silent row stays 0
        if any(col[u] == col[v] for u, v in ed):
            continue
        E, D = energy(m, col, C)
        cand.append((E, D, col))
    if not cand:
        return {"col": [0] * U, "value": float("nan"), "status": 1, "E": float("nan"), "all": [], "gap_db": float("inf")}
    best = min(range(len(cand)), key=lambda i: (cand[i][0], i))                             # the first minimiser
    E, D, col = cand[best]
    others = sorted({c[0] for c in cand if c[0] != E})
    gap = abs(value_of(others[0], D, eps, snr_max) - value_of(E, D, eps, snr_max)) if others else float("inf")
    return {"col": list(col), "value": value_of(E, D, eps, snr_max), "status": 0, "E": E, "D": D, "all": [(c[0], c[2]) for c in cand],
            "gap_db": gap}


def assemble(rows, spans, col, C):
    """rows ``[U, T]`` float32 -> ``[C, T]`` float32: ``((+0.0 + t_u1) + t_u2) + ...`` over the rows of each colour, ascending, each row zero
    outside its span."""
    U, T = rows.shape
    out = np.zeros((C, T), dtype=np.float32)
    for u in range(U):
        on, off = clamp_span(spans[u][0], spans[u][1], T)
        t = np.zeros(T, dtype=np.float32)
        t[on:off] = rows[u, on:off]
        c = min(max(int(col[u]), 0), C - 1)
        out[c] = out[c] + t
    return out


def dry_layout_bytes(C, U, B):
    """``sepr_graph_pit_bytes``: one float64 array [B][2 C + 2 U + C U + U (U - 1) / 2], rounded up to the arena's 256 bytes."""
    if not (1 <= C <= 3 and 1 <= U <= 8 and 1 <= B <= 65535):
        return 0
    n = 8 * B * (2 * C + 2 * U + C * U + U * (U - 1) // 2)
    return (n + 255) // 256 * 256


# ---- windows of a conversation ------------------------------------------------------------------------------------------------------------
def _rooms(c):
    rir, taps, direct = crr.rooms_of(c)
    return np.asarray(rir, dtype=np.int64), np.asarray(taps, dtype=np.int64), np.asarray(direct, dtype=np.int64)


def window_ref(c, w0, T, U):
    """The window ``[w0, w0 + T)`` of conversation ``c`` by the rules of DESIGN.md section 5e-8, or ``None`` when it needs more than ``U``
    rows -> SimpleNamespace(segs: list of (row or "bed", g, place'), spans [U][2], adj [U], used)."""
    rir, taps, direct = _rooms(c)
    segs, spans, dry = [], [], []
    for s in range(c.S):
        tails = []
        for g in range(len(c.utt)):
            if int(c.track[g]) != s:
                continue
            p, ln = int(c.place[g]) - w0, int(c.len[g])
            if not (p < T and p + ln + int(taps[g]) - 1 > 0):
                continue                                               # its wet support misses the window
            if p + ln + int(direct[g]) - 1 > 0:                        # the direct path reaches the window: a row
                row = len(spans)
                segs += [(row, t, tp) for t, tp in tails] + [(row, g, p)]
                tails = []
                spans.append((max(0, p), min(T, p + ln + int(direct[g]) - 1)))
                dry.append((max(0, p), min(T, p + ln)))
            else:
                tails.append((g, p))
        if tails:                                                      # nobody's target and no later segment of the talker: a row of silence
            row = len(spans)
            segs += [(row, t, tp) for t, tp in tails]
            spans.append((0, 0))
            dry.append((0, 0))
    used = len(spans)
    if used > U:
        return None
    adj = [0] * U
    for u in range(used):
        for v in range(used):
            if u != v and max(dry[u][0], dry[v][0]) < min(dry[u][1], dry[v][1]):
                adj[u] |= 1 << v
    if getattr(c, "bed", 0):
        for g in range(len(c.utt)):
            p = int(c.place[g]) - w0
            if int(c.track[g]) == c.S and p < T and p + int(c.len[g]) > 0:
                segs.append(("bed", g, p))
    return SimpleNamespace(segs=segs, spans=spans + [(0, 0)] * (U - used), adj=adj, used=used)


def render_window_ref(arrays, bank, c, w0, T, U):
    """-> (mix [T], rows [U, T], bed [T] or None) float32: the window's schedule - rows as tracks, the bed after them - rendered by
    tests/conversation_rooms_ref.py on a time line that begins ``pad`` samples before the window, so that no segment begins before it."""
    w = window_ref(c, w0, T, U)
    rir, taps, direct = _rooms(c)
    bed = int(getattr(c, "bed", 0))
    pad = max([0] + [-p for _, _, p in w.segs])
    order = sorted(range(len(w.segs)), key=lambda i: (U if w.segs[i][0] == "bed" else w.segs[i][0], w.segs[i][2]))
    gs = [w.segs[i][1] for i in order]
    col = lambda a, dt: np.array([a[g] for g in gs], dtype=dt)
    shifted = SimpleNamespace(n=pad + T, S=U, bed=bed, utt=col(c.utt, np.int64), start=col(c.start, np.int64),
                              place=np.array([w.segs[i][2] + pad for i in order], dtype=np.int64), len=col(c.len, np.int64),
                              norm=col(c.norm, np.float32), gain=col(c.gain, np.float32),
                              track=np.array([U if w.segs[i][0] == "bed" else w.segs[i][0] for i in order], dtype=np.int64),
                              rir=col(rir, np.int64), taps=col(taps, np.int64), direct=col(direct, np.int64))
    if not gs:
        return np.zeros(T, dtype=np.float32), np.zeros((U, T), dtype=np.float32), None
    mix, tracks, _, _ = crr.render_ref(arrays, bank, [shifted], S_max=U + bed)
    return mix[pad:], tracks[:U, pad:], (tracks[U, pad:] if bed else None)
