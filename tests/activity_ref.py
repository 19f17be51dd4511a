"""Restatement of the frame-activity entries (include/sepr.h) in numpy float64, in the header's stated orders, and of
``conversation.colour`` by enumeration."""
import itertools

import numpy as np


def butterfly(v):
    """``v [..., 64]``: for o = 32, 16, .., 1 every lane adds the value of lane ``l ^ o`` to its own; lane 0 of the result."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def frame_energy_ref(x, frame):
    """``x [rows][T]`` float32, the valid samples only -> float64 ``[rows][ceil(T / frame)]``: lane ``l`` adds the squares of the samples
    ``4 q .. 4 q + 3`` for ``q = l, l + 64, ..`` in ascending order from +0.0, then the butterfly.  Samples past the frame's end are laid out as
    zeros here: a partial sum that began at +0.0 of squares is never -0.0, so adding +0.0 changes no bit of it."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    rows, T = x.shape
    nF = -(-T // frame)
    steps = -(-frame // 256)
    sq = np.zeros((rows, nF, steps * 256), dtype=np.float64)
    flat = np.zeros((rows, nF * frame), dtype=np.float64)
    flat[:, :T] = x.astype(np.float64) * x.astype(np.float64)            # exact
    sq[:, :, :frame] = flat.reshape(rows, nF, frame)
    sq = sq.reshape(rows, nF, steps, 64, 4)
    acc = np.zeros((rows, nF, 64), dtype=np.float64)
    for s in range(steps):
        for k in range(4):
            acc = acc + sq[:, :, s, :, k]
    return butterfly(acc)


def activity_ref(e, ratio, floor, hang, planted=()):
    """-> ``(active uint8 [rows][nF], level [rows], thr [rows])``.  Asserts first that no frame other than the ``planted`` ``(row, frame)``
    pairs lies within 1e-9 relative of its row's threshold: the comparison is then beyond doubt."""
    e = np.atleast_2d(np.asarray(e, dtype=np.float64))
    rows, nF = e.shape
    active = np.zeros((rows, nF), dtype=np.uint8)
    level, thr = np.zeros(rows), np.zeros(rows)
    for r in range(rows):
        m = -np.inf
        for v in e[r] + 0.0:
            m = v if v > m else m
        t = m * ratio
        level[r], thr[r] = m, (t if t > floor else floor)
        for f in range(nF):
            if (r, f) not in planted and not np.isnan(e[r, f]):
                assert abs(e[r, f] - thr[r]) > 1e-9 * thr[r], (r, f, e[r, f], thr[r])
        raw = np.array([bool(v > thr[r]) for v in e[r]])
        for f in range(nF):
            active[r, f] = raw[max(0, f - hang):min(nF, f + hang + 1)].any()
    return active, level, thr


def class_sums_ref(e_est, e_mix, active, cls):
    """-> ``(out [C][4][4], part [C][4][4][4])``: thread i of 256 takes the frames i, i + 256, .. of its class from +0.0, a wave adds its lanes
    by butterfly, the four wave sums (``part``) are added in wave order."""
    e_est = np.atleast_2d(np.asarray(e_est, dtype=np.float64))
    e_mix, active, cls = np.asarray(e_mix, dtype=np.float64), np.atleast_2d(active), np.atleast_2d(cls)
    C, nF = e_est.shape
    out, part = np.zeros((C, 4, 4)), np.zeros((C, 4, 4, 4))
    with np.errstate(invalid="ignore"):
        for c in range(C):
            for k in range(4):
                acc = np.zeros((4, 256))
                for base in range(0, nF, 256):
                    f = np.arange(base, min(nF, base + 256))
                    sel = (cls[c, f] & 3) == k
                    i, f = f[sel] - base, f[sel]
                    acc[0, i] = acc[0, i] + 1.0
                    acc[1, i] = acc[1, i] + (active[c, f] != 0)
                    acc[2, i] = acc[2, i] + e_est[c, f]
                    acc[3, i] = acc[3, i] + e_mix[f]
                w = butterfly(acc.reshape(4, 4, 64))
                part[c, k] = w
                out[c, k] = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return out, part


def colour_brute(v, begin, length, C):
    """All ``C^G`` assignments in lexicographic order over the segments ordered by ``(begin, table index)``; the total from 0.0, left to
    right, in float64; the first maximiser among the valid ones.  -> ``(a [G] by table index or None, best total, second-best total)``."""
    v = np.asarray(v, dtype=np.float64)
    b = np.asarray(begin, dtype=np.int64)
    e = b + np.asarray(length, dtype=np.int64)
    G = len(b)
    order = sorted(range(G), key=lambda g: (int(b[g]), g))
    adj = [(i, j) for i in range(G) for j in range(i + 1, G) if max(b[order[i]], b[order[j]]) < min(e[order[i]], e[order[j]])]
    best, second, top = -np.inf, -np.inf, None
    for a in itertools.product(range(C), repeat=G):
        if any(a[i] == a[j] for i, j in adj):
            continue
        tot = 0.0
        for i in range(G):
            tot = tot + v[order[i], a[i]]
        if tot > best:
            best, second, top = tot, best, a
        elif tot > second:
            second = tot
    if top is None:
        return None, best, second
    out = np.empty(G, dtype=np.int64)
    out[np.asarray(order)] = top
    return out, best, second


def frame_classes_brute(begin, length, coloured, n, C, frame, collar):
    """Per sample: which kinds of span hold it; a frame takes the first rule that any of its samples meets."""
    nF = -(-n // frame)
    t = np.arange(n)
    cls = np.zeros((C, nF), dtype=np.uint8)
    wide_any = np.zeros(n, dtype=bool)
    for b, ln in zip(begin, length):
        wide_any |= (t >= b - collar) & (t < b + ln + collar)
    for c in range(C):
        own, wide = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for b, ln, a in zip(begin, length, coloured):
            if a == c:
                own |= (t >= b) & (t < b + ln)
                wide |= (t >= b - collar) & (t < b + ln + collar)
        for f in range(nF):
            s = slice(f * frame, min(n, (f + 1) * frame))
            cls[c, f] = 0 if own[s].any() else (3 if wide[s].any() else (1 if wide_any[s].any() else 2))
    return cls
