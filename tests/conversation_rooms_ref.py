"""Restatement of conversations in rooms, written from the definition of ``sepr_conversation_render_rooms`` in
include/sepr.h.  It shares no code with ``sepreformer_amd/conversation.py``, ``sepreformer_amd/reverb.py`` or the kernel: the sample values come
from tests/conversation_ref.py and the float64 sums from tests/dynmix_reverb_ref.py, whose sequential ``acc = acc + h64[j] * x64`` is the device's
``fma(h, x, acc)`` because the product of two float32 values is exact in float64.

A conversation here is anything with the attributes ``n, S, utt, start, place, len, norm, gain, track`` and ``rir, taps, direct`` (arrays, or
``None`` = no response anywhere) and ``bed`` (1: track ``S`` is a noise bed).  The hand schedule and its bank live here too, as plain tuples, so
that the test without a device can assert from the restatement that the schedule holds what the device test says it exercises."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import conversation_ref as cref
import dynmix_reverb_ref as drr

MAX_TAPS = 16384
UNIT = np.ones(1, dtype=np.float32)


def rooms_of(c):
    """(rir, taps, direct) int arrays of a conversation: -1, 1, 1 where it carries none."""
    G = len(c.utt)
    if getattr(c, "rir", None) is None:
        return np.full(G, -1), np.ones(G, dtype=np.int64), np.ones(G, dtype=np.int64)
    return np.asarray(c.rir), np.asarray(c.taps), np.asarray(c.direct)


def segment_value(x_seg: np.ndarray, h: np.ndarray, K: int, norm, gain, place: int, n: int) -> np.ndarray:
    """``v_g^K`` on its support ``place <= t < min(n, place + len + K - 1)``: the segment's samples, zero outside the SEGMENT, under the first
    ``K`` taps of ``h`` - float64 sums in tap order, one rounding, then the two float32 multiplies."""
    ln = x_seg.shape[0]
    padded = np.concatenate([x_seg, np.zeros(K - 1, dtype=np.float32)])            # an utterance of its own: zero before 0 and after len + K - 2
    z = drr.conv64(padded, h, 0, ln + K - 1, K).astype(np.float32)
    a = (z * np.float32(norm)).astype(np.float32)
    v = (a * np.float32(gain)).astype(np.float32)
    return v[:max(0, min(n, place + ln + K - 1) - place)]


def render_ref(arrays, bank, convs, S_max=None):
    """-> (mix [total], tracks [S_max, total], wet [S_max, total], out_off), float32.  ``arrays``: the utterances in corpus storage order; ``bank``:
    the impulse responses as float32 arrays.  ``tracks`` runs over the first ``direct`` taps, ``wet`` over ``taps``; a bed is the row after the
    talkers."""
    S_max = S_max or max(c.S + int(getattr(c, "bed", 0)) for c in convs)
    out_off = np.concatenate([[0], np.cumsum([c.n for c in convs])]).astype(np.int64)
    total = int(out_off[-1])
    wet = np.zeros((S_max, total), dtype=np.float32)                               # running sums that start at +0.0
    tracks = np.zeros((S_max, total), dtype=np.float32)
    for r, c in enumerate(convs):
        rir, taps, direct = rooms_of(c)
        for g in range(len(c.utt)):                                                # table order: by (track, place)
            x = cref.sample_values(arrays[int(c.utt[g])])[int(c.start[g]):int(c.start[g]) + int(c.len[g])]
            assert x.shape[0] == int(c.len[g]), "the segment reads past its utterance"
            h = UNIT if int(rir[g]) < 0 else bank[int(rir[g])]
            s, o = int(c.track[g]), int(out_off[r]) + int(c.place[g])
            for row, K in ((wet, int(taps[g])), (tracks, int(direct[g]))):
                v = segment_value(x, h, K, c.norm[g], c.gain[g], int(c.place[g]), int(c.n))
                row[s, o:o + v.shape[0]] = row[s, o:o + v.shape[0]] + v
    mix = np.zeros(total, dtype=np.float32)
    for s in range(S_max):                                                         # ((0 + wet 0) + wet 1) + ...
        mix = mix + wet[s]
    return mix, tracks, wet, out_off


def contributors(convs, S_max=None):
    """int [S_max, total]: how many segments' supports (under ``taps``) hold each sample of each track."""
    S_max = S_max or max(c.S + int(getattr(c, "bed", 0)) for c in convs)
    out_off = np.concatenate([[0], np.cumsum([c.n for c in convs])]).astype(np.int64)
    cnt = np.zeros((S_max, int(out_off[-1])), dtype=np.int64)
    for r, c in enumerate(convs):
        _, taps, _ = rooms_of(c)
        for g in range(len(c.utt)):
            lo, hi = int(c.place[g]), min(int(c.n), int(c.place[g]) + int(c.len[g]) + int(taps[g]) - 1)
            cnt[int(c.track[g]), int(out_off[r]) + lo:int(out_off[r]) + hi] += 1
    return cnt


def check_schedule(c, bank_lengths=None, max_active=None, lengths=None):
    """The invariants of tests/conversation_ref.py on the talkers, and those of the new fields and the bed: three int32 columns or none,
    ``rir >= -1``, ``1 <= direct <= taps <= 16384``, ``taps = direct = 1`` where ``rir = -1``, with ``bank_lengths`` every ``rir`` inside the
    bank and ``taps <= len_r``; a bed lies on track ``S <= 7``, carries no response and one gain, and covers ``[0, n)`` without a gap."""
    G = len(c.utt)
    bed = int(getattr(c, "bed", 0))
    assert bed in (0, 1) and c.S + bed <= 8
    talk = np.asarray(c.track) < c.S
    assert talk.any() and np.all(np.asarray(c.track)[~talk] == c.S) and (bed or talk.all())
    assert np.all(talk[:-1] >= talk[1:])                                           # sorted by track: the bed comes last
    cols = ("utt", "start", "place", "len", "norm", "gain", "track")
    cref.check_schedule(SimpleNamespace(n=c.n, S=c.S, **{f: getattr(c, f)[talk] for f in cols}), max_active=max_active, lengths=lengths)
    have = [getattr(c, f, None) is not None for f in ("rir", "taps", "direct")]
    assert all(have) or not any(have)
    rir, taps, direct = rooms_of(c)
    if all(have):
        for col in (c.rir, c.taps, c.direct):
            assert col.dtype == np.int32 and col.shape == (G,)
    assert rir.min() >= -1 and direct.min() >= 1 and np.all(direct <= taps) and taps.max() <= MAX_TAPS
    assert np.all(taps[rir < 0] == 1)
    if bank_lengths is not None and (rir >= 0).any():
        assert rir.max() < len(bank_lengths) and np.all(taps[rir >= 0] <= np.asarray(bank_lengths)[rir[rir >= 0]])
    if bed:
        b = ~talk
        assert b.any() and np.all(rir[b] == -1)
        place, ln = c.place[b].astype(np.int64), c.len[b].astype(np.int64)
        assert place[0] == 0 and np.array_equal(place[1:], (place + ln)[:-1]) and place[-1] + ln[-1] == c.n and ln.min() >= 1
        assert len(set(np.ascontiguousarray(c.gain[b], dtype=np.float32).view(np.int32).tolist())) == 1
        if lengths is not None:
            assert np.all(c.start[b].astype(np.int64) + ln <= np.asarray(lengths)[c.utt[b]])


# ---- the hand schedule of the device test ---------------------------------------------------------------------------------------------------
CORPUS_LENGTHS = ((5000, True), (4101, True), (2600, True), (4999, False), (3000, False), (37, False))      # tests/test_conversation_gpu.py's
BANK_TAPS = (1, 2, 1023, 1024, 1025, 2049)               # random-sign responses: the kernel's tap chunk is 1024 and its tile 2048
R_UNIT, R_DELAY, DELAY = 6, 7, 700                        # bank[6] = [1.0]; bank[7] = [0] * 700 + [1.0]
HAND_N = 4100


def corpus_arrays(fmt, noise=False):
    """name -> array of the six-utterance synthetic corpus, role ``s1``; ``fmt`` "int16" / "float32" stores all six in that format, "both" three
    of each.  Large values, so a read into a neighbour is not a read of zeros.  ``noise``: two short utterances more, role ``noise``."""
    rng = np.random.default_rng(7)
    arrays = {}
    for i, (n, is16) in enumerate(CORPUS_LENGTHS):
        if fmt == "int16" or (fmt == "both" and is16):
            arrays[f"s1/u{i}"] = rng.integers(-20000, 20000, size=n, dtype=np.int16)
        else:
            arrays[f"s1/u{i}"] = rng.normal(0, 0.1, size=n).astype(np.float32)
    if noise:
        arrays["noise/n0"] = rng.integers(-3000, 3000, size=1901, dtype=np.int16)
        arrays["noise/n1"] = rng.normal(0, 0.02, size=2750).astype(np.float32)
    return arrays


def roles_of(arrays):
    """role -> keys in the order given: what ``Corpus.from_scp`` would have recorded."""
    roles = {}
    for name in arrays:
        role, _, key = name.partition("/")
        roles.setdefault(role, []).append(key)
    return roles


def hand_bank():
    """The eight responses as float32 arrays, to be stored as given (no normalisation)."""
    rng = np.random.default_rng(11)
    hs = [(rng.normal(0, 0.4, size=k) * np.exp(-np.arange(k) / 600.0)).astype(np.float32) for k in BANK_TAPS]
    hs.append(np.ones(1, dtype=np.float32))
    hs.append(np.concatenate([np.zeros(DELAY), [1.0]]).astype(np.float32))
    assert all(h.any() for h in hs)
    return hs


# (track, utt, start, place, len, rir, taps, direct) on 4100 samples
HAND_SEGMENTS = [
    (0, 5, 3, 0, 1, 5, 2049, 1),                  # one sample under 2049 taps: its tail crosses sample 2048
    (0, 0, 20, 100, 5, 4, 1025, 500),             # three of 5 samples, 3 apart, each under a 1025-tap tail: with the one above, four
    (0, 1, 30, 108, 5, 4, 1025, 1025),            #   contributors to the samples from 116 on; direct = a middle value, taps, 1
    (0, 2, 40, 116, 5, 4, 1025, 1),
    (0, 0, 7, 1000, 1048, 3, 1024, 9),            # ends at 2048 where the next begins (pause 0); its tail lies under that one
    (0, 1, 0, 2048, 1500, -1, 1, 1),              # no response on a track that has some
    (0, 2, 10, 3600, 400, 5, 2049, 77),           # ends at 4000: its tail crosses 4096 and is cut by n
    (1, 4, 1, 30, 2000, 1, 2, 2),
    (1, 0, 100, 2030, 18, R_DELAY, DELAY + 1, DELAY + 1),     # abuts; lands 700 later, across 2048
    (1, 3, 5, 3000, 1100, 2, 1023, 300),          # ends at n
    # track 2 holds no segment
    (3, 1, 2, 5, 4095, 0, 1, 1),                # a one-tap response that is not 1.0, to the last sample
    (4, 2, 0, 1500, 2600, R_UNIT, 1, 1),
    (5, 4, 0, 2047, 2, -1, 1, 1), (5, 0, 9, 2049, 2047, 4, 1025, 1025),
    (6, 3, 0, 0, 4100, 5, 2049, 2049),            # the whole line under the longest response
    (7, 5, 0, 4090, 10, -1, 1, 1),
]


def _conv(key, n, S, rows, factors):
    rows = sorted(rows, key=lambda s: (s[0], s[3]))
    col = lambda i, dt: np.array([s[i] for s in rows], dtype=dt)
    f = np.array([factors() for _ in range(2 * len(rows))], dtype=np.float32).reshape(2, -1)
    return SimpleNamespace(key=key, n=n, S=S, track=col(0, np.int32), utt=col(1, np.int32), start=col(2, np.int32), place=col(3, np.int32),
                           len=col(4, np.int32), norm=f[0], gain=f[1], rir=col(5, np.int32), taps=col(6, np.int32), direct=col(7, np.int32),
                           bed=0)


def hand_conversations(S, seed):
    """R = 2: the hand schedule on ``S`` tracks, and 4 samples on min(S, 2) tracks whose 1025-tap tail is cut at once."""
    rng = np.random.default_rng(seed)
    f = lambda: float(np.float32(rng.uniform(0.3, 1.7)))
    a = _conv("a", HAND_N, S, [s for s in HAND_SEGMENTS if s[0] < S], f)
    b = _conv("b", 4, min(S, 2), [(0, 5, 33, 0, 2, 4, 1025, 1)] + ([(1, 0, 4996, 1, 2, -1, 1, 1)] if S > 1 else []), f)
    return [a, b]


def dry(c):
    """The conversation without its rooms: what ``sepr_conversation_render`` takes."""
    d = SimpleNamespace(**vars(c))
    d.rir = d.taps = d.direct = None
    return d
