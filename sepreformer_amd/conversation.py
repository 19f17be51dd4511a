"""Conversations rendered and scored on the device (contracts in include/sepr.h).

``separate_long``, ``StreamBank`` and ``separate_many`` take recordings of any length; this module makes such recordings from the resident
``Corpus`` of the training feed and scores what the separator does with them, utterance by utterance, as the continuous-speech-separation
literature (LibriCSS) does:

    convs = [plan_conversation(corpus, random.Random(i), seconds=600) for i in range(20)]
    rd = render(corpus, convs)                                  # ONE launch: every mixture and every talker track
    est = separate_long(model, [rd.mixture(r) for r in range(len(convs))])
    ...                                                         # infer.evaluate_conversations is the whole loop

* ``plan_conversation`` lays corpus utterances along a time line (a schedule: it touches no sample);
* ``render`` is one ``sepr_conversation_render`` launch for all conversations - the arithmetic of ``sepr_dynmix_fwd``, so a numpy
  restatement is bit-equal (tests/conversation_ref.py); conversations whose talkers sit in rooms (``plan_conversation(rirs=...)``) or that
  carry a noise bed (``noise=...``) go through ``sepr_conversation_render_rooms`` - the float64 convolution of the mixing launch per segment,
  the tails running on under the next turns, the direct paths as the scoring references (section 5h-2, tests/conversation_rooms_ref.py);
* ``segment_sisnr`` is one ``sepr_segment_sisnr_fwd`` call: the SI-SNR of every output channel and of the mixture against every
  utterance over that utterance's span, in float64;
* ``score`` turns the two small matrices into utterance-wise SI-SNRi, the consistent-assignment SI-SNRi and the channel switch rate;
* ``colour`` is the assignment that exists for any number of talkers - utterances whose spans intersect go on different channels -,
  ``frame_classes`` says which frames of a channel are its own, a collar, another talker's or nobody's, and ``idle_figures`` turns the class
  sums of ``activity.frame_class_sums`` into leak, false-alarm and miss figures (section 5h-3).
"""
from __future__ import annotations

import itertools
import random
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L_
from .datafeed import Corpus, _gain, _norm

MAX_TRACKS = 8                       # talker tracks of a conversation, and channels of a scored separator
MAX_TAPS = 16384                     # samples of the longest impulse response (reverb.MAX_TAPS)
OVERLAP_BINS = ("0", "(0,0.2]", "(0.2,0.5]", "(0.5,1]")


class _Schedule(NamedTuple):
    key: str
    n: int                           # output samples, a multiple of 4
    S: int                           # talker tracks, 1 .. 8
    utt: np.ndarray                  # int32 [G]
    start: np.ndarray                # int32 [G]
    place: np.ndarray                # int32 [G]
    len: np.ndarray                  # int32 [G], at least 1
    norm: np.ndarray                 # float32 [G]
    gain: np.ndarray                 # float32 [G]
    track: np.ndarray                # int32 [G]


class Conversation(_Schedule):
    """A schedule: ``G`` segments sorted by ``(track, place)``.  Segment ``g`` puts the samples ``start[g] .. start[g] + len[g] - 1`` of utterance
    ``utt[g]``, scaled by ``norm[g]`` and then ``gain[g]``, on the output samples ``place[g] .. place[g] + len[g] - 1`` of track ``track[g]``.

    Four trailing fields with defaults carry the rooms (section 5h-2): ``rir``, ``taps``, ``direct`` (int32 ``[G]``, all three or ``None``) -
    segment ``g`` rings with the first ``taps[g]`` samples of response ``rir[g]`` of an ``RirBank`` (-1: no response, ``taps = direct = 1``) and
    its scoring reference keeps the first ``direct[g]`` - and ``bed`` (1: track ``S`` holds a noise bed, outside the talkers).  They are taken
    positionally or by name and ``_replace`` knows them, but they are attributes beside the tuple: what iteration, slicing and comparison
    see stays the ten fields above, as code that walks ``conv[3:]`` as the seven columns expects."""
    ROOM_FIELDS = ("rir", "taps", "direct", "bed")

    def __new__(cls, key, n, S, utt, start, place, len, norm, gain, track, rir=None, taps=None, direct=None, bed=0):
        self = super().__new__(cls, key, n, S, utt, start, place, len, norm, gain, track)
        self.rir, self.taps, self.direct, self.bed = rir, taps, direct, int(bed)
        return self

    def _replace(self, **kw):
        rooms = {f: kw.pop(f, getattr(self, f)) for f in self.ROOM_FIELDS}
        return Conversation(*super()._replace(**kw), **rooms)

    def __reduce__(self):
        return (Conversation, tuple(self) + tuple(getattr(self, f) for f in self.ROOM_FIELDS))


def make_conversation(key: str, n: int, S: int, segments: Sequence[Tuple[int, int, int, int, float, float, int]],
                      rooms: Optional[Sequence[Tuple[int, int, int]]] = None, bed: bool = False) -> Conversation:
    """A ``Conversation`` from ``(utt, start, place, len, norm, gain, track)`` tuples in any order: sorted by ``(track, place)`` and checked -
    ``n`` a positive multiple of 4, ``S`` in 1..8, every segment of at least one sample inside ``[0, n)`` on a track below ``S``, no two
    segments of one track overlapping.  ``rooms``: a ``(rir, taps, direct)`` triple per segment, sorted along with the segments -
    ``rir >= -1``, ``1 <= direct <= taps <= 16384``, ``taps = direct = 1`` where ``rir = -1``.  ``bed=True``: segments may also lie on track
    ``S``, the noise bed (``S + 1 <= 8``); they carry no response."""
    n, S, bed = int(n), int(S), bool(bed)
    if n < 4 or n % 4 or not 1 <= S <= MAX_TRACKS:
        raise ValueError(f"a conversation has a positive multiple of 4 samples and 1..{MAX_TRACKS} tracks, got n = {n}, S = {S}")
    if bed and S + 1 > MAX_TRACKS:
        raise ValueError(f"{S} talkers leave no track for a noise bed: talkers and bed share {MAX_TRACKS} tracks")
    if not segments:
        raise ValueError("a conversation holds at least one segment")
    if rooms is not None and len(rooms) != len(segments):
        raise ValueError("rooms holds one (rir, taps, direct) triple per segment")
    order = sorted(range(len(segments)), key=lambda i: (int(segments[i][6]), int(segments[i][2])))
    segs = [segments[i] for i in order]
    end = {}
    for utt, start, place, ln, _, _, trk in segs:
        if not 0 <= trk < S + bed or ln < 1 or place < 0 or place + ln > n or start < 0 or utt < 0:
            raise ValueError(f"segment {(utt, start, place, ln, trk)} does not lie inside a conversation of {n} samples and {S} tracks")
        if place < end.get(trk, 0):
            raise ValueError(f"two segments of track {trk} overlap at sample {place}")
        end[trk] = place + ln
    col = lambda i, dt: np.array([s[i] for s in segs], dtype=dt)
    room_cols = (None, None, None)
    if rooms is not None:
        rms = [tuple(int(v) for v in rooms[i]) for i in order]
        for (r, taps, direct), sg in zip(rms, segs):
            if r < -1 or not 1 <= direct <= taps <= MAX_TAPS or (r == -1 and taps != 1):
                raise ValueError(f"rooms {(r, taps, direct)}: rir >= -1, 1 <= direct <= taps <= {MAX_TAPS}, and taps = direct = 1 where rir = -1")
            if r >= 0 and int(sg[6]) == S:
                raise ValueError("a segment of the noise bed carries no response (rir = -1)")
        room_cols = tuple(np.array([m[k] for m in rms], dtype=np.int32) for k in range(3))
    return Conversation(key, n, S, col(0, np.int32), col(1, np.int32), col(2, np.int32), col(3, np.int32), col(4, np.float32),
                        col(5, np.float32), col(6, np.int32), *room_cols, int(bed))


def wsj0_speaker(name: str) -> Optional[str]:
    """The speaker of corpus utterance ``role/key`` by the rule ``datafeed.wsj0_distinct_speakers`` reads: the first three letters of the 2nd
    ``_`` field of the key for role ``s1``, of the 4th for ``s2``; ``None`` when the name does not parse."""
    role, _, key = name.partition("/")
    f = key.split("_")
    i = {"s1": 1, "s2": 3}.get(role)
    if i is None or len(f) <= i or len(f[i]) < 3:
        return None
    return f[i][:3]


def plan_conversation(corpus: Corpus, rng: random.Random, seconds: float, roles: Sequence[str] = ("s1", "s2"), speakers: int = 2,
                      overlap: Tuple[float, float] = (0.0, 0.4), pause: Tuple[float, float] = (0.0, 1.0), p_overlap: float = 0.5,
                      gain_db: Tuple[float, float] = (-2.5, 2.5), max_active: int = 2, speaker_of: Optional[Callable[[str], Optional[str]]] = None,
                      fs: Optional[int] = None, key: Optional[str] = None, rirs=None, target: str = "direct", early_ms: float = 0.0,
                      noise: Optional[str] = None, noise_db: Tuple[float, float] = (-6.0, 3.0)) -> Conversation:
    """Lay corpus utterances along ``n = seconds * fs`` samples (rounded down to a multiple of 4; ``fs`` defaults to the corpus's), one track per
    speaker.  The planner reads names, lengths and energies only - it touches no sample.

    The pool is the utterances of ``roles`` (``corpus.roles``, in file order; a corpus without roles offers all its utterances).
    ``speaker_of(name)`` names the speaker of corpus utterance ``name`` (``"role/key"``), by default ``wsj0_speaker``; an utterance it
    returns ``None`` for counts as a speaker of its own.  Draws from ``rng``, in this order:

    1. ``rng.sample`` of ``speakers`` distinct speakers from the sorted speaker names: track ``s`` belongs to the ``s``-th drawn;
    2. per utterance: its track - track 0 for the first, then ``rng.randrange`` over the tracks other than the one before (no draw for
       one or two tracks) -, ``rng.choice`` among that speaker's utterances, then the placement - the first utterance at sample 0, every
       later one either ``rng.random() < p_overlap`` and ``u = rng.uniform(*overlap)``: it starts ``round(u * min(len_prev, len_new))`` samples
       before the previous one ends, or ``rng.uniform(*pause)`` seconds after it ends -, then ``_gain(rng, *gain_db)``.

    The start is then moved later, if need be, to the first sample where the track itself is free and at most ``max_active - 1`` other tracks
    are still talking.  Every utterance is used from its first sample, RMS-normalised to the conversation's first (``_norm``) and scaled by its
    gain.  The utterance that reaches ``n`` is cut there and ends the conversation; one that would start at or after ``n`` is dropped.

    Rooms and noise (section 5h-2); with both off not one more draw is made:

    * ``rirs`` (an ``RirBank``): directly after step 1, one ``rng.randrange(len(rirs))`` per track, in track order - a talker sits still for
      the conversation.  Every segment of the track takes that response ``r`` with ``taps = len_r``; ``direct`` is the direct path the mixing
      planners use for ``target="direct"``, ``rirs._direct[r]``, plus ``round(early_ms fs / 1000)`` taps of early reflections, capped at
      ``taps``; with ``target="full"`` it is ``taps``.
    * ``noise`` (a role of the corpus): after the talker loop one ``_gain(rng, *noise_db)`` for the whole bed, then ``rng.choice`` over that
      role's utterances in file order, repeated: each is laid from its first sample where the one before ended, normalised by
      ``_norm(rms[first], rms[u])`` (``first`` the conversation's first utterance), and the last is cut at ``n`` - the bed covers ``[0, n)``
      without a gap, on track ``speakers``, with no response."""
    fs = int(fs if fs is not None else (corpus.fs or 0))
    if fs < 1:
        raise ValueError("the corpus carries no sampling rate: pass fs")
    n = int(seconds * fs) // 4 * 4
    S = int(speakers)
    if n < 4 or not 1 <= S <= MAX_TRACKS or max_active < 1:
        raise ValueError(f"a conversation needs at least 4 samples, 1..{MAX_TRACKS} speakers and max_active >= 1")
    if not (0.0 <= overlap[0] <= overlap[1] <= 1.0 and 0.0 <= pause[0] <= pause[1] and 0.0 <= p_overlap <= 1.0):
        raise ValueError("overlap is a range inside [0, 1], pause a range of non-negative seconds, p_overlap a probability")
    speaker_of = speaker_of or wsj0_speaker
    names = [f"{r}/{k}" for r in roles for k in corpus.roles.get(r, [])] or list(corpus.names)
    by_spk: Dict[str, List[int]] = {}
    for nm in names:
        spk = speaker_of(nm)
        by_spk.setdefault(f"utt:{nm}" if spk is None else f"spk:{spk}", []).append(corpus.index[nm])
    if len(by_spk) < S:
        raise ValueError(f"{S} tracks need {S} distinct speakers, the pool holds {len(by_spk)}")
    who = rng.sample(sorted(by_spk), S)
    if target not in ("direct", "full"):
        raise ValueError(f"target = {target!r}: 'direct' or 'full'")
    if noise is not None and (S + 1 > MAX_TRACKS or not corpus.roles.get(noise)):
        raise ValueError(f"a noise bed needs a role {noise!r} with utterances in the corpus and a free track beside {S} talkers")
    room_of = None
    if rirs is not None:
        extra = int(round(float(early_ms) * fs / 1000.0))
        room_of = []
        for _ in range(S):
            r = rng.randrange(len(rirs))
            taps = int(rirs.lengths[r])
            room_of.append((r, taps, taps if target == "full" else min(taps, int(rirs._direct[r]) + extra)))
    rms, lengths = corpus.rms, corpus.lengths
    end = [0] * S                                  # the sample after each track's last segment
    segs, prev, prev_len, first = [], -1, 0, -1
    while True:
        if prev < 0:
            trk = 0
        else:
            others = [s for s in range(S) if s != prev] or [prev]
            trk = others[rng.randrange(len(others))] if len(others) > 1 else others[0]
        u = int(rng.choice(by_spk[who[trk]]))
        ln = int(lengths[u])
        if prev < 0:
            place, first = 0, u
        elif S > 1 and rng.random() < p_overlap:
            place = end[prev] - int(round(rng.uniform(*overlap) * min(prev_len, ln)))
        else:
            place = end[prev] + int(round(rng.uniform(*pause) * fs))
        gain = _gain(rng, *gain_db)
        busy = sorted((end[s] for s in range(S) if s != trk), reverse=True)
        place = max(place, end[trk], busy[max_active - 1] if len(busy) >= max_active else 0)
        if place >= n:
            break
        ln = min(ln, n - place)
        segs.append((u, 0, place, ln, _norm(rms[first], rms[u]), gain, trk))
        end[trk], prev, prev_len = place + ln, trk, ln
        if end[trk] >= n:
            break
    rooms = None if room_of is None else [room_of[sg[6]] for sg in segs]
    if noise is not None:
        gain = _gain(rng, *noise_db)
        pool = [corpus.index[f"{noise}/{k}"] for k in corpus.roles[noise]]
        if any(int(lengths[u]) < 1 for u in pool):
            raise ValueError(f"role {noise!r} holds an empty utterance")
        at = 0
        while at < n:
            u = int(rng.choice(pool))
            ln = min(int(lengths[u]), n - at)
            segs.append((u, 0, at, ln, _norm(rms[first], rms[u]), gain, S))
            if rooms is not None:
                rooms.append((-1, 1, 1))
            at += ln
    return make_conversation(key if key is not None else f"conv_{corpus.names[first]}", n, S, segs, rooms=rooms, bed=noise is not None)


def overlap_fraction(conv: Conversation) -> np.ndarray:
    """float64 ``[G]``: the share of each segment's samples during which another track is active.  From the schedule alone, on the host.  A noise
    bed is ignored: it is no talker (its own segments get 0)."""
    G = len(conv.utt)
    out = np.zeros(G, dtype=np.float64)
    a, b = conv.place.astype(np.int64), conv.place.astype(np.int64) + conv.len
    talker = conv.track < conv.S
    for g in np.nonzero(talker)[0]:
        other = (conv.track != conv.track[g]) & talker
        lo, hi = np.maximum(a[other], a[g]), np.minimum(b[other], b[g])
        keep = hi > lo
        covered, reach = 0, a[g]
        for l, h in sorted(zip(lo[keep].tolist(), hi[keep].tolist())):          # the union of the other tracks' spans inside the segment
            if h > reach:
                covered += h - max(l, reach)
                reach = h
        out[g] = covered / float(b[g] - a[g])
    return out


# ---- render ---------------------------------------------------------------------------------------------------------------------------
class ConvTable:
    """The device tables of ``R`` conversations for ``sepr_conversation_render``: ``words`` int32 ``[6 G + R S_max + 1]`` - the columns utt,
    start, place, len, norm, gain (the two float32 columns as their bits), then ``track_off`` - and ``out_off`` int64 ``[R + 1]``.
    ``pack`` makes the host arrays of a list of conversations with the same ``(R, S_max, G)``; copying them into ``words`` / ``out_off``
    re-targets a captured launch.  A noise bed counts as one more track of its conversation.

    When a conversation carries rooms or a bed (``has_rooms``), ``rooms`` int32 ``[3 G]`` holds the columns rir, taps, direct of
    ``sepr_conversation_render_rooms``; ``pack_rooms`` is its half of ``pack``, and copying its result into ``rooms`` re-targets a captured
    rooms launch."""

    def __init__(self, convs: Sequence[Conversation], device):
        self.R, self.S_max, self.G = len(convs), max(c.S + c.bed for c in convs), sum(len(c.utt) for c in convs)
        words, out_off = self.pack(convs)
        self.total = int(out_off[-1])
        self.words = torch.from_numpy(words).to(device)
        self.out_off = torch.from_numpy(out_off).to(device)
        self.out_off_host = out_off
        self.has_rooms = any(c.rir is not None or c.bed for c in convs)
        self.needs_bank = False
        self.rooms = torch.from_numpy(self.pack_rooms(convs)).to(device) if self.has_rooms else None

    def pack(self, convs: Sequence[Conversation]) -> Tuple[np.ndarray, np.ndarray]:
        R, S_max, G = self.R, self.S_max, self.G
        if not 1 <= R <= 65535 or len(convs) != R or max(c.S + c.bed for c in convs) > S_max or sum(len(c.utt) for c in convs) != G:
            raise ValueError("the conversations do not fit this table's (R, S_max, G)")
        cat = lambda f, dt: np.concatenate([np.asarray(getattr(c, f), dtype=dt) for c in convs])
        counts = np.zeros(R * S_max, dtype=np.int64)
        for r, c in enumerate(convs):
            if np.any(np.diff(c.track.astype(np.int64) * (1 << 32) + c.place) < 0):
                raise ValueError(f"{c.key}: the segments are not sorted by (track, place)")
            counts[r * S_max:r * S_max + c.S + c.bed] = np.bincount(c.track, minlength=c.S + c.bed)
        words = np.concatenate([cat("utt", np.int32), cat("start", np.int32), cat("place", np.int32), cat("len", np.int32),
                                cat("norm", np.float32).view(np.int32), cat("gain", np.float32).view(np.int32),
                                np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)])
        out_off = np.concatenate([[0], np.cumsum([int(c.n) for c in convs])]).astype(np.int64)
        if any(c.n % 4 or c.n < 4 for c in convs):
            raise ValueError("every conversation holds a positive multiple of 4 samples")
        return words, out_off

    def pack_rooms(self, convs: Sequence[Conversation], rirs=None) -> np.ndarray:
        """int32 ``[3 G]``: rir, taps, direct of every segment (-1, 1, 1 for a conversation without rooms).  With ``rirs`` every response index and
        tap count is checked against the bank."""
        if len(convs) != self.R or sum(len(c.utt) for c in convs) != self.G:
            raise ValueError("the conversations do not fit this table's (R, S_max, G)")
        cols = []
        for f, fill in (("rir", -1), ("taps", 1), ("direct", 1)):
            cols.append(np.concatenate([np.full(len(c.utt), fill, dtype=np.int32) if getattr(c, f) is None else
                                        np.asarray(getattr(c, f), dtype=np.int32) for c in convs]))
        if rirs is not None:
            check_rooms(convs, rirs)
        self.needs_bank = bool((cols[0] >= 0).any())
        return np.concatenate(cols)

    def columns(self) -> List[int]:
        """Device addresses of utt, start, place, len, norm, gain and track_off."""
        p = self.words.data_ptr()
        return [p + 4 * k * self.G for k in range(7)]

    def room_columns(self) -> List[int]:
        """Device addresses of rir, taps and direct."""
        p = self.rooms.data_ptr()
        return [p + 4 * k * self.G for k in range(3)]


def check_rooms(convs: Sequence[Conversation], rirs) -> None:
    """The host's check of the rooms of ``convs`` against the bank ``rirs`` (``ValueError``): a bank as soon as any ``rir >= 0``, every
    ``rir < len(rirs)`` and every ``taps <= rirs.lengths[rir]``.  The kernel cannot make it: its tables are device memory."""
    for c in convs:
        if c.rir is None or not (c.rir >= 0).any():
            continue
        if rirs is None:
            raise ValueError(f"{c.key}: its segments name impulse responses: pass the bank as rirs=")
        wet = c.rir >= 0
        if int(c.rir.max()) >= len(rirs):
            raise ValueError(f"{c.key}: response {int(c.rir.max())} of a bank of {len(rirs)}")
        if np.any(c.taps[wet] > rirs.lengths[c.rir[wet]]):
            raise ValueError(f"{c.key}: a segment takes more taps than its response holds")


def render_into(corpus: Corpus, table: ConvTable, mix: torch.Tensor, tracks: Optional[torch.Tensor], rirs=None) -> None:
    """The one ``sepr_conversation_render`` launch on the current stream - ``sepr_conversation_render_rooms`` for a table with rooms or a bed -:
    ``mix`` float32 ``[total]``, ``tracks`` float32 ``[S_max, total]`` or ``None``.  ``rirs``: the ``RirBank`` the table's response indices
    name, on the corpus's device.  No allocation, no synchronisation: capturable, and the tables are read at replay."""
    dev = table.words.device
    if dev.type != "cuda" or corpus.device is None:
        raise RuntimeError("conversations are rendered on the HIP device, from a corpus resident there (there is no CPU path)")
    for t, shape in ((mix, (table.total,)), (tracks, (table.S_max, table.total))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"expected a contiguous float32 {shape} tensor on {dev}")
    lib = L_.load()
    out = (table.out_off.data_ptr(), table.R, table.S_max, table.G, table.total, mix.data_ptr(), None if tracks is None else tracks.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    if not table.has_rooms:
        with torch.cuda.device(dev):
            L_.check(lib.sepr_conversation_render(*corpus._corpus_args(), *table.columns(), *out, stream), "sepr_conversation_render")
        return
    if rirs is None and table.needs_bank:
        raise ValueError("the table's segments name impulse responses: pass the bank as rirs=")
    if rirs is not None and (rirs.device is None or rirs.device != torch.device(corpus.device)):
        raise ValueError(f"the RIR bank must be resident on the corpus's device {corpus.device}")
    bank = rirs._bank_args() if rirs is not None else (None, 0, None, 0)
    cols = table.columns()
    with torch.cuda.device(dev):
        L_.check(lib.sepr_conversation_render_rooms(*corpus._corpus_args(), *cols[:6], *table.room_columns(), cols[6], *out, *bank, stream),
                 "sepr_conversation_render_rooms")


class Rendered:
    """``mix`` float32 ``[total]`` with conversation ``r`` at ``out_off[r]``; ``tracks`` ``[S_max, total]`` or ``None`` - of a conversation in
    rooms the direct-path references, and after its talkers the noise bed."""

    def __init__(self, convs, table: ConvTable, mix: torch.Tensor, tracks: Optional[torch.Tensor]):
        self.convs, self.table, self.mix, self.tracks = list(convs), table, mix, tracks
        self.out_off = table.out_off_host

    def mixture(self, r: int) -> torch.Tensor:
        return self.mix[int(self.out_off[r]):int(self.out_off[r + 1])]

    def tracks_of(self, r: int) -> torch.Tensor:
        """``[S_r, n_r]`` view: the talker tracks of conversation ``r`` (row stride ``total``)."""
        if self.tracks is None:
            raise RuntimeError("rendered without tracks")
        return self.tracks[:self.convs[r].S, int(self.out_off[r]):int(self.out_off[r + 1])]

    def bed_of(self, r: int) -> Optional[torch.Tensor]:
        """``[n_r]`` view: the noise bed of conversation ``r``, or ``None`` when it has none."""
        if self.tracks is None:
            raise RuntimeError("rendered without tracks")
        c = self.convs[r]
        return self.tracks[c.S, int(self.out_off[r]):int(self.out_off[r + 1])] if c.bed else None


def render(corpus: Corpus, convs: Sequence[Conversation], tracks: bool = True, rirs=None) -> Rendered:
    """Mixture and talker tracks of every conversation, in one launch from the resident corpus.  Conversations with rooms or a noise bed go
    through ``sepr_conversation_render_rooms`` (``rirs``: the bank their response indices name; the tracks are then the direct-path references);
    all others through ``sepr_conversation_render`` as ever."""
    check_rooms(convs, rirs)
    if corpus.device is None:
        raise RuntimeError("conversations are rendered on the HIP device, from a corpus resident there (there is no CPU path)")
    table = ConvTable(convs, corpus.device)
    mix = torch.empty(table.total, dtype=torch.float32, device=corpus.device)
    trk = torch.empty(table.S_max, table.total, dtype=torch.float32, device=corpus.device) if tracks else None
    render_into(corpus, table, mix, trk, rirs=rirs)
    return Rendered(convs, table, mix, trk)


# ---- segment-wise SI-SNR --------------------------------------------------------------------------------------------------------------
def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.dtype != torch.float32 or x.device.type != "cuda":
        raise ValueError(f"{what} must be a float32 [rows, T] tensor on the HIP device (there is no CPU path)")
    return x if x.stride(1) == 1 and (x.shape[0] == 1 or x.stride(0) >= x.shape[1]) else x.contiguous()


def segment_sisnr(est: torch.Tensor, ref: torch.Tensor, mix: torch.Tensor, rows, begin, length, eps: float = 1e-15
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``sepr_segment_sisnr_fwd`` call.  ``est`` ``[C, T]``, ``ref`` ``[S, T]``, ``mix`` ``[T]`` float32 on the device, each with any row
    stride; segment ``g`` is ``ref[rows[g]][begin[g] : begin[g] + length[g]]``.  -> ``(v [G, C], v_mix [G])`` float64 on the device: the
    SI-SNR in dB of every channel, and of the mixture, against every segment over that segment's span (include/sepr.h)."""
    est, ref, mixr = _rows(est, "est"), _rows(ref, "ref"), _rows(mix, "mix")
    T = int(mixr.shape[1])
    if mixr.shape[0] != 1 or est.shape[1] != T or ref.shape[1] != T:
        raise ValueError("est, ref and mix must hold the same number of samples per row")
    C, S = int(est.shape[0]), int(ref.shape[0])
    strides = {int(x.stride(0)) for x in (est, ref) if x.shape[0] > 1}
    if len(strides) > 1:                                          # one row stride for the call: repack rows that have two
        est, ref, strides = est.contiguous(), ref.contiguous(), {T}
    ld = strides.pop() if strides else T
    seg = np.stack([np.asarray(rows, dtype=np.int32), np.asarray(begin, dtype=np.int32), np.asarray(length, dtype=np.int32)])
    G = int(seg.shape[1])
    if seg.ndim != 2 or G < 1:
        raise ValueError("rows, begin and length are one-dimensional, of the same positive length")
    if seg[0].min() < 0 or seg[0].max() >= S or seg[1].min() < 0 or seg[2].min() < 1 or int((seg[1].astype(np.int64) + seg[2]).max()) > T:
        raise ValueError("a segment lies outside ref")
    dev = est.device
    lib = L_.load()
    segd = torch.from_numpy(np.ascontiguousarray(seg)).to(dev)
    v = torch.empty(G, C, dtype=torch.float64, device=dev)
    v_mix = torch.empty(G, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, int(lib.sepr_segment_sisnr_bytes(G, C))), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L_.check(lib.sepr_segment_sisnr_fwd(est.data_ptr(), ref.data_ptr(), mixr.data_ptr(), segd[0].data_ptr(), segd[1].data_ptr(),
                                            segd[2].data_ptr(), G, C, S, T, ld, float(eps), v.data_ptr(), v_mix.data_ptr(), ws.data_ptr(),
                                            ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "sepr_segment_sisnr_fwd")
    return v, v_mix


# ---- scores ---------------------------------------------------------------------------------------------------------------------------
def overlap_bin(f: float) -> int:
    """The bin of an overlap fraction: 0 for no overlap, then (0, 0.2], (0.2, 0.5], (0.5, 1]."""
    return 0 if f <= 0.0 else (1 if f <= 0.2 else (2 if f <= 0.5 else 3))


def _mean(x: np.ndarray) -> float:
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else float("nan")


def colour(v, begin, length, C: int) -> Optional[np.ndarray]:
    """The consistent assignment for any number of talkers: ``v [G][C]`` the scores of one conversation's segments
    on every channel, ``begin``, ``length [G]`` their scored spans.  Segments ``g`` and ``h`` are adjacent iff ``[begin, begin + length)`` of
    the two intersect - spans that only abut are not -, an assignment ``a: g -> channel`` is valid iff adjacent segments differ, and the
    result is the valid ``a`` (int64 ``[G]``, by table index) maximising ``sum_g v[g][a(g)]``: the total accumulated in float64 from 0.0, left
    to right over the segments ordered by ``(begin, table index)``; on a tie the lexicographically first ``(a(g_0), a(g_1), ..)`` in that
    order.  ``None`` when more than ``C`` segments are open at once: there is no colouring.

    The graph is an interval graph, so this is a sweep over the ordered segments whose state is the channels of the segments still open -
    at most ``C`` of them, hence at most ``C! / (C - k)!`` states, never ``C^G`` assignments.  Two prefixes that reach the same open state
    are merged: the larger total is kept, and on equal totals the lexicographically smaller prefix.  That is exact, because float addition
    is monotone - ``s <= t`` implies ``fl(s + x) <= fl(t + x)`` -, so whatever follows, the kept prefix ends at least as high as the
    dropped one, and a prefix with the very same total ends at the very same total.  One caveat: a strict gap between two prefixes can
    round to a tie further on; the enumeration would then take the lexicographically first of the two, the sweep has kept the one that was
    ahead."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, int(C))
    b = np.asarray(begin, dtype=np.int64).reshape(-1)
    e = b + np.asarray(length, dtype=np.int64).reshape(-1)
    G, C = v.shape[0], int(C)
    if b.shape[0] != G or e.shape[0] != G or G < 1:
        raise ValueError("one row of v, begin and length per segment, and at least one segment")
    order = sorted(range(G), key=lambda g: (int(b[g]), g))
    open_: List[int] = []                                          # positions (in order) of the segments still open, ascending
    states: Dict[Tuple[int, ...], Tuple[float, Tuple[int, ...]]] = {(): (0.0, ())}      # channels of the open segments -> (total, prefix)
    for j, g in enumerate(order):
        keep = [i for i, p in enumerate(open_) if e[order[p]] > b[g]]
        if len(keep) >= C:
            return None
        open_ = [open_[i] for i in keep] + [j]
        nxt: Dict[Tuple[int, ...], Tuple[float, Tuple[int, ...]]] = {}
        for st, (tot, pre) in states.items():
            held = tuple(st[i] for i in keep)
            for c in range(C):
                if c in held:
                    continue
                cand = (tot + v[g, c], pre + (c,))
                old = nxt.get(held + (c,))
                if old is None or cand[0] > old[0] or (cand[0] == old[0] and cand[1] < old[1]):
                    nxt[held + (c,)] = cand
        states = nxt
    top = None
    for tot, pre in states.values():
        if top is None or tot > top[0] or (tot == top[0] and pre < top[1]):
            top = (tot, pre)
    out = np.empty(G, dtype=np.int64)
    out[np.asarray(order)] = np.asarray(top[1], dtype=np.int64)
    return out


def frame_classes(conv_spans, coloured, n: int, C: int, frame: int, collar: int) -> np.ndarray:
    """uint8 ``[C][nF]``, ``nF = ceil(n / frame)``: the class of every frame ``[f frame, min(n, (f + 1) frame))`` of every channel of one
    conversation of ``n`` samples.  ``conv_spans = (begin, length)``: the scored spans of its segments, ``coloured [G]`` their channels
    (``colour``; -1: none).  For channel ``c`` the first rule that holds:

    * 0 (own): the frame intersects a scored span coloured ``c``;
    * 3 (collar): it intersects such a span widened by ``collar`` samples on both sides;
    * 1 (cross): it intersects any talker's widened span;
    * 2 (quiet): nothing of the above.

    The idle classes 1 and 2 therefore hold only frames that lie entirely outside every span that ``c`` owns, collar included."""
    begin, length = (np.asarray(x, dtype=np.int64).reshape(-1) for x in conv_spans)
    coloured = np.asarray(coloured, dtype=np.int64).reshape(-1)
    n, C, frame, collar = int(n), int(C), int(frame), int(collar)
    if n < 1 or frame < 1 or collar < 0 or C < 1 or not (begin.shape == length.shape == coloured.shape):
        raise ValueError("n, frame and C are positive, collar is not negative, and begin, length and coloured hold one value per segment")
    nF = -(-n // frame)
    cls = np.full((C, nF), 2, dtype=np.uint8)

    def frames(lo, hi):                                            # the frames that [lo, hi) clipped to [0, n) intersects
        lo, hi = max(0, int(lo)), min(n, int(hi))
        return slice(lo // frame, (hi - 1) // frame + 1) if hi > lo else slice(0, 0)

    for b, ln in zip(begin, length):
        cls[:, frames(b - collar, b + ln + collar)] = 1
    for c in range(C):
        own = np.nonzero(coloured == c)[0]
        for g in own:
            cls[c, frames(begin[g] - collar, begin[g] + length[g] + collar)] = 3
        for g in own:
            cls[c, frames(begin[g], begin[g] + length[g])] = 0
    return cls


def idle_figures(sums, eps: float = 1e-15) -> dict:
    """The idle figures from class sums ``[..., 4, 4]`` (``activity.frame_class_sums``: per class the frames, the active frames, the sum of
    ``e_est``, the sum of ``e_mix``), each of the leading shape: ``leak_db = 10 log10((sum e_est + eps) / (sum e_mix + eps))`` over class 1,
    NaN where it has no frame or no mixture energy; ``quiet_db`` the same over class 2; ``false_alarm`` = active / all frames of the classes 1
    and 2 together; ``miss`` = inactive / all frames of class 0; NaN where there is no such frame."""
    s = np.asarray(sums, dtype=np.float64)
    nan = np.full(s.shape[:-2], np.nan)

    def db(k):
        ok = (s[..., k, 0] > 0) & (s[..., k, 3] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(ok, 10.0 * np.log10((s[..., k, 2] + eps) / (s[..., k, 3] + eps)), nan)

    n_idle, a_idle = s[..., 1, 0] + s[..., 2, 0], s[..., 1, 1] + s[..., 2, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        fa = np.where(n_idle > 0, a_idle / n_idle, nan)
        miss = np.where(s[..., 0, 0] > 0, (s[..., 0, 0] - s[..., 0, 1]) / s[..., 0, 0], nan)
    return {"leak_db": db(1), "quiet_db": db(2), "false_alarm": fa, "miss": miss}


def score(v, v_mix, conv_of, track, S_of, C: int, overlap=None, spans=None) -> dict:
    """Scores from the two matrices of ``segment_sisnr`` - pure host arithmetic, after one copy.  ``conv_of [G]``: the conversation of each
    segment, ``track [G]``: its track, ``S_of[r]``: the tracks of conversation ``r``, ``C``: the separator's channels.

    * ``best[g]``: the lowest channel attaining ``max_c v[g][c]``; ``utt[g] = v[g][best[g]] - v_mix[g]``.
    * A conversation with ``S <= C``: the injective track -> channel assignment ``pi`` maximising ``sum_g v[g][pi(track_g)]`` - the sum
      taken per (track, channel) in segment order and then over the tracks in order, ties to the lexicographically first ``pi`` -,
      ``cons[g] = v[g][pi(track_g)] - v_mix[g]``, ``assigned[g] = pi(track_g)``, ``switch[g] = best[g] != assigned[g]``.
    * ``S > C``: ``cons`` and ``switch`` are NaN, ``assigned`` is -1, and the means leave them out.

    Means: ``sisnri_utt``, ``sisnri_cons``, ``switch_rate``; with ``overlap`` (``overlap_fraction`` per segment) also ``bins``: per overlap bin
    ``{"n", "sisnri_utt", "sisnri_cons"}`` in the order of ``OVERLAP_BINS``.

    ``spans = (begin [G], length [G])``, the scored spans: the dict gains the assignment that exists for any number of talkers (``colour``,
    per conversation) - ``coloured [G]`` (-1 where a conversation has no colouring), ``graph[g] = v[g][coloured[g]] - v_mix[g]`` (NaN
    there), their mean ``sisnri_graph``, ``bins[*]["sisnri_graph"]`` and ``graph_switch_rate``, the share of coloured segments with
    ``best != coloured``.  Without ``spans`` the dict is as it always was."""
    v = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64).reshape(-1, int(C))
    v_mix = (v_mix.detach().cpu().numpy() if isinstance(v_mix, torch.Tensor) else np.asarray(v_mix)).astype(np.float64).reshape(-1)
    conv_of, track = np.asarray(conv_of, dtype=np.int64), np.asarray(track, dtype=np.int64)
    G = v.shape[0]
    if not (v_mix.shape[0] == conv_of.shape[0] == track.shape[0] == G):
        raise ValueError("one row of v, v_mix, conv_of and track per segment")
    best = np.argmax(v, axis=1).astype(np.int64)                  # numpy's argmax returns the first maximum: the lowest channel
    utt = v[np.arange(G), best] - v_mix
    cons = np.full(G, np.nan)
    switch = np.full(G, np.nan)
    assigned = np.full(G, -1, dtype=np.int64)
    assignment: Dict[int, Optional[Tuple[int, ...]]] = {}
    for r in sorted(set(conv_of.tolist())):
        S = int(S_of[r])
        idx = np.nonzero(conv_of == r)[0]
        if S > C:
            assignment[r] = None
            continue
        M = np.zeros((S, C))
        for g in idx:                                             # in segment order
            M[track[g]] += v[g]
        top, pi = -np.inf, None
        for cand in itertools.permutations(range(C), S):          # lexicographic order; a later candidate must be strictly better
            tot = 0.0
            for s in range(S):
                tot += M[s, cand[s]]
            if pi is None or tot > top:
                top, pi = tot, cand
        assignment[r] = pi
        assigned[idx] = np.asarray(pi, dtype=np.int64)[track[idx]]
        cons[idx] = v[idx, assigned[idx]] - v_mix[idx]
        switch[idx] = (best[idx] != assigned[idx]).astype(np.float64)
    out = {"best": best, "assigned": assigned, "utt": utt, "cons": cons, "switch": switch, "assignment": assignment,
           "sisnri_utt": _mean(utt), "sisnri_cons": _mean(cons), "switch_rate": _mean(switch), "n": int(G)}
    if overlap is not None:
        ov = np.asarray(overlap, dtype=np.float64)
        which = np.array([overlap_bin(f) for f in ov])
        out["overlap"] = ov
        out["bins"] = {name: {"n": int((which == k).sum()), "sisnri_utt": _mean(utt[which == k]), "sisnri_cons": _mean(cons[which == k])}
                       for k, name in enumerate(OVERLAP_BINS)}
    if spans is not None:
        begin, length = (np.asarray(x, dtype=np.int64).reshape(-1) for x in spans)
        if not (begin.shape[0] == length.shape[0] == G):
            raise ValueError("spans holds one begin and one length per segment")
        coloured = np.full(G, -1, dtype=np.int64)
        for r in sorted(set(conv_of.tolist())):
            idx = np.nonzero(conv_of == r)[0]
            a = colour(v[idx], begin[idx], length[idx], C)
            if a is not None:
                coloured[idx] = a
        has = coloured >= 0
        graph = np.full(G, np.nan)
        graph[has] = v[has, coloured[has]] - v_mix[has]
        gsw = np.full(G, np.nan)
        gsw[has] = (best[has] != coloured[has]).astype(np.float64)
        out.update(coloured=coloured, graph=graph, sisnri_graph=_mean(graph), graph_switch_rate=_mean(gsw))
        if overlap is not None:
            for k, name in enumerate(OVERLAP_BINS):
                out["bins"][name]["sisnri_graph"] = _mean(graph[which == k])
    return out
