"""Training windows cut out of planned conversations.

    feed = ConversationWindowFeed(corpus, batch=16, max_len=32000, channels=2, rirs=bank,
                                  planner=functools.partial(plan_conversation, speakers=3, max_active=2, noise="noise"))
    Trainer(model, feed, valid, "checkpoints/", criterion="graph_sasdr").run()

``DynamicMixFeed`` draws one turn per talker and window, with exactly ``num_spks`` talkers.  A window of a conversation holds a varying
number of utterances, a talker can have two of them, and there can be more talkers than output channels.  This feed plans ``conversations``
conversations per epoch with ``conversation.plan_conversation``, cuts them into windows of ``max_len`` samples and hands each window out as

* the mixture - every segment the window hears, the reverberation of segments that ended before it included;
* up to ``rows`` target ROWS, one per utterance whose direct path meets the window, each with its span ``[on, off)``;
* the adjacency mask: which rows talk at the same time and so may not share an output channel.

``criterion.GraphPIT`` turns rows, spans and mask into one target per output channel.  A batch is ONE ``sepr_conversation_render`` /
``sepr_conversation_render_rooms`` launch over ``R = batch`` window schedules of ``n = max_len``: a row is a track of its window's schedule.
``window_schedule`` is the host-only statement of a window; tests/graphpit_ref.py restates it.
"""
from __future__ import annotations

import functools
from typing import Callable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .conversation import MAX_TRACKS, Conversation, ConvTable, plan_conversation, render_into
from .datafeed import Corpus, FeedOrder, _same_device


class Window(NamedTuple):
    conv: Conversation               # the window's schedule: n = T, S = the feed's rows, track = row, place relative to the window
    spans: np.ndarray                # int32 [U, 2]: the direct-path support of each row clipped to the window; (0, 0) for a row that has none
    adj: np.ndarray                  # int64 [U]: bit v of adj[u] = the dry talk spans of rows u and v intersect inside the window
    used: int                        # rows in use
    talker: np.ndarray               # int32 [U]: the conversation track of each row, -1 past ``used``


class WindowPlan(NamedTuple):
    windows: Tuple[Window, ...]
    spans: np.ndarray                # int32 [B, U, 2]
    adj: np.ndarray                  # int64 [B, U]
    keys: List[str]
    n: np.ndarray                    # int64 [B]: every row holds max_len samples


def window_rows(rows: int, bed: bool) -> int:
    """The rows of a window of a feed asked for ``rows``: talker rows and a noise bed share the 8 tracks of a render launch."""
    rows = int(rows)
    if not 1 <= rows <= MAX_TRACKS:
        raise ValueError(f"rows: 1..{MAX_TRACKS}, got {rows}")
    return min(rows, MAX_TRACKS - 1) if bed else rows


def window_schedule(conv: Conversation, w0: int, T: int, rows: int) -> Optional[Window]:
    """The window ``[w0, w0 + T)`` of ``conv`` as a schedule of its own, or ``None`` when it needs more than ``rows`` rows.

    The schedule is the conversation's shifted by ``-w0``, nothing clipped: ``place' = place - w0``.  A segment is kept iff its wet support
    ``[place', place' + len + taps - 1)`` meets ``[0, T)``.  Rows are numbered over the kept talker segments in ``(track, place)`` order, one per
    segment whose direct-path support ``[place', place' + len + direct - 1)`` meets the window; the row's span is that support clipped to the
    window.  A segment of which only the tail reaches the window is heard in the mixture but is nobody's target: it lies on the row of its
    talker's next segment in the window, and where there is none the talker's tail-only segments share a row with an empty span.  The bed's
    segments lie on track ``rows``, after every row."""
    w0, T, U = int(w0), int(T), int(rows)
    G = len(conv.utt)
    place = conv.place.astype(np.int64) - w0
    ln = conv.len.astype(np.int64)
    taps = np.ones(G, dtype=np.int64) if conv.taps is None else conv.taps.astype(np.int64)
    direct = np.ones(G, dtype=np.int64) if conv.direct is None else conv.direct.astype(np.int64)
    rir = np.full(G, -1, dtype=np.int64) if conv.rir is None else conv.rir.astype(np.int64)
    kept = (place < T) & (place + ln + taps - 1 > 0)
    has_row = kept & (place + ln + direct - 1 > 0)
    seg_row = np.full(G, -1, dtype=np.int64)
    main: List[int] = []                                           # the segment that gives each row its span, -1 for a row of tails
    talker: List[int] = []
    for s in range(conv.S):
        pending: List[int] = []
        for g in np.nonzero(kept & (conv.track == s))[0]:          # sorted by place
            if has_row[g]:
                seg_row[g] = len(main)
                seg_row[pending] = len(main)
                pending = []
                main.append(int(g))
                talker.append(s)
            else:
                pending.append(int(g))
        if pending:
            seg_row[pending] = len(main)
            main.append(-1)
            talker.append(s)
    used = len(main)
    if used > U:
        return None
    spans = np.zeros((U, 2), dtype=np.int32)
    dry = np.zeros((U, 2), dtype=np.int64)
    for u, g in enumerate(main):
        if g >= 0:
            spans[u] = max(0, place[g]), min(T, place[g] + ln[g] + direct[g] - 1)
            dry[u] = max(0, place[g]), max(max(0, place[g]), min(T, place[g] + ln[g]))
    adj = np.zeros(U, dtype=np.int64)
    for u in range(used):
        for v in range(used):
            if u != v and max(dry[u, 0], dry[v, 0]) < min(dry[u, 1], dry[v, 1]):
                adj[u] |= 1 << v
    talk = np.nonzero(seg_row >= 0)[0]
    talk = talk[np.lexsort((place[talk], seg_row[talk]))]          # by (row, place)
    bed = np.nonzero(kept & (conv.track == conv.S))[0] if conv.bed else np.zeros(0, dtype=np.int64)
    order = np.concatenate([talk, bed]).astype(np.int64)
    if order.size == 0:
        # silence: one segment that ends before the window keeps the tables non-empty and renders nothing
        order = np.zeros(1, dtype=np.int64)
        place = place.copy()
        place[0] = -int(ln[0]) - int(taps[0]) - 4
        seg_row[0] = 0
    track = np.where(conv.track[order] == conv.S, U, seg_row[order]).astype(np.int32) if conv.bed else seg_row[order].astype(np.int32)
    rooms = conv.rir is not None
    w = Conversation(f"{conv.key}@{w0}", T, U, conv.utt[order].astype(np.int32), conv.start[order].astype(np.int32), place[order].astype(np.int32),
                     conv.len[order].astype(np.int32), conv.norm[order].astype(np.float32), conv.gain[order].astype(np.float32), track,
                     rir[order].astype(np.int32) if rooms else None, taps[order].astype(np.int32) if rooms else None,
                     direct[order].astype(np.int32) if rooms else None, int(conv.bed))
    return Window(w, spans, adj, used, np.array(talker + [-1] * (U - used), dtype=np.int32))


def window_starts(n: int, offset: int, T: int) -> List[int]:
    """``offset + k T`` while the window fits inside ``[0, n)``."""
    return list(range(int(offset), int(n) - int(T) + 1, int(T)))


class _WindowTable(ConvTable):
    """``ConvTable`` for a feed: one device buffer of growing capacity that every batch's tables are copied into through pinned staging, so a
    batch costs one asynchronous copy and no wait.  ``(R, S_max)`` are fixed, ``G`` follows the batch, every ``n`` is ``T``."""

    SLOTS = 4

    def __init__(self, R: int, S_max: int, T: int, device):
        self.R, self.S_max, self.G = int(R), int(S_max), 0
        self.device = torch.device(device)
        self.total = self.R * int(T)
        self.out_off_host = (np.arange(self.R + 1, dtype=np.int64) * int(T))
        self.out_off = torch.from_numpy(self.out_off_host).to(self.device)
        self.has_rooms, self.needs_bank = False, False
        self.words = self.rooms = None
        self._dev: Optional[torch.Tensor] = None
        self._stage: List[torch.Tensor] = []
        self._events: list = []
        self._slot = 0

    def set(self, convs: Sequence[Conversation], rirs=None) -> None:
        self.G = sum(len(c.utt) for c in convs)
        words, out_off = self.pack(convs)
        if not np.array_equal(out_off, self.out_off_host):
            raise ValueError("every window of a batch holds max_len samples")
        self.has_rooms = any(c.rir is not None or c.bed for c in convs)
        rooms = self.pack_rooms(convs, rirs) if self.has_rooms else np.zeros(0, dtype=np.int32)
        nw = (len(words) + 3) // 4 * 4
        need = nw + len(rooms)
        if self._dev is None or self._dev.numel() < need:
            cap = max(1024, 2 * need)
            self._dev = torch.empty(cap, dtype=torch.int32, device=self.device)
            self._stage = [torch.empty(cap, dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)]
            self._events = [None] * self.SLOTS
        k = self._slot
        self._slot = (k + 1) % self.SLOTS
        if self._events[k] is not None:
            self._events[k].synchronize()               # the copy that last read this staging buffer has run (SLOTS batches ago)
        host = self._stage[k].numpy()
        host[:len(words)] = words
        host[nw:need] = rooms
        self._dev[:need].copy_(self._stage[k][:need], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._events[k] = ev
        self.words = self._dev[:len(words)]
        self.rooms = self._dev[nw:need] if self.has_rooms else None


class ConversationWindowFeed:
    """``for input_sizes, mixture, rows, keys in feed`` - ``DynamicMixFeed``'s protocol (``batch``, ``max_len``, ``fixed_length``, ``plans()``,
    ``write(plan, x, rows)``, ``last_plan``, ``state_dict()`` / ``load_state_dict()``) with ``rows`` target rows in the place of the sources and,
    on every plan, the ``spans`` and ``adj`` tables ``criterion.GraphPIT.load`` takes.

    Per epoch: ``conversations`` conversations of ``seconds`` seconds are planned with the feed's ``random.Random(seed)`` (``planner(corpus, rng,
    seconds=, key=)``, ``rirs=`` bound on when the feed has a bank), each followed by its one offset ``rng.randrange(0, max_len, 4)``; windows of
    ``max_len`` samples start at ``offset + k max_len`` while they fit.  Windows that need more than ``rows`` rows are dropped and counted in
    ``dropped`` (with a noise bed at most 7 rows fit beside it: ``rows`` then reads ``min(rows, 7)``).  The epoch's windows are shuffled with the
    same generator and cut into batches; a trailing partial batch is dropped.  ``max_active`` of the planner above ``channels`` is refused: the
    planner's rule then bounds the overlap depth of the talk spans by ``channels``, so every window's graph has a colouring.
    ``rank`` / ``world``: this rank's contiguous shard of the shuffled windows (untested in a data-parallel run)."""

    fixed_length = True

    def __init__(self, corpus: Corpus, batch: int, max_len: int, channels: int, rows: int = 8, conversations: int = 32, seconds: float = 120.0,
                 planner: Callable[..., Conversation] = functools.partial(plan_conversation, speakers=3, max_active=2), seed: int = 0,
                 rirs=None, rank: int = 0, world: int = 1):
        if batch < 1 or max_len < 4 or max_len % 4:
            raise ValueError("batch >= 1 and max_len a positive multiple of 4")
        if conversations < 1 or not 1 <= int(channels) <= 3:
            raise ValueError("conversations >= 1 and 1..3 channels")
        kw = getattr(planner, "keywords", None) or {}
        max_active = int(kw.get("max_active", 2))
        if max_active > int(channels):
            raise ValueError(f"the planner lets {max_active} talkers speak at once, the separator has {channels} channels: no colouring of such a "
                             "window exists - bind max_active <= channels")
        if rirs is not None and corpus.device is not None and not _same_device(rirs.device, corpus.device):
            raise ValueError(f"the RIR bank is on {rirs.device}, the corpus on {corpus.device}")
        self.corpus, self.batch, self.max_len, self.channels = corpus, int(batch), int(max_len), int(channels)
        self.bed = kw.get("noise") is not None
        self.rows = window_rows(rows, self.bed)
        self.conversations, self.seconds, self.rirs, self.rank, self.world = int(conversations), float(seconds), rirs, rank, world
        self.planner = planner if rirs is None or "rirs" in kw else functools.partial(planner, rirs=rirs)
        self.order = FeedOrder([], self.batch, seed, None, rank, world, True, fixed_length=True)
        self.dropped = 0
        self.last_plan: Optional[WindowPlan] = None
        self._table: Optional[_WindowTable] = None
        self._tracks: Optional[torch.Tensor] = None
        self._mix: Optional[torch.Tensor] = None
        self._sizes = torch.full((self.batch,), float(self.max_len))
        self._epoch: Optional[Iterator[WindowPlan]] = None

    rng = property(lambda self: self.order.rng)
    epoch = property(lambda self: self.order.epoch, lambda self, v: setattr(self.order, "epoch", int(v)))

    def state_dict(self) -> dict:
        """What a checkpoint written between epochs keeps of the feed: the generator's state and the epoch counter."""
        return self.order.state_dict()

    def load_state_dict(self, state: dict) -> None:
        self.order.load_state_dict(state)
        self._epoch = None                              # a batch iterator in flight belonged to the state that was replaced

    # ---- host side ---------------------------------------------------------------------------------------------------------
    def epoch_windows(self) -> List[Window]:
        """Plan the epoch's conversations, cut them, drop what does not fit, shuffle: the epoch's windows in batch order."""
        from .dist import shard_range
        epoch, self.epoch = self.epoch, self.epoch + 1
        T = self.max_len
        out: List[Window] = []
        for i in range(self.conversations):
            conv = self.planner(self.corpus, self.rng, seconds=self.seconds, key=f"e{epoch}c{i}")
            if bool(conv.bed) != self.bed:
                raise ValueError("the planner's conversations carry a noise bed the feed did not read off its keywords (bind noise= with "
                                 "functools.partial)" if conv.bed else "the planner was bound with noise= but made a conversation without a bed")
            offset = self.rng.randrange(0, T, 4)
            for w0 in window_starts(conv.n, offset, T):
                w = window_schedule(conv, w0, T, self.rows)
                if w is None:
                    self.dropped += 1
                else:
                    out.append(w)
        self.rng.shuffle(out)
        lo, hi = shard_range(len(out), self.rank, self.world)
        return out[lo:hi]

    def plans(self) -> Iterator[WindowPlan]:
        """The batch plans of one epoch (host only)."""
        wins = self.epoch_windows()
        B = self.batch
        for i in range(0, len(wins) - len(wins) % B, B):
            ws = tuple(wins[i:i + B])
            yield WindowPlan(ws, np.stack([w.spans for w in ws]), np.stack([w.adj for w in ws]), [w.conv.key for w in ws],
                             np.full(B, self.max_len, dtype=np.int64))

    # ---- device side -------------------------------------------------------------------------------------------------------
    def _launch(self, plan: WindowPlan, x: torch.Tensor, rows: Sequence[torch.Tensor]) -> None:
        dev = self.corpus.device
        if dev is None:
            raise RuntimeError("ConversationWindowFeed renders on the HIP device, from a corpus resident there (there is no CPU path)")
        B, T, U = self.batch, self.max_len, self.rows
        rows = list(rows)
        if len(rows) != U or tuple(x.shape) != (B, T) or not x.is_contiguous() or any(tuple(r.shape) != (B, T) for r in rows):
            raise ValueError(f"write: x and {U} rows, contiguous float32 [{B}, {T}]")
        if self._table is None:
            self._table = _WindowTable(B, U + self.bed, T, dev)
            self._tracks = torch.empty(U + self.bed, B * T, dtype=torch.float32, device=dev)
        self._table.set([w.conv for w in plan.windows], self.rirs)
        render_into(self.corpus, self._table, x.view(B * T), self._tracks, rirs=self.rirs)
        for u in range(U):
            rows[u].copy_(self._tracks[u].view(B, T))
        self.last_plan = plan

    def write(self, plan: WindowPlan, x: torch.Tensor, rows: Sequence[torch.Tensor]) -> None:
        """Render the batch of ``plan`` (one of ``plans()``) into ``x [B, max_len]`` and the ``rows`` tensors ``[B, max_len]``."""
        self._launch(plan, x, rows)

    def next_plan(self) -> WindowPlan:
        """The next batch plan, running on into the next epoch when one ends."""
        for _ in range(2):
            if self._epoch is None:
                self._epoch = self.plans()
            plan = next(self._epoch, None)
            if plan is not None:
                return plan
            self._epoch = None
        raise ValueError(f"an epoch of this feed holds fewer than {self.batch} windows")

    def next_into(self, x: torch.Tensor, rows: Sequence[torch.Tensor]) -> WindowPlan:
        """Render the next batch into ``x`` and ``rows``, e.g. ``step.x`` and ``step.targets`` of a ``CapturedTrainStep``.  Returns the plan:
        its ``spans`` and ``adj`` are what ``GraphPIT.load`` takes before the step runs."""
        plan = self.next_plan()
        self._launch(plan, x, rows)
        return plan

    def bed_track(self) -> Optional[torch.Tensor]:
        """``[B, max_len]`` view of the noise bed of the batch written last, or ``None`` for a feed without one."""
        return self._tracks[self.rows].view(self.batch, self.max_len) if self.bed and self._tracks is not None else None

    def __iter__(self):
        dev = self.corpus.device
        for plan in self.plans():
            x = torch.empty(self.batch, self.max_len, dtype=torch.float32, device=dev)
            rows = [torch.empty_like(x) for _ in range(self.rows)]
            self._launch(plan, x, rows)
            yield self._sizes.clone(), x, rows, plan.keys
