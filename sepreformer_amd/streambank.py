"""The stream bank: continuous batching of live and queued recordings.

``separate_long`` needs a whole recording before it starts and never puts the windows of two recordings into one forward.  A
``StreamBank`` keeps, for each of its ``slots``, the stitch state of one stream on the device - the raw tail of its latest window, its
track permutation and its float64 gains (``include/sepr.h`` sepr_streambank_step, csrc/sepr_stitch.hip) - and advances it one window
at a time.  One ``step()`` is one hop: one gather launch forms the ``[A, W]`` input from the pending samples of every stream that has
a window ready, one ``model(x)`` at batch ``A`` separates them, one step launch aligns each window with its stream's saved tail
(the permutation, the optional gain, the sin^2 crossfade of the offline stitch, with the same arithmetic in the same order) and emits
the samples that have become final.  The per-hop tables travel through pinned staging in a ring guarded by events; a hop never
drains the queue.

Latency, stated plainly: a sample waits between ``O`` and ``W`` samples of audio - the rest of its window, whose first ``H`` samples
are final once the window has run - plus one hop's compute before it is emitted.  The models are non-causal: this is chunked-online
operation, not low-latency streaming.

What a stream receives equals ``longform.stitch`` of the windows the bank ran for it, bit for bit; with one slot (batch-1 forwards) it
equals ``separate_long(model, x, batch=1)``.  Out of scope: resampling inside the bank (convert before ``push``), more than one device,
threads (one bank is driven by one thread).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .longform import _as_list, check_geometry

STEP_COLS, GATHER_COLS = 6, 3          # include/sepr.h: slot, k, n_emit, has_window, out offset, track stride | base, start, received


def next_action(received: int, k: int, closed: bool, W: int, O: int) -> Optional[Tuple[str, int, bool]]:
    """What the next hop does for a stream that has received ``received`` samples and run ``k`` windows: ``None`` (nothing ready) or
    ``(kind, n_emit, finishes)`` with kind ``"window"`` (run window ``k`` and emit ``n_emit`` samples from ``kH``), ``"flush"`` (no
    window: emit the saved tail, the stream ended on a full window), ``"short"`` (a closed stream of at most ``W`` samples that never
    ran a window: the ``separate`` path) or ``"empty"`` (closed without a sample)."""
    H = W - O
    if not closed:
        return ("window", H, False) if received >= k * H + W else None
    T = received
    if T == 0:
        return ("empty", 0, True)
    if k == 0 and T <= W:
        return ("short", T, True)
    rem = T - k * H
    if rem > W:
        return ("window", H, False)
    if k == 0 or rem > O:
        return ("window", rem, True)
    return ("flush", rem, True)                    # rem == O: window k - 1 ended exactly at T


class _Stream:
    __slots__ = ("sid", "received", "k", "closed")

    def __init__(self, sid: int):
        self.sid, self.received, self.k, self.closed = sid, 0, 0, False


class SlotTable:
    """The bank's host-side bookkeeping, free of any device: which stream holds which slot, what each has received and run, whether a
    push fits the store of ``cap`` samples, and what the next hop does (``next_action``)."""

    def __init__(self, slots: int, W: int, O: int, cap: int):
        if slots < 1:
            raise ValueError("slots must be at least 1")
        if cap < W:
            raise ValueError("the store must hold at least one window")
        self.slots, self.W, self.O, self.H, self.cap = int(slots), W, O, W - O, int(cap)
        self.streams: List[Optional[_Stream]] = [None] * self.slots
        self.slot_of: Dict[int, int] = {}
        self._next_sid = 0

    def open(self) -> int:
        for slot, st in enumerate(self.streams):
            if st is None:
                sid = self._next_sid
                self._next_sid += 1
                self.streams[slot] = _Stream(sid)
                self.slot_of[sid] = slot
                return sid
        raise RuntimeError(f"no free slot: all {self.slots} are in use")

    def free_slots(self) -> int:
        return sum(st is None for st in self.streams)

    def lookup(self, sid: int) -> Tuple[int, _Stream]:
        if sid not in self.slot_of:
            raise KeyError(f"stream {sid} is not open")
        slot = self.slot_of[sid]
        return slot, self.streams[slot]

    def push(self, sid: int, n: int) -> Tuple[int, int]:
        """Account for ``n`` more samples of stream ``sid`` -> (its slot, the ring index they start at)."""
        slot, st = self.lookup(sid)
        if st.closed:
            raise RuntimeError(f"stream {sid} is closed")
        pending = st.received - st.k * self.H                   # the samples from the next window's start on are still needed
        if pending + n > self.cap:
            raise OverflowError(f"stream {sid}: {n} more samples overflow the store of {self.cap} ({pending} pending); "
                                "call step() first or size the bank with store_seconds")
        p0 = st.received % self.cap
        st.received += n
        return slot, p0

    def close(self, sid: int) -> None:
        self.lookup(sid)[1].closed = True

    def plan(self) -> List[Tuple[int, _Stream, Tuple[str, int, bool]]]:
        """(slot, stream, action) of every stream the next hop serves, in slot order."""
        acts = []
        for slot, st in enumerate(self.streams):
            act = None if st is None else next_action(st.received, st.k, st.closed, self.W, self.O)
            if act is not None:
                acts.append((slot, st, act))
        return acts

    def done(self, slot: int, act: Tuple[str, int, bool]) -> None:
        """The hop has served ``slot`` with ``act``: a window advances the stream, a finishing action frees the slot - its next
        occupant starts at k = 0, which resets the device state."""
        st = self.streams[slot]
        if act[0] == "window":
            st.k += 1
        if act[2]:
            self.streams[slot] = None
            del self.slot_of[st.sid]


class StreamBank:
    """``StreamBank(model, slots=32, chunk_seconds=4.0, overlap_seconds=1.0, fs=8000, match_gain=False)``.

    ``open() -> sid``; ``push(sid, samples)`` (1-D tensor or array, host or device, any length, at the model's rate); ``close(sid)``
    marks the end; ``step()`` runs ONE hop and returns ``{sid: [S, n] device tensor}``, the samples that became final, valid until the
    next ``step()``; ``ready()`` is the number of streams a ``step()`` would serve; ``drain()`` steps until nothing is pending.
    A stream has a window ready when it has received ``kH + W`` samples, or when it is closed and a last window or the flush of its
    tail is pending.  A closed stream of at most ``W`` samples that never ran a window is ``infer.separate(model, x)`` itself.  A closed
    stream whose last samples have been returned frees its slot.  The model is put in ``eval()``; the auxiliary heads are switched off
    around the bank's forwards and restored.  A sample waits between ``O`` and ``W`` samples of audio plus one hop's compute before it is
    emitted: chunked-online, not low-latency (the models are non-causal).  No resampling, one device, one driving thread.

    ``store_seconds``: pending-sample store per slot (default ``2 W + H`` samples; at least ``W`` plus the largest push).
    ``keep_windows=True`` (debugging) keeps every window output the bank ran, per stream, in ``kept[sid]`` as ``[S, W]`` tensors."""

    def __init__(self, model, slots: int = 32, chunk_seconds: float = 4.0, overlap_seconds: float = 1.0, fs: int = 8000,
                 match_gain: bool = False, store_seconds: Optional[float] = None, keep_windows: bool = False):
        cfg = model.cfg
        self.W, self.O = int(round(chunk_seconds * fs)), int(round(overlap_seconds * fs))
        check_geometry(self.W, self.O, cfg.enc_stride, cfg.enc_kernel)
        self.H, self.S, self.slots = self.W - self.O, int(model.num_spks), int(slots)
        self.model, self.match_gain = model.eval(), bool(match_gain)
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("the stream bank runs on the HIP device only (there is no CPU path)")
        cap = 2 * self.W + self.H if store_seconds is None else int(round(store_seconds * fs))
        self.cap = max(self.W + 4, -(-cap // 4) * 4)
        self.table = SlotTable(slots, self.W, self.O, self.cap)
        self.lib = L.load()
        W, S, dev = self.W, self.S, self.dev
        self._store = torch.zeros(self.slots, self.cap, dtype=torch.float32, device=dev)
        nbytes = int(self.lib.sepr_streambank_state_bytes(self.slots, S, self.O))
        if nbytes <= 0:
            raise ValueError(f"unsupported bank shape: slots {slots}, {S} speakers, overlap {self.O}")
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._x = torch.zeros(self.slots, W, dtype=torch.float32, device=dev)
        self._live = torch.zeros(self.slots, S, W, dtype=torch.float32, device=dev)
        self.perm = torch.zeros(self.slots, S, dtype=torch.int32, device=dev)       # P and g of the last hop's rows
        self.gain = torch.zeros(self.slots, S, dtype=torch.float32, device=dev)
        # per-hop tables: pinned staging -> device, a ring so that a hop never waits for the one before it
        depth, cols = 3, STEP_COLS + GATHER_COLS
        self._pin = torch.zeros(depth, self.slots * cols, dtype=torch.int64).pin_memory()
        self._tab = torch.zeros(depth, self.slots * cols, dtype=torch.int64, device=dev)
        self._events: List[Optional[torch.cuda.Event]] = [None] * depth
        self._hop_no = 0
        self.keep_windows = bool(keep_windows)
        self.kept: Dict[int, List[torch.Tensor]] = {}
        self.profile = False                                                         # tools/stream_bench.py: time the parts of a hop
        self.hop_events: List[List[torch.cuda.Event]] = []                           # per hop: before gather, forward, step, and after

    # ---- the streams -----------------------------------------------------------------------------------
    def open(self) -> int:
        sid = self.table.open()
        if self.keep_windows:
            self.kept[sid] = []
        return sid

    def free_slots(self) -> int:
        return self.table.free_slots()

    def push(self, sid: int, samples) -> None:
        x = torch.from_numpy(np.ascontiguousarray(samples)) if isinstance(samples, np.ndarray) else torch.as_tensor(samples)
        if x.dim() != 1:
            raise ValueError("push takes a 1-D tensor or array")
        n = int(x.shape[0])
        slot, p0 = self.table.push(sid, n)
        if n == 0:
            return
        x = x.to(device=self.dev, dtype=torch.float32, non_blocking=True)
        first = min(n, self.cap - p0)
        self._store[slot, p0:p0 + first].copy_(x[:first])
        if n > first:
            self._store[slot, :n - first].copy_(x[first:])

    def close(self, sid: int) -> None:
        self.table.close(sid)

    def ready(self) -> int:
        return len(self.table.plan())

    # ---- one hop ---------------------------------------------------------------------------------------
    def step(self) -> Dict[int, torch.Tensor]:
        return self._hop(None, None)

    @torch.no_grad()
    def _hop(self, dest: Optional[torch.Tensor], place: Optional[Dict[int, Tuple[int, int]]]) -> Dict[int, torch.Tensor]:
        """One hop.  ``dest`` / ``place``: emit into the flat tensor ``dest``, stream ``sid`` at ``place[sid] = (offset of its [S, row]
        block, row)`` plus ``kH`` - the offline face; default: into the bank's live buffer."""
        from .infer import separate
        W, O, H, S = self.W, self.O, self.H, self.S
        wins, flushes, shorts, empties = [], [], [], []
        for slot, st, act in self.table.plan():
            {"window": wins, "flush": flushes, "short": shorts, "empty": empties}[act[0]].append((slot, st, act))
        out: Dict[int, torch.Tensor] = {}
        rows = wins + flushes                                   # the windows first: table row a < Aw reads row a of the forward's output
        A, Aw = len(rows), len(wins)
        if A:
            base = self._live if dest is None else dest
            tab = np.zeros((A, STEP_COLS), np.int64)
            gat = np.zeros((max(Aw, 1), GATHER_COLS), np.int64)
            for a, (slot, st, (kind, n_emit, _)) in enumerate(rows):
                off, stride = (a * S * W, W) if dest is None else (place[st.sid][0] + st.k * H, place[st.sid][1])
                tab[a] = (slot, st.k, n_emit, kind == "window", off, stride)
                if kind == "window":
                    gat[a] = (slot * self.cap, st.k * H, st.received)
            ring = self._hop_no % len(self._events)
            self._hop_no += 1
            if self._events[ring] is not None:
                self._events[ring].synchronize()                # the copy that last read this staging row (hops ago) has landed
            pin = self._pin[ring].numpy()
            pin[:A * STEP_COLS] = tab.reshape(-1)
            pin[self.slots * STEP_COLS:self.slots * STEP_COLS + gat.size] = gat.reshape(-1)
            with torch.cuda.device(self.dev):
                stream = torch.cuda.current_stream(self.dev)
                self._tab[ring].copy_(self._pin[ring], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                self._events[ring] = ev
                t_step = self._tab[ring].data_ptr()
                t_gather = t_step + 8 * self.slots * STEP_COLS
                ptrs = (L._fp * S)(*([self._x.data_ptr()] * S))
                ld = W
                marks: List[torch.cuda.Event] = []

                def mark():
                    if self.profile:
                        marks.append(torch.cuda.Event(enable_timing=True))
                        marks[-1].record(stream)

                mark()
                if Aw:
                    L.check(self.lib.sepr_streambank_gather(self._store.data_ptr(), self._store.numel(), self.cap, t_gather, Aw, W,
                                                            self._x.data_ptr(), stream.cuda_stream), "sepr_streambank_gather")
                    mark()
                    aux = self.model.compute_aux
                    self.model.compute_aux = False              # main outputs only, as in separate_long
                    try:
                        audio, _ = self.model(self._x[:Aw])
                    finally:
                        self.model.compute_aux = aux
                    ld = int(audio[0].stride(0)) if Aw > 1 else int(audio[0].shape[-1])
                    if any(a.stride(-1) != 1 or a.shape[-1] < W or (Aw > 1 and a.stride(0) != ld) or a.data_ptr() % 16 for a in audio) \
                            or ld % 4:
                        buf = torch.empty(S, Aw, W, dtype=torch.float32, device=self.dev)      # rows the kernel cannot read in place
                        for s in range(S):
                            buf[s].copy_(audio[s][..., :W])
                        audio, ld = [buf[s] for s in range(S)], W
                    ptrs = (L._fp * S)(*[a.data_ptr() for a in audio])
                    if self.keep_windows:
                        for a, (_, st, _) in enumerate(wins):
                            self.kept[st.sid].append(torch.stack([audio[s][a, :W] for s in range(S)]).clone())
                mark()
                L.check(self.lib.sepr_streambank_step(ptrs, ld, t_step, A, self.slots, S, W, O, int(self.match_gain), base.data_ptr(),
                                                      base.numel(), self.perm.data_ptr(), self.gain.data_ptr(), self._state.data_ptr(),
                                                      self._state.numel(), stream.cuda_stream), "sepr_streambank_step")
                mark()
                if self.profile and Aw:
                    self.hop_events.append(marks)
            for a, (slot, st, act) in enumerate(rows):
                n_emit = act[1]
                if dest is None:
                    out[st.sid] = self._live[a, :, :n_emit]
                else:
                    off, row = place[st.sid]
                    out[st.sid] = dest[off:off + S * row].view(S, row)[:, st.k * H:st.k * H + n_emit]
                self.table.done(slot, act)
        for slot, st, act in shorts:
            T = act[1]
            x = self._store[slot, :T].clone()                   # never wrapped: T <= W <= cap, written from index 0
            out[st.sid] = torch.stack([e[0] for e in separate(self.model, x[None])])
            self.table.done(slot, act)
        for slot, st, act in empties:
            out[st.sid] = torch.empty(S, 0, dtype=torch.float32, device=self.dev)
            self.table.done(slot, act)
        return out

    def drain(self) -> Dict[int, torch.Tensor]:
        """``step()`` until nothing is pending; per stream, everything those steps emitted, concatenated."""
        parts: Dict[int, List[torch.Tensor]] = {}
        while self.ready():
            for sid, y in self.step().items():
                parts.setdefault(sid, []).append(y.clone())
        return {sid: torch.cat(p, dim=1) for sid, p in parts.items()}


@torch.no_grad()
def separate_many(model, recordings: Sequence[torch.Tensor], slots: int = 32, chunk_seconds: float = 4.0, overlap_seconds: float = 1.0,
                  fs: int = 8000, match_gain: bool = False, return_bank: bool = False, keep_windows: bool = False):
    """The offline face of the bank: the recordings queue for ``slots`` slots and are fed one hop of audio per ``step``, so one forward
    carries one window of up to ``slots`` recordings.  Returns what ``separate_long`` returns for a sequence: per recording,
    ``num_spks`` tensors ``[T]`` on the model's device.  Emissions go straight into each recording's ``[S, T]`` result.  Recordings of
    at most ``W`` samples take the ``separate`` path.  ``return_bank=True`` also returns the bank and the stream id of every
    recording (``None`` for the short ones) - with ``keep_windows`` the way to look at the windows that were run."""
    from .infer import separate
    xs, _ = _as_list(list(recordings))
    bank = StreamBank(model, slots=slots, chunk_seconds=chunk_seconds, overlap_seconds=overlap_seconds, fs=fs, match_gain=match_gain,
                      keep_windows=keep_windows)
    W, H, S, dev = bank.W, bank.H, bank.S, bank.dev
    outs: List[Optional[List[torch.Tensor]]] = [None] * len(xs)
    sids: List[Optional[int]] = [None] * len(xs)
    queue = []
    for r, x in enumerate(xs):
        if x.shape[-1] <= W:
            outs[r] = [e[0] for e in separate(model, x[None])]
        else:
            queue.append(r)
    rows = {r: -(-int(xs[r].shape[-1]) // 4) * 4 for r in queue}
    offs, total = {}, 0
    for r in queue:
        offs[r] = total
        total += S * rows[r]
    y = torch.empty(max(total, 4), dtype=torch.float32, device=dev)
    place: Dict[int, Tuple[int, int]] = {}
    active: Dict[int, Tuple[int, torch.Tensor, int]] = {}       # sid -> (recording, its samples on the device, samples fed)
    queue.reverse()
    while queue or active:
        while queue and bank.free_slots():
            r = queue.pop()
            sid = bank.open()
            sids[r] = sid
            place[sid] = (offs[r], rows[r])
            active[sid] = (r, xs[r].to(device=dev, dtype=torch.float32), 0)
        for sid, (r, x, fed) in list(active.items()):
            T = int(x.shape[0])
            if fed < T:
                n = min(W if fed == 0 else H, T - fed)
                bank.push(sid, x[fed:fed + n])
                fed += n
                active[sid] = (r, x, fed)
                if fed == T:
                    bank.close(sid)
        bank._hop(y, place)
        for sid in [s for s in active if s not in bank.table.slot_of]:
            del active[sid]
    for r, sid in enumerate(sids):
        if sid is not None:
            T = int(xs[r].shape[-1])
            block = y[offs[r]:offs[r] + S * rows[r]].view(S, rows[r])
            outs[r] = [block[s, :T] for s in range(S)]
    return (outs, bank, sids) if return_bank else outs
