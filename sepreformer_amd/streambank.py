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
equals ``separate_long(model, x, batch=1)``.

A stream may arrive at its own rate and be emitted at its own rate: ``open(fs_in=, fs_out=)``.  ``push`` then copies
the raw samples into a ring at the input rate, a hop begins with one convert launch that brings the model-rate store of every converting
stream up to date and ends with one convert launch over the emitted tracks (plus the small launch that carries their history), all with
``resample.resample``'s filter and arithmetic (``sepr_streambank_convert``, csrc/sepr_streamrate.hip).  When a sample may be computed is host
integer arithmetic (``ready_count``), so the host knows how many model-rate samples a stream holds without asking the device.  What such a
stream returns equals ``resample(separate_long(model, resample(x, fs_in, fs), batch=1), fs, fs_out)`` bit for bit when its windows ran alone.
Out of scope: changing a stream's rate after ``open``, more than one device, threads (one bank is driven by one thread).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .longform import _as_list, check_geometry
from .resample import MAX_CONVERTERS, _table, converter_args, geometry, out_len, span_fits   # the converter's one definition

STEP_COLS, GATHER_COLS = 6, 3          # include/sepr.h: slot, k, n_emit, has_window, out offset, track stride | base, start, received
CONVERT_COLS = 10                      # conv, n0, n1, T_known, src base, src origin, src cap, dst base, dst origin, dst cap

def ready_count(received: int, closed: bool, L: int, M: int, Hh: int) -> int:
    """How many outputs of a converter ``L / M`` with half length ``Hh`` may be computed from the first ``received`` input samples.  Output
    ``n`` reads inputs up to ``floor(n M / L) + Hh + 1``: while the stream is open it is computed once ``received >= floor(n M / L) + Hh +
    2``; once it is closed its length is known and all ``ceil(received L / M)`` outputs are, with zero extension.  Either way an output
    reads exactly what the whole-recording conversion reads."""
    if closed:
        return out_len(received, L, M)
    c = received - Hh - 2                           # floor(n M / L) <= c  <=>  n M <= (c + 1) L - 1
    return 0 if c < 0 else ((c + 1) * L - 1) // M + 1


def raw_capacity(cap: int, fs: int, max_rate: int) -> int:
    """The input-rate ring of a slot: the model-rate store of ``cap`` samples at the highest rate, plus one span of that converter."""
    _, _, K, _ = geometry(max_rate, fs)
    return -(-(-(-cap * max_rate // fs) + K + 2) // 4) * 4


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


class _Rate:
    """One side of a converting stream: the rates, the converter's geometry and its index among the bank's converters."""
    __slots__ = ("fs_a", "fs_b", "L", "M", "K", "Hh", "conv")

    def __init__(self, fs_a: int, fs_b: int, conv: int):
        self.fs_a, self.fs_b, self.conv = int(fs_a), int(fs_b), conv
        self.L, self.M, self.K, self.Hh = geometry(fs_a, fs_b)


class _Stream:
    """``received``: the samples at the model's rate the stream holds - pushed, or converted (counted when their conversion is planned).
    ``received_in`` / ``closed_in``: what was pushed at the input rate and whether ``close`` was called; ``closed`` follows ``closed_in``
    once the last sample has been converted.  ``n_out``: samples returned at the output rate."""
    __slots__ = ("sid", "received", "k", "closed", "rin", "rout", "received_in", "closed_in", "n_out")

    def __init__(self, sid: int):
        self.sid, self.received, self.k, self.closed = sid, 0, 0, False
        self.rin: Optional[_Rate] = None
        self.rout: Optional[_Rate] = None
        self.received_in, self.closed_in, self.n_out = 0, False, 0


class SlotTable:
    """The bank's host-side bookkeeping, free of any device: which stream holds which slot, what each has received and run, whether a
    push fits the store of ``cap`` samples, and what the next hop does (``next_action``).  For streams at a rate of their own
    (``open(fs_in, fs_out)``, model rate ``fs``, rates up to ``max_rate``): the bank's converters, the input-rate ring of ``raw_cap``
    samples, and which model-rate samples the next convert launch computes (``convert`` / ``take_rows``)."""

    def __init__(self, slots: int, W: int, O: int, cap: int, fs: int = 8000, max_rate: int = 48000):
        if slots < 1:
            raise ValueError("slots must be at least 1")
        if cap < W:
            raise ValueError("the store must hold at least one window")
        self.slots, self.W, self.O, self.H, self.cap = int(slots), W, O, W - O, int(cap)
        self.fs, self.max_rate = int(fs), max(int(max_rate), int(fs))
        self.raw_cap = raw_capacity(self.cap, self.fs, self.max_rate)
        self.streams: List[Optional[_Stream]] = [None] * self.slots
        self.slot_of: Dict[int, int] = {}
        self._next_sid = 0
        self.convs: List[Tuple[int, int]] = []                   # converter k = (fs_a, fs_b); an entry nobody uses stays valid until reused
        self._conv_users: List[int] = []
        self.conv_epoch = 0                                      # bumped whenever `convs` changes
        self._rows: Dict[int, List[int]] = {}                    # slot -> [conv, n0, n1, T_known] the next input-convert launch computes

    # ---- converters ------------------------------------------------------------------------------------
    def _acquire(self, fs_a: int, fs_b: int) -> int:
        key = (int(fs_a), int(fs_b))
        for k, c in enumerate(self.convs):
            if c == key and self._conv_users[k] > 0:
                self._conv_users[k] += 1
                return k
        alive = sum(u > 0 for u in self._conv_users)
        if alive >= MAX_CONVERTERS:
            raise RuntimeError(f"{fs_a} -> {fs_b} Hz would be converter {alive + 1} alive in this bank: one launch takes at most "
                               f"{MAX_CONVERTERS}, both sides together")
        for k, u in enumerate(self._conv_users):
            if u == 0:
                self.convs[k], self._conv_users[k] = key, 1
                break
        else:
            self.convs.append(key)
            self._conv_users.append(1)
            k = len(self.convs) - 1
        self.conv_epoch += 1
        return k

    def _release(self, r: Optional[_Rate]) -> None:
        if r is not None:
            self._conv_users[r.conv] -= 1

    def _check_rate(self, fs_a: int, fs_b: int, out_side: bool) -> None:
        other = fs_b if out_side else fs_a
        if other > self.max_rate:
            raise ValueError(f"{other} Hz is above this bank's max_rate of {self.max_rate} Hz")
        Lr, Mr, K, _ = geometry(fs_a, fs_b)
        if not span_fits(Lr, Mr, K):
            raise RuntimeError(f"{fs_a} -> {fs_b} Hz: the converter's tile span exceeds the kernel's LDS: " + L._ERR[L.SEPR_EINVAL])
        if out_side and K > self.H:
            raise ValueError(f"{fs_a} -> {fs_b} Hz needs the last {K} emitted samples, more than one hop of {self.H}")

    def open(self, fs_in: Optional[int] = None, fs_out: Optional[int] = None) -> int:
        fs_in = None if fs_in is None or int(fs_in) == self.fs else int(fs_in)
        fs_out = None if fs_out is None or int(fs_out) == self.fs else int(fs_out)
        if fs_in is not None:
            self._check_rate(fs_in, self.fs, False)
        if fs_out is not None:
            self._check_rate(self.fs, fs_out, True)
        for slot, st in enumerate(self.streams):
            if st is None:
                st = _Stream(self._next_sid)
                if fs_in is not None:
                    st.rin = _Rate(fs_in, self.fs, self._acquire(fs_in, self.fs))
                if fs_out is not None:
                    try:
                        st.rout = _Rate(self.fs, fs_out, self._acquire(self.fs, fs_out))
                    except RuntimeError:
                        self._release(st.rin)
                        raise
                self._next_sid += 1
                self.streams[slot] = st
                self.slot_of[st.sid] = slot
                return st.sid
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
        if st.closed or st.closed_in:
            raise RuntimeError(f"stream {sid} is closed")
        if st.rin is not None:
            room = self.room(sid)
            if n > room:
                raise OverflowError(f"stream {sid}: {n} more samples overflow the input ring of {self.raw_cap} ({self.raw_cap - room} "
                                    "pending); call step() first or size the bank with store_seconds")
            p0 = st.received_in % self.raw_cap
            st.received_in += n
            return slot, p0
        pending = st.received - st.k * self.H                   # the samples from the next window's start on are still needed
        if pending + n > self.cap:
            raise OverflowError(f"stream {sid}: {n} more samples overflow the store of {self.cap} ({pending} pending); "
                                "call step() first or size the bank with store_seconds")
        p0 = st.received % self.cap
        st.received += n
        return slot, p0

    def room(self, sid: int) -> int:
        """How many more samples a push may bring (at the rate the stream is pushed at)."""
        slot, st = self.lookup(sid)
        if st.rin is None:
            return self.cap - (st.received - st.k * self.H)
        n_next = self._rows[slot][1] if slot in self._rows else st.received       # the first output whose inputs are still to be read
        first = max(0, n_next * st.rin.M // st.rin.L - st.rin.Hh)
        return self.raw_cap - (st.received_in - first)

    def close(self, sid: int) -> None:
        st = self.lookup(sid)[1]
        st.closed_in = True
        if st.rin is None:
            st.closed = True

    def convert(self) -> None:
        """Plan the input conversion of every converting stream: the outputs that have become computable (``ready_count``) and fit the
        model-rate store join the stream's row of the next convert launch, and count as received from now on.  A stream counts as closed
        once its last sample is among them."""
        for slot, st in enumerate(self.streams):
            if st is None or st.rin is None or st.closed:
                continue
            r = st.rin
            total = ready_count(st.received_in, st.closed_in, r.L, r.M, r.Hh)
            n1 = min(total, st.k * self.H + self.cap)
            if n1 > st.received:
                row = self._rows.setdefault(slot, [r.conv, st.received, n1, st.received_in])
                row[2], row[3] = n1, st.received_in
                st.received = n1
            if st.closed_in and st.received == total:
                st.closed = True

    def take_rows(self) -> List[Tuple[int, int, int, int, int]]:
        """(slot, conv, n0, n1, T_known) for the convert launch that now runs, in slot order."""
        rows = [(slot, *self._rows[slot]) for slot in sorted(self._rows)]
        self._rows = {}
        return rows

    def plan(self) -> List[Tuple[int, _Stream, Tuple[str, int, bool]]]:
        """(slot, stream, action) of every stream the next hop serves, in slot order."""
        self.convert()
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
            self._release(st.rin)
            self._release(st.rout)


class StreamBank:
    """``StreamBank(model, slots=32, chunk_seconds=4.0, overlap_seconds=1.0, fs=8000, match_gain=False)``.

    ``open() -> sid``; ``push(sid, samples)`` (1-D tensor or array, host or device, any length, at the model's rate); ``close(sid)``
    marks the end; ``step()`` runs ONE hop and returns ``{sid: [S, n] device tensor}``, the samples that became final, valid until the
    next ``step()``; ``ready()`` is the number of streams a ``step()`` would serve; ``drain()`` steps until nothing is pending.
    A stream has a window ready when it has received ``kH + W`` samples, or when it is closed and a last window or the flush of its
    tail is pending.  A closed stream of at most ``W`` samples that never ran a window is ``infer.separate(model, x)`` itself.  A closed
    stream whose last samples have been returned frees its slot.  The model is put in ``eval()``; the auxiliary heads are switched off
    around the bank's forwards and restored.  A sample waits between ``O`` and ``W`` samples of audio plus one hop's compute before it is
    emitted: chunked-online, not low-latency (the models are non-causal).  One device, one driving thread.

    ``open(fs_in=None, fs_out=None)``: the stream is pushed at ``fs_in`` and returned at ``fs_out`` (``None`` or ``fs``: no conversion on
    that side; rates up to ``max_rate``).  Conversion runs on the device inside the hop, for all streams in one launch per side
    (DESIGN.md section 5c-3); a window is then ready once ``kH + W`` model-rate samples have been converted, a sample of the output rate
    is returned once the emitted model-rate samples it reads exist, and a short stream is ``resample`` around ``separate``.  A bank in
    which no stream converts launches nothing more than before.  At most 16 distinct converters are alive in a bank, both sides
    together; an output converter must not need more history than one hop.

    ``store_seconds``: pending-sample store per slot (default ``2 W + H`` samples; at least ``W`` plus the largest push); the ring a
    converting stream is pushed into holds that much audio at ``max_rate`` plus one converter span.
    ``keep_windows=True`` (debugging) keeps every window output the bank ran, per stream, in ``kept[sid]`` as ``[S, W]`` tensors."""

    def __init__(self, model, slots: int = 32, chunk_seconds: float = 4.0, overlap_seconds: float = 1.0, fs: int = 8000,
                 match_gain: bool = False, store_seconds: Optional[float] = None, keep_windows: bool = False, max_rate: int = 48000):
        cfg = model.cfg
        self.W, self.O = int(round(chunk_seconds * fs)), int(round(overlap_seconds * fs))
        check_geometry(self.W, self.O, cfg.enc_stride, cfg.enc_kernel)
        self.H, self.S, self.slots = self.W - self.O, int(model.num_spks), int(slots)
        self.model, self.match_gain, self.fs = model.eval(), bool(match_gain), int(fs)
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("the stream bank runs on the HIP device only (there is no CPU path)")
        cap = 2 * self.W + self.H if store_seconds is None else int(round(store_seconds * fs))
        self.cap = max(self.W + 4, -(-cap // 4) * 4)
        self.table = SlotTable(slots, self.W, self.O, self.cap, fs=fs, max_rate=max_rate)
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
        # per-hop tables: pinned staging -> device, a ring so that a hop never waits for the one before it.  One row of the ring holds
        # the step table, the gather table and the two convert tables (input side: a row per stream, output side: a row per track)
        depth = 3
        self._t_gather = self.slots * STEP_COLS
        self._t_cin = self._t_gather + self.slots * GATHER_COLS
        self._t_cout = self._t_cin + self.slots * CONVERT_COLS
        width = self._t_cout + self.slots * S * CONVERT_COLS
        self._pin = torch.zeros(depth, width, dtype=torch.int64).pin_memory()
        self._tab = torch.zeros(depth, width, dtype=torch.int64, device=dev)
        self._events: List[Optional[torch.cuda.Event]] = [None] * depth
        self._hop_no = 0
        self.keep_windows = bool(keep_windows)
        self.kept: Dict[int, List[torch.Tensor]] = {}
        self.profile = False                                                         # tools/stream_bench.py: time the parts of a hop
        # per hop with a forward: before the input conversion, the gather, the forward, the step, the output conversion, and after
        self.hop_events: List[List[torch.cuda.Event]] = []
        # conversion (allocated by the first stream that converts): the input-rate rings; the emitted tracks of the streams that convert
        # on the way out, rows [slot][S][H + W] = the last H samples emitted before the hop, then the hop's emission; the output-rate
        # samples of a hop, rows [output row][S][ocap]
        self._raw: Optional[torch.Tensor] = None
        self._hist: Optional[torch.Tensor] = None
        self._hist_off = 0
        self._olive: Optional[torch.Tensor] = None
        self._ocap = -(-(-(-(W + self.H) * self.table.max_rate // self.fs) + 8) // 4) * 4
        self._conv_epoch = -1
        self._conv_args = None

    # ---- the streams -----------------------------------------------------------------------------------
    def open(self, fs_in: Optional[int] = None, fs_out: Optional[int] = None) -> int:
        sid = self.table.open(fs_in, fs_out)
        st = self.table.lookup(sid)[1]
        W, H, S = self.W, self.H, self.S
        if st.rin is not None and self._raw is None:
            self._raw = torch.zeros(self.slots, self.table.raw_cap, dtype=torch.float32, device=self.dev)
        if st.rout is not None and self._hist is None:
            # the step kernel emits through ONE base pointer: the live buffer and the history rows share an allocation
            both = torch.zeros(self.slots * S * W + self.slots * S * (H + W), dtype=torch.float32, device=self.dev)
            self._hist_off = self.slots * S * W
            self._live = both[:self._hist_off].view(self.slots, S, W)
            self._hist = both
            self._olive = torch.zeros(self.slots * S, self._ocap, dtype=torch.float32, device=self.dev)
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
        ring, cap = (self._store, self.cap) if self.table.streams[slot].rin is None else (self._raw, self.table.raw_cap)
        first = min(n, cap - p0)
        ring[slot, p0:p0 + first].copy_(x[:first])
        if n > first:
            ring[slot, :n - first].copy_(x[first:])

    def close(self, sid: int) -> None:
        self.table.close(sid)

    def ready(self) -> int:
        return len(self.table.plan())

    # ---- one hop ---------------------------------------------------------------------------------------
    def step(self) -> Dict[int, torch.Tensor]:
        return self._hop(None, None)

    def _converters(self):
        """The host arrays ``sepr_streambank_convert`` takes, rebuilt when the bank's converters changed."""
        if self._conv_epoch != self.table.conv_epoch:
            self._conv_args = converter_args([_table(a, b, self.dev) for a, b in self.table.convs])
            self._conv_epoch = self.table.conv_epoch
        return self._conv_args

    @torch.no_grad()
    def _hop(self, dest: Optional[torch.Tensor], place: Optional[Dict[int, Tuple[int, int]]]) -> Dict[int, torch.Tensor]:
        """One hop.  ``dest`` / ``place``: emit into the flat tensor ``dest``, stream ``sid`` at ``place[sid] = (offset of its [S, row]
        block, row)`` plus ``kH`` - the offline face; default: into the bank's live buffer."""
        from .infer import separate
        from .resample import resample
        W, O, H, S = self.W, self.O, self.H, self.S
        wins, flushes, shorts, empties = [], [], [], []
        for slot, st, act in self.table.plan():
            {"window": wins, "flush": flushes, "short": shorts, "empty": empties}[act[0]].append((slot, st, act))
        cin = self.table.take_rows()                            # the model-rate samples `plan` counted as received: computed first
        out: Dict[int, torch.Tensor] = {}
        rows = wins + flushes                                   # the windows first: table row a < Aw reads row a of the forward's output
        A, Aw = len(rows), len(wins)
        if A or cin:
            converting = dest is None and any(st.rout is not None for _, st, _ in rows)
            base = (self._hist if self._hist is not None else self._live) if dest is None else dest
            tab = np.zeros((max(A, 1), STEP_COLS), np.int64)
            gat = np.zeros((max(Aw, 1), GATHER_COLS), np.int64)
            ctab = np.zeros((max(len(cin), 1), CONVERT_COLS), np.int64)
            otab = np.zeros((max(A, 1) * S, CONVERT_COLS), np.int64)
            orow: Dict[int, Tuple[int, int]] = {}               # table row a -> (its output row, samples at the output rate)
            for a, (slot, st, (kind, n_emit, fin)) in enumerate(rows):
                if dest is not None:
                    off, stride = place[st.sid][0] + st.k * H, place[st.sid][1]
                elif st.rout is not None:
                    off, stride = self._hist_off + slot * S * (H + W) + H, H + W
                    r, E, q = st.rout, st.k * H + n_emit, len(orow)
                    n1 = ready_count(E, fin, r.L, r.M, r.Hh)
                    if n1 - st.n_out > self._ocap:
                        raise RuntimeError(f"stream {st.sid}: {n1 - st.n_out} samples at the output rate in one hop")
                    for s in range(S):
                        otab[q * S + s] = (r.conv, st.n_out, n1, E, off - H + s * stride, st.k * H - H, H + W,
                                           (q * S + s) * self._ocap, st.n_out, self._ocap)
                    orow[a] = (q, n1 - st.n_out)
                    st.n_out = n1
                else:
                    off, stride = a * S * W, W
                tab[a] = (slot, st.k, n_emit, kind == "window", off, stride)
                if kind == "window":
                    gat[a] = (slot * self.cap, st.k * H, st.received)
            for i, (slot, conv, n0, n1, T) in enumerate(cin):
                ctab[i] = (conv, n0, n1, T, slot * self.table.raw_cap, 0, self.table.raw_cap, slot * self.cap, 0, self.cap)
            ring = self._hop_no % len(self._events)
            self._hop_no += 1
            if self._events[ring] is not None:
                self._events[ring].synchronize()                # the copy that last read this staging row (hops ago) has landed
            pin = self._pin[ring].numpy()
            pin[:A * STEP_COLS] = tab[:A].reshape(-1)
            pin[self._t_gather:self._t_gather + gat.size] = gat.reshape(-1)
            if cin:
                pin[self._t_cin:self._t_cin + ctab.size] = ctab.reshape(-1)
            if orow:
                pin[self._t_cout:self._t_cout + len(orow) * S * CONVERT_COLS] = otab[:len(orow) * S].reshape(-1)
            with torch.cuda.device(self.dev):
                stream = torch.cuda.current_stream(self.dev)
                self._tab[ring].copy_(self._pin[ring], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                self._events[ring] = ev
                t_step = self._tab[ring].data_ptr()
                t_gather = t_step + 8 * self._t_gather
                ptrs = (L._fp * S)(*([self._x.data_ptr()] * S))
                ld = W
                marks: List[torch.cuda.Event] = []

                def mark():
                    if self.profile:
                        marks.append(torch.cuda.Event(enable_timing=True))
                        marks[-1].record(stream)

                mark()
                if cin:
                    L.check(self.lib.sepr_streambank_convert(self._raw.data_ptr(), self._raw.numel(), self._store.data_ptr(),
                                                             self._store.numel(), t_step + 8 * self._t_cin, len(cin),
                                                             max(r[3] - r[2] for r in cin), *self._converters(), stream.cuda_stream),
                            "sepr_streambank_convert")
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
                if A:
                    L.check(self.lib.sepr_streambank_step(ptrs, ld, t_step, A, self.slots, S, W, O, int(self.match_gain), base.data_ptr(),
                                                          base.numel(), self.perm.data_ptr(), self.gain.data_ptr(),
                                                          self._state.data_ptr(), self._state.numel(), stream.cuda_stream),
                            "sepr_streambank_step")
                mark()
                if converting:
                    nmax = max(n for _, n in orow.values())
                    if nmax > 0:
                        L.check(self.lib.sepr_streambank_convert(self._hist.data_ptr(), self._hist.numel(), self._olive.data_ptr(),
                                                                 self._olive.numel(), t_step + 8 * self._t_cout, len(orow) * S, nmax,
                                                                 *self._converters(), stream.cuda_stream), "sepr_streambank_convert")
                    # the history of the next hop, once the conversion has read this one's (every row of the hop: a row that finishes
                    # its stream or does not convert carries samples nobody reads)
                    L.check(self.lib.sepr_streambank_carry(self._hist.data_ptr() + 4 * self._hist_off, self._hist.numel() - self._hist_off,
                                                           t_step, A, self.slots, S, H, H + W, stream.cuda_stream),
                            "sepr_streambank_carry")
                mark()
                if self.profile and Aw:
                    self.hop_events.append(marks)
            for a, (slot, st, act) in enumerate(rows):
                n_emit = act[1]
                if dest is not None:
                    off, row = place[st.sid]
                    out[st.sid] = dest[off:off + S * row].view(S, row)[:, st.k * H:st.k * H + n_emit]
                elif a in orow:
                    q, n = orow[a]
                    out[st.sid] = self._olive[q * S:(q + 1) * S, :n]
                else:
                    out[st.sid] = self._live[a, :, :n_emit]
                self.table.done(slot, act)
        for slot, st, act in shorts:
            if st.rin is None:
                x = self._store[slot, :act[1]].clone()          # never wrapped: T <= W <= cap, written from index 0
            else:                                               # nor has the input ring: it holds more than W samples' worth
                x = resample(self._raw[slot, :st.received_in].clone(), st.rin.fs_a, self.fs)
            y = [e[0] for e in separate(self.model, x[None])]
            if st.rout is not None:
                y = resample([e.contiguous() for e in y], self.fs, st.rout.fs_b)
            out[st.sid] = torch.stack(y)
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
                  fs: int = 8000, match_gain: bool = False, return_bank: bool = False, keep_windows: bool = False,
                  rates: Optional[Sequence[int]] = None):
    """The offline face of the bank: the recordings queue for ``slots`` slots and are fed one hop of audio per ``step``, so one forward
    carries one window of up to ``slots`` recordings.  Returns what ``separate_long`` returns for a sequence: per recording,
    ``num_spks`` tensors ``[T]`` on the model's device.  Emissions go straight into each recording's ``[S, T]`` result.  Recordings of
    at most ``W`` samples take the ``separate`` path.  ``return_bank=True`` also returns the bank and the stream id of every
    recording (``None`` for the short ones) - with ``keep_windows`` the way to look at the windows that were run.
    ``rates``: recording ``r`` holds samples at ``rates[r]`` Hz; it is pushed as it is and converted to ``fs`` inside the bank, one hop of
    audio at a time.  The results stay at ``fs``: ``T = ceil(T_in fs / rate)`` samples, equal to those of the
    recordings converted with ``resample`` beforehand."""
    from .infer import separate
    from .resample import resample
    xs, _ = _as_list(list(recordings))
    rates = [int(fs)] * len(xs) if rates is None else [int(v) for v in rates]
    if len(rates) != len(xs):
        raise ValueError(f"{len(rates)} rates for {len(xs)} recordings")
    bank = StreamBank(model, slots=slots, chunk_seconds=chunk_seconds, overlap_seconds=overlap_seconds, fs=fs, match_gain=match_gain,
                      keep_windows=keep_windows, max_rate=max(rates + [48000]))
    W, H, S, dev = bank.W, bank.H, bank.S, bank.dev
    geo = [geometry(v, fs) for v in rates]                      # (L, M, K, Hh); L = M = 1 at the model's rate
    Ts = [int(x.shape[-1]) if v == fs else out_len(int(x.shape[-1]), g[0], g[1]) for x, v, g in zip(xs, rates, geo)]
    outs: List[Optional[List[torch.Tensor]]] = [None] * len(xs)
    sids: List[Optional[int]] = [None] * len(xs)
    queue = []
    for r, x in enumerate(xs):
        if Ts[r] <= W:
            outs[r] = [e[0] for e in separate(model, resample(x, rates[r], fs, device=dev)[None])]
        else:
            queue.append(r)
    rows = {r: -(-Ts[r] // 4) * 4 for r in queue}
    offs, total = {}, 0
    for r in queue:
        offs[r] = total
        total += S * rows[r]
    y = torch.empty(max(total, 4), dtype=torch.float32, device=dev)
    place: Dict[int, Tuple[int, int]] = {}
    active: Dict[int, Tuple[int, torch.Tensor, int, int]] = {}  # sid -> (recording, its samples on the device, samples fed, hops fed)
    queue.reverse()
    while queue or active:
        while queue and bank.free_slots():
            r = queue.pop()
            sid = bank.open(fs_in=rates[r])
            sids[r] = sid
            place[sid] = (offs[r], rows[r])
            active[sid] = (r, xs[r].to(device=dev, dtype=torch.float32), 0, 0)
        for sid, (r, x, fed, hop) in list(active.items()):
            T = int(x.shape[0])
            if fed < T:
                if rates[r] == fs:
                    n = min(W if fed == 0 else H, T - fed)
                else:                                           # what makes W + hop H samples at the model's rate computable
                    Lr, Mr, _, Hh = geo[r]
                    n = min((W + hop * H - 1) * Mr // Lr + Hh + 2, T) - fed
                    n = max(0, min(n, bank.table.room(sid)))
                bank.push(sid, x[fed:fed + n])
                fed += n
                active[sid] = (r, x, fed, hop + 1)
                if fed == T:
                    bank.close(sid)
        bank._hop(y, place)
        for sid in [s for s in active if s not in bank.table.slot_of]:
            del active[sid]
    for r, sid in enumerate(sids):
        if sid is not None:
            block = y[offs[r]:offs[r] + S * rows[r]].view(S, rows[r])
            outs[r] = [block[s, :Ts[r]] for s in range(S)]
    return (outs, bank, sids) if return_bank else outs
