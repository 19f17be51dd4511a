"""The stream bank without a device: the scheduler (streambank.next_action / SlotTable) against the restatement in tests/stream_ref.py
and the geometry of tests/longform_ref.py, slot reuse, the overflow error, and the argument checks of the new C entries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as ref                                                   # noqa: E402
import stream_ref as sref                                                    # noqa: E402

from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import streambank as sb                                 # noqa: E402

GEOMETRIES = [(64, 32), (64, 16), (48, 4)]


def _lengths(W, O):
    H = W - O
    return [1, W - 1, W, W + 1, W + H - 1, W + H, W + H + 1, W + 5 * H + 3]


def _drive(pushes, W, O, step_after_push=True, cap=None):
    """One stream through a SlotTable: -> the (kind, k, start, n) of every hop that served it."""
    H = W - O
    t = sb.SlotTable(1, W, O, cap if cap is not None else 2 * W + sum(pushes))
    sid = t.open()
    ev = []

    def hops():
        while True:
            plan = t.plan()
            if not plan:
                return
            (slot, st, act), = plan
            ev.append((act[0], st.k, st.k * H if act[0] != "short" else 0, act[1]))
            t.done(slot, act)
            if act[2]:
                return

    for n in pushes:
        t.push(sid, n)
        if step_after_push:
            hops()
    t.close(sid)
    hops()
    assert t.free_slots() == 1 and not t.plan()
    return ev


def _splits(T, seed):
    rng = np.random.default_rng(seed)
    yield [T]
    yield [1] * T
    for _ in range(6):
        cuts = np.sort(rng.integers(0, T + 1, size=int(rng.integers(1, 9))))
        yield [int(v) for v in np.diff(np.concatenate([[0], cuts, [T]]))]          # zero-length pushes included


@pytest.mark.parametrize("W,O", GEOMETRIES)
def test_schedule_matches_offline_geometry(W, O):
    H = W - O
    lengths = _lengths(W, O)
    counts = []
    for T in lengths:
        ev = _drive([T], W, O, step_after_push=False)            # the whole recording, then the close: the offline windows
        assert ev == sref.schedule([T], W, O, step_after_push=False)
        nc = ref.num_chunks(T, W, O)
        if T <= W:
            assert ev == [("short", 0, 0, T)]
            counts.append(1)
            continue
        wins = [e for e in ev if e[0] == "window"]
        assert len(wins) == nc == len(ev)                        # no flush: the last window knows it is the last
        assert [e[2] for e in wins] == [k * H for k in range(nc)]
        assert all(e[3] == H for e in wins[:-1]) and wins[-1][3] == T - (nc - 1) * H and O < wins[-1][3] <= W
        counts.append(len(wins))
    assert list(np.concatenate([[0], np.cumsum(counts)])) == list(ref.chunk_offsets(lengths, W, O))


@pytest.mark.parametrize("W,O", GEOMETRIES)
def test_spans_tile_the_recording_for_any_split(W, O):
    H = W - O
    for T in _lengths(W, O):
        for pushes in _splits(T, seed=T):
            assert sum(pushes) == T
            for eager in (True, False):
                ev = _drive(pushes, W, O, step_after_push=eager)
                assert ev == sref.schedule(pushes, W, O, step_after_push=eager), (T, pushes, eager)
                pos = 0
                for kind, k, start, n in ev:                     # exactly once and in order
                    assert start == pos and n > 0
                    pos += n
                assert pos == T
                nwin = sum(e[0] == "window" for e in ev)
                if ev[0][0] != "short":
                    assert nwin == (ref.num_chunks(T, W, O) if T > W else 1)
                    assert [e[0] for e in ev].count("flush") == (1 if eager and (T - W) % H == 0 else 0)


def test_flush_only_when_the_end_falls_on_a_full_window():
    W, O = 64, 16
    H = W - O
    assert sb.next_action(W + H, 2, True, W, O) == ("flush", O, True)
    assert sb.next_action(W + H, 1, True, W, O) == ("window", W, True)        # n_emit = W: the last window, exactly full
    assert sb.next_action(W + H + 1, 1, True, W, O) == ("window", H, False)
    assert sb.next_action(W + H + 1, 2, True, W, O) == ("window", O + 1, True)
    assert sb.next_action(W - 1, 0, False, W, O) is None and sb.next_action(W, 0, False, W, O) == ("window", H, False)
    assert sb.next_action(W, 0, True, W, O) == ("short", W, True) and sb.next_action(0, 0, True, W, O) == ("empty", 0, True)


def test_slot_reuse_and_errors():
    W, O = 64, 16
    t = sb.SlotTable(2, W, O, cap=W + 40)
    a, b = t.open(), t.open()
    assert (a, b) == (0, 1) and t.free_slots() == 0
    with pytest.raises(RuntimeError, match="no free slot"):
        t.open()
    t.push(a, 10)
    t.close(a)
    (slot, st, act), = t.plan()
    assert slot == 0 and act == ("short", 10, True)
    t.done(slot, act)
    assert t.free_slots() == 1
    c = t.open()                                                 # the freed slot, a fresh stream: k = 0, nothing received
    assert c == 2 and t.lookup(c)[0] == 0 and (t.lookup(c)[1].k, t.lookup(c)[1].received) == (0, 0)
    with pytest.raises(KeyError):
        t.push(a, 1)
    t.close(b)
    with pytest.raises(RuntimeError, match="closed"):
        t.push(b, 1)


def test_overflow_error():
    W, O = 64, 16
    H = W - O
    t = sb.SlotTable(1, W, O, cap=W + 40)
    s = t.open()
    assert t.push(s, W + 40) == (0, 0)                           # exactly full
    with pytest.raises(OverflowError):
        t.push(s, 1)
    assert t.lookup(s)[1].received == W + 40                     # a refused push leaves the stream as it was
    (slot, st, act), = t.plan()
    t.done(slot, act)                                            # window 0 has run: its first H samples are no longer needed
    assert t.push(s, H) == (0, 0)                                # and the ring wraps to index (W + 40) mod cap = 0
    with pytest.raises(OverflowError):
        t.push(s, 1)
    t.push(s, 0)
    with pytest.raises(ValueError):
        sb.SlotTable(0, W, O, 100)
    with pytest.raises(ValueError):
        sb.SlotTable(1, W, O, W - 4)


# ---- C ABI: every argument check comes before any HIP call ------------------------------------------------------------
def _step(S=2, A=1, slots=4, W=64, O=16, ld=64, win=(4096, 4096, 4096), table=4096, out=4096, out_elems=1 << 20, perm=4096, gain=4096,
          state=4096, state_bytes=None, no_win=False):
    lib = L.load()
    if state_bytes is None:
        state_bytes = max(int(lib.sepr_streambank_state_bytes(slots, S, O)), 0) if 2 <= S <= 3 else 1 << 20
    ptrs = None if no_win else (L._fp * 3)(*win)
    return lib.sepr_streambank_step(ptrs, ld, table, A, slots, S, W, O, 1, out, out_elems, perm, gain, state, state_bytes, None)


def test_abi_state_bytes():
    lib = L.load()
    up = lambda n: -(-n // 256) * 256                                          # noqa: E731
    for S in (2, 3):
        for slots, O in ((1, 4), (32, 8000), (64, 32)):
            assert lib.sepr_streambank_state_bytes(slots, S, O) == up(slots * S * O * 4) + up(slots * S * 4) + up(slots * S * 8)
    for bad in ((0, 2, 16), (4, 1, 16), (4, 4, 16), (4, 2, 0), (4, 2, 18), (-1, 2, 16)):
        assert lib.sepr_streambank_state_bytes(*bad) == 0, bad
    assert L.SIGNATURES["sepr_streambank_state_bytes"][0] is L._ll


def test_abi_step_argument_checks():
    E = L.SEPR_EINVAL
    assert _step(no_win=True) == E
    for name in ("table", "out", "perm", "gain"):
        assert _step(**{name: None}) == E, name
    assert _step(win=(4096, None, 4096)) == E                               # a null source pointer
    assert _step(S=3, win=(4096, 4096, None)) == E
    assert _step(S=1) == E and _step(S=4) == E
    assert _step(A=0) == E and _step(A=-3) == E
    assert _step(slots=0) == E
    assert _step(W=66, ld=68) == E and _step(O=18) == E                     # W % 4, O % 4
    assert _step(O=0) == E and _step(O=36) == E                             # O = 0, 2 O > W
    assert _step(ld=60) == E and _step(ld=66) == E                          # rows shorter than a window, rows not a multiple of 4
    assert _step(win=(4100, 4096, 4096)) == E and _step(out=4104) == E and _step(state=4100) == E      # not 16-byte aligned
    assert _step(table=4100) == E
    assert _step(out_elems=0) == E
    assert _step(state_bytes=100) == L.SEPR_EWORKSPACE
    assert _step(state=None) == L.SEPR_EWORKSPACE
    full = int(L.load().sepr_streambank_state_bytes(4, 2, 16))
    assert _step(state_bytes=full - 1) == L.SEPR_EWORKSPACE


def test_abi_gather_argument_checks():
    lib, E = L.load(), L.SEPR_EINVAL

    def g(store=4096, elems=1 << 20, cap=256, table=4096, A=1, W=64, x=4096):
        return lib.sepr_streambank_gather(store, elems, cap, table, A, W, x, None)

    for name in ("store", "table", "x"):
        assert g(**{name: None}) == E, name
    assert g(A=0) == E and g(W=0) == E and g(W=66) == E
    assert g(cap=60) == E and g(cap=258) == E and g(elems=100) == E         # cap < W, cap % 4, a store shorter than one ring
    assert g(store=4100) == E and g(x=4104) == E and g(table=4100) == E


def test_binding_declares_the_entries():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sepr.h")).read()
    declared = set(re.findall(r"\b(sepr_[a-z0-9_]+)\s*\(", hdr))
    names = {"sepr_streambank_state_bytes", "sepr_streambank_step", "sepr_streambank_gather"}
    assert names <= declared and names <= set(L.SIGNATURES)
    assert "DESIGN.md section 5c-2" in hdr
    lib = L.load()
    assert all(hasattr(lib, n) for n in names)
    assert sb.STEP_COLS == 6 and sb.GATHER_COLS == 3
    assert C.sizeof(L._ll) == 8
