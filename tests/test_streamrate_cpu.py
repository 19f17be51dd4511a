"""Sample-rate conversion inside the stream bank without a device: when a sample may be computed
(streambank.ready_count against a loop over n), the hop-by-hop conversion against the whole-recording one (tests/stream_rate_ref.py on
tests/resample_ref.py), the bank's host bookkeeping, and the C entry's declaration and argument checks."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as rr                                                    # noqa: E402
import stream_rate_ref as srr                                                # noqa: E402

from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402
from sepreformer_amd import streambank as sb                                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- readiness arithmetic ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_in,fs_out", srr.PLANS)
def test_geometry_is_the_plans(fs_in, fs_out):
    Lr, Mr, K, Hh, _ = rr.geometry(fs_in, fs_out)
    assert sb.geometry(fs_in, fs_out) == (Lr, Mr, K, Hh)
    p = rs.plan(fs_in, fs_out)
    assert (p.L, p.M, p.K, p.Hh) == (Lr, Mr, K, Hh)


@pytest.mark.parametrize("fs_in,fs_out", srr.PLANS)
def test_ready_count_against_a_loop(fs_in, fs_out):
    Lr, Mr, K, Hh, _ = rr.geometry(fs_in, fs_out)
    for received in range(0, 2 * srr.span(fs_in, fs_out) + 1):
        for closed in (False, True):
            got = sb.ready_count(received, closed, Lr, Mr, Hh)
            assert got == srr.ready_brute(received, closed, fs_in, fs_out), (received, closed)
        # what is computed while the stream is open is a prefix of what its end will give, whenever that comes
        assert sb.ready_count(received, False, Lr, Mr, Hh) <= sb.ready_count(received, True, Lr, Mr, Hh)
    assert sb.out_len(12345, Lr, Mr) == rr.out_len(12345, Lr, Mr)


def test_an_output_reads_nothing_beyond_what_was_received():
    for fs_in, fs_out in srr.PLANS:
        Lr, Mr, K, Hh, _ = rr.geometry(fs_in, fs_out)
        for received in (0, 1, Hh + 1, Hh + 2, Hh + 3, 5 * K + 7):
            n = sb.ready_count(received, False, Lr, Mr, Hh)
            if n:
                assert (n - 1) * Mr // Lr + Hh + 1 <= received - 1           # the last input the last ready output reads
            assert n * Mr // Lr + Hh + 1 > received - 1                      # and the next output is not ready


# ---- the chunked restatement equals the whole-recording conversion ------------------------------------------------------
@pytest.mark.parametrize("fs_in,fs_out", srr.PLANS)
def test_chunked_conversion_is_the_whole_recording(fs_in, fs_out):
    rng = np.random.default_rng(fs_in + fs_out)
    for case in range(3):
        T = int(rng.integers(3000, 6001))
        x = rng.standard_normal(T).astype(np.float32)
        want = rr.resample(x, fs_in, fs_out)
        c = srr.Chunked(fs_in, fs_out)
        parts, pos = [], 0
        for n in srr.schedule(T, seed=1000 * case + T, small=case < 2):
            parts.append(c.push(x[pos:pos + n]))
            pos += n
        parts.append(c.close())
        got = np.concatenate(parts)
        assert got.shape == want.shape and np.array_equal(got, want)
        at = 0
        for n0, n1 in c.spans:                                               # every output once, in order
            assert n0 == at and n1 >= n0
            at = n1
        assert at == want.shape[0] == rr.out_len(T, *rr.ratio(fs_in, fs_out))


def test_chunked_restatement_notices_an_early_sample():
    """The restatement has teeth: a sample computed a push too early differs from the whole-recording one.  (At phase 0 the last two
    taps of a row are zero - |u| = Z lies outside the window - so the first output past the rule still has the right value as long as the
    samples are finite; the rule is the issue's, by what the chain reads.  The one after it reads missing samples under non-zero taps.)"""
    fs_in, fs_out = 16000, 8000
    Lr, Mr, K, Hh, _ = rr.geometry(fs_in, fs_out)
    x = np.random.default_rng(3).standard_normal(4000).astype(np.float32)
    want = rr.resample(x, fs_in, fs_out)
    received = 1000
    n = sb.ready_count(received, False, Lr, Mr, Hh)
    early = rr.resample(x[:received], fs_in, fs_out, positions=[n + 1])[0]   # reads inputs that have not arrived
    assert early != want[n + 1]
    assert rr.resample(x[:received], fs_in, fs_out, positions=[n - 1])[0] == want[n - 1]


# ---- the SlotTable with converting streams -------------------------------------------------------------------------------
def _model_table(slots=1, W=4000, O=1000, cap=None, max_rate=48000):
    return sb.SlotTable(slots, W, O, cap if cap is not None else 2 * W + (W - O), fs=8000, max_rate=max_rate)


def test_converted_count_drives_the_schedule():
    W, O = 4000, 1000
    H = W - O
    t = _model_table()
    sid = t.open(fs_in=48000)
    Lr, Mr, K, Hh = sb.geometry(48000, 8000)
    slot, st = t.lookup(sid)
    assert t.push(sid, 6 * W) == (0, 0)                         # W model-rate samples' worth: the last Hh + 1 of them are not computable yet
    assert t.plan() == [] and st.received == sb.ready_count(6 * W, False, Lr, Mr, Hh) < W
    assert t.take_rows() == [(0, st.rin.conv, 0, st.received, 6 * W)]
    n_before = st.received
    t.push(sid, Hh + 2)
    (slot, st, act), = t.plan()
    assert act == ("window", H, False) and st.received >= W
    assert t.take_rows() == [(0, st.rin.conv, n_before, st.received, 6 * W + Hh + 2)]
    assert t.take_rows() == []                                  # a row is taken once
    t.done(slot, act)
    assert st.k == 1


def test_rows_merge_until_they_are_taken():
    t = _model_table()
    sid = t.open(fs_in=16000)
    t.push(sid, 1000)
    t.plan()
    a = t.lookup(sid)[1].received
    t.push(sid, 1000)
    t.plan()
    b = t.lookup(sid)[1].received
    assert 0 < a < b
    assert t.take_rows() == [(0, 0, 0, b, 2000)]                # one row: nothing computed twice, nothing skipped


def test_closed_only_after_the_last_conversion():
    W, O = 4000, 1000
    H = W - O
    t = _model_table(cap=W + 4)                                 # a store that holds hardly more than a window
    sid = t.open(fs_in=16000)
    slot, st = t.lookup(sid)
    T_in = 2 * (W + 2 * H) + 1
    t.push(sid, T_in)
    t.close(sid)
    assert st.closed_in and not st.closed
    with pytest.raises(RuntimeError, match="closed"):
        t.push(sid, 1)
    N = sb.out_len(T_in, 1, 2)
    seen, k = [], 0
    while True:
        plan = t.plan()
        for row in t.take_rows():
            seen.append(row[2:4])
        assert st.received <= st.k * H + t.cap                   # never more than the store holds
        assert st.closed == (st.received == N)
        if not plan:
            break
        (slot, st_, act), = plan
        assert act[0] == "window" and act[2] == (st.closed and N - st.k * H <= W)
        t.done(slot, act)
        if act[2]:
            break
    assert [a for a, _ in seen] == [0] + [b for _, b in seen[:-1]] and seen[-1][1] == N
    assert t.free_slots() == 1


def test_closed_without_a_sample_and_short():
    t = _model_table(slots=2)
    a, b = t.open(fs_in=44100), t.open(fs_in=48000, fs_out=16000)
    t.close(a)
    t.push(b, 600)
    t.close(b)
    acts = {st.sid: act for _, st, act in t.plan()}
    assert acts[a] == ("empty", 0, True) and acts[b] == ("short", 100, True)


def test_input_ring_overflow():
    t = _model_table()
    assert t.raw_cap >= t.cap * 6 + sb.geometry(48000, 8000)[2] and t.raw_cap % 4 == 0
    sid = t.open(fs_in=48000)
    st = t.lookup(sid)[1]
    assert t.room(sid) == t.raw_cap
    t.push(sid, t.raw_cap)
    with pytest.raises(OverflowError, match="input ring"):
        t.push(sid, 1)
    assert st.received_in == t.raw_cap                           # a refused push leaves the stream as it was
    (slot, st, act), = t.plan()
    before = t.room(sid)
    assert before == 0                                           # planned, not yet launched: the samples are still to be read
    rows = t.take_rows()
    Lr, Mr, K, Hh = sb.geometry(48000, 8000)
    assert t.room(sid) == max(0, rows[0][3] * Mr // Lr - Hh)     # everything before the next output's first input may go
    p0 = t.push(sid, 8)[1]
    assert p0 == 0                                               # the ring wraps
    t2 = _model_table()
    s2 = t2.open()                                               # a stream at the model's rate overflows as before
    t2.push(s2, t2.cap)
    with pytest.raises(OverflowError, match="store"):
        t2.push(s2, 1)


def test_open_refusals():
    t = _model_table(slots=2)
    with pytest.raises(ValueError, match="max_rate"):
        t.open(fs_in=96000)
    with pytest.raises(ValueError, match="max_rate"):
        t.open(fs_out=48001)
    t96 = _model_table(max_rate=192000)
    with pytest.raises(RuntimeError, match="SEPR_EINVAL"):
        t96.open(fs_in=192000)                                   # beyond the span limit, as resample says it
    small = sb.SlotTable(1, 64, 16, 200)
    with pytest.raises(ValueError, match="more than one hop"):
        small.open(fs_out=16000)                                 # K' = 130 > H = 48
    assert small.free_slots() == 1 and small.convs == []
    sid = t.open(fs_in=8000, fs_out=None)                        # the model's rate: no converter
    assert t.lookup(sid)[1].rin is None and t.lookup(sid)[1].rout is None and t.convs == []


def test_seventeenth_converter_is_refused():
    t = _model_table(slots=20)
    sids = [t.open(fs_in=8001 + i, fs_out=(16000 + i) if i < 4 else None) for i in range(12)]       # 12 + 4 = 16 converters
    assert len(t.convs) == 16
    again = t.open(fs_in=8001, fs_out=16000)                     # converters that are alive are shared
    assert len(t.convs) == 16
    with pytest.raises(RuntimeError, match="converter 17"):
        t.open(fs_in=9000)
    with pytest.raises(RuntimeError, match="converter 17"):
        t.open(fs_in=8001, fs_out=9000)
    assert t.free_slots() == 7 and t._conv_users[0] == 2         # a refused open leaves nothing behind
    gone = t.lookup(sids[11])[1].rin.conv
    t.close(sids[11])                                            # 8012 -> 8000 goes with its only stream
    (slot, st, act), = t.plan()
    t.done(slot, act)
    new = t.open(fs_in=9000)
    assert t.lookup(new)[1].rin.conv == gone and t.convs[gone] == (9000, 8000) and len(t.convs) == 16
    assert t.lookup(again)[1].rin.conv == 0


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    declared = set(re.findall(r"\b(sepr_[a-z0-9_]+)\s*\(", hdr))
    names = {"sepr_streambank_convert", "sepr_streambank_carry"}
    assert names <= declared and names <= set(L.SIGNATURES)
    assert all(L.SIGNATURES[n][0] is L._i for n in names)                    # status codes: no size_t entry was added
    assert "DESIGN.md section 5c-3" in hdr
    assert re.search(r"#define\s+SEPR_VERSION\s+413\b", hdr) and L.ABI_VERSION == 413
    lib = L.load()
    assert all(hasattr(lib, n) for n in names) and lib.sepr_version() == 413
    assert sb.CONVERT_COLS == 10 and sb.MAX_CONVERTERS == 16


def _convert(src=4096, src_elems=1 << 20, dst=8192, dst_elems=1 << 20, table=4096, A=1, nmax=256, taps=(4096,), Ls=(1,), Ms=(6,), Ks=(770,),
             NC=1, null=None):
    lib = L.load()
    n = len(taps)
    arrs = [(L._fp * n)(*taps), (L._i * n)(*Ls), (L._i * n)(*Ms), (L._i * n)(*Ks)]
    if null is not None:
        arrs[null] = None
    return lib.sepr_streambank_convert(src, src_elems, dst, dst_elems, table, A, nmax, *arrs, NC, None)


def test_abi_convert_argument_checks():
    """Every check comes before any HIP call: the pointers below are not memory."""
    E = L.SEPR_EINVAL
    for name in ("src", "dst", "table"):
        assert _convert(**{name: None}) == E, name
    for i in range(4):
        assert _convert(null=i) == E
    assert _convert(taps=(None,)) == E
    assert _convert(A=0) == E and _convert(A=-1) == E and _convert(A=65536) == E
    assert _convert(NC=0) == E and _convert(NC=17, taps=(4096,) * 17, Ls=(1,) * 17, Ms=(6,) * 17, Ks=(770,) * 17) == E
    assert _convert(Ls=(0,)) == E and _convert(Ms=(0,)) == E and _convert(Ks=(0,)) == E and _convert(Ks=(771,)) == E
    assert _convert(nmax=0) == E and _convert(src_elems=0) == E and _convert(dst_elems=0) == E
    assert _convert(src=4097) == E and _convert(dst=8194) == E and _convert(table=4100) == E and _convert(taps=(4098,)) == E
    assert _convert(Ms=(24,), Ks=(3074,)) == E                                # 192 kHz -> 8 kHz: the span limit of sepr_resample_fwd
    assert _convert(NC=2, taps=(4096, 4096), Ls=(1, 1), Ms=(6, 24), Ks=(770, 3074)) == E        # every converter is checked


def test_abi_carry_argument_checks():
    lib, E = L.load(), L.SEPR_EINVAL

    def c(buf=4096, elems=1 << 20, table=4096, A=1, slots=4, S=2, hist=48, row=112):
        return lib.sepr_streambank_carry(buf, elems, table, A, slots, S, hist, row, None)

    assert c(buf=None) == E and c(table=None) == E
    assert c(A=0) == E and c(slots=0) == E and c(S=0) == E and c(S=4) == E
    assert c(hist=0) == E and c(hist=50) == E and c(row=114) == E and c(row=92) == E      # row_len < 2 hist
    assert c(elems=4 * 2 * 112 - 1) == E
    assert c(buf=4100) == E and c(table=4100) == E
