"""Sample-rate conversion inside the stream bank on the device.  Everything is held to the offline composition

    resample(separate_long(model, resample(x, fs_in, fs), batch=1), fs, fs_out)

with torch.equal: sepr_streambank_convert alone against resample.resample of the whole recording (itself held to float64 by
tests/test_resample_gpu.py), the bank with a stub model that is bitwise independent of its batch, the real forward through one slot,
separate_many(rates=...), and the CLI's bytes."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rate_ref as srr                                                # noqa: E402

from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402
from sepreformer_amd import streambank as sb                                 # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402
from sepreformer_amd.synth import synth_mixture                              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = sb.CONVERT_COLS


def _conv_args(plans):
    tabs = [rs._table(a, b, torch.device(DEV)) for a, b in plans]
    n = len(tabs)
    return ((L._fp * n)(*[t.data_ptr() for _, t in tabs]), (L._i * n)(*[p.L for p, _ in tabs]), (L._i * n)(*[p.M for p, _ in tabs]),
            (L._i * n)(*[p.K for p, _ in tabs]), n)


def _launch(src, dst, table, nmax, args):
    lib = L.load()
    tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).to(DEV)
    L.check(lib.sepr_streambank_convert(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), tab.data_ptr(), table.shape[0], nmax,
                                        *args, torch.cuda.current_stream().cuda_stream), "sepr_streambank_convert")
    return tab                                                               # alive until the caller drops it, after the launch is queued


# ---- 1. the entry alone against the offline kernel ------------------------------------------------------------------------------------
def test_convert_in_pieces_is_the_whole_recording():
    """Six converters in ONE launch per step (L = 1 and L > 1 among them), six lengths each; every row reads a ring hardly longer than one
    output's inputs plus a push and writes a ring hardly longer than a step's outputs, so both wrap many times over 5000 samples."""
    INC = 150
    rng = np.random.default_rng(5)
    args = _conv_args(srr.PLANS)
    rows = []
    sbase = dbase = 0
    for c, (fa, fb) in enumerate(srr.PLANS):
        Lr, Mr, K, Hh = sb.geometry(fa, fb)
        span = srr.span(fa, fb)
        for T in (1, Hh + 1, Hh + 2, span - 1, span + 1, 5000 + 7 * c):
            x = torch.from_numpy(rng.standard_normal(T).astype(np.float32)).to(DEV)
            scap, dcap = K + Mr // Lr + 4 + INC, (INC + K) * Lr // Mr + 4         # the close brings the tail's outputs at once
            rows.append(dict(c=c, L=Lr, M=Mr, Hh=Hh, T=T, x=x, scap=scap, dcap=dcap, sbase=sbase, dbase=dbase, recv=0, done=0, closed=False,
                             N=sb.out_len(T, Lr, Mr), y=torch.full((sb.out_len(T, Lr, Mr),), float("nan"), device=DEV)))
            sbase += scap + 3                                                # a gap between the rings: a stray write would be seen
            dbase += dcap + 3
    assert min(r["T"] for r in rows if r["T"] > 4000) // max(r["scap"] for r in rows) >= 5         # at least five wraps
    src = torch.zeros(sbase, device=DEV)
    dst = torch.full((dbase,), 7.0, device=DEV)
    steps = 0
    while any(r["done"] < r["N"] for r in rows):
        table, live = [], []
        for r in rows:
            if r["closed"]:
                continue
            inc = min(int(rng.choice([0, 1, int(rng.integers(2, INC)), int(rng.integers(INC // 2, INC + 1))])), r["T"] - r["recv"])
            if inc == 0 and r["recv"] == r["T"]:
                r["closed"] = True
            a, b = r["recv"], r["recv"] + inc
            if inc:
                src[r["sbase"] + torch.arange(a, b, device=DEV) % r["scap"]] = r["x"][a:b]
            r["recv"] = b
            n1 = sb.ready_count(b, r["closed"], r["L"], r["M"], r["Hh"])
            assert n1 - r["done"] <= r["dcap"]
            table.append((r["c"], r["done"], n1, b, r["sbase"], 0, r["scap"], r["dbase"], 0, r["dcap"]))
            live.append((r, r["done"], n1))
            r["done"] = n1
        keep = _launch(src, dst, np.array(table), max(1, max(n1 - n0 for _, n0, n1 in live)), args)
        for r, n0, n1 in live:
            if n1 > n0:
                r["y"][n0:n1] = dst[r["dbase"] + torch.arange(n0, n1, device=DEV) % r["dcap"]]
        del keep
        steps += 1
    assert steps > 60
    for c, (fa, fb) in enumerate(srr.PLANS):
        mine = [r for r in rows if r["c"] == c]
        for r, w in zip(mine, rs.resample([r["x"] for r in mine], fa, fb)):
            assert r["y"].shape == w.shape and torch.equal(r["y"], w), (fa, fb, r["T"])
    gaps = torch.ones(dbase, dtype=torch.bool, device=DEV)
    for r in rows:
        gaps[r["dbase"]:r["dbase"] + r["dcap"]] = False
    assert bool((dst[gaps] == 7.0).all())                                    # nothing was written between the rings


@pytest.mark.parametrize("fs_a,fs_b", srr.PLANS)
def test_output_direction_with_the_history_carry(fs_a, fs_b):
    """A track of 3 H + W samples emitted hop by hop into rows [slot][S][H + W] (history, then the hop's emission), converted from there
    and carried by sepr_streambank_carry; a slot that does not step keeps its row."""
    W, O, S, slots, slot = 4000, 1000, 2, 3, 1
    H = W - O
    T = 3 * H + W
    lib = L.load()
    Lr, Mr, K, Hh = sb.geometry(fs_a, fs_b)
    assert K <= H
    tracks = torch.from_numpy(np.random.default_rng(fs_a + fs_b).standard_normal((S, T)).astype(np.float32)).to(DEV)
    buf = torch.full((slots, S, H + W), 3.0, device=DEV)                     # stale history: window 0 must not read it
    ocap = (W + H) * Lr // Mr + 8
    dst = torch.zeros(S, ocap, device=DEV)
    args = _conv_args([(fs_a, fs_b)])
    got, done = [], 0
    for k in range(4):
        n_emit, fin = (H, False) if k < 3 else (W, True)
        buf[slot, :, H:H + n_emit] = tracks[:, k * H:k * H + n_emit]         # what the step emits
        E = k * H + n_emit
        n1 = sb.ready_count(E, fin, Lr, Mr, Hh)
        table = np.array([(0, done, n1, E, (slot * S + s) * (H + W), k * H - H, H + W, s * ocap, done, ocap) for s in range(S)])
        keep = _launch(buf, dst, table, n1 - done, args)
        got.append(dst[:, :n1 - done].clone())
        step_tab = torch.tensor([[slot, k, n_emit, 1, 0, 0]], dtype=torch.int64, device=DEV)
        L.check(lib.sepr_streambank_carry(buf.data_ptr(), buf.numel(), step_tab.data_ptr(), 1, slots, S, H, H + W,
                                          torch.cuda.current_stream().cuda_stream), "sepr_streambank_carry")
        if not fin:
            assert torch.equal(buf[slot, :, :H], tracks[:, E - H:E])
        done = n1
        del keep
    want = torch.stack(rs.resample([t for t in tracks], fs_a, fs_b))
    assert torch.equal(torch.cat(got, dim=1), want)
    assert bool((buf[0] == 3.0).all()) and bool((buf[2] == 3.0).all())


# ---- 2. the bank, with a stub model -----------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """Elementwise in the input and different per source: bitwise independent of the batch it runs in."""

    def __init__(self, S=2):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.cfg = SimpleNamespace(enc_stride=4, enc_kernel=16)
        self.num_spks, self.compute_aux = S, True
        self.batches = []

    def forward(self, x):
        self.batches.append((int(x.shape[0]), self.compute_aux))
        return [x * 1.5 + x.abs(), x * x * 0.5 - x, (x + 0.25) * x.abs()][:self.num_spks], []


FS, W, O = 8000, 4000, 1000
H = W - O
KW = dict(chunk_seconds=W / FS, overlap_seconds=O / FS, fs=FS)
RATES = (48000, 44100, 16000, 8000)
LENGTHS = (W - 3, W + 1, 3 * H + W, 5 * H + W - 7)                           # at the model's rate
_cache = {}


def offline(model, x, fs_in, fs_out, **kw):
    """The definition."""
    y = longform.separate_long(model, rs.resample(x.to(DEV), fs_in, FS), batch=1, **kw)
    return torch.stack(rs.resample([t.contiguous() for t in y], FS, fs_out))


def stub_case():
    if not _cache:
        stub = Stub(2).to(DEV)
        xs, want = {}, {}
        for i, rate in enumerate(RATES):
            Lr, Mr, _, _ = sb.geometry(rate, FS)
            for j, N in enumerate(LENGTHS):
                T_in = N * Mr // Lr
                assert sb.out_len(T_in, Lr, Mr) == N
                xs[rate, N] = synth_mixture(1, T_in, seed=100 + 10 * i + j)[0]
                want[rate, N] = offline(stub, xs[rate, N], rate, rate, **KW)
        _cache.update(stub=stub, xs=xs, want=want)
    return _cache["stub"], _cache["xs"], _cache["want"]


def run_pair(bank, jobs, block):
    """``jobs``: [(x on the device, rate)] - at most as many as the bank has slots - pushed in turns in blocks of ``block`` samples
    (None: the whole recording) with every ready hop run in between -> what each stream returned, concatenated."""
    sids = [bank.open(fs_in=rate, fs_out=rate) for _, rate in jobs]
    parts = {s: [] for s in sids}
    pos = 0
    while any(pos < len(x) for x, _ in jobs):
        for s, (x, _) in zip(sids, jobs):
            if pos < len(x):
                bank.push(s, x[pos:pos + (block or len(x))])
        pos += block or max(len(x) for x, _ in jobs)
        while bank.ready():
            for s, y in bank.step().items():
                parts[s].append(y.clone())
    for s in sids:
        bank.close(s)
    for s, y in bank.drain().items():
        parts[s].append(y)
    assert bank.free_slots() == bank.slots and bank.ready() == 0
    return [torch.cat(parts[s], dim=1) for s in sids]


@pytest.mark.parametrize("block", [997, None])
def test_bank_is_the_offline_composition(block):
    stub, xs, want = stub_case()
    bank = sb.StreamBank(stub, slots=2, store_seconds=(max(LENGTHS) + 8) / FS, **KW)
    keys = [(rate, N) for rate in RATES for N in LENGTHS]
    half = len(keys) // 2
    for ka, kb in zip(keys[:half], keys[half:]):                              # a 48 or 44.1 kHz stream beside a 16 or 8 kHz one
        got = run_pair(bank, [(xs[ka].to(DEV), ka[0]), (xs[kb].to(DEV), kb[0])], block)
        for k, g in zip((ka, kb), got):
            assert g.shape == want[k].shape and torch.equal(g, want[k]), (block, k)
    for N in LENGTHS:                                                         # the model's rate: today's bits
        w = torch.stack(longform.separate_long(stub, xs[8000, N], batch=1, **KW))
        assert torch.equal(want[8000, N], w)
    assert 4 <= len(bank.table.convs) <= 6 and stub.compute_aux is True       # four alive at a time, freed entries are reused


def test_bank_one_sample_at_a_time():
    stub, xs, want = stub_case()
    bank = sb.StreamBank(stub, slots=2, **KW)
    k = (16000, W + 1)
    got, = run_pair(bank, [(xs[k].to(DEV), 16000)], 1)
    assert torch.equal(got, want[k])


def test_a_bank_without_rates_allocates_and_launches_nothing_new():
    stub, xs, want = stub_case()
    bank = sb.StreamBank(stub, slots=2, store_seconds=(3 * H + W + 8) / FS, **KW)
    sid = bank.open(fs_in=FS, fs_out=None)
    bank.push(sid, xs[8000, 3 * H + W])
    bank.close(sid)
    got = bank.drain()[sid]
    assert torch.equal(got, want[8000, 3 * H + W])
    assert bank._raw is None and bank._hist is None and bank._olive is None and bank.table.convs == []
    with pytest.raises(ValueError, match="max_rate"):
        bank.open(fs_in=96000)
    assert bank.free_slots() == 2


# ---- 3. the real forward, one slot --------------------------------------------------------------------------------------------------------
def test_real_forward_one_slot_16k():
    m = Model.from_config(VARIANTS["tiny"], init_seed=0, precision="fp32").load_synthetic_(0).eval().to(DEV)
    x = synth_mixture(1, 2 * (32000 + 2 * 24000 + 22403) + 1, seed=21)[0]    # 3.2 windows' worth of 4 s at the model's rate
    want = offline(m, x, 16000, 16000)
    bank = sb.StreamBank(m, slots=1)
    sid = bank.open(fs_in=16000, fs_out=16000)
    parts = []
    for p in range(0, len(x), 8000):                                         # 0.5 s pushes
        bank.push(sid, x[p:p + 8000])
        while bank.ready():
            parts.append(bank.step()[sid].clone())
    bank.close(sid)
    parts.append(bank.drain()[sid])
    got = torch.cat(parts, dim=1)
    assert got.shape == want.shape and torch.equal(got, want)
    assert bank.free_slots() == 1 and m.compute_aux is True


# ---- 4. separate_many(rates=...) --------------------------------------------------------------------------------------------------------
def test_separate_many_with_rates_stub():
    stub, xs, _ = stub_case()
    keys = [(48000, 5 * H + W - 7), (8000, 3 * H + W), (16000, W - 3), (44100, 3 * H + W), (16000, W + 1), (48000, W + 1)]
    recs = [xs[k] for k in keys]
    rates = [k[0] for k in keys]
    want = sb.separate_many(stub, [rs.resample(x.to(DEV), r, FS) for x, r in zip(recs, rates)], slots=2, **KW)
    stub.batches.clear()
    got, bank, sids = sb.separate_many(stub, recs, slots=2, rates=rates, return_bank=True, **KW)
    assert [s is None for s in sids] == [False, False, True, False, False, False]
    assert bank.free_slots() == 2 and max(b for b, _ in stub.batches) == 2
    for k, g, w in zip(keys, got, want):
        assert len(g) == 2 and g[0].shape == (k[1],)
        assert torch.equal(torch.stack(g), torch.stack(w)), k
    with pytest.raises(ValueError, match="rates"):
        sb.separate_many(stub, recs, slots=2, rates=rates[:-1], **KW)


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_files_at_16k(tmp_path):
    names = {"short": 2 * (2 * 8000 + 11), "long": 2 * (9 * 8000 + 37) + 1}
    for d in ("bank", "single"):
        os.makedirs(tmp_path / d)
        for i, (name, n) in enumerate(names.items()):
            x = synth_mixture(1, n, seed=70 + i)[0].numpy()
            infer.write_wav(str(tmp_path / d / f"{name}.wav"), 0.5 * x / np.abs(x).max(), 16000)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SEPR_PRECISION="fp32")
    base = [sys.executable, "-m", "sepreformer_amd.infer"]
    common = ["--model", "tiny", "--chunk-seconds", "4", "--overlap-seconds", "1", "--resample", "--out-rate", "input"]
    wavs = [str(tmp_path / "bank" / f"{n}.wav") for n in names]
    r = subprocess.run(base + wavs + common + ["--slots", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().split("\n") == [str(tmp_path / "bank" / f"{n}{suffix}.wav") for n in names
                                            for suffix in ("_in", "_out_0", "_out_1")]
    for n in names:
        wav = str(tmp_path / "single" / f"{n}.wav")
        r = subprocess.run(base + [wav] + common + ["--batch", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        for suffix in ("_in", "_out_0", "_out_1"):
            a = open(tmp_path / "bank" / f"{n}{suffix}.wav", "rb").read()
            b = open(tmp_path / "single" / f"{n}{suffix}.wav", "rb").read()
            assert a == b and len(a) > 44, (n, suffix)
