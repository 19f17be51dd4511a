"""The stream bank on the device: sepr_streambank_step (csrc/sepr_stitch.hip) fed one window per launch against the offline
sepr_stitch_fwd on the same chunk buffers, bit for bit; the bank's logic with a stub model whose forward does not depend on the batch;
the real forward through one slot against separate_long at batch 1; several slots against the offline stitch of the windows the bank
ran; the CLI."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as ref                                                   # noqa: E402

from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import streambank as sb                                 # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402
from sepreformer_amd.synth import synth_mixture                              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                                                   # guard floats on either side of the emission buffer
_models = {}


def gpu_model(variant, precision):
    key = (variant, precision)
    if key not in _models:
        _models[key] = Model.from_config(VARIANTS[variant], init_seed=0, precision=precision).load_synthetic_(0).eval().to(DEV)
    return _models[key]


def rec_chunks(S, nc, W, O, T, seed, kind, match_gain):
    """One recording's [nc, S, W] chunk buffer, the generator of tests/test_longform_gpu.py restated: 'planted' (windows of AR
    sources, sources permuted and scaled per window), 'random' (independent noise); zero past T in the last window; 'silent' zeroes a
    source over some overlaps."""
    rng = np.random.default_rng(seed)
    H = W - O
    if kind == "random":
        ch = rng.standard_normal((nc, S, W))
    else:
        n = (nc - 1) * H + W
        src = np.cumsum(rng.standard_normal((S, n)), axis=1)
        src -= src.mean(axis=1, keepdims=True)
        src = np.stack([ref.cut(src[s], W, O) for s in range(S)], axis=1)
        ch = np.empty_like(src)
        for k in range(nc):
            p = rng.permutation(S)
            g = rng.uniform(0.3, 3.0, S) * rng.choice([-1.0, 1.0], S) if match_gain else np.ones(S)
            for s in range(S):
                ch[k, p[s]] = g[s] * src[k, s]
    if kind == "silent" and nc > 1:
        for k in range(0, nc - 1, 2):
            ch[k, 0, H:] = 0.0
            ch[k + 1, 1, :O] = 0.0
    ch[-1, :, T - (nc - 1) * H:] = 0.0
    return ch.astype(np.float32)


def length_for(nc, W, O, mode):
    """'pad1': the last window holds one sample past the overlap; 'flush' / 'full': the last window is exactly full - run as a window
    like any other and then flushed, or run as the last window with n_emit = W."""
    H = W - O
    return (nc - 2) * H + W + 1 if mode == "pad1" else (nc - 1) * H + W


def steps_of(nc, T, W, O, mode):
    """(k, n_emit, has_window) of every step of a stream."""
    H = W - O
    if mode == "flush":
        return [(k, H, 1) for k in range(nc)] + [(nc, O, 0)]
    return [(k, H, 1) for k in range(nc - 1)] + [(nc - 1, T - (nc - 1) * H, 1)]


def run_streams(recs, S, W, O, match_gain, slots, ld):
    """recs: dicts with chunks [nc, S, W] (numpy), T, mode, start (first hop) and slot.  Every hop is ONE sepr_streambank_step launch
    over the streams active in it; every stream emits straight into its own packed [S, roundup4(T)] block of one buffer.
    -> per recording (y [S, T], perm [steps, S], gain [steps, S]) and the raw buffers, guards checked."""
    lib, H = L.load(), W - O
    for r in recs:
        r["steps"] = steps_of(r["chunks"].shape[0], r["T"], W, O, r["mode"])
        r["row"] = -(-r["T"] // 4) * 4
    offs, total = [], GUARD
    for r in recs:
        offs.append(total)
        total += S * r["row"]
    nhops = max(r["start"] + len(r["steps"]) for r in recs)
    out = torch.full((total + GUARD,), -7.5, dtype=torch.float32, device=DEV)
    nstate = int(lib.sepr_streambank_state_bytes(slots, S, O))
    assert nstate > 0
    state = torch.full((nstate + 512,), 0xA5, dtype=torch.uint8, device=DEV)            # garbage inside: k = 0 must reset a slot
    dev_chunks = [torch.from_numpy(r["chunks"]).to(DEV) for r in recs]
    results = [([], []) for _ in recs]
    for h in range(nhops):
        act = [(i, r, r["steps"][h - r["start"]]) for i, r in enumerate(recs) if 0 <= h - r["start"] < len(r["steps"])]
        if not act:
            continue
        act.sort(key=lambda t: -t[2][2])                                                  # rows with a window first
        A = len(act)
        assert len({r["slot"] for _, r, _ in act}) == A
        win = torch.zeros(S, A, ld, dtype=torch.float32, device=DEV)
        tab = np.zeros((A, 6), np.int64)
        for a, (i, r, (k, n_emit, has)) in enumerate(act):
            if has:
                win[:, a, :W] = dev_chunks[i][k]
            tab[a] = (r["slot"], k, n_emit, has, offs[i] - GUARD + k * H, r["row"])
        table = torch.from_numpy(tab).to(DEV)
        perm = torch.full((A, S), -1, dtype=torch.int32, device=DEV)
        gain = torch.full((A, S), -1.0, dtype=torch.float32, device=DEV)
        ptrs = (L._fp * S)(*[win[s].data_ptr() for s in range(S)])
        with torch.cuda.device(DEV):
            L.check(lib.sepr_streambank_step(ptrs, ld, table.data_ptr(), A, slots, S, W, O, int(match_gain),
                                             out.data_ptr() + 4 * GUARD, total - GUARD, perm.data_ptr(), gain.data_ptr(),
                                             state.data_ptr() + 256, nstate, torch.cuda.current_stream().cuda_stream),
                    "sepr_streambank_step")
        for a, (i, _, _) in enumerate(act):
            results[i][0].append(perm[a])
            results[i][1].append(gain[a])
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == -7.5).all()) and bool((out[total:] == -7.5).all())
    assert bool((state[:256] == 0xA5).all()) and bool((state[256 + nstate:] == 0xA5).all())
    res = []
    for i, r in enumerate(recs):
        block = out[offs[i]:offs[i] + S * r["row"]].view(S, r["row"])
        assert bool((block[:, r["T"]:] == 0).all())                                      # zeros up to roundup4, written by the kernel
        res.append((block[:, :r["T"]], torch.stack(results[i][0]), torch.stack(results[i][1])))
    return res, out, state


def check_against_offline(recs, S, W, O, match_gain, slots, ld):
    buf = torch.from_numpy(np.concatenate([r["chunks"] for r in recs])).to(DEV)
    ys, perm, gain = longform.stitch(buf, [r["T"] for r in recs], O, match_gain)
    got, out1, st1 = run_streams(recs, S, W, O, match_gain, slots, ld)
    k0 = 0
    for r, y, (gy, gp, gg) in zip(recs, ys, got):
        nc = r["chunks"].shape[0]
        assert torch.equal(gy, y), (r["T"], nc, r["mode"])
        rows = list(range(k0, k0 + nc)) + ([k0 + nc - 1] if r["mode"] == "flush" else [])   # a flush reports the state it leaves
        assert torch.equal(gp, perm[rows]), (r["T"], nc, r["mode"])
        assert torch.equal(gg.view(torch.int32), gain[rows].view(torch.int32)), (r["T"], nc, r["mode"])
        k0 += nc
    _, out2, st2 = run_streams(recs, S, W, O, match_gain, slots, ld)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32)) and torch.equal(st1, st2)


# ---- 1. the step against the offline stitch, no model ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("match_gain", [False, True])
@pytest.mark.parametrize("kind", ["planted", "random", "silent"])
def test_step_is_the_offline_stitch_one_window_per_launch(S, match_gain, kind):
    for W, O in ((64, 32), (48, 4), (2048, 512)):
        for nc in (2, 3, 70):
            recs = []
            for mode in ("pad1", "flush", "full"):
                T = length_for(nc, W, O, mode)
                assert ref.num_chunks(T, W, O) == nc
                recs.append(dict(chunks=rec_chunks(S, nc, W, O, T, 1000 * S + 10 * nc + len(recs), kind, match_gain), T=T, mode=mode,
                                 start=0, slot=len(recs)))
            for r in recs:                                                               # A = 1: one stream, one window per launch
                check_against_offline([dict(r, slot=0)], S, W, O, match_gain, slots=1, ld=W)
            check_against_offline(recs, S, W, O, match_gain, slots=3, ld=W + 4)           # A = 3, rows longer than a window


def test_step_training_geometry():
    """4 s windows, 1 s overlap: the geometry the product uses."""
    W, O, S = 32000, 8000, 2
    recs = []
    for i, (nc, mode) in enumerate(((3, "pad1"), (2, "flush"), (3, "full"))):
        T = length_for(nc, W, O, mode)
        recs.append(dict(chunks=rec_chunks(S, nc, W, O, T, 40 + i, "planted", True), T=T, mode=mode, start=i, slot=i))
    check_against_offline(recs, S, W, O, True, slots=4, ld=W)


@pytest.mark.parametrize("A", [1, 5, 33])
@pytest.mark.parametrize("S,match_gain,kind", [(2, True, "planted"), (3, False, "random"), (3, True, "silent"), (2, False, "planted")])
def test_streams_at_different_k_in_one_launch(A, S, match_gain, kind):
    """A streams with staggered starts, different window counts and endings; every slot is taken by a second recording once the first
    has emitted its last samples (the second starts at k = 0 on the state the first left)."""
    for W, O in ((64, 32), (48, 4)):
        recs = []
        for slot in range(A):
            start = slot % 4
            for gen in range(2):
                nc = (2, 3, 5, 9)[(slot + 3 * gen) % 4]
                mode = ("pad1", "flush", "full")[(slot + gen) % 3]
                T = length_for(nc, W, O, mode)
                r = dict(chunks=rec_chunks(S, nc, W, O, T, 7 * slot + gen + 100 * S, kind, match_gain), T=T, mode=mode, start=start,
                         slot=slot)
                recs.append(r)
                start += len(steps_of(nc, T, W, O, mode))                                 # the slot's next occupant
        check_against_offline(recs, S, W, O, match_gain, slots=max(A, 2) + 3, ld=W)


def test_bad_table_stays_in_bounds():
    """Slots, n_emit and offsets out of range: wrong samples at most, the guards around state and emission buffer intact."""
    W, O, S = 64, 16, 2
    T = length_for(3, W, O, "pad1")
    base = dict(chunks=rec_chunks(S, 3, W, O, T, 5, "random", True), T=T, mode="pad1", start=0)
    run_streams([dict(base, slot=99), dict(base, slot=-5, start=1)], S, W, O, True, slots=2, ld=W)
    lib = L.load()
    nstate = int(lib.sepr_streambank_state_bytes(6, S, O))
    state = torch.full((nstate + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((GUARD + 256 + GUARD,), -7.5, dtype=torch.float32, device=DEV)
    win = torch.randn(S, 6, W, device=DEV)
    tab = torch.tensor([[0, 0, 10 ** 12, 1, 0, 64],            # n_emit far past W: clamped to W
                        [1, 3, -9, 1, 128, 64],                # negative n_emit: nothing emitted; k > 0 on a state of garbage
                        [2, 1, 48, 1, 200, 64],                # the second track would end past the buffer: no emission
                        [3, 1, 48, 1, -64, 64],                # negative offset
                        [4, 1, 48, 1, 2, 64],                  # misaligned offset
                        [5, 1, 16, 0, 0, 10 ** 15]], dtype=torch.int64, device=DEV)      # a stride past everything
    perm = torch.zeros(6, S, dtype=torch.int32, device=DEV)
    gain = torch.zeros(6, S, dtype=torch.float32, device=DEV)
    ptrs = (L._fp * S)(*[win[s].data_ptr() for s in range(S)])
    with torch.cuda.device(DEV):
        L.check(lib.sepr_streambank_step(ptrs, W, tab.data_ptr(), 6, 6, S, W, O, 1, out.data_ptr() + 4 * GUARD, 256, perm.data_ptr(),
                                         gain.data_ptr(), state.data_ptr() + 256, nstate, torch.cuda.current_stream().cuda_stream), "step")
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == -7.5).all()) and bool((out[GUARD + 256:] == -7.5).all())
    assert bool((state[:256] == 0xA5).all()) and bool((state[256 + nstate:] == 0xA5).all())
    assert bool(((perm >= 0) & (perm < S)).all())


# ---- 2. the bank's logic at bitwise strength, with a stub model ---------------------------------------------------------------------
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


STUB_FS, STUB_W, STUB_O = 8000, 4000, 1000                                   # 0.5 s windows, 0.125 s overlap
STUB_KW = dict(chunk_seconds=STUB_W / STUB_FS, overlap_seconds=STUB_O / STUB_FS, fs=STUB_FS)
_stub_cache = {}


def stub_case():
    if not _stub_cache:
        W, H = STUB_W, STUB_W - STUB_O
        stub = Stub(2).to(DEV)
        xs = [synth_mixture(1, n, seed=30 + i)[0] for i, n in enumerate((W - 3, W, W + 1, 3 * H + W, 9 * H + W - 7))]
        want = [torch.stack(longform.separate_long(stub, x, batch=1, **STUB_KW)) for x in xs]
        _stub_cache.update(stub=stub, xs=xs, want=want)
    return _stub_cache["stub"], _stub_cache["xs"], _stub_cache["want"]


def test_separate_many_stub_is_separate_long_per_recording():
    stub, xs, want = stub_case()
    stub.batches.clear()
    got, bank, sids = sb.separate_many(stub, xs, slots=2, return_bank=True, **STUB_KW)
    assert len(got) == len(xs) and bank.free_slots() == 2 and stub.compute_aux is True
    assert [s is None for s in sids] == [True, True, False, False, False]                # at most W samples: the separate path
    for x, g, w in zip(xs, got, want):
        assert len(g) == 2 and all(t.shape == (x.shape[-1],) for t in g)
        assert torch.equal(torch.stack(g), w)
    assert max(b for b, _ in stub.batches) == 2                                          # two recordings shared a forward
    assert all(aux is False for b, aux in stub.batches if b == 2)


@pytest.mark.parametrize("block", [1, 1000, 7777, None])
def test_push_blocks_do_not_change_the_emissions(block):
    stub, xs, want = stub_case()
    bank = sb.StreamBank(stub, slots=2, match_gain=False, store_seconds=(len(xs[-1]) + 8) / STUB_FS, **STUB_KW)
    got = {}
    for pair in ([0, 1], [2, 3], [4]):
        sid = {r: bank.open() for r in pair}
        parts = {r: [] for r in pair}
        dx = [xs[r].to(DEV) for r in pair]
        pos = 0
        while any(pos < len(x) for x in dx):
            for r, x in zip(pair, dx):
                if pos < len(x):
                    bank.push(sid[r], x[pos:pos + (block or len(x))])
            pos += block or max(len(x) for x in dx)
            while bank.ready():
                for s, y in bank.step().items():
                    parts[[r for r in pair if sid[r] == s][0]].append(y.clone())
        for r in pair:
            bank.close(sid[r])
        for s, y in bank.drain().items():
            parts[[r for r in pair if sid[r] == s][0]].append(y)
        assert bank.free_slots() == 2 and bank.ready() == 0
        for r in pair:
            got[r] = torch.cat(parts[r], dim=1)
    for r, w in enumerate(want):
        assert torch.equal(got[r], w), (block, r)


def test_bank_refuses_what_it_cannot_hold():
    stub, xs, _ = stub_case()
    bank = sb.StreamBank(stub, slots=1, **STUB_KW)
    s = bank.open()
    with pytest.raises(RuntimeError):
        bank.open()
    bank.push(s, np.zeros(bank.cap, np.float32))
    with pytest.raises(OverflowError):
        bank.push(s, torch.zeros(1))
    bank.push(s, torch.zeros(0))
    with pytest.raises(ValueError):
        bank.push(s, torch.zeros(2, 2))


# ---- 3. the real forward through one slot --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,precision", [("tiny", "fp32"), ("tiny", "bf16x3"), ("SepReformer_Base_WSJ0", "bf16x3")])
def test_one_slot_is_separate_long_at_batch_1(variant, precision):
    m = gpu_model(variant, precision)
    x = synth_mixture(1, 160000 + 1234, seed=11)[0]
    want = torch.stack(longform.separate_long(m, x, batch=1))
    bank = sb.StreamBank(m, slots=1)
    sid = bank.open()
    parts = []
    for p in range(0, len(x), 4000):                                                    # 0.5 s pushes
        bank.push(sid, x[p:p + 4000])
        while bank.ready():
            parts.append(bank.step()[sid].clone())
    bank.close(sid)
    parts.append(bank.drain()[sid])
    assert torch.equal(torch.cat(parts, dim=1), want)
    assert bank.free_slots() == 1 and m.compute_aux is True
    short = synth_mixture(1, 20003, seed=3)[0]
    sid = bank.open()
    bank.push(sid, short.numpy())
    bank.close(sid)
    got = bank.step()[sid]
    for g, w in zip(got, infer.separate(m, short[None])):
        assert torch.equal(g, w[0])


# ---- 4. the real forward, several slots ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match_gain", [False, True])
def test_several_slots_equal_the_offline_stitch_of_the_windows_run(match_gain):
    m = gpu_model("tiny", "bf16x3")
    lengths = (70001, 1000, 32000, 40000, 32000 + 2 * 24000, 100003)
    xs = [synth_mixture(1, n, seed=50 + i)[0] for i, n in enumerate(lengths)]
    assert m.compute_aux is True
    outs, bank, sids = sb.separate_many(m, xs, slots=3, match_gain=match_gain, return_bank=True, keep_windows=True)
    assert bank.free_slots() == 3 and bank.ready() == 0 and m.compute_aux is True
    for x, out, sid in zip(xs, outs, sids):
        T = x.shape[-1]
        y = torch.stack(out)
        assert y.shape == (m.num_spks, T) and bool(torch.isfinite(y).all())
        if sid is None:
            assert T <= bank.W
            continue
        kept = torch.stack(bank.kept[sid])
        assert kept.shape[0] == ref.num_chunks(T, bank.W, bank.O)
        want, _, _ = longform.stitch(kept, [T], bank.O, match_gain)
        assert torch.equal(y, want[0]), T


# ---- 5. the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_several_files(tmp_path):
    names = {"short": 2 * 8000 + 11, "long": 9 * 8000 + 37}
    for d in ("bank", "single"):
        os.makedirs(tmp_path / d)
        for i, (name, n) in enumerate(names.items()):
            x = synth_mixture(1, n, seed=60 + i)[0].numpy()
            infer.write_wav(str(tmp_path / d / f"{name}.wav"), 0.5 * x / np.abs(x).max(), 8000)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SEPR_PRECISION="fp32")
    base = [sys.executable, "-m", "sepreformer_amd.infer"]
    common = ["--model", "tiny", "--chunk-seconds", "4", "--overlap-seconds", "1"]
    wavs = [str(tmp_path / "bank" / f"{n}.wav") for n in names]
    r = subprocess.run(base + wavs + common + ["--slots", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    written = r.stdout.strip().split("\n")
    assert written == [str(tmp_path / "bank" / f"{n}{suffix}.wav") for n in names for suffix in ("_in", "_out_0", "_out_1")]
    for n in names:
        wav = str(tmp_path / "single" / f"{n}.wav")
        r = subprocess.run(base + [wav] + common + ["--batch", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        for suffix in ("_in", "_out_0", "_out_1"):
            a = open(tmp_path / "bank" / f"{n}{suffix}.wav", "rb").read()
            b = open(tmp_path / "single" / f"{n}{suffix}.wav", "rb").read()
            assert a == b and len(a) > 44, (n, suffix)
