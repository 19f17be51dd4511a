"""Long-form separation on the device: sepr_stitch_fwd (csrc/sepr_stitch.hip) against the float64 restatement
(tests/longform_ref.py) on planted and random chunk buffers; separate_long against separate, the oracle and the restatement;
bounded memory on 10 minutes; the multi-recording surface and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as ref                                                   # noqa: E402

from oracle import sepreformer_oracle as orc                                 # noqa: E402
from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402
from sepreformer_amd.synth import synth_mixture, synth_state_dict            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_DB = 80.0
_models = {}


def gpu_model(variant, precision):
    key = (variant, precision)
    if key not in _models:
        _models[key] = Model.from_config(VARIANTS[variant], init_seed=0, precision=precision).load_synthetic_(0).eval().to(DEV)
    return _models[key]


def _rec_chunks(S, nc, W, O, T, seed, kind, match_gain):
    """One recording's [nc, S, W] chunk buffer: 'planted' (windows of AR sources, sources permuted and scaled per window) or
    'random' (independent noise); zero past T in the last window; 'silent' zeroes a source over some overlaps."""
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


def _check_stitch(recs, lengths, O, match_gain):
    """recs: list of [nc, S, W] float32 -> device vs restatement, exact permutations, gains / outputs within 1e-6 of the peak,
    two calls bit-identical."""
    buf = torch.from_numpy(np.concatenate(recs)).to(DEV)
    ys, perm, gain = longform.stitch(buf, lengths, O, match_gain)
    ys2, perm2, gain2 = longform.stitch(buf, lengths, O, match_gain)
    assert torch.equal(perm, perm2) and torch.equal(gain, gain2)
    for a, b in zip(ys, ys2):
        assert torch.equal(a, b)
    perm, gain = perm.cpu().numpy(), gain.cpu().numpy()
    k = 0
    for ch, T, y in zip(recs, lengths, ys):
        nc = ch.shape[0]
        want_y, want_p, want_g = ref.stitch(ch.astype(np.float64), T, O, match_gain)
        assert np.array_equal(perm[k:k + nc], want_p), (T, nc)
        gp = np.abs(want_g).max()
        assert np.abs(gain[k:k + nc] - want_g).max() <= 1e-6 * gp
        y = y.cpu().numpy()
        assert y.shape == want_y.shape
        assert np.abs(y - want_y).max() <= 1e-6 * max(np.abs(want_y).max(), 1e-30), (T, nc)
        k += nc


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("match_gain", [False, True])
@pytest.mark.parametrize("kind", ["planted", "random", "silent"])
def test_stitch_matches_restatement(S, match_gain, kind):
    W, O = 64, 16
    H = W - O
    ncs = [1, 2, 3, 57, 1200]
    lengths = [W - 5 if nc == 1 else W + (nc - 2) * H + 1 + (7 * nc) % H for nc in ncs]   # the last windows zero-padded
    recs = [_rec_chunks(S, nc, W, O, T, 100 * S + nc, kind, match_gain) for nc, T in zip(ncs, lengths)]
    for ch, T, nc in zip(recs, lengths, ncs):
        assert ch.shape[0] == nc == ref.num_chunks(T, W, O)
        _check_stitch([ch], [T], O, match_gain)                         # R = 1
    _check_stitch(recs, lengths, O, match_gain)                         # R = 5, one call


def test_stitch_training_geometry():
    """4 s windows, 1 s overlap: the geometry the product uses (float4 paths over 8000-sample overlaps)."""
    W, O = 32000, 8000
    lengths = [73600, 32000 + 24000 * 4 + 3]
    recs = [_rec_chunks(2, ref.num_chunks(T, W, O), W, O, T, 7 + i, "planted", True) for i, T in enumerate(lengths)]
    _check_stitch(recs, lengths, O, True)
    _check_stitch(recs, lengths, O, False)


@pytest.mark.parametrize("variant,precision", [("tiny", "fp32"), ("tiny", "bf16x3"), ("SepReformer_Base_WSJ0", "fp32"),
                                               ("SepReformer_Base_WSJ0", "bf16x3")])
def test_short_recording_is_separate(variant, precision):
    m = gpu_model(variant, precision)
    x = synth_mixture(1, 20003, seed=3)[0]
    got = longform.separate_long(m, x)
    want = infer.separate(m, x[None])
    assert len(got) == len(want) == m.num_spks
    for g, w in zip(got, want):
        assert torch.equal(g, w[0])
    got2 = longform.separate_long(m, x[None].to(DEV), chunk_seconds=20004 / 8000, overlap_seconds=0.5)
    for g, w in zip(got2, want):
        assert torch.equal(g, w[0])


def _end_to_end(variant, precision, x, oracle_chunks):
    m = gpu_model(variant, precision)
    out, plan = longform.separate_long(m, x, return_plan=True)
    W, O = plan["W"], plan["O"]
    T = x.shape[-1]
    nc = ref.num_chunks(T, W, O)
    chunks = plan["chunks"]
    assert tuple(chunks.shape) == (nc, m.num_spks, W) and plan["stitched"] == [0]
    # forward part: the window outputs against the oracle on the same zero-padded windows
    wins = torch.from_numpy(ref.cut(x.numpy(), W, O))
    sd = synth_state_dict(VARIANTS[variant], 0)
    for k in (range(nc) if oracle_chunks is None else oracle_chunks):
        audio, _ = orc.model_forward(sd, m.cfg, wins[k:k + 1])
        db = orc.agreement_db(chunks[k].cpu(), torch.cat(list(audio), 0))
        assert db >= MIN_DB, (variant, precision, k, db)
    # stitch part: the restatement applied to the device's window outputs
    ch = chunks.cpu().numpy().astype(np.float64)
    want_y, want_p, want_g = ref.stitch(ch, T, O, False)
    assert np.array_equal(plan["perm"].cpu().numpy(), want_p)
    assert np.array_equal(plan["gain"].cpu().numpy(), want_g)
    y = torch.stack(out).cpu().numpy()
    assert y.shape == (m.num_spks, T) and np.isfinite(y).all()
    assert np.abs(y - want_y).max() <= 1e-6 * np.abs(want_y).max()
    _, plan_g = longform.separate_long(m, x, match_gain=True, return_plan=True)
    want_y, want_p, want_g = ref.stitch(ch, T, O, True)
    assert np.array_equal(plan_g["perm"].cpu().numpy(), want_p)
    assert np.abs(plan_g["gain"].cpu().numpy() - want_g).max() <= 1e-6 * np.abs(want_g).max()


@pytest.mark.parametrize("variant,precision,oracle_chunks", [("tiny", "fp32", None), ("tiny", "bf16x3", None),
                                                             ("SepReformer_Base_WSJ0", "bf16x3", (0, 3, 6))])
def test_end_to_end_20s(variant, precision, oracle_chunks):
    _end_to_end(variant, precision, synth_mixture(1, 160000 + 1234, seed=11)[0], oracle_chunks)


def test_end_to_end_sample_wav():
    x = torch.from_numpy(infer.load_wav(os.path.join(ROOT, "tests", "golden", "sample_WSJ.wav"), 8000))
    assert ref.num_chunks(x.shape[-1], 32000, 8000) == 3
    _end_to_end("SepReformer_Base_WSJ0", "bf16x3", x, None)


def test_bounded_memory_10_minutes():
    m = gpu_model("SepReformer_Base_WSJ0", "bf16x3")
    W, O, B, S = 32000, 8000, 32, m.num_spks
    H = W - O
    T = 600 * 8000
    nc = ref.num_chunks(T, W, O)
    x = synth_mixture(1, T, seed=5)[0]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m(torch.zeros(B, W, device=DEV))                                    # one batch of windows: workspace + activations
    torch.cuda.synchronize()
    one_batch = torch.cuda.max_memory_allocated() - base
    ws = m.engine().workspace_bytes(B, m.cfg.frames(W), m.cfg.padded_frames(m.cfg.frames(W)))     # held already if cached
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = longform.separate_long(m, x, batch=B)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    # section 5c: one batch's forward + O(S sum T W / H): the window outputs, y, the padded input and the batch's windows
    per_rec = 4 * (S * nc * W + S * (nc * H + O) + (nc - 1) * H + W + T)
    bound = ws + one_batch + 2 * per_rec
    assert grew <= bound, (grew, one_batch, per_rec)
    assert len(out) == S and all(tuple(o.shape) == (T,) for o in out)
    assert all(bool(torch.isfinite(o).all()) for o in out)


def test_multi_recording_call_is_bitwise_the_single_calls():
    m = gpu_model("tiny", "bf16x3")
    xs = [synth_mixture(1, n, seed=20 + i)[0] for i, n in enumerate((70001, 1000, 32000, 40000))]
    multi = longform.separate_long(m, xs)
    assert len(multi) == len(xs)
    for x, got in zip(xs, multi):
        want = longform.separate_long(m, x)
        assert len(got) == len(want) == m.num_spks
        for g, w in zip(got, want):
            assert g.shape == (x.shape[-1],) and torch.equal(g, w)


def test_cli_chunk_seconds(tmp_path):
    from sepreformer_amd.synth import synth_mixture as mix
    x = mix(1, 9 * 8000 + 37, seed=9)[0].numpy()
    x = 0.5 * x / np.abs(x).max()
    wav = str(tmp_path / "long.wav")
    infer.write_wav(wav, x, 8000)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "sepreformer_amd.infer", wav, "--model", "tiny", "--chunk-seconds", "4",
                        "--overlap-seconds", "1", "--match-gain"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    written = r.stdout.strip().split("\n")
    assert written == [str(tmp_path / "long_in.wav")] + [str(tmp_path / f"long_out_{i}.wav") for i in range(2)]
    m = gpu_model("tiny", Model.from_config(VARIANTS["tiny"]).precision)
    est = longform.separate_long(m, torch.from_numpy(infer.load_wav(wav, 8000)), match_gain=True)
    from scipy.io import wavfile
    for i, e in enumerate(est):
        want = np.clip(np.rint(infer.peak_normalise(e.cpu().numpy(), 0.9).astype(np.float64) * 32767.0), -32768, 32767)
        _, got = wavfile.read(written[1 + i])
        assert got.dtype == np.int16 and np.array_equal(got.astype(np.float64), want)
