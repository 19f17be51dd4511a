"""Sample-rate conversion on the device: sepr_resample_fwd (csrc/sepr_resample.hip) against the float64 restatement
(tests/resample_ref.py) on noise, speech and ragged lengths at every ratio; run-to-run and batch independence; 64-bit indexing
on 12 minutes; the file path (separate_file / separate_long_file / the CLI with resample and out_rate).

The bound of every comparison, derived and not measured: the only float32 rounding is the last one (half an ulp, at most
2^-24 |y|; 2^-23 |y_ref| allows for y_ref itself being unrounded), and the float64 sum of at most 770 exact products errs by less
than 770 * 2^-52 * sum|tap| * max|x|, about 1e-12 max|x|; the second term is 100 times that."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref                                                   # noqa: E402
import test_gpu_parity as tgp                                                # noqa: E402

from oracle import sepreformer_oracle as orc                                 # noqa: E402
from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_WSJ.wav")
RATIOS = [(48000, 8000), (44100, 8000), (16000, 8000), (22050, 8000), (32000, 8000), (8000, 16000), (8000, 44100), (8000, 48000)]
_models = {}


def gpu_model(variant="tiny"):
    if variant not in _models:
        _models[variant] = Model.from_config(VARIANTS[variant], init_seed=0).load_synthetic_(0).eval().to(DEV)
    return _models[variant]


def _check(x, y, fs_in, fs_out, positions=None, what=""):
    """Every sample of the device result y (or those at `positions`) against the restatement of x."""
    want = ref.resample(x, fs_in, fs_out, positions=positions)
    got = y.cpu().numpy().astype(np.float64)
    if positions is not None:
        got = got[positions]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    excess = np.abs(got - want) - (2.0 ** -23 * np.abs(want) + 1e-10 * np.abs(x).max())
    print(f"{what} {fs_in}->{fs_out}: {want.shape[0]} samples, max |err| {np.abs(got - want).max():.3g}, max|x| {np.abs(x).max():.3g}, "
          f"worst margin to the bound {excess.max():.3g}")
    assert np.all(excess <= 0.0), (what, fs_in, fs_out, int(np.argmax(excess)), float(excess.max()))


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_noise_matches_restatement(fs_in, fs_out):
    x = np.random.default_rng(fs_in + fs_out).standard_normal(40003).astype(np.float32)
    y = rs.resample(torch.from_numpy(x).to(DEV), fs_in, fs_out)
    assert y.device.type == "cuda" and y.dtype == torch.float32 and y.dim() == 1
    _check(x, y, fs_in, fs_out, what="noise")
    y2 = rs.resample(torch.from_numpy(x)[None], fs_in, fs_out)           # a CPU [1, T] tensor is copied to the device
    assert y2.device.type == "cuda" and tuple(y2.shape) == (1, y.shape[0]) and torch.equal(y2[0], y)


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_speech_matches_restatement(fs_in, fs_out):
    x = infer.load_wav(SAMPLE, 8000)                                     # the samples, read as a recording at fs_in
    y = rs.resample(torch.from_numpy(x).to(DEV), fs_in, fs_out)
    _check(x, y, fs_in, fs_out, what="speech")


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_ragged_lengths_match_restatement(fs_in, fs_out):
    L, M, K, Hh, _ = ref.geometry(fs_in, fs_out)
    lengths = [1, 5, M + 1, K - 1, K // 3, 1000 * M + 3, 12345, 256 * M, 2]   # T % M != 0, T < K, a tile boundary, T = 1
    rng = np.random.default_rng(7)
    xs = [(rng.standard_normal(T) * rng.uniform(0.01, 10)).astype(np.float32) for T in lengths]
    ys = rs.resample([torch.from_numpy(x).to(DEV) for x in xs], fs_in, fs_out)
    assert isinstance(ys, list) and len(ys) == len(xs)
    for x, y in zip(xs, ys):
        assert y.shape[0] == ref.out_len(x.shape[0], L, M)
        _check(x, y, fs_in, fs_out, what=f"ragged T={x.shape[0]}")


@pytest.mark.parametrize("fs_in,fs_out", [(48000, 8000), (44100, 8000), (8000, 44100), (8000, 16000)])
def test_bit_identical_and_independent_of_the_batch(fs_in, fs_out):
    rng = np.random.default_rng(3)
    xs = [torch.from_numpy(rng.standard_normal(T).astype(np.float32)).to(DEV) for T in (70001, 1, 999, 32000, 443)]
    a = rs.resample(xs, fs_in, fs_out)
    b = rs.resample(xs, fs_in, fs_out)
    for x, ya, yb in zip(xs, a, b):
        assert torch.equal(ya, yb)                                       # two calls
        assert torch.equal(ya, rs.resample(x, fs_in, fs_out))            # five recordings in one call = the five single calls


def test_index_width_12_minutes():
    """44.1 kHz -> 8 kHz: n * M passes 2^31 after 4.87 M outputs of the 5.76 M."""
    fs_in, fs_out = 44100, 8000
    T = 12 * 60 * fs_in
    x = np.random.default_rng(11).standard_normal(T).astype(np.float32)
    y = rs.resample(torch.from_numpy(x).to(DEV), fs_in, fs_out)
    N = y.shape[0]
    assert N == 12 * 60 * fs_out and (N - 1) * 441 > 2 ** 31
    pos = np.concatenate([np.arange(4096), N // 2 + np.arange(4096), N - 4096 + np.arange(4096),
                          2 ** 31 // 441 - 2048 + np.arange(4096)])        # and the crossing itself
    _check(x, y, fs_in, fs_out, positions=pos, what="12 minutes")


def test_equal_rates_return_the_very_tensor():
    x = torch.randn(1000, device=DEV)
    y = rs.resample(x, 8000, 8000)
    assert y is x and y.data_ptr() == x.data_ptr()


# ---- the file path ----------------------------------------------------------------------------------------------------------
def _write_16k(path, x8):
    """x8 at 8 kHz -> a PCM16 file at 16 kHz, converted by the restatement."""
    y = ref.resample(x8, 8000, 16000)
    infer.write_wav(path, 0.9 * y / np.abs(y).max(), 16000)
    return infer.load_audio(path)[0]


def _read(path):
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    assert data.dtype == np.int16 and data.ndim == 1
    return sr, data


def _pcm(x):
    return np.clip(np.rint(infer.peak_normalise(x, 0.9).astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)


def _check_files(written, prefix, rate, want_in, want_outs):
    assert written == [prefix + "_in.wav"] + [f"{prefix}_out_{i}.wav" for i in range(len(want_outs))]
    for path, want in zip(written, [want_in] + list(want_outs)):
        sr, got = _read(path)
        assert sr == rate and np.array_equal(got, _pcm(want)), path


def test_separate_file_resamples(tmp_path):
    m = gpu_model()
    p16 = str(tmp_path / "s16.wav")
    x16 = _write_16k(p16, infer.load_wav(SAMPLE, 8000))
    data, sr = infer.load_audio(p16)
    assert sr == 16000
    x8 = rs.resample(torch.from_numpy(data), sr, 8000, device=DEV)
    T8 = x8.shape[0]
    assert T8 == -(-x16.shape[0] // 2)
    want = torch.stack([e[0] for e in infer.separate(m, x8[None])])
    with pytest.raises(RuntimeError, match="sampling rate"):
        infer.separate_file(m, p16)                                      # the default still raises
    raw, written = infer.separate_file(m, p16, resample=True, out_prefix=str(tmp_path / "a"))
    assert raw.shape == (m.num_spks, T8) and np.array_equal(raw, want.cpu().numpy())
    _check_files(written, str(tmp_path / "a"), 8000, x8.cpu().numpy(), raw)
    # out_rate = "input": 16 kHz files of ceil(2 T8) samples; the copy of the input is the file's own samples
    raw2, written = infer.separate_file(m, p16, resample=True, out_rate="input", out_prefix=str(tmp_path / "b"))
    assert np.array_equal(raw2, raw)
    up = rs.resample([e for e in want], 8000, 16000)
    assert all(u.shape[0] == 2 * T8 for u in up)
    _check_files(written, str(tmp_path / "b"), 16000, x16, [u.cpu().numpy() for u in up])
    # a number: 48 kHz outputs from the 8 kHz estimates, the copy converted from the file's rate
    _, written = infer.separate_file(m, p16, resample=True, out_rate=48000, out_prefix=str(tmp_path / "c"))
    up = rs.resample([e for e in want], 8000, 48000)
    _check_files(written, str(tmp_path / "c"), 48000, rs.resample(torch.from_numpy(x16), 16000, 48000, device=DEV).cpu().numpy(),
                 [u.cpu().numpy() for u in up])
    # out_rate without resample on a file at the model's rate
    _, written = infer.separate_file(m, SAMPLE, out_rate=16000, out_prefix=str(tmp_path / "d"))
    assert [_read(w)[0] for w in written] == [16000] * 3 and _read(written[1])[1].shape[0] == 2 * infer.load_wav(SAMPLE, 8000).shape[0]


def test_separate_long_file_resamples(tmp_path):
    m = gpu_model()
    x = infer.load_wav(SAMPLE, 8000)
    p16 = str(tmp_path / "long16.wav")
    x16 = _write_16k(p16, np.tile(x, 3)[:160000])                        # 20 s
    x8 = rs.resample(torch.from_numpy(x16), 16000, 8000, device=DEV)
    assert x8.shape[0] == 160000
    want = torch.stack(longform.separate_long(m, x8))
    raw, written = infer.separate_long_file(m, p16, resample=True, out_prefix=str(tmp_path / "a"))
    assert np.array_equal(raw, want.cpu().numpy())
    _check_files(written, str(tmp_path / "a"), 8000, x8.cpu().numpy(), raw)
    raw2, written = infer.separate_long_file(m, p16, resample=True, out_rate="input", out_prefix=str(tmp_path / "b"))
    assert np.array_equal(raw2, raw)
    up = rs.resample([e for e in want], 8000, 16000)
    assert all(u.shape[0] == 320000 for u in up)
    _check_files(written, str(tmp_path / "b"), 16000, x16, [u.cpu().numpy() for u in up])


@pytest.mark.parametrize("long_form", [False, True])
def test_cli_resample(tmp_path, long_form):
    m = gpu_model()
    x = infer.load_wav(SAMPLE, 8000)
    p16 = str(tmp_path / "clip.wav")
    x16 = _write_16k(p16, np.tile(x, 2)[:80000] if long_form else x[:24000])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    extra = ["--chunk-seconds", "4", "--overlap-seconds", "1"] if long_form else []
    base = [sys.executable, "-m", "sepreformer_amd.infer", p16, "--model", "tiny"] + extra
    r = subprocess.run(base, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "sampling rate" in r.stderr              # without --resample the file is refused
    r = subprocess.run(base + ["--resample", "--out-rate", "input"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    written = r.stdout.strip().split("\n")
    x8 = rs.resample(torch.from_numpy(x16), 16000, 8000, device=DEV)
    est = longform.separate_long(m, x8) if long_form else [e[0] for e in infer.separate(m, x8[None])]
    up = rs.resample([e.contiguous() for e in est], 8000, 16000)
    _check_files(written, str(tmp_path / "clip"), 16000, x16, [u.cpu().numpy() for u in up])


@pytest.mark.parametrize("variant", ["tiny", "SepReformer_Base_WSJ0"])
def test_report_round_trip_separation(variant):
    """8 kHz -> 16 kHz -> 8 kHz, then separated, against the direct separation of the 8 kHz file.  Reported, not bounded: the
    band above 0.875 of Nyquist is lost in the round trip, and how much the separator cares is unmeasured."""
    m = gpu_model(variant)
    x = torch.from_numpy(infer.load_wav(SAMPLE, 8000)).to(DEV)
    back = rs.resample(rs.resample(x, 8000, 16000), 16000, 8000)
    assert back.shape == x.shape
    tgp.record("resample.roundtrip_8k_16k_8k.waveform_db", orc.agreement_db(back.cpu(), x.cpu()))
    direct = infer.separate(m, x[None])
    trip = infer.separate(m, back[None])
    db = min(orc.agreement_db(t[0].cpu(), d[0].cpu()) for t, d in zip(trip, direct))
    tgp.record(f"resample.roundtrip_8k_16k_8k.{variant}.separation_db", db)
    print(f"round trip 8k -> 16k -> 8k: waveform {orc.agreement_db(back.cpu(), x.cpu()):.1f} dB, {variant} separation {db:.1f} dB")
    assert all(bool(torch.isfinite(t).all()) for t in trip)
