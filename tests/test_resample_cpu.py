"""Sample-rate conversion without a device: resample.plan against the formulas of DESIGN.md section 5d, the float64 restatement
(tests/resample_ref.py) against analytically sampled sines, a direct evaluation and scipy's polyphase filter, the C-ABI argument
checks of the three sepr_resample_* entries, and the file-loading surface of infer.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref                                                   # noqa: E402

from sepreformer_amd import infer                                            # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_WSJ.wav")
RATIOS = [(48000, 8000), (44100, 8000), (16000, 8000), (22050, 8000), (32000, 8000), (8000, 16000), (8000, 44100), (8000, 48000)]
MIN_DB = 110.0      # the specification's own worst figures (120.2 dB agreement, 121.2 dB attenuation) less a 10 dB margin


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_plan_matches_the_formulas(fs_in, fs_out):
    p = rs.plan(fs_in, fs_out)
    g = math.gcd(fs_in, fs_out)
    L, M = fs_out // g, fs_in // g
    s = min(1.0, L / M)
    Hh = math.ceil(64 / s)
    assert (p.L, p.M, p.K, p.Hh) == (L, M, 2 * Hh + 2, Hh) == ref.geometry(fs_in, fs_out)[:4]
    assert p.taps.shape == (L, p.K) and p.taps.dtype == np.float32
    want = np.zeros((L, p.K))
    for ph in range(L):
        for j in range(p.K):
            u = (ph / L + Hh - j) * s
            if abs(u) < 64:
                v = 0.945 * u
                sinc = 1.0 if v == 0 else math.sin(math.pi * v) / (math.pi * v)
                want[ph, j] = 0.945 * s * sinc * float(np.i0(12.0 * math.sqrt(1.0 - (u / 64) ** 2)) / np.i0(12.0))
    assert np.array_equal(p.taps, ref.taps(fs_in, fs_out))
    assert np.abs(p.taps.astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-15
    dc = p.taps.astype(np.float64).sum(axis=1)
    print(f"{fs_in}->{fs_out}: L {L} M {M} K {p.K} DC gain error {np.abs(dc - 1).max():.3g}")
    assert np.abs(dc - 1.0).max() <= 1e-6
    # the kernel's layout: [K][L], column q = the row of phase (q M) mod L
    dev = rs.device_table(p)
    assert dev.shape == (p.K, L) and dev.dtype == np.float32 and dev.flags["C_CONTIGUOUS"]
    for q in {0, 1 % L, L // 2, L - 1}:
        assert np.array_equal(dev[:, q], p.taps[(q * M) % L])


def test_known_table_sizes():
    assert [rs.plan(a, 8000).K for a in (48000, 44100, 22050, 16000)] == [770, 708, 356, 258]
    p = rs.plan(8000, 44100)
    assert (p.K, p.L) == (130, 441) and rs.plan(22050, 8000).L == 160
    with pytest.raises(ValueError):
        rs.plan(0, 8000)


def _sine(fs, f, T, phase=0.3):
    return np.sin(2.0 * np.pi * f * np.arange(T) / fs + phase)


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_restatement_on_sines(fs_in, fs_out):
    T = fs_in // 2                                                       # 0.5 s
    N = ref.out_len(T, *ref.ratio(fs_in, fs_out))
    mid = np.arange(N // 4, 3 * N // 4)                                  # the middle half
    nyq = min(fs_in, fs_out) / 2.0
    for frac in (0.5, 0.8, 0.875):
        f = frac * nyq
        x = _sine(fs_in, f, T).astype(np.float32)
        y = ref.resample(x, fs_in, fs_out, positions=mid)
        want = np.sin(2.0 * np.pi * f * mid / fs_out + 0.3)
        agree = ref.db(y, want)
        print(f"{fs_in}->{fs_out}: agreement at {frac} of the lower Nyquist {agree:.1f} dB")
        assert agree >= MIN_DB, (fs_in, fs_out, frac, agree)
    if fs_out < fs_in:
        for frac in (1.03, 1.5):
            x = _sine(fs_in, frac * nyq, T).astype(np.float32)
            y = ref.resample(x, fs_in, fs_out, positions=mid)
            att = -10.0 * np.log10(np.mean(y * y) / 0.5)
            print(f"{fs_in}->{fs_out}: attenuation at {frac} of the new Nyquist {att:.1f} dB")
            assert att >= MIN_DB, (fs_in, fs_out, frac, att)


def _direct(x, fs_in, fs_out, n):
    """One output by the definition, with explicit zero extension."""
    L, M, K, Hh, _ = ref.geometry(fs_in, fs_out)
    tab = ref.taps(fs_in, fs_out).astype(np.float64)
    b, p = (n * M) // L, (n * M) % L
    acc = 0.0
    for j in range(K):
        i = b - Hh + j
        if 0 <= i < len(x):
            acc += tab[p, j] * float(x[i])
    return acc


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_output_length_and_zero_extension(fs_in, fs_out):
    L, M, K, Hh, _ = ref.geometry(fs_in, fs_out)
    rng = np.random.default_rng(fs_in + fs_out)
    for T in (1, 2, 7, M, M + 1, K - 1, K, 3 * K + 5):
        N = ref.out_len(T, L, M)
        assert N == rs.out_len(T, L, M) == -(-T * L // M) and (N - 1) * M < T * L <= N * M
        x = rng.standard_normal(T).astype(np.float32)
        y = ref.resample(x, fs_in, fs_out)
        assert y.shape == (N,)
        for n in sorted({0, 1 % N, N // 2, N - 1}):                      # both ends read zeros beyond the recording
            d = _direct(x, fs_in, fs_out, n)
            assert abs(y[n] - d) <= 1e-13 * np.abs(x).max(), (T, n)
    # T = 1: the outputs are the taps that meet the one sample
    y = ref.resample(np.array([0.5], dtype=np.float32), fs_in, fs_out)
    tab = ref.taps(fs_in, fs_out).astype(np.float64)
    assert y.shape == (-(-L // M),)
    for n in range(y.shape[0]):
        assert y[n] == 0.5 * tab[(n * M) % L, Hh - (n * M) // L]


@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_cross_check_scipy_polyphase(fs_in, fs_out):
    """scipy.signal.resample_poly fed the same prototype filter (the float32 table laid out at the rate fs_in L) computes the
    same sums by a different route."""
    from scipy.signal import resample_poly
    L, M, K, Hh, _ = ref.geometry(fs_in, fs_out)
    tab = ref.taps(fs_in, fs_out).astype(np.float64)
    Hc = (Hh + 1) * L                                                    # m = p + (Hh - j) L spans [-(Hh + 1) L + 1, Hh L + L - 1]
    h = np.zeros(2 * Hc + 1)
    for p in range(L):
        for j in range(K):
            h[Hc + p + (Hh - j) * L] = tab[p, j] / L                     # resample_poly multiplies the filter by L
    x = np.random.default_rng(5).standard_normal(3 * K + 11).astype(np.float32)
    y = ref.resample(x, fs_in, fs_out)
    got = resample_poly(x.astype(np.float64), L, M, window=h)
    assert got.shape == y.shape
    assert np.abs(got - y).max() <= 1e-12 * np.abs(x).max()


# ---- C ABI: every argument check comes before any HIP call ------------------------------------------------------------
def _call(T=(100,), L=1, M=6, K=770, N=None, R=None, ws_bytes=None, null=None, ioff0=0, ooff0=0):
    lib = L_.load()
    R = len(T) if R is None else R
    N = [int(lib.sepr_resample_out_len(t, L, M)) if L > 0 and M > 0 else 1 for t in T] if N is None else N
    ioff = (C.c_longlong * (len(T) + 1))(ioff0, *[ioff0 + int(v) for v in np.cumsum(T)])
    ooff = (C.c_longlong * (len(N) + 1))(ooff0, *[ooff0 + int(v) for v in np.cumsum(N)])
    if ws_bytes is None:
        ws_bytes = lib.sepr_resample_workspace(R) or 1 << 20
    args = dict(x=4096, ioff=ioff, y=4096, ooff=ooff, taps=4096, ws=4096)        # never dereferenced: every check comes first
    if null:
        args[null] = None
    return lib.sepr_resample_fwd(args["x"], args["ioff"], args["y"], args["ooff"], R, args["taps"], L, M, K, args["ws"], ws_bytes, None)


def test_abi_size_functions():
    lib = L_.load()
    assert lib.sepr_resample_out_len(73600, 2, 1) == 147200 and lib.sepr_resample_out_len(73600, 80, 441) == 13352
    assert lib.sepr_resample_out_len(1, 1, 6) == 1 and lib.sepr_resample_out_len(31752000, 80, 441) == 5760000
    assert lib.sepr_resample_out_len(0, 1, 6) == 0 and lib.sepr_resample_out_len(10, 0, 6) == 0 and lib.sepr_resample_out_len(10, 1, 0) == 0
    assert lib.sepr_resample_out_len(-5, 1, 6) == 0 and lib.sepr_resample_out_len(1 << 62, 441, 80) == 0
    assert lib.sepr_resample_workspace(1) == 512 and lib.sepr_resample_workspace(40) == 1024
    assert lib.sepr_resample_workspace(0) == 0 and lib.sepr_resample_workspace(-1) == 0 and lib.sepr_resample_workspace(65536) == 0


def test_abi_argument_checks():
    E = L_.SEPR_EINVAL
    for name in ("x", "ioff", "y", "ooff", "taps"):
        assert _call(null=name) == E, name
    assert _call(R=0) == E and _call(R=65536) == E
    assert _call(L=0) == E and _call(M=0) == E and _call(L=-1) == E
    assert _call(K=0) == E and _call(K=769) == E                         # K = 2 Hh + 2 is even
    assert _call(T=(0,), N=[1]) == E                                     # empty recording
    assert _call(T=(100,), N=[16]) == E and _call(T=(100,), N=[18]) == E  # 17 outputs expected
    assert _call(T=(100, 50), N=[17, 8]) == E                            # the second needs ceil(50 / 6) = 9
    assert _call(ioff0=1) == E and _call(ooff0=1) == E                   # offsets start at 0
    assert _call(L=1, M=40, K=5122) == E                                 # a tile's span beyond the LDS of one workgroup
    assert _call(ws_bytes=100) == L_.SEPR_EWORKSPACE
    assert _call(null="ws") == L_.SEPR_EWORKSPACE


# ---- Python surface ---------------------------------------------------------------------------------------------------------
def test_equal_rates_are_the_identity_without_a_device():
    x = torch.randn(100)
    assert rs.resample(x, 8000, 8000) is x
    xs = [x, torch.randn(5)]
    assert rs.resample(xs, 16000, 16000) is xs


def test_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # CPU tensors and no device to copy them to
    with pytest.raises(RuntimeError, match="HIP device"):
        rs.resample(torch.randn(100), 16000, 8000)
    with pytest.raises(RuntimeError, match="HIP device"):
        rs.resample([torch.randn(100), torch.randn(7)], 16000, 8000, device="cpu")


def test_input_forms_are_checked():
    with pytest.raises(ValueError):
        rs.resample(torch.randn(2, 100), 16000, 8000)
    with pytest.raises(ValueError):
        rs.resample([torch.randn(1, 100)], 16000, 8000)


def test_load_audio_is_load_wav_without_the_rate_check(tmp_path):
    x, sr = infer.load_audio(SAMPLE)
    assert sr == 8000 and x.dtype == np.float32 and np.array_equal(x, infer.load_wav(SAMPLE, 8000))
    y = ref.resample(x, 8000, 16000)
    p16 = str(tmp_path / "s16.wav")
    infer.write_wav(p16, 0.9 * y / np.abs(y).max(), 16000)
    x16, sr16 = infer.load_audio(p16)
    assert sr16 == 16000 and x16.shape == (2 * x.shape[0],) and x16.dtype == np.float32
    with pytest.raises(RuntimeError, match="sampling rate"):
        infer.load_wav(p16, 8000)


def test_separate_file_still_raises_on_a_rate_mismatch(tmp_path):
    x, _ = infer.load_audio(SAMPLE)
    p16 = str(tmp_path / "s16.wav")
    infer.write_wav(p16, np.repeat(x[:8000], 2), 16000)
    for fn in (infer.separate_file, infer.separate_long_file):
        with pytest.raises(RuntimeError, match="sampling rate"):      # raised by the load, before the model is touched
            fn(None, p16)
        with pytest.raises(RuntimeError, match="sampling rate"):
            fn(None, p16, resample=False, out_rate="input")
