"""Float64 numpy / scipy restatement of STOI and ESTOI (Taal et al. 2011; Jensen & Taal 2016) as DESIGN.md section 5f and
include/sepr.h (sepr_stoi_fwd) define them, written from the definition and independent of sepreformer_amd:

    FS = 10000, frames of 256 at hop 128, w = hanning(258)[1:-1], NFFT 512, 15 one-third-octave bands from 150 Hz,
    segments of N = 30 frames, BETA = -15 dB, dynamic range 40 dB, EPS = 2^-52
    1. rate: fs != FS -> scipy.signal.resample_poly(x, L, M, window=h), L / M = FS / fs reduced, h the Kaiser-windowed sinc of oct_filter
    2. silent frames: e_k = 20 log10(||x[128 k : 128 k + 256] w|| + EPS), k while 128 k <= len - 256; kept iff max(e) - 40 - e_k < 0;
       the kept frames of x (and the frames of y at the same indices) are overlap-added at hop 128
    3. spectra: frames of the compacted signals at 128 m < len - 256 (kept - 1 frames), windowed again, rfft at 512, band value =
       sqrt(sum |X|^2 over bins [lo_b, hi_b))
    4. fewer than 30 spectral frames: 1e-5 ("too short")
    5. segments of 30 frames: STOI = clipped, row-normalised correlation; ESTOI = row- then column-normalised correlation

The transform is np.fft.rfft and the converter scipy's resample_poly - a different formulation from the device's matrix product and
phase table.  ``round_taps`` / ``round_signals`` apply the two float32 roundings the device design makes (the converter's taps, the
10 kHz signals) so that their effect on the values can be measured on the CPU.
"""
from math import ceil, gcd

import numpy as np
from scipy.signal import resample_poly

FS, N_FRAME, HOP, NFFT, NUMBAND, MINFREQ, N, BETA, DYN_RANGE = 10000, 256, 128, 512, 15, 150, 30, -15.0, 40.0
EPS = float(np.finfo(np.float64).eps)
W = np.hanning(N_FRAME + 2)[1:-1]
SHORT = 1e-5


def ratio(fs):
    g = gcd(FS, int(fs))
    return FS // g, int(fs) // g


def oct_filter(L, M):
    """-> (h [2 Lh + 1] of unit sum, Lh)"""
    fc = 1.0 / (2 * max(L, M))
    Lh = int(ceil((60 - 8) / (28.714 * fc / 10)))
    t = np.arange(-Lh, Lh + 1, dtype=np.float64)
    h = np.kaiser(2 * Lh + 1, 0.1102 * (60 - 8.7)) * (2 * L * fc * np.sinc(2 * fc * t))
    return h / np.sum(h), Lh


def to_10k(x, fs, round_taps=False, round_signals=False):
    x = np.asarray(x, dtype=np.float64)
    if int(fs) != FS:
        L, M = ratio(fs)
        h, _ = oct_filter(L, M)
        if round_taps:                                   # the device's table holds float32(L h)
            h = (L * h).astype(np.float32).astype(np.float64) / L
        x = resample_poly(x, L, M, window=h)
    return x.astype(np.float32).astype(np.float64) if round_signals else x


def band_edges():
    grid = np.linspace(0, FS, NFFT + 1)[: NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=np.float64)
    lo = [int(np.argmin(np.square(grid - MINFREQ * 2.0 ** ((2 * b - 1) / 6)))) for b in k]
    hi = [int(np.argmin(np.square(grid - MINFREQ * 2.0 ** ((2 * b + 1) / 6)))) for b in k]
    return lo, hi


def _frames(x, strict):
    stop = len(x) - N_FRAME
    starts = [i for i in range(0, max(stop + 1, 0), HOP) if (i < stop if strict else i <= stop)]
    if not starts:
        return np.zeros((0, N_FRAME))
    return np.stack([x[i:i + N_FRAME] * W for i in starts])


def _ola(frames):
    out = np.zeros((len(frames) - 1) * HOP + N_FRAME)
    for j, f in enumerate(frames):
        out[j * HOP:j * HOP + N_FRAME] += f
    return out


def silent_mask(x):
    """-> (mask [frames] bool, margin = the smallest |max(e) - 40 - e_k| in dB)"""
    fr = _frames(x, strict=False)
    if len(fr) == 0:
        return np.zeros(0, bool), np.inf
    e = 20 * np.log10(np.linalg.norm(fr, axis=1) + EPS)
    d = np.max(e) - DYN_RANGE - e
    return d < 0, float(np.min(np.abs(d)))


def _bands(x):
    lo, hi = band_edges()
    fr = _frames(x, strict=True)
    p = np.abs(np.fft.rfft(fr, n=NFFT, axis=1)) ** 2                              # [frames][257]
    return np.stack([np.sqrt(np.sum(p[:, a:b], axis=1)) for a, b in zip(lo, hi)])  # [15][frames]


def _segments(v):
    return np.lib.stride_tricks.sliding_window_view(v, N, axis=1).transpose(1, 0, 2)   # [segments][15][30]


def _rownorm(a):
    a = a - np.mean(a, axis=2, keepdims=True)
    return a / (np.linalg.norm(a, axis=2, keepdims=True) + EPS)


def _colnorm(a):
    a = a - np.mean(a, axis=1, keepdims=True)
    return a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)


def _measures(xb, yb):
    X, Y = _segments(xb), _segments(yb)
    M = X.shape[0]
    nc = np.linalg.norm(X, axis=2, keepdims=True) / (np.linalg.norm(Y, axis=2, keepdims=True) + EPS)
    Yp = np.minimum(Y * nc, X * (1 + 10 ** (-BETA / 20)))
    d = float(np.sum(_rownorm(X) * _rownorm(Yp)) / (M * NUMBAND))
    de = float(np.sum(_colnorm(_rownorm(X)) * _colnorm(_rownorm(Y)) / N) / M)
    return d, de


def evaluate(x, ys, fs, round_taps=False, round_signals=False):
    """Clean ``x`` against every processed signal of ``ys`` (all of x's length, all sampled at ``fs``): the kept-frame set depends on x
    alone and is shared.  -> dict(stoi [len(ys)], estoi [len(ys)], frames, kept, margin, short)."""
    x = to_10k(x, fs, round_taps, round_signals)
    ys = [to_10k(y, fs, round_taps, round_signals) for y in ys]
    mask, margin = silent_mask(x)
    kept = int(mask.sum())
    out = {"frames": int(mask.size), "kept": kept, "margin": margin, "short": kept - 1 < N,
           "stoi": np.full(len(ys), SHORT), "estoi": np.full(len(ys), SHORT)}
    if out["short"]:
        return out
    xb = _bands(_ola(_frames(x, strict=False)[mask]))
    for j, y in enumerate(ys):
        assert len(y) == len(x)
        out["stoi"][j], out["estoi"][j] = _measures(xb, _bands(_ola(_frames(y, strict=False)[mask])))
    return out


def stoi(x, y, fs, extended=False):
    out = evaluate(x, [y], fs)
    return float(out["estoi" if extended else "stoi"][0])


def pit(values, values_mix):
    """values [S][S] (reference i, estimate j), values_mix [S] -> (perm [S], chosen values [S], improvement [S]), indexed by reference;
    the first maximiser of the mean over itertools.permutations."""
    from itertools import permutations
    S = len(values)
    best, perm = None, None
    for p in permutations(range(S)):
        m = float(np.mean([values[k][p[k]] for k in range(S)]))
        if best is None or m > best:
            best, perm = m, p
    chosen = np.array([values[k][perm[k]] for k in range(S)])
    return list(perm), chosen, chosen - np.asarray(values_mix)
