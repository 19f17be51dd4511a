"""Float64 restatement of the sample-rate converter (include/sepr.h sepr_resample_fwd), written from the
definitions and independent of sepreformer_amd/resample.py:

    g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g, s = min(1, L / M), Hh = ceil(Z / s), K = 2 Hh + 2
    tap[p][j] = rolloff s sinc(rolloff u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta),  u = (p / L + Hh - j) s,  0 for |u| >= Z
    y[n] = sum_j tap[(n M) mod L][j] x[floor(n M / L) - Hh + j],  x = 0 outside [0, T),  n < N = ceil(T L / M)

The table is rounded once to float32; the products of float32 taps and float32 samples are exact in float64 and are summed in
float64; ``resample`` returns that float64 sum (the device rounds it once to float32).
"""
from fractions import Fraction
from math import gcd

import numpy as np

Z, ROLLOFF, BETA = 64, 0.945, 12.0


def ratio(fs_in, fs_out):
    g = gcd(int(fs_in), int(fs_out))
    return int(fs_out) // g, int(fs_in) // g


def geometry(fs_in, fs_out):
    """-> (L, M, K, Hh, s)"""
    L, M = ratio(fs_in, fs_out)
    s = min(Fraction(1), Fraction(L, M))
    Hh = int(-(-Fraction(Z) / s // 1))
    return L, M, 2 * Hh + 2, Hh, float(s)


def taps(fs_in, fs_out):
    """float32 [L][K]"""
    L, M, K, Hh, s = geometry(fs_in, fs_out)
    t = np.zeros((L, K), dtype=np.float64)
    for p in range(L):
        u = (p / L + Hh - np.arange(K, dtype=np.float64)) * s
        ok = np.abs(u) < Z
        uu = u[ok]
        t[p, ok] = ROLLOFF * s * np.sinc(ROLLOFF * uu) * np.i0(BETA * np.sqrt(1.0 - (uu / Z) ** 2)) / np.i0(BETA)
    return t.astype(np.float32)


def out_len(T, L, M):
    return -((-int(T) * L) // M)


def resample(x, fs_in, fs_out, positions=None, block=16384):
    """x: 1-D float32 (or values exactly representable in float32).  -> float64 y[positions] (all N outputs by default)."""
    x = np.asarray(x)
    assert x.ndim == 1 and np.array_equal(x.astype(np.float32).astype(np.float64), x.astype(np.float64))
    L, M, K, Hh, _ = geometry(fs_in, fs_out)
    tab = taps(fs_in, fs_out).astype(np.float64)
    T = x.shape[0]
    N = out_len(T, L, M)
    n = np.arange(N, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)
    assert n.size == 0 or (n.min() >= 0 and n.max() < N)
    xp = np.concatenate([np.zeros(Hh), x.astype(np.float64), np.zeros(K)])      # x[b - Hh + j] = xp[b + j]
    win = np.lib.stride_tricks.sliding_window_view(xp, K)
    y = np.empty(n.shape[0], dtype=np.float64)
    for i0 in range(0, n.shape[0], block):
        nn = n[i0:i0 + block]
        nm = nn * M                                                              # int64
        y[i0:i0 + block] = np.einsum("nk,nk->n", tab[nm % L], win[nm // L])
    return y


def db(a, b):
    """10 log10(sum b^2 / sum (a - b)^2)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 10.0 * np.log10(np.sum(b * b) / max(np.sum((a - b) ** 2), 1e-300))
