"""numpy restatement of dynamic mixing with speed perturbation, written from the definition in include/sepr.h
(sepr_dynmix_speed_fwd).  It shares no code with sepreformer_amd/datafeed.py or sepreformer_amd/resample.py: the converter's geometry and
taps come from tests/resample_ref.py, the sample values and the plain term from tests/dynmix_ref.py.

A speed is an integer percentage p; the perturbed utterance is the stored one through the converter p -> 100 (L / M = 100 / p in lowest
terms): N = ceil(T L / M) samples,

    y[n] = float32(sum_{j = 0 .. K - 1} tap[(n M) mod L][j] * x[floor(n M / L) - Hh + j]),   x = 0 outside [0, T) of that utterance,

the products exact in float64 and summed SEQUENTIALLY over j in float64 (``acc = acc + tab[:, j] * x[:, j]``), one rounding to float32 -
the device's order, so the two are comparable bit for bit.  A perturbed term is (y[start + t] * norm) * gain, two rounded float32
multiplies; a term at 100 % is dynmix_ref.term.
"""
import functools

import numpy as np

import dynmix_ref as dr
import resample_ref as rr


@functools.lru_cache(maxsize=None)
def converter(p):
    """-> (L, M, K, Hh, taps float64 [L][K]) of speed p (the float32 taps, widened)."""
    L, M, K, Hh, _ = rr.geometry(int(p), 100)
    return L, M, K, Hh, rr.taps(int(p), 100).astype(np.float64)


def perturbed_len(T, p):
    if int(p) == 100:
        return int(T)
    L, M = rr.ratio(int(p), 100)
    return rr.out_len(T, L, M)


def convert(x, p, positions=None):
    """x: the float32 sample values of ONE utterance.  -> float32 y[positions] (all N by default); p = 100 is x as recorded."""
    assert x.dtype == np.float32 and x.ndim == 1
    if int(p) == 100:
        return x if positions is None else x[np.asarray(positions, dtype=np.int64)]
    L, M, K, Hh, tab = converter(p)
    N = perturbed_len(x.shape[0], p)
    n = np.arange(N, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)
    assert n.size == 0 or (n.min() >= 0 and n.max() < N), "an output outside the perturbed utterance"
    xp = np.concatenate([np.zeros(Hh), x.astype(np.float64), np.zeros(K)])      # x[b - Hh + j] = xp[b + j]
    win = np.lib.stride_tricks.sliding_window_view(xp, K)
    nm = n * M                                                                   # int64
    t, w = tab[nm % L], win[nm // L]
    acc = np.zeros(n.shape[0], dtype=np.float64)
    for j in range(K):
        acc = acc + t[:, j] * w[:, j]
    return acc.astype(np.float32)


def term(utts, u, start, norm, gain, n, speed):
    if int(speed) == 100:
        return dr.term(utts, u, start, norm, gain, n)
    y = convert(dr.values(utts[int(u)]), speed, np.arange(int(start), int(start) + int(n), dtype=np.int64))
    a = (y * np.float32(norm)).astype(np.float32)
    return (a * np.float32(gain)).astype(np.float32)


def mix_batch(utts, n, utt, start, norm, gain, speed, M, S, Tmax):
    """dynmix_ref.mix_batch with a speed per term ([B, M + S] percent).  -> (mix [B, Tmax], src [S, B, Tmax]) float32."""
    B = len(n)
    mix = np.zeros((B, Tmax), np.float32)
    src = np.zeros((S, B, Tmax), np.float32)
    for b in range(B):
        nb = int(n[b])
        acc = np.zeros(nb, np.float32)
        done = {}
        for j in range(M + S):
            key = (int(utt[b, j]), int(start[b, j]), np.float32(norm[b, j]).tobytes(), np.float32(gain[b, j]).tobytes(), int(speed[b, j]))
            if key not in done:                                                  # the same term again gives the same samples
                done[key] = term(utts, utt[b, j], start[b, j], norm[b, j], gain[b, j], nb, speed[b, j])
            if j < M:
                acc = (acc + done[key]).astype(np.float32)
            else:
                src[j - M, b, :nb] = done[key]
        mix[b, :nb] = acc
    return mix, src
