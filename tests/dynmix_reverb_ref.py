"""numpy restatement of dynamic mixing with reverberation, written from the definition in include/sepr.h
(sepr_dynmix_reverb_fwd).  It shares no code with sepreformer_amd/datafeed.py, sepreformer_amd/reverb.py or the kernel: the sample
values and the plain term come from tests/dynmix_ref.py.

A reverberant term names an impulse response h (float32) and a tap count; with x the stored utterance's float32 sample values,

    y[t] = float32(sum_{j = 0 .. taps - 1} double(h[j]) * double(x[start + t - j])),   x = 0 outside [0, T) of that utterance,

the products exact in float64 (two 24-bit significands) and added SEQUENTIALLY over j from 0.0 (``acc = acc + h[j] * x[...]``, which is
the device's ``fma(h, x, acc)`` because the product is exact), one rounding to float32.  The term is (y[t] * norm) * gain, two rounded
float32 multiplies; a term with rir < 0 is dynmix_ref.term.
"""
import numpy as np

import dynmix_ref as dr


def conv64(x_values, h, start, n, taps):
    """The float64 sums of outputs start .. start + n - 1 (before the rounding).  x_values: ONE utterance's float32 sample values."""
    assert x_values.dtype == np.float32 and x_values.ndim == 1 and h.dtype == np.float32 and h.ndim == 1
    start, n, taps = int(start), int(n), int(taps)
    assert 1 <= taps <= h.shape[0] and start >= 0 and start + n <= x_values.shape[0], "a term leaves its utterance or its impulse response"
    xpad = np.concatenate([np.zeros(taps - 1), x_values.astype(np.float64)])            # x[i] = xpad[i + taps - 1]
    h64 = h.astype(np.float64)
    acc = np.zeros(n, dtype=np.float64)
    for j in range(taps):
        lo = start - j + taps - 1
        acc = acc + h64[j] * xpad[lo:lo + n]
    return acc


def term(utts, bank, u, start, norm, gain, n, rir, taps):
    """``bank``: the impulse responses as a list of float32 arrays."""
    if int(rir) < 0:
        return dr.term(utts, u, start, norm, gain, n)
    y = conv64(dr.values(utts[int(u)]), bank[int(rir)], start, n, taps).astype(np.float32)
    a = (y * np.float32(norm)).astype(np.float32)
    return (a * np.float32(gain)).astype(np.float32)


def batch(utts, bank, n, utt, start, norm, gain, rir, taps, M, S, Tmax):
    """dynmix_ref.mix_batch with an impulse response and a tap count per term ([B, M + S]).  -> (mix [B, Tmax], src [S, B, Tmax])."""
    B = len(n)
    mix = np.zeros((B, Tmax), np.float32)
    src = np.zeros((S, B, Tmax), np.float32)
    for b in range(B):
        nb = int(n[b])
        acc = np.zeros(nb, np.float32)
        done = {}
        for j in range(M + S):
            key = (int(utt[b, j]), int(start[b, j]), np.float32(norm[b, j]).tobytes(), np.float32(gain[b, j]).tobytes(), int(rir[b, j]),
                   int(taps[b, j]))
            if key not in done:                                                          # the same term again gives the same samples
                done[key] = term(utts, bank, utt[b, j], start[b, j], norm[b, j], gain[b, j], nb, rir[b, j], taps[b, j])
            if j < M:
                acc = (acc + done[key]).astype(np.float32)
            else:
                src[j - M, b, :nb] = done[key]
        mix[b, :nb] = acc
    return mix, src
