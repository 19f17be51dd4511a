"""numpy restatement of dynamic mixing with speed perturbation AND reverberation of one source, written from the
definition in include/sepr.h (sepr_dynmix_speed_reverb_fwd).  It shares no code with sepreformer_amd: it is composed from
tests/dynmix_speed_ref.py (``convert`` of the WHOLE utterance) and tests/dynmix_reverb_ref.py (``conv64``).

A term is (utt, start, norm, gain, speed p, rir, taps).  With p != 100 and rir >= 0, x the stored utterance of T samples:

    y     the perturbed utterance, P = ceil(T L / M) samples (L / M = 100 / p in lowest terms), each the float32 sample of the speed form;
    z[t]  = float32(sum_{j = 0 .. taps - 1} double(h[j]) * double(y[start + t - j])),   y ZERO outside [0, P),

the products exact in float64 and added sequentially over j from 0.0, one rounding.  The term is (z[t] * norm) * gain, two rounded float32
multiplies.  p = 100 is dynmix_reverb_ref.term, rir < 0 is dynmix_speed_ref.term, both is dynmix_ref.term.
"""
import numpy as np

import dynmix_ref as dr
import dynmix_reverb_ref as rr
import dynmix_speed_ref as sr

_whole = {}


def perturbed(utts, u, speed):
    """The whole perturbed utterance (float32 [P]), converted once per (utterance, speed)."""
    x = utts[int(u)]
    hit = _whole.get((id(x), int(speed)))
    if hit is None or hit[0] is not x:
        hit = _whole[(id(x), int(speed))] = (x, sr.convert(dr.values(x), int(speed)))
    return hit[1]


def term(utts, bank, u, start, norm, gain, n, speed, rir, taps):
    if int(rir) < 0:
        return sr.term(utts, u, start, norm, gain, n, speed)
    if int(speed) == 100:
        return rr.term(utts, bank, u, start, norm, gain, n, rir, taps)
    z = rr.conv64(perturbed(utts, u, speed), bank[int(rir)], start, n, taps).astype(np.float32)
    a = (z * np.float32(norm)).astype(np.float32)
    return (a * np.float32(gain)).astype(np.float32)


def batch(utts, bank, n, utt, start, norm, gain, speed, rir, taps, M, S, Tmax):
    """-> (mix [B, Tmax], src [S, B, Tmax]) float32; every table array is [B, M + S]."""
    B = len(n)
    mix = np.zeros((B, Tmax), np.float32)
    src = np.zeros((S, B, Tmax), np.float32)
    for b in range(B):
        nb = int(n[b])
        acc = np.zeros(nb, np.float32)
        done = {}
        for j in range(M + S):
            key = (int(utt[b, j]), int(start[b, j]), np.float32(norm[b, j]).tobytes(), np.float32(gain[b, j]).tobytes(), int(speed[b, j]),
                   int(rir[b, j]), int(taps[b, j]))
            if key not in done:                                                  # the same term again gives the same samples
                done[key] = term(utts, bank, utt[b, j], start[b, j], norm[b, j], gain[b, j], nb, speed[b, j], rir[b, j], taps[b, j])
            if j < M:
                acc = (acc + done[key]).astype(np.float32)
            else:
                src[j - M, b, :nb] = done[key]
        mix[b, :nb] = acc
    return mix, src
