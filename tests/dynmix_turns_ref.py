"""numpy restatement of dynamic mixing with turn-taking, written from the definition in include/sepr.h
(sepr_dynmix_turns_fwd).  It shares no code with sepreformer_amd: it is the composition of tests/dynmix_ref.py (the sample values and the
plain term), tests/dynmix_speed_ref.py (``convert`` of the WHOLE utterance, through tests/dynmix_speed_reverb_ref.py's cache) and
tests/dynmix_reverb_ref.py (``conv64``), plus one function - the gate.

A term is (utt, start, norm, gain, speed p, rir, taps, on, off); [on, off) is its turn in output samples.  With ramp the float32 table [RL],
ramp[i] = float32(0.5 - 0.5 cos(pi (i + 0.5) / RL)) formed in float64, and for any integer t, d = t - on, e = off - 1 - t:

    w(t) = 0 if d < 0 or e < 0,   ramp[min(d, e)] if min(d, e) < RL,   1 otherwise.

y is the talker's float32 signal - the stored utterance's sample values, or the whole perturbed utterance when p != 100 - and the gate acts on
it at index q = start + t, before any response:

    g[q] = +0.0 where w(q - start) == 0 (selected, never -0.0),   float32(y[q] * w(q - start)) elsewhere.

The term is what the existing restatements make of g in place of y: ``dynmix_ref.term`` without a response, ``conv64`` of g, one rounding and
the two multiplies with one.  The WHOLE of y is gated, so the history a response reaches before the crop is gated by the same w.
"""
import numpy as np

import dynmix_ref as dr
import dynmix_reverb_ref as rr
import dynmix_speed_reverb_ref as srr

FAR = 1 << 30                                                                # (-FAR, FAR): the open turn


def ramp_table(RL):
    i = np.arange(int(RL), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(int(RL), 1))).astype(np.float32)


def weight(t, on, off, ramp):
    """w(t), float32, for an integer array t (int64 arithmetic: no difference overflows for |on|, |off| <= 2^31)."""
    t = np.asarray(t, dtype=np.int64)
    m = np.minimum(t - int(on), int(off) - 1 - t)
    w = np.ones(t.shape, np.float32)
    fade = (m >= 0) & (m < len(ramp))
    w[fade] = np.asarray(ramp, np.float32)[m[fade]]
    w[m < 0] = np.float32(0.0)
    return w


def gated(y, start, on, off, ramp):
    """The whole signal y (float32) under the gate of a term that starts at ``start``."""
    assert y.dtype == np.float32 and y.ndim == 1
    w = weight(np.arange(y.shape[0], dtype=np.int64) - int(start), on, off, ramp)
    g = (y * w).astype(np.float32)
    g[w == 0] = np.float32(0.0)                                              # a selection: +0.0 whatever y holds
    return g


def term(utts, bank, u, start, norm, gain, n, speed, rir, taps, on, off, ramp):
    y = dr.values(utts[int(u)]) if int(speed) == 100 else srr.perturbed(utts, u, speed)
    g = gated(y, start, on, off, ramp)
    if int(rir) < 0:
        return dr.term([g], 0, start, norm, gain, n)
    z = rr.conv64(g, bank[int(rir)], start, n, taps).astype(np.float32)
    a = (z * np.float32(norm)).astype(np.float32)
    return (a * np.float32(gain)).astype(np.float32)


def batch(utts, bank, n, utt, start, norm, gain, speed, rir, taps, on, off, ramp, M, S, Tmax):
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
                   int(rir[b, j]), int(taps[b, j]), int(on[b, j]), int(off[b, j]))
            if key not in done:                                                  # the same term again gives the same samples
                done[key] = term(utts, bank, utt[b, j], start[b, j], norm[b, j], gain[b, j], nb, speed[b, j], rir[b, j], taps[b, j],
                                 on[b, j], off[b, j], ramp)
            if j < M:
                acc = (acc + done[key]).astype(np.float32)
            else:
                src[j - M, b, :nb] = done[key]
        mix[b, :nb] = acc
    return mix, src
