"""Restatement of the stream bank's hop-by-hop sample-rate conversion, built on tests/resample_ref.py and
independent of sepreformer_amd/streambank.py.

Output n of a converter L / M with half length Hh reads inputs floor(n M / L) - Hh .. floor(n M / L) + Hh + 1.  While a stream is open,
output n is computed once ``received >= floor(n M / L) + Hh + 2``; once it is closed, T is known and all ceil(T L / M) outputs are
computed with zero extension.  ``ready_brute`` counts them with a loop over n; ``Chunked`` converts a recording push by push and treats
WHAT HAS BEEN RECEIVED as the whole recording - so an output computed too early reads zeros where samples were still to come, and
differs from the whole-recording conversion.
"""
import numpy as np

import resample_ref as rr

PLANS = [(48000, 8000), (16000, 8000), (44100, 8000), (11025, 8000), (8000, 16000), (8000, 44100)]


def ready_brute(received, closed, fs_in, fs_out):
    L, M, K, Hh, _ = rr.geometry(fs_in, fs_out)
    if closed:
        n = 0
        while n * M < received * L:                 # n < T L / M  <=>  n < ceil(T L / M)
            n += 1
        return n
    n = 0
    while (n * M) // L + Hh + 2 <= received:
        n += 1
    return n


def span(fs_in, fs_out):
    """input samples one tile of 256 outputs reads"""
    L, M, K, Hh, _ = rr.geometry(fs_in, fs_out)
    return 255 * M // L + K + 1


class Chunked:
    """One stream: ``push(samples)`` / ``close()`` -> the float64 outputs that became computable, with the span [n0, n1) they cover."""

    def __init__(self, fs_in, fs_out):
        self.fs_in, self.fs_out = fs_in, fs_out
        self.x = np.zeros(0, dtype=np.float32)
        self.done, self.spans = 0, []

    def _advance(self, closed):
        n1 = ready_brute(self.x.shape[0], closed, self.fs_in, self.fs_out)
        n0, self.done = self.done, max(self.done, n1)
        self.spans.append((n0, self.done))
        if self.done == n0:
            return np.zeros(0)
        return rr.resample(self.x, self.fs_in, self.fs_out, positions=np.arange(n0, self.done))

    def push(self, samples):
        self.x = np.concatenate([self.x, np.asarray(samples, dtype=np.float32)])
        return self._advance(False)

    def close(self):
        return self._advance(True)


def schedule(T, seed, small=True):
    """Random push sizes that sum to T, pushes of 0 and 1 samples among them."""
    rng = np.random.default_rng(seed)
    out, left = [], T
    while left > 0:
        c = int(rng.choice([0, 1, int(rng.integers(2, 40)), int(rng.integers(40, 700 if small else 3000))]))
        c = min(c, left)
        out.append(c)
        left -= c
    return out
