"""numpy restatement of the dynamic-mixing arithmetic, written from the definitions in include/sepr.h: the
energies, the RMS / norm-factor / gain formulas, and what one batch table means sample by sample.  It shares no code with
sepreformer_amd/datafeed.py or the kernel; the tests compare both with it (bit for bit) and all three with the reference's recorded
outputs (tests/golden/dynmix.npz)."""
import hashlib

import numpy as np


def state_digest(state) -> str:
    """The digest make_dynmix_golden.py stores of ``random.getstate()``."""
    return hashlib.sha256(repr(state).encode()).hexdigest()


def energy(x: np.ndarray):
    """int16: the exact integer sum of squares (int64).  float32: the float64 sum of the exact float64 squares."""
    if x.dtype == np.int16:
        return int(np.sum(x.astype(np.int64) ** 2))
    assert x.dtype == np.float32
    return float(np.sum(x.astype(np.float64) ** 2))


def rms(x: np.ndarray) -> np.float32:
    """float32(sqrt(mean square)) of the sample VALUES (int16 / 32768), formed in float64 from the energy."""
    ss = float(energy(x))
    if x.dtype == np.int16:
        ss /= 32768.0 ** 2
    return np.float32(np.sqrt(ss / x.shape[0]))


def values(x: np.ndarray) -> np.ndarray:
    """The float32 sample values: int16 * 2^-15 (exact) or the float32 samples themselves."""
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x


def term(utts, u, start, norm, gain, n) -> np.ndarray:
    """(x * norm) * gain on n samples from ``start``: two float32 multiplies, each rounded."""
    x = values(utts[int(u)][int(start):int(start) + int(n)])
    assert x.shape[0] == n, "a term leaves its utterance"
    a = (x * np.float32(norm)).astype(np.float32)
    return (a * np.float32(gain)).astype(np.float32)


def mix_batch(utts, n, utt, start, norm, gain, M, S, Tmax):
    """``utts``: the corpus as a list of arrays in storage order; the table arrays are [B, M + S] (mixture terms, then target terms).
    -> (mix [B, Tmax], src [S, B, Tmax]) float32, zero from n[b] on."""
    B = len(n)
    mix = np.zeros((B, Tmax), np.float32)
    src = np.zeros((S, B, Tmax), np.float32)
    for b in range(B):
        nb = int(n[b])
        acc = np.zeros(nb, np.float32)
        for m in range(M):
            acc = (acc + term(utts, utt[b, m], start[b, m], norm[b, m], gain[b, m], nb)).astype(np.float32)
        mix[b, :nb] = acc
        for s in range(S):
            j = M + s
            src[s, b, :nb] = term(utts, utt[b, j], start[b, j], norm[b, j], gain[b, j], nb)
    return mix, src


def agreement_db(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.sum((got - want) ** 2))
    ref = float(np.sum(want ** 2))
    if err == 0.0:
        return float("inf")
    return 10.0 * np.log10(ref / err) if ref > 0 else float("-inf")


def fixture_corpus(g):
    """tests/golden/dynmix.npz -> ({name: int16 array} in the fixture's order, {role: keys in scp order})."""
    names, lens = [str(s) for s in g["corpus.names"]], g["corpus.lengths"]
    off = np.concatenate([[0], np.cumsum(lens)])
    arrays = {nm: g["corpus.data"][off[i]:off[i + 1]] for i, nm in enumerate(names)}
    roles = {str(r): [str(k) for k in g["keys"]] for r in g["roles"]}
    return arrays, roles
