"""float64 numpy restatement of long-form separation's stitching (csrc/sepr_stitch.hip), the role
tests/bss_eval_ref.py plays for BSS-eval: geometry, boundary statistics, permutation, gain and overlap-add, written out
directly from the definitions."""
import itertools
import math

import numpy as np

DELTA = 1e-20        # inside the square root of the normalised correlation
SILENCE = 1e-10      # mean square per sample below which a gain is carried
RHO_MIN = 0.5        # normalised correlation below which a gain is carried


def num_chunks(T, W, O):
    """Nc = 1 for T <= W, else 1 + ceil((T - W) / H)."""
    H = W - O
    return 1 if T <= W else 1 + -(-(T - W) // H)


def chunk_offsets(lengths, W, O):
    """CSR offsets [R + 1] of the recordings' windows in the packed chunk buffer."""
    return np.concatenate([[0], np.cumsum([num_chunks(T, W, O) for T in lengths])]).astype(np.int64)


def cut(x, W, O):
    """[Nc, W] windows of a 1-D recording; only the last is zero-padded past T."""
    H, nc = W - O, num_chunks(len(x), W, O)
    xp = np.zeros((nc - 1) * H + W, dtype=x.dtype)
    xp[:len(x)] = x
    return np.stack([xp[k * H:k * H + W] for k in range(nc)])


def crossfade(O):
    """(incoming, outgoing) float64 weights over an overlap: w = sin^2(pi (j + 0.5) / (2 O)), 1 - w."""
    j = np.arange(O, dtype=np.float64)
    w_in = np.sin(math.pi * (j + 0.5) / (2.0 * O)) ** 2
    return w_in, 1.0 - w_in


def crossfade_f32(O):
    """The same weights as the kernel forms them: w = (float) sin^2 in double, 1.0f - w in float32."""
    w_in = crossfade(O)[0].astype(np.float32)
    return w_in, np.float32(1.0) - w_in


def boundary_stats(ck, ck1, O):
    """ck, ck1 [S, W] (window k and k + 1) -> C [S, S], Ea [S], Eb [S] in float64."""
    a = np.asarray(ck, np.float64)[:, -O:]
    b = np.asarray(ck1, np.float64)[:, :O]
    return a @ b.T, np.einsum("it,it->i", a, a), np.einsum("jt,jt->j", b, b)


def choose(C, Ea, Eb, O, match_gain):
    """-> (pi as a tuple, ratio [S]): the lexicographically first maximiser and the per-source gain ratio (1 = carried)."""
    S = len(Ea)
    best, bpi, bratio = None, None, None
    for pi in itertools.permutations(range(S)):
        score, ratio = 0.0, []
        for i in range(S):
            j = pi[i]
            rho = abs(C[i, j]) / math.sqrt(Ea[i] * Eb[j] + DELTA)
            score += rho
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.float64(C[i, j]) / np.float64(Eb[j])
            carry = (not match_gain or Ea[i] / O < SILENCE or Eb[j] / O < SILENCE or rho < RHO_MIN or not np.isfinite(q))
            ratio.append(1.0 if carry else float(q))
        if best is None or score > best:
            best, bpi, bratio = score, pi, ratio
    return bpi, np.array(bratio)


def plan(chunks, O, match_gain=False):
    """chunks [Nc, S, W] of ONE recording -> perm [Nc, S] (P_k(s)) int, gain [Nc, S] float64 (g_k(s))."""
    nc, S, _ = chunks.shape
    perm = np.zeros((nc, S), np.int64)
    gain = np.ones((nc, S))
    perm[0] = np.arange(S)
    for k in range(nc - 1):
        C, Ea, Eb = boundary_stats(chunks[k], chunks[k + 1], O)
        pi, ratio = choose(C, Ea, Eb, O, match_gain)
        for s in range(S):
            i = perm[k, s]
            gain[k + 1, s] = gain[k, s] * ratio[i]
            perm[k + 1, s] = pi[i]
    return perm, gain


def overlap_add(chunks, perm, gain, T, O):
    """y [S, T] = sum_k w_k(t) g_k(s) chunks[k][P_k(s)][t - kH] in float64."""
    nc, S, W = chunks.shape
    H = W - O
    w_in, w_out = crossfade(O)
    y = np.zeros((S, (nc - 1) * H + W))
    for k in range(nc):
        w = np.ones(W)
        if k > 0:
            w[:O] = w_in
        if k < nc - 1:
            w[H:] = w_out
        for s in range(S):
            y[s, k * H:k * H + W] += w * gain[k, s] * np.asarray(chunks[k, perm[k, s]], np.float64)
    return y[:, :T]


def stitch(chunks, T, O, match_gain=False):
    """chunks [Nc, S, W] of one recording of T samples -> (y [S, T], perm, gain)."""
    perm, gain = plan(chunks, O, match_gain)
    return overlap_add(chunks, perm, gain, T, O), perm, gain
