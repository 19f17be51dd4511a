"""numpy / plain-Python restatement of the stream bank's schedule, built on tests/longform_ref.py: which
window of a stream runs when, which span of the recording each step emits, and the step-by-step form of the stitch itself.  It shares
no code with sepreformer_amd/streambank.py."""
import numpy as np

import longform_ref as ref


def schedule(pushes, W, O, step_after_push=True):
    """The steps of ONE stream that receives ``pushes`` (a list of sample counts) and is then closed, as a list of
    (kind, k, start, n): kind "window" runs window k and emits [start, start + n), "flush" emits the saved tail with no window,
    "short" is the whole recording through ``separate``.  ``step_after_push``: the bank steps as long as a window is ready after
    every push; otherwise only after the close."""
    H = W - O
    recv, k, ev = 0, 0, []
    for n in pushes:
        recv += n
        while step_after_push and recv >= k * H + W:            # the stream's length is not known yet: never its last window
            ev.append(("window", k, k * H, H))
            k += 1
    T = recv
    if T == 0:
        return ev
    if k == 0 and T <= W:
        return [("short", 0, 0, T)]
    nc = ref.num_chunks(T, W, O)
    if T <= W:                                                  # T == W and window 0 ran before the end was known
        nc = 1
    while k < nc - 1:
        ev.append(("window", k, k * H, H))
        k += 1
    if k == nc - 1:
        ev.append(("window", k, k * H, T - k * H))              # the last window: everything up to T
    else:
        assert k == nc and T - k * H == O                       # the last window ran before the close: its tail is pending
        ev.append(("flush", k, k * H, O))
    return ev


def step_stitch(chunks, T, O, match_gain=False):
    """The stitch of longform_ref taken one window at a time with carried state (tail, P, g): -> the emissions [S, n] of every step,
    in float64.  Their concatenation is ref.stitch(chunks, T, O)[0]."""
    nc, S, W = chunks.shape
    H = W - O
    w_in, w_out = ref.crossfade(O)
    P, g, tail, outs = np.arange(S), np.ones(S), None, []
    for k in range(nc):
        c = np.asarray(chunks[k], np.float64)
        Pold, gold = P.copy(), g.copy()
        if k > 0:
            Cm, Ea, Eb = tail @ c[:, :O].T, np.einsum("it,it->i", tail, tail), np.einsum("jt,jt->j", c[:, :O], c[:, :O])
            pi, ratio = ref.choose(Cm, Ea, Eb, O, match_gain)
            g = np.array([gold[s] * ratio[Pold[s]] for s in range(S)])
            P = np.array([pi[Pold[s]] for s in range(S)])
        n = H if k < nc - 1 else T - k * H
        y = np.stack([g[s] * c[P[s], :n] for s in range(S)])
        if k > 0:
            for s in range(S):
                y[s, :O] = w_in * g[s] * c[P[s], :O] + w_out * gold[s] * tail[Pold[s]]
        outs.append(y)
        tail = c[:, H:]
    return outs
